#!/usr/bin/env python3
"""ps.typed_spmm (prebuilt RelationalPlan) against the route a user writes without it: the entries ordered by type,
msg = ps.segment_matmul(x, ptr, W, index=col_by_type) and ops.scatter(msg, row_by_type, M, "sum") (float atomics;
bfloat16 messages are widened for it, scatter takes no bfloat16; ops.scatter is a raw op, so the route carries the
three-line autograd Function a user has to add: the gradient of a row sum is a row gather).  The type sort and the plan are built outside the
timing on both sides; the plan's build time is reported by itself.

Shapes: the config-3 pattern (bench.make_workload: 2 M x 2 M, 20 M entries) with uniform random types,
T = 4 / 16 / 64 / 1024, K = F = 64 and 128, float32 and bfloat16; R-MAT 21 (bench.rmat_graph(21, 20 M)) at T = 16.
Per case: S / nnz (S = plan.segments), the forward (no_grad) and forward + backward wrt x and weight, both sides
ALTERNATING in the same run, three rounds, device events around whole calls, medians; the peak device memory of one
training step of each side above what is resident before it; the fused forward's rate on its own flop count
2 (nnz K + 64 S K F) and its fraction of the larger of that over the MFMA peak and the algorithmic bytes over 8 TB/s.

usage: python tools/typed_spmm_bench.py [--quick]   (--quick: T = 16, K = F = 64, fp32, one round)"""
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import paddle_sparse_amd as ps  # noqa: E402
from bench import event_ms, make_workload, rmat_graph  # noqa: E402
from paddle_sparse_amd import ops  # noqa: E402

dev = torch.device("cuda", 0)
QUICK = "--quick" in sys.argv
ROUNDS, REPS = (1, 2) if QUICK else (3, 3)
PEAK = {torch.float32: 157.3e12, torch.bfloat16: 2516e12}
HBM = 8e12


class ScatterRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, msg, index, M):
        ctx.save_for_backward(index)
        return ops.scatter(msg, index, M, "sum")

    @staticmethod
    def backward(ctx, grad):
        return grad[ctx.saved_tensors[0]], None, None


def messages(x, weight, ptr, col_by_type, row_by_type, M):
    msg = ps.segment_matmul(x, ptr, weight, index=col_by_type)
    return ScatterRows.apply(msg.float(), row_by_type, M).to(x.dtype)


def peak_of(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**30


def run(name, plan, sorted_by_type, K, F, dt, gen):
    ptr, col_by_type, row_by_type = sorted_by_type
    M, N, T, nnz, S = plan.M, plan.N, plan.T, plan.nnz, plan.segments
    x = torch.randn(N, K, device=dev, generator=gen).to(dt)
    weight = (torch.randn(T, K, F, device=dev, generator=gen) / K ** 0.5).to(dt)
    g = torch.randn(M, F, device=dev, generator=gen).to(dt)
    xg, wg = x.clone().requires_grad_(), weight.clone().requires_grad_()
    sides = {"fused": lambda a, w: ps.typed_spmm(plan, a, w),
             "messages": lambda a, w: messages(a, w, ptr, col_by_type, row_by_type, M)}

    def step(side):
        xg.grad = wg.grad = None
        sides[side](xg, wg).backward(g)

    with torch.no_grad():
        a, b = sides["fused"](x, weight).float(), sides["messages"](x, weight).float()
        print(f"== {name}, T = {T}, K = {K}, F = {F}, {str(dt)[6:]}: S / nnz = {S / nnz:.3f}; max |fused - messages| "
              f"{(a - b).abs().max().item():.3e} (largest |value| {b.abs().max().item():.3e})", flush=True)
        del a, b
    step("fused")
    plan.t()  # built by the first backward; not part of the timed steps
    mem = {side: peak_of(lambda: step(side)) for side in sides}
    work = {(what, side): ((lambda s=side: sides[s](x, weight)) if what == "forward" else (lambda s=side: step(s)))
            for what in ("forward", "forward + backward") for side in sides}
    times = {w: [] for w in work}
    for _ in range(ROUNDS):
        for w, fn in work.items():
            with torch.no_grad() if w[0] == "forward" else torch.enable_grad():
                fn()  # warm-up
                times[w].append(event_ms(fn, REPS))
    flop = 2.0 * (nnz * K + 64.0 * S * K * F)
    es = x.element_size()
    nbytes = nnz * (K * es + 4 + 1) + S * (12 + K * F * es) + M * F * es
    bound = max(flop / PEAK[dt], nbytes / HBM)
    for what in ("forward", "forward + backward"):
        tf, tm = times[(what, "fused")], times[(what, "messages")]
        f, m = statistics.median(tf), statistics.median(tm)
        line = (f"     {what:18s} fused {f:9.3f} ms [{min(tf):.3f} .. {max(tf):.3f}]   messages {m:9.3f} ms "
                f"[{min(tm):.3f} .. {max(tm):.3f}]   x{f / m:6.3f}{'  ** the fused op loses **' if f > m else ''}")
        if what == "forward":
            line += (f"   {flop / f / 1e9:7.2f} TFLOP/s on {flop / 1e9:.1f} Gflop ({flop / (2.0 * nnz * K * F):.2f}x the "
                     f"message form's), {bound * 1e3 / f:5.3f} of the "
                     f"{'MFMA' if flop / PEAK[dt] >= nbytes / HBM else 'HBM'} bound ({nbytes / 1e9:.2f} GB)")
        print(line, flush=True)
    print(f"     peak memory of one training step above the resident operands: fused {mem['fused']:.3f} GiB, messages "
          f"{mem['messages']:.3f} GiB (an [nnz, F] tensor of this dtype is {nnz * F * es / 2**30:.3f} GiB)", flush=True)


def pattern(name, M, rowptr, col, types, shapes, gen):
    adj = ps.SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(M, M), is_sorted=True, trust_data=True)
    row = adj.storage.row()
    for T in types:
        etype = torch.randint(0, T, (col.numel(),), device=dev, generator=gen)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan = ps.RelationalPlan(adj, etype, T)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        plan.t()
        torch.cuda.synchronize()
        print(f"-- {name}, T = {T}: plan built in {(t1 - t0) * 1e3:.1f} ms, its transpose in "
              f"{(time.perf_counter() - t1) * 1e3:.1f} ms (host clock, first build of this process included); "
              f"S = {plan.segments}, nnz = {plan.nnz}", flush=True)
        _, perm = ops.index_sort(etype, max_value=T, check=True)  # the entries ordered by type, once
        by_type = (ops.count2ptr(ops.bincount(etype, T)), col[perm].contiguous(), row[perm].contiguous())
        del perm, etype
        for K, dt in shapes:
            run(name, plan, by_type, K, K, dt, gen)
        del plan, by_type


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}; ms per call, medians [range] of {ROUNDS} alternating rounds of "
          f"{REPS} calls; x = fused over messages (below 1: the fused op is faster)", flush=True)
    gen = torch.Generator(device=dev).manual_seed(0)
    full = [(K, dt) for K in (64, 128) for dt in (torch.float32, torch.bfloat16)]
    M = 2_000_000
    rowptr, col, _ = make_workload(M, M, 20_000_000, 64, 3, dev)
    pattern("config-3 pattern", M, rowptr, col, (16,) if QUICK else (4, 16, 64, 1024),
            [(64, torch.float32)] if QUICK else full, gen)
    del rowptr, col
    if not QUICK:
        N, rowptr, _, col, _ = rmat_graph(21, 20_000_000, dev)
        pattern("R-MAT 21", N, rowptr, col, (16,), full, gen)
