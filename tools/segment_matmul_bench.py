#!/usr/bin/env python3
"""ps.segment_matmul against what a user writes today at the same commit: a Python loop of torch.mm over the T
slices, WITH the host read of ptr that the loop needs, and for the index form x[index] materialised in front of it.

Shapes: R = 2 M rows in T = 4 / 64 / 1024 segments of equal and of Zipf-skewed lengths (length ~ 1 / rank),
K = F = 64 and 128, float32 and bfloat16, forward (no_grad; the op is the public ps.segment_matmul, which allocates
its output and map on every call, the loop writes its slices into one preallocated output) and forward + backward
wrt x and weight (the loop concatenates its slices, autograd does the rest).  The RGCN form:
the config-3 pattern (bench.make_workload: 2 M x 2 M, 20 M entries), T = 16 random edge types, the entries ordered by
type once, index = col by type, K = F = 64.

The two forms are held to each other first and then timed ALTERNATELY, three rounds, device events around whole
calls (the loop's host read included); medians.  Next to the op's forward: its rate on 2 R K F flop and the fraction
of its bound, the larger of flop over the MFMA peak (fp32 157.3 TFLOP/s, bf16 2516 TFLOP/s) and the bytes of x rows
read, out written, the weights and the index over 8 TB/s; the bound that applies is named.

usage: python tools/segment_matmul_bench.py [--quick]   (--quick: T = 64, K = F = 64 and the RGCN form, one round)"""
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import paddle_sparse_amd as ps  # noqa: E402
from bench import event_ms, make_workload  # noqa: E402
from paddle_sparse_amd import ops  # noqa: E402

dev = torch.device("cuda", 0)
QUICK = "--quick" in sys.argv
ROUNDS, REPS = (1, 2) if QUICK else (3, 5)
PEAK = {torch.float32: 157.3e12, torch.bfloat16: 2516e12}
HBM = 8e12


def lengths(R, T, skew):
    if not skew:
        n = torch.full((T,), R // T, dtype=torch.int64)
    else:
        w = 1.0 / torch.arange(1, T + 1, dtype=torch.float64)
        n = (w / w.sum() * R).floor().to(torch.int64)
    n[0] += R - int(n.sum())
    return n


def loop(x, ptr, weight, index=None, out=None):
    """The form without the op.  out: a preallocated [R, F] for the forward; None concatenates (autograd)."""
    rows = x if index is None else x[index]
    p = ptr.tolist()  # the host read the loop cannot do without
    if out is None:
        return torch.cat([rows[p[t]:p[t + 1]] @ weight[t] for t in range(len(p) - 1)])
    for t in range(len(p) - 1):
        torch.mm(rows[p[t]:p[t + 1]], weight[t], out=out[p[t]:p[t + 1]])
    return out


def run(name, x, ptr, weight, index):
    R = x.shape[0] if index is None else index.numel()
    (T, K, F), dt = weight.shape, x.dtype
    out = torch.empty((R, F), dtype=dt, device=dev)
    g = torch.randn(R, F, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).to(dt)
    xg, wg = x.clone().requires_grad_(), weight.clone().requires_grad_()

    def step(form):
        xg.grad = wg.grad = None
        (ps.segment_matmul(xg, ptr, wg, index=index) if form == "op" else loop(xg, ptr, wg, index)).backward(g)

    with torch.no_grad():
        a, b = ps.segment_matmul(x, ptr, weight, index=index), loop(x, ptr, weight, index, out)
        err = (a.float() - b.float()).abs().max().item()
        print(f"== {name}: max |op - loop| forward {err:.3e} (largest |value| {b.float().abs().max().item():.3e})",
              flush=True)
        del a, b
    work = {("forward", "op"): lambda: ps.segment_matmul(x, ptr, weight, index=index),
            ("forward", "loop"): lambda: loop(x, ptr, weight, index, out)}
    step("op")
    gx, gw = xg.grad.float(), wg.grad.float()
    step("loop")
    print(f"     max |op - loop| grad_x {(gx - xg.grad.float()).abs().max().item():.3e}, grad_weight "
          f"{(gw - wg.grad.float()).abs().max().item():.3e} (largest {wg.grad.float().abs().max().item():.3e})",
          flush=True)
    del gx, gw
    work[("forward + backward", "op")] = lambda: step("op")
    work[("forward + backward", "loop")] = lambda: step("loop")
    times = {w: [] for w in work}
    for _ in range(ROUNDS):
        for w, fn in work.items():
            ctx = torch.no_grad() if w[0] == "forward" else torch.enable_grad()
            with ctx:
                fn()  # warm-up: code objects, the GEMM library's choice, the allocator's blocks
                times[w].append(event_ms(fn, REPS))
    flop = 2.0 * R * K * F
    es = x.element_size()
    nbytes = R * (K + F) * es + T * K * F * es + (8 * R if index is not None else 0) + 8 * (T + 1)
    t_flop, t_byte = flop / PEAK[dt], nbytes / HBM
    for what in ("forward", "forward + backward"):
        t_op, t_loop = times[(what, "op")], times[(what, "loop")]
        op, base = statistics.median(t_op), statistics.median(t_loop)
        mult = 1 if what == "forward" else 3
        line = (f"     {what:18s} op {op:9.3f} ms [{min(t_op):.3f} .. {max(t_op):.3f}]   loop {base:9.3f} ms "
                f"[{min(t_loop):.3f} .. {max(t_loop):.3f}]   x{op / base:6.3f}   {mult * flop / op / 1e9:7.2f} TFLOP/s")
        if what == "forward":
            line += (f"   {max(t_flop, t_byte) * 1e3 / op:5.3f} of the {'MFMA' if t_flop >= t_byte else 'HBM'} bound "
                     f"({flop / 1e9:.1f} Gflop, {nbytes / 1e9:.2f} GB)")
        print(line, flush=True)


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}; ms per call, medians [range] of {ROUNDS} alternating rounds of "
          f"{REPS} calls; x = op over loop (below 1: the op is faster)", flush=True)
    gen = torch.Generator(device=dev).manual_seed(0)
    R = 2_000_000
    for K in (64,) if QUICK else (64, 128):
        for dt in (torch.float32, torch.bfloat16):
            x = torch.randn(R, K, device=dev, generator=gen).to(dt)
            for T in (64,) if QUICK else (4, 64, 1024):
                weight = (torch.randn(T, K, K, device=dev, generator=gen) / K ** 0.5).to(dt)
                for skew in (False, True):
                    ptr = ops.count2ptr(lengths(R, T, skew).to(dev))
                    run(f"R = {R}, T = {T} {'Zipf' if skew else 'equal'}, K = F = {K}, {str(dt)[6:]}", x, ptr, weight,
                        None)
            del x
    M, T, K = 2_000_000, 16, 64
    rowptr, col, _ = make_workload(M, M, 20_000_000, 64, 3, dev)
    etype = torch.randint(0, T, (col.numel(),), device=dev, generator=gen)
    _, perm = ops.index_sort(etype, max_value=T, check=True)  # the entries ordered by type, once
    col_by_type, ptr = col[perm].contiguous(), ops.count2ptr(ops.bincount(etype, T))
    del rowptr, col, etype, perm
    for dt in (torch.float32, torch.bfloat16):
        x = torch.randn(M, K, device=dev, generator=gen).to(dt)
        weight = (torch.randn(T, K, K, device=dev, generator=gen) / K ** 0.5).to(dt)
        run(f"RGCN messages, config-3 pattern: {col_by_type.numel()} entries, T = {T}, index = col, K = F = {K}, "
            f"{str(dt)[6:]}", x, ptr, weight, col_by_type)
