#!/usr/bin/env python3
"""ps.basis_spmm (prebuilt BasisPlan) against the two routes a user with bases has without it, each given the weights
W = einsum("tb,bkf->tkf", comp, basis) INSIDE the timing: ps.typed_spmm(RelationalPlan, x, W), and the message form of
tools/typed_spmm_bench.py (ps.segment_matmul(index=col_by_type) + ops.scatter).  Plans and the type sort are built
outside the timing on every side.

Shapes: the config-3 pattern (bench.make_workload: 2 M x 2 M, 20 M entries) with uniform random types, T = 16 / 64 /
1024, and R-MAT 21 at T = 16; B = 2 / 8 / 30; K = F = 64 and 128; float32 and bfloat16.  Per case the forward (no_grad)
and a training step (gradients wrt x, basis and comp), the three sides ALTERNATING in the same run, three rounds,
device events around whole calls, medians; the peak device memory of one training step of each side above what is
resident before it; the fused forward's fraction of the larger of its flop model (2 nnz K B on the vector units at
the fp32 FMA peak, 2 M B K F on MFMA) and its byte model over 8 TB/s.

usage: python tools/basis_spmm_bench.py [--quick] [--part 16|64|1024|rmat ...]
(--quick: config-3 at T = 64, B = 8, K = F = 64, one round; --part: only these T of config-3 / R-MAT 21, so that the
matrix can be run in pieces)"""
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import paddle_sparse_amd as ps  # noqa: E402
from bench import event_ms, make_workload, rmat_graph  # noqa: E402
from paddle_sparse_amd import ops  # noqa: E402
from typed_spmm_bench import messages, peak_of  # noqa: E402

dev = torch.device("cuda", 0)
QUICK = "--quick" in sys.argv
PARTS = [sys.argv[i + 1] for i, a in enumerate(sys.argv[:-1]) if a == "--part"] or ["16", "64", "1024", "rmat"]
ROUNDS, REPS = (1, 2) if QUICK else (3, 3)
MFMA = {torch.float32: 157.3e12, torch.bfloat16: 2516e12}
VALU, HBM = 157.3e12, 8e12


def run(name, plan, typed, by_type, B, K, F, dt, gen):
    M, N, T, nnz = plan.M, plan.N, plan.T, plan.nnz
    x = torch.randn(N, K, device=dev, generator=gen).to(dt)
    basis = (torch.randn(B, K, F, device=dev, generator=gen) / K ** 0.5).to(dt)
    comp = torch.randn(T, B, device=dev, generator=gen) / B ** 0.5
    g = torch.randn(M, F, device=dev, generator=gen).to(dt)
    leaves = [t.clone().requires_grad_() for t in (x, basis, comp)]
    expand = lambda v, c: torch.einsum("tb,bkf->tkf", c, v.float()).to(v.dtype)  # noqa: E731
    sides = {"fused": lambda a, v, c: ps.basis_spmm(plan, a, v, c),
             "typed": lambda a, v, c: ps.typed_spmm(typed, a, expand(v, c)),
             "messages": lambda a, v, c: messages(a, expand(v, c), *by_type, M)}

    def step(side):
        for t in leaves:
            t.grad = None
        sides[side](*leaves).backward(g)

    with torch.no_grad():
        a, b = sides["fused"](x, basis, comp).float(), sides["typed"](x, basis, comp).float()
        print(f"== {name}, T = {T}, B = {B}, K = {K}, F = {F}, {str(dt)[6:]}: max |fused - typed| "
              f"{(a - b).abs().max().item():.3e} (largest |value| {b.abs().max().item():.3e})", flush=True)
        del a, b
    step("fused")  # builds plan.t() and the by-type order; not part of the timed steps
    step("typed")
    mem = {side: peak_of(lambda: step(side)) for side in sides}
    work = {(what, side): ((lambda s=side: sides[s](x, basis, comp)) if what == "forward" else (lambda s=side: step(s)))
            for what in ("forward", "training step") for side in sides}
    times = {w: [] for w in work}
    for _ in range(ROUNDS):
        for w, fn in work.items():
            with torch.no_grad() if w[0] == "forward" else torch.enable_grad():
                fn()  # warm-up
                times[w].append(event_ms(fn, REPS))
    es, groups = x.element_size(), -(-B // ops.BASIS_SPMM_G)
    t_flop = 2.0 * nnz * K * B / VALU + 2.0 * M * B * K * F / MFMA[dt]
    nbytes = groups * nnz * (K * es + 12) + (M // 64) * B * K * F * es + M * F * es
    bound = max(t_flop, nbytes / HBM)
    for what in ("forward", "training step"):
        med = {s: statistics.median(times[(what, s)]) for s in sides}
        line = f"     {what:14s}" + "".join(
            f" {s} {med[s]:9.3f} ms [{min(times[(what, s)]):.3f} .. {max(times[(what, s)]):.3f}]  " for s in sides)
        line += "".join(f" x{med['fused'] / med[s]:6.3f} of {s}{' ** the fused op loses **' if med['fused'] > med[s] else ''}"
                        for s in ("typed", "messages"))
        if what == "forward":
            line += (f"   {bound * 1e3 / med['fused']:5.3f} of the {'flop' if t_flop >= nbytes / HBM else 'byte'} bound "
                     f"({t_flop * 1e3:.3f} ms of flops, {nbytes / 1e9:.2f} GB)")
        print(line, flush=True)
    print("     peak memory of one training step above the resident operands: "
          + ", ".join(f"{s} {mem[s]:.3f} GiB" for s in sides), flush=True)


def pattern(name, M, rowptr, col, types, cases, gen):
    adj = ps.SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(M, M), is_sorted=True, trust_data=True)
    row = adj.storage.row()
    for T in types:
        etype = torch.randint(0, T, (col.numel(),), device=dev, generator=gen)
        plan, typed = ps.BasisPlan(adj, etype, T), ps.RelationalPlan(adj, etype, T)
        print(f"-- {name}, T = {T}: nnz = {plan.nnz}, typed_spmm's S / nnz = {typed.segments / plan.nnz:.3f}", flush=True)
        _, perm = ops.index_sort(etype, max_value=T, check=True)  # the entries ordered by type, once
        by_type = (ops.count2ptr(ops.bincount(etype, T)), col[perm].contiguous(), row[perm].contiguous())
        del perm, etype
        for B, K, dt in cases:
            run(name, plan, typed, by_type, B, K, K, dt, gen)
        del plan, typed, by_type


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}; ms per call, medians [range] of {ROUNDS} alternating rounds of "
          f"{REPS} calls; x = fused over the other side (below 1: the fused op is faster)", flush=True)
    gen = torch.Generator(device=dev).manual_seed(0)
    full = [(B, K, dt) for B in (2, 8, 30) for K in (64, 128) for dt in (torch.float32, torch.bfloat16)]
    quick = [(8, 64, torch.float32), (8, 64, torch.bfloat16)]
    types = (64,) if QUICK else tuple(int(p) for p in PARTS if p != "rmat")
    if types:
        M = 2_000_000
        rowptr, col, _ = make_workload(M, M, 20_000_000, 64, 3, dev)
        pattern("config-3 pattern", M, rowptr, col, types, quick if QUICK else full, gen)
        del rowptr, col
    if not QUICK and "rmat" in PARTS:
        N, rowptr, _, col, _ = rmat_graph(21, 20_000_000, dev)
        pattern("R-MAT 21", N, rowptr, col, (16,), full, gen)
