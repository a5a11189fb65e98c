#!/usr/bin/env python3
"""adj.spmm_multi against the calls a user writes today, at the same commit: one adj.matmul(x, r) per
reduction, and for var / std `x * x`, a second mean and the difference in torch ops, concatenated.

Shapes: the config-3 shape (2 M x 2 M, 20 M entries, bench.make_workload) at K = 64 and 128, and R-MAT 21
(bench.rmat_graph(21, 20 M): 19.5 M entries, power-law) at K = 128, with the matrices' values.  Sets:
("mean", "min", "max", "std") and ("sum", "max").  Forward (no_grad) and forward + backward wrt x (one fixed
random upstream gradient; the matrix with squared values the separate form needs is built once, outside the
timing; the separate form computes the mean once and reuses it for var / std: 4 SpMMs for the first set).  Both
forms are held to each other first, then timed ALTERNATELY, several rounds, device events; per form the median and the range of the rounds and the peak memory of one step
above what was allocated before it.

Byte model of the fused forward: one gather, nnz * (12 + 4 K) bytes, the pointers, and
A * M * K * 4 bytes of output; the fraction of 8 TB/s is printed next to the fused forward.

usage: python tools/multi_aggr_bench.py [--quick]   (--quick: config 3 at K = 64 only, one round)"""
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from bench import event_ms, make_workload, rmat_graph  # noqa: E402
from paddle_sparse_amd import SparseTensor  # noqa: E402

dev = torch.device("cuda", 0)
QUICK = "--quick" in sys.argv
ROUNDS, REPS = (1, 3) if QUICK else (3, 10)
EPS = 1e-5
SETS = (("mean", "min", "max", "std"), ("sum", "max"))


def separate(adj, adj_sq, x, reduce):
    """What a user writes without the op: [M, A, K] from one SpMM per reduction, plus `x * x` and a second mean for the
    moments (adj_sq: the same matrix with squared values, built once outside the timed region)."""
    parts = []
    mean = adj.matmul(x, "mean") if any(r in ("mean", "var", "std") for r in reduce) else None  # computed once, reused
    for r in reduce:
        if r == "mean":
            parts.append(mean)
        elif r in ("var", "std"):
            var = (adj_sq.matmul(x * x, "mean") - mean * mean).clamp(min=0)
            # an empty group is 0 in every statistic, std included
            parts.append(var if r == "var" else (var + EPS).sqrt() * (adj.storage.rowcount() > 0).unsqueeze(1))
        else:
            parts.append(adj.matmul(x, r))
    return torch.stack(parts, dim=1)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 2**30


def run(name, M, rowptr, col, value, K):
    nnz = col.numel()
    adj = SparseTensor(rowptr=rowptr, col=col, value=value, sparse_sizes=(M, M), is_sorted=True, trust_data=True)
    adj_sq = SparseTensor(rowptr=rowptr, col=col, value=value * value, sparse_sizes=(M, M), is_sorted=True, trust_data=True)
    x = torch.randn(M, K, device=dev, generator=torch.Generator(device=dev).manual_seed(K))
    xg = x.clone().requires_grad_()
    print(f"== {name}, K = {K}: {M} rows, {nnz} entries, longest row {adj.storage._longest_row()}", flush=True)
    for reduce in SETS:
        A = len(reduce)
        g = torch.randn(M, A, K, device=dev, generator=torch.Generator(device=dev).manual_seed(1))

        def step(form, xg=xg, reduce=reduce, g=g):
            xg.grad = None
            (adj.spmm_multi(xg, reduce, EPS) if form == "fused" else separate(adj, adj_sq, xg, reduce)).backward(g)

        with torch.no_grad():
            a, b = adj.spmm_multi(x, reduce, EPS), separate(adj, adj_sq, x, reduce)
            scale = b.abs().max().item()
            print(f"   {reduce}: forward max |fused - separate| = {(a - b).abs().max().item():.3e} (largest |value| {scale:.3e})", flush=True)
            del a, b
        step("fused")
        ga = xg.grad.clone()
        step("separate")
        print(f"   {reduce}: grad_x max |fused - separate| = {(ga - xg.grad).abs().max().item():.3e} "
              f"(largest |value| {xg.grad.abs().max().item():.3e})", flush=True)
        del ga
        work = {}
        for form in ("fused", "separate"):
            fw = (lambda: adj.spmm_multi(x, reduce, EPS)) if form == "fused" else (lambda: separate(adj, adj_sq, x, reduce))

            def fw_ng(fw=fw):
                with torch.no_grad():
                    fw()

            work[("forward", form)] = fw_ng
            work[("forward + backward", form)] = lambda form=form: step(form)
        times = {w: [] for w in work}
        for _ in range(ROUNDS):
            for w, fn in work.items():
                fn()  # warm-up: the allocator has the blocks afterwards
                times[w].append(event_ms(fn, REPS))
        nbytes = nnz * (12 + 4 * K) + 8 * (M + 1) + A * M * K * 4
        for what in ("forward", "forward + backward"):
            base = statistics.median(times[(what, "separate")])
            for form in ("fused", "separate"):
                ts = times[(what, form)]
                med = statistics.median(ts)
                model = f"   {nbytes / 1e9:.2f} GB = {nbytes / med / 1e9 / 8:.3f} of 8 TB/s" if (what, form) == ("forward", "fused") else ""
                print(f"     {what:18s} {form:8s} median {med:8.3f} ms   range {min(ts):8.3f} .. {max(ts):8.3f}   x{med / base:5.3f}"
                      f"   peak {peak_of(work[(what, form)]):6.2f} GiB{model}", flush=True)
        del g, work
    del adj, adj_sq, x, xg
    torch.cuda.empty_cache()


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}; ms per call over {ROUNDS} alternating rounds of {REPS} calls; "
          f"ratio = median over the median of the separate calls", flush=True)
    M = 2_000_000
    rowptr, col, val = make_workload(M, M, 20_000_000, 64, 3, dev)
    for K in (64,) if QUICK else (64, 128):
        run("config-3 shape", M, rowptr, col, val, K)
    del rowptr, col, val
    if not QUICK:
        N, rowptr, _, col, val = rmat_graph(21, 20_000_000, dev)
        run("R-MAT 21", N, rowptr, col, val, 128)
