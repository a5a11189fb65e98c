#!/usr/bin/env python3
"""Weighted against uniform neighbor_sample on the config-3 shape (2 M x 2 M,
20 M entries) and R-MAT 24 (bench.rmat_graph(24, 100 M)), the batches of tools/neighbor_bench.py:
1024 seeds x [15, 10, 5] and [25, 10]; 8192 seeds x [10, 10].  Without replacement.

Two weightings: "random" = float64 weights uniform in [0, 1); "dominated" = every row holds
one weight of 1e18 among ones (what a rejection sampler cannot do in bounded tries), as the
row's LAST entry: float64 prefix sums absorb a 1 added to 1e18, so entries behind the heavy
one would weigh nothing in the row CDF and the rows would make fewer picks than the uniform ones.

Both contenders are NeighborSamplers kept between calls (the relabel map stays clean), one with
weighted=EdgeCDF, one without; the EdgeCDF is built once outside the timing and its build time
is printed.  HIP-event time of a whole call (its host reads, sort and gathers included), REPEATS
alternating rounds of CALLS calls each after a warm-up round; min / median / max over the rounds
and the ratio of the medians.  The weighted sample is checked first: every entry at most once,
none of weight zero, bit-equal on a second call.

usage: python tools/weighted_neighbor_bench.py [--quick | --trace]   (--quick: config 3 only; --trace: 53 calls
each of the uniform and of the weighted sampler at 1024 seeds x [25, 10] on R-MAT 24, random weights, the batch
with the largest ratio, for a kernel trace)"""
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bench import event_ms  # noqa: E402
from neighbor_bench import BATCHES, config3, rmat24, spread  # noqa: E402
import paddle_sparse_amd as psa  # noqa: E402
from paddle_sparse_amd import SparseTensor  # noqa: E402

dev = torch.device("cuda", 0)
REPEATS, CALLS = 3, 10


def weights(kind, rowptr, nnz):
    g = torch.Generator(device=dev).manual_seed(7)
    if kind == "random":
        return torch.rand(nnz, dtype=torch.float64, device=dev, generator=g)
    w = torch.ones(nnz, dtype=torch.float64, device=dev)
    deg = rowptr[1:] - rowptr[:-1]
    rows = torch.nonzero(deg > 0).flatten()
    w[rowptr[rows + 1] - 1] = 1e18
    return w


def run(name, make):
    N, rowptr, col = make()
    deg = rowptr[1:] - rowptr[:-1]
    print(f"== {name}: {N} nodes, {col.numel()} entries, longest row {int(deg.max())}", flush=True)
    print(f"   ms per call, min / median / max of {REPEATS} alternating rounds of {CALLS} calls", flush=True)
    del deg
    seed = 20261021
    uniform_adj = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    with torch.no_grad():
        for kind in ("random", "dominated"):
            w = weights(kind, rowptr, col.numel())
            adj = SparseTensor(rowptr=rowptr, col=col, value=w, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
            cdf = psa.EdgeCDF(adj)
            print(f"   -- {kind} weights; EdgeCDF built in {event_ms(lambda: psa.EdgeCDF(adj), 3):.3f} ms", flush=True)
            for S, fanouts in BATCHES:
                seeds = torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(S))[:S]
                weighted = psa.NeighborSampler(adj, fanouts, weighted=cdf)
                uniform = psa.NeighborSampler(uniform_adj, fanouts)
                a, b, u = weighted(seeds, seed=seed), weighted(seeds, seed=seed), uniform(seeds, seed=seed)
                assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3]
                assert torch.unique(a[2]).numel() == a[2].numel() and bool((w[a[2]] > 0).all())
                if kind == "dominated":  # every expanded row that has entries took its heavy one
                    expanded = a[1][:sum(a[3][0][:-1])]
                    assert int((w[a[2]] == 1e18).sum()) == int(((rowptr[expanded + 1] - rowptr[expanded]) > 0).sum())
                fns = {"uniform": lambda: uniform(seeds, seed=seed), "weighted": lambda: weighted(seeds, seed=seed)}
                res = {k: [] for k in fns}
                for rnd in range(REPEATS + 1):
                    for k, fn in fns.items():
                        t = event_ms(fn, CALLS)
                        if rnd > 0:  # round 0 warms the allocator
                            res[k].append(t)
                med = {k: statistics.median(v) for k, v in res.items()}
                print(f"   {S} seeds x {fanouts}: weighted n = {a[1].numel()} nodes, E = {a[2].numel()} entries; "
                      f"uniform n = {u[1].numel()}, E = {u[2].numel()}", flush=True)
                for k in fns:
                    rel = "" if k == "uniform" else f"   weighted / uniform = x{med['weighted'] / med['uniform']:5.2f}"
                    print(f"     {k:9s} {spread(res[k])}{rel}", flush=True)
                del weighted, uniform, a, b, u
            del adj, cdf, w
    del uniform_adj, rowptr, col
    torch.cuda.empty_cache()


def trace():
    N, rowptr, col = rmat24()
    w = weights("random", rowptr, col.numel())
    adj = SparseTensor(rowptr=rowptr, col=col, value=w, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    S, fanouts = BATCHES[1]
    seeds = torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(S))[:S]
    with torch.no_grad():
        for name, sampler in (("uniform", psa.NeighborSampler(adj, fanouts)),
                              ("weighted", psa.NeighborSampler(adj, fanouts, weighted=psa.EdgeCDF(adj)))):
            for _ in range(53):
                sampler(seeds, seed=1)
            torch.cuda.synchronize()
            print(f"   53 calls of the {name} sampler, {S} seeds x {fanouts}, R-MAT 24", flush=True)


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}", flush=True)
    if "--trace" in sys.argv:
        trace()
        sys.exit(0)
    run("config-3 shape", config3)
    if "--quick" not in sys.argv:
        run("R-MAT 24", rmat24)
