#!/usr/bin/env python3
"""Edge-weighted random_walk against the uniform one, on the config-3 shape (2 M x 2 M, 20 M
entries) and R-MAT 24 (bench.rmat_graph(24, 100 M)), with uniform random weights in [0, 1).

Four walks are timed ALTERNATELY on the same inputs, several rounds, so that drift hits all of
them alike:

  uniform           ops.random_walk: psa_random_walk, the entry point the weighted walk is held to
  uniform + e_id    psa_random_walk_weighted with cum = NULL and edge ids: what the edge ids cost
  weighted          psa_random_walk_weighted with the row CDF
  weighted + e_id   the same with edge ids

Workloads: DeepWalk (every node a start, L = 80) and GraphSAINT's roots (20 k roots, L = 2).
Also the construction of the EdgeCDF (the psa_row_cdf launch alone, and EdgeCDF(adj) with its
.double() pass and host read), next to the longest row, whose serial chain is the launch's
critical path.  HIP-event means after a warm-up call.

Byte model of a weighted step: the uniform step's 24 B (the rowptr pair, one col
entry) plus 8 B for the row's total and 8 B per search step, ceil(log2(deg + 1)) of them, every one
a dependent load; 8 B written, 16 B with edge ids.  `depth` below is the mean number of search steps
over the steps of a sample of the walks.

usage: python tools/weighted_walk_bench.py [--quick]   (--quick: config 3 only)"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bench import event_ms, rmat_graph  # noqa: E402
import paddle_sparse_amd as psa  # noqa: E402
from paddle_sparse_amd import SparseTensor, ops  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS = 3


def config3():
    M = 2_000_000
    g = torch.Generator(device=dev).manual_seed(3)
    keys = torch.sort(torch.randint(0, M, (20_000_000,), generator=g, device=dev) * M
                      + torch.randint(0, M, (20_000_000,), generator=g, device=dev))[0]
    row, col = keys // M, keys % M
    del keys
    return M, ops.ind2ptr(row, M), col


def rmat24():
    N, rowptr, row, col, _ = rmat_graph(24, 100_000_000, dev)
    del row
    return N, rowptr, col


def alternate(label, S, L, rowptr, col, cum, start, seed, reps):
    fns = {
        "uniform": lambda: ops.random_walk(rowptr, col, start, L, seed),
        "uniform + e_id": lambda: ops.random_walk_weighted(rowptr, col, None, start, L, seed, True),
        "weighted": lambda: ops.random_walk_weighted(rowptr, col, cum, start, L, seed),
        "weighted + e_id": lambda: ops.random_walk_weighted(rowptr, col, cum, start, L, seed, True),
    }
    times = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            fn()  # warm-up: the allocator has the output's block afterwards
            times[k].append(event_ms(fn, reps))
    print(f"   {label} (ms, {ROUNDS} alternating rounds; ratio = mean over mean of uniform):", flush=True)
    base = sum(times["uniform"]) / ROUNDS
    for k, ts in times.items():
        mean = sum(ts) / ROUNDS
        print(f"     {k:16s} " + " ".join(f"{t:9.3f}" for t in ts) + f"   mean {mean:9.3f}   x{mean / base:5.2f}   "
              f"{S * L / mean / 1e6:7.2f} G steps/s", flush=True)


def run(name, make):
    N, rowptr, col = make()
    nnz = col.numel()
    value = torch.rand(nnz, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    a = SparseTensor(rowptr=rowptr, col=col, value=value, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    deg = rowptr[1:] - rowptr[:-1]
    longest = int(deg.max())
    print(f"== {name}: {N} nodes, {nnz} entries, {int((deg == 0).sum())} without entries, longest row {longest}",
          flush=True)
    seed = 20261020
    with torch.no_grad():
        w64 = value.double()
        ops.row_cdf(rowptr, w64)
        t_launch = event_ms(lambda: ops.row_cdf(rowptr, w64), 5)
        psa.EdgeCDF(a)
        t_obj = event_ms(lambda: psa.EdgeCDF(a), 5)
        del w64
        print(f"   EdgeCDF: psa_row_cdf {t_launch:.3f} ms ({16 * nnz / t_launch / 1e9:.2f} TB/s of 16 B per entry), "
              f"EdgeCDF(adj) {t_obj:.3f} ms; longest row {longest} entries = {-(-longest // 64)} chained 64-entry "
              f"chunks", flush=True)
        cdf = psa.EdgeCDF(a)
        # what the weighted walk does: same nodes with and without edge ids, entries of positive weight
        start = torch.arange(N, device=dev)
        probe = start[:: max(N // 200_000, 1)]
        nodes, e_id = psa.random_walk(a, probe, 80, seed=seed, weighted=cdf, return_edge_ids=True)
        assert torch.equal(nodes, psa.random_walk(a, probe, 80, seed=seed, weighted=cdf))
        moved = e_id >= 0
        assert torch.equal(col[e_id[moved]], nodes[:, 1:][moved]) and bool((value[e_id[moved]] > 0).all())
        d = deg[nodes[:, :-1]].double()
        depth = float(torch.ceil(torch.log2(d + 1)).mean())
        print(f"   weighted walks of {probe.numel()} sampled starts, L = 80: edge ids consistent; mean degree met "
              f"{float(d.mean()):.1f}, depth {depth:.2f} search steps -> {24 + 8 + 8 * depth:.0f} B read per weighted "
              f"step against 24 B", flush=True)
        del nodes, e_id, moved, d
        alternate(f"DeepWalk: all {N} nodes, L = 80", N, 80, rowptr, col, cdf.cum, start, seed, 2)
        roots = torch.randint(0, N, (20_000,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        alternate("GraphSAINT roots: 20 k roots, L = 2", 20_000, 2, rowptr, col, cdf.cum, roots, seed, 50)
    del a, rowptr, col, value, cdf
    torch.cuda.empty_cache()


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}", flush=True)
    run("config-3 shape", config3)
    if "--quick" not in sys.argv:
        run("R-MAT 24", rmat24)
