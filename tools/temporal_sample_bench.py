#!/usr/bin/env python3
"""temporal_neighbor_sample and EdgeTimeOrder on the config-3 shape (2 M x 2 M, 20 M entries)
and R-MAT 24 (bench.rmat_graph(24, 100 M)), each next to the nearest op that was there before.

  build    EdgeTimeOrder(adj, edge_time=t), random int64 times in [0, 2^40): two stable sorts, two
           gathers, three host reads
  sort     one index_sort of nnz keys on the same matrix (the row of every entry, bounded by N):
           what one of the two sorts of the build costs
  sample   adj.temporal_neighbor_sample(seeds, seed_time, fanouts, time=order): seed_time random
           over the times' range, so about half of every row is eligible on average
  ego      adj.ego_k_hop_sample(seeds, fanouts) on the same seeds: the same walk list without the
           time bound, and the INDUCED entries where the sample returns the sampled ones

Batches: 1 024 and 16 384 seeds x [10, 5] and [15, 10, 5], "uniform" without replacement.  HIP-event
time of a whole call (host reads included), REPEATS alternating rounds after a warm-up round, CALLS
calls per round; min / median / max over the rounds, and the ratios of the medians.  No ratio is a
pass mark.

usage: python tools/temporal_sample_bench.py [--quick | --trace]   (--quick: config 3 only; --trace:
23 calls of the sample at 1 024 seeds x [10, 5] on config 3, the batch where it is behind the ego op,
for a kernel trace in a run of its own)"""
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bench import event_ms  # noqa: E402
from neighbor_bench import config3, rmat24, spread  # noqa: E402
from paddle_sparse_amd import EdgeTimeOrder, SparseTensor, ops  # noqa: E402

dev = torch.device("cuda", 0)
BATCHES = ((1024, [10, 5]), (1024, [15, 10, 5]), (16384, [10, 5]), (16384, [15, 10, 5]))
REPEATS, CALLS = 5, 5
T_MAX = 2**40


def alternate(fns):
    """{name: [ms per call]} over REPEATS rounds that run every fn in turn; round 0 warms up."""
    res = {k: [] for k in fns}
    for rnd in range(REPEATS + 1):
        for k, (fn, calls) in fns.items():
            t = event_ms(fn, calls)
            if rnd > 0:
                res[k].append(t)
    return res


def setup(make):
    N, rowptr, col = make()
    adj = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    g = torch.Generator(device=dev).manual_seed(16)
    edge_time = torch.randint(0, T_MAX, (col.numel(),), generator=g, device=dev)
    return N, rowptr, col, adj, edge_time, g


def run(name, make):
    N, rowptr, col, adj, edge_time, g = setup(make)
    deg = rowptr[1:] - rowptr[:-1]
    print(f"== {name}: {N} nodes, {col.numel()} entries, longest row {int(deg.max())}", flush=True)
    print(f"   ms per call, min / median / max of {REPEATS} alternating rounds", flush=True)
    rows = ops.ptr2ind(rowptr, col.numel())
    with torch.no_grad():
        res = alternate({"build": (lambda: EdgeTimeOrder(adj, edge_time=edge_time), 1),
                         "sort": (lambda: ops.index_sort(rows, N, check=True), 1)})
        med = {k: statistics.median(v) for k, v in res.items()}
        print(f"   EdgeTimeOrder build  {spread(res['build'])}", flush=True)
        print(f"   one index_sort       {spread(res['sort'])}   build / sort = x{med['build'] / med['sort']:.2f}", flush=True)
        del rows
        order = EdgeTimeOrder(adj, edge_time=edge_time)
        seed = 20261021
        for S, fanouts in BATCHES:
            seeds = torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(S))[:S]
            seed_time = torch.randint(0, T_MAX, (S,), generator=g, device=dev)
            stats, ego_stats = {}, {}
            ops.temporal_neighbor_sample(rowptr, col, order.order, order.sorted_time, seeds, seed_time, fanouts,
                                         "uniform", False, seed, stats=stats)
            ops.ego_k_hop_sample(rowptr, col, seeds, fanouts, False, seed, stats=ego_stats)
            sub, n_id, e_id, ptr, _ = adj.temporal_neighbor_sample(seeds, seed_time, fanouts, time=order, seed=seed)
            ego_of = torch.repeat_interleave(torch.arange(S, device=dev), ptr[1:] - ptr[:-1])
            rows_out = ops.ptr2ind(sub.storage.rowptr(), e_id.numel())
            assert bool((edge_time[e_id] <= seed_time[ego_of[rows_out]]).all())  # nothing from a seed's future
            _, ego_n_id, ego_e_id, _, _ = adj.ego_k_hop_sample(seeds, fanouts, seed=seed)
            res = alternate({"sample": (lambda: adj.temporal_neighbor_sample(seeds, seed_time, fanouts, time=order,
                                                                             seed=seed), CALLS),
                             "ego": (lambda: adj.ego_k_hop_sample(seeds, fanouts, seed=seed), CALLS)})
            med = {k: statistics.median(v) for k, v in res.items()}
            print(f"   {S} seeds x {fanouts}: {stats['walk_entries']} walk entries, {stats['host_reads']} host reads; "
                  f"sample: n = {n_id.numel()}, nnz' = {e_id.numel()}; ego: n = {ego_n_id.numel()}, "
                  f"nnz' = {ego_e_id.numel()}, {ego_stats['host_reads']} host reads", flush=True)
            print(f"     temporal_neighbor_sample  {spread(res['sample'])}", flush=True)
            print(f"     ego_k_hop_sample          {spread(res['ego'])}   sample / ego = x{med['sample'] / med['ego']:.2f}",
                  flush=True)
            del sub, n_id, e_id, ptr, ego_n_id, ego_e_id
    del adj, rowptr, col, order, edge_time
    torch.cuda.empty_cache()


def trace():
    import time

    N, rowptr, col, adj, edge_time, g = setup(config3)
    order = EdgeTimeOrder(adj, edge_time=edge_time)
    S, fanouts = BATCHES[0]
    seeds = torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(S))[:S]
    seed_time = torch.randint(0, T_MAX, (S,), generator=g, device=dev)
    for _ in range(3):
        adj.temporal_neighbor_sample(seeds, seed_time, fanouts, time=order, seed=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        adj.temporal_neighbor_sample(seeds, seed_time, fanouts, time=order, seed=1)
    torch.cuda.synchronize()
    print(f"   23 calls of the sample, {S} seeds x {fanouts}; wall time of the last 20: "
          f"{(time.perf_counter() - t0) * 50:.3f} ms per call", flush=True)


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}", flush=True)
    if "--trace" in sys.argv:
        trace()
        sys.exit(0)
    run("config-3 shape", config3)
    if "--quick" not in sys.argv:
        run("R-MAT 24", rmat24)
