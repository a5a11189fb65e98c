#!/usr/bin/env python3
"""neighbor_sample on the config-3 shape (2 M x 2 M, 20 M entries) and R-MAT 24
(bench.rmat_graph(24, 100 M)): three contenders, alternated in one process.

  one-shot   adj.neighbor_sample(seeds, fanouts): a fresh relabel map per call (an N-sized fill)
  sampler    a NeighborSampler kept between calls: the map stays clean, nothing sized N runs
  composed   what a user writes today: a loop of adj.sample_adj(frontier, k), the node lists merged
             with torch ops (torch.isin and cat; sample_adj's new nodes are distinct, so no
             unique()).  Every hop pays sample_adj's N-sized fill of its relabel scratch and its
             host reads, and the loop samples nodes again that an earlier hop already expanded
             (sample_adj cannot know them), so it does MORE sampling work than the op and returns
             one bipartite block per hop instead of one matrix.

Batches: 1024 seeds x [15, 10, 5] and [25, 10]; 8192 seeds x [10, 10].  HIP-event time of a whole
call (its host reads included), REPEATS alternating rounds of CALLS calls each after a warm-up round;
min / median / max over the rounds.  The one-shot op and the sampler are checked bit-equal first.

usage: python tools/neighbor_bench.py [--quick | --trace]   (--quick: config 3 only; --trace: 50 calls
of a reused sampler at 1024 seeds x [15, 10, 5] on config 3 with their wall time, for a kernel trace)"""
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bench import event_ms, rmat_graph  # noqa: E402
import paddle_sparse_amd as psa  # noqa: E402
from paddle_sparse_amd import SparseTensor, ops  # noqa: E402

dev = torch.device("cuda", 0)
BATCHES = ((1024, [15, 10, 5]), (1024, [25, 10]), (8192, [10, 10]))
REPEATS, CALLS = 7, 10


def composed(adj, seeds, fanouts, seed):
    """The hand-written loop: (n_id, [(block, block n_id) per hop])."""
    n_id, frontier, blocks = seeds, seeds, []
    for hop, k in enumerate(fanouts):
        block, ids = adj.sample_adj(frontier, k, seed=seed + hop)
        picked = ids[frontier.numel():]
        n_id = torch.cat([n_id, picked[~torch.isin(picked, n_id)]])
        blocks.append((block, ids))
        frontier = picked  # distinct already; also holds nodes that an earlier hop expanded
    return n_id, blocks


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


def spread(ts):
    return f"{min(ts):7.3f} / {statistics.median(ts):7.3f} / {max(ts):7.3f}"


def run(name, make):
    N, rowptr, col = make()
    adj = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    deg = rowptr[1:] - rowptr[:-1]
    print(f"== {name}: {N} nodes, {col.numel()} entries, longest row {int(deg.max())}", flush=True)
    print(f"   ms per call, min / median / max of {REPEATS} alternating rounds of {CALLS} calls", flush=True)
    seed = 20261019
    with torch.no_grad():
        for S, fanouts in BATCHES:
            seeds = torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(S))[:S]
            sampler = psa.NeighborSampler(adj, fanouts)
            a, b = adj.neighbor_sample(seeds, fanouts, seed=seed), sampler(seeds, seed=seed)
            assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3]
            assert all(torch.equal(x, y) for x, y in zip(a[0].csr()[:2], b[0].csr()[:2]))
            stats = {}
            ops.neighbor_sample(rowptr, col, seeds, fanouts, False, seed, stats=stats)
            n_loop, _ = composed(adj, seeds, fanouts, seed)
            fns = {"one-shot": lambda: adj.neighbor_sample(seeds, fanouts, seed=seed),
                   "sampler": lambda: sampler(seeds, seed=seed),
                   "composed": lambda: composed(adj, seeds, fanouts, seed)}
            res = {k: [] for k in fns}
            for rnd in range(REPEATS + 1):
                for k, fn in fns.items():
                    t = event_ms(fn, CALLS)
                    if rnd > 0:  # round 0 warms the allocator
                        res[k].append(t)
            med = {k: statistics.median(v) for k, v in res.items()}
            print(f"   {S} seeds x {fanouts}: n = {a[1].numel()} nodes, E = {a[2].numel()} entries, "
                  f"{stats['host_reads']} host reads (composed loop: {n_loop.numel()} nodes)", flush=True)
            for k in fns:
                rel = "" if k == "composed" else f"   composed / this = x{med['composed'] / med[k]:5.2f}"
                print(f"     {k:9s} {spread(res[k])}{rel}", flush=True)
            del sampler, a, b
    del adj, rowptr, col
    torch.cuda.empty_cache()


def trace():
    import time

    N, rowptr, col = config3()
    adj = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    S, fanouts = BATCHES[0]
    seeds = torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(S))[:S]
    sampler = psa.NeighborSampler(adj, fanouts)
    for _ in range(3):
        sampler(seeds, seed=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        sampler(seeds, seed=1)
    torch.cuda.synchronize()
    print(f"   53 calls of the sampler, {S} seeds x {fanouts}; wall time of the last 50: "
          f"{(time.perf_counter() - t0) * 20:.3f} ms per call", flush=True)


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}", flush=True)
    if "--trace" in sys.argv:
        trace()
        sys.exit(0)
    run("config-3 shape", config3)
    if "--quick" not in sys.argv:
        run("R-MAT 24", rmat24)
