#!/usr/bin/env python3
"""ego_k_hop_sample on the config-3 shape (2 M x 2 M, 20 M entries) and R-MAT 24
(bench.rmat_graph(24, 100 M)): the op against the loop a user writes without it.

  op     adj.ego_k_hop_sample(seeds, fanouts): one call for all S egos
  loop   for every seed: adj.neighbor_sample(seeds[i:i+1], fanouts, directed=False), the n_id and
         e_id lists concatenated.  That is S fresh relabel maps, S * (L + 2) host reads and S
         sorts; the block-diagonal assembly of the S matrices, which a user would still have to
         write, is NOT in the loop's time.  The loop de-duplicates between hops and draws from
         other streams, so for k >= 0 its egos are other samples of the same distribution; with
         -1 fan-outs they are the same node sets, which is checked on the first egos.

Batches: 256 and 1024 seeds x [10, 5]; 64 seeds x [-1, -1].  HIP-event time of a whole call (host
reads included), REPEATS alternating rounds after a warm-up round, CALLS calls of the op and one
pass of the loop per round; min / median / max over the rounds, and loop / op of the medians.

T sweep: the induce passes alone (count, scan, write, on the structures of a finished call) with
T = 8, 16, 32, 64, alternated the same way.

usage: python tools/ego_sample_bench.py [--quick | --trace]   (--quick: config 3 only; --trace: 23
calls of the op at 1024 seeds x [10, 5] on config 3 with their wall time, for a kernel trace)"""
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bench import event_ms  # noqa: E402
from neighbor_bench import config3, rmat24, spread  # noqa: E402
from paddle_sparse_amd import SparseTensor, _lib, ops  # noqa: E402

dev = torch.device("cuda", 0)
BATCHES = ((256, [10, 5]), (1024, [10, 5]), (64, [-1, -1]))
REPEATS, CALLS = 5, 5
THRESHOLDS = (8, 16, 32, 64)


def loop(adj, seeds, fanouts, seed):
    ids, edges = [], []
    for i in range(seeds.numel()):
        _, n_id, e_id, _ = adj.neighbor_sample(seeds[i:i + 1], fanouts, directed=False, seed=seed + i)
        ids.append(n_id)
        edges.append(e_id)
    return torch.cat(ids), torch.cat(edges)


def induce_passes(rowptr, col, seeds, n_id, ptr):
    """The count pass, the scan and the write pass as ops.ego_k_hop_sample issues them, on preallocated outputs."""
    lib = _lib.load()
    N, S, n = rowptr.numel() - 1, seeds.numel(), n_id.numel()
    ego_of = torch.repeat_interleave(torch.arange(S, device=dev), ptr[1:] - ptr[:-1])
    root, counts = torch.empty(S, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    p = lambda t: t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream

    def count():
        _lib.check(lib.psa_ego_induce_count(p(rowptr), p(col), N, p(seeds), S, p(n_id), p(ego_of), p(ptr), n, p(root), S,
                                            p(counts), n, stream))
        return ops.count2ptr(counts)

    rowptr_out = count()
    nnz = int(rowptr_out[-1])
    out = torch.empty((2, nnz), dtype=torch.int64, device=dev)

    def both():
        rp = count()
        _lib.check(lib.psa_ego_induce_write(p(rowptr), p(col), N, S, p(n_id), p(ego_of), p(ptr), n, p(rp), nnz,
                                            p(out[0]), p(out[1]), nnz, stream))

    return both, nnz


def run(name, make):
    N, rowptr, col = make()
    adj = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    deg = rowptr[1:] - rowptr[:-1]
    print(f"== {name}: {N} nodes, {col.numel()} entries, longest row {int(deg.max())}", flush=True)
    print(f"   ms per call, min / median / max of {REPEATS} alternating rounds ({CALLS} calls of the op, one pass of "
          f"the loop)", flush=True)
    seed = 20261020
    with torch.no_grad():
        for S, fanouts in BATCHES:
            seeds = torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(S))[:S]
            stats = {}
            try:
                ops.ego_k_hop_sample(rowptr, col, seeds, fanouts, False, seed, stats=stats)
            except ValueError as exc:  # a -1 batch whose walk list passes a limit: said, not worked around
                print(f"   {S} seeds x {fanouts}: refused: {exc}", flush=True)
                continue
            sub, n_id, e_id, ptr, root = adj.ego_k_hop_sample(seeds, fanouts, seed=seed)
            if all(k < 0 for k in fanouts):
                for g in range(min(S, 4)):
                    _, ids, _, _ = adj.neighbor_sample(seeds[g:g + 1], fanouts, directed=False, seed=seed)
                    assert torch.equal(torch.sort(ids)[0], n_id[ptr[g]:ptr[g + 1]])
            n_loop, e_loop = loop(adj, seeds, fanouts, seed)
            fns = {"op": (lambda: adj.ego_k_hop_sample(seeds, fanouts, seed=seed), CALLS),
                   "loop": (lambda: loop(adj, seeds, fanouts, seed), 1)}
            res = {k: [] for k in fns}
            for rnd in range(REPEATS + 1):
                for k, (fn, calls) in fns.items():
                    t = event_ms(fn, calls)
                    if rnd > 0:  # round 0 warms the allocator
                        res[k].append(t)
            med = {k: statistics.median(v) for k, v in res.items()}
            sizes = ptr[1:] - ptr[:-1]
            print(f"   {S} seeds x {fanouts}: {stats['walk_entries']} walk entries, n = {n_id.numel()} nodes (largest ego "
                  f"{int(sizes.max())}), nnz' = {e_id.numel()}, {stats['host_reads']} host reads "
                  f"(loop: {n_loop.numel()} nodes, {e_loop.numel()} entries)", flush=True)
            print(f"     op    {spread(res['op'])}", flush=True)
            print(f"     loop  {spread(res['loop'])}   loop / op = x{med['loop'] / med['op']:.1f}", flush=True)
            both, nnz = induce_passes(rowptr, col, seeds, n_id, ptr)
            assert nnz == e_id.numel()
            sweep = {T: [] for T in THRESHOLDS}
            for rnd in range(REPEATS + 1):
                for T in THRESHOLDS:
                    ops.ego_set_threshold(T)
                    t = event_ms(both, 20)
                    if rnd > 0:
                        sweep[T].append(t)
            ops.ego_set_threshold(32)
            print("     induce passes alone (count + scan + write), ms: "
                  + ";  ".join(f"T = {T}: {spread(v)}" for T, v in sweep.items()), flush=True)
            del sub, n_id, e_id, ptr, root
    del adj, rowptr, col
    torch.cuda.empty_cache()


def trace():
    import time

    N, rowptr, col = config3()
    adj = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    S, fanouts = BATCHES[1]
    seeds = torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(S))[:S]
    for _ in range(3):
        adj.ego_k_hop_sample(seeds, fanouts, seed=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        adj.ego_k_hop_sample(seeds, fanouts, seed=1)
    torch.cuda.synchronize()
    print(f"   23 calls of the op, {S} seeds x {fanouts}; wall time of the last 20: "
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
