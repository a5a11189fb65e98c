#!/usr/bin/env python3
"""node2vec (p, q) random_walk against the first-order walks, DeepWalk shape (every node a start,
L = 80), on the config-3 shape (2 M x 2 M, 20 M entries) and R-MAT 24 (bench.rmat_graph(24,
100 M)), both symmetrised (every entry stored both ways, coalesced), uniform random weights.

The walks are timed ALTERNATELY on the same inputs, several rounds, so that drift hits all of
them alike; per walk the median and the range of the rounds are printed:

  uniform                 ops.random_walk: psa_random_walk, the baseline of the uniform rows
  weighted                ops.random_walk_weighted with the row CDF, the baseline of the weighted row
  n2v (1, 1)              psa_node2vec_walk with every threshold at 2^53: no search, no acceptance
                          word; the same bits as `uniform` (checked here), held to its time
  n2v (0.25, 4), (4, 0.25), (1, 0.5)
  n2v weighted (0.25, 4)

Next to each biased walk: the mean tries per drawing step and the mean ceil(log2(deg(t) + 1)) of
the rows searched, both from the serial restatement (tests/node2vec_ref.py) on a sample of the
walks, which is first held to the kernel's output bit for bit.

Model of a try: the plain step's dependent loads (the rowptr pair, one col
entry; weighted: the total and log2(deg) of cum), then, unless the proposal leads back or q == 1,
about log2(deg(t)) dependent 8-byte loads in row t, then one more mix64.

usage: python tools/node2vec_bench.py [--quick]   (--quick: config 3 only)"""
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from bench import event_ms, rmat_graph  # noqa: E402
import node2vec_ref as nr  # noqa: E402
import paddle_sparse_amd as psa  # noqa: E402
from paddle_sparse_amd import SparseTensor, ops  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS, L, SAMPLE = 3, 80, 192
ONE = 2**53


def symmetrised(N, row, col):
    keys = torch.unique(torch.cat([row * N + col, col * N + row]))  # sorted
    row, col = keys // N, keys % N
    return N, ops.ind2ptr(row, N), col.contiguous()


def config3():
    M = 2_000_000
    g = torch.Generator(device=dev).manual_seed(3)
    row = torch.randint(0, M, (20_000_000,), generator=g, device=dev)
    col = torch.randint(0, M, (20_000_000,), generator=g, device=dev)
    return symmetrised(M, row, col)


def rmat24():
    N, _, row, col, _ = rmat_graph(24, 100_000_000, dev)
    return symmetrised(N, row, col)


def sample_stats(rowptr_np, col_np, cum_np, rowptr, col, cum, start, seed, thr, max_tries):
    """(mean tries per drawing step, mean search depth) from the restatement on SAMPLE walks,
    after holding it to the kernel on them."""
    stats = {}
    want = nr.ref_node2vec_walk(rowptr_np, col_np, cum_np, start.cpu().numpy(), L, seed, thr, max_tries, stats)
    got = ops.node2vec_walk(rowptr, col, cum, start, L, seed, thr, max_tries, True)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    prev = want[0][:, :-2]  # the row searched at step l >= 1 is that of the node of step l - 1
    depth = np.ceil(np.log2(np.diff(rowptr_np)[prev] + 1.0)).mean()
    return stats["tries"] / max(stats["steps"], 1), float(depth)


def run(name, make):
    N, rowptr, col = make()
    nnz = col.numel()
    value = torch.rand(nnz, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    a = SparseTensor(rowptr=rowptr, col=col, value=value, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    deg = rowptr[1:] - rowptr[:-1]
    print(f"== {name}, symmetrised: {N} nodes, {nnz} entries, {int((deg == 0).sum())} without entries, "
          f"longest row {int(deg.max())}", flush=True)
    seed = 20261020
    with torch.no_grad():
        cum = psa.EdgeCDF(a).cum
        start = torch.arange(N, device=dev)
        probe = start[:: max(N // SAMPLE, 1)][:SAMPLE].contiguous()
        rowptr_np, col_np, cum_np = rowptr.cpu().numpy(), col.cpu().numpy(), cum.cpu().numpy()
        one = ((ONE,) * 3, 32)
        assert torch.equal(ops.node2vec_walk(rowptr, col, None, start, L, seed, *one),
                           ops.random_walk(rowptr, col, start, L, seed))
        cases = {"uniform": (None, None), "weighted": (cum, None), "n2v (1, 1)": (None, one)}
        for p, q in ((0.25, 4), (4, 0.25), (1, 0.5)):
            cases[f"n2v ({p}, {q})"] = (None, nr.bias(p, q))
        cases["n2v weighted (0.25, 4)"] = (cum, nr.bias(0.25, 4))
        fns, notes = {}, {}
        for k, (c, b) in cases.items():
            if b is None:
                fns[k] = (lambda: ops.random_walk(rowptr, col, start, L, seed)) if c is None else \
                    (lambda: ops.random_walk_weighted(rowptr, col, cum, start, L, seed))
                notes[k] = ""
            else:
                fns[k] = lambda c=c, b=b: ops.node2vec_walk(rowptr, col, c, start, L, seed, *b)
                tries, depth = sample_stats(rowptr_np, col_np, None if c is None else cum_np, rowptr, col, c, probe,
                                            seed, *b)
                notes[k] = f"   tries/step {tries:6.2f}   search depth {depth:5.2f}"
        del rowptr_np, col_np, cum_np
        times = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                fn()  # warm-up: the allocator has the output's block afterwards
                times[k].append(event_ms(fn, 2))
        print(f"   DeepWalk shape: all {N} nodes, L = {L} (ms over {ROUNDS} alternating rounds; ratio = median over "
              f"median of the baseline: uniform, or weighted for the weighted row):", flush=True)
        for k, ts in times.items():
            med = statistics.median(ts)
            base = statistics.median(times["weighted" if "weighted" in k else "uniform"])
            print(f"     {k:24s} median {med:10.3f}   range {min(ts):10.3f} .. {max(ts):10.3f}   x{med / base:7.2f}   "
                  f"{N * L / med / 1e6:7.3f} G steps/s{notes[k]}", flush=True)
    del a, rowptr, col, value, cum
    torch.cuda.empty_cache()


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}", flush=True)
    run("config-3 shape", config3)
    if "--quick" not in sys.argv:
        run("R-MAT 24", rmat24)
