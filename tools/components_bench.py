#!/usr/bin/env python3
"""connected_components and largest_connected_components against what a user does today, on five
graphs, every entry stored both ways (symmetrised, coalesced) as in tools/node2vec_bench.py:

  config-3     the 2 M x 2 M shape of bench.py with 20 M random entries
  R-MAT 24     bench.rmat_graph(24, 100 M)
  grid         the 1414 x 1414 five-point grid of tools/rcm_bench.py, labels shuffled: a large diameter
  path         2 M nodes in identity order: init leaves ONE chain of depth N, the known worst case of
               the find (reported whether it wins or loses)
  matching     a perfect matching of 2 M nodes: 1 M components, nothing to compress

Forms, timed ALTERNATELY on the same graph over several rounds so that drift hits all alike (wall
clock around a synchronised call: both new calls end in a host read); per form the median and the
range of the rounds are printed:

  hip cc         adj.connected_components()
  hip largest    adj.largest_connected_components()  (the components, bincount, the ranking, saint_subgraph)
  torch          min-label propagation in torch ops: labels.scatter_reduce_(amin) over the entries plus one
                 pointer jump labels[labels], looped until nothing changes (one host read per round); stopped
                 after TORCH_BUDGET_S seconds, and then reported as NOT converged with the rounds it made
  scipy          scipy.sparse.csgraph.connected_components(directed=True, connection="weak") on the host, on a
                 csr_matrix built outside the timing
  scipy + copies the same plus the copy of rowptr and col to the host and of the labels back

The labels of the HIP op are held to scipy's bit for bit on every graph, and to the torch form's when it
converged.  Next to each graph: the share of entries whose two ends init had joined already (the first
column of a row as its parent), which is the work the hook does not have to do.  The CAS retries per entry
are NOT counted: counting them needs a counter in the kernel, that is a second build of it, and no variant
switch is kept in the tree.

usage: python tools/components_bench.py [--quick]   (--quick: the grid, the path and the matching only)"""
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import scipy.sparse
import torch
from scipy.sparse.csgraph import connected_components as scipy_components

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from node2vec_bench import config3, rmat24, symmetrised  # noqa: E402
from paddle_sparse_amd import SparseTensor, ops  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS = 3
TORCH_BUDGET_S = 20.0
NODES = 2_000_000


def grid():
    n = 1414
    idx = torch.arange(n * n, device=dev).view(n, n)
    a = torch.cat([idx[:, :-1].reshape(-1), idx[:-1].reshape(-1)])
    b = torch.cat([idx[:, 1:].reshape(-1), idx[1:].reshape(-1)])
    lab = torch.randperm(n * n, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    return symmetrised(n * n, lab[a], lab[b])


def path():
    v = torch.arange(NODES - 1, device=dev)
    return symmetrised(NODES, v, v + 1)


def matching():
    p = torch.randperm(NODES, device=dev, generator=torch.Generator(device=dev).manual_seed(6))
    return symmetrised(NODES, p[:NODES // 2], p[NODES // 2:])


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def torch_components(N, row, col):
    """(labels = the smallest node id of every node's component, rounds, converged)."""
    labels = torch.arange(N, device=dev)
    start, rounds = time.perf_counter(), 0
    while True:
        rounds += 1
        new = labels.clone()
        new.scatter_reduce_(0, row, labels[col], "amin")  # every entry is stored both ways: one direction does
        new = new[new]
        if bool((new == labels).all()):
            return labels, rounds, True
        labels = new
        if time.perf_counter() - start > TORCH_BUDGET_S:
            return labels, rounds, False


def run(name, make):
    N, rowptr, col = make()
    nnz = col.numel()
    a = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    row = a.storage.row()
    with torch.no_grad():
        n, labels = a.connected_components()  # warm-up, and the result every form is held to
        sizes = ops.bincount(labels, n)
        root0, _ = ops.components_flatten(ops.components_init(rowptr, col))
        joined = float((root0[row] == root0[col]).double().mean()) if nnz else 0.0
        del root0
        print(f"== {name}, symmetrised: {N} nodes, {nnz} entries, {n} components, the largest {int(sizes.max())} nodes; "
              f"{100 * joined:.1f} % of the entries joined by init", flush=True)

        host = scipy.sparse.csr_matrix((np.ones(nnz, np.int8), col.cpu().numpy(), rowptr.cpu().numpy()), shape=(N, N))
        want_n, want = scipy_components(host, directed=True, connection="weak")
        assert want_n == n and np.array_equal(labels.cpu().numpy(), want), "labels differ from scipy's"
        del want

        def scipy_with_copies():
            m = scipy.sparse.csr_matrix((np.ones(nnz, np.int8), col.cpu().numpy(), rowptr.cpu().numpy()), shape=(N, N))
            return torch.from_numpy(scipy_components(m, directed=True, connection="weak")[1]).to(dev)

        forms = {
            "hip cc": a.connected_components,
            "hip largest": a.largest_connected_components,
            "torch": lambda: torch_components(N, row, col),
            "scipy": lambda: scipy_components(host, directed=True, connection="weak"),
            "scipy + copies": scipy_with_copies,
        }
        a.largest_connected_components()  # warm-up
        times, note = {k: [] for k in forms}, ""
        for r in range(ROUNDS):
            for k, fn in forms.items():
                if r > 0 and k.startswith("scipy") and nnz > 100_000_000:
                    continue  # tens of seconds a call there: one round
                ms, out = wall_ms(fn)
                times[k].append(ms)
                if k == "torch":
                    lab, rounds, converged = out
                    note = f"{rounds} rounds" + ("" if converged else f", NOT converged in {TORCH_BUDGET_S:.0f} s")
                    if converged:  # the smallest node of the component, ranked, is the label
                        is_root = (lab == torch.arange(N, device=dev)).to(torch.int64)
                        assert torch.equal((torch.cumsum(is_root, 0) - is_root)[lab], labels), "torch form differs"
                    del lab, out
        base = statistics.median(times["hip cc"])
        print(f"   ms per call, wall clock, {ROUNDS} alternating rounds (scipy: one round above 100 M entries); "
              f"ratio = median over the median of hip cc:", flush=True)
        for k, ts in times.items():
            med = statistics.median(ts)
            print(f"     {k:15s} median {med:11.3f}   range {min(ts):11.3f} .. {max(ts):11.3f}   x{med / base:8.2f}   "
                  f"{note if k == 'torch' else ''}", flush=True)
    del a, rowptr, col, row, host, labels
    torch.cuda.empty_cache()


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}", flush=True)
    run("grid 1414 x 1414, shuffled", grid)
    run("path of 2 M nodes, identity order", path)
    run("perfect matching of 2 M nodes", matching)
    if "--quick" not in sys.argv:
        run("config-3 shape", config3)
        run("R-MAT 24", rmat24)
