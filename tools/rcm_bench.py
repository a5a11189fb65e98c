#!/usr/bin/env python3
"""reverse_cuthill_mckee on three matrices, and what the ordering does to SpMM:

  grid     a 2-D five-point grid, 1414 x 1414 nodes (the config-3 node count), labels shuffled
  config-3 the 2 M x 2 M, 20 M-entry random matrix of bench.py, symmetrised
  R-MAT 21 bench.rmat_graph(21, 20 M), symmetrised

Per matrix: the ordering (ops.reverse_cuthill_mckee: wall clock including its host reads, mean
of 3 after a warm-up call) under the default variant and with every level forced through the
large path, with level counts, host reads and the share of levels each path served; the
SparseTensor op end to end (ordering + permute, is_symmetric=True); scipy's
reverse_cuthill_mckee on the host; the bandwidth max |row - col| before and after; and
spmm_sum at F = 128 on the matrix as given, RCM-permuted and randomly permuted, the three
alternating in one run (HIP-event means of 5 launches, 3 rounds).  The default and the
forced-large runs must agree bit for bit and perm must be a permutation.

usage: python tools/rcm_bench.py [--quick]   (--quick: a 300 x 300 grid only)"""
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bench import event_ms, make_workload, rmat_graph  # noqa: E402
import paddle_sparse_amd as psa  # noqa: E402
from paddle_sparse_amd import SparseTensor, ops  # noqa: E402

dev = torch.device("cuda", 0)
F = 128


def from_pairs(N, row, col):
    keys = torch.sort(row * N + col)[0]
    row, col = keys // N, keys % N
    return SparseTensor(rowptr=ops.ind2ptr(row, N), col=col.contiguous(), value=torch.ones(col.numel(), device=dev),
                        sparse_sizes=(N, N), is_sorted=True, trust_data=True)


def grid(n):
    idx = torch.arange(n * n, device=dev).view(n, n)
    a = torch.cat([idx[:, :-1].reshape(-1), idx[:-1].reshape(-1)])
    b = torch.cat([idx[:, 1:].reshape(-1), idx[1:].reshape(-1)])
    lab = torch.randperm(n * n, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    return from_pairs(n * n, lab[torch.cat([a, b])], lab[torch.cat([b, a])])


def config3():
    M = 2_000_000
    rowptr, col, val = make_workload(M, M, 20_000_000, F, 3, dev)
    row = ops.ptr2ind(rowptr, col.numel())  # make_workload leaves the columns of a row unsorted: the constructor sorts
    return SparseTensor(row=row, col=col, value=val, sparse_sizes=(M, M), is_sorted=False).to_symmetric()


def rmat21():
    N, rowptr, row, col, val = rmat_graph(21, 20_000_000, dev)
    return SparseTensor(rowptr=rowptr, row=row, col=col, value=val, sparse_sizes=(N, N), is_sorted=True,
                        trust_data=True).to_symmetric()


def wall_ms(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def bandwidth(a):
    row, col, _ = a.coo()
    return int((row - col).abs().max()) if col.numel() else 0


def run(name, make):
    a = make()
    N = a.sparse_size(0)
    rowptr, col, _ = a.csr()
    deg = rowptr[1:] - rowptr[:-1]
    print(f"== {name}: {N} nodes, {col.numel()} entries, {int((deg == 0).sum())} without entries, longest row "
          f"{int(deg.max())}, bandwidth {bandwidth(a)}", flush=True)
    perms = {}
    for variant, label in ((0, "default"), (1, "every level large")):
        prev = ops.rcm_set_variant(variant)
        stats = {}
        perms[variant] = ops.reverse_cuthill_mckee(rowptr, col, stats=stats)
        ms = wall_ms(lambda: ops.reverse_cuthill_mckee(rowptr, col))
        ops.rcm_set_variant(prev)
        levels = stats["small_levels"] + stats["large_levels"]
        print(f"   ordering, {label:18s} {ms:10.3f} ms   {levels} levels: {stats['small_levels']} small "
              f"({100.0 * stats['small_levels'] / max(levels, 1):.1f} %) in {stats['small_launches']} launches, "
              f"{stats['large_levels']} large; {stats['host_reads']} host reads", flush=True)
    perm = perms[0]
    assert torch.equal(perm, perms[1]), "the two paths disagree"
    assert torch.equal(torch.sort(perm)[0], torch.arange(N, device=dev)), "not a permutation"
    ms = wall_ms(lambda: psa.reverse_cuthill_mckee(a, is_symmetric=True))
    print(f"   SparseTensor.reverse_cuthill_mckee (ordering + permute) {ms:10.3f} ms", flush=True)
    out = a.permute(perm)
    rnd = a.permute(torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(7)))
    print(f"   bandwidth after RCM {bandwidth(out)}, after a random permutation {bandwidth(rnd)}", flush=True)
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import reverse_cuthill_mckee as scipy_rcm
    except ImportError:
        print("   scipy not installed", flush=True)
    else:
        m = sp.csr_matrix((torch.ones(col.numel()).numpy(), col.cpu().numpy(), rowptr.cpu().numpy()), shape=(N, N))
        t = time.perf_counter()
        sperm = scipy_rcm(m, symmetric_mode=True)
        ms = (time.perf_counter() - t) * 1e3
        sperm = torch.from_numpy(sperm.astype("int64")).to(dev)
        print(f"   scipy reverse_cuthill_mckee on the host {ms:10.3f} ms (one call, without the copies), bandwidth "
              f"{bandwidth(a.permute(sperm))}, same perm: {bool(torch.equal(sperm, perm))}", flush=True)
        del m, sperm
    x = torch.randn(N, F, device=dev, generator=torch.Generator(device=dev).manual_seed(9))
    forms = {"as given": a, "RCM": out, "random": rnd}
    times = {k: [] for k in forms}
    with torch.no_grad():
        for k, m in forms.items():
            ops.spmm_sum(*m.csr(), x)  # warm-up
        for _ in range(3):
            for k, m in forms.items():
                r, c, v = m.csr()
                times[k].append(event_ms(lambda: ops.spmm_sum(r, c, v, x), 5))
    for k in forms:
        print(f"   spmm_sum F = {F}, {k:9s} " + " ".join(f"{t:8.3f}" for t in times[k]) + " ms", flush=True)
    best = {k: min(v) for k, v in times.items()}
    print(f"   spmm_sum RCM / as given = {best['RCM'] / best['as given']:.3f}, RCM / random = "
          f"{best['RCM'] / best['random']:.3f} (best of the rounds)", flush=True)
    del a, out, rnd, x, forms
    torch.cuda.empty_cache()


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}", flush=True)
    if "--quick" in sys.argv:
        run("grid 300 x 300, shuffled", lambda: grid(300))
    else:
        run("grid 1414 x 1414, shuffled", lambda: grid(1414))
        run("config-3 random, symmetrised", config3)
        run("R-MAT 21, symmetrised", rmat21)
