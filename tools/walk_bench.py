#!/usr/bin/env python3
"""random_walk / saint_subgraph on the config-3 shape (2 M x 2 M, 20 M entries) and R-MAT 24
(bench.rmat_graph(24, 100 M)), against the same semantics written with torch ops on the GPU:

  random_walk    a Python loop over the steps.  "torch exact" restates the counter-based draw of
                 csrc/rng.h in int64 ops and is checked bit-equal; "torch rand" is the loop a user
                 writes (torch.rand draws, five gathers per step), the cheaper of the two and the
                 one the HIP time is compared with.
  saint_subgraph full + index_put (assoc), repeat_interleave over the selected rows, a mask and
                 nonzero, a stable re-sort of (row, col') and a bincount for rowptr'; checked
                 bit-equal.

Workloads: DeepWalk (every node a start, L = 80), GraphSAINT (20 k roots, L = 2, then
saint_subgraph of the unique() nodes), saint_subgraph of a sorted 10 % node sample.  HIP-event
means after a warm-up call; the end-to-end calls include the op's host read.  Byte model of a walk
step: 24 B read (the rowptr pair, one col entry) and 8 B written; line-granular,
two random 128-byte lines read and 8 B written.  The random_walk store schemes (variants 1-4 of
psa_random_walk_set_variant) are timed alternately on the same inputs.

usage: python tools/walk_bench.py [--quick]   (--quick: config 3 only)"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bench import event_ms, rmat_graph  # noqa: E402
import paddle_sparse_amd as psa  # noqa: E402
from paddle_sparse_amd import SparseTensor, ops  # noqa: E402

dev = torch.device("cuda", 0)
M64 = (1 << 64) - 1
VARIANTS = {1: "store per step", 2: "16-step bursts", 3: "store per step, 2 walks/lane",
            4: "16-step bursts, 2 walks/lane"}


def _s64(c):
    return c - (1 << 64) if c >= 1 << 63 else c


def _srl(z, k):  # logical right shift of int64 bits
    return (z >> k) & ((1 << (64 - k)) - 1)


def torch_mix64(z):
    z = z + _s64(0x9E3779B97F4A7C15)
    z = (z ^ _srl(z, 30)) * _s64(0xBF58476D1CE4E5B9)
    z = (z ^ _srl(z, 27)) * _s64(0x94D049BB133111EB)
    return z ^ _srl(z, 31)


def torch_walk_exact(rowptr, col, start, L, seed):
    """random_walk in torch ops, bit-equal (degrees < 2^31)."""
    S = start.numel()
    cur = start.clone()
    stream = torch_mix64(torch_mix64(torch.arange(S, device=dev)) ^ _s64(seed & M64))
    out = torch.empty((S, L + 1), dtype=torch.int64, device=dev)
    out[:, 0] = cur
    for l in range(L):
        s = rowptr[cur]
        deg = rowptr[cur + 1] - s
        r = torch_mix64(stream + l)
        pick = _srl(_srl(r, 32) * deg + _srl((r & 0xFFFFFFFF) * deg, 32), 32)
        cur = torch.where(deg > 0, col[(s + pick).clamp_(max=col.numel() - 1)], cur)
        out[:, l + 1] = cur
    return out


def torch_walk_rand(rowptr, col, start, L):
    """The same walk with torch.rand draws (not the same stream): the loop a user writes."""
    cur = start.clone()
    out = torch.empty((start.numel(), L + 1), dtype=torch.int64, device=dev)
    out[:, 0] = cur
    for l in range(L):
        s = rowptr[cur]
        deg = rowptr[cur + 1] - s
        pick = (torch.rand(cur.numel(), device=dev) * deg).long()
        cur = torch.where(deg > 0, col[(s + pick).clamp_(max=col.numel() - 1)], cur)
        out[:, l + 1] = cur
    return out


def torch_saint(rowptr, col, node_idx, N):
    S = node_idx.numel()
    assoc = torch.full((N,), -1, dtype=torch.int64, device=dev)
    assoc[node_idx] = torch.arange(S, device=dev)
    start, deg = rowptr[node_idx], rowptr[node_idx + 1] - rowptr[node_idx]
    rows = torch.repeat_interleave(torch.arange(S, device=dev), deg)
    first = torch.cumsum(deg, 0) - deg
    e = torch.arange(rows.numel(), device=dev) - first[rows] + start[rows]
    c = assoc[col[e]]
    keep = (c >= 0).nonzero().view(-1)
    rows, c, e = rows[keep], c[keep], e[keep]
    _, order = torch.sort(rows * S + c, stable=True)
    rows, c, e = rows[order], c[order], e[order]
    ptr = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=S), 0)
    return ptr, c, e


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


def walk_line(label, S, L, t_ours, t_theirs):
    steps = S * L
    alg = (24 + 8) * steps
    lines = (2 * 128 + 8) * steps
    print(f"   {label:44s} {t_ours:9.3f} ms   torch ops {t_theirs:9.3f} ms   x{t_theirs / t_ours:6.1f}   "
          f"{steps / t_ours / 1e6:7.2f} G steps/s   algorithmic {alg / t_ours / 1e9:5.2f} TB/s, "
          f"line-granular {lines / t_ours / 1e9:5.2f} TB/s", flush=True)


def run(name, make):
    N, rowptr, col = make()
    nnz = col.numel()
    a = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    deg = rowptr[1:] - rowptr[:-1]
    print(f"== {name}: {N} nodes, {nnz} entries, {int((deg == 0).sum())} without entries, longest row "
          f"{int(deg.max())}", flush=True)
    seed = 20261016
    with torch.no_grad():
        # ---- DeepWalk: every node a start, L = 80
        start = torch.arange(N, device=dev)
        L = 80
        ours = psa.random_walk(a, start, L, seed=seed)
        assert torch.equal(ours, torch_walk_exact(rowptr, col, start, L, seed))
        del ours
        print("   DeepWalk walks bit-equal to the torch restatement", flush=True)
        t_ours = event_ms(lambda: psa.random_walk(a, start, L, seed=seed), 3)
        t_exact = event_ms(lambda: torch_walk_exact(rowptr, col, start, L, seed), 1)
        t_rand = event_ms(lambda: torch_walk_rand(rowptr, col, start, L), 2)
        print(f"   torch exact restatement {t_exact:.3f} ms, torch.rand loop {t_rand:.3f} ms", flush=True)
        walk_line(f"random_walk all {N} nodes, L = 80", N, L, t_ours, min(t_exact, t_rand))
        # ---- GraphSAINT: 20 k roots, L = 2, then the subgraph of the unique nodes
        roots = torch.randint(0, N, (20_000,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        ours = psa.random_walk(a, roots, 2, seed=seed)
        assert torch.equal(ours, torch_walk_exact(rowptr, col, roots, 2, seed))
        t_ours = event_ms(lambda: psa.random_walk(a, roots, 2, seed=seed), 20)
        t_rand = event_ms(lambda: torch_walk_rand(rowptr, col, roots, 2), 20)
        t_exact = event_ms(lambda: torch_walk_exact(rowptr, col, roots, 2, seed), 20)
        walk_line("random_walk 20 k roots, L = 2", 20_000, 2, t_ours, min(t_exact, t_rand))
        node_idx = ours.view(-1).unique()
        for label, idx, reps in (("saint_subgraph(unique walk nodes)", node_idx, 20),
                                 ("saint_subgraph(10 % node sample)",
                                  torch.randperm(N, device=dev)[:N // 10].sort()[0], 5)):
            sub, e = psa.saint_subgraph(a, idx)
            p, c, er = torch_saint(rowptr, col, idx, N)
            assert torch.equal(sub.storage.rowptr(), p) and torch.equal(sub.storage.col(), c) and torch.equal(e, er)
            t_ours = event_ms(lambda: psa.saint_subgraph(a, idx), reps)
            t_theirs = event_ms(lambda: torch_saint(rowptr, col, idx, N), reps)
            C = int(deg[idx].sum())
            S = idx.numel()
            model = 8 * 2 * S + 8 * S + 16 * C + 8 * 3 * sub.nnz() + 8 * (S + 1)  # node_idx/pairs, assoc, col+assoc per candidate, outputs
            print(f"   {label:44s} {t_ours:9.3f} ms   torch ops {t_theirs:9.3f} ms   x{t_theirs / t_ours:6.1f}   "
                  f"S = {S}, {C} candidates, {sub.nnz()} kept, model {model / t_ours / 1e9:5.2f} TB/s", flush=True)
            del sub, e, p, c, er
        # ---- store schemes, alternated on the same inputs
        res = {v: [] for v in VARIANTS}
        for _ in range(2):
            for v in VARIANTS:
                prev = ops.random_walk_set_variant(v)
                psa.random_walk(a, start, L, seed=seed)
                res[v].append((event_ms(lambda: psa.random_walk(a, start, L, seed=seed), 2),
                               event_ms(lambda: psa.random_walk(a, roots, 2, seed=seed), 20),
                               event_ms(lambda: psa.random_walk(a, roots, 80, seed=seed), 5)))
                ops.random_walk_set_variant(prev)
        print("   store schemes (ms; DeepWalk all nodes L = 80 | 20 k roots L = 2 | 20 k roots L = 80), two "
              "alternating rounds:", flush=True)
        for v, name_v in VARIANTS.items():
            cells = " | ".join(" ".join(f"{t[i]:8.3f}" for t in res[v]) for i in range(3))
            print(f"     {v} {name_v:32s} {cells}", flush=True)
    del a, rowptr, col
    torch.cuda.empty_cache()


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}", flush=True)
    run("config-3 shape", config3)
    if "--quick" not in sys.argv:
        run("R-MAT 24", rmat24)
