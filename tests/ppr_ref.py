"""Serial restatement of the forward push of csrc/ppr.hip in plain Python ints, the case list that the
CPU and the GPU suite share, and the seeded graph builder.  Nothing here imports the package."""
import functools
from fractions import Fraction

import numpy as np

ONE = 1 << 48


def quantise(alpha, eps):
    """round(alpha * 2^32), round(eps * 2^48), halves up, in exact arithmetic"""
    return int(Fraction(alpha) * 2**32 + Fraction(1, 2)), int(Fraction(eps) * ONE + Fraction(1, 2))


def bound(alpha_q, eps_q):
    return ONE // ((alpha_q * eps_q) >> 32)


def push(rowptr, col, s, alpha_q, eps_q, max_rounds=None):
    """(p, r, rounds, pushes, edges): dicts of the positive p and r of source s, the rounds that had an
    active node, the pushes and the sum of their degrees.  Asserts the invariants of the contract."""
    rowptr, col = [int(x) for x in rowptr], [int(x) for x in col]
    r, p, touched = {s: ONE}, {}, {s}
    rounds = pushes = edges = 0
    while max_rounds is None or rounds < max_rounds:
        active = [(u, x) for u, x in r.items() if x >= eps_q * max(rowptr[u + 1] - rowptr[u], 1)]
        if not active:
            break
        rounds += 1
        shares = []
        for u, x in active:  # phase A
            deg = rowptr[u + 1] - rowptr[u]
            if deg == 0:
                p[u] = p.get(u, 0) + x
                r[u] = 0
                continue
            keep = (x * alpha_q) >> 32
            share = (x - keep) // deg
            p[u] = p.get(u, 0) + keep
            r[u] = x - keep - share * deg
            shares.append((u, share))
            edges += deg
        pushes += len(active)
        for u, share in shares:  # phase B
            for v in col[rowptr[u]:rowptr[u + 1]]:
                r[v] = r.get(v, 0) + share
                touched.add(v)
    assert sum(p.values()) + sum(r.values()) == ONE
    assert edges <= bound(alpha_q, eps_q) and len(touched) <= 1 + edges
    return {k: v for k, v in p.items() if v}, {k: v for k, v in r.items() if v}, rounds, pushes, edges


@functools.lru_cache(maxsize=None)
def graph(kind, N, seed=0):
    """(rowptr, col) of a seeded graph, rows sorted.  Row 0 is a hub with all N columns; about two random
    entries per other row; one entry is stored twice.  "sym": every entry has its mirror (the duplicate
    too).  "dir": directed, and node N - 1 is dangling (no entries) but a neighbour of the hub and others."""
    rng = np.random.default_rng(seed)
    u, v = rng.integers(1, N, 2 * N), rng.integers(1, N, 2 * N)
    u, v = np.concatenate([u, np.zeros(N, np.int64), [5]]), np.concatenate([v, np.arange(N), [6]])
    pairs = np.unique(np.stack([u, v]), axis=1)
    if kind == "sym":
        pairs = np.unique(np.concatenate([pairs, pairs[::-1]], axis=1), axis=1)
        pairs = np.concatenate([pairs, [[5, 6], [6, 5]]], axis=1)
    else:
        pairs = np.concatenate([pairs[:, pairs[0] != N - 1], [[5], [6]]], axis=1)
    order = np.lexsort((pairs[1], pairs[0]))
    row, col = pairs[0][order], pairs[1][order]
    rowptr = np.searchsorted(row, np.arange(N + 1)).astype(np.int64)
    rowptr.setflags(write=False), col.setflags(write=False)
    return rowptr, col.astype(np.int64)


# name: (kind, N, sources, alpha, eps, max_rounds).  Sources: the hub, the last node (dangling in "dir"),
# a node twice, an ordinary one.  N = 2048 gives cap = 4096, the LDS limit; N = 2500 twice that; the hub
# as source makes a frontier of N - 1 nodes (more than a chunk) and is a row longer than a workgroup.
_PAIRS = {"a": (0.15, 1e-4), "b": (0.15, 1e-6), "c": (0.5, 1e-3), "d": (0.05, 1e-5)}
CASES = {f"{kind}300{k}": (kind, 300, (0, 299, 5, 5, 17), a, e, None)
         for kind in ("sym", "dir") for k, (a, e) in _PAIRS.items()}
CASES.update({
    "below_threshold": ("dir", 300, (0, 7), 0.15, 1e-2, None),  # eps * deg(hub) = 3: an empty row
    "rounds1": ("dir", 300, (0, 299, 17), 0.15, 1e-4, 1),
    "rounds2": ("sym", 300, (0, 17), 0.15, 1e-4, 2),
    "lds_limit": ("sym", 2048, (0, 9), 0.15, 1e-5, None),
    "twice_lds": ("dir", 2500, (0, 11, 2499), 0.15, 1e-5, None),
})


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """[(p, r, rounds, pushes, edges) for every source of the case], computed once"""
    kind, N, sources, alpha, eps, max_rounds = CASES[name]
    rowptr, col = graph(kind, N)
    aq, eq = quantise(alpha, eps)
    memo = {}
    return [memo.setdefault(s, push(rowptr, col, s, aq, eq, max_rounds)) for s in sources]


def dense_rows(rows, N, field):
    """float64 [S, N] of p (field 0) or r (field 1) / 2^48 of case_ref's rows: exact in a double"""
    out = np.zeros((len(rows), N))
    for i, row in enumerate(rows):
        for node, x in row[field].items():
            out[i, node] = x / ONE
    return out
