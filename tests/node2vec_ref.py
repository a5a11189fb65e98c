"""The node2vec (p, q) walk restated serially in Python on numpy arrays (csrc/node2vec_step.h,
csrc/node2vec.hip), built on weighted_ref's mix64, pick and row_cdf, with the graphs and the
case table that the CPU suite (host export) and the GPU suite (kernel) both run.  Both compare
bit for bit with ref_node2vec_walk; tests/test_zz_node2vec_ref.py pins it to hand-checked
answers.  Not a test module."""
import functools
import math

import numpy as np

import weighted_ref as wr

ONE = 1 << 53
M64 = wr.M64


def bias(p, q):
    """((thr0, thr1, thr2), max_tries) for the return parameter p and the in-out parameter q."""
    a = (1.0 / p, 1.0, 1.0 / q)
    hi, lo = max(a), min(a)
    return tuple(int(x / hi * 2.0 ** 53) for x in a), 32 * math.ceil(hi / lo)


def ref_node2vec_walk(rowptr, col, cum, start, L, seed, thr, max_tries, stats=None):
    """(nodes int64[S, L + 1], e_id int64[S, L]).  cum None: uniform proposals.  stats, a dict,
    gets the number of steps that drew ("steps") and of tries they made ("tries") added."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    start = np.asarray(start, np.int64)
    S = start.size
    nodes, eids = np.empty((S, L + 1), np.int64), np.empty((S, L), np.int64)
    steps = tries = 0
    for n in range(S):
        stream = wr.mix64((seed & M64) ^ wr.mix64(n))
        v, t = int(start[n]), -1
        nodes[n, 0] = v
        for l in range(L):
            s, end = int(rowptr[v]), int(rowptr[v + 1])
            deg = end - s
            e, x = -1, v
            if deg > 0 and (cum is None or cum[end - 1] > 0):
                steps += 1
                for j in range(max_tries):
                    tries += 1
                    c = (stream + l + (j << 32)) & M64
                    r = wr.mix64(c)
                    e = s + ((r * deg) >> 64 if cum is None else wr.pick(cum[s:end], r))
                    x = int(col[e])
                    if l == 0:
                        break
                    if x == t:
                        k = 0
                    else:
                        row_t = col[rowptr[t]:rowptr[t + 1]]
                        i = int(np.searchsorted(row_t, x, side="left"))
                        k = 1 if i < len(row_t) and row_t[i] == x else 2
                    if (wr.mix64((c + (1 << 63)) & M64) >> 11) < thr[k]:
                        break
            t, v = v, x
            nodes[n, l + 1] = v
            eids[n, l] = e
    if stats is not None:
        stats["steps"] = stats.get("steps", 0) + steps
        stats["tries"] = stats.get("tries", 0) + tries
    return nodes, eids


def sorted_csr(row, col, N):
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    order = np.lexsort((col, row))
    return np.searchsorted(row[order], np.arange(N + 1), side="left").astype(np.int64), col[order]


# ---- small graphs with answers that need no random number ------------------------------------
def path_graph(n=10):
    """The symmetric path 0 - 1 - ... - (n - 1)."""
    a = np.arange(n - 1)
    return sorted_csr(np.concatenate([a, a + 1]), np.concatenate([a + 1, a]), n)


KITE_EDGES = ((0, 1, 1.0), (0, 2, 2.0), (1, 2, 3.0), (2, 3, 0.5), (3, 4, 1.0))  # (u, v, weight of both entries)
KITE_WALKS = 1 << 15


def kite_graph():
    """(rowptr, col, w): symmetric edges 0-1, 0-2, 1-2, 2-3, 3-4.  From 2, having come from 0,
    node 0 is the way back, 1 is a neighbour of 0 and 3 is neither."""
    u, v, w = (np.array(x) for x in zip(*KITE_EDGES))
    row, col, w = np.concatenate([u, v]), np.concatenate([v, u]), np.concatenate([w, w])
    order = np.lexsort((col, row))
    rowptr, scol = sorted_csr(row, col, 5)
    return rowptr, scol, w[order].astype(np.float64)


def kite_sigmas(nodes, p, q, weighted):
    """Largest |count - n pi| / sigma over the third nodes 0, 1, 3 of the walks 0 -> 2 -> ?, and n."""
    third = nodes[nodes[:, 1] == 2, 2]
    n = len(third)
    pi = np.array([1 / p, 1.0, 1 / q]) * (np.array([2.0, 3.0, 0.5]) if weighted else 1.0)
    pi = pi / pi.sum()
    counts = np.array([(third == x).sum() for x in (0, 1, 3)])
    assert counts.sum() == n
    return float((np.abs(counts - n * pi) / np.sqrt(n * pi * (1 - pi))).max()), n


KITE_CASES = ((0.25, 4, False, 7), (4, 0.25, False, 11), (2, 1, False, 7), (1, 0.5, False, 11),
              (0.25, 4, True, 7))  # (p, q, weighted, seed)


# ---- the case table ------------------------------------------------------------------------------
DEGS = (0, 1, 2, 7, 8, 9, 63, 64, 65)
DENSE = 297  # nodes 0 .. 296 carry DEGS in turn; node 297 is the hub; the rest are its leaves
HUB, HUB_DEG, N_NODES = 297, 5000, 5298
ZERO_ROW = 7  # its weights are all zero


@functools.lru_cache(maxsize=None)
def case_graph(symmetric):
    """(rowptr, col, w float32, cum float64), read-only.  About 300 nodes with rows of DEGS
    entries in turn, drawn with repeats from themselves and the hub; a self loop on every fifth
    of them; a hub of 5000 distinct columns; leaves with one entry or none.  symmetric: every
    entry also stored the other way round (duplicates kept).  30 % of the weights are zero, and
    all of row ZERO_ROW."""
    rng = np.random.default_rng(12)
    rows, cols = [], []
    for i in range(DENSE):
        c = rng.integers(0, HUB + 1, DEGS[i % len(DEGS)])
        if i % 5 == 0 and len(c):
            c[0] = i
        rows.append(np.full(len(c), i))
        cols.append(c)
    rows.append(np.full(HUB_DEG, HUB))
    cols.append(np.sort(rng.choice(N_NODES, HUB_DEG, replace=False)))
    leaves = np.arange(HUB + 1, N_NODES)
    leaves = leaves[leaves % 3 != 0]
    rows.append(leaves)
    cols.append(rng.integers(0, HUB + 1, len(leaves)))
    row, col = np.concatenate(rows), np.concatenate(cols)
    if symmetric:
        row, col = np.concatenate([row, col]), np.concatenate([col, row])
    rowptr, col = sorted_csr(row, col, N_NODES)
    w = rng.random(len(col), dtype=np.float32)
    w[rng.random(len(col)) < 0.3] = 0
    w[rowptr[ZERO_ROW]:rowptr[ZERO_ROW + 1]] = 0
    cum = wr.row_cdf(rowptr, w.astype(np.float64))
    for a in (rowptr, col, w, cum):
        a.setflags(write=False)
    return rowptr, col, w, cum


SIZES = (1, 63, 64, 65, 257, 2 * N_NODES)  # lane, wave and workgroup tails; every node twice
LENGTHS = (0, 1, 2, 15, 16, 17, 40)  # around the bursts of 8 and 16 stores
PQS = ((0.25, 4), (4, 0.25), (2, 1), (1, 0.5), (1, 1), (1 / 32, 32))
MODES = ("uniform", "weighted", "cdf")  # weighted=True and a reused EdgeCDF draw the same walks


def _cases():
    """(symmetric, S, L, (p, q), mode, edge ids): every S with every L (every node twice only
    up to L = 2), the other columns dealt round so that every pair of their values meets.
    (1/32, 32) needs about a thousand tries per step where the way back is not stored, too many
    for the restatement: on the directed graph it runs once, for one walk."""
    out = []
    for S in SIZES:
        for L in LENGTHS:
            if S == SIZES[-1] and L > 2:
                continue
            k = len(out)
            pq = PQS[k % 6]
            symmetric = S > 1 if pq == PQS[5] else (k // 2) % 2 == 0
            out.append((symmetric, S, L, pq, MODES[(k // 6 + k) % 3], (k // 6) % 2 == 0))
    return tuple(out)


CASES = _cases()
CASE_SEED = 2**63 + 11  # a seed with the top bit set


def case_start(S):
    if S == SIZES[-1]:
        return np.tile(np.arange(N_NODES), 2)
    start = np.random.default_rng(S).integers(0, HUB + 1, S)
    start[0] = HUB
    return start


@functools.lru_cache(maxsize=None)
def case_ref(k):
    """(nodes, e_id) of CASES[k], computed once per process."""
    symmetric, S, L, pq, mode, _ = CASES[k]
    rowptr, col, _, cum = case_graph(symmetric)
    thr, max_tries = bias(*pq)  # (1, 1) too: the public call would not reach the new kernel with it
    nodes, e_id = ref_node2vec_walk(rowptr, col, None if mode == "uniform" else cum, case_start(S), L, CASE_SEED + k,
                                    thr, max_tries)
    nodes.setflags(write=False)
    e_id.setflags(write=False)
    return nodes, e_id
