"""The edge-weighted samplers restated in numpy (csrc/weighted.hip, csrc/weighted_pick.h):
the row CDF, the pick, the weighted walk with its edge ids and the weighted sample_adj.
The GPU suite compares the kernels with these bit for bit; tests/test_weighted_ref.py pins
them to hand-checked answers.  Not a test module."""
import numpy as np

M64 = (1 << 64) - 1
U64 = np.uint64


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def word(seed, i, t):
    """The random word of draw t of stream i (csrc/rng.h): what rand_draw turns into an index."""
    return mix64((mix64((seed & M64) ^ mix64(i & M64)) + t) & M64)


def mix64_np(z):
    z = z + U64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def row_cdf(rowptr, w):
    """np.cumsum of every row's float64 weights: sequential, left to right."""
    rowptr, w = np.asarray(rowptr, np.int64), np.asarray(w, np.float64)
    cum = np.empty_like(w)
    for s, t in zip(rowptr[:-1].tolist(), rowptr[1:].tolist()):
        if t > s:
            cum[s:t] = np.cumsum(w[s:t])
    return cum


def pick(cum_row, r):
    """Index picked in one row's cum by the random word r, or -1 for no pick."""
    cum_row = np.asarray(cum_row, np.float64)
    deg = len(cum_row)
    if deg == 0:
        return -1
    total = cum_row[-1]
    if not total > 0:
        return -1
    u = np.float64(r >> 11) * np.float64(2.0 ** -53)
    target = u * total  # one rounded multiply
    e = int(np.searchsorted(cum_row, target, side="right"))  # smallest e with cum[e] > target
    if e < deg:
        return e
    return min(int(np.searchsorted(cum_row, total, side="left")), deg - 1)  # smallest e with cum[e] == total


def _picks_np(cum, s, deg, r):
    """pick() for arrays of rows [s, s + deg) and words r: -1 for no pick.  Binary search
    over all rows at once; any search finds the same index in a non-decreasing row."""
    has = deg > 0
    total = np.where(has, cum[np.where(has, s + deg - 1, 0)], 0.0) if cum.size else np.zeros(len(s))
    ok = has & (total > 0)
    u = (r >> U64(11)).astype(np.float64) * np.float64(2.0 ** -53)
    target = u * total

    def first(pred_value, strict):
        lo, hi = np.zeros_like(s), np.where(ok, deg, 0)
        while True:
            live = lo < hi
            if not live.any():
                return lo
            mid = lo + ((hi - lo) >> 1)
            c = cum[np.where(live, s + mid, 0)]
            right = (c > pred_value) if strict else (c >= pred_value)
            hi = np.where(live & right, mid, hi)
            lo = np.where(live & ~right, mid + 1, lo)

    e = first(target, True)
    none = ok & (e >= deg)
    if none.any():
        e = np.where(none, np.minimum(first(total, False), deg - 1), e)
    return np.where(ok, e, -1)


def ref_weighted_walk(rowptr, col, cum, start, L, seed):
    """(nodes int64[S, L + 1], e_id int64[S, L]) of the weighted walk; cum None: the uniform
    draw of random_walk."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    cur = np.asarray(start, np.int64).copy()
    S = cur.size
    nodes, eids = np.empty((S, L + 1), np.int64), np.empty((S, L), np.int64)
    nodes[:, 0] = cur
    with np.errstate(over="ignore"):
        stream = mix64_np(U64(seed & M64) ^ mix64_np(np.arange(S, dtype=U64)))
        for l in range(L):
            s = rowptr[cur]
            deg = rowptr[cur + 1] - s
            r = mix64_np(stream + U64(l))
            if cum is None:
                d = deg.astype(U64)
                p = ((r >> U64(32)) * d + (((r & U64(0xFFFFFFFF)) * d) >> U64(32))) >> U64(32)  # degrees < 2^32
                p = np.where(deg > 0, p.astype(np.int64), -1)
            else:
                p = _picks_np(cum, s, deg, r)
            e = np.where(p >= 0, s + p, -1)
            cur = np.where(e >= 0, col[np.where(e >= 0, e, 0)], cur) if col.size else cur
            nodes[:, l + 1] = cur
            eids[:, l] = e
    return nodes, eids


def ref_weighted_select(rowptr, col, cum, idx, k, seed):
    """Weighted sample_adj with replacement (k >= 0) or of every entry (k < 0), through the
    whole chain: (n_id, out_rowptr, out_col, e_id).  Subset nodes keep their position in idx
    (the last one for a duplicate); other picked columns are numbered in order of their first
    slot; a row's picks are sorted by new column id, equal ids in draw order."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    idx = [int(v) for v in idx]
    slots = []
    for i, n in enumerate(idx):
        s, deg = int(rowptr[n]), int(rowptr[n + 1] - rowptr[n])
        if k < 0:
            slots.append(list(range(s, s + deg)))
        elif deg > 0 and cum[s + deg - 1] > 0:
            slots.append([s + pick(cum[s:s + deg], word(seed, i, t)) for t in range(k)])
        else:
            slots.append([])
    newid = {n: i for i, n in enumerate(idx)}
    n_id = list(idx)
    for es in slots:
        for e in es:
            c = int(col[e])
            if c not in newid:
                newid[c] = len(n_id)
                n_id.append(c)
    out_rowptr, out_col, e_id = [0], [], []
    for es in slots:
        es = sorted(es, key=lambda e: newid[int(col[e])])  # stable
        out_col += [newid[int(col[e])] for e in es]
        e_id += es
        out_rowptr.append(len(e_id))
    return (np.array(n_id, np.int64), np.array(out_rowptr, np.int64), np.array(out_col, np.int64),
            np.array(e_id, np.int64))


def star(weights):
    """(rowptr, col, w) of a star: node 0 holds one entry to leaf j + 1 of weight weights[j];
    the leaves have no entries."""
    K = len(weights)
    rowptr = np.concatenate([[0], np.full(K + 1, K)]).astype(np.int64)
    return rowptr, np.arange(1, K + 1, dtype=np.int64), np.asarray(weights, np.float64)


def star_bounds(counts, weights, S):
    """(largest |count - S p| / sigma over the leaves of positive weight, chi^2 over them)."""
    w = np.asarray(weights, np.float64)
    p = w / w.sum()
    pos = w > 0
    mean = S * p[pos]
    dev = np.abs(np.asarray(counts, np.float64)[pos] - mean)
    return float((dev / np.sqrt(S * p[pos] * (1 - p[pos]))).max()), float((dev ** 2 / mean).sum())
