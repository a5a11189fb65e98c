"""numpy restatements of psa_pair_intersect (csrc/intersect.hip).

A list family is a (ptr, idx, val | None) triple of numpy arrays in CSR form.  Two restatements:

  pair_intersect_math     what the op means: sorted intersection, float64 terms and sums (Python
                          integers in the counting form).
  pair_intersect_ordered  what the kernel does, operation for operation in the given dtype: the
                          shorter list probes (tie: X); a probe list of at most T elements is split over
                          GROUP lanes, a longer one over WAVE lanes, lane l taking elements l, l + W, ...;
                          a lane starts from 0 and adds (x * y) * w for its matches in probe order, each
                          multiply and add rounded on its own; the W partials are folded by the xor
                          butterfly 1, 2, 4, ...  The GPU tests hold the kernel to it bit for bit.

T, GROUP and WAVE are the kernel's constants; test_masked_spspmm_gpu.py compares them to the source.
"""
import numpy as np

T = 32      # probe lists LONGER than this are run by a whole wave
GROUP = 8   # lanes of a pair in short mode
WAVE = 64


def _list(family, i):
    ptr, idx, val = family
    if not 0 <= i < len(ptr) - 1:
        return None
    lo, hi = int(ptr[i]), int(ptr[i + 1])
    return idx[lo:hi], (None if val is None else val[lo:hi])


def pair_intersect_math(x, y, pair_x, pair_y, weight=None):
    """float64[P] (int64[P] when there are no values and no weight)."""
    counting = x[2] is None and y[2] is None and weight is None
    out = []
    for px, py in zip(np.asarray(pair_x).tolist(), np.asarray(pair_y).tolist()):
        lx, ly = _list(x, px), _list(y, py)
        if lx is None or ly is None:
            out.append(0)
            continue
        (xi, xv), (yi, yv) = lx, ly
        common, ix, iy = np.intersect1d(xi, yi, assume_unique=True, return_indices=True)
        if counting:
            out.append(len(common))
            continue
        term = np.ones(len(common), np.float64)
        if xv is not None:
            term = term * xv[ix].astype(np.float64)
        if yv is not None:
            term = term * yv[iy].astype(np.float64)
        if weight is not None:
            term = term * np.asarray(weight, np.float64)[common]
        out.append(float(np.sum(term)))
    return np.asarray(out, np.int64 if counting else np.float64).reshape(-1)


def abs_term_sum(x, y, pair_x, pair_y, weight=None):
    """(sum of |terms|, number of terms) per pair: the scale of the rounding bound n * eps * sum|terms|."""
    ax = (x[0], x[1], np.ones(len(x[1])) if x[2] is None else np.abs(x[2]))
    ay = (y[0], y[1], np.ones(len(y[1])) if y[2] is None else np.abs(y[2]))
    mag = pair_intersect_math(ax, ay, pair_x, pair_y, None if weight is None else np.abs(weight))
    cnt = pair_intersect_math((x[0], x[1], None), (y[0], y[1], None), pair_x, pair_y)
    return mag, cnt


def _ordered_pair(pidx, pval, sidx, sval, weight, dtype):
    n = len(pidx)
    W = GROUP if n <= T else WAVE
    if n == 0 or len(sidx) == 0:
        return dtype.type(0)
    pos = np.searchsorted(sidx, pidx, side="left")
    at = np.minimum(pos, len(sidx) - 1)
    hit = (pos < len(sidx)) & (sidx[at] == pidx)
    if dtype == np.int64:
        term = np.ones(n, np.int64)
    else:
        if pval is not None and sval is not None:
            term = pval * sval[at]
        elif pval is not None:
            term = pval.copy()
        elif sval is not None:
            term = sval[at]
        else:
            term = np.ones(n, dtype)
        if weight is not None:
            term = term * weight[np.where(hit, pidx, 0)]
        assert term.dtype == dtype
    steps = -(-n // W)
    term = np.concatenate([term, np.zeros(steps * W - n, dtype)]).reshape(steps, W)
    hit = np.concatenate([hit, np.zeros(steps * W - n, bool)]).reshape(steps, W)
    acc = np.zeros(W, dtype)
    for s in range(steps):  # lane l meets elements l, l + W, ... in order
        acc = np.where(hit[s], acc + term[s], acc)
    lanes = np.arange(W)
    off = 1
    while off < W:
        acc = acc + acc[lanes ^ off]
        off *= 2
    return acc[0]


def pair_intersect_ordered(x, y, pair_x, pair_y, weight=None, dtype=np.float32):
    """dtype[P] with the kernel's bits; dtype np.int64 is the counting form."""
    dtype = np.dtype(dtype)
    cast = (lambda v: None if v is None else np.ascontiguousarray(v, dtype))
    x, y, weight = (x[0], x[1], cast(x[2])), (y[0], y[1], cast(y[2])), cast(weight)
    if dtype == np.int64:
        assert x[2] is None and y[2] is None and weight is None
    out = np.zeros(len(pair_x), dtype)
    with np.errstate(all="ignore"):
        for p, (px, py) in enumerate(zip(np.asarray(pair_x).tolist(), np.asarray(pair_y).tolist())):
            lx, ly = _list(x, px), _list(y, py)
            if lx is None or ly is None:
                continue
            if len(lx[0]) <= len(ly[0]):  # the shorter list probes; X on a tie
                out[p] = _ordered_pair(lx[0], lx[1], ly[0], ly[1], weight, dtype)
            else:
                out[p] = _ordered_pair(ly[0], ly[1], lx[0], lx[1], weight, dtype)
    return out


# ---- the public functions, restated on CSR arrays -----------------------------------------------
def csc_of(rowptr, col, val, N):
    """(colptr, row in CSC order, val in CSC order) of a coalesced CSR matrix."""
    row = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    order = np.argsort(col, kind="stable")
    colptr = np.searchsorted(col[order], np.arange(N + 1), side="left").astype(np.int64)
    return colptr, row[order], (None if val is None else val[order])


def common_neighbors_ref(rowptr, col, val, u, v, weight=None):
    return pair_intersect_math((rowptr, col, val), (rowptr, col, val), u, v, weight)


def triangle_count_ref(rowptr, col):
    n = len(rowptr) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    per_edge = pair_intersect_math((rowptr, col, None), csc_of(rowptr, col, None, n), row, col)
    return np.bincount(row, weights=per_edge, minlength=n).astype(np.int64) // 2
