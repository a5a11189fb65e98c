"""float64 restatement of the attention-path ops, numpy only: segmented softmax forward and
backward (with the `perm` rule of psa_segment_softmax) and sddmm.  The GPU tests hold the
kernels to it; tests/test_softmax_ref.py holds it to hand-worked answers and to torch on the CPU.

Non-finite rule (torch.softmax on the dense row): plain IEEE arithmetic on max / exp / sum
gives it — a NaN or +inf, or nothing but -inf, makes the whole group NaN; -inf among finite
entries gives exactly 0."""
import numpy as np


def _flat(a):
    """[n, ...] -> [n, D]; an array without rows too (reshape(0, -1) cannot infer D)."""
    return a.reshape(a.shape[0], int(np.prod(a.shape[1:], dtype=np.int64)))


def _rows(n, perm):
    return np.arange(n, dtype=np.int64) if perm is None else np.asarray(perm, dtype=np.int64)


def softmax_ref(src, indptr, perm=None):
    """out[perm[j]] = softmax over segment(j) of src[perm[j]], per trailing column; float64.
    Entries outside every segment keep NaN-free zeros (the kernel leaves them unwritten)."""
    src = np.asarray(src, dtype=np.float64)
    indptr = np.asarray(indptr, dtype=np.int64)
    n = src.shape[0] if perm is None else len(perm)
    rows = _rows(n, perm)
    flat = _flat(src)
    out = np.zeros_like(flat)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for s in range(indptr.size - 1):
            r = rows[indptr[s]:indptr[s + 1]]
            if r.size == 0:
                continue
            x = flat[r]
            m = np.max(x, axis=0, keepdims=True)  # NaN propagates
            e = np.exp(x - m)
            out[r] = e / np.sum(e, axis=0, keepdims=True)
    return out.reshape(src.shape)


def softmax_bw_ref(y, g, indptr, perm=None):
    """grad_src = y * (g - sum over the segment of y * g), per trailing column; float64."""
    y = np.asarray(y, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    indptr = np.asarray(indptr, dtype=np.int64)
    n = y.shape[0] if perm is None else len(perm)
    rows = _rows(n, perm)
    fy, fg = _flat(y), _flat(g)
    out = np.zeros_like(fy)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(indptr.size - 1):
            r = rows[indptr[s]:indptr[s + 1]]
            if r.size == 0:
                continue
            dot = np.sum(fy[r] * fg[r], axis=0, keepdims=True)
            out[r] = fy[r] * (fg[r] - dot)
    return out.reshape(y.shape)


def softmax_bw_bound_terms(y, g, indptr, perm=None):
    """Per element: (segment length, |g| + sum over the segment of |y * g|) for the derived bound."""
    y = np.asarray(y, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    indptr = np.asarray(indptr, dtype=np.int64)
    n = y.shape[0] if perm is None else len(perm)
    rows = _rows(n, perm)
    fy, fg = _flat(y), _flat(g)
    length = np.zeros(fy.shape, dtype=np.float64)
    scale = np.zeros(fy.shape, dtype=np.float64)
    for s in range(indptr.size - 1):
        r = rows[indptr[s]:indptr[s + 1]]
        if r.size == 0:
            continue
        length[r] = r.size
        scale[r] = np.abs(fg[r]) + np.sum(np.abs(fy[r] * fg[r]), axis=0, keepdims=True)
    return length.reshape(y.shape), scale.reshape(y.shape)


def segment_lengths(indptr, n, perm=None, trailing=()):
    """Per element of an [n, *trailing] array: the length of the segment that holds it."""
    indptr = np.asarray(indptr, dtype=np.int64)
    rows = _rows(n, perm)
    length = np.zeros(n, dtype=np.float64)
    for s in range(indptr.size - 1):
        length[rows[indptr[s]:indptr[s + 1]]] = indptr[s + 1] - indptr[s]
    return np.broadcast_to(length.reshape((n,) + (1,) * len(trailing)), (n,) + tuple(trailing))


def sddmm_ref(rowptr, col, x, y):
    """out[e] = <x[row(e)], y[col[e]]>; float64."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    row = np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr))
    return np.einsum("ek,ek->e", x[row], y[col])
