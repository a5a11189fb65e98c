"""float64 restatement of fused sparse attention, numpy only: the forward and the four gradients in
closed form.  The GPU tests hold the kernels to it; tests/test_attention_ref.py holds it to a
hand-worked case and to dense torch.softmax autograd on the CPU.

    s[e, h]      = scale * <q[row(e), h, :], k[col[e], h, :]> (+ bias[e, h] or bias[e])
    p[e, h]      = exp(s[e, h] - m[r, h]) / l[r, h]: the softmax of s[., h] over the entries of row r
    out[r, h, :] = sum_{e in row r} p[e, h] * v[col[e], h, :]

and, with g = the upstream gradient of out,

    dP[e, h]     = <g[row(e), h, :], v[col[e], h, :]>
    delta[r, h]  = sum_{e in row r} p[e, h] * dP[e, h]            (= <g[r, h, :], out[r, h, :]>)
    dS[e, h]     = p[e, h] * (dP[e, h] - delta[row(e), h])
    grad_q[r, h] = scale * sum_{e in row r} dS[e, h] * k[col[e], h]
    grad_k[c, h] = scale * sum_{e in column c} dS[e, h] * q[row(e), h]
    grad_v[c, h] = sum_{e in column c} p[e, h] * g[row(e), h]
    grad_bias    = dS, summed over the heads for a bias [nnz]

Operands in heads form (q [M, H, K], k [N, H, K], v [N, H, F]) or 2-D (one head).  Non-finite values by
plain IEEE arithmetic: the maximum drops a NaN but exp(NaN - m) poisons the sum, +inf gives inf - inf, a
row of nothing but -inf gives -inf - -inf: NaN throughout that row and head; -inf among finite scores
gives exactly 0; no zero skipping (0 * inf = NaN).  A row without entries gives out = 0, stat = {-inf, 0}."""
import numpy as np


def rows_of(rowptr):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    return np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr))


def _heads(*arrays):
    """float64, heads form."""
    out = [np.asarray(a, dtype=np.float64) for a in arrays]
    return [a[:, None, :] if a.ndim == 2 else a for a in out]


def _scatter(index, n, weight, dense):
    """out[index[e], h, :] += weight[e, h] * dense[e, h, :]."""
    out = np.zeros((n,) + dense.shape[1:], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(out, index, weight[:, :, None] * dense)
    return out


def scores_ref(rowptr, col, q, k, scale=1.0, bias=None):
    """s [nnz, H]."""
    q, k = _heads(q, k)
    col = np.asarray(col, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = float(scale) * np.einsum("ehk,ehk->eh", q[rows_of(rowptr)], k[col])
        if bias is not None:
            bias = np.asarray(bias, dtype=np.float64)
            s = s + (bias[:, None] if bias.ndim == 1 else bias)
    return s


def softmax_ref(rowptr, s):
    """(p [nnz, H], m [M, H], l [M, H]) of scores s [nnz, H]."""
    row = rows_of(rowptr)
    M = np.asarray(rowptr).size - 1
    m = np.full((M, s.shape[1]), -np.inf)
    np.fmax.at(m, row, s)  # drops a NaN, as fmaxf does
    l = np.zeros_like(m)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = np.exp(s - m[row])
        np.add.at(l, row, e)
        p = e / l[row]
    return p, m, l


def attention_ref(rowptr, col, q, k, v, scale=1.0, bias=None):
    """out [M, H, F] ([M, F] for 2-D operands)."""
    flat = np.asarray(q).ndim == 2
    (v3,) = _heads(v)
    p, _, _ = softmax_ref(rowptr, scores_ref(rowptr, col, q, k, scale, bias))
    out = _scatter(rows_of(rowptr), np.asarray(rowptr).size - 1, p, v3[np.asarray(col, dtype=np.int64)])
    return out[:, 0] if flat else out


def attention_stat_ref(rowptr, col, q, k, scale=1.0, bias=None):
    """stat [M, H, 2] = {m, l}."""
    _, m, l = softmax_ref(rowptr, scores_ref(rowptr, col, q, k, scale, bias))
    return np.stack([m, l], axis=-1)


def attention_grads_ref(rowptr, col, q, k, v, grad_out, scale=1.0, bias=None):
    """dict(q, k, v, bias, p, ds): the four gradients in the operands' forms (bias: None without one) and the
    per-entry p and dS [nnz, H] they are built from."""
    flat = np.asarray(q).ndim == 2
    q3, k3, v3, g3 = _heads(q, k, v, grad_out)
    col = np.asarray(col, dtype=np.int64)
    row = rows_of(rowptr)
    M, N = q3.shape[0], k3.shape[0]
    p, _, _ = softmax_ref(rowptr, scores_ref(rowptr, col, q, k, scale, bias))
    with np.errstate(invalid="ignore", over="ignore"):
        dp = np.einsum("ehf,ehf->eh", g3[row], v3[col])
        delta = np.zeros((M, p.shape[1]))
        np.add.at(delta, row, p * dp)
        ds = p * (dp - delta[row])
    grads = {
        "q": float(scale) * _scatter(row, M, ds, k3[col]),
        "k": float(scale) * _scatter(col, N, ds, q3[row]),
        "v": _scatter(col, N, p, g3[row]),
        "bias": None,
        "p": p,
        "ds": ds,
    }
    if bias is not None:
        grads["bias"] = ds.sum(axis=1) if np.asarray(bias).ndim == 1 else ds
    if flat:
        for name in ("q", "k", "v"):
            grads[name] = grads[name][:, 0]
    return grads
