"""numpy restatement of the dropout of fused sparse attention: the counter-based mask in uint64 arithmetic (bit
for bit what csrc/rng.h and csrc/attention_dropout.h compute) and the forward and the four gradients in float64,
on top of tests/attention_ref.py.

    T          = floor(dropout_p * 2^24)                      (in double)
    r(e, h)    = mix64(rand_stream(seed, e) + h)              (e = position of the entry in CSR order, h = head)
    keep(e, h) = (r(e, h) >> 40) >= T
    inv_keep   = float32(1 / (1 - dropout_p))
    out[r, h, :] = inv_keep * sum_{e in row r} keep(e, h) * p[e, h] * v[col[e], h, :]

and, with D = keep * inv_keep and g the upstream gradient,

    dP[e, h] = D * <g[row(e), h, :], v[col[e], h, :]>,  delta[r, h] = sum_e p dP (= <g, out>),  dS = p (dP - delta)
    grad_v[c, h] = sum_{e in column c} p D g[row(e), h];  grad_q, grad_k, grad_bias from dS as without dropout.

s, p and stat = {m, l} are those of attention_ref: dropout comes after the softmax.  0 * inf is NaN (no zero
skipping) and a NaN score poisons its row and head whether or not its entry is dropped."""
import math

import numpy as np

import attention_ref as ar

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def mix64(z):
    """SplitMix64's output function of z + golden ratio, elementwise on uint64 with wrap-around."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + _GOLDEN
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def rand_stream(seed, i):
    """The per-stream part: mix64(seed ^ mix64(i))."""
    return mix64(np.uint64(seed) ^ mix64(i))


def threshold(dropout_p):
    return int(math.floor(float(dropout_p) * 2.0 ** 24))


def inv_keep(dropout_p):
    return float(np.float32(1.0 / (1.0 - float(dropout_p))))


def keep_ref(nnz, H, dropout_p, seed):
    """bool [nnz, H]."""
    stream = rand_stream(seed, np.arange(nnz, dtype=np.uint64))[:, None]
    with np.errstate(over="ignore"):
        r = mix64(stream + np.arange(H, dtype=np.uint64)[None, :])
    return (r >> np.uint64(40)) >= np.uint64(threshold(dropout_p))


def _d(nnz, H, dropout_p, seed):
    return keep_ref(nnz, H, dropout_p, seed).astype(np.float64) * inv_keep(dropout_p)


def attention_dropout_ref(rowptr, col, q, k, v, scale=1.0, bias=None, dropout_p=0.0, seed=0):
    """out [M, H, F] ([M, F] for 2-D operands)."""
    flat = np.asarray(q).ndim == 2
    (v3,) = ar._heads(v)
    col = np.asarray(col, dtype=np.int64)
    p, _, _ = ar.softmax_ref(rowptr, ar.scores_ref(rowptr, col, q, k, scale, bias))
    with np.errstate(invalid="ignore", over="ignore"):
        out = ar._scatter(ar.rows_of(rowptr), np.asarray(rowptr).size - 1, p * _d(col.size, p.shape[1], dropout_p, seed),
                          v3[col])
    return out[:, 0] if flat else out


def attention_dropout_grads_ref(rowptr, col, q, k, v, grad_out, scale=1.0, bias=None, dropout_p=0.0, seed=0):
    """dict(q, k, v, bias, p, pd, ds): as attention_ref.attention_grads_ref, with pd = p * D."""
    flat = np.asarray(q).ndim == 2
    q3, k3, v3, g3 = ar._heads(q, k, v, grad_out)
    col = np.asarray(col, dtype=np.int64)
    row = ar.rows_of(rowptr)
    M, N = q3.shape[0], k3.shape[0]
    p, _, _ = ar.softmax_ref(rowptr, ar.scores_ref(rowptr, col, q, k, scale, bias))
    D = _d(col.size, p.shape[1], dropout_p, seed)
    with np.errstate(invalid="ignore", over="ignore"):
        dp = D * np.einsum("ehf,ehf->eh", g3[row], v3[col])
        delta = np.zeros((M, p.shape[1]))
        np.add.at(delta, row, p * dp)
        ds = p * (dp - delta[row])
        pd = p * D
    grads = {
        "q": float(scale) * ar._scatter(row, M, ds, k3[col]),
        "k": float(scale) * ar._scatter(col, N, ds, q3[row]),
        "v": ar._scatter(col, N, pd, g3[row]),
        "bias": None,
        "p": p,
        "pd": pd,
        "ds": ds,
    }
    if bias is not None:
        grads["bias"] = ds.sum(axis=1) if np.asarray(bias).ndim == 1 else ds
    if flat:
        for name in ("q", "k", "v"):
            grads[name] = grads[name][:, 0]
    return grads
