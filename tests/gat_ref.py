"""float64 restatement of fused GAT attention, numpy only, on top of tests/attention_ref.py (rows, the softmax, the
scatter), tests/dropout_ref.py (the mask) and tests/bf16_ref.py (the once-rounded results).  The GPU tests hold the
kernels to it; tests/test_gat_ref.py holds it to a hand-worked case and to dense torch autograd on the CPU.

    z[e, h]      = (a_row[row(e), h] + a_col[col[e], h]) (+ bias[e, h] or bias[e])     (in this order)
    s[e, h]      = z where z > 0, negative_slope * z otherwise    (z == 0 and a NaN take the slope branch)
    p[e, h]      = exp(s[e, h] - m[r, h]) / l[r, h]: the softmax of s[., h] over the entries of row r
    out[r, h, :] = inv_keep * sum_{e in row r} keep(e, h) * p[e, h] * v[col[e], h, :]

and, with g = the upstream gradient of out and D = keep * inv_keep (1 without dropout),

    dP[e, h]        = D * <g[row(e), h, :], v[col[e], h, :]>
    delta[r, h]     = sum_{e in row r} p[e, h] * dP[e, h]            (= <g[r, h, :], out[r, h, :]>)
    dS[e, h]        = p * (dP - delta[row(e), h])
    dZ[e, h]        = dS * (1 where z > 0, negative_slope otherwise)
    grad_a_row[r,h] = sum_{e in row r} dZ[e, h]
    grad_a_col[c,h] = sum_{e in column c} dZ[e, h]
    grad_v[c, h, :] = sum_{e in column c} (p * D)[e, h] * g[row(e), h, :]
    grad_bias       = dZ, summed over the heads for a bias [nnz]

Operands in heads form (a_row [M, H], a_col [N, H], v [N, H, F]) or the one-head form ([M], [N], [N, F]).  Non-finite
values by plain IEEE arithmetic, as attention_ref; negative_slope == 0 against a -inf z is 0 * -inf = NaN."""
import numpy as np

import attention_ref as ar
import bf16_ref
import dropout_ref as dr


def _forms(a_row, a_col, v, *more):
    """float64, heads form, and whether the caller gave the one-head form."""
    flat = np.asarray(v).ndim == 2
    arrays = [np.asarray(a, dtype=np.float64) for a in (a_row, a_col, v) + more]
    if flat:
        arrays = [a[:, None] if i < 2 else a[:, None, :] for i, a in enumerate(arrays)]
    return arrays, flat


def z_ref(rowptr, col, a_row, a_col, bias=None):
    """z [nnz, H] from heads-form a_row, a_col."""
    col = np.asarray(col, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        z = np.asarray(a_row, dtype=np.float64)[ar.rows_of(rowptr)] + np.asarray(a_col, dtype=np.float64)[col]
        if bias is not None:
            bias = np.asarray(bias, dtype=np.float64)
            z = z + (bias[:, None] if bias.ndim == 1 else bias)
    return z


def act_ref(z, negative_slope):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(z > 0, z, float(negative_slope) * z)


def scores_ref(rowptr, col, a_row, a_col, negative_slope=0.2, bias=None):
    """s [nnz, H] from heads-form a_row, a_col."""
    return act_ref(z_ref(rowptr, col, a_row, a_col, bias), negative_slope)


def _d(nnz, H, dropout_p, seed):
    if dropout_p == 0.0:
        return np.ones((nnz, H))
    return dr.keep_ref(nnz, H, dropout_p, seed).astype(np.float64) * dr.inv_keep(dropout_p)


def gat_ref(rowptr, col, a_row, a_col, v, negative_slope=0.2, bias=None, dropout_p=0.0, seed=0):
    """out [M, H, F] ([M, F] for the one-head form)."""
    (a_row, a_col, v3), flat = _forms(a_row, a_col, v)
    col = np.asarray(col, dtype=np.int64)
    p, _, _ = ar.softmax_ref(rowptr, scores_ref(rowptr, col, a_row, a_col, negative_slope, bias))
    with np.errstate(invalid="ignore", over="ignore"):
        out = ar._scatter(ar.rows_of(rowptr), np.asarray(rowptr).size - 1, p * _d(col.size, p.shape[1], dropout_p, seed),
                          v3[col])
    return out[:, 0] if flat else out


def gat_stat_ref(rowptr, col, a_row, a_col, v, negative_slope=0.2, bias=None):
    """stat [M, H, 2] = {m, l} of the scores after the activation ([M, 2] for the one-head form)."""
    (a_row, a_col, _), flat = _forms(a_row, a_col, v)
    _, m, l = ar.softmax_ref(rowptr, scores_ref(rowptr, col, a_row, a_col, negative_slope, bias))
    stat = np.stack([m, l], axis=-1)
    return stat[:, 0] if flat else stat


def gat_grads_ref(rowptr, col, a_row, a_col, v, grad_out, negative_slope=0.2, bias=None, dropout_p=0.0, seed=0):
    """dict(a_row, a_col, v, bias, p, pd, ds, dz): the four gradients in the operands' forms (bias: None without one)
    and the per-entry p, p * D, dS and dZ [nnz, H] they are built from."""
    (a_row, a_col, v3, g3), flat = _forms(a_row, a_col, v, grad_out)
    col = np.asarray(col, dtype=np.int64)
    row = ar.rows_of(rowptr)
    M, N = a_row.shape[0], a_col.shape[0]
    z = z_ref(rowptr, col, a_row, a_col, bias)
    p, _, _ = ar.softmax_ref(rowptr, act_ref(z, negative_slope))
    D = _d(col.size, p.shape[1], dropout_p, seed)
    with np.errstate(invalid="ignore", over="ignore"):
        dp = D * np.einsum("ehf,ehf->eh", g3[row], v3[col])
        delta = np.zeros((M, p.shape[1]))
        np.add.at(delta, row, p * dp)
        ds = p * (dp - delta[row])
        dz = ds * np.where(z > 0, 1.0, float(negative_slope))
        pd = p * D
        ones = np.ones(dz.shape + (1,))
        grads = {
            "a_row": ar._scatter(row, M, dz, ones)[:, :, 0],
            "a_col": ar._scatter(col, N, dz, ones)[:, :, 0],
            "v": ar._scatter(col, N, pd, g3[row]),
            "bias": None,
            "p": p,
            "pd": pd,
            "ds": ds,
            "dz": dz,
        }
    if bias is not None:
        grads["bias"] = dz.sum(axis=1) if np.asarray(bias).ndim == 1 else dz
    if flat:
        for name in ("a_row", "a_col", "v"):
            grads[name] = grads[name][:, 0]
    return grads


def once_rounded(x):
    """The bf16 result of a float64 reference: rounded to fp32, then once to bf16."""
    return bf16_ref.round_bf16(np.asarray(x).astype(np.float32))
