"""CPU checks of tests/gat_ref.py, the float64 restatement the GPU suite of fused GAT attention is held to: a
hand-worked case, dense torch autograd on a small random pattern, and the presence of the four entry points in
the header and the binding table."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import attention_ref as ar
import dropout_ref as dr
import gat_ref as gr

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("psa_gat_attention_fw", "psa_gat_attention_bw_entries", "psa_gat_attention_half_fw",
           "psa_gat_attention_half_bw_entries")


def test_hand_worked_case():
    """Three rows over three columns, one head, negative_slope = 1/2:

        row 0: columns 0, 2    a_row = 1     a_col = (1, 5, -3)
        row 1: column 1        a_row = -3
        row 2: no entries

    z = (2, -2 | 2), s = (2, -1 | 2).  Row 0: m = 2, l = 1 + e^-3, p = (p0, p1) = (1, e^-3) / l =
    (0.95257412682243..., 0.04742587317756...); row 1: p = 1.  With v = ((1, 0), (0, 2), (3, -1)):
    out = ((p0 + 3 p1, -p1), (0, 2), (0, 0)).  With g = ((1, 1), (1, 0), (5, 5)): dP = (1, 2 | 0), delta =
    (p0 + 2 p1, 0) = (1 + p1, 0), dS = (-p0 p1, p0 p1 | 0), and the factors (1, 1/2 | 1) give
    dZ = (-p0 p1, p0 p1 / 2 | 0) with p0 p1 = 0.04517665973091..."""
    rowptr, col = np.array([0, 2, 3, 3]), np.array([0, 2, 1])
    a_row, a_col = np.array([1.0, -3.0, 7.0]), np.array([1.0, 5.0, -3.0])
    v = np.array([[1.0, 0.0], [0.0, 2.0], [3.0, -1.0]])
    g = np.array([[1.0, 1.0], [1.0, 0.0], [5.0, 5.0]])
    p0, p1, pp = 0.9525741268224334, 0.04742587317756679, 0.045176659730912144
    assert math.isclose(p0, 1 / (1 + math.exp(-3)), rel_tol=1e-15) and math.isclose(p0 + p1, 1.0, rel_tol=1e-15)
    assert math.isclose(pp, p0 * p1, rel_tol=1e-15)

    assert np.array_equal(gr.z_ref(rowptr, col, a_row[:, None], a_col[:, None])[:, 0], [2.0, -2.0, 2.0])
    assert np.array_equal(gr.scores_ref(rowptr, col, a_row[:, None], a_col[:, None], 0.5)[:, 0], [2.0, -1.0, 2.0])
    out = gr.gat_ref(rowptr, col, a_row, a_col, v, 0.5)
    assert out.shape == (3, 2)
    assert np.allclose(out, [[p0 + 3 * p1, -p1], [0.0, 2.0], [0.0, 0.0]], rtol=1e-15, atol=0)
    stat = gr.gat_stat_ref(rowptr, col, a_row, a_col, v, 0.5)
    assert stat.shape == (3, 2)
    assert np.allclose(stat[:2], [[2.0, 1.0497870683678638], [2.0, 1.0]], rtol=1e-15, atol=0)
    assert stat[2, 0] == -np.inf and stat[2, 1] == 0.0
    grads = gr.gat_grads_ref(rowptr, col, a_row, a_col, v, g, 0.5)
    assert np.allclose(grads["p"][:, 0], [p0, p1, 1.0], rtol=1e-15, atol=0)
    assert np.allclose(grads["ds"][:, 0], [-pp, pp, 0.0], rtol=1e-13, atol=1e-17)
    assert np.allclose(grads["dz"][:, 0], [-pp, pp / 2, 0.0], rtol=1e-13, atol=1e-17)
    assert np.allclose(grads["a_row"], [-pp / 2, 0.0, 0.0], rtol=1e-13, atol=1e-17)
    assert np.allclose(grads["a_col"], [-pp, 0.0, pp / 2], rtol=1e-13, atol=1e-17)
    assert np.allclose(grads["v"], [[p0, p0], [1.0, 0.0], [p1, p1]], rtol=1e-15, atol=0)
    assert grads["bias"] is None

    # z == 0 takes the slope: a_col[2] = -1 makes the second score of row 0 zero
    a_col0 = np.array([1.0, 5.0, -1.0])
    g0 = gr.gat_grads_ref(rowptr, col, a_row, a_col0, v, g, 0.5)
    assert g0["dz"][1, 0] == g0["ds"][1, 0] / 2 and g0["ds"][1, 0] != 0
    # a bias [nnz] goes inside the activation, and its gradient is dZ summed over the one head
    gb = gr.gat_grads_ref(rowptr, col, a_row, a_col - np.array([0.0, 0.0, 1.0]), v, g, 0.5,
                          bias=np.array([0.0, 1.0, 0.0]))
    assert np.array_equal(gb["dz"], grads["dz"]) and np.array_equal(gb["bias"], grads["dz"][:, 0])
    # negative_slope = 0 against a -inf bias: 0 * -inf = NaN in its row and head only
    masked = gr.gat_ref(rowptr, col, a_row, a_col, v, 0.0, bias=np.array([0.0, -np.inf, 0.0]))
    assert np.isnan(masked[0]).all() and np.array_equal(masked[1:], out[1:])
    assert np.array_equal(gr.gat_ref(rowptr, col, a_row, a_col, v, 0.5, bias=np.array([0.0, -np.inf, 0.0]))[0], v[0])


def _dense(rowptr, col, a_row, a_col, v, slope, bias, D):
    """out through dense torch ops: softmax over the columns of the activated scores, -inf off the pattern."""
    M, N = a_row.shape[0], a_col.shape[0]
    row = torch.from_numpy(ar.rows_of(rowptr))
    colt = torch.from_numpy(col)
    H = a_row.shape[1]
    on = torch.zeros(M, N, dtype=torch.bool)
    on[row, colt] = True
    z = a_row[:, None, :] + a_col[None, :, :]
    if bias is not None:
        b = torch.zeros(M, N, H, dtype=torch.float64)
        b[row, colt] = bias if bias.dim() == 2 else bias[:, None].expand(-1, H)
        z = z + b
    s = torch.nn.functional.leaky_relu(z, slope)
    s = torch.where(on[:, :, None], s, torch.full_like(s, float("-inf")))
    p = torch.softmax(s, dim=1)
    if D is not None:
        d = torch.zeros(M, N, H, dtype=torch.float64)
        d[row, colt] = torch.from_numpy(D)
        p = p * d
    return torch.einsum("mnh,nhf->mhf", p, v)


@pytest.mark.parametrize("dropout_p", [0.0, 0.5])
@pytest.mark.parametrize("bias_form", ["none", "shared", "per_head"])
@pytest.mark.parametrize("slope", [0.2, -0.5, 0.0])
def test_reference_against_dense_torch_autograd(slope, bias_form, dropout_p):
    rng = np.random.default_rng(5)
    M, N, H, F = 7, 9, 3, 4
    lens = [1, 9, 3, 2, 5, 1, 4]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(N, size=ln, replace=False)) for ln in lens]).astype(np.int64)
    nnz = col.size
    a_row, a_col, v, g = (rng.normal(size=s) for s in ((M, H), (N, H), (N, H, F), (M, H, F)))
    bias = {"none": None, "shared": rng.normal(size=nnz), "per_head": rng.normal(size=(nnz, H))}[bias_form]
    D = None if dropout_p == 0.0 else dr.keep_ref(nnz, H, dropout_p, 11) * dr.inv_keep(dropout_p)

    leaves = [torch.from_numpy(a).requires_grad_() for a in (a_row, a_col, v)]
    bt = None if bias is None else torch.from_numpy(bias).requires_grad_()
    out = _dense(rowptr, col, *leaves, slope, bt, D)
    out.backward(torch.from_numpy(g))

    want = gr.gat_ref(rowptr, col, a_row, a_col, v, slope, bias, dropout_p, 11)
    grads = gr.gat_grads_ref(rowptr, col, a_row, a_col, v, g, slope, bias, dropout_p, 11)
    assert np.allclose(out.detach().numpy(), want, rtol=1e-12, atol=1e-14)
    for leaf, name in zip(leaves, ("a_row", "a_col", "v")):
        assert np.allclose(leaf.grad.numpy(), grads[name], rtol=1e-11, atol=1e-13), name
    if bias is not None:
        assert grads["bias"].shape == bias.shape
        assert np.allclose(bt.grad.numpy(), grads["bias"], rtol=1e-11, atol=1e-13)
    # the one-head form is head 0 of the heads form (the mask of head 0 does not depend on H)
    flat = gr.gat_grads_ref(rowptr, col, a_row[:, 0], a_col[:, 0], v[:, 0], g[:, 0], slope,
                            None if bias is None else (bias if bias.ndim == 1 else bias[:, 0]), dropout_p, 11)
    assert flat["a_row"].shape == (M,) and np.array_equal(flat["a_row"], grads["a_row"][:, 0])
    assert flat["v"].shape == (N, F) and np.array_equal(flat["v"], grads["v"][:, 0])


def test_the_entry_points_are_declared_and_bound():
    from paddle_sparse_amd import _lib

    header = (ROOT / "include" / "paddle_sparse_hip.h").read_text()
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.SIGNATURES, name
    fw, bw = _lib.SIGNATURES[SYMBOLS[0]][1], _lib.SIGNATURES[SYMBOLS[1]][1]
    assert len(bw) == len(fw) + 3  # grad_out, out, stat in; (out, stat) and (p, dz) pair off
    for plain, half in ((SYMBOLS[0], SYMBOLS[2]), (SYMBOLS[1], SYMBOLS[3])):
        assert len(_lib.SIGNATURES[half][1]) == len(_lib.SIGNATURES[plain][1]) + 1  # the dtype in front
