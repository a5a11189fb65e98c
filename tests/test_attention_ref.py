"""CPU suite: tests/attention_ref.py (the float64 restatement the GPU tests of fused attention use) against a
hand-worked case and against dense torch.softmax float64 autograd with the missing entries at -inf."""
import numpy as np
import pytest
import torch

import attention_ref as ar


def pattern(rng, lens, n):
    cols = [np.sort(rng.choice(n, size=ln, replace=False)) for ln in lens]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rowptr, np.concatenate(cols).astype(np.int64)


def test_hand_worked_case():
    """Two rows over three columns, one head, K = 1, F = 2.
    Row 0 holds columns 0 and 2 with scores ln 1 and ln 3: p = 1/4, 3/4.  Row 1 holds column 1 alone: p = 1."""
    rowptr, col = np.array([0, 2, 3]), np.array([0, 2, 1])
    q = np.array([[1.0], [2.0]])
    k = np.array([[0.0], [5.0], [np.log(3.0)]])
    v = np.array([[4.0, 8.0], [1.0, -1.0], [0.0, 4.0]])
    out = ar.attention_ref(rowptr, col, q, k, v)
    assert np.allclose(out, [[1.0, 5.0], [1.0, -1.0]], rtol=0, atol=1e-15)
    stat = ar.attention_stat_ref(rowptr, col, q, k)
    assert np.allclose(stat[:, 0, 0], [np.log(3.0), 10.0]) and np.allclose(stat[:, 0, 1], [4.0 / 3.0, 1.0])
    # g = [[1, 0], [0, 1]]: dP = 4, 0 (row 0) and -1 (row 1); delta = 1 and -1; dS = 1/4 * 3, 3/4 * -1, 0
    g = np.array([[1.0, 0.0], [0.0, 1.0]])
    grads = ar.attention_grads_ref(rowptr, col, q, k, v, g)
    assert np.allclose(grads["ds"][:, 0], [0.75, -0.75, 0.0], rtol=0, atol=1e-15)
    assert np.allclose(grads["q"], [[0.75 * 0.0 - 0.75 * np.log(3.0)], [0.0]], rtol=0, atol=1e-15)
    assert np.allclose(grads["k"], [[0.75], [0.0], [-0.75]], rtol=0, atol=1e-15)
    assert np.allclose(grads["v"], [[0.25, 0.0], [0.0, 1.0], [0.75, 0.0]], rtol=0, atol=1e-15)
    # scale and a bias: scale 2 with bias -s gives equal scores again
    s = ar.scores_ref(rowptr, col, q, k)
    assert np.allclose(ar.attention_ref(rowptr, col, q, k, v, scale=2.0, bias=-s[:, 0]), out, rtol=0, atol=1e-15)


def dense_autograd(rowptr, col, q, k, v, g, scale, bias):
    """Dense float64 torch: missing entries at -inf; the row without entries at 0, so that no NaN enters the
    dense backward (as test_multi_head_attention_step_exact builds it)."""
    M, N, H = q.shape[0], k.shape[0], q.shape[1]
    row = ar.rows_of(rowptr)
    qt, kt, vt = (torch.from_numpy(a.astype(np.float64)).requires_grad_() for a in (q, k, v))
    mask = torch.zeros(M, N, dtype=torch.bool)
    mask[torch.from_numpy(row), torch.from_numpy(col)] = True
    mask = mask[:, :, None]
    fill = torch.where(mask.any(1, keepdim=True), torch.tensor(float("-inf"), dtype=torch.float64),
                       torch.tensor(0.0, dtype=torch.float64))
    scores = scale * torch.einsum("mhk,nhk->mnh", qt, kt)
    bt = None
    if bias is not None:
        bt = torch.from_numpy(bias.astype(np.float64)).requires_grad_()
        dense_b = torch.zeros(M, N, H, dtype=torch.float64)
        dense_b = dense_b.index_put((torch.from_numpy(row), torch.from_numpy(col)),
                                    bt[:, None].expand(-1, H) if bt.dim() == 1 else bt)
        scores = scores + dense_b
    scores = torch.where(mask, scores, fill.expand(M, N, H))
    att = torch.softmax(scores, dim=1)
    att = torch.where(mask, att, torch.zeros_like(att))
    out = torch.einsum("mnh,nhf->mhf", att, vt)
    out.backward(torch.from_numpy(g.astype(np.float64)))
    return out.detach().numpy(), qt.grad.numpy(), kt.grad.numpy(), vt.grad.numpy(), None if bt is None else bt.grad.numpy()


@pytest.mark.parametrize("bias_form", [None, "shared", "heads"])
@pytest.mark.parametrize("scale", [1.0, 0.25])
def test_against_dense_float64_autograd(bias_form, scale):
    rng = np.random.default_rng(7)
    lens = [3, 0, 1, 17, 40, 2]
    M, N, H, K, F = len(lens), 40, 3, 5, 4
    rowptr, col = pattern(rng, lens, N)
    q, k, v = rng.normal(size=(M, H, K)), rng.normal(size=(N, H, K)), rng.normal(size=(N, H, F))
    g = rng.normal(size=(M, H, F))
    bias = {None: None, "shared": rng.normal(size=col.size), "heads": rng.normal(size=(col.size, H))}[bias_form]
    want = dense_autograd(rowptr, col, q, k, v, g, scale, bias)
    out = ar.attention_ref(rowptr, col, q, k, v, scale, bias)
    grads = ar.attention_grads_ref(rowptr, col, q, k, v, g, scale, bias)
    tol = dict(rtol=1e-12, atol=1e-12)
    assert np.allclose(out, want[0], **tol) and not out[1].any()
    assert np.allclose(grads["q"], want[1], **tol) and np.allclose(grads["k"], want[2], **tol)
    assert np.allclose(grads["v"], want[3], **tol)
    if bias is None:
        assert grads["bias"] is None
    else:
        assert grads["bias"].shape == bias.shape and np.allclose(grads["bias"], want[4], **tol)
    # delta in its other closed form
    row = ar.rows_of(rowptr)
    delta = np.zeros((M, H))
    np.add.at(delta, row, grads["p"] * np.einsum("ehf,ehf->eh", g[row], v[col]))
    assert np.allclose(delta, np.einsum("mhf,mhf->mh", g, out), **tol)


def test_two_d_form_is_one_head():
    rng = np.random.default_rng(8)
    rowptr, col = pattern(rng, [2, 5, 0, 9], 12)
    q, k, v, g = rng.normal(size=(4, 6)), rng.normal(size=(12, 6)), rng.normal(size=(12, 3)), rng.normal(size=(4, 3))
    out = ar.attention_ref(rowptr, col, q, k, v, 0.5)
    assert out.shape == (4, 3)
    assert np.array_equal(out, ar.attention_ref(rowptr, col, q[:, None], k[:, None], v[:, None], 0.5)[:, 0])
    grads = ar.attention_grads_ref(rowptr, col, q, k, v, g, 0.5)
    heads = ar.attention_grads_ref(rowptr, col, q[:, None], k[:, None], v[:, None], g[:, None], 0.5)
    for name in ("q", "k", "v"):
        assert grads[name].shape == {"q": q, "k": k, "v": v}[name].shape
        assert np.array_equal(grads[name], heads[name][:, 0])


def test_non_finite_rule():
    rowptr, col = np.array([0, 3, 6, 9, 9, 12]), np.array([0, 1, 2] * 4)
    q = np.ones((5, 1, 1))
    k = np.array([1.0, 2.0, 3.0]).reshape(3, 1, 1)
    v = np.ones((3, 1, 2))
    bias = np.zeros(12)
    bias[1] = -np.inf      # row 0: a mask among finite scores
    bias[3:6] = -np.inf    # row 1: nothing but -inf
    bias[7] = np.nan       # row 2
    bias[10] = np.inf      # row 4
    out = ar.attention_ref(rowptr, col, q, k, v, bias=bias)
    stat = ar.attention_stat_ref(rowptr, col, q, k, bias=bias)
    assert np.isfinite(out[0]).all() and np.isnan(out[1]).all() and np.isnan(out[2]).all() and np.isnan(out[4]).all()
    assert not out[3].any() and stat[3, 0, 0] == -np.inf and stat[3, 0, 1] == 0.0
    e1, e3 = np.exp(-2.0), 1.0
    assert np.allclose(out[0], 1.0) and np.isclose(stat[0, 0, 1], e1 + e3) and stat[0, 0, 0] == 3.0
    v[1] = np.inf  # weight 0 against an inf: NaN
    assert np.isnan(ar.attention_ref(rowptr, col, q, k, v, bias=bias)[0]).all()
