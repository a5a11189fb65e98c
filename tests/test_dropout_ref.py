"""CPU suite of tests/dropout_ref.py: the generator against published SplitMix64 vectors, the statistics of the
mask, a hand-worked case, and the gradient reference against CPU torch float64 autograd of the masked chain."""
import numpy as np
import pytest
import torch

import attention_ref as ar
import dropout_ref as dr

SEEDS = [0, 1, 12345, 2 ** 63 - 1]


def test_mix64_reproduces_the_published_splitmix64_vectors():
    """SplitMix64 seeded with 0 yields 0xE220A8397B1DCDAF, then 0x6E789E6AA1B965F4: mix64 of the state before
    each increment."""
    assert int(dr.mix64(0)) == 0xE220A8397B1DCDAF
    assert int(dr.mix64(0x9E3779B97F4A7C15)) == 0x6E789E6AA1B965F4
    z = np.array([0, 0x9E3779B97F4A7C15], dtype=np.uint64)
    assert dr.mix64(z).tolist() == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]
    assert int(dr.rand_stream(7, 3)) == int(dr.mix64(np.uint64(7) ^ dr.mix64(3)))


def test_threshold_zero_keeps_everything():
    assert dr.threshold(0.0) == 0 and dr.threshold(2.0 ** -25) == 0
    assert dr.threshold(0.5) == 2 ** 23 and dr.threshold(1.0 - 2.0 ** -30) == 2 ** 24 - 1
    for seed in SEEDS:
        assert dr.keep_ref(1000, 5, 0.0, seed).all()
    assert dr.inv_keep(0.5) == 2.0 and dr.inv_keep(0.0) == 1.0
    assert dr.inv_keep(0.1) == float(np.float32(1.0 / 0.9))


@pytest.mark.parametrize("dropout_p", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("seed", SEEDS)
def test_dropped_count_per_head_is_binomial(seed, dropout_p):
    nnz, H = 20000, 8
    keep = dr.keep_ref(nnz, H, dropout_p, seed)
    assert keep.shape == (nnz, H) and keep.dtype == bool
    prob = dr.threshold(dropout_p) / 2.0 ** 24
    sd = np.sqrt(nnz * prob * (1 - prob))
    z = np.abs((~keep).sum(axis=0) - nnz * prob) / sd
    print(f"seed {seed} p {dropout_p}: worst head at {z.max():.2f} standard deviations")
    assert np.all(z <= 5.0)
    # heads and seeds are different draws
    assert not np.array_equal(keep[:, 0], keep[:, 1])
    assert not np.array_equal(keep, dr.keep_ref(nnz, H, dropout_p, seed + 1))


def test_the_mask_is_a_function_of_seed_entry_and_head_only():
    big = dr.keep_ref(500, 17, 0.5, 12345)
    assert np.array_equal(dr.keep_ref(200, 3, 0.5, 12345), big[:200, :3])
    e, h = 123, 9
    r = dr.mix64(dr.rand_stream(12345, e) + np.uint64(h))
    assert bool(big[e, h]) == (int(r) >> 40 >= 2 ** 23)


def test_hand_worked_two_rows():
    """Row 0: two entries with equal scores (p = 1/2 each); row 1: one entry (p = 1).  dropout_p = 0.5: inv_keep = 2,
    so out[0] = k0 v[0] + k1 v[2] and out[1] = 2 k2 v[1] with k the keep bits."""
    rowptr, col = np.array([0, 2, 3]), np.array([0, 2, 1])
    q = np.array([[1.0, 0.0], [0.0, 1.0]])
    k = np.array([[3.0, 1.0], [5.0, 2.0], [3.0, 7.0]])
    v = np.array([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0]])
    g = np.array([[1.0, 1.0], [1.0, -1.0]])
    seen = set()
    for seed in range(40):
        kp = dr.keep_ref(3, 1, 0.5, seed)[:, 0].astype(np.float64)
        seen.add(tuple(kp))
        want = np.stack([kp[0] * v[0] + kp[1] * v[2], 2 * kp[2] * v[1]])
        assert np.array_equal(dr.attention_dropout_ref(rowptr, col, q, k, v, dropout_p=0.5, seed=seed), want)
        grads = dr.attention_dropout_grads_ref(rowptr, col, q, k, v, g, dropout_p=0.5, seed=seed)
        # grad_v[c] = p D g[row]: column 0 and 2 from row 0, column 1 from row 1
        assert np.array_equal(grads["v"], np.stack([kp[0] * g[0], 2 * kp[2] * g[1], kp[1] * g[0]]))
        dp = np.array([2 * kp[0] * 11.0, 2 * kp[1] * 44.0])
        delta = 0.5 * dp.sum()
        assert np.array_equal(grads["ds"][:2, 0], 0.5 * (dp - delta)) and grads["ds"][2, 0] == 0
    assert len(seen) > 4
    # dropout_p = 0 is the op without dropout
    assert np.array_equal(dr.attention_dropout_ref(rowptr, col, q, k, v), ar.attention_ref(rowptr, col, q, k, v))


@pytest.mark.parametrize("per_head", [None, False, True])
@pytest.mark.parametrize("dropout_p", [0.1, 0.5])
def test_gradients_agree_with_torch_autograd_of_the_masked_chain(dropout_p, per_head):
    rng = np.random.default_rng(5)
    lens = [0, 1, 3, 7, 2, 5]
    M, N, H, K, F = len(lens), 9, 3, 4, 5
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(N, size=n, replace=False)) for n in lens]).astype(np.int64)
    nnz = col.size
    q, k, v, g = (rng.normal(size=s) for s in ((M, H, K), (N, H, K), (N, H, F), (M, H, F)))
    bias = None if per_head is None else rng.normal(size=(nnz, H) if per_head else (nnz,))
    seed, scale = 12345, 0.7
    mask = dr.keep_ref(nnz, H, dropout_p, seed)
    assert 0 < mask.sum() < mask.size

    row = torch.from_numpy(ar.rows_of(rowptr))
    cl = torch.from_numpy(col)
    tq, tk, tv = (torch.from_numpy(a).requires_grad_() for a in (q, k, v))
    tb = None if bias is None else torch.from_numpy(bias).requires_grad_()
    s = scale * (tq[row] * tk[cl]).sum(-1)
    if tb is not None:
        s = s + (tb if tb.dim() == 2 else tb[:, None])
    dense = torch.full((M, N, H), float("-inf"), dtype=torch.float64)
    dense = dense.index_put((row, cl), s)
    att = torch.softmax(dense[1:], dim=1)  # row 0 has no entries
    w = att[row - 1, cl] * torch.from_numpy(mask.astype(np.float64) * dr.inv_keep(dropout_p))
    out = torch.zeros(M, H, F, dtype=torch.float64).index_add(0, row, w[:, :, None] * tv[cl])
    out.backward(torch.from_numpy(g))

    want = dr.attention_dropout_ref(rowptr, col, q, k, v, scale, bias, dropout_p, seed)
    grads = dr.attention_dropout_grads_ref(rowptr, col, q, k, v, g, scale, bias, dropout_p, seed)
    assert np.allclose(out.detach().numpy(), want, rtol=1e-12, atol=1e-12)
    for name, t in (("q", tq), ("k", tk), ("v", tv)):
        assert np.allclose(t.grad.numpy(), grads[name], rtol=1e-11, atol=1e-12), name
    if tb is not None:
        assert np.allclose(tb.grad.numpy(), grads["bias"], rtol=1e-11, atol=1e-12)
