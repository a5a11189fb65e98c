"""GPU suite of attention dropout inside fused sparse attention (the psa_attention_*dropout* entry points behind
SparseTensor.attention(..., dropout_p, seed), ops.attention and ops.attention_dropout_mask) against
tests/dropout_ref.py: the mask bit for bit, the exact regimes of tests/test_attention_gpu.py with dropout_p = 0.5
(inv_keep = 2 is exact in any order), general values within derived bounds, the unfused chain with the same mask,
non-finite values, reproducibility and argument errors.  Shapes and helpers are those of test_attention_gpu.py."""
import numpy as np
import pytest
import torch

import attention_ref as ar
import bf16_ref
import dropout_ref as dr
from test_attention_gpu import (LENGTHS, N, U, _col_sum, bias_case, dev, host, ints, one_hot_data, one_hot_pattern,
                                pattern, same, tensor_of)

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
UB = 2.0 ** -8  # the bound for one bf16 rounding, as tests/test_attention_half_gpu.py
SEEDS = [0, 1, 12345, 2 ** 63 - 1]


@pytest.fixture(scope="module")
def big():
    return pattern(np.random.default_rng(61), LENGTHS, N)


@pytest.fixture(scope="module")
def one_hot():
    return one_hot_pattern(np.random.default_rng(71))


def same_bf(got, want):
    """The bf16 result equals the float64 reference rounded to fp32 and then once to bf16."""
    assert got.dtype == BF
    return np.array_equal(got.detach().float().cpu().numpy().astype(np.float64),
                          bf16_ref.round_bf16(want.astype(np.float32)))


def run(A, q, k, v, g, scale=1.0, bias=False, dropout_p=0.5, seed=0, dtype=torch.float32, shift=False):
    make = (lambda a: one_off(dev(a).to(dtype))) if shift else (lambda a: dev(a).to(dtype))
    qd, kd, vd = (make(a).requires_grad_() for a in (q, k, v))
    out = A.attention(qd, kd, vd, scale=scale, bias=bias, dropout_p=dropout_p, seed=seed)
    out.backward(make(g))
    return out.detach(), qd.grad, kd.grad, vd.grad


def one_off(t):
    """The same numbers in a view that starts one element into its allocation."""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = base[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size()
    return view


# ---- 1. the mask kernel ----------------------------------------------------------------------------

@pytest.mark.parametrize("dropout_p", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("H", [1, 3, 8, 17])
def test_mask_kernel_is_bit_equal_to_the_reference(H, dropout_p):
    from paddle_sparse_amd import ops

    for nnz in (0, 1, 63, 64, 65, 4099 * 3):
        for seed in SEEDS:
            got = ops.attention_dropout_mask(nnz, H, dropout_p, seed)
            assert got.shape == (nnz, H) and got.dtype == torch.bool and got.is_cuda
            assert np.array_equal(got.cpu().numpy(), dr.keep_ref(nnz, H, dropout_p, seed)), (nnz, seed)
    assert bool(ops.attention_dropout_mask(100, H, 0.0, 5).all())


# ---- 2. the dropout entry points at dropout_p = 0 --------------------------------------------------

def raw_dropout_fw(rp, cl, q, k, v, scale, dropout_p, seed):
    """psa_attention_dropout_fw / psa_attention_half_dropout_fw called directly, whatever dropout_p is."""
    from paddle_sparse_amd import _lib, ops

    lib = _lib.load()
    (M, H, K), (N_, _, F), nnz = q.shape, v.shape, cl.numel()
    out = torch.full((M, H, F), 9.0, dtype=q.dtype, device=DEV)
    stat = torch.full((M, H, 2), 9.0, device=DEV)
    nb = lib.psa_attention_workspace_bytes(nnz, H, F)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
    tail = (rp.data_ptr(), cl.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), None, 1, scale, dropout_p, seed, M,
            N_, H, K, F, nnz, out.data_ptr(), stat.data_ptr(), ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream)
    if q.dtype == torch.float32:
        status = lib.psa_attention_dropout_fw(*tail)
    else:
        status = lib.psa_attention_half_dropout_fw(ops._DTYPE_ID[q.dtype], *tail)
    return status, out, stat


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("H,K,F", [(8, 16, 16), (3, 5, 7), (65, 8, 8)])
def test_dropout_entry_points_at_zero_give_the_plain_bits(big, H, K, F, dtype):
    from paddle_sparse_amd import ops

    rowptr, col = big
    M = rowptr.size - 1
    rng = np.random.default_rng(90 + H)
    q, k, v = (dev(rng.normal(size=s).astype(np.float32)).to(dtype) for s in ((M, H, K), (N, H, K), (N, H, F)))
    rp, cl = dev(rowptr), dev(col)
    want_out, want_stat = ops.attention_raw(rp, cl, q, k, v, scale=0.25)
    status, out, stat = raw_dropout_fw(rp, cl, q, k, v, 0.25, 0.0, 12345)
    assert status == 0
    assert torch.equal(out, want_out) and torch.equal(stat, want_stat)
    # through the public op: dropout_p = 0 ignores the seed
    assert torch.equal(ops.attention(rp, cl, q, k, v, scale=0.25, dropout_p=0.0, seed=7), want_out)
    # stat does not change under dropout: it comes before it
    status, out5, stat5 = raw_dropout_fw(rp, cl, q, k, v, 0.25, 0.5, 12345)
    assert status == 0 and torch.equal(stat5, want_stat) and not torch.equal(out5, want_out)


# ---- 3. exact regime -------------------------------------------------------------------------------

# (H, K, F): 16-byte and 4-byte forms of fp32 (bf16: K, F multiples of 8 and not), more heads than four head blocks,
# a head wider than four tiles of accumulators, more slices of q than stay in registers
EXACT_SHAPES = [(1, 4, 4), (3, 5, 7), (8, 16, 16), (2, 64, 64), (65, 8, 8), (1, 3, 261), (1, 261, 3)]


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("H,K,F", EXACT_SHAPES)
def test_one_hot_exact(one_hot, H, K, F, scale, dtype):
    """The one-hot regime of test_attention_gpu.py (p is 0, 1, 1/2 or 1/4; small integers elsewhere, all bf16
    numbers) with dropout_p = 0.5: D is 0 or 2, so out and the four gradients are dyadic and must equal the float64
    reference bit for bit (bf16: rounded once).  The rows of 127 ... 4099 entries put winners on both sides of the
    128-entry chunk edge and in the first and the last chunk."""
    rowptr, col = one_hot
    M = rowptr.size - 1
    rng = np.random.default_rng(100 * H + 10 * K + F)
    q, k, v, g = one_hot_data(rng, M, H, K, F)
    seed = 12345 + H
    want = dr.attention_dropout_ref(rowptr, col, q, k, v, scale, None, 0.5, seed)
    grads = dr.attention_dropout_grads_ref(rowptr, col, q, k, v, g, scale, None, 0.5, seed)
    plain = ar.attention_ref(rowptr, col, q, k, v, scale)
    assert np.abs(want - plain).max() > 0 and np.abs(grads["ds"]).max() > 0
    eq = (lambda t, w: same(t, w, scale == 1.0)) if dtype == torch.float32 else same_bf

    A = tensor_of(rowptr, col, N)
    out, gq, gk, gv = run(A, q, k, v, g, scale, seed=seed, dtype=dtype)
    assert out.shape == (M, H, F) and out.dtype == dtype
    assert eq(out, want) and not host(out.float())[0].any()
    assert eq(gq, grads["q"]) and eq(gk, grads["k"]) and eq(gv, grads["v"])
    # operands one element off alignment
    out_o, gq_o, gk_o, gv_o = run(A, q, k, v, g, scale, seed=seed, dtype=dtype, shift=True)
    assert torch.equal(out_o, out) and torch.equal(gq_o, gq) and torch.equal(gk_o, gk) and torch.equal(gv_o, gv)


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("K,F", [(8, 8), (5, 7)])
def test_one_hot_exact_two_d_form(one_hot, K, F, dtype):
    rowptr, col = one_hot
    M = rowptr.size - 1
    rng = np.random.default_rng(200 + K)
    q, k, v, g = (a[:, 0] for a in one_hot_data(rng, M, 1, K, F))
    want = dr.attention_dropout_ref(rowptr, col, q, k, v, 1.0, None, 0.5, 1)
    grads = dr.attention_dropout_grads_ref(rowptr, col, q, k, v, g, 1.0, None, 0.5, 1)
    eq = (lambda t, w: same(t, w, True)) if dtype == torch.float32 else same_bf
    out, gq, gk, gv = run(tensor_of(rowptr, col, N), q, k, v, g, seed=1, dtype=dtype)
    assert out.shape == (M, F) and gq.shape == (M, K) and gk.shape == (N, K) and gv.shape == (N, F)
    assert eq(out, want) and eq(gq, grads["q"]) and eq(gk, grads["k"]) and eq(gv, grads["v"])


@pytest.mark.parametrize("H", [1, 3, 8])
def test_uniform_exact(H):
    """The uniform regime of test_attention_gpu.py (p = 1 / length, lengths powers of two) with dropout_p = 0.5."""
    rng = np.random.default_rng(72 + H)
    lens = [1, 2, 4, 8, 16, 32, 64, 128, 256, 0, 4, 2, 256, 1]
    M, n, K, F = len(lens), 300, 4, 8
    rowptr, col = pattern(rng, lens, n)
    q = ints(rng, (M, H, K), -2, 2)
    k = np.tile(ints(rng, (1, H, K), -2, 2), (n, 1, 1))
    v, g = ints(rng, (n, H, F), -2, 2), ints(rng, (M, H, F), -2, 2)
    want = dr.attention_dropout_ref(rowptr, col, q, k, v, 1.0, None, 0.5, 12345)
    grads = dr.attention_dropout_grads_ref(rowptr, col, q, k, v, g, 1.0, None, 0.5, 12345)
    out, gq, gk, gv = run(tensor_of(rowptr, col, n), q, k, v, g, seed=12345)
    assert same(out, want, True) and not host(out)[9].any()
    assert same(gq, grads["q"], True) and same(gk, grads["k"], True) and same(gv, grads["v"], True)


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("per_head", [False, True])
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_bias_makes_the_winners_exact(big, per_head, scale, dtype):
    rowptr, col = big
    H = 3
    q, k, v, g, bias = bias_case(np.random.default_rng(73), rowptr, col, H, -2048.0, per_head)
    want = dr.attention_dropout_ref(rowptr, col, q, k, v, scale, bias, 0.5, 2 ** 63 - 1)
    grads = dr.attention_dropout_grads_ref(rowptr, col, q, k, v, g, scale, bias, 0.5, 2 ** 63 - 1)
    assert np.abs(grads["bias"]).max() > 0
    eq = (lambda t, w: same(t, w, True)) if dtype == torch.float32 else same_bf
    bd = dev(bias).requires_grad_()
    out, gq, gk, gv = run(tensor_of(rowptr, col, N, bd), q, k, v, g, scale, bias=True, seed=2 ** 63 - 1, dtype=dtype)
    assert eq(out, want) and eq(gq, grads["q"]) and eq(gk, grads["k"]) and eq(gv, grads["v"])
    assert bd.grad.dtype == torch.float32 and bd.grad.shape == bias.shape and same(bd.grad, grads["bias"], True)


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_rows_across_the_chunk_edge(dtype):
    """One row each of 127, 128, 129, 257 and 4099 entries, the bias making winners at the first and last entry and
    at entries 127 and 128: the combine's inv_keep and the chunk kernels' entry index."""
    rng = np.random.default_rng(81)
    rowptr, col = pattern(rng, [127, 128, 129, 257, 4099], N)
    q, k, v, g, bias = bias_case(rng, rowptr, col, 3, -2048.0, True)
    eq = (lambda t, w: same(t, w, True)) if dtype == torch.float32 else same_bf
    differ = 0
    for seed in SEEDS:
        want = dr.attention_dropout_ref(rowptr, col, q, k, v, 1.0, bias, 0.5, seed)
        grads = dr.attention_dropout_grads_ref(rowptr, col, q, k, v, g, 1.0, bias, 0.5, seed)
        out, gq, gk, gv = run(tensor_of(rowptr, col, N, dev(bias)), q, k, v, g, bias=True, seed=seed, dtype=dtype)
        assert eq(out, want) and eq(gq, grads["q"]) and eq(gk, grads["k"]) and eq(gv, grads["v"])
        differ += int(np.abs(want - ar.attention_ref(rowptr, col, q, k, v, 1.0, bias)).max() > 0)
    assert differ == len(SEEDS)


def test_same_mask_across_dtypes(one_hot):
    """v > 0, so a (row, head) of the one-hot regime is exactly 0 only where every winner was dropped (and in the
    row without entries): the same set in fp32, in bf16 and in the reference."""
    rowptr, col = one_hot
    M, H, K, F = rowptr.size - 1, 8, 8, 8
    rng = np.random.default_rng(82)
    q, k, _, _ = one_hot_data(rng, M, H, K, F)
    v = ints(rng, (N, H, F), 1, 2)
    A = tensor_of(rowptr, col, N)
    seen = 0
    for seed in SEEDS:
        want = dr.attention_dropout_ref(rowptr, col, q, k, v, 1.0, None, 0.5, seed)
        zero = (want == 0).all(axis=2)
        z32 = (A.attention(dev(q), dev(k), dev(v), dropout_p=0.5, seed=seed) == 0).all(dim=2).cpu().numpy()
        z16 = (A.attention(dev(q).to(BF), dev(k).to(BF), dev(v).to(BF), dropout_p=0.5, seed=seed) == 0).all(dim=2)
        assert np.array_equal(z32, zero) and np.array_equal(z16.cpu().numpy(), zero)
        seen += int(zero[1:].sum())
    assert seen > 8  # single winners were dropped somewhere


# ---- 4. general values -----------------------------------------------------------------------------

def general_case(rowptr, col, H, K, F, dropout_p, seed, half):
    """Inputs, references and bounds.  The bounds are those of test_general_values_within_the_derived_bounds
    (fp32: tests/test_attention_gpu.py; bf16: tests/test_attention_half_gpu.py adds ub |result| per rounded result
    and ub sum_f |g out| in delta), with D = keep * inv_keep (inv_keep is the same float32 number on both sides) and
    the roundings of the added multiplies:

    out.     inv_keep * (acc / l) with acc over the kept entries: the weights' relative error eps on sum_e D p |v|,
             and one more rounding, the multiply by inv_keep: (eps + u) sum_e D p |v|.
    grad_v.  p D is one more multiply: sum_{e in col} (eps + u + (clen + 2) u) p D |g|.
    dP.      D * dot is one more multiply: D_dP = (F + 3) u D sum_f |g v|.
    delta.   <g, out^> with the bound of out above.
    dS, grad_q, grad_k: the same expressions on these terms."""
    M = rowptr.size - 1
    row = ar.rows_of(rowptr)
    rng = np.random.default_rng(75 + H)
    q, k, v, g = (rng.normal(size=s).astype(np.float32) for s in ((M, H, K), (N, H, K), (N, H, F), (M, H, F)))
    if half:
        q, k, v, g = (bf16_ref.round_bf16(a).astype(np.float32) for a in (q, k, v, g))
    scale = float(np.float32(1.0 / np.sqrt(K)))
    want = dr.attention_dropout_ref(rowptr, col, q, k, v, scale, None, dropout_p, seed)
    grads = dr.attention_dropout_grads_ref(rowptr, col, q, k, v, g, scale, None, dropout_p, seed)
    p, pd, ds = grads["p"], grads["pd"], grads["ds"]
    D = dr.keep_ref(col.size, H, dropout_p, seed) * dr.inv_keep(dropout_p)
    q64, k64, v64, g64 = (a.astype(np.float64) for a in (q, k, v, g))
    ub = UB if half else 0.0

    length = np.diff(rowptr).astype(np.float64)
    clen = np.bincount(col, minlength=N).astype(np.float64)
    abs_qk = np.einsum("ehk,ehk->eh", np.abs(q64[row]), np.abs(k64[col]))
    Delta = np.zeros((M, H))
    np.maximum.at(Delta, row, (K + 2) * U * scale * abs_qk)
    eps = 2 * Delta + (length[:, None] + 64) * U
    pv = np.zeros((M, H, F))
    np.add.at(pv, row, pd[:, :, None] * np.abs(v64[col]))                         # sum_e D p |v|
    f_out = (eps + U)[:, :, None] * pv
    b_out = f_out + ub * np.abs(want)
    b_gv = _col_sum(col, N, ((eps[row] + U + (clen[col, None] + 2) * U) * pd)[:, :, None] * np.abs(g64[row])) + \
        ub * np.abs(grads["v"])
    dp = D * np.einsum("ehf,ehf->eh", g64[row], v64[col])
    delta = np.einsum("mhf,mhf->mh", g64, want)
    g_out = np.einsum("mhf,mhf->mh", np.abs(g64), np.abs(want))
    d_dp = (F + 3) * U * D * np.einsum("ehf,ehf->eh", np.abs(g64[row]), np.abs(v64[col]))
    d_delta = (F + 2) * U * g_out + np.einsum("mhf,mhf->mh", np.abs(g64), f_out) + ub * g_out
    d_ds = eps[row] * p * np.abs(dp - delta[row]) + p * (d_dp + d_delta[row]) + \
        4 * U * p * (np.abs(dp) + np.abs(delta[row]))
    b_gq = np.zeros((M, H, K))
    np.add.at(b_gq, row, scale * (d_ds + (length[row, None] + 3) * U * np.abs(ds))[:, :, None] * np.abs(k64[col]))
    b_gq += ub * np.abs(grads["q"])
    b_gk = _col_sum(col, N, scale * (d_ds + (clen[col, None] + 3) * U * np.abs(ds))[:, :, None] * np.abs(q64[row])) + \
        ub * np.abs(grads["k"])
    # the chain softmax(sddmm * scale) * mask * inv_keep -> spmm_heads, fp32: the same eps on the weights, one rounding
    # for the multiply by inv_keep and a sum of len products
    b_chain = (eps + U + (length[:, None] + 2) * U)[:, :, None] * pv
    return (q, k, v, g, scale), (want, grads["q"], grads["k"], grads["v"]), (b_out, b_gq, b_gk, b_gv), b_chain


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("dropout_p", [0.1, 0.5])
@pytest.mark.parametrize("H,K,F", [(1, 64, 64), (8, 16, 16), (3, 5, 7)])
def test_general_values_within_the_derived_bounds(big, H, K, F, dropout_p, dtype):
    rowptr, col = big
    (q, k, v, g, scale), wants, bounds, _ = general_case(rowptr, col, H, K, F, dropout_p, 12345, dtype == BF)
    got = run(tensor_of(rowptr, col, N), q, k, v, g, scale, dropout_p=dropout_p, seed=12345, dtype=dtype)
    ratios = [float(np.max(np.abs(host(t.float()) - w) / np.maximum(b, 1e-300))) for t, w, b in zip(got, wants, bounds)]
    print(f"attention dropout {dropout_p} {dtype} ({H}, {K}, {F}): worst err / bound  out {ratios[0]:.4f}  grad_q "
          f"{ratios[1]:.4f}  grad_k {ratios[2]:.4f}  grad_v {ratios[3]:.4f}")
    for t, w, b in zip(got, wants, bounds):
        assert np.all(np.abs(host(t.float()) - w) <= b)


@pytest.mark.parametrize("dropout_p", [0.1, 0.5])
@pytest.mark.parametrize("H,K,F", [(8, 16, 16), (3, 5, 7)])
def test_equivalence_with_the_chain_on_the_device(big, H, K, F, dropout_p):
    """The chain with the mask of ops.attention_dropout_mask: e is the CSR position the public ops see."""
    from paddle_sparse_amd import ops

    rowptr, col = big
    (q, k, v, g, scale), wants, bounds, b_chain = general_case(rowptr, col, H, K, F, dropout_p, 1, False)
    rp, cl = dev(rowptr), dev(col)
    fused = ops.attention(rp, cl, dev(q), dev(k), dev(v), scale=scale, dropout_p=dropout_p, seed=1)
    mask = ops.attention_dropout_mask(col.size, H, dropout_p, 1)
    att = ops.segment_softmax(ops.sddmm(rp, cl, dev(q), dev(k)) * scale, rp)
    chain = ops.spmm_heads(rp, cl, att * mask * dr.inv_keep(dropout_p), dev(v))
    diff = np.abs(host(fused) - host(chain))
    print(f"fused vs chain, dropout {dropout_p} ({H}, {K}, {F}): worst diff / bound "
          f"{float(np.max(diff / np.maximum(bounds[0] + b_chain, 1e-300))):.4f}")
    assert np.all(diff <= bounds[0] + b_chain)
    assert np.all(np.abs(host(chain) - wants[0]) <= b_chain)


# ---- 5. non-finite values --------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_non_finite_values(big, dtype):
    rowptr, col = big
    M, nnz = rowptr.size - 1, col.size
    H, K, F = 3, 8, 8
    seed = 12345
    rng = np.random.default_rng(76)
    q, k, v = (bf16_ref.round_bf16(rng.normal(size=s).astype(np.float32)).astype(np.float32)
               for s in ((M, H, K), (N, H, K), (N, H, F)))
    keep = dr.keep_ref(nnz, H, 0.5, seed)
    row = ar.rows_of(rowptr)
    A = tensor_of(rowptr, col, N)

    def fused(q, k, v):
        return host(A.attention(dev(q).to(dtype), dev(k).to(dtype), dev(v).to(dtype), dropout_p=0.5, seed=seed).float())

    base = fused(q, k, v)
    assert np.isfinite(base).all() and not base[0].any()  # the row without entries gives 0
    # a dropped entry against an inf in v: NaN in the rows and heads that drop it, inf where it is kept, that feature only
    e, h = int(np.flatnonzero(~keep[rowptr[10]:rowptr[11], 1])[0] + rowptr[10]), 1
    c = int(col[e])
    v2 = v.copy()
    v2[c, h, 5] = np.inf
    got = fused(q, k, v2)
    assert np.isnan(got[10, h, 5])
    touched = np.zeros((M, H, F), dtype=bool)
    touched[row[col == c], h, 5] = True
    assert np.array_equal(~np.isfinite(got), touched)
    assert np.array_equal(np.isnan(got)[:, h, 5], np.bincount(row[(col == c) & ~keep[:, h]], minlength=M) > 0)
    # a NaN score poisons its row and head whether its entry is dropped or kept
    for want_kept in (False, True):
        at = int(np.flatnonzero(keep[rowptr[12]:rowptr[13], 2] == want_kept)[0] + rowptr[12])
        bias = np.zeros((nnz, H), dtype=np.float32)
        bias[at, 2] = np.nan
        B = tensor_of(rowptr, col, N, dev(bias))
        got = host(B.attention(dev(q).to(dtype), dev(k).to(dtype), dev(v).to(dtype), bias=True, dropout_p=0.5,
                               seed=seed).float())
        bad = np.zeros((M, H), dtype=bool)
        bad[12, 2] = True
        assert np.array_equal(np.isnan(got).all(axis=2), bad) and np.array_equal(np.isnan(got).any(axis=2), bad)
    # a row with every entry dropped is exactly 0 when v is finite
    heads = [int(hh) for hh in range(H)]
    dropped = [(r, hh) for r in range(1, M) for hh in heads if not keep[rowptr[r]:rowptr[r + 1], hh].any()]
    assert dropped, "rows 1 and 2 (one and two entries) over three heads: some are dropped under this seed"
    for r, hh in dropped:
        assert not base[r, hh].any()
    want = dr.attention_dropout_ref(rowptr, col, q, k, v, 1.0, None, 0.5, seed)
    assert np.array_equal((base == 0).all(axis=2), (want == 0).all(axis=2))


# ---- 6. reproducibility ----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_seeds_runs_and_a_captured_graph(big, dtype):
    from paddle_sparse_amd import ops

    rowptr, col = big
    M = rowptr.size - 1
    H, K, F = 8, 16, 16
    rng = np.random.default_rng(79)

    def normal(*shape):
        return dev(rng.normal(size=shape).astype(np.float32)).to(dtype)

    q, k, v, g = normal(M, H, K), normal(N, H, K), normal(N, H, F), normal(M, H, F)
    A = tensor_of(rowptr, col, N)
    st = A.storage
    rp, cl = st.rowptr(), st.col()
    csc = (st.colptr(), st._row_in_csc_order(), st.csr2csc())

    def autograd_step(seed):
        qd, kd, vd = (t.detach().requires_grad_() for t in (q, k, v))
        out = A.attention(qd, kd, vd, scale=0.25, dropout_p=0.5, seed=seed)
        out.backward(g)
        return out.detach(), qd.grad, kd.grad, vd.grad

    first, second, other = autograd_step(7), autograd_step(7), autograd_step(8)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert not torch.equal(first[0], other[0])

    def step():
        out, stat = ops.attention_raw(rp, cl, q, k, v, None, 0.25, dropout_p=0.5, seed=7)
        return (out,) + ops.attention_bw(rp, cl, q, k, v, None, 0.25, g, out, stat, csc, dropout_p=0.5, seed=7)[:3]

    for a, b in zip(first, step()):
        assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # the workspaces are in the allocator before the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for t in (q, k, v, g):
        t.copy_(normal(*t.shape))
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(captured, step()):
        assert torch.equal(got, want)


def test_the_backward_uses_the_forwards_mask(one_hot):
    """Exact regime: the gradients equal the reference under the forward's seed and under no other."""
    rowptr, col = one_hot
    M, H, K, F = rowptr.size - 1, 3, 5, 7
    q, k, v, g = one_hot_data(np.random.default_rng(83), M, H, K, F)
    got = run(tensor_of(rowptr, col, N), q, k, v, g, seed=12345)
    for seed, match in ((12345, True), (12346, False), (0, False)):
        grads = dr.attention_dropout_grads_ref(rowptr, col, q, k, v, g, 1.0, None, 0.5, seed)
        assert same(got[3], grads["v"], True) == match
        assert (same(got[1], grads["q"], True) and same(got[2], grads["k"], True)) == match


def test_seed_none_draws_from_the_cpu_generator(big):
    rowptr, col = big
    M, H, K, F = rowptr.size - 1, 2, 4, 4
    rng = np.random.default_rng(84)
    q, k, v = (dev(rng.normal(size=s).astype(np.float32)) for s in ((M, H, K), (N, H, K), (N, H, F)))
    A = tensor_of(rowptr, col, N)

    def pair():
        torch.manual_seed(1234)
        return A.attention(q, k, v, dropout_p=0.5), A.attention(q, k, v, dropout_p=0.5)

    a1, a2 = pair()
    b1, b2 = pair()
    assert not torch.equal(a1, a2) and torch.equal(a1, b1) and torch.equal(a2, b2)
    # the backward sees the forward's draw
    qd = q.clone().requires_grad_()
    torch.manual_seed(1234)
    out = A.attention(qd, k, v, dropout_p=0.5)
    assert torch.equal(out.detach(), a1)
    torch.manual_seed(99)  # the generator moving on between forward and backward changes nothing
    out.sum().backward()
    assert bool(torch.isfinite(qd.grad).all())


def test_nothing_with_nnz_rows_is_saved(big):
    rowptr, col = big
    M, nnz = rowptr.size - 1, col.size
    H, K, F = 8, 16, 16
    assert nnz not in (M, N, H, K, F, 2)
    rng = np.random.default_rng(78)
    qd, kd, vd = (dev(rng.normal(size=s).astype(np.float32)).requires_grad_() for s in ((M, H, K), (N, H, K), (N, H, F)))
    saved = []

    def pack(t):
        saved.append(tuple(t.shape))
        return t

    A = tensor_of(rowptr, col, N)
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = A.attention(qd, kd, vd, scale=0.25, dropout_p=0.1, seed=3)
    assert len(saved) >= 5  # q, k, v, out, stat
    assert all(nnz not in shape for shape in saved), saved
    out.sum().backward()
    assert qd.grad is not None and kd.grad is not None and vd.grad is not None


# ---- 7. argument errors ----------------------------------------------------------------------------

def test_errors():
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import _lib, ops

    H, K, F = 2, 4, 3
    row, col = torch.tensor([0, 1], device=DEV), torch.tensor([1, 2], device=DEV)
    A = psa.SparseTensor(row=row, col=col, sparse_sizes=(2, 3))
    q, k, v = torch.zeros(2, H, K, device=DEV), torch.zeros(3, H, K, device=DEV), torch.ones(3, H, F, device=DEV)
    rowptr = torch.tensor([0, 1, 2], device=DEV)
    assert A.attention(q, k, v, dropout_p=0.5, seed=0).shape == (2, H, F)
    assert A.attention(q, k, v, dropout_p=0, seed="ignored at 0").shape == (2, H, F)
    for bad in (-0.1, 1.0, float("nan"), "0.5"):
        with pytest.raises(ValueError):
            A.attention(q, k, v, dropout_p=bad, seed=0)
        with pytest.raises(ValueError):
            ops.attention(rowptr, col, q, k, v, dropout_p=bad, seed=0)
        with pytest.raises(ValueError):
            ops.attention_dropout_mask(4, H, bad, 0)
    for bad, err in ((-1, ValueError), (2 ** 64, ValueError), (1.0, TypeError)):
        with pytest.raises(err):
            A.attention(q, k, v, dropout_p=0.5, seed=bad)
        with pytest.raises(err):
            ops.attention(rowptr, col, q, k, v, dropout_p=0.5, seed=bad)
        with pytest.raises(err):
            ops.attention_dropout_mask(4, H, 0.5, bad)
    assert A.attention(q, k, v, dropout_p=0.5, seed=2 ** 64 - 1).shape == (2, H, F)
    # the C-ABI
    status, _, _ = raw_dropout_fw(rowptr, col, q, k, v, 1.0, 1.0, 0)
    assert status == 1 and b"dropout_p" in _lib.load().psa_last_error()  # PSA_ERR_INVALID_ARG
    for p in (-0.5, float("nan")):
        assert raw_dropout_fw(rowptr, col, q.to(BF), k.to(BF), v.to(BF), 1.0, p, 0)[0] == 1
    assert _lib.load().psa_attention_dropout_mask(4, H, 1.0, 0, None, None) == 1
