"""GPU suite of fused sparse attention (psa_attention_fw / psa_attention_bw_entries behind
SparseTensor.attention and ops.attention) against the float64 restatement of tests/attention_ref.py.

Exact wherever it says so.  Two regimes make the softmax a dyadic rational, so that the fp32 results must
equal the float64 reference bit for bit whatever the order of the additions, the online rescales and the
chunk merges:
  * one-hot: per row and head 1, 2 or 4 "winner" entries share the largest score and every other score is
    at least 512 below it, so exp underflows to exactly 0 in fp32 and p is 0 or 2^-j;
  * uniform: identical rows in k, so the scores of a row are equal, with row lengths that are powers of two.
Everything else is a small integer, so every sum stays within 24 bits."""
import numpy as np
import pytest
import torch

import attention_ref as ar

pytestmark = pytest.mark.gpu

DEV = "cuda"
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1024, 4099]
N = 4200
U = 2.0 ** -24
# (H, K, F): the smallest; the smallest 16-byte form; a 4-byte form with nothing a power of two; the bench widths;
# K != F both ways; one pass of two slices and two tiles; a head block of 5 with K >> F; more heads than one
# head block (16); K wider than the wave
SHAPES = [(1, 1, 1), (1, 4, 4), (3, 5, 7), (8, 16, 16), (8, 8, 32), (2, 64, 64), (5, 64, 4), (65, 4, 4), (2, 200, 12)]


def pattern(rng, lens, n):
    """Sorted CSR pattern with the given row lengths, distinct columns inside a row."""
    cols = [np.sort(rng.choice(n, size=ln, replace=False)) for ln in lens]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rowptr, np.concatenate(cols).astype(np.int64) if cols else np.zeros(0, dtype=np.int64)


def ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def dev(a):
    return torch.from_numpy(a).to(DEV)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def offset_copy(t):
    """The same numbers in a view that starts 4 bytes into its allocation."""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = base[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def tensor_of(rowptr, col, n, value=None):
    import paddle_sparse_amd as psa

    return psa.SparseTensor(rowptr=dev(rowptr), col=dev(col), value=value, sparse_sizes=(rowptr.size - 1, n),
                            is_sorted=True)


@pytest.fixture(scope="module")
def big():
    rowptr, col = pattern(np.random.default_rng(61), LENGTHS, N)
    return rowptr, col


def run(A, q, k, v, g, scale=1.0, bias=False):
    """out and the gradients of q, k, v (and of the tracked values of A) through the tensor form."""
    qd, kd, vd = (dev(a).requires_grad_() for a in (q, k, v))
    out = A.attention(qd, kd, vd, scale=scale, bias=bias)
    out.backward(dev(g))
    return out.detach(), qd.grad, kd.grad, vd.grad


def same(got, want, exact64):
    """Bit for bit: got (fp32) equals the float64 reference, or the reference rounded to fp32 where the
    reference holds terms below fp32's range (see test_one_hot_exact)."""
    got = host(got)
    return np.array_equal(got, want) if exact64 else np.array_equal(got, want.astype(np.float32).astype(np.float64))


# ---- 1. exact, one-hot regime ----------------------------------------------------------------------

W_ALL = [0, 1, 2100, 2101, N - 2, N - 1]   # winner columns of the even heads
W_ODD = [0, 2100, N - 1]                   # ... of the odd heads: a subset that leaves every row 1 or 2 of them


def one_hot_pattern(rng):
    """Rows of LENGTHS whose winner columns (a subset of W_ALL per row) sit where the kernel can go wrong: the
    first entry, the last entry, entries 127 and 128 (either side of the chunk edge), the first and the last
    chunk of the longest row, and 4 winners.  Every other column of a row is drawn from the loser columns.
    Per row the winners number 1, 2 or 4 under W_ALL and 1 or 2 under W_ODD."""
    losers = np.setdiff1d(np.arange(N), W_ALL)
    lo_part = losers[losers < 2100]
    winners = {1: [2100], 2: [0, N - 1], 63: [0], 64: [N - 1], 65: [0, N - 1], 127: [2100], 128: [2100, 2101],
               129: [2100, 2101], 255: [0, 1, N - 2, N - 1], 256: [2100, 2101], 257: [0, N - 1],
               1024: [0, 1, 2100, 2101], 4099: [0, N - 1]}
    cols, where = [], {}
    for ln in LENGTHS:
        if ln == 0:
            cols.append(np.zeros(0, dtype=np.int64))
            continue
        w = winners[ln]
        if ln in (129, 256):  # exactly 127 losers below column 2100: the winners are entries 127 and 128
            below = rng.choice(lo_part, size=127, replace=False)
            above = rng.choice(losers[losers > 2101], size=ln - 129, replace=False)
            c = np.concatenate([below, above, w])
        else:
            c = np.concatenate([rng.choice(losers, size=ln - len(w), replace=False), w])
        c = np.sort(c).astype(np.int64)
        cols.append(c)
        where[ln] = [int(np.searchsorted(c, x)) for x in w]
    assert where[129] == [127, 128] and where[256] == [127, 128] and where[63] == [0] and where[64] == [63]
    assert where[4099] == [0, 4098] and where[257] == [0, 256]  # two winners in different chunks
    rowptr = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    return rowptr, np.concatenate(cols)


@pytest.fixture(scope="module")
def one_hot():
    return one_hot_pattern(np.random.default_rng(71))


def one_hot_data(rng, M, H, K, F):
    q = ints(rng, (M, H, K), -3, 3)
    q[:, :, 0] = 32
    k = np.zeros((N, H, K), dtype=np.float32)
    k[:, :, 0] = ints(rng, (N, H), -32, 0)
    for h in range(H):
        k[W_ALL if h % 2 == 0 else W_ODD, h, 0] = 32
    return q, k, ints(rng, (N, H, F), -2, 2), ints(rng, (M, H, F), -2, 2)


@pytest.mark.parametrize("scale", [1.0, 0.5])
# the last two: one head wider than four tiles of accumulators, and more slices of q than stay in registers
@pytest.mark.parametrize("H,K,F", SHAPES + [(1, 3, 261), (1, 261, 3)])
def test_one_hot_exact(one_hot, H, K, F, scale):
    """Winners score scale * 1024, losers scale * 32 * k0 <= 0: at least 512 apart.  fp32 exp(-512) is exactly 0,
    so p is 0 or 1 / (number of winners) on the GPU.  At scale = 1 the gap is 1024 and the float64 reference
    underflows to exactly 0 as well: the comparison is on the float64 values.  At scale = 0.5 the reference keeps
    exp(-512) ~ 1e-223 on the losers, which no fp32 number can hold: there the reference is rounded to fp32
    first (the correctly rounded result), which is what "bit for bit" can mean for an fp32 output."""
    rowptr, col = one_hot
    M = rowptr.size - 1
    rng = np.random.default_rng(100 * H + 10 * K + F)
    q, k, v, g = one_hot_data(rng, M, H, K, F)
    p = ar.softmax_ref(rowptr, ar.scores_ref(rowptr, col, q, k, scale))[0]
    assert set(np.unique(np.round(p[p > 1e-100], 12))) <= {1.0, 0.5, 0.25} and (p > 1e-100).sum() > H * 13
    want = ar.attention_ref(rowptr, col, q, k, v, scale)
    grads = ar.attention_grads_ref(rowptr, col, q, k, v, g, scale)
    assert np.abs(grads["ds"]).max() > 0  # two winners with different dP somewhere
    x64 = scale == 1.0

    A = tensor_of(rowptr, col, N)
    out, gq, gk, gv = run(A, q, k, v, g, scale)
    assert out.shape == (M, H, F) and out.dtype == torch.float32
    assert same(out, want, x64) and not host(out)[0].any()
    assert same(gq, grads["q"], x64) and same(gk, grads["k"], x64) and same(gv, grads["v"], x64)

    # operands that start 4 bytes into an allocation, without autograd
    out_o = A.attention(offset_copy(dev(q)), offset_copy(dev(k)), offset_copy(dev(v)), scale=scale)
    assert torch.equal(out_o, out)


@pytest.mark.parametrize("K,F", [(4, 4), (5, 7), (64, 64)])
def test_one_hot_exact_two_d_form(one_hot, K, F):
    rowptr, col = one_hot
    M = rowptr.size - 1
    rng = np.random.default_rng(200 + K)
    q, k, v, g = (a[:, 0] for a in one_hot_data(rng, M, 1, K, F))
    want = ar.attention_ref(rowptr, col, q, k, v)
    grads = ar.attention_grads_ref(rowptr, col, q, k, v, g)
    A = tensor_of(rowptr, col, N)
    out, gq, gk, gv = run(A, q, k, v, g)
    assert out.shape == (M, F) and gq.shape == (M, K) and gk.shape == (N, K) and gv.shape == (N, F)
    assert same(out, want, True) and same(gq, grads["q"], True) and same(gk, grads["k"], True)
    assert same(gv, grads["v"], True)
    heads = A.attention(dev(q)[:, None], dev(k)[:, None], dev(v)[:, None])
    assert torch.equal(heads[:, 0], out)


# ---- 2. exact, uniform regime ----------------------------------------------------------------------

@pytest.mark.parametrize("H", [1, 3, 8])
def test_uniform_exact(H):
    """k identical across nodes per head: equal scores within a row and head, row lengths the powers of two
    1 .. 256 plus an empty row, integers in [-2, 2] (the ranges of test_multi_head_attention_step_exact): p is
    1 / length, every sum stays within 24 bits, and grad_q = scale * k * sum(dS) is exactly 0."""
    rng = np.random.default_rng(72 + H)
    lens = [1, 2, 4, 8, 16, 32, 64, 128, 256, 0, 4, 2, 256, 1]
    M, n, K, F = len(lens), 300, 4, 8
    rowptr, col = pattern(rng, lens, n)
    q = ints(rng, (M, H, K), -2, 2)
    k = np.tile(ints(rng, (1, H, K), -2, 2), (n, 1, 1))
    v, g = ints(rng, (n, H, F), -2, 2), ints(rng, (M, H, F), -2, 2)
    want = ar.attention_ref(rowptr, col, q, k, v)
    grads = ar.attention_grads_ref(rowptr, col, q, k, v, g)
    out, gq, gk, gv = run(tensor_of(rowptr, col, n), q, k, v, g)
    assert same(out, want, True) and not host(out)[9].any()
    assert not host(gq).any() and not np.abs(grads["q"]).max() > 1e-12
    assert same(gk, grads["k"], True) and same(gv, grads["v"], True)


# ---- 3. bias ---------------------------------------------------------------------------------------

def winner_positions(rowptr):
    """Per row: the positions of 1, 2 or 4 winners — first, last, 127 and 128, the first and the last chunk."""
    pos = []
    for r in range(rowptr.size - 1):
        ln = int(rowptr[r + 1] - rowptr[r])
        if ln == 0:
            pos.append([])
        elif ln < 4:
            pos.append([ln - 1])
        elif ln in (129, 256):
            pos.append([127, 128])
        elif ln >= 255:
            pos.append([0, 1, ln - 2, ln - 1])
        else:
            pos.append([0, ln - 1])
    return pos


def bias_case(rng, rowptr, col, H, low, per_head):
    """Equal raw scores within a row and head (k identical across nodes); the bias alone makes the winners: 0
    against `low`.  Per head form: odd heads keep only the last winner of a row."""
    M, nnz = rowptr.size - 1, col.size
    K, F = 4, 8
    q = ints(rng, (M, H, K), -2, 2)
    k = np.tile(ints(rng, (1, H, K), -2, 2), (N, 1, 1))
    v, g = ints(rng, (N, H, F), -2, 2), ints(rng, (M, H, F), -2, 2)
    bias = np.full((nnz, H) if per_head else (nnz,), low, dtype=np.float32)
    for r, pos in enumerate(winner_positions(rowptr)):
        for i, at in enumerate(pos):
            if per_head:
                bias[rowptr[r] + at, 0::2] = 0
                if i == len(pos) - 1:
                    bias[rowptr[r] + at, 1::2] = 0
            else:
                bias[rowptr[r] + at] = 0
    return q, k, v, g, bias


@pytest.mark.parametrize("low", [-2048.0, float("-inf")])
@pytest.mark.parametrize("per_head", [False, True])
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_bias_makes_the_winners_exact(big, per_head, low, scale):
    rowptr, col = big
    H = 3
    rng = np.random.default_rng(73)
    q, k, v, g, bias = bias_case(rng, rowptr, col, H, low, per_head)
    want = ar.attention_ref(rowptr, col, q, k, v, scale, bias)
    grads = ar.attention_grads_ref(rowptr, col, q, k, v, g, scale, bias)
    assert np.abs(grads["bias"]).max() > 0
    bd = dev(bias).requires_grad_()
    A = tensor_of(rowptr, col, N, bd)
    out, gq, gk, gv = run(A, q, k, v, g, scale, bias=True)
    assert same(out, want, True)
    assert bd.grad.shape == bias.shape and same(bd.grad, grads["bias"], True)
    assert same(gq, grads["q"], True) and same(gk, grads["k"], True) and same(gv, grads["v"], True)
    # a -inf entry gives the bits of the pattern without it
    if low == float("-inf") and not per_head:
        keep = bias == 0
        row = ar.rows_of(rowptr)
        rowptr_b = np.concatenate([[0], np.cumsum(np.bincount(row[keep], minlength=rowptr.size - 1))]).astype(np.int64)
        B = tensor_of(rowptr_b, col[keep], N, dev(bias[keep]))
        out_b = B.attention(dev(q), dev(k), dev(v), scale=scale, bias=True)
        assert torch.equal(out_b, out)


def test_stored_values_are_ignored_without_bias(big):
    rowptr, col = big
    rng = np.random.default_rng(74)
    M, H, K, F = rowptr.size - 1, 2, 4, 4
    q, k, v = (dev(rng.normal(size=s).astype(np.float32)) for s in ((M, H, K), (N, H, K), (N, H, F)))
    plain = tensor_of(rowptr, col, N).attention(q, k, v)
    nan = tensor_of(rowptr, col, N, torch.full((col.size,), float("nan"), device=DEV))
    assert torch.equal(nan.attention(q, k, v), plain) and not torch.isnan(plain).any()
    assert torch.isnan(nan.attention(q, k, v, bias=True)[1:]).all()


# ---- 4. general values -----------------------------------------------------------------------------

def _col_sum(col, n, x):
    out = np.zeros((n,) + x.shape[1:])
    np.add.at(out, col, x)
    return out


@pytest.mark.parametrize("H,K,F", [(1, 64, 64), (8, 16, 16), (3, 5, 7)])
def test_general_values_within_the_derived_bounds(big, H, K, F):
    """Normal q, k, v, g; scale = 1 / sqrt(K); the float64 reference is fed the same fp32 inputs.  u = 2^-24,
    len = the row's length, clen = the column's.

    Score.  K products summed in any order, with or without fma, then scaled: |s^ - s| <= (K + 2) u scale
    sum_k |q k|; Delta[r, h] is its maximum over the row.
    Weight.  exp turns the absolute error of s - m (both carry Delta) into a relative one, 2 Delta; the sum l of
    len terms, the exp itself, the rescales and the division add (len + 64) u — the softmax bound of
    test_softmax_gpu.py.  eps[r, h] = 2 Delta + (len + 64) u bounds |p^ - p| / p, for the forward's online
    weights and for the backward's exp(s - m) / l alike.
    out.       |out^ - out| <= eps * sum_e p |v|                                             (the issue's bound)
    grad_v.    A sum over the column of p^ g: |err| <= sum_{e in col} (eps[row e] + (clen + 2) u) p |g|.
    dS = p (dP - delta).  dP is a dot of F products: D_dP = (F + 2) u sum_f |g v|.  delta = <g, out^> carries
    the dot's rounding and out's error: D_delta = (F + 2) u sum_f |g| |out| + sum_f |g| eps sum_e p |v|.
               D_dS = eps p |dP - delta| + p (D_dP + D_delta) + 4 u p (|dP| + |delta|)
    grad_q.    scale * a sum over the row of dS^ k: |err| <= scale sum_e (D_dS + (len + 3) u |dS|) |k|.
    grad_k.    scale * a sum over the column of dS^ q: |err| <= scale sum_{e in col} (D_dS + (clen + 3) u |dS|) |q|.

    Prints worst error / bound for the fused op and for the unfused chain sddmm -> softmax -> spmm_heads on
    the same inputs; only the fused op is held to the bounds here (the chain has its own tests)."""
    from paddle_sparse_amd import ops

    rowptr, col = big
    M, nnz = rowptr.size - 1, col.size
    row = ar.rows_of(rowptr)
    rng = np.random.default_rng(75 + H)
    q, k, v, g = (rng.normal(size=s).astype(np.float32) for s in ((M, H, K), (N, H, K), (N, H, F), (M, H, F)))
    scale = float(np.float32(1.0 / np.sqrt(K)))
    want = ar.attention_ref(rowptr, col, q, k, v, scale)
    grads = ar.attention_grads_ref(rowptr, col, q, k, v, g, scale)
    p, ds = grads["p"], grads["ds"]
    q64, k64, v64, g64 = (a.astype(np.float64) for a in (q, k, v, g))

    length = np.diff(rowptr).astype(np.float64)
    clen = np.bincount(col, minlength=N).astype(np.float64)
    abs_qk = np.einsum("ehk,ehk->eh", np.abs(q64[row]), np.abs(k64[col]))
    Delta = np.zeros((M, H))
    np.maximum.at(Delta, row, (K + 2) * U * scale * abs_qk)
    eps = 2 * Delta + (length[:, None] + 64) * U                                  # [M, H]
    pv = np.zeros((M, H, F))
    np.add.at(pv, row, p[:, :, None] * np.abs(v64[col]))                          # sum_e p |v|
    b_out = eps[:, :, None] * pv
    b_gv = _col_sum(col, N, ((eps[row] + (clen[col, None] + 2) * U) * p)[:, :, None] * np.abs(g64[row]))
    dp = np.einsum("ehf,ehf->eh", g64[row], v64[col])
    delta = np.einsum("mhf,mhf->mh", g64, want)
    d_dp = (F + 2) * U * np.einsum("ehf,ehf->eh", np.abs(g64[row]), np.abs(v64[col]))
    d_delta = (F + 2) * U * np.einsum("mhf,mhf->mh", np.abs(g64), np.abs(want)) + \
        np.einsum("mhf,mhf->mh", np.abs(g64), b_out)
    d_ds = eps[row] * p * np.abs(dp - delta[row]) + p * (d_dp + d_delta[row]) + \
        4 * U * p * (np.abs(dp) + np.abs(delta[row]))
    b_gq = np.zeros((M, H, K))
    np.add.at(b_gq, row, scale * (d_ds + (length[row, None] + 3) * U * np.abs(ds))[:, :, None] * np.abs(k64[col]))
    b_gk = _col_sum(col, N, scale * (d_ds + (clen[col, None] + 3) * U * np.abs(ds))[:, :, None] * np.abs(q64[row]))
    wants = (want, grads["q"], grads["k"], grads["v"])
    bounds = (b_out, b_gq, b_gk, b_gv)

    A = tensor_of(rowptr, col, N)
    fused = run(A, q, k, v, g, scale)

    qd, kd, vd = (dev(a).requires_grad_() for a in (q, k, v))
    rp, cl = dev(rowptr), dev(col)
    att = ops.segment_softmax(ops.sddmm(rp, cl, qd, kd) * scale, rp)
    out_c = ops.spmm_heads(rp, cl, att, vd)
    out_c.backward(dev(g))
    chain = (out_c.detach(), qd.grad, kd.grad, vd.grad)

    ratios = {}
    for side, got in (("fused", fused), ("chain", chain)):
        ratios[side] = [float(np.max(np.abs(host(t) - w) / np.maximum(b, 1e-300))) for t, w, b in zip(got, wants, bounds)]
        print(f"attention ({H}, {K}, {F}) {side}: worst err / bound  out {ratios[side][0]:.4f}  grad_q "
              f"{ratios[side][1]:.4f}  grad_k {ratios[side][2]:.4f}  grad_v {ratios[side][3]:.4f}")
    for t, w, b in zip(fused, wants, bounds):
        assert np.all(np.abs(host(t) - w) <= b)


# ---- 5. non-finite values --------------------------------------------------------------------------

def test_non_finite_reaches_its_row_and_head_only(big):
    from paddle_sparse_amd import ops

    rowptr, col = big
    M, nnz = rowptr.size - 1, col.size
    H, K, F = 3, 4, 8
    rng = np.random.default_rng(76)
    q, k, v, g = (rng.normal(size=s).astype(np.float32) for s in ((M, H, K), (N, H, K), (N, H, F), (M, H, F)))
    bias = np.zeros((nnz, H), dtype=np.float32)
    q[13, 0, 1] = np.nan                                  # a NaN in q: row 13 (4099 entries), head 0
    bias[rowptr[12] + 700, 1] = np.inf                    # a +inf score: row 12 (1024 entries), head 1
    bias[rowptr[9]:rowptr[10], 2] = -np.inf               # nothing but -inf: row 9 (255 entries), head 2
    bias[rowptr[5]:rowptr[6], 0] = -np.inf                # ... and a short row: row 5, head 0
    bias[rowptr[10] + 3, 1] = -np.inf                     # a mask among finite scores: weight exactly 0
    want = ar.attention_ref(rowptr, col, q, k, v, 1.0, bias)
    bad = np.zeros((M, H), dtype=bool)
    bad[13, 0] = bad[12, 1] = bad[9, 2] = bad[5, 0] = True
    assert np.array_equal(np.isnan(want).all(axis=2), bad) and np.array_equal(np.isnan(want).any(axis=2), bad)

    bd = dev(bias).requires_grad_()
    A = tensor_of(rowptr, col, N, bd)
    qd, kd, vd = (dev(a).requires_grad_() for a in (q, k, v))
    out = A.attention(qd, kd, vd, bias=True)
    got = host(out)
    assert np.array_equal(np.isnan(got).all(axis=2), bad) and np.array_equal(~np.isfinite(got).all(axis=2), bad)
    assert np.allclose(got[~bad], want[~bad], rtol=1e-4, atol=1e-5)
    out.backward(dev(g))
    assert bd.grad[rowptr[10] + 3, 1] == 0  # the masked entry
    # the NaN stays in its rows' heads: grad_q only there, and the row without entries gets zeros
    gq = host(qd.grad)
    assert np.array_equal(np.isnan(gq).any(axis=2), bad) and not gq[0].any()

    # weight 0 against an inf in v: NaN (no zero skipping) in that row, head and feature only
    c = int(col[rowptr[10] + 3])
    v2 = v.copy()
    v2[c, 1, 5] = np.inf
    only = np.zeros((nnz, H), dtype=np.float32)
    only[rowptr[10] + 3, 1] = -np.inf
    got2 = host(ops.attention(dev(rowptr), dev(col), dev(q[:, 1:2]), dev(k[:, 1:2]), dev(v2[:, 1:2]), bias=dev(only[:, 1])))
    assert np.isnan(got2[10, 0, 5])
    touched = np.zeros((M, 1, F), dtype=bool)
    touched[ar.rows_of(rowptr)[col == c], 0, 5] = True
    assert np.array_equal(~np.isfinite(got2), touched)


def test_the_row_without_entries(big):
    from paddle_sparse_amd import ops

    rowptr, col = big
    M, H, K, F = rowptr.size - 1, 3, 5, 7
    rng = np.random.default_rng(77)
    q, k, v, g = (rng.normal(size=s).astype(np.float32) for s in ((M, H, K), (N, H, K), (N, H, F), (M, H, F)))
    out, stat = ops.attention_raw(dev(rowptr), dev(col), dev(q), dev(k), dev(v), scale=0.5)
    assert out.shape == (M, H, F) and stat.shape == (M, H, 2)
    assert not out[0].any() and bool((stat[0, :, 0] == float("-inf")).all()) and not stat[0, :, 1].any()
    want = ar.attention_stat_ref(rowptr, col, q, k, 0.5)
    assert np.allclose(host(stat)[1:], want[1:], rtol=1e-4, atol=1e-5)
    grads = run(tensor_of(rowptr, col, N), q, k, v, g, 0.5)
    assert all(bool(torch.isfinite(t).all()) for t in grads) and not grads[1][0].any()
    # a matrix of nothing but rows without entries
    rp0 = torch.zeros(4, dtype=torch.int64, device=DEV)
    out0, stat0 = ops.attention_raw(rp0, torch.zeros(0, dtype=torch.int64, device=DEV), dev(q[:3]), dev(k), dev(v))
    assert not out0.any() and bool((stat0[..., 0] == float("-inf")).all()) and not stat0[..., 1].any()


# ---- 6. no per-entry state -------------------------------------------------------------------------

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
        out = A.attention(qd, kd, vd, scale=0.25)
    assert len(saved) >= 5  # q, k, v, out, stat
    assert all(nnz not in shape for shape in saved), saved
    out.sum().backward()
    assert qd.grad is not None and kd.grad is not None and vd.grad is not None


# ---- 7. reproducible and capturable ----------------------------------------------------------------

def test_two_runs_give_the_same_bits_and_a_graph_replays_them(big):
    from paddle_sparse_amd import ops

    rowptr, col = big
    M, nnz = rowptr.size - 1, col.size
    H, K, F = 8, 16, 16
    rng = np.random.default_rng(79)

    def normal(*shape):
        return dev(rng.normal(size=shape).astype(np.float32))

    q, k, v, g, bias = normal(M, H, K), normal(N, H, K), normal(N, H, F), normal(M, H, F), normal(nnz, H)
    A = tensor_of(rowptr, col, N, bias)
    st = A.storage
    rp, cl = st.rowptr(), st.col()
    csc = (st.colptr(), st._row_in_csc_order(), st.csr2csc())

    def autograd_step():
        qd, kd, vd = (t.detach().requires_grad_() for t in (q, k, v))
        out = A.attention(qd, kd, vd, scale=0.25, bias=True)
        out.backward(g)
        return out.detach(), qd.grad, kd.grad, vd.grad

    first, second = autograd_step(), autograd_step()
    for a, b in zip(first, second):
        assert torch.equal(a, b)

    def step():  # what the autograd Function runs, forward and backward
        out, stat = ops.attention_raw(rp, cl, q, k, v, bias, 0.25)
        return (out,) + ops.attention_bw(rp, cl, q, k, v, bias, 0.25, g, out, stat, csc)

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
    for t in (q, k, v, g, bias):
        t.copy_(normal(*t.shape))
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(captured, step()):
        assert torch.equal(got, want)


# ---- 8. bare ops.attention -------------------------------------------------------------------------

def test_bare_pattern_equals_the_tensor_form_and_only_requested_gradients_are_made(big):
    from paddle_sparse_amd import ops

    rowptr, col = big
    M = rowptr.size - 1
    H, K, F = 3, 5, 7
    rng = np.random.default_rng(80)
    q, k, v, g = (rng.normal(size=s).astype(np.float32) for s in ((M, H, K), (N, H, K), (N, H, F), (M, H, F)))
    want = run(tensor_of(rowptr, col, N), q, k, v, g, 0.5)
    qd, kd, vd = (dev(a).requires_grad_() for a in (q, k, v))
    out = ops.attention(dev(rowptr), dev(col), qd, kd, vd, scale=0.5)  # no CSC view: the backward sorts col
    out.backward(dev(g))
    for a, b in zip(want, (out.detach(), qd.grad, kd.grad, vd.grad)):
        assert torch.equal(a, b)

    q1, k1, v1 = dev(q), dev(k), dev(v).requires_grad_()
    out = ops.attention(dev(rowptr), dev(col), q1, k1, v1, scale=0.5)
    out.backward(dev(g))
    assert q1.grad is None and k1.grad is None and torch.equal(v1.grad, want[3])


# ---- 9. argument errors ----------------------------------------------------------------------------

def test_errors():
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import ops

    H, K, F = 2, 4, 3
    row, col = torch.tensor([0, 1], device=DEV), torch.tensor([1, 2], device=DEV)
    A = psa.SparseTensor(row=row, col=col, sparse_sizes=(2, 3))
    q, k, v = torch.zeros(2, H, K, device=DEV), torch.zeros(3, H, K, device=DEV), torch.ones(3, H, F, device=DEV)
    assert torch.equal(A.attention(q, k, v), torch.ones(2, H, F, device=DEV))
    assert torch.equal(psa.attention(A, q[:, 0], k[:, 0], v[:, 0]), torch.ones(2, F, device=DEV))
    with pytest.raises(TypeError):
        A.attention(q.half(), k.half(), v.half())
    with pytest.raises(TypeError):
        A.attention(q, k, v.double())
    with pytest.raises(TypeError):
        A.attention(q, k, [1.0])
    with pytest.raises(TypeError):
        A.attention(q, k, v, scale="1")
    with pytest.raises(TypeError):
        A.attention(q, k, v, bias=torch.zeros(2, device=DEV))
    with pytest.raises(ValueError):
        A.attention(q[:, 0], k, v)  # mixed ranks
    with pytest.raises(ValueError):
        A.attention(q, k, v[:, 0])
    with pytest.raises(ValueError):
        A.attention(q[:, :, :, None], k[:, :, :, None], v[:, :, :, None])  # rank 4
    with pytest.raises(ValueError):
        A.attention(q, torch.zeros(3, H + 1, K, device=DEV), v)  # H of k
    with pytest.raises(ValueError):
        A.attention(q, k, torch.ones(3, H + 1, F, device=DEV))  # H of v
    with pytest.raises(ValueError):
        A.attention(q, torch.zeros(3, H, K + 1, device=DEV), v)  # K
    with pytest.raises(ValueError):
        A.attention(torch.zeros(3, H, K, device=DEV), k, v)  # M
    with pytest.raises(ValueError):
        A.attention(q, k, torch.ones(2, H, F, device=DEV))  # N
    with pytest.raises(ValueError):
        A.attention(q, k, v, bias=True)  # no values
    with pytest.raises(RuntimeError, match="GPU tensor"):
        A.attention(q.cpu(), k, v)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        A.attention(q, k, v.cpu())

    def with_value(value):
        return psa.SparseTensor(row=row, col=col, value=value, sparse_sizes=(2, 3))

    assert with_value(torch.zeros(2, device=DEV)).attention(q, k, v, bias=True).shape == (2, H, F)
    assert with_value(torch.zeros(2, H, device=DEV)).attention(q, k, v, bias=True).shape == (2, H, F)
    with pytest.raises(ValueError):
        with_value(torch.zeros(2, H + 1, device=DEV)).attention(q, k, v, bias=True)
    with pytest.raises(ValueError):
        with_value(torch.zeros(2, H, device=DEV)).attention(q[:, 0], k[:, 0], v[:, 0], bias=True)
    with pytest.raises(TypeError):
        with_value(torch.zeros(2, dtype=torch.float64, device=DEV)).attention(q, k, v, bias=True)

    rowptr = torch.tensor([0, 1, 2], device=DEV)
    with pytest.raises(TypeError):
        ops.attention(rowptr.int(), col, q, k, v)
    with pytest.raises(ValueError):
        ops.attention(rowptr, col, q, k, v, bias=torch.zeros(3, device=DEV))
    with pytest.raises(TypeError):
        ops.attention(rowptr, col, q, k, v, bias=torch.zeros(2, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.attention(rowptr.cpu(), col, q, k, v)
