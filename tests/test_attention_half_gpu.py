"""GPU suite of fused sparse attention with bfloat16 operands (psa_attention_half_fw / psa_attention_half_bw_entries
/ psa_spmm_heads_half behind SparseTensor.attention, ops.attention and ops.spmm_heads_half_raw).

The reference is tests/attention_ref.py (float64) applied to the bf16 inputs, which are exact in float64, and
rounded once to bf16 by tests/bf16_ref.py where a bf16 result is compared bit for bit.  The two exact regimes
are those of tests/test_attention_gpu.py, restated here: one-hot (winners lead by >= 512, every other weight
is exactly 0 in fp32) and uniform (equal scores, power-of-two row lengths).  Every fp32 sum of the kernels is
exact there, so the one rounding must land on round_bf16(reference) whatever the order of the additions."""
import numpy as np
import pytest
import torch

import attention_ref as ar
import bf16_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 300]
N = 340
U = 2.0 ** -24
UB = 2.0 ** -8   # the bound the tests use for one bf16 rounding (round to nearest is within 2^-9 relative)
# (H, K, F): the smallest 16-byte form; the bench widths; one pass of one slice and one tile per lane; an element
# form with nothing a power of two; 16-byte form with K != F and widths that are no power of two; one head wider
# than the accumulator tiles (element form); more slices of q than stay in registers; more heads than a head block
SHAPES = [(1, 8, 8), (8, 16, 16), (1, 64, 64), (3, 5, 7), (2, 24, 40), (1, 3, 261), (1, 261, 3), (17, 8, 8)]


def pattern(rng, lens, n):
    """Sorted CSR pattern with the given row lengths, distinct columns inside a row."""
    cols = [np.sort(rng.choice(n, size=ln, replace=False)) for ln in lens]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rowptr, np.concatenate(cols).astype(np.int64) if cols else np.zeros(0, dtype=np.int64)


def ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def bf_values(rng, shape):
    """Normal values that are bf16 numbers, as fp32."""
    return bf16_ref.round_bf16(rng.normal(size=shape).astype(np.float32)).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bf(a):
    """The bf16 tensor of an fp32 array whose values are bf16 numbers."""
    t = dev(a)
    h = t.to(BF)
    assert torch.equal(h.float(), t) or bool(torch.isnan(t).any())
    return h


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def offset_copy(t):
    """The same numbers in a view that starts one element into its allocation."""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = base[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size()
    return view


def tensor_of(rowptr, col, n, value=None):
    import paddle_sparse_amd as psa

    return psa.SparseTensor(rowptr=dev(rowptr), col=dev(col), value=value, sparse_sizes=(rowptr.size - 1, n),
                            is_sorted=True)


def run(A, q, k, v, g, scale=1.0, bias=False, shift=False):
    """bf16 out and the bf16 gradients of q, k, v through the tensor form; shift: operands one element off."""
    make = (lambda a: offset_copy(bf(a))) if shift else bf
    qd, kd, vd = (make(a).requires_grad_() for a in (q, k, v))
    out = A.attention(qd, kd, vd, scale=scale, bias=bias)
    out.backward(make(g))
    return out.detach(), qd.grad, kd.grad, vd.grad


def same(got, want):
    """Bit for bit: the bf16 result equals the float64 reference rounded to fp32 (which drops what no fp32 can
    hold, as in tests/test_attention_gpu.py::test_one_hot_exact) and then once to bf16."""
    assert got.dtype == BF
    return np.array_equal(host(got), bf16_ref.round_bf16(want.astype(np.float32)))


# ---- 1. exact, one-hot regime ----------------------------------------------------------------------

W_ALL = [0, 1, 170, 171, N - 2, N - 1]   # winner columns of the even heads
W_ODD = [0, 170, N - 1]                  # ... of the odd heads: a subset that leaves every row 1 or 2 of them


def one_hot_pattern(rng):
    """Rows of LENGTHS whose winners sit at the first entry, the last entry, entries 127 and 128 (either side of
    the chunk edge) and in the first and the last chunk of the longest row; 1, 2 or 4 winners per row."""
    losers = np.setdiff1d(np.arange(N), W_ALL)
    winners = {1: [170], 2: [0, N - 1], 63: [0], 64: [N - 1], 65: [0, N - 1], 127: [170], 128: [170, 171],
               129: [170, 171], 300: [0, 1, N - 2, N - 1]}
    cols, where = [], {}
    for ln in LENGTHS:
        if ln == 0:
            cols.append(np.zeros(0, dtype=np.int64))
            continue
        w = winners[ln]
        if ln == 129:  # exactly 127 losers below column 170: the winners are entries 127 and 128
            c = np.concatenate([rng.choice(losers[losers < 170], size=127, replace=False), w])
        else:
            c = np.concatenate([rng.choice(losers, size=ln - len(w), replace=False), w])
        c = np.sort(c).astype(np.int64)
        cols.append(c)
        where[ln] = [int(np.searchsorted(c, x)) for x in w]
    assert where[129] == [127, 128] and where[63] == [0] and where[64] == [63] and where[300] == [0, 1, 298, 299]
    rowptr = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    return rowptr, np.concatenate(cols)


@pytest.fixture(scope="module")
def one_hot():
    return one_hot_pattern(np.random.default_rng(71))


def one_hot_data(rng, M, H, K, F):
    """Integers of magnitude <= 32: bf16 numbers.  Winners score scale * 1024, losers scale * 32 * k0 <= 0."""
    q = ints(rng, (M, H, K), -3, 3)
    q[:, :, 0] = 32
    k = np.zeros((N, H, K), dtype=np.float32)
    k[:, :, 0] = ints(rng, (N, H), -32, 0)
    for h in range(H):
        k[W_ALL if h % 2 == 0 else W_ODD, h, 0] = 32
    return q, k, ints(rng, (N, H, F), -2, 2), ints(rng, (M, H, F), -2, 2)


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("H,K,F", SHAPES)
def test_one_hot_exact(one_hot, H, K, F, scale):
    """The gap between winners and losers is at least 512 at either scale and fp32 exp(-512) is exactly 0, so p is 0
    or 1 / (1, 2 or 4) on the GPU, out is a multiple of 1/4 of magnitude <= 2 (a bf16 number: the delta of the
    backward, formed from the rounded out, is the exact one) and dP, delta, dS and the three gradient sums are
    dyadic rationals within 24 bits: exact in fp32 in any order.  `scale` is a power of two.  So out must equal the
    reference and each gradient the reference rounded once."""
    rowptr, col = one_hot
    M = rowptr.size - 1
    rng = np.random.default_rng(100 * H + 10 * K + F)
    q, k, v, g = one_hot_data(rng, M, H, K, F)
    for a in (q, k, v, g):
        assert bf16_ref.is_bf16(a).all() and np.abs(a).max() <= 256
    s = ar.scores_ref(rowptr, col, q, k, scale)
    p = ar.softmax_ref(rowptr, s)[0]
    assert set(np.unique(np.round(p[p > 1e-100], 12))) <= {1.0, 0.5, 0.25} and (p > 1e-100).sum() > H * 9
    row = ar.rows_of(rowptr)
    top = np.full((M, H), -np.inf)
    np.fmax.at(top, row, s)
    assert np.all((s == top[row]) | (s <= top[row] - 512))  # every other weight is exactly 0 in fp32
    want = ar.attention_ref(rowptr, col, q, k, v, scale)
    # a condition on the construction, not on the kernel: the reference's out is a bf16 number already
    assert bf16_ref.is_bf16(want.astype(np.float32).astype(np.float64)).all()
    grads = ar.attention_grads_ref(rowptr, col, q, k, v, g, scale)
    assert np.abs(grads["ds"]).max() > 0  # two winners with different dP somewhere

    A = tensor_of(rowptr, col, N)
    for shift in (False, True):  # aligned operands: the 16-byte form where K % 8 == F % 8 == 0; one element off
        out, gq, gk, gv = run(A, q, k, v, g, scale, shift=shift)
        assert out.shape == (M, H, F) and same(out, want) and not host(out)[0].any()
        assert same(gq, grads["q"]) and same(gk, grads["k"]) and same(gv, grads["v"])
    # the element form itself (the tensor form copies a misaligned operand when that buys the 16-byte form)
    from paddle_sparse_amd import _lib, ops

    qo, ko, vo = (offset_copy(bf(a)) for a in (q, k, v))
    raw = torch.empty((M, H, F), dtype=BF, device=DEV)
    stat = torch.empty((M, H, 2), dtype=torch.float32, device=DEV)
    lib = _lib.load()
    nb = lib.psa_attention_workspace_bytes(col.size, H, F)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
    rp, cl = dev(rowptr), dev(col)
    _lib.check(lib.psa_attention_half_fw(PSA_BF16(), rp.data_ptr(), cl.data_ptr(), qo.data_ptr(), ko.data_ptr(),
                                         vo.data_ptr(), None, 1, scale, M, N, H, K, F, col.size, raw.data_ptr(),
                                         stat.data_ptr(), ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream))
    assert torch.equal(raw, out)
    assert ops.attention_raw(rp, cl, bf(q), bf(k), bf(v), scale=scale)[1].equal(stat)
    # ... and of the backward's per-entry half: q, k, v, grad_out and out one element off.  p and dS are exact in
    # fp32 here, so both forms must give the reference (rounded to fp32: see same())
    for shift in (False, True):
        make = offset_copy if shift else (lambda x: x)
        pe, ds = bw_entries_raw(rp, cl, make(bf(q)), make(bf(k)), make(bf(v)), None, scale, make(bf(g)), make(out), stat)
        for got, ref in ((pe, grads["p"]), (ds, grads["ds"])):
            assert np.array_equal(host(got), ref.astype(np.float32).astype(np.float64))


def PSA_BF16():
    from paddle_sparse_amd import ops

    return ops._DTYPE_ID[torch.bfloat16]


def bw_entries_raw(rp, cl, q, k, v, bias, scale, g, out, stat):
    """psa_attention_half_bw_entries on the operands as they are (no copy to a 16-byte boundary): (p, dS)."""
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    (M, H, K), (N_, _, F), nnz = q.shape, v.shape, cl.numel()
    pe = torch.full((nnz, H), 9.0, device=DEV)
    ds = torch.full((nnz, H), 9.0, device=DEV)
    nb = lib.psa_attention_workspace_bytes(nnz, H, F)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
    _lib.check(lib.psa_attention_half_bw_entries(
        PSA_BF16(), rp.data_ptr(), cl.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
        None if bias is None else bias.data_ptr(), 1 if bias is None or bias.dim() == 1 else H, scale, g.data_ptr(),
        out.data_ptr(), stat.data_ptr(), M, N_, H, K, F, nnz, pe.data_ptr(), ds.data_ptr(), ws.data_ptr(), nb,
        torch.cuda.current_stream().cuda_stream))
    return pe, ds


def test_one_hot_exact_two_d_form(one_hot):
    rowptr, col = one_hot
    M, K, F = rowptr.size - 1, 8, 16
    rng = np.random.default_rng(208)
    q, k, v, g = (a[:, 0] for a in one_hot_data(rng, M, 1, K, F))
    want = ar.attention_ref(rowptr, col, q, k, v)
    grads = ar.attention_grads_ref(rowptr, col, q, k, v, g)
    out, gq, gk, gv = run(tensor_of(rowptr, col, N), q, k, v, g)
    assert out.shape == (M, F) and gq.shape == (M, K) and gk.shape == (N, K) and gv.shape == (N, F)
    assert same(out, want) and same(gq, grads["q"]) and same(gk, grads["k"]) and same(gv, grads["v"])


# ---- 2. exact, uniform regime ----------------------------------------------------------------------

@pytest.mark.parametrize("H,F", [(1, 8), (3, 7), (8, 16)])
def test_uniform_exact(H, F):
    """q = 0: every score is 0, p = 1 / length with lengths 1, 2, 4, 64, 128, 256, and out is the mean of integer
    rows of v whose sums stay below 256 in magnitude: an integer of at most 8 bits over a power of two, a bf16
    number.  The 256-entry row runs as two 128-entry chunks with equal maxima, which merge with factors exactly
    1: it must equal the mean of two 128-entry rows that hold its two halves (one chunk each, no merge)."""
    rng = np.random.default_rng(72 + H)
    n, K = 300, 8
    cols256 = np.sort(rng.choice(n, size=256, replace=False))
    lens = [1, 2, 4, 64, 128, 256, 128, 128]
    rowptr, col = pattern(rng, lens, n)
    col[rowptr[5]:rowptr[6]] = cols256
    col[rowptr[6]:rowptr[7]] = cols256[:128]
    col[rowptr[7]:rowptr[8]] = cols256[128:]
    M = len(lens)
    q = np.zeros((M, H, K), dtype=np.float32)
    k = ints(rng, (n, H, K), -3, 3)
    v = ints(rng, (n, H, F), -1, 1)
    v[::2] = np.abs(v[::2])  # sums of 256 entries stay far below 256 without being 0
    row = ar.rows_of(rowptr)
    sums = np.zeros((M, H, F))
    np.add.at(sums, row, v[col].astype(np.float64))
    assert np.abs(sums).max() < 256 and np.abs(sums[5]).min() >= 0 and np.abs(sums[5]).max() > 16
    want = ar.attention_ref(rowptr, col, q, k, v)
    assert bf16_ref.is_bf16(want).all()
    out = tensor_of(rowptr, col, n).attention(bf(q), bf(k), bf(v))
    assert out.dtype == BF and np.array_equal(host(out), want)
    got = host(out)
    assert np.array_equal(got[5], (got[6] + got[7]) / 2)


# ---- 3. bias ---------------------------------------------------------------------------------------

def winner_positions(rowptr):
    """Per row: the positions of 1, 2 or 4 winners - first, last, 127 and 128, the first and the last chunk."""
    pos = []
    for r in range(rowptr.size - 1):
        ln = int(rowptr[r + 1] - rowptr[r])
        pos.append([] if ln == 0 else [ln - 1] if ln < 4 else [127, 128] if ln == 129 else
                   [0, 1, ln - 2, ln - 1] if ln >= 255 else [0, ln - 1])
    return pos


@pytest.mark.parametrize("low", [-2048.0, float("-inf")])
@pytest.mark.parametrize("per_head", [False, True])
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("K,F", [(8, 8), (5, 7)])
def test_bias_makes_the_winners_exact(one_hot, K, F, scale, per_head, low):
    """tests/test_attention_gpu.py's bias test restated for bf16 operands and an fp32 bias.  k is identical across
    nodes, so the raw scores of a row and head are equal and the bias alone makes the winners: 0 against `low`
    (exp(-2048) is 0 in fp32 and in float64).  In the per-head form the odd heads keep only the last winner of a
    row, so a bias read with the wrong stride or head shows.  Integers of magnitude <= 2: out is a mean of 1, 2 or 4
    integers (a bf16 number), every fp32 sum is exact, grad_bias (fp32) must equal the float64 reference and the
    bf16 gradients the reference rounded once."""
    rowptr, col = one_hot
    M, nnz, H = rowptr.size - 1, col.size, 3
    rng = np.random.default_rng(73 + K)
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
    want = ar.attention_ref(rowptr, col, q, k, v, scale, bias)
    assert bf16_ref.is_bf16(want).all()
    grads = ar.attention_grads_ref(rowptr, col, q, k, v, g, scale, bias)
    assert np.abs(grads["bias"]).max() > 0
    bd = dev(bias).requires_grad_()
    out, gq, gk, gv = run(tensor_of(rowptr, col, N, bd), q, k, v, g, scale, bias=True)
    assert same(out, want) and same(gq, grads["q"]) and same(gk, grads["k"]) and same(gv, grads["v"])
    assert bd.grad.dtype == torch.float32 and bd.grad.shape == bias.shape
    assert np.array_equal(host(bd.grad), grads["bias"])


# ---- 4. general values -----------------------------------------------------------------------------

def _col_sum(col, n, x):
    out = np.zeros((n,) + x.shape[1:])
    np.add.at(out, col, x)
    return out


@pytest.fixture(scope="module")
def general():
    rng = np.random.default_rng(61)
    lens = list(rng.integers(0, 41, size=196)) + [129, 200, 300, 0]
    return pattern(rng, lens, N)


@pytest.mark.parametrize("bias_form", ["none", "shared", "per_head"])
@pytest.mark.parametrize("H,K,F", [(1, 64, 64), (8, 16, 16), (3, 5, 7)])
def test_general_values_within_the_derived_bounds(general, H, K, F, bias_form):
    """Normal q, k, v, g rounded to bf16; scale = 1 / sqrt(K); the float64 reference is fed the same bf16 values.
    u = 2^-24, ub = 2^-8, len = the row's length, clen = the column's.  Inside the kernels everything is fp32, so
    the fp32 terms are those of tests/test_attention_gpu.py::test_general_values_within_the_derived_bounds:

    Score.  |s^ - s| <= (K + 2) u scale sum_k |q k|; Delta[r, h] is its maximum over the row.  With a bias (normal
            fp32 values, [nnz] shared by the heads or [nnz, H]) the score is fl(fl(scale dot) + bias): one more
            rounding, of a number of magnitude <= scale sum_k |q k| + |bias| (to first order):
            |s^ - s| <= (K + 3) u scale sum_k |q k| + u |bias|.
    Weight.  eps[r, h] = 2 Delta + (len + 64) u bounds |p^ - p| / p, forward and backward.
    out.       fp32: eps * sum_e p |v|.  The result is rounded once: + ub |out|.
    grad_v.    fp32: sum_{e in col} (eps[row e] + (clen + 2) u) p |g|; rounded once: + ub |grad_v|.
    dS = p (dP - delta).  D_dP = (F + 2) u sum_f |g v|.  delta = <g, round(out^)>: the dot's rounding, out's fp32
               error and out's final rounding, the last being |Ddelta| <= ub sum_f |g out|:
               D_delta = (F + 2) u sum_f |g| |out| + sum_f |g| eps sum_e p |v| + ub sum_f |g| |out|
               D_dS = eps p |dP - delta| + p (D_dP + D_delta) + 4 u p (|dP| + |delta|)
    grad_q.    scale sum_e (D_dS + (len + 3) u |dS|) |k|, rounded once: + ub |grad_q|.
    grad_k.    scale sum_{e in col} (D_dS + (clen + 3) u |dS|) |q|, rounded once: + ub |grad_k|.
    grad_bias. fp32, not rounded to bf16.  [nnz, H]: dS itself, D_dS.  [nnz]: the fp32 sum of H terms in any order,
               sum_h D_dS + H u sum_h |dS|.
    (Round to nearest is within 2^-9 of the computed value; ub = 2^-8 of the reference leaves the other 2^-9 for
    the computed value's own distance from the reference.)

    Prints worst error / bound per output."""
    rowptr, col = general
    M = rowptr.size - 1
    row = ar.rows_of(rowptr)
    rng = np.random.default_rng(75 + H)
    q, k, v, g = (bf_values(rng, s) for s in ((M, H, K), (N, H, K), (N, H, F), (M, H, F)))
    scale = float(np.float32(1.0 / np.sqrt(K)))
    bias = None if bias_form == "none" else rng.normal(size=(col.size,) if bias_form == "shared" else
                                                        (col.size, H)).astype(np.float32)
    want = ar.attention_ref(rowptr, col, q, k, v, scale, bias)
    grads = ar.attention_grads_ref(rowptr, col, q, k, v, g, scale, bias)
    p, ds = grads["p"], grads["ds"]
    q64, k64, v64, g64 = (a.astype(np.float64) for a in (q, k, v, g))

    length = np.diff(rowptr).astype(np.float64)
    clen = np.bincount(col, minlength=N).astype(np.float64)
    abs_qk = np.einsum("ehk,ehk->eh", np.abs(q64[row]), np.abs(k64[col]))
    Delta = np.zeros((M, H))
    d_score = (K + 2) * U * scale * abs_qk
    if bias is not None:
        abs_b = np.abs(bias.astype(np.float64))
        d_score = (K + 3) * U * scale * abs_qk + U * (abs_b[:, None] if abs_b.ndim == 1 else abs_b)
    np.maximum.at(Delta, row, d_score)
    eps = 2 * Delta + (length[:, None] + 64) * U
    pv = np.zeros((M, H, F))
    np.add.at(pv, row, p[:, :, None] * np.abs(v64[col]))
    f_out = eps[:, :, None] * pv
    b_out = f_out + UB * np.abs(want)
    b_gv = _col_sum(col, N, ((eps[row] + (clen[col, None] + 2) * U) * p)[:, :, None] * np.abs(g64[row])) + \
        UB * np.abs(grads["v"])
    dp = np.einsum("ehf,ehf->eh", g64[row], v64[col])
    delta = np.einsum("mhf,mhf->mh", g64, want)
    g_out = np.einsum("mhf,mhf->mh", np.abs(g64), np.abs(want))
    d_dp = (F + 2) * U * np.einsum("ehf,ehf->eh", np.abs(g64[row]), np.abs(v64[col]))
    d_delta = (F + 2) * U * g_out + np.einsum("mhf,mhf->mh", np.abs(g64), f_out) + UB * g_out
    d_ds = eps[row] * p * np.abs(dp - delta[row]) + p * (d_dp + d_delta[row]) + \
        4 * U * p * (np.abs(dp) + np.abs(delta[row]))
    b_gq = np.zeros((M, H, K))
    np.add.at(b_gq, row, scale * (d_ds + (length[row, None] + 3) * U * np.abs(ds))[:, :, None] * np.abs(k64[col]))
    b_gq += UB * np.abs(grads["q"])
    b_gk = _col_sum(col, N, scale * (d_ds + (clen[col, None] + 3) * U * np.abs(ds))[:, :, None] * np.abs(q64[row])) + \
        UB * np.abs(grads["k"])
    wants = [want, grads["q"], grads["k"], grads["v"]]
    bounds = [b_out, b_gq, b_gk, b_gv]

    bd = None if bias is None else dev(bias).requires_grad_()
    got = list(run(tensor_of(rowptr, col, N, bd), q, k, v, g, scale, bias=bias is not None))
    assert all(t.dtype == BF for t in got)
    if bias is not None:
        assert bd.grad.dtype == torch.float32 and bd.grad.shape == bias.shape
        got.append(bd.grad)
        wants.append(grads["bias"])
        bounds.append(d_ds if bias_form == "per_head" else d_ds.sum(axis=1) + H * U * np.abs(ds).sum(axis=1))
    ratios = [float(np.max(np.abs(host(t) - w) / np.maximum(b, 1e-300))) for t, w, b in zip(got, wants, bounds)]
    print(f"attention bf16 ({H}, {K}, {F}) bias {bias_form}: worst err / bound  " +
          "  ".join(f"{n} {r:.4f}" for n, r in zip(("out", "grad_q", "grad_k", "grad_v", "grad_bias"), ratios)))
    for t, w, b in zip(got, wants, bounds):
        assert np.all(np.abs(host(t) - w) <= b)


# ---- 5. psa_spmm_heads_half alone ------------------------------------------------------------------

def spmm_heads_ref(rowptr, col, value, mat, alpha):
    row = ar.rows_of(rowptr)
    out = np.zeros((rowptr.size - 1,) + mat.shape[1:])
    np.add.at(out, row, value.astype(np.float64)[:, :, None] * mat.astype(np.float64)[col])
    return alpha * out


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("H,F", [(1, 8), (8, 16), (3, 7), (2, 40), (1, 261), (1, 1032)])
def test_spmm_heads_half_exact(H, F, alpha):
    """Integers of magnitude <= 3 (value positive, mat positive in the even and negative in the odd features, so
    that sums pass 256 and do round) and rows of at most 300 entries: every fp32 sum is an exact integer below
    2^12, alpha is a power of two, and the result is the reference rounded once."""
    from paddle_sparse_amd import ops

    rng = np.random.default_rng(300 + H + F)
    lens = [0, 1, 128, 129, 300, 5, 0]
    rowptr, col = pattern(rng, lens, N)
    value, mat = ints(rng, (col.size, H), 1, 3), ints(rng, (N, H, F), 0, 3)
    mat[:, :, 1::2] *= -1
    want = spmm_heads_ref(rowptr, col, value, mat, alpha)
    assert np.abs(want).max() > 256  # some results do round
    rp, cl = dev(rowptr), dev(col)
    out = ops.spmm_heads_half_raw(rp, cl, dev(value), bf(mat), alpha)
    assert out.shape == (len(lens), H, F) and same(out, want) and not host(out)[0].any()
    assert torch.equal(ops.spmm_heads_half_raw(rp, cl, dev(value), offset_copy(bf(mat)), alpha), out)
    # the element form itself: mat and out one element off
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    mo = offset_copy(bf(mat))
    raw = offset_copy(torch.full((len(lens), H, F), 7.0, dtype=BF, device=DEV))
    nb = lib.psa_spmm_heads_workspace_bytes(col.size, H, F)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
    _lib.check(lib.psa_spmm_heads_half(PSA_BF16(), rp.data_ptr(), cl.data_ptr(), dev(value).data_ptr(), mo.data_ptr(),
                                       alpha, len(lens), N, H, F, col.size, raw.data_ptr(), ws.data_ptr(), nb,
                                       torch.cuda.current_stream().cuda_stream))
    assert torch.equal(raw, out)
    # a pattern without entries: zeros
    rp0 = torch.zeros(4, dtype=torch.int64, device=DEV)
    out0 = ops.spmm_heads_half_raw(rp0, cl[:0], dev(value)[:0], bf(mat), alpha)
    assert out0.shape == (3, H, F) and out0.dtype == BF and not out0.any()


@pytest.mark.parametrize("H,F", [(8, 16), (3, 7)])
def test_spmm_heads_half_general_values(general, H, F):
    """fp32 value, bf16 mat: a sum of len products in fp32, then alpha, then one rounding:
    |err| <= (len + 3) u |alpha| sum_e |value mat| + ub |ref|."""
    from paddle_sparse_amd import ops

    rowptr, col = general
    rng = np.random.default_rng(310 + H)
    value = rng.normal(size=(col.size, H)).astype(np.float32)
    mat = bf_values(rng, (N, H, F))
    alpha = 0.3
    want = spmm_heads_ref(rowptr, col, value, mat, float(np.float32(alpha)))
    mag = spmm_heads_ref(rowptr, col, np.abs(value), np.abs(mat), float(np.float32(alpha)))
    length = np.diff(rowptr).astype(np.float64)
    bound = (length[:, None, None] + 3) * U * mag + UB * np.abs(want)
    out = ops.spmm_heads_half_raw(dev(rowptr), dev(col), dev(value), bf(mat), alpha)
    err = np.abs(host(out) - want)
    print(f"spmm_heads_half ({H}, {F}): worst err / bound {float(np.max(err / np.maximum(bound, 1e-300))):.4f}")
    assert np.all(err <= bound)


def test_spmm_heads_half_errors():
    from paddle_sparse_amd import _lib, ops

    rp = torch.tensor([0, 1], dtype=torch.int64, device=DEV)
    cl = torch.tensor([0], dtype=torch.int64, device=DEV)
    val = torch.ones(1, 2, device=DEV)
    mat = torch.ones(1, 2, 4, device=DEV)
    with pytest.raises(TypeError):
        ops.spmm_heads_half_raw(rp, cl, val, mat)
    with pytest.raises(TypeError):
        ops.spmm_heads_half_raw(rp, cl, val, mat.half())
    with pytest.raises(TypeError):
        ops.spmm_heads_half_raw(rp, cl, val.to(BF), mat.to(BF))
    with pytest.raises(ValueError):
        ops.spmm_heads_half_raw(rp, cl, val[:, :1], mat.to(BF))
    lib = _lib.load()
    m, o = mat.to(BF), torch.empty(1, 2, 4, dtype=BF, device=DEV)
    for code in (ops._DTYPE_ID[torch.float32], ops._DTYPE_ID[torch.float16]):  # not served
        assert lib.psa_spmm_heads_half(code, rp.data_ptr(), cl.data_ptr(), val.data_ptr(), m.data_ptr(), 1.0, 1, 1, 2, 4,
                                       1, o.data_ptr(), None, 0, None) == 1
        assert b"dtype" in lib.psa_last_error()
        assert lib.psa_attention_half_fw(code, rp.data_ptr(), cl.data_ptr(), m.data_ptr(), m.data_ptr(), m.data_ptr(),
                                         None, 1, 1.0, 1, 1, 2, 4, 4, 1, o.data_ptr(), val.data_ptr(), None, 0,
                                         None) == 1
        assert b"dtype" in lib.psa_last_error()


# ---- 6. non-finite values --------------------------------------------------------------------------

def test_non_finite_reaches_its_row_and_head_only(general):
    rowptr, col = general
    M, nnz = rowptr.size - 1, col.size
    H, K, F = 3, 8, 8
    rng = np.random.default_rng(76)
    q, k, v, g = (bf_values(rng, s) for s in ((M, H, K), (N, H, K), (N, H, F), (M, H, F)))
    length = np.diff(rowptr)
    r_nan, r_inf, r_all, r_short = 198, 197, 196, int(np.flatnonzero(length[:190] > 3)[0])
    assert length[r_nan] == 300 and length[r_inf] == 200 and length[r_all] == 129 and length[M - 1] == 0
    r_mask = int(np.flatnonzero(length[:190] > 8)[1])
    assert len({r_nan, r_inf, r_all, r_short, r_mask}) == 5
    bias = np.zeros((nnz, H), dtype=np.float32)
    q[r_nan, 0, 1] = np.nan                                     # a NaN in q: a 300-entry row, head 0
    bias[rowptr[r_inf] + 150, 1] = np.inf                       # a +inf score: a 200-entry row, head 1
    bias[rowptr[r_all]:rowptr[r_all + 1], 2] = -np.inf          # nothing but -inf: a 129-entry row, head 2
    bias[rowptr[r_short]:rowptr[r_short + 1], 0] = -np.inf      # ... and a short row, head 0
    bias[rowptr[r_mask] + 3, 1] = -np.inf                       # a mask among finite scores: weight exactly 0
    want = ar.attention_ref(rowptr, col, q, k, v, 1.0, bias)
    bad = np.zeros((M, H), dtype=bool)
    bad[r_nan, 0] = bad[r_inf, 1] = bad[r_all, 2] = bad[r_short, 0] = True
    assert np.array_equal(np.isnan(want).all(axis=2), bad) and np.array_equal(np.isnan(want).any(axis=2), bad)

    bd = dev(bias).requires_grad_()
    A = tensor_of(rowptr, col, N, bd)
    qd, kd, vd = (bf(a).requires_grad_() for a in (q, k, v))
    out = A.attention(qd, kd, vd, bias=True)
    got = host(out)
    assert np.array_equal(np.isnan(got).all(axis=2), bad) and np.array_equal(~np.isfinite(got).all(axis=2), bad)
    assert np.allclose(got[~bad], want[~bad], rtol=2 ** -7, atol=1e-3)
    out.backward(bf(g))
    assert bd.grad.dtype == torch.float32 and bd.grad[rowptr[r_mask] + 3, 1] == 0  # the masked entry
    gq = host(qd.grad)
    assert np.array_equal(np.isnan(gq).any(axis=2), bad) and not gq[M - 1].any()



def test_a_masked_entry_has_weight_exactly_zero(general):
    """A -inf bias among finite scores: the output equals the same row without those entries.  In the exact
    regime, so that the order of the additions (which the missing entries change) cannot show: q = 0, integer
    v, and per row 1, 2 or 4 entries keep bias 0 (the first, the last, and two around the middle) while every
    other entry is masked: out is a mean of 1, 2 or 4 integers either way."""
    rowptr, col = general
    M, nnz = rowptr.size - 1, col.size
    H, K, F = 3, 8, 8
    rng = np.random.default_rng(81)
    q = np.zeros((M, H, K), dtype=np.float32)
    k, v = ints(rng, (N, H, K), -3, 3), ints(rng, (N, H, F), -2, 2)
    one = np.full(nnz, -np.inf, dtype=np.float32)
    for r in range(M):
        s, ln = rowptr[r], int(rowptr[r + 1] - rowptr[r])
        at = [] if ln == 0 else [0] if ln < 2 else [0, ln - 1] if ln < 4 else [0, ln // 2 - 1, ln // 2, ln - 1]
        one[[s + a for a in at]] = 0
    keep = one == 0
    assert 0 < keep.sum() < nnz / 2 and keep[rowptr[198] + 299] and not keep[rowptr[198] + 128]
    want = ar.attention_ref(rowptr, col, q, k, v, 1.0, one)
    assert bf16_ref.is_bf16(want).all()
    masked = tensor_of(rowptr, col, N, dev(one)).attention(bf(q), bf(k), bf(v), bias=True)
    rowptr_b = np.concatenate([[0], np.cumsum(np.bincount(row_of(rowptr)[keep], minlength=M))]).astype(np.int64)
    without = tensor_of(rowptr_b, col[keep], N).attention(bf(q), bf(k), bf(v))
    assert torch.equal(masked, without) and np.array_equal(host(masked), want)


def row_of(rowptr):
    return ar.rows_of(rowptr)


# ---- 7. the row without entries --------------------------------------------------------------------

def test_the_row_without_entries(general):
    from paddle_sparse_amd import ops

    rowptr, col = general
    M, H, K, F = rowptr.size - 1, 3, 5, 7
    empty = np.flatnonzero(np.diff(rowptr) == 0)
    assert empty.size >= 2 and empty[-1] == M - 1
    rng = np.random.default_rng(77)
    q, k, v, g = (bf_values(rng, s) for s in ((M, H, K), (N, H, K), (N, H, F), (M, H, F)))
    out, stat = ops.attention_raw(dev(rowptr), dev(col), bf(q), bf(k), bf(v), scale=0.5)
    assert out.dtype == BF and stat.dtype == torch.float32 and out.shape == (M, H, F) and stat.shape == (M, H, 2)
    e = torch.from_numpy(empty).to(DEV)
    assert not out[e].any() and bool((stat[e, :, 0] == float("-inf")).all()) and not stat[e, :, 1].any()
    want = ar.attention_stat_ref(rowptr, col, q, k, 0.5)
    full = np.diff(rowptr) > 0
    assert np.allclose(host(stat)[full], want[full], rtol=1e-4, atol=1e-5)
    # no gradient contribution: g of the rows without entries does not matter, and their grad_q is 0
    g2 = g.copy()
    g2[empty] = 100.0
    A = tensor_of(rowptr, col, N)
    first, second = run(A, q, k, v, g, 0.5), run(A, q, k, v, g2, 0.5)
    for a, b in zip(first, second):
        assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all())
    assert not first[1][e].any()
    # nothing is written for it: p and dS of a pattern of nothing but such rows stay as they were (none exist),
    # and the forward of that pattern is zeros and {-inf, 0}
    rp0 = torch.zeros(4, dtype=torch.int64, device=DEV)
    out0, stat0 = ops.attention_raw(rp0, torch.zeros(0, dtype=torch.int64, device=DEV), bf(q[:3]), bf(k), bf(v))
    assert out0.dtype == BF and not out0.any() and bool((stat0[..., 0] == float("-inf")).all()) and not stat0[..., 1].any()
    # the entries' half of the backward leaves the slots of other rows alone: poison p / dS and look at what is written
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    nnz = col.size
    pbuf = torch.full((nnz + 2, H), 9.0, device=DEV)
    dbuf = torch.full((nnz + 2, H), 9.0, device=DEV)
    nb = lib.psa_attention_workspace_bytes(nnz, H, F)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
    rp, cl, qb, kb, vb, gb = dev(rowptr), dev(col), bf(q), bf(k), bf(v), bf(g)
    _lib.check(lib.psa_attention_half_bw_entries(PSA_BF16(), rp.data_ptr(), cl.data_ptr(), qb.data_ptr(), kb.data_ptr(),
                                                 vb.data_ptr(), None, 1, 0.5, gb.data_ptr(), out.data_ptr(),
                                                 stat.data_ptr(), M, N, H, K, F, nnz, pbuf[1:].data_ptr(),
                                                 dbuf[1:].data_ptr(), ws.data_ptr(), nb,
                                                 torch.cuda.current_stream().cuda_stream))
    for buf in (pbuf, dbuf):
        assert bool((buf[0] == 9).all()) and bool((buf[-1] == 9).all()) and not bool((buf[1:-1] == 9).any())


# ---- 8. saved tensors, reproducibility, graph replay -----------------------------------------------

def test_saved_tensors_are_half_width_and_none_has_nnz_rows(general):
    rowptr, col = general
    M, nnz = rowptr.size - 1, col.size
    H, K, F = 8, 16, 16
    assert nnz not in (M, N, H, K, F, 2)
    rng = np.random.default_rng(78)
    qd, kd, vd = (bf(bf_values(rng, s)).requires_grad_() for s in ((M, H, K), (N, H, K), (N, H, F)))
    saved = []

    def pack(t):
        saved.append((tuple(t.shape), t.dtype))
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = tensor_of(rowptr, col, N).attention(qd, kd, vd, scale=0.25)
    assert out.dtype == BF
    assert sorted(saved, key=str) == sorted([((M, H, K), BF), ((N, H, K), BF), ((N, H, F), BF), ((M, H, F), BF),
                                             ((M, H, 2), torch.float32)], key=str), saved
    out.float().sum().backward()
    assert qd.grad.dtype == BF and kd.grad.dtype == BF and vd.grad.dtype == BF


def test_two_runs_give_the_same_bits_and_a_graph_replays_them(general):
    from paddle_sparse_amd import ops

    rowptr, col = general
    M, nnz = rowptr.size - 1, col.size
    H, K, F = 8, 16, 16
    rng = np.random.default_rng(79)

    def normal(*shape, dtype=BF):
        return dev(rng.normal(size=shape).astype(np.float32)).to(dtype)

    q, k, v, g = normal(M, H, K), normal(N, H, K), normal(N, H, F), normal(M, H, F)
    bias = normal(nnz, H, dtype=torch.float32)
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
        assert a.dtype == BF and torch.equal(a, b)

    def step():  # what the autograd Function runs, forward and backward
        out, stat = ops.attention_raw(rp, cl, q, k, v, bias, 0.25)
        return (out,) + ops.attention_bw(rp, cl, q, k, v, bias, 0.25, g, out, stat, csc)

    eager = step()
    assert eager[4].dtype == torch.float32 and eager[4].shape == (nnz, H)  # grad_bias
    for a, b in zip(first, eager):
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
        t.copy_(normal(*t.shape, dtype=t.dtype))
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(captured, step()):
        assert torch.equal(got, want)


# ---- 9. errors and small behaviours ----------------------------------------------------------------

def test_bare_pattern_equals_the_tensor_form_and_only_requested_gradients_are_made(general):
    from paddle_sparse_amd import ops

    rowptr, col = general
    M = rowptr.size - 1
    H, K, F = 3, 5, 7
    rng = np.random.default_rng(80)
    q, k, v, g = (bf_values(rng, s) for s in ((M, H, K), (N, H, K), (N, H, F), (M, H, F)))
    want = run(tensor_of(rowptr, col, N), q, k, v, g, 0.5)
    qd, kd, vd = (bf(a).requires_grad_() for a in (q, k, v))
    out = ops.attention(dev(rowptr), dev(col), qd, kd, vd, scale=0.5)  # no CSC view: the backward sorts col
    out.backward(bf(g))
    for a, b in zip(want, (out.detach(), qd.grad, kd.grad, vd.grad)):
        assert torch.equal(a, b)

    q1, k1, v1 = bf(q), bf(k), bf(v).requires_grad_()
    out = ops.attention(dev(rowptr), dev(col), q1, k1, v1, scale=0.5)
    out.backward(bf(g))
    assert q1.grad is None and k1.grad is None and torch.equal(v1.grad, want[3])
    got = ops.attention_bw(dev(rowptr), dev(col), q1, k1, v1.detach(), None, 0.5, bf(g), *ops.attention_raw(
        dev(rowptr), dev(col), q1, k1, v1.detach(), scale=0.5), want=(True, False, False, True))
    assert torch.equal(got[0], want[1]) and got[1] is None and got[2] is None and got[3] is None


def test_errors():
    from paddle_sparse_amd import ops

    rowptr = np.array([0, 1, 2], dtype=np.int64)
    col = np.array([0, 2], dtype=np.int64)
    A = tensor_of(rowptr, col, 3)
    H, K, F = 2, 4, 4
    q = torch.zeros(2, H, K, dtype=BF, device=DEV)
    k = torch.zeros(3, H, K, dtype=BF, device=DEV)
    v = torch.ones(3, H, F, dtype=BF, device=DEV)
    assert A.attention(q, k, v).dtype == BF
    for bad in ((q.float(), k, v), (q, k.float(), v), (q, k, v.float()), (q, k, v.half()), (q.float(), k.float(), v)):
        with pytest.raises(TypeError):
            A.attention(*bad)  # mixed dtypes
        with pytest.raises(TypeError):
            ops.attention(dev(rowptr), dev(col), *bad)
    with pytest.raises(TypeError):
        A.attention(q.half(), k.half(), v.half())  # fp16 is not served
    with pytest.raises(TypeError):
        ops.attention(dev(rowptr), dev(col), q.half(), k.half(), v.half())
    with pytest.raises(TypeError):
        A.attention(q.double(), k.double(), v.double())
    with pytest.raises(TypeError):
        tensor_of(rowptr, col, 3, torch.zeros(2, dtype=torch.float64, device=DEV)).attention(q, k, v, bias=True)
    with pytest.raises(TypeError):
        ops.attention(dev(rowptr), dev(col), q, k, v, bias=torch.zeros(2, dtype=torch.float64, device=DEV))
    with pytest.raises(TypeError):
        ops.attention(dev(rowptr), dev(col), q, k, v, bias=torch.zeros(2, dtype=BF, device=DEV))  # the bias stays fp32
    with pytest.raises(RuntimeError, match="GPU tensor"):
        A.attention(q.cpu(), k, v)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.attention(dev(rowptr), dev(col), q, k, v.cpu())
    with pytest.raises(ValueError):
        A.attention(q[:, 0], k, v)  # mixed ranks
    # an fp32 bias [nnz] with bf16 operands, 2-D form
    out = tensor_of(rowptr, col, 3, torch.zeros(2, device=DEV)).attention(q[:, 0], k[:, 0], v[:, 0], bias=True)
    assert out.dtype == BF and out.shape == (2, F) and bool((out == 1).all())
