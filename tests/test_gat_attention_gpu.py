"""GPU suite of fused GAT attention (psa_gat_attention_fw / _bw_entries and their _half forms behind
SparseTensor.gat_attention and ops.gat_attention) against the float64 restatement of tests/gat_ref.py.

Exact wherever it says so, in the two regimes of tests/test_attention_gpu.py: one-hot (1, 2 or 4 winners per row and
head share the largest score, every other score is at least 512 below it after the activation, so exp underflows to
exactly 0 and p is 0 or 2^-j) and uniform (equal scores within a row, row lengths that are powers of two).  Everything
else is a small integer, so every sum stays within 24 bits and the order of the additions does not matter.  Shapes,
patterns and helpers are those of test_attention_gpu.py."""
import numpy as np
import pytest
import torch

import attention_ref as ar
import dropout_ref as dr
import gat_ref as gr
from test_attention_gpu import (LENGTHS, N, U, W_ALL, W_ODD, _col_sum, dev, ints, one_hot_data as dot_one_hot_data,
                                one_hot_pattern, pattern, tensor_of, winner_positions)

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
BF = torch.bfloat16
UB = 2.0 ** -8  # the bound for one bf16 rounding, as tests/test_attention_half_gpu.py
SLOPE = 0.25    # of the exact tests: a power of two
# (H, F), fp32: the smallest; the smallest 16-byte form; an element form with nothing a power of two; the bench widths;
# a head block of 5; four head blocks and a last one of a single head; one head wider than four tiles, in each form
FP32_SHAPES = [(1, 1), (1, 4), (3, 7), (8, 16), (8, 64), (5, 4), (65, 4), (1, 261), (1, 1028)]
BF16_SHAPES = [(1, 1), (1, 8), (3, 7), (8, 16), (8, 64), (65, 8), (1, 1032)]
ALL_SHAPES = [(F32,) + s for s in FP32_SHAPES] + [(BF,) + s for s in BF16_SHAPES]


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def to(a, dtype):
    return dev(np.ascontiguousarray(a, dtype=np.float32)).to(dtype)


def one_off(t):
    """The same numbers in a view that starts one element into its allocation."""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = base[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size()
    return view


def run(A, a_row, a_col, v, g, slope=SLOPE, bias=False, dropout_p=0.0, seed=0, dtype=F32, shift=False):
    """out and the gradients of a_row, a_col, v through the tensor form; shift: operands one element off."""
    make = (lambda a: one_off(to(a, dtype))) if shift else (lambda a: to(a, dtype))
    rd, cd, vd = (make(a).requires_grad_() for a in (a_row, a_col, v))
    out = A.gat_attention(rd, cd, vd, negative_slope=slope, bias=bias, dropout_p=dropout_p, seed=seed)
    out.backward(make(g))
    return out.detach(), rd.grad, cd.grad, vd.grad


def same(got, want, exact64=True):
    """Bit for bit.  fp32: got equals the float64 reference, or (exact64=False) the reference rounded to fp32, the
    correctly rounded result; bf16: the reference rounded to fp32 and then once to bf16."""
    if got.dtype == BF:
        return np.array_equal(host(got), gr.once_rounded(want))
    assert got.dtype == F32
    return np.array_equal(host(got), want if exact64 else want.astype(np.float32).astype(np.float64))


@pytest.fixture(scope="module")
def big():
    return pattern(np.random.default_rng(61), LENGTHS, N)


@pytest.fixture(scope="module")
def one_hot():
    return one_hot_pattern(np.random.default_rng(71))


# ---- the derived bounds (tests 1 at dropout_p = 0.25, and 4) ---------------------------------------

def gat_bounds(rowptr, col, a_row, a_col, v, g, slope, bias, dropout_p, seed, half, exact_weights=False):
    """(wants, bounds) for out, grad_a_row, grad_a_col, grad_v (and grad_bias with a bias); the float64 reference is
    fed the inputs the kernels get.  u = 2^-24, ub = 2^-8 (bf16 results only), len = the row's length, clen = the
    column's, D = keep * inv_keep (1 without dropout).  The derivation is that of
    tests/test_attention_gpu.py::test_general_values_within_the_derived_bounds with another score:

    Score.  z is two rounded additions and s at most one rounded product of it; the activation is Lipschitz with
            constant max(1, |slope|), also across z = 0: |s^ - s| <= 3 u max(1, |slope|) (|a_row| + |a_col| + |bias|).
            Delta[r, h] is its maximum over the row; it takes the place of (K + 2) u scale sum |q k|.
    Weight. eps[r, h] = 2 Delta + (len + 64) u bounds |p^ - p| / p, forward and backward.
    out.    (eps + du) sum_e p D |v|, du = u for the multiply by inv_keep with dropout, 0 without; + ub |out| (bf16).
    grad_v. sum_{e in col} (eps[row e] + du + (clen + 2) u) p D |g|; + ub |grad_v|.
    dS = p (D dP - delta).  D_dP = (F + 2) u D sum_f |g v| (+ u D sum_f |g v| with dropout), D_delta = (F + 2) u
            sum_f |g| |out| + sum_f |g| (eps + du) sum_e p D |v| + ub sum_f |g| |out| (delta is taken from the rounded out),
            D_dS = eps p |dP - delta| + p (D_dP + D_delta) + 4 u p (|dP| + |delta|).
    dZ = dS * (1 or slope): one more rounding.  D_dZ = |factor| D_dS + u |dZ|.  The factor itself is that of the
            reference wherever the sign of z^ is that of z: one addition keeps the sign; with a bias the callers
            check that no |z| is within 2 u (|a_row| + |a_col| + |bias|) of 0, a condition on the inputs.
    grad_a_row.  A sum of len terms of dZ^: sum_e D_dZ + (len + 1) u sum_e |dZ|; + ub |grad_a_row|.
    grad_a_col.  A sum of clen terms: sum_{e in col} D_dZ + (clen + 1) u sum |dZ|; + ub |grad_a_col|.
    grad_bias.   fp32.  [nnz, H]: D_dZ.  [nnz]: the sum of H terms, sum_h D_dZ + H u sum_h |dZ|.

    exact_weights (the one-hot regime): the scores are exact, exp(0) = 1 and exp(below -512) = 0 exactly, l is a
    small integer, so p^ = p: Delta = 0 and eps = 0.  An entry of weight 0 adds an exact 0 to every sum, which rounds
    nothing: len and clen become the numbers of entries with p > 0 in the row and the column, per head."""
    M, H = a_row.shape
    F = v.shape[2]
    row = ar.rows_of(rowptr)
    want = gr.gat_ref(rowptr, col, a_row, a_col, v, slope, bias, dropout_p, seed)
    grads = gr.gat_grads_ref(rowptr, col, a_row, a_col, v, g, slope, bias, dropout_p, seed)
    p, pd, dz = grads["p"], grads["pd"], grads["dz"]
    D = gr._d(col.size, H, dropout_p, seed)
    ub = UB if half else 0.0
    du = U if dropout_p else 0.0
    r64, c64, v64, g64 = (a.astype(np.float64) for a in (a_row, a_col, v, g))
    length = np.diff(rowptr).astype(np.float64)
    clen = np.bincount(col, minlength=N).astype(np.float64)
    mag = np.abs(r64[row]) + np.abs(c64[col])
    if bias is not None:
        b64 = np.abs(bias.astype(np.float64))
        mag = mag + (b64[:, None] if b64.ndim == 1 else b64)
        z = gr.z_ref(rowptr, col, r64, c64, bias)
        assert np.all(np.abs(z) > 2 * U * mag)  # the sign of z is not in doubt: a condition on the inputs
    Delta = np.zeros((M, H))
    np.maximum.at(Delta, row, 3 * U * max(1.0, abs(slope)) * mag)
    eps = 2 * Delta + (length[:, None] + 64) * U
    len_e, clen_e = length[row, None], clen[col, None]  # [nnz, 1]: the terms of the sum an entry belongs to
    if exact_weights:
        eps = np.zeros((M, H))
        live = (p > 0).astype(np.float64)
        n_row = np.zeros((M, H))
        np.add.at(n_row, row, live)
        len_e, clen_e = n_row[row], _col_sum(col, N, live)[col]  # [nnz, H]
    pv = np.zeros((M, H, F))
    np.add.at(pv, row, pd[:, :, None] * np.abs(v64[col]))
    f_out = (eps + du)[:, :, None] * pv
    b_out = f_out + ub * np.abs(want)
    b_gv = _col_sum(col, N, ((eps[row] + du + (clen_e + 2) * U) * pd)[:, :, None] * np.abs(g64[row])) + \
        ub * np.abs(grads["v"])
    gv_abs = np.einsum("ehf,ehf->eh", np.abs(g64[row]), np.abs(v64[col]))
    dp = D * np.einsum("ehf,ehf->eh", g64[row], v64[col])
    delta = np.einsum("mhf,mhf->mh", g64, want)
    g_out = np.einsum("mhf,mhf->mh", np.abs(g64), np.abs(want))
    d_dp = ((F + 2) * U + du) * D * gv_abs
    d_delta = (F + 2) * U * g_out + np.einsum("mhf,mhf->mh", np.abs(g64), f_out) + ub * g_out
    d_ds = eps[row] * p * np.abs(dp - delta[row]) + p * (d_dp + d_delta[row]) + \
        4 * U * p * (np.abs(dp) + np.abs(delta[row]))
    fac = np.where(gr.z_ref(rowptr, col, r64, c64, bias) > 0, 1.0, abs(slope))
    d_dz = fac * d_ds + U * np.abs(dz)
    b_gr = np.zeros((M, H))
    np.add.at(b_gr, row, d_dz + (len_e + 1) * U * np.abs(dz))
    b_gr += ub * np.abs(grads["a_row"])
    b_gc = _col_sum(col, N, d_dz + (clen_e + 1) * U * np.abs(dz)) + ub * np.abs(grads["a_col"])
    wants = [want, grads["a_row"], grads["a_col"], grads["v"]]
    bounds = [b_out, b_gr, b_gc, b_gv]
    if bias is not None:
        wants.append(grads["bias"])
        bounds.append(d_dz if bias.ndim == 2 else d_dz.sum(axis=1) + H * U * np.abs(dz).sum(axis=1))
    return wants, bounds


def worst(got, wants, bounds):
    return [float(np.max(np.abs(host(t) - w) / np.maximum(b, 1e-300))) for t, w, b in zip(got, wants, bounds)]


# ---- 1. exact, one-hot regime ----------------------------------------------------------------------

def one_hot_data(rng, M, H, F):
    """a_row in [-3, 3].  Even heads: the winners share a_col = 32, so z in [29, 35] > 0 and s = z.  Odd heads: the
    winners share a_col = -32, so z in [-35, -29], s = z / 4 and the gradient factor is the slope.  Every loser has
    a_col = -4096 - 32 j: s <= (3 - 4096) / 4, at least 1000 below either kind of winner.  All are bf16 numbers."""
    a_row = ints(rng, (M, H), -3, 3)
    a_col = -4096 - 32 * ints(rng, (N, H), 0, 3)
    for h in range(H):
        a_col[W_ALL if h % 2 == 0 else W_ODD, h] = 32 if h % 2 == 0 else -32
    return a_row, a_col, ints(rng, (N, H, F), -2, 2), ints(rng, (M, H, F), -2, 2)


def check_one_hot(rowptr, col, a_row, a_col, bias=None):
    """Conditions on the construction: the winners' branch per head, the gap, p in {0, 1, 1/2, 1/4}."""
    row = ar.rows_of(rowptr)
    z = gr.z_ref(rowptr, col, a_row, a_col, bias)
    s = gr.act_ref(z, SLOPE)
    top = np.full((rowptr.size - 1, s.shape[1]), -np.inf)
    np.fmax.at(top, row, s)
    win = s == top[row]
    assert np.all(win | (s <= top[row] - 512))
    p = ar.softmax_ref(rowptr, s)[0]
    assert set(np.unique(p)) <= {0.0, 1.0, 0.5, 0.25}  # the float64 reference underflows to exactly 0 as well
    return z, win


@pytest.mark.parametrize("dropout_p", [0.0, 0.25, 0.5])
@pytest.mark.parametrize("dtype,H,F", ALL_SHAPES)
def test_one_hot_exact(one_hot, dtype, H, F, dropout_p):
    """p is 0 or 1 / (1, 2 or 4), out a multiple of 1/4, stat = {the winners' s, their number}, dP, delta, dS and dZ
    = dS or dS / 4 dyadic rationals within 24 bits: out, stat and the three gradients equal the float64 reference
    bit for bit (bf16: rounded once), without dropout and with dropout_p = 0.5, where inv_keep = 2 is exact too.

    dropout_p = 0.25: inv_keep = float32(4 / 3) is no power of two.  out = fl(x * inv_keep) with x exact is the
    correctly rounded product, so out still equals the reference rounded to fp32 bit for bit, stat does not change,
    and the entries dropped are visible exactly (grad_v is exactly 0 wherever no kept entry reaches it).  But delta sums
    F rounded products and dS, dZ and the gradient sums round again, where the reference rounds once: no arithmetic
    in fp32 gives the bits of the rounded float64 gradients, so these are held to gat_bounds with exact weights (a few u of the terms'
    magnitudes; the ratios are printed)."""
    from paddle_sparse_amd import ops

    rowptr, col = one_hot
    M = rowptr.size - 1
    seed = 12345
    a_row, a_col, v, g = one_hot_data(np.random.default_rng(100 * H + F), M, H, F)
    z, win = check_one_hot(rowptr, col, a_row, a_col)
    for h in range(H):
        assert np.all(z[win[:, h], h] > 0) if h % 2 == 0 else np.all(z[win[:, h], h] < 0)
    want = gr.gat_ref(rowptr, col, a_row, a_col, v, SLOPE, None, dropout_p, seed)
    want_stat = gr.gat_stat_ref(rowptr, col, a_row, a_col, v, SLOPE)
    grads = gr.gat_grads_ref(rowptr, col, a_row, a_col, v, g, SLOPE, None, dropout_p, seed)
    assert np.abs(grads["dz"]).max() > 0 or H * F == 1

    A = tensor_of(rowptr, col, N)
    out, g_r, g_c, g_v = run(A, a_row, a_col, v, g, dropout_p=dropout_p, seed=seed, dtype=dtype)
    assert out.shape == (M, H, F) and out.dtype == dtype and not host(out)[0].any()
    out_raw, stat = ops.gat_attention_raw(dev(rowptr), dev(col), to(a_row, dtype), to(a_col, dtype), to(v, dtype),
                                          negative_slope=SLOPE, dropout_p=dropout_p, seed=seed)
    assert torch.equal(out_raw, out)
    assert stat.dtype == F32 and stat.shape == (M, H, 2) and np.array_equal(host(stat), want_stat)
    got = (g_r, g_c, g_v)
    names = ("a_row", "a_col", "v")
    if dropout_p != 0.25:
        assert same(out, want)
        for t, name in zip(got, names):
            assert t.dtype == dtype and same(t, grads[name]), name
        return
    assert same(out, want, exact64=False)
    wants, bounds = gat_bounds(rowptr, col, a_row, a_col, v, g, SLOPE, None, dropout_p, seed, dtype == BF,
                               exact_weights=True)
    print(f"gat one-hot dropout 0.25 {dtype} ({H}, {F}): worst err / bound  " +
          "  ".join(f"grad_{n} {r:.4f}" for n, r in zip(names, worst(got, wants[1:], bounds[1:]))))
    for t, w, b in zip(got, wants[1:], bounds[1:]):
        assert np.all(np.abs(host(t) - w) <= b)
    # what the mask removed is removed exactly: a column and head none of whose kept entries has a weight gets 0
    reach = _col_sum(col, N, grads["pd"][:, :, None] * np.abs(g[ar.rows_of(rowptr)]).astype(np.float64))
    assert (reach == 0).any() and not host(g_v)[reach == 0].any()


def test_one_hot_exact_one_head_form(one_hot):
    rowptr, col = one_hot
    M, F = rowptr.size - 1, 7
    a_row, a_col, v, g = one_hot_data(np.random.default_rng(200), M, 1, F)
    a_row, a_col, v, g = a_row[:, 0], a_col[:, 0], v[:, 0], g[:, 0]
    want = gr.gat_ref(rowptr, col, a_row, a_col, v, SLOPE)
    grads = gr.gat_grads_ref(rowptr, col, a_row, a_col, v, g, SLOPE)
    A = tensor_of(rowptr, col, N)
    out, g_r, g_c, g_v = run(A, a_row, a_col, v, g)
    assert out.shape == (M, F) and g_r.shape == (M,) and g_c.shape == (N,) and g_v.shape == (N, F)
    assert same(out, want) and same(g_r, grads["a_row"]) and same(g_c, grads["a_col"]) and same(g_v, grads["v"])
    heads = A.gat_attention(dev(a_row)[:, None], dev(a_col)[:, None], dev(v)[:, None], negative_slope=SLOPE)
    assert torch.equal(heads[:, 0], out)


# ---- 2. exact, uniform regime ----------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("case", ["negative", "zero", "slope0"])
def test_uniform_exact(case, dtype):
    """a_col identical across the nodes per head: equal scores within a row and head, row lengths the powers of two
    1 .. 256 plus an empty row.  p = 1 / len, out has a granularity of 2^-8, dP and delta are at most 16 with v in
    [-2, 2] and g in [-1, 1], dZ = dS * slope is a shift, and the sums over a column stay within 23 bits; the sum of
    dZ over a row is exactly 0.
      negative: a_col = -32, slope = 1/2: z < 0 throughout.
      zero:     a_row = 32, a_col = -32, slope = 1/2: z == 0 exactly, and the factor at zero is the slope.
      slope0:   a_col = 0, slope = 0: rows with a_row > 0 have the factor 1, the others s = -0 or 0 and dZ = 0."""
    rng = np.random.default_rng(72)
    lens = [1, 2, 4, 8, 16, 32, 64, 128, 256, 0, 4, 2, 256, 1]
    M, n, H, F = len(lens), 300, 3, 8
    rowptr, col = pattern(rng, lens, n)
    a_row = ints(rng, (M, H), -3, 3)
    slope, c = (0.0, 0.0) if case == "slope0" else (0.5, -32.0)
    if case == "zero":
        a_row[:] = 32
    a_col = np.full((n, H), c, dtype=np.float32)
    v, g = ints(rng, (n, H, F), -2, 2), ints(rng, (M, H, F), -1, 1)
    z = gr.z_ref(rowptr, col, a_row, a_col)
    assert {"negative": np.all(z < 0), "zero": np.all(z == 0), "slope0": (z > 0).any() and (z <= 0).any()}[case]
    want = gr.gat_ref(rowptr, col, a_row, a_col, v, slope)
    grads = gr.gat_grads_ref(rowptr, col, a_row, a_col, v, g, slope)
    assert np.abs(grads["ds"]).max() > 0
    if dtype == BF:  # a condition on the construction: out is a bf16 number, so the delta of the backward is exact
        import bf16_ref
        assert bf16_ref.is_bf16(want).all()
    if case != "slope0":
        assert np.array_equal(grads["dz"], grads["ds"] / 2) and np.abs(grads["a_col"]).max() > 0
    A = tensor_of(rowptr, col, n)
    out, g_r, g_c, g_v = run(A, a_row, a_col, v, g, slope=slope, dtype=dtype)
    assert same(out, want) and not host(out)[9].any()
    assert not host(g_r).any() and not np.abs(grads["a_row"]).max() > 1e-12
    assert same(g_c, grads["a_col"]) and same(g_v, grads["v"])


# ---- 3. bias ---------------------------------------------------------------------------------------

def bias_case(rng, rowptr, col, H, F, low, per_head):
    """Equal a_row + a_col within a row and head (a_col identical across the nodes: 32 on the even heads, -32 on
    the odd ones, so both branches are met); the bias alone makes the winners, 0 against `low`.  Per-head form: odd
    heads keep only the last winner of a row."""
    M, nnz = rowptr.size - 1, col.size
    a_row = ints(rng, (M, H), -3, 3)
    a_col = np.tile(np.where(np.arange(H) % 2 == 0, 32.0, -32.0).astype(np.float32), (N, 1))
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
    return a_row, a_col, v, g, bias


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("low", [-8192.0, float("-inf")])
@pytest.mark.parametrize("per_head", [False, True])
def test_bias_makes_the_winners_exact(big, per_head, low, dtype):
    """The bias is added inside the activation: losers have z = a_row + a_col - 8192 and s = z / 4 <= -2000, or
    z = s = -inf (slope 1/4 > 0: a mask).  grad_bias is dZ, fp32 for either dtype: the full [nnz, H], or summed over
    the heads for [nnz]; the tracked stored values receive it through the tensor form."""
    from paddle_sparse_amd import ops

    rowptr, col = big
    H, F = 3, 8
    a_row, a_col, v, g, bias = bias_case(np.random.default_rng(73), rowptr, col, H, F, low, per_head)
    check_one_hot(rowptr, col, a_row, a_col, bias)
    want = gr.gat_ref(rowptr, col, a_row, a_col, v, SLOPE, bias)
    grads = gr.gat_grads_ref(rowptr, col, a_row, a_col, v, g, SLOPE, bias)
    assert np.abs(grads["bias"]).max() > 0 and np.isfinite(grads["bias"]).all()
    bd = dev(bias).requires_grad_()
    A = tensor_of(rowptr, col, N, bd)
    out, g_r, g_c, g_v = run(A, a_row, a_col, v, g, bias=True, dtype=dtype)
    assert same(out, want)
    assert bd.grad.dtype == F32 and bd.grad.shape == bias.shape and same(bd.grad, grads["bias"])
    assert same(g_r, grads["a_row"]) and same(g_c, grads["a_col"]) and same(g_v, grads["v"])
    if low == float("-inf") and not per_head:
        # a -inf entry has weight exactly 0: the bits of the pattern without it, forward and grad_v, and p == 0
        keep = bias == 0
        row = ar.rows_of(rowptr)
        rowptr_b = np.concatenate([[0], np.cumsum(np.bincount(row[keep], minlength=rowptr.size - 1))]).astype(np.int64)
        B = tensor_of(rowptr_b, col[keep], N, dev(bias[keep]))
        out_b, _, _, g_v_b = run(B, a_row, a_col, v, g, bias=True, dtype=dtype)
        assert torch.equal(out_b, out) and torch.equal(g_v_b, g_v)
        rp, cl = dev(rowptr), dev(col)
        ops_in = (to(a_row, dtype), to(a_col, dtype), to(v, dtype))
        _, stat = ops.gat_attention_raw(rp, cl, *ops_in, bias=dev(bias), negative_slope=SLOPE)
        p, dz = ops._gat_bw_entries_raw(rp, cl, *ops_in, dev(bias), SLOPE, to(g, dtype), out, stat)
        masked = torch.from_numpy(~keep).to(DEV)
        assert not p[masked].any() and not dz[masked].any() and bool((p[~masked] > 0).all())


def test_stored_values_are_ignored_without_bias(big):
    rowptr, col = big
    rng = np.random.default_rng(74)
    M, H, F = rowptr.size - 1, 2, 4
    a_row, a_col, v = (dev(rng.normal(size=s).astype(np.float32)) for s in ((M, H), (N, H), (N, H, F)))
    plain = tensor_of(rowptr, col, N).gat_attention(a_row, a_col, v)
    nan = tensor_of(rowptr, col, N, torch.full((col.size,), float("nan"), device=DEV))
    assert torch.equal(nan.gat_attention(a_row, a_col, v), plain) and not torch.isnan(plain).any()
    assert torch.isnan(nan.gat_attention(a_row, a_col, v, bias=True)[1:]).all()


# ---- 4. general values -----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("bias_form", ["none", "shared", "per_head"])
@pytest.mark.parametrize("slope", [0.2, -0.5])
@pytest.mark.parametrize("H,F", [(1, 64), (8, 16), (3, 7)])
def test_general_values_within_the_derived_bounds(big, H, F, slope, bias_form, dtype):
    """Normal a_row, a_col, v, g (bf16: rounded to bf16 first, and the reference is fed those values) and a normal
    fp32 bias; the bounds and their derivation are gat_bounds'.  Prints worst error / bound for the fused op and,
    for fp32, for the unfused chain (torch indexing, torch.where, segment_softmax, spmm_heads) on the same inputs;
    only the fused op is held to the bounds."""
    import bf16_ref
    from paddle_sparse_amd import ops

    rowptr, col = big
    M, nnz = rowptr.size - 1, col.size
    rng = np.random.default_rng(75 + H)
    a_row, a_col, v, g = (rng.normal(size=s).astype(np.float32) for s in ((M, H), (N, H), (N, H, F), (M, H, F)))
    if dtype == BF:
        a_row, a_col, v, g = (bf16_ref.round_bf16(a).astype(np.float32) for a in (a_row, a_col, v, g))
    bias = {"none": None, "shared": rng.normal(size=nnz).astype(np.float32),
            "per_head": rng.normal(size=(nnz, H)).astype(np.float32)}[bias_form]
    wants, bounds = gat_bounds(rowptr, col, a_row, a_col, v, g, slope, bias, 0.0, 0, dtype == BF)
    names = ("out", "grad_a_row", "grad_a_col", "grad_v", "grad_bias")

    bd = None if bias is None else dev(bias).requires_grad_()
    got = list(run(tensor_of(rowptr, col, N, bd), a_row, a_col, v, g, slope=slope, bias=bias is not None, dtype=dtype))
    assert all(t.dtype == dtype for t in got)
    if bias is not None:
        assert bd.grad.dtype == F32 and bd.grad.shape == bias.shape
        got.append(bd.grad)
    tag = f"gat {dtype} ({H}, {F}) slope {slope} bias {bias_form}"
    print(f"{tag} fused: worst err / bound  " + "  ".join(f"{n} {r:.4f}" for n, r in zip(names, worst(got, wants, bounds))))
    if dtype == F32:
        rp, cl, rowi = dev(rowptr), dev(col), dev(ar.rows_of(rowptr))
        rd, cd, vd = (dev(a).requires_grad_() for a in (a_row, a_col, v))
        bc = None if bias is None else dev(bias).requires_grad_()
        zc = rd[rowi] + cd[cl]
        if bc is not None:
            zc = zc + (bc[:, None] if bc.dim() == 1 else bc)
        out_c = ops.spmm_heads(rp, cl, ops.segment_softmax(torch.where(zc > 0, zc, slope * zc), rp), vd)
        out_c.backward(dev(g))
        chain = [out_c.detach(), rd.grad, cd.grad, vd.grad] + ([] if bc is None else [bc.grad])
        print(f"{tag} chain: worst err / bound  " +
              "  ".join(f"{n} {r:.4f}" for n, r in zip(names, worst(chain, wants, bounds))))
    for t, w, b in zip(got, wants, bounds):
        assert np.all(np.abs(host(t) - w) <= b)


# ---- 5. the mask of the dot-product op -------------------------------------------------------------

def test_same_mask_as_the_dot_product_op(one_hot):
    """v, g > 0, so a (row, head) of out is exactly 0 only where every winner of it was dropped (and in the row
    without entries), and a (column, head) of grad_v only where every winner of that column was: the same sets in
    fp32 and bf16, in the reference with the numpy mask, from ops.attention_dropout_mask, and, for out, in the
    dot-product op on the same winners."""
    from paddle_sparse_amd import ops

    rowptr, col = one_hot
    M, H, F = rowptr.size - 1, 8, 8
    rng = np.random.default_rng(82)
    a_row, a_col, _, _ = one_hot_data(rng, M, H, F)
    q, k, _, _ = dot_one_hot_data(rng, M, H, 8, F)
    v, g = ints(rng, (N, H, F), 1, 2), ints(rng, (M, H, F), 1, 2)
    _, win = check_one_hot(rowptr, col, a_row, a_col)
    row = ar.rows_of(rowptr)
    A = tensor_of(rowptr, col, N)
    seen = 0
    for seed in (0, 12345, 2 ** 63 - 1):
        want = gr.gat_ref(rowptr, col, a_row, a_col, v, SLOPE, None, 0.5, seed)
        want_gv = gr.gat_grads_ref(rowptr, col, a_row, a_col, v, g, SLOPE, None, 0.5, seed)["v"]
        zero, zero_gv = (want == 0).all(axis=2), (want_gv == 0).all(axis=2)
        mask = ops.attention_dropout_mask(col.size, H, 0.5, seed).cpu().numpy()
        assert np.array_equal(mask, dr.keep_ref(col.size, H, 0.5, seed))
        alive = np.zeros((M, H), dtype=bool)
        np.logical_or.at(alive, row, win & mask)
        assert np.array_equal(~alive, zero)
        for dtype in (F32, BF):
            out, _, _, g_v = run(A, a_row, a_col, v, g, dropout_p=0.5, seed=seed, dtype=dtype)
            assert np.array_equal((out == 0).all(dim=2).cpu().numpy(), zero)
            assert np.array_equal((g_v == 0).all(dim=2).cpu().numpy(), zero_gv)
        dot = A.attention(dev(q), dev(k), dev(v), dropout_p=0.5, seed=seed)
        assert np.array_equal((dot == 0).all(dim=2).cpu().numpy(), zero)
        seen += int(zero[1:].sum())
    assert seen > 8  # single winners were dropped somewhere


@pytest.mark.parametrize("dtype", [F32, BF])
def test_dropout_zero_is_the_op_without_dropout_and_draws_nothing(big, dtype):
    from paddle_sparse_amd import ops

    rowptr, col = big
    M, H, F = rowptr.size - 1, 8, 16
    rng = np.random.default_rng(90)
    a_row, a_col, v = (to(rng.normal(size=s), dtype) for s in ((M, H), (N, H), (N, H, F)))
    rp, cl = dev(rowptr), dev(col)
    torch.manual_seed(5)
    state = torch.get_rng_state()
    plain = ops.gat_attention(rp, cl, a_row, a_col, v)
    assert torch.equal(ops.gat_attention(rp, cl, a_row, a_col, v, dropout_p=0.0, seed=None), plain)
    assert torch.equal(ops.gat_attention(rp, cl, a_row, a_col, v, dropout_p=0.0, seed=77), plain)
    assert torch.equal(torch.get_rng_state(), state)
    dropped = ops.gat_attention(rp, cl, a_row, a_col, v, dropout_p=0.5)  # seed=None: drawn from the CPU generator
    assert not torch.equal(torch.get_rng_state(), state) and not torch.equal(dropped, plain)
    # stat comes before the dropout
    assert torch.equal(ops.gat_attention_raw(rp, cl, a_row, a_col, v, dropout_p=0.5, seed=3)[1],
                       ops.gat_attention_raw(rp, cl, a_row, a_col, v)[1])


# ---- 6. non-finite values --------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF])
def test_non_finite_reaches_its_row_and_head_only(big, dtype):
    import bf16_ref

    rowptr, col = big
    M, nnz = rowptr.size - 1, col.size
    H, F = 3, 8
    rng = np.random.default_rng(76)
    a_row, a_col, v, g = (bf16_ref.round_bf16(rng.normal(size=s).astype(np.float32)).astype(np.float32)
                          for s in ((M, H), (N, H), (N, H, F), (M, H, F)))
    bias = np.zeros((nnz, H), dtype=np.float32)
    row = ar.rows_of(rowptr)
    a_row[13, 0] = np.nan                                 # a NaN in a_row: row 13 (4099 entries), head 0
    bias[rowptr[12] + 700, 1] = np.inf                    # a +inf score: row 12 (1024 entries), head 1
    bias[rowptr[9]:rowptr[10], 2] = -np.inf               # nothing but -inf: row 9 (255 entries), head 2
    bias[rowptr[5]:rowptr[6], 0] = -np.inf                # ... and a short row: row 5, head 0
    bias[rowptr[10] + 3, 1] = -np.inf                     # a mask among finite scores: weight exactly 0
    c_inf = int(col[rowptr[11] + 5])
    a_col[c_inf, 2] = np.inf                              # a +inf in a_col: every row that holds the column, head 2
    bad = np.zeros((M, H), dtype=bool)
    bad[13, 0] = bad[12, 1] = bad[9, 2] = bad[5, 0] = True
    bad[row[col == c_inf], 2] = True
    want = gr.gat_ref(rowptr, col, a_row, a_col, v, 0.2, bias)
    assert np.array_equal(np.isnan(want).all(axis=2), bad) and np.array_equal(np.isnan(want).any(axis=2), bad)

    bd = dev(bias).requires_grad_()
    A = tensor_of(rowptr, col, N, bd)
    rd, cd, vd = (to(a, dtype).requires_grad_() for a in (a_row, a_col, v))
    out = A.gat_attention(rd, cd, vd, negative_slope=0.2, bias=True)
    got = host(out)
    assert np.array_equal(np.isnan(got).all(axis=2), bad) and np.array_equal(~np.isfinite(got).all(axis=2), bad)
    tol = dict(rtol=1e-4, atol=1e-5) if dtype == F32 else dict(rtol=2 ** -7, atol=2 ** -7)
    assert np.allclose(got[~bad], want[~bad], **tol)
    out.backward(to(g, dtype))
    assert bd.grad[rowptr[10] + 3, 1] == 0  # the masked entry
    g_r = host(rd.grad)
    assert np.array_equal(np.isnan(g_r), bad) and not g_r[0].any()  # the row without entries gets zeros
    # negative_slope = 0: the same -inf bias is 0 * -inf = NaN and poisons its row and head (documented)
    out0 = host(A.gat_attention(rd.detach(), cd.detach(), vd.detach(), negative_slope=0.0, bias=True))
    bad0 = bad.copy()
    bad0[10, 1] = True
    assert np.array_equal(np.isnan(out0).all(axis=2), bad0) and np.array_equal(~np.isfinite(out0).all(axis=2), bad0)


@pytest.mark.parametrize("dtype", [F32, BF])
def test_the_row_without_entries(big, dtype):
    from paddle_sparse_amd import ops

    rowptr, col = big
    M, H, F = rowptr.size - 1, 3, 7
    rng = np.random.default_rng(77)
    a_row, a_col, v, g = (rng.normal(size=s).astype(np.float32) for s in ((M, H), (N, H), (N, H, F), (M, H, F)))
    out, stat = ops.gat_attention_raw(dev(rowptr), dev(col), to(a_row, dtype), to(a_col, dtype), to(v, dtype))
    assert out.shape == (M, H, F) and stat.shape == (M, H, 2) and stat.dtype == F32
    assert not out[0].any() and bool((stat[0, :, 0] == float("-inf")).all()) and not stat[0, :, 1].any()
    grads = run(tensor_of(rowptr, col, N), a_row, a_col, v, g, slope=0.2, dtype=dtype)
    assert all(bool(torch.isfinite(t).all()) for t in grads) and not grads[1][0].any()
    # a matrix of nothing but rows without entries
    rp0, cl0 = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV)
    out0, stat0 = ops.gat_attention_raw(rp0, cl0, to(a_row[:3], dtype), to(a_col, dtype), to(v, dtype))
    assert not out0.any() and bool((stat0[..., 0] == float("-inf")).all()) and not stat0[..., 1].any()


# ---- 7. no per-entry state -------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF])
def test_nothing_with_nnz_rows_is_saved(big, dtype):
    rowptr, col = big
    M, nnz = rowptr.size - 1, col.size
    H, F = 8, 16
    assert nnz not in (M, N, H, F, 2)
    rng = np.random.default_rng(78)
    rd, cd, vd = (to(rng.normal(size=s), dtype).requires_grad_() for s in ((M, H), (N, H), (N, H, F)))
    saved = []

    def pack(t):
        saved.append((tuple(t.shape), t.dtype))
        return t

    A = tensor_of(rowptr, col, N)
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = A.gat_attention(rd, cd, vd, dropout_p=0.1, seed=3)
    assert all(nnz not in shape for shape, _ in saved), saved
    assert sorted(saved, key=str) == sorted([((M, H), dtype), ((N, H), dtype), ((N, H, F), dtype), ((M, H, F), dtype),
                                             ((M, H, 2), F32)], key=str)
    out.sum().backward()
    assert rd.grad is not None and cd.grad is not None and vd.grad is not None


# ---- 8. reproducible and capturable ----------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF])
def test_two_runs_give_the_same_bits_and_a_graph_replays_them(big, dtype):
    from paddle_sparse_amd import ops

    rowptr, col = big
    M, nnz = rowptr.size - 1, col.size
    H, F = 8, 16
    rng = np.random.default_rng(79)

    def normal(*shape):
        return to(rng.normal(size=shape), dtype)

    a_row, a_col, v, g = normal(M, H), normal(N, H), normal(N, H, F), normal(M, H, F)
    bias = dev(rng.normal(size=(nnz, H)).astype(np.float32))
    A = tensor_of(rowptr, col, N, bias)
    st = A.storage
    rp, cl = st.rowptr(), st.col()
    csc = (st.colptr(), st._row_in_csc_order(), st.csr2csc())

    def autograd_step(seed):
        rd, cd, vd = (t.detach().requires_grad_() for t in (a_row, a_col, v))
        out = A.gat_attention(rd, cd, vd, bias=True, dropout_p=0.5, seed=seed)
        out.backward(g)
        return out.detach(), rd.grad, cd.grad, vd.grad

    first, second, other = autograd_step(7), autograd_step(7), autograd_step(8)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert not torch.equal(first[0], other[0])

    def step():  # what the autograd Function runs, forward and backward
        out, stat = ops.gat_attention_raw(rp, cl, a_row, a_col, v, bias, 0.2, dropout_p=0.5, seed=7)
        return (out,) + ops.gat_attention_bw(rp, cl, a_row, a_col, v, bias, 0.2, g, out, stat, csc, dropout_p=0.5,
                                             seed=7)[:3]

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
    for t in (a_row, a_col, v, g):
        t.copy_(normal(*t.shape))
    for _ in range(2):  # the same mask at every replay
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured, step()):
            assert torch.equal(got, want)


# ---- 9. bare ops.gat_attention ---------------------------------------------------------------------

def test_bare_pattern_equals_the_tensor_form_and_only_requested_gradients_are_made(big):
    from paddle_sparse_amd import ops

    rowptr, col = big
    M, H, F = rowptr.size - 1, 3, 7
    rng = np.random.default_rng(80)
    a_row, a_col, v, g = (rng.normal(size=s).astype(np.float32) for s in ((M, H), (N, H), (N, H, F), (M, H, F)))
    want = run(tensor_of(rowptr, col, N), a_row, a_col, v, g, slope=0.2)
    rd, cd, vd = (dev(a).requires_grad_() for a in (a_row, a_col, v))
    out = ops.gat_attention(dev(rowptr), dev(col), rd, cd, vd)  # no CSC view: the backward sorts col
    out.backward(dev(g))
    for a, b in zip(want, (out.detach(), rd.grad, cd.grad, vd.grad)):
        assert torch.equal(a, b)

    calls = []

    def csc():
        calls.append(1)
        return None

    r1, c1, v1 = dev(a_row).requires_grad_(), dev(a_col), dev(v)
    ops.gat_attention(dev(rowptr), dev(col), r1, c1, v1, csc=csc).backward(dev(g))
    assert not calls and c1.grad is None and v1.grad is None and torch.equal(r1.grad, want[1])
    r2, c2, v2 = dev(a_row), dev(a_col), dev(v).requires_grad_()
    ops.gat_attention(dev(rowptr), dev(col), r2, c2, v2, csc=csc).backward(dev(g))
    assert calls and r2.grad is None and c2.grad is None and torch.equal(v2.grad, want[3])


@pytest.mark.parametrize("dtype,H,F", [(F32, 8, 16), (F32, 1, 1028), (BF, 8, 16), (BF, 1, 1032)])
def test_offset_views_take_the_element_form_and_give_the_same_bits(one_hot, dtype, H, F):
    """Operands that start one element (4 / 2 bytes) into their allocation are not copied: v, out and grad_out then
    go through the element form.  In the exact regime both forms must give the reference's bits."""
    rowptr, col = one_hot
    M = rowptr.size - 1
    a_row, a_col, v, g = one_hot_data(np.random.default_rng(300 + F), M, H, F)
    A = tensor_of(rowptr, col, N)
    aligned = run(A, a_row, a_col, v, g, dropout_p=0.5, seed=9, dtype=dtype)
    shifted = run(A, a_row, a_col, v, g, dropout_p=0.5, seed=9, dtype=dtype, shift=True)
    want = gr.gat_ref(rowptr, col, a_row, a_col, v, SLOPE, None, 0.5, 9)
    assert same(aligned[0], want)
    for a, b in zip(aligned, shifted):
        assert torch.equal(a, b)


# ---- 10. argument errors ---------------------------------------------------------------------------

def test_errors():
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import ops

    H, F = 2, 3
    row, col = torch.tensor([0, 1], device=DEV), torch.tensor([1, 2], device=DEV)
    A = psa.SparseTensor(row=row, col=col, sparse_sizes=(2, 3))
    a_row, a_col, v = torch.zeros(2, H, device=DEV), torch.zeros(3, H, device=DEV), torch.ones(3, H, F, device=DEV)
    assert torch.equal(A.gat_attention(a_row, a_col, v), torch.ones(2, H, F, device=DEV))
    assert torch.equal(psa.gat_attention(A, a_row[:, 0], a_col[:, 0], v[:, 0]), torch.ones(2, F, device=DEV))
    with pytest.raises(TypeError):
        A.gat_attention(a_row.half(), a_col.half(), v.half())
    with pytest.raises(TypeError):
        A.gat_attention(a_row, a_col, v.bfloat16())  # mixed dtypes
    with pytest.raises(TypeError):
        A.gat_attention(a_row.bfloat16(), a_col, v)
    with pytest.raises(TypeError):
        A.gat_attention(a_row, a_col, [1.0])
    with pytest.raises(TypeError):
        A.gat_attention(a_row, a_col, v, bias=torch.zeros(2, device=DEV))
    with pytest.raises(ValueError):
        A.gat_attention(a_row[:, 0], a_col, v)  # mixed ranks
    with pytest.raises(ValueError):
        A.gat_attention(a_row, a_col, v[:, 0])
    with pytest.raises(ValueError):
        A.gat_attention(a_row[:, :, None], a_col[:, :, None], v[:, :, :, None])  # one rank too many
    with pytest.raises(ValueError):
        A.gat_attention(torch.zeros(2, H + 1, device=DEV), a_col, v)  # H of a_row against v
    with pytest.raises(ValueError):
        A.gat_attention(a_row, torch.zeros(3, H + 1, device=DEV), v)  # H of a_col
    with pytest.raises(ValueError):
        A.gat_attention(torch.zeros(3, H, device=DEV), a_col, v)  # M
    with pytest.raises(ValueError):
        A.gat_attention(a_row, a_col, torch.ones(2, H, F, device=DEV))  # N
    with pytest.raises(ValueError):
        A.gat_attention(a_row, a_col, v, bias=True)  # no values
    with pytest.raises(RuntimeError, match="GPU tensor"):
        A.gat_attention(a_row.cpu(), a_col, v)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        A.gat_attention(a_row, a_col, v.cpu())
    for slope in (True, "0.2", None):
        with pytest.raises(TypeError):
            A.gat_attention(a_row, a_col, v, negative_slope=slope)
    for slope in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError):
            A.gat_attention(a_row, a_col, v, negative_slope=slope)
    assert A.gat_attention(a_row, a_col, v, negative_slope=0).shape == (2, H, F)
    for p in (-0.1, 1.0, float("nan"), "0.5", True):
        with pytest.raises(ValueError):
            A.gat_attention(a_row, a_col, v, dropout_p=p)
    with pytest.raises(TypeError):
        A.gat_attention(a_row, a_col, v, dropout_p=0.5, seed=1.5)
    with pytest.raises(ValueError):
        A.gat_attention(a_row, a_col, v, dropout_p=0.5, seed=-1)
    with pytest.raises(ValueError):
        A.gat_attention(a_row, a_col, v, dropout_p=0.5, seed=1 << 64)

    def with_value(value):
        return psa.SparseTensor(row=row, col=col, value=value, sparse_sizes=(2, 3))

    assert with_value(torch.zeros(2, device=DEV)).gat_attention(a_row, a_col, v, bias=True).shape == (2, H, F)
    assert with_value(torch.zeros(2, H, device=DEV)).gat_attention(a_row, a_col, v, bias=True).shape == (2, H, F)
    with pytest.raises(ValueError):
        with_value(torch.zeros(2, H + 1, device=DEV)).gat_attention(a_row, a_col, v, bias=True)
    with pytest.raises(ValueError):
        with_value(torch.zeros(2, H, device=DEV)).gat_attention(a_row[:, 0], a_col[:, 0], v[:, 0], bias=True)
    with pytest.raises(TypeError):
        with_value(torch.zeros(2, dtype=torch.float64, device=DEV)).gat_attention(a_row, a_col, v, bias=True)

    rowptr = torch.tensor([0, 1, 2], device=DEV)
    with pytest.raises(TypeError):
        ops.gat_attention(rowptr.int(), col, a_row, a_col, v)
    with pytest.raises(ValueError):
        ops.gat_attention(rowptr, col, a_row, a_col, v, bias=torch.zeros(3, device=DEV))
    with pytest.raises(TypeError):
        ops.gat_attention(rowptr, col, a_row, a_col, v, bias=torch.zeros(2, dtype=torch.float64, device=DEV))
    with pytest.raises(TypeError):
        ops.gat_attention(rowptr, col, a_row, a_col, v, negative_slope=False)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.gat_attention(rowptr.cpu(), col, a_row, a_col, v)

    # the C-ABI refuses a non-finite slope by itself, with the caller's name in the message
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    out, stat = torch.empty(2, H, F, device=DEV), torch.empty(2, H, 2, device=DEV)
    status = lib.psa_gat_attention_fw(rowptr.data_ptr(), col.data_ptr(), a_row.data_ptr(), a_col.data_ptr(),
                                      v.data_ptr(), None, 1, float("nan"), 0.0, 0, 2, 3, H, F, 2, out.data_ptr(),
                                      stat.data_ptr(), None, 0, torch.cuda.current_stream().cuda_stream)
    assert status != 0
    with pytest.raises(_lib.HipCoreError, match="psa_gat_attention_fw"):
        _lib.check(status)
