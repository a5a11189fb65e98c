"""GPU suite for spmm_multi (csrc/spmm_multi.hip, multi_aggr.py) against the float64 restatement of
tests/multi_aggr_ref.py.  Outputs of the raw op start as 0xAB bytes, so an element that was not written shows.
The file name sorts behind every other GPU file on purpose: the new tests are collected last."""
import functools

import numpy as np
import pytest
import torch

import multi_aggr_ref as ref
import paddle_sparse_amd as ps
from paddle_sparse_amd import SparseTensor, ops

pytestmark = pytest.mark.gpu

EPS = 1e-5
U24 = 2.0 ** -24
LONG = ops.LONG_ROW
LANES = sorted({ops.spmm_multi_lanes(k) for k in (1, 32, 64, 128, 256)})  # every LPR the launch can choose: 4 .. 64
STEP = sorted({64 // lanes for lanes in LANES})                          # entries one wave instruction takes
# row lengths of the one matrix: empty rows at the head, in the middle and at the tail; 1 and 2; either side of
# every step and of SPMM_MULTI_STEPS steps; either side of LONG_ROW; two chunks plus one entry
EDGES = sorted({m * g + d for g in STEP for m in (1, ops.SPMM_MULTI_STEPS) for d in (-1, 0, 1)} - {0})  # 1, 2, 3, .. 65
LENGTHS = [0] + EDGES[:6] + [0] + EDGES[6:] + [LONG - 1, LONG, LONG + 1, 2 * LONG + 1, 0]
# the issue's list, plus 64 (16 lanes per entry, the benchmarked width) and one float4 beyond a tile (two 16-byte tiles)
WIDTHS = (1, 3, 4, 5, ops.SPMM_MULTI_TILE_VEC4, ops.SPMM_MULTI_TILE_VEC4 + 1, 128, 64, ops.SPMM_MULTI_TILE_VEC4 + 4)
SETS = tuple((n,) for n in ref.NAMES) + (("mean", "min", "max", "std"), ("std", "max", "sum", "var", "min", "mean"),
                                         ("mean", "max"))


def csr(lengths, N, seed):
    rng = np.random.default_rng(seed)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(N, n, replace=False)) for n in lengths] + [np.zeros(0, np.int64)]).astype(np.int64)
    return rowptr, col


@functools.lru_cache(maxsize=None)
def exact_case(K, lengths=tuple(LENGTHS), N=300):
    """Integer x in [-8, 8] and values out of {-2, -1, 0.5, 1, 2}: every sum of m and of m^2 is exact in fp32.  The
    float64 reference of all six statistics with and without values, computed once and shared."""
    rng = np.random.default_rng(K)
    rowptr, col = csr(lengths, N, K)
    x = rng.integers(-8, 9, (N, K)).astype(np.float32)
    value = rng.choice(np.array([-2, -1, 0.5, 1, 2], np.float32), len(col))
    refs = {v: ref.forward(rowptr, col, value if v else None, x, ref.NAMES, EPS) for v in (False, True)}
    return rowptr, col, value, x, refs


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw(rowptr, col, value, x, reduce, **kw):
    out = torch.full((len(rowptr) - 1, len(reduce), 4 * x.shape[1]), 0xAB, dtype=torch.uint8, device="cuda").view(torch.float32)
    got, amin, amax = ops.spmm_multi(cuda(rowptr), cuda(col), cuda(value), cuda(x), reduce, EPS, out=out, **kw)
    assert got is out
    return got.cpu().numpy(), None if amin is None else amin.cpu().numpy(), None if amax is None else amax.cpu().numpy()


def assert_forward(got, want, ex2, reduce):
    """sum, mean, min, max: Σm is an exact integer multiple of 0.5 below 2^24, so the statistic equals the float64
    reference rounded once to fp32 (the quotient of two exact numbers rounds the same way through float64).
    var = Σm²/n - mean²: two quotients, one product and one difference, every one at most Σm²/n in size and each
    rounded to half an ulp (2^-24 relative), the product carrying its operand's error twice: within 8 · 2^-24 · Σm²/n,
    absolute, with or without contraction.  std = sqrt(var + eps): d sqrt = d var / (2 sqrt(var + eps)), plus the
    roundings of eps, of the sum and of the root: 2 ulp of the result."""
    names = [("sum" if n == "add" else n) for n in reduce]
    var_ref = want[:, ref.NAMES.index("var")]
    for a, n in enumerate(names):
        w = want[:, ref.NAMES.index(n)]
        if n == "var":
            assert np.all(np.abs(got[:, a] - w) <= 8 * U24 * ex2), n
        elif n == "std":
            bound = 8 * U24 * ex2 / (2 * np.sqrt(var_ref + EPS)) + 2 * np.spacing(w.astype(np.float32))
            assert np.all(np.abs(got[:, a] - w) <= bound), n
        else:
            assert np.array_equal(got[:, a], w.astype(np.float32)), n


@pytest.mark.parametrize("values", (False, True))
@pytest.mark.parametrize("reduce", SETS, ids="-".join)
@pytest.mark.parametrize("K", WIDTHS)
def test_forward_exact_data(K, reduce, values):
    rowptr, col, value, x, refs = exact_case(K)
    want, arg, ex2 = refs[values]
    v = value if values else None
    got, amin, amax = raw(rowptr, col, v, x, reduce)
    assert amin is None and amax is None
    assert_forward(got, want, ex2, reduce)
    got_arg, amin, amax = raw(rowptr, col, v, x, reduce, want_arg=True)  # the instantiations that track the winners
    assert_forward(got_arg, want, ex2, reduce)
    for n, a in (("min", amin), ("max", amax)):
        assert (a is not None) == (n in reduce)
        if a is not None:
            assert np.array_equal(a, arg[n])
    one_wave = raw(rowptr, col, v, x, reduce, no_long_rows=True)[0]  # no workspace: the long rows stay on their wave
    assert_forward(one_wave, want, ex2, reduce)


@pytest.mark.parametrize("K", (3, 128))
def test_ties_go_to_the_first_entry(K):
    rowptr, col = csr([5, 2 * LONG + 44], 400, 1)
    x = np.full((400, K), -3.0, np.float32)
    got, amin, amax = raw(rowptr, col, None, x, ("min", "max", "var", "std"), want_arg=True)
    first = np.repeat(rowptr[:-1, None], K, 1)
    assert np.array_equal(amin, first) and np.array_equal(amax, first)
    assert np.all(got[:, :2] == -3.0) and np.all(got[:, 2] == 0.0)
    assert np.all(got[:, 3] == np.sqrt(np.float32(EPS)))


def test_held_to_the_existing_op():
    """min / max: the bits of adj.matmul, with a NaN in one row and +-inf in another.  sum: both ops against float64;
    a sum of n products in fp32, whatever its order, is within n · 2^-24 · Σ|m| of the exact one, and the new op may be
    that far beyond the distance the existing op keeps."""
    K, N = 128, 300
    rng = np.random.default_rng(7)
    rowptr, col = csr(LENGTHS, N, 7)
    x = rng.standard_normal((N, K)).astype(np.float32)
    value = rng.standard_normal(len(col)).astype(np.float32)
    nan_row, inf_row = 6, len(LENGTHS) - 2  # a row of 7 entries, and the one of two chunks plus one
    x[col[rowptr[nan_row]], 5] = np.nan
    x[col[rowptr[inf_row] + 1], 7], x[col[rowptr[inf_row] + 130], 9] = np.inf, -np.inf
    adj = SparseTensor(rowptr=cuda(rowptr), col=cuda(col), value=cuda(value), sparse_sizes=(len(LENGTHS), N), is_sorted=True)
    xd = cuda(x)
    got = adj.spmm_multi(xd, ("min", "sum", "max"))
    for a, n in ((0, "min"), (2, "max")):
        assert torch.equal(got[:, a].view(torch.int32), adj.matmul(xd, n).view(torch.int32)), n
    with np.errstate(invalid="ignore"):
        want, _, _ = ref.forward(rowptr, col, value, x, ("sum",), EPS)
        m_abs = ref.forward(rowptr, col, np.abs(value), np.abs(x), ("sum",), EPS)[0][:, 0]
    finite = np.isfinite(want[:, 0])
    n = np.diff(rowptr)[:, None]
    new, old = got[:, 1].cpu().numpy().astype(np.float64), adj.matmul(xd, "sum").cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(new), np.isnan(old))
    new, old, exact = new[finite], old[finite], want[:, 0][finite]
    assert np.all(np.abs(new - exact) <= np.abs(old - exact) + (n * U24 * m_abs)[finite])


@pytest.mark.parametrize("values", (False, True))
@pytest.mark.parametrize("reduce", (("mean", "min", "max", "std"), ("sum", "var"), ("std", "max")), ids="-".join)
@pytest.mark.parametrize("K", (3, 128))
def test_gradient_of_x(K, reduce, values):
    """Exact data, rows of at most 8 entries plus one long row; ("std", "max") names neither the mean nor the sum, so
    the kernel writes the mean beside out for the backward, and the tracked forward is held to the reference too.  An element of grad_x is the sum of one term per
    stored entry of its column.  A term goes through at most 24 fp32 roundings: 1 / n, g_m / n and its sum with g_s
    (3); 0.5 / std, its product with g_d and the sum with g_v (3); 2 gv / n (1); the mean as the forward rounded it,
    its product with that and the difference (3); value * u and its addition (2); value², its product and its
    addition (3); x * the second sum and the sum of the two parts (2); a product, an atomic addition and a final
    addition for each of min and max (6); 1 spare.  Each is at most 2^-24 of the largest sum of absolute pieces of a
    term of that element, so the margin is terms · 24 · 2^-24 · largest, all from the float64 reference.  The std the
    backward reads is the forward's, which test_forward_exact_data holds to 8 · 2^-24 · (Σm²/n) / (2 std) + 2 ulp:
    `slack` is what that relative error does to the std pieces.  The min / max part comes through float atomics and
    is compared the same way."""
    lengths = tuple(int(n) for n in np.random.default_rng(3).integers(0, 9, 40)) + (LONG + 77,)
    rowptr, col, value, x, refs = exact_case(K, lengths, 260)
    v = value if values else None
    g = np.random.default_rng(K).integers(-4, 5, (len(lengths), len(reduce), K)).astype(np.float32)
    out64, _, ex2 = refs[values]
    std = out64[:, ref.NAMES.index("std")]
    with np.errstate(divide="ignore", invalid="ignore"):  # std is 0 in a row without entries, which has no terms
        std_rel = (8 * U24 * ex2 / (2 * std) + 2 * np.spacing(std.astype(np.float32))) / std
    want, terms, largest, slack = ref.grad_x(rowptr, col, v, x, reduce, EPS, g, std_rel)
    adj = SparseTensor(rowptr=cuda(rowptr), col=cuda(col), value=cuda(v), sparse_sizes=(len(lengths), 260), is_sorted=True)
    xd = cuda(x).requires_grad_()
    out = adj.spmm_multi(xd, reduce, eps=EPS)
    assert_forward(out.detach().cpu().numpy(), out64, ex2, reduce)
    out.backward(cuda(g))
    err = np.abs(xd.grad.cpu().numpy().astype(np.float64) - want)
    assert np.all(err <= terms[:, None] * 24 * U24 * largest + slack), float((err - terms[:, None] * 24 * U24 * largest - slack).max())


def _adj(value=None):
    rowptr, col = csr([2, 0, 3], 6, 0)
    return SparseTensor(rowptr=cuda(rowptr), col=cuda(col), value=value, sparse_sizes=(3, 6), is_sorted=True)


@pytest.mark.parametrize("case,error", (("duplicate", ValueError), ("empty", ValueError), ("unknown", ValueError),
                                        ("bf16", TypeError), ("3d", ValueError), ("tracked value", NotImplementedError),
                                        ("cpu", RuntimeError)))
def test_refusals(case, error):
    x = torch.ones(6, 4, device="cuda")
    reduce = {"duplicate": ("sum", "add"), "empty": (), "unknown": ("median",)}.get(case, ("mean", "std"))
    adj = _adj(torch.ones(5, device="cuda", requires_grad=True) if case == "tracked value" else None)
    x = {"bf16": x.bfloat16(), "3d": x.view(6, 2, 2), "cpu": x.cpu()}.get(case, x)
    with pytest.raises(error):
        adj.spmm_multi(x, reduce)
    with pytest.raises(error):
        ps.spmm_multi(adj, x, reduce)


def test_no_entries_gives_zeros():
    rowptr, col = csr([0, 0, 0], 6, 0)
    got, amin, amax = raw(rowptr, col, None, np.ones((6, 5), np.float32), ref.NAMES, want_arg=True)
    assert np.all(got == 0) and np.all(amin == 0) and np.all(amax == 0)


def test_every_row_long_and_a_second_trip_of_the_chunk_grid():
    rows = ops.SPMM_MULTI_CHUNK_WAVES // 2 + 8  # two chunks a row: more chunks than the capped grid has waves
    rowptr, col, value, x, refs = exact_case(4, (LONG + 1,) * rows, 200)
    want, arg, ex2 = refs[True]
    got, amin, amax = raw(rowptr, col, value, x, ref.NAMES, want_arg=True)
    assert_forward(got, want, ex2, ref.NAMES)
    assert np.array_equal(amin, arg["min"]) and np.array_equal(amax, arg["max"])
