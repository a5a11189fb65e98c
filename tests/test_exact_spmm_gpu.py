"""Exact-arithmetic SpMM parity over every forward and backward route.

Integer data (value in [-3, 3], dense operands in [-8, 8]) keeps every fp32 sum exact in any order
(tests/exact_ref.py; each test asserts that bound on its own data), so the kernels must match the
float64 reference BIT FOR BIT: out, arg_out (or the row-local bytes decoded back to edge ids),
grad_mat and grad_value.  A dropped, duplicated or misrouted edge fails at any row length, and the
many ties under min / max pin the first-edge rule across chunk, range and piece boundaries.

Where the C dispatch picks the route, the test cites the line that sends the case there; where
Python picks it, a spy asserts the choice, so that a heuristic change fails here instead of
quietly moving coverage elsewhere."""
import sys

import numpy as np
import pytest
import torch

from exact_ref import (assert_exact_preconditions, csr_with_col_degrees, csr_with_degrees, int_data, integers,
                       pow2_degrees, spmm_backward_ref, spmm_ref, with_specials)

pytestmark = pytest.mark.gpu

REDUCES = ["sum", "mean", "min", "max"]
HALF = [torch.bfloat16, torch.float16]


def cuda(x):
    return None if x is None else x.cuda()


def eb_range_len(K: int, E: int = 4) -> int:
    """Edges per range of the edge-range kernels for this K (eb_plan, csrc/spmm_eb.hip:647-661)."""
    q = K // E
    lpr = 4 if q <= 4 else 8 if q <= 8 else 16 if q <= 16 else 32 if q <= 32 else 64 if q < 48 else 32
    return 256 if lpr >= 32 else 128 if lpr == 16 else 64 if lpr == 8 else 32


def boundary_degrees(K: int, E: int = 4, long=(1023, 1024, 1025), short: int = 150, seed: int = 0):
    """Row degrees at the edges of every route: 0-3, warp and chunk sizes (31-33 ... 255-257), the range length
    of K's class +-1, long rows; among `short` rows of 0-4 entries, shuffled."""
    r = eb_range_len(K, E)
    deg = [0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, r - 1, r, r + 1, *long]
    rng = np.random.default_rng(seed)
    deg = np.array(deg + list(rng.integers(0, 5, short)), np.int64)
    return deg[rng.permutation(deg.size)]


def graph(K, N=600, E=4, long=(1023, 1024, 1025), seed=0, skew=1.0):
    rowptr, col = csr_with_degrees(boundary_degrees(K, E, long, seed=seed), N, seed=seed + 1, col_skew=skew)
    return rowptr, col


def decode_bytes(arg_bytes, rowptr, nnz):
    """Row-local arg_out (vec_io.h: width 1 = index mod 128 | 0x80 for rows above 128, 0xff no winner; width 2 =
    index, 0xffff no winner) back to edge ids, for the rows where the form is exact."""
    width = arg_bytes.element_size()
    b = arg_bytes.cpu().to(torch.int64) & (0xffff if width == 2 else 0xff)
    none = b == (0xffff if width == 2 else 0xff)
    local = b if width == 2 else b & 127
    arg = torch.where(none, torch.full_like(b, nnz), rowptr[:-1, None] + local)
    exact = rowptr.diff() <= (65535 if width == 2 else 128)
    return arg, exact


def assert_forward(reduce, rowptr, col, value, mat, res, specials=False):
    out, arg = res[0], res[1]
    bytes_ = res[2] if len(res) > 2 else None
    ref, ref_arg = spmm_ref(reduce, rowptr, col, value, mat)
    got = out.cpu()
    assert got.dtype == ref.dtype
    if specials:
        assert torch.equal(got.isnan(), ref.isnan()), "NaN in other places"
        assert torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(ref, nan=0.0))
    else:
        diff = (got.double() - ref.double()).abs()
        assert torch.equal(got, ref), f"max |diff| {float(diff.max())} at {int(diff.argmax())}"
    if arg is not None:
        assert torch.equal(arg.cpu(), ref_arg)
    if bytes_ is not None and reduce in ("min", "max"):
        dec, exact = decode_bytes(bytes_, rowptr, col.numel())
        assert torch.equal(dec[exact], ref_arg[exact])
    return ref_arg


def variant(v, half=False):
    """Context: force an SpMM kernel variant (psa_spmm_set_variant / psa_spmm_half_set_variant)."""
    from paddle_sparse_amd import _lib, ops

    class _V:
        def __enter__(self):
            self.prev = _lib.load().psa_spmm_half_set_variant(v) if half else ops.spmm_set_variant(v)

        def __exit__(self, *exc):
            if half:
                _lib.load().psa_spmm_half_set_variant(0)
            else:
                ops.spmm_set_variant(self.prev)

    return _V()


class Spy:
    """Records calls of `ops.<name>` (kwargs kept) while active."""

    def __init__(self, *names):
        from paddle_sparse_amd import ops

        self.ops, self.names, self.calls = ops, names, []
        self.real = {n: getattr(ops, n) for n in names}

    def __enter__(self):
        for n in self.names:
            setattr(self.ops, n, (lambda n_: lambda *a, **k: self.calls.append((n_, k)) or self.real[n_](*a, **k))(n))
        return self

    def __exit__(self, *exc):
        for n, f in self.real.items():
            setattr(self.ops, n, f)

    def named(self, n):
        return [k for m, k in self.calls if m == n]


def hot_columns(n):
    """Context: storage.HOT_COLUMNS lowered, so that small power-law test matrices get the hub-row copies."""
    import paddle_sparse_amd.storage as st_mod

    class _H:
        def __enter__(self):
            self.old, st_mod.HOT_COLUMNS = st_mod.HOT_COLUMNS, n

        def __exit__(self, *exc):
            st_mod.HOT_COLUMNS = self.old

    return _H()


# ---------------------------------------------------------------------------------------------
# fp32 forward
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("K", [4, 8, 16, 32, 48, 64])
@pytest.mark.parametrize("v", [0, 1])
def test_fp32_multirow_and_row_kernels(reduce, K, v):
    """K <= 64: the multirow kernel (spmm.hip:1411-1415, several rows per wave); variant 1 sends the same shapes to
    the one-row-per-wave kernel (spmm.hip:1423-1425).  Rows above 128 entries take the long-row chunks either way;
    the byte form of arg_out comes from the multirow kernel itself."""
    from paddle_sparse_amd import ops

    rowptr, col = graph(K, seed=K)
    value, mat, _ = int_data(rowptr, 600, K, seed=K)
    assert_exact_preconditions(rowptr, col, value, mat)
    with variant(v):
        res = ops._spmm(reduce, cuda(rowptr), cuda(col), cuda(value), cuda(mat), want_arg_bytes=2, algo="row_waves")
        assert_forward(reduce, rowptr, col, value, mat, res)
        res = ops._spmm(reduce, cuda(rowptr), cuda(col), None, cuda(mat), algo="row_waves")
        assert_forward(reduce, rowptr, col, None, mat, res)


@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("K", [68, 96, 128])
def test_fp32_row_kernel_when_the_surface_knows_no_row_is_long(reduce, K):
    """64 < K <= 128 and no row above 128 entries: SparseTensor.matmul passes no_long_rows (spied), the call brings
    no workspace and the row kernel takes every row (spmm.hip:1457, q <= 32) — no fused roles, no chunks."""
    from paddle_sparse_amd import SparseTensor

    deg = np.minimum(boundary_degrees(K, long=()), 128)
    rowptr, col = csr_with_degrees(deg, 500, seed=K)
    value, mat, _ = int_data(rowptr, 500, K, seed=K)
    assert_exact_preconditions(rowptr, col, value, mat)
    a = SparseTensor(rowptr=cuda(rowptr), col=cuda(col), value=cuda(value), sparse_sizes=(rowptr.numel() - 1, 500),
                     is_sorted=True)
    a.storage._spmm_algo_memo = "row_waves"
    with Spy("_spmm") as spy, torch.no_grad():
        out = a.matmul(cuda(mat), reduce)
    assert [k.get("no_long_rows") for k in spy.named("_spmm")] == [True]
    assert torch.equal(out.cpu(), spmm_ref(reduce, rowptr, col, value, mat)[0])


@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("K", [68, 128, 132, 192, 256, 260, 384, 512, 520])
@pytest.mark.parametrize("v", [0, 15, 10, 18])
def test_fp32_fused_roles_and_long_row_chunks(reduce, K, v):
    """64 < K with rows above 128 entries and a workspace: the fused-roles kernel (spmm.hip:1436-1452; K >= 192 as
    128-wide tiles); variant 15 the separate chunk and combine launches (spmm.hip:1457-1461 with the chunk list),
    variant 10 no long-row path at all (spmm.hip:1377), variant 18 the fused kernel with non-temporal gathers."""
    from paddle_sparse_amd import ops

    rowptr, col = graph(K, seed=K + v)
    value, mat, _ = int_data(rowptr, 600, K, seed=K + v)
    assert_exact_preconditions(rowptr, col, value, mat)
    with variant(v):
        kw = {"want_arg_bytes": 2} if K % 4 == 0 and K <= 256 else {}
        res = ops._spmm(reduce, cuda(rowptr), cuda(col), cuda(value), cuda(mat), algo="row_waves", **kw)
        assert_forward(reduce, rowptr, col, value, mat, res)


@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("K", [1, 2, 3, 5, 7, 31, 33, 65, 127, 129, 257])
def test_fp32_one_wide_kernels(reduce, K):
    """K % 4 != 0: the 1-wide row kernels (spmm.hip:1465-1467), with the long-row chunks behind them."""
    from paddle_sparse_amd import ops

    rowptr, col = graph(K, seed=K)
    value, mat, _ = int_data(rowptr, 600, K, seed=K)
    assert_exact_preconditions(rowptr, col, value, mat)
    res = ops._spmm(reduce, cuda(rowptr), cuda(col), cuda(value), cuda(mat), algo="row_waves")
    assert_forward(reduce, rowptr, col, value, mat, res)


@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("K", [4, 16, 64, 128, 256])
def test_fp32_misaligned_operand_takes_the_one_wide_kernels(reduce, K):
    """K % 4 == 0 but `mat` a contiguous view that does not start on 16 bytes: v4 is false (spmm.hip:1392) and the
    1-wide kernels run; the forward (both families) and the autograd backward give the aligned bits."""
    from paddle_sparse_amd import SparseTensor, ops

    rowptr, col = graph(K, seed=K)
    N = 600
    value, mat, grad = int_data(rowptr, N, K, seed=K)
    assert_exact_preconditions(rowptr, col, value, mat, grad)
    flat = torch.zeros(N * K + 1, device="cuda")
    flat[1:] = cuda(mat).flatten()
    bad = flat[1:].view(N, K)
    assert bad.is_contiguous() and bad.data_ptr() % 16 != 0
    for algo in ("row_waves", "edge_ranges"):
        res = ops._spmm(reduce, cuda(rowptr), cuda(col), cuda(value), bad, algo=algo)
        ref_arg = assert_forward(reduce, rowptr, col, value, mat, res)
    v = cuda(value).requires_grad_()
    a = SparseTensor(rowptr=cuda(rowptr), col=cuda(col), value=v, sparse_sizes=(rowptr.numel() - 1, N), is_sorted=True)
    b = bad.detach().requires_grad_()
    assert b.data_ptr() % 16 != 0
    gflat = torch.zeros(grad.numel() + 1, device="cuda")
    gflat[1:] = cuda(grad).flatten()
    g = gflat[1:].view_as(grad)
    assert g.data_ptr() % 16 != 0
    a.matmul(b, reduce).backward(g)
    gv, gm = spmm_backward_ref(reduce, rowptr, col, value, mat, grad, arg=ref_arg) if reduce != "mean" else (None, None)
    if reduce != "mean":  # (the mean backward is exact on power-of-two degrees only: test_fp32_backward_routes)
        assert torch.equal(v.grad.cpu(), gv) and torch.equal(b.grad.cpu(), gm)


@pytest.mark.parametrize("reduce", ["sum", "max"])
@pytest.mark.parametrize("wide", [40, 41])
def test_fp32_out_column_slice(reduce, wide):
    """ops._spmm(..., out=wide[:, a:b]) (distributed.py's rank-local product): ldo = the wide matrix's width, both
    ldo % 4 == 0 (16-byte rows) and not (the 1-wide kernels, spmm.hip:1392); columns outside the slice untouched."""
    from paddle_sparse_amd import ops

    K = 16
    rowptr, col = graph(K, seed=wide)
    value, mat, _ = int_data(rowptr, 600, K, seed=wide)
    M = rowptr.numel() - 1
    base = torch.full((M, wide), 7.5, device="cuda")
    for a in (4, 8):
        w = base.clone()
        res = ops._spmm(reduce, cuda(rowptr), cuda(col), cuda(value), cuda(mat), out=w[:, a:a + K], algo="row_waves")
        assert res[0].data_ptr() == w[:, a:a + K].data_ptr()
        assert torch.equal(w[:, a:a + K].cpu(), spmm_ref(reduce, rowptr, col, value, mat)[0])
        assert bool((w[:, :a] == 7.5).all()) and bool((w[:, a + K:] == 7.5).all())


@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("K", [4, 8])
def test_fp32_rows_near_and_above_65535_entries(reduce, K):
    """Rows of 65 535 - 65 537 and 140 000 entries among short ones: long-row chunks (row waves), the edge-range
    walk with and without `row`, and both arg forms (the two-byte one exact up to 65 535 entries)."""
    from paddle_sparse_amd import ops

    rowptr, col = graph(K, N=3000, long=(65535, 65536, 65537, 140_000), seed=K)
    value, mat, _ = int_data(rowptr, 3000, K, seed=K)
    assert_exact_preconditions(rowptr, col, value, mat)
    row = torch.repeat_interleave(torch.arange(rowptr.numel() - 1), rowptr.diff())
    for kw in ({"algo": "row_waves"}, {"algo": "edge_ranges", "row": cuda(row)}, {"algo": "edge_ranges"}):
        res = ops._spmm(reduce, cuda(rowptr), cuda(col), cuda(value), cuda(mat), want_arg_bytes=2, **kw)
        assert_forward(reduce, rowptr, col, value, mat, res)


@pytest.mark.parametrize("reduce", REDUCES)
def test_fp32_specials(reduce):
    """+-inf and NaN in the dense operand: NaN / inf where the reference has them, NaN never wins, infinite products
    only where they beat the init; rows without a winner keep the sentinel.  Row waves and edge ranges."""
    from paddle_sparse_amd import ops

    for K in (8, 128, 5):
        rowptr, col = graph(K, seed=3 + K)
        value, mat, _ = int_data(rowptr, 600, K, seed=K)
        mat = with_specials(mat, seed=K)
        mat[:4] = float("nan")
        col[rowptr[4]:rowptr[5]] = col[rowptr[4]:rowptr[5]] % 4  # a row reading NaN only
        assert_exact_preconditions(rowptr, col, value, mat)
        for algo in ("row_waves", "edge_ranges"):
            res = ops._spmm(reduce, cuda(rowptr), cuda(col), cuda(value), cuda(mat), algo=algo)
            assert_forward(reduce, rowptr, col, value, mat, res, specials=True)


# ---------------------------------------------------------------------------------------------
# edge ranges
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("K", [4, 16, 32, 64, 128, 256])
@pytest.mark.parametrize("v", [0, 31, 32, 33, 35])
def test_fp32_edge_ranges(reduce, K, v):
    """algo="edge_ranges" (spmm.hip:1357-1366): ranges of the planned length for K's class, or 128 / 512 / 1024 edges
    (variants 31-33), ordinary stores (35); degrees at range_len +- 1 put segments across range boundaries.  With
    the COO row ids and without (derived by the call); min / max leave the two-byte row-local form as well."""
    from paddle_sparse_amd import ops

    rowptr, col = graph(K, seed=K + v)
    value, mat, _ = int_data(rowptr, 600, K, seed=K + v)
    assert_exact_preconditions(rowptr, col, value, mat)
    row = torch.repeat_interleave(torch.arange(rowptr.numel() - 1), rowptr.diff())
    with variant(v):
        for r in (cuda(row), None):
            res = ops._spmm(reduce, cuda(rowptr), cuda(col), cuda(value), cuda(mat), algo="edge_ranges", row=r,
                            want_arg_bytes=2)
            assert_forward(reduce, rowptr, col, value, mat, res)


def power_law(M=4000, N=3000, seed=0, K=None):
    """Mostly empty and 1-2 entry rows (the edge-range family), a few long rows, columns crowded towards 0 (hub
    columns, and long columns in the CSC view)."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 3, M)
    deg[rng.choice(M, 12, replace=False)] = [129, 200, 255, 256, 257, 300, 513, 1000, 1023, 1025, 2000, 4000]
    return csr_with_degrees(deg, N, seed=seed + 1, col_skew=5.0)


@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("K", [4, 16, 64, 128, 256])
def test_fp32_edge_ranges_with_hot_rows(reduce, K):
    """The tensor surface on a power-law matrix: edge-range forward with the compact copy of the hub rows
    (hot_rows, spied), bit-equal to the reference."""
    from paddle_sparse_amd import SparseTensor

    rowptr, col = power_law(seed=K)
    M, N = rowptr.numel() - 1, 3000
    value, mat, _ = int_data(rowptr, N, K, seed=K)
    assert_exact_preconditions(rowptr, col, value, mat)
    a = SparseTensor(rowptr=cuda(rowptr), col=cuda(col), value=cuda(value), sparse_sizes=(M, N), is_sorted=True)
    with hot_columns(64), Spy("_spmm") as spy, torch.no_grad():
        out = a.matmul(cuda(mat), reduce)
    (kw,) = spy.named("_spmm")
    assert kw["algo"] == "edge_ranges" and kw["hot_rows"] is not None and kw["row"] is not None
    assert torch.equal(out.cpu(), spmm_ref(reduce, rowptr, col, value, mat)[0])


# ---------------------------------------------------------------------------------------------
# half-width forward
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("K", [8, 16, 24, 64, 128, 136, 256, 520])
@pytest.mark.parametrize("v", [0, 1, 2, 4])
def test_half_forward(dtype, reduce, K, v):
    """psa_spmm_half: fp32 products and sums, one rounding on store.  Variant 0 the row kernel (spmm_half.hip:361-
    369), 1 the multirow kernel for K <= 128 (spmm_half.hip:353-358, no byte form), 2 the 16-lane K = 128 form, 4 the
    64-bit addressing.  fp32 values and values of mat's dtype; min / max with the int64 arg_out and the byte form."""
    from paddle_sparse_amd import ops

    rowptr, col = graph(K, E=8, seed=K + v)
    for vdt in (torch.float32, dtype):
        value, mat, _ = int_data(rowptr, 600, K, dtype=dtype, value_dtype=vdt, seed=K + v)
        assert_exact_preconditions(rowptr, col, value, mat)
        with variant(v, half=True):
            res = ops._spmm(reduce, cuda(rowptr), cuda(col), cuda(value), cuda(mat))
            assert_forward(reduce, rowptr, col, value, mat, res)
            if reduce in ("min", "max") and v != 1:
                res = ops._spmm(reduce, cuda(rowptr), cuda(col), cuda(value), cuda(mat), want_arg=False, want_arg_bytes=2)
                assert res[1] is None
                assert_forward(reduce, rowptr, col, value, mat, res)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("K", [4, 12, 20])
def test_half_forward_odd_widths_widen(dtype, reduce, K):
    """K % 8 != 0: the fp32 kernels on widened operands, rounded once (ops._spmm_half)."""
    from paddle_sparse_amd import ops

    rowptr, col = graph(K, E=8, seed=K)
    value, mat, _ = int_data(rowptr, 600, K, dtype=dtype, seed=K)
    assert_exact_preconditions(rowptr, col, value, mat)
    assert_forward(reduce, rowptr, col, value, mat, ops._spmm(reduce, cuda(rowptr), cuda(col), cuda(value), cuda(mat)))


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("K", [8, 64, 128])
def test_half_edge_ranges_with_hot_rows(dtype, reduce, K):
    """Half width on a power-law matrix through the tensor surface: edge-range kernels (psa_spmm_half_coo) with the
    hub-row copy (spied); and the same call without hot rows or `row`."""
    from paddle_sparse_amd import SparseTensor, ops

    rowptr, col = power_law(seed=K)
    M, N = rowptr.numel() - 1, 3000
    value, mat, _ = int_data(rowptr, N, K, dtype=dtype, seed=K)
    assert_exact_preconditions(rowptr, col, value, mat)
    a = SparseTensor(rowptr=cuda(rowptr), col=cuda(col), value=cuda(value), sparse_sizes=(M, N), is_sorted=True)
    with hot_columns(64), Spy("_spmm_half") as spy, torch.no_grad():
        out = a.matmul(cuda(mat), reduce)
    (kw,) = spy.named("_spmm_half")
    assert kw["algo"] == "edge_ranges" and kw["hot_rows"] is not None
    assert torch.equal(out.cpu(), spmm_ref(reduce, rowptr, col, value, mat)[0])
    res = ops._spmm(reduce, cuda(rowptr), cuda(col), cuda(value), cuda(mat), algo="edge_ranges")
    assert_forward(reduce, rowptr, col, value, mat, res)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("algo", ["auto", "edge_ranges"])
def test_half_sums_round_once_and_overflow(dtype, algo):
    """Sums past 256 (bf16) / 2048 (fp16) round once on store, to nearest even; fp16 overflows to +-inf."""
    from paddle_sparse_amd import ops

    K = 16
    rowptr, col = graph(K, N=50, E=8, seed=5)
    value = integers(col.numel(), 20, 30, torch.float32, seed=6)
    mat = integers((50, K), -40, 40, dtype, seed=7)
    mat[:, :2] = 40  # one-signed columns: sums up to 10^6 (fp16 overflows), the others odd values past 2048
    assert_exact_preconditions(rowptr, col, value, mat)
    ref = spmm_ref("sum", rowptr, col, value, mat)[0]
    assert bool((ref.float().abs() > 2048).any())
    if dtype == torch.float16:
        assert bool(ref.isinf().any())
    for reduce in REDUCES:
        res = ops._spmm(reduce, cuda(rowptr), cuda(col), cuda(value), cuda(mat), algo=algo)
        assert_forward(reduce, rowptr, col, value, mat, res, specials=True)


# ---------------------------------------------------------------------------------------------
# fp32 backward
# ---------------------------------------------------------------------------------------------

def autograd_step(rowptr, col, value, mat, grad, reduce, want_value=True, want_mat=True, N=None, hot=None):
    from paddle_sparse_amd import SparseTensor

    M, N = rowptr.numel() - 1, N or mat.shape[0]
    v = None if value is None else cuda(value).requires_grad_(want_value)
    b = cuda(mat).requires_grad_(want_mat)
    a = SparseTensor(rowptr=cuda(rowptr), col=cuda(col), value=v, sparse_sizes=(M, N), is_sorted=True)
    if hot:
        with hot_columns(hot):
            out = a.matmul(b, reduce)
            out.backward(cuda(grad))
    else:
        out = a.matmul(b, reduce)
        out.backward(cuda(grad))
    return out, (None if v is None else v.grad), b.grad


def assert_backward(reduce, rowptr, col, value, mat, grad, out, gv, gm, want_value=True, want_mat=True):
    ref, arg = spmm_ref(reduce, rowptr, col, value, mat)
    assert torch.equal(out.detach().cpu(), ref)
    rgv, rgm = spmm_backward_ref(reduce, rowptr, col, value, mat, grad, arg=arg, value_dtype=value.dtype if value is not None else torch.float32)
    if want_value and value is not None:
        assert torch.equal(gv.cpu(), rgv), f"grad_value: max |diff| {float((gv.cpu().double() - rgv.double()).abs().max())}"
    else:
        assert gv is None
    if want_mat:
        assert torch.equal(gm.cpu(), rgm), f"grad_mat: max |diff| {float((gm.cpu().double() - rgm.double()).abs().max())}"


FP32_BW = ["sum_bw_csc", "value_bw", "transposed", "value_bw_wide"]


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("K", [4, 64, 128, 256, 260])
@pytest.mark.parametrize("grads", ["both", "value", "mat"])
def test_fp32_sum_mean_backward_routes(reduce, K, grads):
    """sum / mean autograd on a matrix with long rows AND long columns (power-of-two row degrees, so the mean's
    folded 1 / deg is exact): both gradients in one pass over the CSC view (spmm_sum_bw_csc, K <= 256), grad_value
    alone (spmm_value_bw, with its long-row kernel), grad_mat alone (the forward over the CSC view with the
    transposed weights).  K = 260: spmm_value_bw + the forward over the CSC view (spied)."""
    deg = pow2_degrees(boundary_degrees(K, short=300, seed=K))
    rowptr, col = csr_with_degrees(deg, 400, seed=K, col_skew=3.0)
    value, mat, grad = int_data(rowptr, 400, K, seed=K)
    assert_exact_preconditions(rowptr, col, value, mat, grad, mean_backward=reduce == "mean")
    wv, wm = grads in ("both", "value"), grads in ("both", "mat")
    with Spy("spmm_sum_bw_csc", "spmm_value_bw", "transpose_weights", "_spmm") as spy:
        out, gv, gm = autograd_step(rowptr, col, value, mat, grad, reduce, wv, wm)
    one_pass = wv and wm and K <= 256
    assert bool(spy.named("spmm_sum_bw_csc")) == one_pass
    assert bool(spy.named("spmm_value_bw")) == (wv and not one_pass)
    assert len(spy.named("_spmm")) == 1 + (wm and not one_pass)
    assert_backward(reduce, rowptr, col, value, mat, grad, out, gv, gm, wv, wm)


@pytest.mark.parametrize("reduce", ["min", "max"])
@pytest.mark.parametrize("K", [4, 64, 128, 256, 260])
@pytest.mark.parametrize("longest", [100, 1025])
@pytest.mark.parametrize("grads", ["both", "value", "mat"])
def test_fp32_minmax_backward_routes(reduce, K, longest, grads):
    """min / max autograd: with grad_mat wanted and K % 4 == 0, K <= 256 the one pass over the CSC view fed by the
    row-local bytes (width 1 when no row exceeds 128 entries, 2 up to 65 535) — spmm_minmax_bw_csc, columns above 128
    entries included; grad_value alone or K = 260: spmm_minmax_bw through the int64 arg_out."""
    deg = np.minimum(boundary_degrees(K, short=300, seed=K), longest)
    rowptr, col = csr_with_degrees(deg, 400, seed=K, col_skew=3.0)
    value, mat, grad = int_data(rowptr, 400, K, seed=K)
    assert_exact_preconditions(rowptr, col, value, mat, grad)
    wv, wm = grads in ("both", "value"), grads in ("both", "mat")
    with Spy("spmm_minmax_bw_csc", "spmm_minmax_bw_eb", "spmm_minmax_bw", "_spmm") as spy:
        out, gv, gm = autograd_step(rowptr, col, value, mat, grad, reduce, wv, wm)
    csc = wm and K <= 256
    # (grad_mat alone on a matrix whose transpose is power-law: the edge-range form of that pass, spmm_minmax_bw_eb)
    one_pass = spy.named("spmm_minmax_bw_csc") + spy.named("spmm_minmax_bw_eb")
    assert len(one_pass) == csc and bool(spy.named("spmm_minmax_bw")) == (not csc)
    if csc:
        (fw,) = spy.named("_spmm")
        assert fw["want_arg_bytes"] == (1 if longest <= 128 else 2) and not fw["want_arg"]
    assert_backward(reduce, rowptr, col, value, mat, grad, out, gv, gm, wv, wm)


@pytest.mark.parametrize("reduce", ["min", "max"])
@pytest.mark.parametrize("K", [4, 64, 128])
@pytest.mark.parametrize("with_value", [True, False])
def test_fp32_minmax_grad_mat_by_edge_ranges_with_hot_ids(reduce, K, with_value):
    """Fixed adjacency on a power-law matrix: grad_mat by the edge-range kernels over the CSC view
    (spmm_minmax_bw_eb, spied), hub rows of grad_out from compact copies (hot_ids)."""
    rowptr, col = power_law(seed=K)
    # the transpose must be power-law too: make most columns hold 0-2 entries
    value, mat, grad = int_data(rowptr, 3000, K, seed=K, with_value=with_value)
    assert_exact_preconditions(rowptr, col, value, mat, grad)
    with Spy("spmm_minmax_bw_eb", "spmm_minmax_bw_csc") as spy:
        out, gv, gm = autograd_step(rowptr, col, value, mat, grad, reduce, want_value=False, hot=64)
    (kw,) = spy.named("spmm_minmax_bw_eb")
    assert kw.get("hot_ids") is not None and not spy.named("spmm_minmax_bw_csc")
    assert_backward(reduce, rowptr, col, value, mat, grad, out, None, gm, want_value=False)


# ---------------------------------------------------------------------------------------------
# half-width backward
# ---------------------------------------------------------------------------------------------

FP32_FALLBACKS = ["spmm_sum_bw_csc", "spmm_value_bw", "spmm_minmax_bw_csc", "spmm_minmax_bw", "spmm_minmax_bw_eb"]


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("K", [8, 64, 136, 512])
@pytest.mark.parametrize("grads", ["both", "mat"])
def test_half_sum_mean_backward(dtype, reduce, K, grads):
    """Half-width sum / mean backward: both gradients in one half-width pass over the CSC view
    (spmm_half_sum_bw_csc; columns above 128 entries in chunks + combine), or grad_mat alone by the half-width
    forward over the CSC view.  No fp32 pass is called (spied)."""
    N = 300
    if reduce == "mean":  # power-of-two row degrees; columns crowded towards 0 for long columns
        rowptr, col = csr_with_degrees(pow2_degrees(boundary_degrees(K, short=300, seed=K)), N, seed=K, col_skew=4.0)
    else:  # long COLUMNS (the chunked path): the row degrees of the transpose at the boundaries
        rowptr, col = csr_with_col_degrees(boundary_degrees(K, short=N - 22, seed=K)[:N], 400, seed=K)
    assert int(torch.bincount(col, minlength=N).max()) > 512  # columns above 128 entries: chunks + combine
    value, mat, grad = int_data(rowptr, N, K, dtype=dtype, seed=K)
    assert_exact_preconditions(rowptr, col, value, mat, grad, mean_backward=reduce == "mean")
    wv = grads == "both"
    with Spy(*FP32_FALLBACKS, "spmm_half_sum_bw_csc") as spy:
        out, gv, gm = autograd_step(rowptr, col, value, mat, grad, reduce, want_value=wv)
    assert [n for n, _ in spy.calls if n in FP32_FALLBACKS] == []
    assert bool(spy.named("spmm_half_sum_bw_csc")) == wv
    assert_backward(reduce, rowptr, col, value, mat, grad, out, gv, gm, wv)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("reduce", ["min", "max"])
@pytest.mark.parametrize("K", [8, 64, 136])
@pytest.mark.parametrize("longest", [100, 1025])
def test_half_minmax_backward(dtype, reduce, K, longest):
    """Half-width min / max backward: the masked pass over the CSC view (spmm_half_minmax_bw_csc) fed by the
    one-byte (rows <= 128) or two-byte row-local form; long columns in chunks.  No fp32 pass (spied)."""
    deg = np.minimum(boundary_degrees(K, short=300, seed=K), longest)
    rowptr, col = csr_with_degrees(deg, 300, seed=K, col_skew=3.0)
    value, mat, grad = int_data(rowptr, 300, K, dtype=dtype, seed=K)
    assert_exact_preconditions(rowptr, col, value, mat, grad)
    with Spy(*FP32_FALLBACKS, "spmm_half_minmax_bw_csc", "_spmm") as spy:
        out, gv, gm = autograd_step(rowptr, col, value, mat, grad, reduce)
    assert [n for n, _ in spy.calls if n in FP32_FALLBACKS] == []
    assert spy.named("_spmm")[0]["want_arg_bytes"] == (1 if longest <= 128 else 2)
    assert len(spy.named("spmm_half_minmax_bw_csc")) == 1
    assert_backward(reduce, rowptr, col, value, mat, grad, out, gv, gm)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("K", [8, 64])
def test_half_misaligned_operands(dtype, reduce, K):
    """bf16 / fp16 `mat` and `grad_out` as contiguous views that do not start on 16 bytes (K % 8 == 0): the tensor
    surface takes them (the half-width kernels need 16-byte rows: an aligned copy is made) and gives the bits of
    the aligned operands, forward and backward."""
    deg = pow2_degrees(boundary_degrees(K, short=300, seed=K)) if reduce == "mean" else boundary_degrees(K, seed=K)
    rowptr, col = csr_with_degrees(deg, 300, seed=K)
    value, mat, grad = int_data(rowptr, 300, K, dtype=dtype, seed=K)
    assert_exact_preconditions(rowptr, col, value, mat, grad, mean_backward=reduce == "mean")

    def shifted(x):
        flat = torch.zeros(x.numel() + 1, dtype=x.dtype, device="cuda")
        flat[1:] = cuda(x).flatten()
        y = flat[1:].view(x.shape)
        assert y.is_contiguous() and y.data_ptr() % 16 != 0
        return y

    from paddle_sparse_amd import SparseTensor

    M = rowptr.numel() - 1
    res = []
    for misaligned in (True, False):
        v = cuda(value).requires_grad_()
        b = shifted(mat).detach().requires_grad_() if misaligned else cuda(mat).requires_grad_()
        a = SparseTensor(rowptr=cuda(rowptr), col=cuda(col), value=v, sparse_sizes=(M, 300), is_sorted=True)
        out = a.matmul(b, reduce)
        out.backward(shifted(grad) if misaligned else cuda(grad))
        res.append((out.detach(), v.grad, b.grad))
        if misaligned:
            assert b.data_ptr() % 16 != 0
            # fixed adjacency too: grad_mat alone
            b2 = shifted(mat).detach().requires_grad_()
            a2 = SparseTensor(rowptr=cuda(rowptr), col=cuda(col), value=cuda(value), sparse_sizes=(M, 300), is_sorted=True)
            a2.matmul(b2, reduce).backward(shifted(grad))
    (o1, gv1, gm1), (o2, gv2, gm2) = res
    assert torch.equal(o1, o2) and torch.equal(gv1, gv2) and torch.equal(gm1, gm2) and torch.equal(b2.grad, gm2)
    assert_backward(reduce, rowptr, col, value, mat, grad, o1, gv1, gm1)


# ---------------------------------------------------------------------------------------------
# rows above 65 535 entries
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reduce", ["min", "max"])
@pytest.mark.parametrize("case", ["negative_extreme", "zero_extreme", "ties"])
@pytest.mark.parametrize("train", [True, False])
def test_huge_rows_with_a_no_winner_piece(reduce, case, train):
    """A 140 000-entry row (three pieces of at most 65 535 entries, matmul._huge_piece_winners) whose FIRST piece
    only gathers +-inf rows of mat — no product there beats the init — among tiny rows: the bytes-only route
    (HUGE_ROW_PIECES True, spied: no int64 arg_out) and the int64 route give the reference's bits.  negative_extreme:
    the row's real extreme lies on the far side of 0; zero_extreme: it is exactly 0; ties: mat of {-1, 0, 1}."""
    mm_mod = sys.modules["paddle_sparse_amd.matmul"]
    from paddle_sparse_amd import SparseTensor, ops

    M, N, K = 2000, 3000, 8
    rng = np.random.default_rng(7)
    deg = rng.integers(0, 3, M)
    deg[5], deg[1000] = 140_000, 70_000
    rowptr = torch.as_tensor(np.concatenate([[0], np.cumsum(deg)]).astype(np.int64))
    nnz = int(rowptr[-1])
    g = torch.Generator().manual_seed(1)
    col = torch.randint(10, N, (nnz,), generator=g)
    s5 = int(rowptr[5])
    col[s5:s5 + 65535] = torch.randint(0, 10, (65535,), generator=g)  # the first piece: inf rows only
    value = integers(nnz, 1, 3, seed=2)  # positive: the sign of every product is mat's
    mx = reduce == "max"
    if case == "negative_extreme":  # max: every finite product < 0 (min: > 0)
        mat = integers((N, K), 1, 8, seed=3) * (-1 if mx else 1)
    elif case == "zero_extreme":
        mat = integers((N, K), 0, 8, seed=3) * (-1 if mx else 1)
    else:
        mat = integers((N, K), -1, 1, seed=3)
    mat[:10] = float("-inf") if mx else float("inf")
    grad = integers((M, K), -8, 8, seed=4)
    assert_exact_preconditions(rowptr, col, value, mat, grad)
    ref, arg = spmm_ref(reduce, rowptr, col, value, mat)
    assert bool((arg[5] >= s5 + 65535).all())  # the first piece never wins
    res = []
    for pieces in (True, False):
        v = cuda(value).requires_grad_(train)
        b = cuda(mat).requires_grad_()
        a = SparseTensor(rowptr=cuda(rowptr), col=cuda(col), value=v, sparse_sizes=(M, N), is_sorted=True)
        mm_mod.HUGE_ROW_PIECES = pieces
        try:
            with Spy("_spmm") as spy:
                out = a.matmul(b, reduce)
                out.backward(cuda(grad))
        finally:
            mm_mod.HUGE_ROW_PIECES = True
        seen = [(k.get("want_arg_bytes", False), k.get("want_arg", True)) for k in spy.named("_spmm")]
        if pieces:
            assert a.storage._huge_rows()["piece_ptr"].tolist() == [0, 3, 5]
            assert seen and all(s == (2, False) for s in seen)
        else:
            assert (1, True) in seen
        res.append((out.detach(), v.grad, b.grad))
    rgv, rgm = spmm_backward_ref(reduce, rowptr, col, value, mat, grad, arg=arg)
    # grad_value of an edge that reads an infinite row of mat is NaN in the pass over the CSC view (its masked dot
    # adds 0 * inf) where the reference has 0: only the edges of finite rows are compared
    finite = torch.isfinite(mat[col]).all(1)
    for out, gv, gm in res:
        assert torch.equal(out.cpu(), ref)
        assert torch.equal(gm.cpu(), rgm)
        if train:
            assert torch.equal(gv.cpu()[finite], rgv[finite])


# ---------------------------------------------------------------------------------------------
# config 3, whole output
# ---------------------------------------------------------------------------------------------

def test_config3_spmm_sum_whole_output():
    """BASELINE config 3 (2 M x 2 M, 20 M entries, F = 128) spmm_sum on integer data through the tensor surface:
    every element bit-equal to the fp32 oracle, which is exact on this data."""
    import oracle
    from paddle_sparse_amd import SparseTensor
    from util import random_csr

    M = N = 2_000_000
    K = 128
    _, rowptr, col, _ = random_csr(M, N, 20_000_000, seed=3, with_value=False)
    g = torch.Generator().manual_seed(3)
    value = torch.randint(-3, 4, (col.size,), generator=g).float().numpy()
    mat = torch.randint(-8, 9, (N, K), generator=g).float().numpy()
    deg = np.diff(rowptr)
    assert int(deg.max()) * 3 * 8 < (1 << 24)  # every partial sum exact
    a = SparseTensor(rowptr=torch.from_numpy(rowptr).cuda(), col=torch.from_numpy(col).cuda(),
                     value=torch.from_numpy(value).cuda(), sparse_sizes=(M, N), is_sorted=True)
    with torch.no_grad():
        out = a.matmul(torch.from_numpy(mat).cuda(), "sum").cpu().numpy()
    want, _ = oracle.spmm("sum", rowptr, col, value, mat, threads=16)
    assert np.array_equal(out, want)
