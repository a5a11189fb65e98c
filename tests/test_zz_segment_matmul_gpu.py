"""GPU suite for segment_matmul / typed_matmul (csrc/segment_matmul.hip, segment_matmul.py) against the float64
restatement of tests/segment_matmul_ref.py.  Exact data: x integers in [-8, 8], weights out of
{-2, -1, -0.5, 0.5, 1, 2}, cotangents integers in [-4, 4], K and F at most 130: every partial sum of the forward and
of grad_x is a multiple of 0.5 below 2^13 and every partial sum of grad_weight an integer below 2^17, exact in fp32 in
any order.  So fp32 results equal the reference bit for bit, bf16 results the reference rounded once.  Outputs of the
raw ops start as 0xAB bytes, so an element that was not written shows."""
import functools
import itertools

import numpy as np
import pytest
import torch

import paddle_sparse_amd as ps
import segment_matmul_ref as ref
from paddle_sparse_amd import ops

pytestmark = pytest.mark.gpu

BM, BN, BK, CH = ops.SEGMENT_MATMUL_BM, ops.SEGMENT_MATMUL_BN, ops.SEGMENT_MATMUL_BK, ops.SEGMENT_MATMUL_CH
# empty segments at the head, in the middle and at the tail; either side of a row tile and of a chunk
LENGTHS = (0, 1, BM - 1, 0, BM, BM + 1, 2 * BM + 1, CH - 1, CH, CH + 1, 2 * CH + 1, 0)
KS = (1, 3, 4, BK - 1, BK, BK + 1, 2 * BK + 4, 128)
FS = (1, 3, 4, BN - 1, BN, BN + 1, 2 * BN + 2)
# every K with every F, so the 16-byte-load kernels (K and F multiples of 4, or of 8 in bf16) meet K and F tails too;
# the last two are bf16 word multiples off the tile sizes
SHAPES = tuple(itertools.product(KS, FS)) + ((128, 2 * BN), (2 * BK, BN), (8, 8), (BK + 8, BN + 8))
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
MODES = ("rows", "gather", "perm")
NX = 300  # rows of x behind a gather


def csr(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


@functools.lru_cache(maxsize=32)
def case(K, F, mode, lengths=LENGTHS):
    """Operands, a cotangent and the float64 results, shared by the cases that follow each other on one shape (the
    cache is bounded: a case holds megabytes); nothing here is written again."""
    rng = np.random.default_rng(1000 * K + F)
    ptr = csr(lengths)
    R, T = int(ptr[-1]), len(lengths)
    x = rng.integers(-8, 9, (NX if mode == "gather" else R, K)).astype(np.float32)
    w = rng.choice(np.array([-2, -1, -0.5, 0.5, 1, 2], np.float32), (T, K, F))
    g = rng.integers(-4, 5, (R, F)).astype(np.float32)  # cotangent of row r, wherever the row is stored
    index = {"rows": None, "gather": rng.integers(0, NX, R), "perm": rng.permutation(R)}[mode]
    out = ref.forward(x, ptr, w, index)
    grad_x, grad_w = ref.backward(x, ptr, w, g, index)
    return ptr, x, w, g, index, out, grad_x, grad_w


def cuda(a, dtype=None, offset=False):
    """a on the device; offset: as a contiguous view that starts one element past an allocation."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = t if dtype is None else t.to(dtype)
    if offset:
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
        flat[1:] = t.reshape(-1)
        t = flat[1:].view(t.shape)
    return t


def blank(shape, dtype):
    """An output of `shape` that starts as 0xAB bytes."""
    nbytes = tuple(shape[:-1]) + (shape[-1] * dtype.itemsize,)
    return torch.full(nbytes, 0xAB, dtype=torch.uint8, device="cuda").view(dtype)


def assert_exact(got, want, dtype):
    want = np.asarray(want, np.float32) if dtype == torch.float32 else ref.round_bf16(want)
    assert np.array_equal(got.float().cpu().numpy(), want)


def placed(a, index, mode):
    """Rows in the order the op stores them: row r at out_index[r] in the permuted form."""
    if mode != "perm":
        return a
    out = np.empty_like(a)
    out[index] = a
    return out


@pytest.mark.parametrize("trans_w", (False, True))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,F", SHAPES)
def test_raw_forward(K, F, dtype, mode, trans_w):
    ptr, x, w, _, index, want, _, _ = case(K, F, mode)
    dt = DTYPES[dtype]
    weight = cuda(w.transpose(0, 2, 1) if trans_w else w, dt)
    out = blank(want.shape, dt)
    got = ops.segment_matmul(cuda(x, dt), cuda(ptr), weight, index=cuda(index), trans_w=trans_w,
                             out_index=cuda(index) if mode == "perm" else None, out=out)
    assert got is out
    assert_exact(got, placed(want, index, mode), dt)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,F", SHAPES)
def test_raw_weight_gradient(K, F, dtype, mode):
    ptr, x, _, g, index, _, _, want = case(K, F, mode)
    dt = DTYPES[dtype]
    out = blank(want.shape, dt)
    ops.segment_matmul_bw_weight(cuda(x, dt), cuda(ptr), cuda(placed(g, index, mode), dt), index=cuda(index),
                                 out_index=cuda(index) if mode == "perm" else None, out=out)
    assert_exact(out, want, dt)


@pytest.mark.parametrize("dtype,K,F", (("fp32", 2 * BK + 3, BN), ("bf16", BK, BN + 1)))
def test_narrow_loads_from_an_offset_base(dtype, K, F):
    """K (fp32) or F (bf16) odd and every dense operand one element past an allocation: the element-load path."""
    ptr, x, w, g, index, want, _, want_w = case(K, F, "gather")
    dt = DTYPES[dtype]
    xd, gd, out, out_w = cuda(x, dt, True), cuda(g, dt, True), blank(want.shape, dt), blank(want_w.shape, dt)
    assert xd.data_ptr() % 16 == dt.itemsize
    ops.segment_matmul(xd, cuda(ptr), cuda(w, dt, True), index=cuda(index), out=out)
    ops.segment_matmul_bw_weight(xd, cuda(ptr), gd, index=cuda(index), out=out_w)
    assert_exact(out, want, dt)
    assert_exact(out_w, want_w, dt)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,F", ((BK + 1, BN + 1), (128, 2 * BN), (3, 4)))
def test_public_op_and_its_gradients(K, F, dtype, mode):
    """ps.segment_matmul (a gather or none) and, for the permuted form, ps.typed_matmul on the type vector whose
    stable sort is that permutation; the empty segments are types without rows."""
    ptr, x, w, g, index, want, want_x, want_w = case(K, F, mode)
    dt = DTYPES[dtype]
    xd, wd = cuda(x, dt).requires_grad_(), cuda(w, dt).requires_grad_()
    if mode == "perm":
        types = np.empty(len(x), np.int64)
        types[index] = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
        index = np.argsort(types, kind="stable")  # the op's permutation; the reference rows follow it
        want, (want_x, want_w) = ref.forward(x, ptr, w, index), ref.backward(x, ptr, w, g, index)
        out = ps.typed_matmul(xd, cuda(types), wd)
        with pytest.raises(AssertionError):
            ps.typed_matmul(xd, cuda(types) + len(w), wd)  # every type id at or above T
    else:
        out = ps.segment_matmul(xd, cuda(ptr), wd, index=cuda(index), trust_data=False)
    out.backward(cuda(placed(g, index, mode), dt))
    assert_exact(out.detach(), placed(want, index, mode), dt)
    assert_exact(xd.grad, want_x, dt)
    assert_exact(wd.grad, want_w, dt)


def test_many_short_segments():
    """T = 5000 segments of 0 .. 3 rows: the map kernels loop, and most tiles of the grid bound are idle."""
    lengths = tuple(np.random.default_rng(5).integers(0, 4, 5000).tolist())
    ptr, x, w, g, _, want, _, want_w = case(5, 3, "rows", lengths)
    out, out_w = blank(want.shape, torch.float32), blank(want_w.shape, torch.float32)
    ops.segment_matmul(cuda(x), cuda(ptr), cuda(w), out=out)
    ops.segment_matmul_bw_weight(cuda(x), cuda(ptr), cuda(g), out=out_w)
    assert_exact(out, want, torch.float32)
    assert_exact(out_w, want_w, torch.float32)


def test_random_data_within_the_dot_product_bound_and_reproducible():
    """|got - ref| <= (K + 2) 2^-24 sum_k |x_rk| |w_kf|: the bound of a length-K fp32 dot product in any order with
    fused multiply-adds.  Two runs of the forward and of the weight gradient (long segments) give the same bits."""
    rng = np.random.default_rng(7)
    ptr, K, F = csr(LENGTHS), 128, BN + 1
    x = rng.standard_normal((int(ptr[-1]), K)).astype(np.float32)
    w = rng.standard_normal((len(LENGTHS), K, F)).astype(np.float32)
    xd, wd, pd = cuda(x), cuda(w), cuda(ptr)
    got = ops.segment_matmul(xd, pd, wd)
    bound = (K + 2) * 2.0 ** -24 * ref.forward(np.abs(x), ptr, np.abs(w))
    assert np.all(np.abs(got.cpu().numpy() - ref.forward(x, ptr, w)) <= bound)
    assert torch.equal(got, ops.segment_matmul(xd, pd, wd))
    assert torch.equal(ops.segment_matmul_bw_weight(xd, pd, got), ops.segment_matmul_bw_weight(xd, pd, got))


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_values_stay_in_their_rows(dtype):
    """One NaN in a row of x and one inf in one weight[t], segment lengths and K off the tile sizes: the float64
    reference has the same NaN and inf elements, all inside that row and that segment, and every other element
    is exact."""
    lengths, K, F = (0, BM + 3, 5, 2 * BM - 1, 0, 7), BK + 1, BN + 1
    ptr, x, w, _, _, _, _, _ = case(K, F, "rows", lengths)
    x, w = x.copy(), w.copy()
    nan_row, inf_seg = int(ptr[1]) + BM + 1, 3
    x[nan_row, K - 1] = np.nan
    w[inf_seg, K - 1, 2] = np.inf
    with np.errstate(invalid="ignore"):
        want = ref.forward(x, ptr, w)
    dt = DTYPES[dtype]
    got = ops.segment_matmul(cuda(x, dt), cuda(ptr), cuda(w, dt), out=blank(want.shape, dt)).float().cpu().numpy()
    rows = np.flatnonzero(~np.isfinite(got).all(axis=1))
    assert set(rows) <= {nan_row} | set(range(ptr[inf_seg], ptr[inf_seg + 1])) and nan_row in rows
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    fine = np.isfinite(want)
    exact = want.astype(np.float32) if dt == torch.float32 else ref.round_bf16(np.where(fine, want, 0))
    assert np.array_equal(got[fine], exact[fine])


def test_graph_capture_replays_on_changed_x():
    ptr, x, w, _, index, _, _, _ = case(BK + 1, BN + 1, "gather")
    xd, wd, pd, idx = cuda(x), cuda(w), cuda(ptr), cuda(index)
    out = torch.empty((len(index), BN + 1), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.segment_matmul(xd, pd, wd, index=idx, out=out)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.segment_matmul(xd, pd, wd, index=idx, out=out)
    for shift in (1.0, -3.0, 2.0):
        xd.add_(shift)
        graph.replay()
        assert torch.equal(out, ops.segment_matmul(xd, pd, wd, index=idx))
