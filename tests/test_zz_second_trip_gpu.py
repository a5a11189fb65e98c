"""Second-trip tests: every kernel that walks a device-side work list on a fixed or capped grid, on a list longer
than its grid, so that the body of `for (c = wave; c < total; c += num_waves)` runs a second time — for some
waves only (tests/grid_cases.py builds lists one and a half grids long).

A wave that keeps state across trips (accumulators, a staged row, a softmax partial), stores its partials at
the wrong stride on trip two, or drops the tail past num_waves fails here.  Every case
  * asserts, on the data it runs, the property it exists for (chunks > waves, listed rows > waves, tiles per
    block >= 3, ...), recomputed from the graph alone by grid_cases.listed / saint_blocks;
  * runs with poisoned scratch (ops._POISON_WORKSPACE): without it the caching allocator can hand back the
    previous call's correct partials and hide a skipped chunk;
  * is held to its family's own exact regime and reference (tests/exact_ref.py, heads_ref.py, softmax_ref.py,
    attention_ref.py, gat_ref.py, dropout_ref.py, intersect_ref.py, test_walk_saint.py): bit for bit, or the
    bound derived in the family's own test file.  No tolerance is introduced here.

Graphs are built once per module and shared.  (The file sorts behind every other test file on purpose, as the other
test_zz_* files do: new GPU tests are appended to the suite's order, not inserted into it.)"""
import functools

import numpy as np
import pytest
import torch

import attention_ref as ar
import bf16_ref
import dropout_ref as dr
import gat_ref as gr
import grid_cases as gc
import heads_ref as hr
import intersect_ref as ir
import softmax_ref as sr
from exact_ref import assert_exact_preconditions, csr_with_col_degrees, int_data
from test_exact_spmm_gpu import Spy, assert_backward, assert_forward, autograd_step, cuda

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
U = 2.0 ** -24
INF = float("inf")
REDUCES = ["sum", "mean", "min", "max"]
BUILDERS = ["many_chunks", "many_long_rows"]
CAPPED = gc.GRIDS["heads"]["sweep"]  # 16 384 waves: the heads / softmax / attention launches at their cap
assert CAPPED == gc.GRIDS["softmax"]["sweep"] == gc.GRIDS["attention"]["sweep"] == gc.GRIDS["heads_half"]["sweep"]


@pytest.fixture(scope="module", autouse=True)
def poisoned_scratch():
    """Scratch starts as 0xff bytes in every call of this module (read at call time in ops._workspace)."""
    from paddle_sparse_amd import ops

    old, ops._POISON_WORKSPACE = ops._POISON_WORKSPACE, True
    yield
    ops._POISON_WORKSPACE = old


@functools.lru_cache(maxsize=None)
def graph_np(builder, waves, pow2=False, N=600):
    rowptr, col = getattr(gc, builder)(waves, seed=waves + len(builder), pow2=pow2, N=N)
    return rowptr, col


@functools.lru_cache(maxsize=None)
def graph_t(builder, waves):
    rowptr, col = graph_np(builder, waves)
    return torch.from_numpy(rowptr.copy()), torch.from_numpy(col.copy())


def assert_second_trip(builder, ptr, waves):
    """The property the case exists for, on the pointers it runs: more chunks on the list than a launch of `waves`
    waves takes in one trip, and under many_long_rows more listed rows than that as well (the combine loops, where
    the combine launch has `waves` waves too)."""
    rows, chunks = gc.listed(np.asarray(ptr))
    assert chunks > waves, (chunks, waves)
    if builder == "many_long_rows":
        assert rows > waves, (rows, waves)
    return rows, chunks


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def tensor_of(rowptr, col, n, value=None):
    import paddle_sparse_amd as psa

    return psa.SparseTensor(rowptr=dev(rowptr), col=dev(col), value=value, sparse_sizes=(rowptr.size - 1, n),
                            is_sorted=True)


# ---------------------------------------------------------------------------------------------
# fp32 SpMM forward
# ---------------------------------------------------------------------------------------------

# route -> (family of GRIDS, K).  K = 4: q = 1 <= 4, the multirow kernel (spmm_dispatch, spmm.hip:1393), whose rows
# above 128 entries go to spmm_long_chunk_kernel + spmm_long_combine_kernel (launch_long, spmm.hip:918: 512 x 1024
# threads = 8192 waves each).  K = 68: q = 17 > 16 with a workspace, the fused-roles kernel (spmm.hip:1411, 1431),
# whose chunk role has kFusedChunkBlocksDefault x 4 = 3072 waves (spmm.hip:649) and whose combine is the 8192-wave
# launch again.  algo="row_waves" keeps the edge-range family out (spmm.hip:1345); nothing is chosen in Python.
ROUTES = {"chunk_and_combine": ("spmm_long", 4), "fused_roles": ("spmm_fused", 68)}


@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_fp32_forward(route, builder, reduce):
    """out, arg_out and the two-byte row-local form, bit for bit against spmm_ref on integer data, with values and
    without.  many_long_rows gives the 8192-wave combine its second trip on the K = 4 route; on the fused route the
    graph is sized for the 3072-wave chunk role (three trips there), its combine stays within one."""
    from paddle_sparse_amd import ops

    family, K = ROUTES[route]
    waves = gc.GRIDS[family]["sweep"]
    rowptr, col = graph_t(builder, waves)
    assert_second_trip(builder, rowptr, waves)
    value, mat, _ = int_data(rowptr, 600, K, seed=K)
    assert_exact_preconditions(rowptr, col, value, mat)
    for val in (value, None):
        res = ops._spmm(reduce, cuda(rowptr), cuda(col), cuda(val), cuda(mat), want_arg_bytes=2, algo="row_waves")
        assert_forward(reduce, rowptr, col, val, mat, res)


@pytest.mark.parametrize("reduce", REDUCES)
def test_half_forward(reduce):
    """The half-width forward (psa_spmm_half) keeps every row on its own wave — it has no chunk list — so this is the
    same graph through it for completeness: bf16 operands, fp32 sums, one rounding."""
    from paddle_sparse_amd import ops

    rowptr, col = graph_t("many_chunks", gc.GRIDS["spmm_long"]["sweep"])
    value, mat, _ = int_data(rowptr, 600, 8, dtype=BF, seed=8)
    assert_exact_preconditions(rowptr, col, value, mat)
    assert_forward(reduce, rowptr, col, value, mat, ops._spmm(reduce, cuda(rowptr), cuda(col), cuda(value), cuda(mat)))


# ---------------------------------------------------------------------------------------------
# SpMM backward
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("builder", BUILDERS)
def test_value_bw_long_rows(builder):
    """grad_value alone: spmm_value_bw (spied), whose rows above 128 entries go to spmm_value_bw_long_kernel on
    kLongBlocks x kLongThreads = 8192 waves (spmm_bw.hip:296), one wave per chunk."""
    waves = gc.GRIDS["spmm_long"]["sweep"]
    rowptr, col = graph_t(builder, waves)
    assert_second_trip(builder, rowptr, waves)
    value, mat, grad = int_data(rowptr, 600, 4, seed=11)
    assert_exact_preconditions(rowptr, col, value, mat, grad)
    with Spy("spmm_value_bw", "spmm_sum_bw_csc") as spy:
        out, gv, gm = autograd_step(rowptr, col, value, mat, grad, "sum", want_mat=False)
    assert len(spy.named("spmm_value_bw")) == 1 and not spy.named("spmm_sum_bw_csc")
    assert_backward("sum", rowptr, col, value, mat, grad, out, gv, None, want_mat=False)


@functools.lru_cache(maxsize=None)
def long_columns(builder, waves, M=2000):
    """A CSR matrix whose COLUMN degrees are the row degrees of the builder's graph: the long lists of the passes
    over the CSC view."""
    deg = np.diff(graph_np(builder, waves)[0])
    rowptr, col = csr_with_col_degrees(deg, M, seed=waves)
    colptr = np.concatenate([[0], np.cumsum(np.bincount(col.numpy(), minlength=deg.size))])
    assert np.array_equal(np.diff(colptr), deg)
    return rowptr, col, colptr, deg.size


@pytest.mark.parametrize("reduce", ["sum", "min", "max"])
@pytest.mark.parametrize("builder", BUILDERS)
def test_fp32_one_pass_csc_backward_long_columns(builder, reduce):
    """Both gradients in one pass over the CSC view: spmm_sum_bw_csc / spmm_minmax_bw_csc (spied), columns above 128
    entries in the chunk role of the masked fused kernel, kMaskedChunkBlocks x 4 = 1536 waves (launch_fused_masked,
    spmm.hip:991), combined by the 8192-wave launch."""
    waves = gc.GRIDS["spmm_masked"]["sweep"]
    rowptr, col, colptr, N = long_columns(builder, waves)
    assert_second_trip(builder, colptr, waves)
    value, mat, grad = int_data(rowptr, N, 4, seed=13)
    assert_exact_preconditions(rowptr, col, value, mat, grad)
    name = "spmm_sum_bw_csc" if reduce == "sum" else "spmm_minmax_bw_csc"
    with Spy(name) as spy:
        out, gv, gm = autograd_step(rowptr, col, value, mat, grad, reduce)
    assert len(spy.named(name)) == 1
    assert_backward(reduce, rowptr, col, value, mat, grad, out, gv, gm)


@pytest.mark.parametrize("reduce", ["sum", "min", "max"])
@pytest.mark.parametrize("builder", BUILDERS)
def test_half_one_pass_csc_backward_long_columns(builder, reduce):
    """bf16: spmm_half_sum_bw_csc / spmm_half_minmax_bw_csc (spied), long columns in the chunk role of
    spmm_half_csc_bw_kernel, kHalfChunkBlocks x 4 = 3072 waves (spmm_half_bw.hip:312), combined on 8192 waves."""
    waves = gc.GRIDS["spmm_half_bw"]["sweep"]
    rowptr, col, colptr, N = long_columns(builder, waves)
    assert_second_trip(builder, colptr, waves)
    value, mat, grad = int_data(rowptr, N, 8, dtype=BF, seed=17)
    assert_exact_preconditions(rowptr, col, value, mat, grad)
    name = "spmm_half_sum_bw_csc" if reduce == "sum" else "spmm_half_minmax_bw_csc"
    with Spy(name) as spy:
        out, gv, gm = autograd_step(rowptr, col, value, mat, grad, reduce)
    assert len(spy.named(name)) == 1
    assert_backward(reduce, rowptr, col, value, mat, grad, out, gv, gm)


# ---------------------------------------------------------------------------------------------
# heads: SpMM over per-head values, sddmm per head
# ---------------------------------------------------------------------------------------------

def reduce_rows(rowptr, terms):
    """Row sums of per-entry terms [nnz, ...] in float64 (np.add.reduceat; empty rows give 0)."""
    rowptr = np.asarray(rowptr)
    out = np.zeros((rowptr.size - 1,) + terms.shape[1:])
    full = np.flatnonzero(np.diff(rowptr) > 0)
    if full.size:
        out[full] = np.add.reduceat(terms, rowptr[full], axis=0)
    return out


@pytest.mark.parametrize("builder", BUILDERS)
def test_spmm_heads_exact(builder):
    """H = 2, F = 1, integers in [-4, 4] / [-2, 2] as test_heads_gpu.py: forward, grad_value (the sddmm-heads chunk
    kernel over the rows) and grad_mat (psa_spmm_heads over the CSC view, whose 600 columns are long lists too) equal
    heads_ref bit for bit.  Chunk and combine launches are at their cap of 4096 workgroups."""
    rowptr, col = graph_np(builder, CAPPED)
    assert_second_trip(builder, rowptr, CAPPED)
    assert gc.launched_waves(col.size) == (CAPPED, CAPPED)
    M, nnz, N, H, F = rowptr.size - 1, col.size, 600, 2, 1
    rng = np.random.default_rng(31)
    value, mat, g = ints(rng, (nnz, H), -4, 4), ints(rng, (N, H, F), -4, 4), ints(rng, (M, H, F), -2, 2)
    want = hr.spmm_heads_ref(rowptr, col, value, mat)
    assert np.array_equal(want, reduce_rows(rowptr, value.astype(np.float64)[:, :, None] * mat.astype(np.float64)[col]))
    want_gv = hr.spmm_heads_grad_value(rowptr, col, mat, g)
    want_gm = hr.spmm_heads_grad_mat(rowptr, col, value, g, N)
    assert np.abs(want).max() < 2 ** 24 and np.abs(want_gm).max() < 2 ** 24 and np.abs(want_gv).max() < 2 ** 24
    # (the bound on the sums of magnitudes, which is what any order of the additions needs)
    assert np.diff(rowptr).max() * 16 < 2 ** 24 and np.bincount(col).max() * 8 < 2 ** 24
    vd, md = dev(value).requires_grad_(), dev(mat).requires_grad_()
    out = tensor_of(rowptr, col, N, vd) @ md
    out.backward(dev(g))
    assert np.array_equal(host(out), want)
    assert np.array_equal(host(vd.grad), want_gv)
    assert np.array_equal(host(md.grad), want_gm)


@pytest.mark.parametrize("builder", BUILDERS)
def test_sddmm_heads_exact(builder):
    """Multi-head sddmm, H = 2, K = 1: the values (sddmm_heads_chunk_kernel), grad_x (psa_spmm_heads over the rows) and
    grad_y (over the CSC view)."""
    import paddle_sparse_amd as psa

    rowptr, col = graph_np(builder, CAPPED)
    assert_second_trip(builder, rowptr, CAPPED)
    M, nnz, N, H, K = rowptr.size - 1, col.size, 600, 2, 1
    rng = np.random.default_rng(37)
    x, y, g = ints(rng, (M, H, K), -4, 4), ints(rng, (N, H, K), -4, 4), ints(rng, (nnz, H), -2, 2)
    want = hr.sddmm_heads_ref(rowptr, col, x, y)
    want_gx = hr.sddmm_heads_grad_x(rowptr, col, y, g)
    want_gy = hr.sddmm_heads_grad_y(rowptr, col, x, g, N)
    assert np.abs(want_gx).max() < 2 ** 24
    assert np.diff(rowptr).max() * 8 < 2 ** 24 and np.bincount(col).max() * 8 < 2 ** 24
    A = tensor_of(rowptr, col, N)
    xd, yd = dev(x).requires_grad_(), dev(y).requires_grad_()
    v = psa.sddmm(A, xd, yd).storage.value()
    assert v.shape == (nnz, H)
    v.backward(dev(g))
    assert np.array_equal(host(v), want)
    assert np.array_equal(host(xd.grad), want_gx)
    assert np.array_equal(host(yd.grad), want_gy)


@pytest.mark.parametrize("builder", BUILDERS)
def test_spmm_heads_half_exact(builder):
    """psa_spmm_heads_half, H = 2, F = 1 (the 2-byte form) and F = 8 (the 16-byte form): integers as
    test_attention_half_gpu.py::test_spmm_heads_half_exact (value in [1, 3], mat in [0, 3], odd features negative, so
    sums pass 256 and do round), fp32 sums exact, the result the reference rounded once to bf16."""
    from paddle_sparse_amd import ops

    rowptr, col = graph_np(builder, CAPPED)
    assert_second_trip(builder, rowptr, CAPPED)
    nnz, N, H = col.size, 600, 2
    rp, cl = dev(rowptr), dev(col)
    for F in (1, 8):
        rng = np.random.default_rng(41 + F)
        value, mat = ints(rng, (nnz, H), 1, 3), ints(rng, (N, H, F), 0, 3)
        mat[:, :, 1::2] *= -1
        want = reduce_rows(rowptr, value.astype(np.float64)[:, :, None] * mat.astype(np.float64)[col])
        assert 256 < np.abs(want).max() < 2 ** 24
        out = ops.spmm_heads_half_raw(rp, cl, dev(value), dev(mat).to(BF))
        assert out.dtype == BF and np.array_equal(host(out), bf16_ref.round_bf16(want.astype(np.float32)))


# ---------------------------------------------------------------------------------------------
# segment softmax
# ---------------------------------------------------------------------------------------------

def softmax_exact_case(indptr, D, rng, pow2):
    """The exact regime of test_softmax_gpu.py (exact_case), vectorised: per segment and head one finite constant in L
    entries (L a power of two when asked, at most 2^16), -inf in the rest; expected 1 / L there and 0 elsewhere."""
    lens = np.diff(indptr)
    n, nseg = int(indptr[-1]), lens.size
    seg = np.repeat(np.arange(nseg), lens)
    src = np.full((n, D), -INF, dtype=np.float32)
    want = np.zeros((n, D), dtype=np.float32)
    for h in range(D):
        if pow2:
            top = np.minimum(np.floor(np.log2(np.maximum(lens, 1))).astype(np.int64), 16)
            L = np.int64(1) << rng.integers(0, top + 1)
        else:
            L = rng.integers(1, np.maximum(lens, 1) + 1)
        order = np.argsort(seg + rng.random(n))            # a random order of the entries inside every segment
        rank = np.arange(n) - indptr[:-1][seg]
        live = order[rank < L[seg]]
        const = (rng.integers(-50, 50, nseg).astype(np.float32) / np.float32(4))
        src[live, h] = const[seg[live]]
        want[live, h] = (np.float32(1) / L.astype(np.float32))[seg[live]]
    return src, want


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("builder", BUILDERS)
def test_softmax_exact(builder, D):
    """Forward (L anywhere in 1 .. len) and backward (L a power of two, integer upstream gradients) bit for bit, with
    the segment lengths of the builders: softmax_chunk_kernel, softmax_combine_kernel and softmax_write_kernel all
    at their cap of 4096 workgroups x 4 waves, the first and the third with more chunks than waves, the second (under
    many_long_rows) with more listed segments than waves."""
    from paddle_sparse_amd import ops

    indptr = graph_np(builder, CAPPED)[0]
    assert_second_trip(builder, indptr, CAPPED)
    n = int(indptr[-1])
    assert gc.launched_waves(n, "softmax") == (CAPPED, CAPPED)
    rng = np.random.default_rng(200 + D)
    src, want = softmax_exact_case(indptr, D, rng, pow2=False)
    got = ops.segment_softmax(dev(src), dev(indptr))
    assert got.shape == src.shape and np.array_equal(got.cpu().numpy(), want)

    src, y = softmax_exact_case(indptr, D, rng, pow2=True)
    g = rng.integers(-8, 9, size=y.shape).astype(np.float32)
    ref = sr.softmax_bw_ref(y, g, indptr)
    want_bw = ref.astype(np.float32)
    assert np.array_equal(want_bw.astype(np.float64), ref)  # exactly representable
    got = ops.segment_softmax_bw(dev(y), dev(g), dev(indptr))
    assert np.array_equal(got.cpu().numpy(), want_bw)
    x = dev(src).requires_grad_()
    out = ops.segment_softmax(x, dev(indptr))
    out.backward(dev(g))
    assert np.array_equal(out.detach().cpu().numpy(), y) and np.array_equal(x.grad.cpu().numpy(), want_bw)


def test_softmax_general_values_within_the_derived_bounds():
    """General values on many_chunks, D = 2, held to the bounds test_softmax_gpu.py derives (u = 2^-24):
    forward |out - ref64| <= (len + 64) u ref64; backward |grad - ref64| <= (len + 8) u y (|g| + sum |y g|)."""
    from paddle_sparse_amd import ops

    indptr = graph_np("many_chunks", CAPPED)[0]
    assert_second_trip("many_chunks", indptr, CAPPED)
    n, D = int(indptr[-1]), 2
    rng = np.random.default_rng(300)
    src = rng.uniform(-8, 8, size=(n, D)).astype(np.float32)
    g = rng.normal(size=(n, D)).astype(np.float32)
    got = ops.segment_softmax(dev(src), dev(indptr))
    y = got.cpu().numpy()
    ref = sr.softmax_ref(src, indptr)
    length = sr.segment_lengths(indptr, n, None, (D,))
    err = np.abs(y.astype(np.float64) - ref)
    bound = (length + 64) * U * ref
    print(f"forward: worst err / bound = {float(np.max(err / np.maximum(bound, 1e-300))):.3f}")
    assert np.all(err <= bound)
    got_bw = ops.segment_softmax_bw(got, dev(g), dev(indptr)).cpu().numpy()
    ref_bw = sr.softmax_bw_ref(y, g, indptr)
    _, scale = sr.softmax_bw_bound_terms(y, g, indptr)
    err = np.abs(got_bw.astype(np.float64) - ref_bw)
    bound = (length + 8) * U * y.astype(np.float64) * scale
    print(f"backward: worst err / bound = {float(np.max(err / np.maximum(bound, 1e-300))):.3f}")
    assert np.all(err <= bound)


# ---------------------------------------------------------------------------------------------
# fused attention: fp32, bf16, GAT, dropout — one kernel template (attention_kernels.h)
# ---------------------------------------------------------------------------------------------

ATT_N = 1 << 18  # columns: few entries per column, so that the column sums of dS stay within 24 bits (below)


def uniform_graph(builder):
    """The pow2 variant of the builders (row lengths 512 and 256 among 0, 1, 2, 4) over ATT_N columns."""
    rowptr, col = graph_np(builder, CAPPED, True, ATT_N)
    deg = np.diff(rowptr)
    assert np.all(deg[deg > 0] & (deg[deg > 0] - 1) == 0)
    assert_second_trip(builder, rowptr, CAPPED)
    assert gc.launched_waves(col.size, "attention") == (CAPPED, CAPPED)
    return rowptr, col


def assert_sums_exact(rowptr, col, p, ds, qmax, kmax, vmax, gmax):
    """The uniform regime's claim on THIS data: every sum the kernels add is a sum of multiples of one power of two
    whose magnitudes add up to less than 2^24 of them, so fp32 is exact in any order.  In a row of `deg` entries p
    [nnz, H] (times the dropout factor where there is one) is a multiple of 1 / deg and dS of 1 / deg^2; a column
    mixes rows, so its unit is that of the longest row."""
    deg = np.diff(rowptr).astype(np.float64)[:, None]
    top = float(deg.max())
    col_abs = lambda t: max(np.bincount(col, weights=np.abs(t[:, h])).max() for h in range(t.shape[1]))
    assert (reduce_rows(rowptr, np.abs(p)) * deg).max() * vmax < 2 ** 24          # out
    assert col_abs(p) * gmax * top < 2 ** 24                                      # grad_v
    assert (reduce_rows(rowptr, np.abs(ds)) * deg ** 2).max() * kmax < 2 ** 24    # grad_q
    assert col_abs(ds) * qmax * top ** 2 < 2 ** 24                                # grad_k


def uniform_operands(rng, M, H, K, F):
    """test_attention_gpu.py::test_uniform_exact: integers in [-2, 2], k identical across the nodes per head (only
    the rows of k that a column can name are kept distinct objects; they hold the same numbers)."""
    q = ints(rng, (M, H, K), -2, 2)
    k = np.tile(ints(rng, (1, H, K), -2, 2), (ATT_N, 1, 1))
    return q, k, ints(rng, (ATT_N, H, F), -2, 2), ints(rng, (M, H, F), -2, 2)


# (builder, H): the float64 reference takes seconds at 6.3 M entries, so many_long_rows runs one head
UNIFORM_CASES = [("many_chunks", 1), ("many_chunks", 2), ("many_long_rows", 1)]


@pytest.mark.parametrize("builder,H", UNIFORM_CASES)
def test_attention_uniform_exact(builder, H):
    """fp32, K = F = 4, the uniform regime: out, grad_q (exactly 0), grad_k and grad_v bit for bit.  Forward chunk
    and combine kernels and the chunk kernel of the per-entry backward, all at their cap."""
    rowptr, col = uniform_graph(builder)
    M, K, F = rowptr.size - 1, 4, 4
    rng = np.random.default_rng(72 + H)
    q, k, v, g = uniform_operands(rng, M, H, K, F)
    want = ar.attention_ref(rowptr, col, q, k, v)
    grads = ar.attention_grads_ref(rowptr, col, q, k, v, g)
    assert_sums_exact(rowptr, col, grads["p"], grads["ds"], 2, 2, 2, 2)
    qd, kd, vd = (dev(a).requires_grad_() for a in (q, k, v))
    out = tensor_of(rowptr, col, ATT_N).attention(qd, kd, vd)
    out.backward(dev(g))
    assert np.array_equal(host(out), want)
    assert not host(qd.grad).any() and not np.abs(grads["q"]).max() > 1e-12
    assert np.array_equal(host(kd.grad), grads["k"]) and np.array_equal(host(vd.grad), grads["v"])


def test_attention_dropout_uniform_exact():
    """dropout_p = 0.5 (inv_keep = 2) in the uniform regime, as test_attention_dropout_gpu.py::test_uniform_exact:
    the mask is recomputed per entry inside the chunk loops of the forward and of the backward."""
    rowptr, col = uniform_graph("many_chunks")
    M, H, K, F = rowptr.size - 1, 2, 4, 4
    rng = np.random.default_rng(75)
    q, k, v, g = uniform_operands(rng, M, H, K, F)
    want = dr.attention_dropout_ref(rowptr, col, q, k, v, 1.0, None, 0.5, 12345)
    grads = dr.attention_dropout_grads_ref(rowptr, col, q, k, v, g, 1.0, None, 0.5, 12345)
    assert_sums_exact(rowptr, col, grads["pd"], grads["ds"], 2, 2, 2, 2)
    qd, kd, vd = (dev(a).requires_grad_() for a in (q, k, v))
    out = tensor_of(rowptr, col, ATT_N).attention(qd, kd, vd, dropout_p=0.5, seed=12345)
    out.backward(dev(g))
    assert np.array_equal(host(out), want)
    assert np.array_equal(host(qd.grad), grads["q"]) and np.array_equal(host(kd.grad), grads["k"])
    assert np.array_equal(host(vd.grad), grads["v"])


@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("builder", BUILDERS)
def test_attention_bf16_uniform_exact(builder, H):
    """bf16, K = F = 8 (the 16-byte form), the uniform regime of test_attention_half_gpu.py: q = 0, so p = 1 / length,
    and v in {-1, 0, 1} whose row sums stay below 256: out is an integer of at most 8 bits over a power of two, a
    bf16 number, and must come out exactly.  (That file's uniform regime has no backward; neither has this.)"""
    rowptr, col = uniform_graph(builder)
    M, K, F = rowptr.size - 1, 8, 8
    rng = np.random.default_rng(76 + H)
    q = np.zeros((M, H, K), dtype=np.float32)
    k, v = ints(rng, (ATT_N, H, K), -3, 3), ints(rng, (ATT_N, H, F), -1, 1)
    sums = reduce_rows(rowptr, v.astype(np.float64)[col])
    assert 16 < np.abs(sums).max() < 256
    want = sums / np.maximum(np.diff(rowptr), 1)[:, None, None]
    assert bf16_ref.is_bf16(want).all()
    out = tensor_of(rowptr, col, ATT_N).attention(dev(q).to(BF), dev(k).to(BF), dev(v).to(BF))
    assert out.dtype == BF and np.array_equal(host(out), want)


@pytest.mark.parametrize("builder,H", UNIFORM_CASES)
def test_gat_attention_uniform_exact(builder, H):
    """GAT scores, fp32, F = 4, the "negative" case of test_gat_attention_gpu.py::test_uniform_exact: a_col = -32 for
    every node, slope = 1/2, z < 0 throughout; v in [-2, 2], g in [-1, 1].  out, grad_a_row (exactly 0), grad_a_col
    and grad_v bit for bit."""
    rowptr, col = uniform_graph(builder)
    M, F = rowptr.size - 1, 4
    rng = np.random.default_rng(78 + H)
    a_row = ints(rng, (M, H), -3, 3)
    a_col = np.full((ATT_N, H), -32.0, dtype=np.float32)
    v, g = ints(rng, (ATT_N, H, F), -2, 2), ints(rng, (M, H, F), -1, 1)
    assert np.all(gr.z_ref(rowptr, col, a_row, a_col) < 0)
    want = gr.gat_ref(rowptr, col, a_row, a_col, v, 0.5)
    grads = gr.gat_grads_ref(rowptr, col, a_row, a_col, v, g, 0.5)
    assert np.array_equal(grads["dz"], grads["ds"] / 2) and np.abs(grads["a_col"]).max() > 0
    assert_sums_exact(rowptr, col, grads["p"], grads["ds"], 1, 1, 2, 1)  # grad_a_row / _col: sums of dZ itself
    rd, cd, vd = (dev(a).requires_grad_() for a in (a_row, a_col, v))
    out = tensor_of(rowptr, col, ATT_N).gat_attention(rd, cd, vd, negative_slope=0.5)
    out.backward(dev(g))
    assert np.array_equal(host(out), want)
    assert not host(rd.grad).any() and not np.abs(grads["a_row"]).max() > 1e-12
    assert np.array_equal(host(cd.grad), grads["a_col"]) and np.array_equal(host(vd.grad), grads["v"])


def test_gat_attention_bf16_uniform_exact():
    """The same case in bf16 (F = 8, the 16-byte form), as the BF leg of test_gat_attention_gpu.py::test_uniform_exact:
    out must be a bf16 number (asserted), so that the delta of the backward is exact; every bf16 result is the
    reference rounded once.  The bf16 forward and per-entry backward come from the same template as the fp32 ones."""
    rowptr, col = uniform_graph("many_chunks")
    M, H, F = rowptr.size - 1, 1, 8
    rng = np.random.default_rng(81)
    a_row = ints(rng, (M, H), -3, 3)
    a_col = np.full((ATT_N, H), -32.0, dtype=np.float32)
    v, g = ints(rng, (ATT_N, H, F), -2, 2), ints(rng, (M, H, F), -1, 1)
    want = gr.gat_ref(rowptr, col, a_row, a_col, v, 0.5)
    grads = gr.gat_grads_ref(rowptr, col, a_row, a_col, v, g, 0.5)
    assert bf16_ref.is_bf16(want).all() and np.abs(grads["a_col"]).max() > 0
    assert_sums_exact(rowptr, col, grads["p"], grads["ds"], 1, 1, 2, 1)
    rd, cd, vd = (dev(a).to(BF).requires_grad_() for a in (a_row, a_col, v))
    out = tensor_of(rowptr, col, ATT_N).gat_attention(rd, cd, vd, negative_slope=0.5)
    out.backward(dev(g).to(BF))
    assert out.dtype == BF and np.array_equal(host(out), gr.once_rounded(want))
    assert not host(rd.grad).any()
    assert np.array_equal(host(cd.grad), gr.once_rounded(grads["a_col"]))
    assert np.array_equal(host(vd.grad), gr.once_rounded(grads["v"]))


# ---------------------------------------------------------------------------------------------
# attention_dropout_mask
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", [1, 5])
def test_dropout_mask_past_one_sweep(H):
    """nnz * H = 16 777 216 + 4 099 elements on 65 536 x 256 lanes: the tail takes a second trip.  H = 5 (the count is
    5 x 3 356 263) has an entry whose heads straddle the end of the sweep.  The whole array against
    dropout_ref.keep_ref."""
    from paddle_sparse_amd import ops

    sweep = gc.GRIDS["dropout_mask"]["sweep"]
    total = sweep + 4099
    assert total % H == 0 and total > sweep and (H == 1 or sweep % H != 0)
    nnz = total // H
    got = ops.attention_dropout_mask(nnz, H, 0.5, 2024)
    assert got.shape == (nnz, H)
    assert np.array_equal(got.cpu().numpy(), dr.keep_ref(nnz, H, 0.5, 2024))


# ---------------------------------------------------------------------------------------------
# pair_intersect / masked_spspmm
# ---------------------------------------------------------------------------------------------

def short_lists(rng, n_lists, universe):
    """A list family of 0 - 3 ascending, distinct indices each, with integer values in [-3, 3]."""
    lens = rng.integers(0, 4, n_lists)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    # distinct and ascending: a random start and strictly positive steps
    pos = np.arange(int(ptr[-1])) - np.repeat(ptr[:-1], lens)
    idx = (np.repeat(rng.integers(0, universe - 8, n_lists), lens) + pos * np.repeat(rng.integers(1, 4, n_lists), lens))
    return ptr, idx.astype(np.int64), rng.integers(-3, 4, idx.size).astype(np.float32)


def intersect_small_ref(x, y, pair_x, pair_y, weight):
    """intersect_ref.pair_intersect_math for lists of at most 3 entries, vectorised: all 9 (i, j) positions.  On
    integer data the sums are exact, so this is also pair_intersect_ordered's result bit for bit (asserted on
    samples by the caller)."""
    (xp, xi, xv), (yp, yi, yv) = x, y
    out = np.zeros(pair_x.size, np.float64)
    xs, xn = xp[pair_x], xp[pair_x + 1] - xp[pair_x]
    ys, yn = yp[pair_y], yp[pair_y + 1] - yp[pair_y]
    for i in range(3):
        for j in range(3):
            ok = (i < xn) & (j < yn)
            a, b = np.where(ok, xs + i, 0), np.where(ok, ys + j, 0)
            hit = ok & (xi[a] == yi[b])
            out += np.where(hit, xv[a].astype(np.float64) * yv[b] * weight[np.where(hit, xi[a], 0)], 0.0)
    return out


def test_pair_intersect_past_one_sweep():
    """2 097 152 + 1 000 003 pairs of short lists (0 - 3 entries, integer values and weights, so every order of the
    additions gives the same fp32 number) on 65 536 workgroups x 4 waves x 8 pairs: the tail is a second sweep, in
    which a few pairs of 40-entry lists run in long mode (probe list above PSA_INTERSECT_T = 32).  Bit for bit
    against the vectorised restatement, which is held to intersect_ref on the first pairs, the pairs around the
    sweep boundary, the long pairs and the last ones."""
    from paddle_sparse_amd import ops

    sweep = gc.GRIDS["pair_intersect"]["sweep"]
    P, universe, L = sweep + 1_000_003, 4000, 50_000
    rng = np.random.default_rng(51)
    xp, xi, xv = short_lists(rng, L, universe)
    yp, yi, yv = short_lists(rng, L, universe)
    # two long lists per family at the end: 40 ascending entries each
    for fam in ("x", "y"):
        p, i, v = (xp, xi, xv) if fam == "x" else (yp, yi, yv)
        extra = [np.sort(rng.choice(80, 40, replace=False)) for _ in range(2)]  # 40 of 80: about 20 in common
        i = np.concatenate([i] + extra).astype(np.int64)
        v = np.concatenate([v, rng.integers(-3, 4, 80).astype(np.float32)])
        p = np.concatenate([p, p[-1] + np.array([40, 80])]).astype(np.int64)
        if fam == "x":
            xp, xi, xv = p, i, v
        else:
            yp, yi, yv = p, i, v
    weight = rng.integers(-2, 3, universe).astype(np.float32)
    pair_x, pair_y = rng.integers(0, L, P), rng.integers(0, L, P)
    long_at = sweep + np.array([5, 8 * 4 * 1000 + 3, 999_999])  # in the second sweep, one of them in the last wave
    pair_x[long_at], pair_y[long_at] = [L, L + 1, L], [L, L, L + 1]
    assert P > sweep and long_at.min() >= sweep and ir.T == 32 and np.all(np.diff(xp)[pair_x[long_at]] > ir.T)
    x, y = (xp, xi, xv), (yp, yi, yv)

    want = np.zeros(P, np.float64)
    short = np.ones(P, bool)
    short[long_at] = False
    want[short] = intersect_small_ref(x, y, pair_x[short], pair_y[short], weight)
    want[long_at] = ir.pair_intersect_math(x, y, pair_x[long_at], pair_y[long_at], weight)
    sample = np.concatenate([np.arange(2000), np.arange(sweep - 1000, sweep + 1000), long_at, np.arange(P - 2000, P)])
    ordered = ir.pair_intersect_ordered(x, y, pair_x[sample], pair_y[sample], weight)
    assert np.array_equal(ordered.astype(np.float64), want[sample]) and np.abs(want[long_at]).max() > 0
    assert np.abs(want).max() < 2 ** 24

    got = ops.pair_intersect(tuple(dev(a) for a in x), tuple(dev(a) for a in y), dev(pair_x), dev(pair_y), dev(weight))
    assert got.dtype == torch.float32 and np.array_equal(host(got), want)


# ---------------------------------------------------------------------------------------------
# saint_subgraph
# ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def saint_cases():
    return gc.saint_cases()


@pytest.mark.parametrize("name", ["a_all", "a_subset", "a_unsorted", "b_runs", "c_small"])
def test_saint_subgraph(name):
    """rowptr, col, edge_index, row and value[e] of the subgraph, bit for bit.  a_*: every block walks two full
    tiles and a ragged third (q0 carried across tiles, every sub-tile and the double-buffered wave counts, the
    prefix across waves); b_runs: tiles that span more than 512 rows are searched, not staged; c_small: blocks
    with empty ranges."""
    from test_walk_saint_gpu import adj_of, gpu

    rowptr, col, idx, N = saint_cases()[name]
    b = gc.saint_blocks(rowptr, idx)
    if name.startswith("a_"):
        assert b["tiles_per_block"].min() >= 3 and np.all(b["per_block"] % gc.SAINT_TILE != 0)
        assert (rowptr[idx + 1] - rowptr[idx]).max() > 3 * gc.SAINT_TILE
    elif name == "b_runs":
        wide = np.flatnonzero(b["rows_per_tile"] > gc.SAINT_ROWS)
        assert wide.size == 2 and np.all(b["rows_per_tile"][wide + 1] <= gc.SAINT_ROWS)
    else:
        assert 0 < b["C"] < gc.SAINT_BLOCKS and (b["per_block"] == 0).any()
    value = torch.arange(col.size, dtype=torch.float32, device=DEV) % 4093
    sub, e = adj_of(rowptr, col, value).saint_subgraph(gpu(idx))
    p, c, er = gc.saint_ref(rowptr, col, idx, N)
    S = idx.size
    if name == "a_subset":
        assert 0.4 < er.size / b["C"] < 0.6  # mixed keep and drop decisions
    assert sub.sparse_sizes() == (S, S)
    assert np.array_equal(sub.storage.rowptr().cpu().numpy(), p)
    assert np.array_equal(sub.storage.col().cpu().numpy(), c)
    assert np.array_equal(e.cpu().numpy(), er)
    assert np.array_equal(sub.storage.row().cpu().numpy(), np.repeat(np.arange(S), np.diff(p)))
    assert torch.equal(sub.storage.value(), value[e])
