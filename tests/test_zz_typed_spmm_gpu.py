"""GPU suite for typed_spmm (csrc/typed_spmm.hip, typed_spmm.py) against the float64 restatement of
tests/typed_spmm_ref.py, on ONE graph: M = N = (CS + 1) * 64 + 1 rows (the last tile holds one row), T = 5.  Type 4
never occurs, type 2 lives in nine tiles only, tile 7 and most rows hold no entry, type 0 lives in CS + 1 tiles and
type 1 in exactly CS (the fold and the direct route of the weight gradient), (row, col) pairs repeat with other types,
and row 70 holds PASS + 90 entries of type 3: more than one pass of the gather.

Exact data: x integers in [-4, 4], values absent or out of {1, 2}, weights out of {-2, -1, -0.5, 0.5, 1, 2}, cotangents
integers in [-4, 4], K and F at most 130, at most 200 entries per row, 12 per column and 2000 in all.  So |H| <= 1600
(integers), every partial sum of the forward is a multiple of 0.5 below 200 * 8 * 2 * 130 < 2^19, of grad_x one below
12 * 8 * 2 * 130 * 5 < 2^17, and of grad_weight an integer below 2000 * 8 * 4 = 2^16: exact in fp32 in any order, and
the bf16 rounding of H keeps all three bounds.  fp32 results equal the reference bit for bit, bf16 results the
reference with H rounded to bf16 and the result rounded once.  Outputs of the raw ops start as 0xAB bytes."""
import functools
import itertools

import numpy as np
import pytest
import torch

import paddle_sparse_amd as ps
import typed_spmm_ref as ref
from paddle_sparse_amd import ops
from segment_matmul_ref import round_bf16

pytestmark = pytest.mark.gpu

BM, BK, CS, PASS = ops.TYPED_SPMM_BM, ops.TYPED_SPMM_BK, ops.TYPED_SPMM_CS, ops.TYPED_SPMM_PASS
M, T, EMPTY_TILE, HUB = (CS + 1) * BM + 1, 5, 7, BM + 6
SHAPES = tuple(itertools.product((1, 3, BK, BK + 1, 130), (1, 3, 64, 65, 130)))
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


@functools.lru_cache(maxsize=None)
def graph():
    """(row, col, etype) in storage order (by row, then column, stable) and the plan on the device."""
    rng = np.random.default_rng(3)
    tiles = [t for t in range(CS + 2) if t != EMPTY_TILE]  # CS + 1 of them; the last one is the one-row tile
    spot = lambda ts: [min(t * BM + int(rng.integers(BM)), M - 1) for t in ts]  # noqa: E731
    parts = [(spot(tiles), 0), (spot(tiles[:CS]), 1), (spot(tiles[:9]), 2), ([HUB] * (PASS + 90), 3), ([HUB] * 5, 0),
             (spot(rng.choice(tiles[:40], 300)), 3), (spot(rng.choice(tiles[:40], 300)), 0)]
    row = np.concatenate([np.asarray(r, np.int64) for r, _ in parts])
    etype = np.concatenate([np.full(len(r), t, np.int64) for r, t in parts])
    col = rng.integers(0, M, len(row))
    col[row == HUB] = rng.permutation(M)[:(row == HUB).sum()]
    extra = np.flatnonzero(etype == 1)[::3]  # the same (row, col) again under type 0: a multigraph
    row, col, etype = (np.concatenate([a, b]) for a, b in ((row, row[extra]), (col, col[extra]),
                                                          (etype, np.zeros(len(extra), np.int64))))
    order = np.lexsort((col, row))
    row, col, etype = row[order], col[order], etype[order]
    assert np.bincount(row).max() <= 200 and np.bincount(col).max() <= 12 and len(row) <= 2000
    adj = ps.SparseTensor(row=cuda(row), col=cuda(col), sparse_sizes=(M, M), is_sorted=True)
    return row, col, etype, ps.RelationalPlan(adj, cuda(etype), T)


@functools.lru_cache(maxsize=None)
def case(K, F, valued, bf16=False):
    """Operands, a cotangent and the float64 results of one shape; nothing here is written again."""
    row, col, etype, _ = graph()
    rng = np.random.default_rng(1000 * K + F)
    x = rng.integers(-4, 5, (M, K)).astype(np.float32)
    w = rng.choice(np.array([-2, -1, -0.5, 0.5, 1, 2], np.float32), (T, K, F))
    g = rng.integers(-4, 5, (M, F)).astype(np.float32)
    value = rng.integers(1, 3, len(row)).astype(np.float32) if valued else None
    out = ref.forward(row, col, etype, x, w, value, M, bf16)
    grad_x, grad_w = ref.backward(row, col, etype, x, w, g, value, bf16)
    return x, w, g, value, out, grad_x, grad_w


def cuda(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def blank(shape, dtype):
    nbytes = tuple(shape[:-1]) + (shape[-1] * dtype.itemsize,)
    return torch.full(nbytes, 0xAB, dtype=torch.uint8, device="cuda").view(dtype)


def assert_exact(got, want, dtype):
    want = np.asarray(want, np.float32) if dtype == torch.float32 else round_bf16(want)
    assert np.array_equal(got.float().cpu().numpy(), want)


def test_the_graph_sits_on_the_edges():
    row, _, etype, plan = graph()
    tiles = lambda t: len(np.unique(row[etype == t] // BM))  # noqa: E731
    assert (tiles(0), tiles(1), tiles(2), tiles(4)) == (CS + 1, CS, 9, 0) and not (row // BM == EMPTY_TILE).any()
    assert ((row == HUB) & (etype == 3)).sum() > PASS and row.max() == M - 1
    assert plan.segments == len(np.unique(np.stack([row // BM, etype]), axis=1).T) and plan.nnz == len(row)
    assert plan.items == T + 1 and plan.partial_chunks == 2  # type 0 alone takes the fold


@pytest.mark.parametrize("valued", (False, True))
@pytest.mark.parametrize("trans_w", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,F", SHAPES)
def test_raw_forward(K, F, dtype, trans_w, valued):
    dt, plan = DTYPES[dtype], graph()[3]
    x, w, _, value, want, _, _ = case(K, F, valued, dtype == "bf16")
    scale = None if value is None else cuda(value)[plan.perm]
    out = blank(want.shape, dt)
    got = ops.typed_spmm(plan, cuda(x, dt), cuda(w.transpose(0, 2, 1) if trans_w else w, dt), scale, trans_w=trans_w,
                         out=out)
    assert got is out
    assert_exact(got, want, dt)


@pytest.mark.parametrize("valued", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,F", SHAPES)
def test_raw_weight_gradient(K, F, dtype, valued):
    dt, plan = DTYPES[dtype], graph()[3]
    x, _, g, value, _, _, want = case(K, F, valued, dtype == "bf16")
    scale = None if value is None else cuda(value)[plan.perm]
    out = blank(want.shape, dt)
    ops.typed_spmm_bw_weight(plan, cuda(x, dt), cuda(g, dt), scale, out=out)
    assert_exact(out, want, dt)


@pytest.mark.parametrize("valued", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,F", ((BK + 1, 65), (130, 64), (3, 130)))
def test_public_op_and_its_gradients(K, F, dtype, valued):
    dt, plan = DTYPES[dtype], graph()[3]
    x, w, g, value, want, want_x, want_w = case(K, F, valued, dtype == "bf16")
    xd, wd = cuda(x, dt).requires_grad_(), cuda(w, dt).requires_grad_()
    out = ps.typed_spmm(plan, xd, wd, cuda(value))
    out.backward(cuda(g, dt))
    assert_exact(out.detach(), want, dt)
    assert_exact(xd.grad, want_x, dt)
    assert_exact(wd.grad, want_w, dt)


def test_mean_is_the_sum_scaled_by_inv_count():
    row, col, etype, plan = graph()
    x, w, g, value, _, _, _ = case(BK + 1, 65, True)
    in_storage = np.empty(len(row), np.float32)
    in_storage[plan.perm.cpu().numpy()] = plan.inv_count.cpu().numpy()
    assert np.array_equal(in_storage.view(np.uint32), ref.inv_count(row, etype).view(np.uint32))
    for v in (None, value):
        results = []
        for kw in ({"value": cuda(v), "reduce": "mean"},
                   {"value": cuda(in_storage if v is None else v * in_storage)}):
            xd, wd = cuda(x).requires_grad_(), cuda(w).requires_grad_()
            out = ps.typed_spmm(plan, xd, wd, **kw)
            out.backward(cuda(g))
            results.append((out.detach(), xd.grad, wd.grad))
        assert all(torch.equal(a, b) for a, b in zip(*results))


def test_random_data_within_the_dot_product_bound_reproducible_and_capturable():
    """|got - ref| <= (n_i + K) 2^-23 sum |v| |x| |w|, n_i the entries of the row: the bound of an fp32 dot product
    of n_i K terms summed in two stages, doubled.  Two runs give equal bits; a captured graph with a prebuilt plan
    replays to the eager result on changed x."""
    row, col, etype, plan = graph()
    rng = np.random.default_rng(7)
    K, F = 130, 65
    x, w = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((T, K, F)).astype(np.float32)
    v = rng.standard_normal(len(row)).astype(np.float32)
    xd, wd, vd = cuda(x), cuda(w), cuda(v)
    got = ps.typed_spmm(plan, xd, wd, vd)
    n_i = np.bincount(row, minlength=M)[:, None]
    bound = (n_i + K) * 2.0 ** -23 * ref.forward(row, col, etype, np.abs(x), np.abs(w), np.abs(v), M)
    assert np.all(np.abs(got.cpu().numpy() - ref.forward(row, col, etype, x, w, v, M)) <= bound)
    assert torch.equal(got, ps.typed_spmm(plan, xd, wd, vd))
    assert torch.equal(ops.typed_spmm_bw_weight(plan, xd, got), ops.typed_spmm_bw_weight(plan, xd, got))
    out = torch.empty_like(got)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out.copy_(ps.typed_spmm(plan, xd, wd, vd, reduce="mean"))  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_):
        out.copy_(ps.typed_spmm(plan, xd, wd, vd, reduce="mean"))
    for shift in (1.0, -3.0, 2.0):
        xd.add_(shift)
        graph_.replay()
        assert torch.equal(out, ps.typed_spmm(plan, xd, wd, vd, reduce="mean"))


def test_a_value_that_requires_grad_is_refused():
    plan = graph()[3]
    x, w, _, value, _, _, _ = case(3, 3, True)
    with pytest.raises(NotImplementedError):
        ps.typed_spmm(plan, cuda(x), cuda(w), cuda(value).requires_grad_())
