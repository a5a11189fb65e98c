"""GPU suite for basis_spmm (csrc/basis_spmm.hip, basis_spmm.py) against the float64 restatement of
tests/basis_spmm_ref.py, on ONE graph: M = N = (TC + 1) * BM + 1 rows (two chunks of the basis gradient, so the fold; the
last tile holds one row), T = 5.  Type 4 never occurs, tile 7 and most rows hold no entry, (row, col) pairs repeat with
other types, and row BM + 6 holds PASS + 26 entries of type 3 and five of type 0: more than one pass of the gather.  The
head of the same graph, its first TC tiles, is the one-chunk matrix that takes the direct route of the basis gradient.

Exact data: x and the cotangent integers in [-2, 2], values absent or out of {1, 2}, comp and basis out of
{-1, -0.5, 0.5, 1}, K and F at most 130, B at most 2 G + 1 = 9; at most 120 entries per row, 12 per column, 160 per
type and 500 in all.  So Z_b is a multiple of 0.5 with |Z_b| <= 120 * 2 * 1 * 2 = 480, and every partial sum
  of the forward is a multiple of 0.25 below 9 * 130 * 480 < 2^20,
  of grad_x one below 9 * 130 * (12 * 4) < 2^16,
  of grad_basis a multiple of 0.5 below (500 * 4) * 2 = 2^12 (a column of Z_b sums to at most 4 per entry),
  of P_b = grad @ basis[b]^T a multiple of 0.5 below 130 * 2 = 260, of s[e, b] one below 2 * K * 2 * F * 2 = 8 K F,
  and of grad_comp one below 160 * 8 K F, which is why the shapes of the comp gradient keep K * F <= 4300:
  160 * 8 * 4300 * 2 half units < 2^24.
All are exact in fp32 in any order; the bf16 roundings of Z_b and P_b keep multiples of 0.5 and grow a magnitude by
at most 2^-8, inside every margin above.  fp32 results equal the reference bit for bit, bf16 results the reference with
Z_b and P_b rounded to bf16, rounded once.  Outputs of the raw ops start as 0xAB bytes."""
import functools
import itertools

import numpy as np
import pytest
import torch

import basis_spmm_ref as ref
import paddle_sparse_amd as ps
from paddle_sparse_amd import ops
from segment_matmul_ref import round_bf16

pytestmark = pytest.mark.gpu

BM, G, KB, PASS, TC = ops.BASIS_SPMM_BM, ops.BASIS_SPMM_G, ops.BASIS_SPMM_KB, ops.BASIS_SPMM_PASS, ops.BASIS_SPMM_TC
M, T, EMPTY_TILE, HUB = (TC + 1) * BM + 1, 5, 7, BM + 6
BASES = (1, G, G + 1, 2 * G + 1)
SHAPES = ((1, 3), (3, 1), (32, KB), (33, KB + 1), (KB, 130), (KB + 1, 33), (130, 130))  # K slab, BK step, column tile
SMALL = ((3, 1), (33, KB + 1), (KB + 1, 64), (130, 33), (32, 130))  # K * F <= 4300 (module text)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
DYADIC = np.array([-1, -0.5, 0.5, 1], np.float32)


def cuda(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


@functools.lru_cache(maxsize=None)
def graph(head=False):
    """(row, col, etype, rows of the matrix) in storage order (by row, then column, stable) and the plan on the
    device; head: the entries of the first TC tiles, a matrix of TC * BM rows and M columns."""
    if head:
        row, col, etype, _, _ = graph()
        keep, rows = row < TC * BM, TC * BM
        row, col, etype = row[keep], col[keep], etype[keep]
    else:
        rng, rows = np.random.default_rng(3), M
        tiles = [t for t in range(TC + 2) if t != EMPTY_TILE]  # the last one is the one-row tile
        spot = lambda ts: [min(t * BM + int(rng.integers(BM)), M - 1) for t in ts]  # noqa: E731
        parts = [(spot(tiles), 0), ([HUB] * (PASS + 26), 3), ([HUB] * 5, 0), (spot(rng.choice(tiles[:40], 100)), 1),
                 (spot(rng.choice(tiles[:40], 100)), 2)]
        row = np.concatenate([np.asarray(r, np.int64) for r, _ in parts])
        etype = np.concatenate([np.full(len(r), t, np.int64) for r, t in parts])
        col = rng.integers(0, M, len(row))
        col[row == HUB] = rng.permutation(M)[:(row == HUB).sum()]
        extra = np.flatnonzero(etype == 1)[::3]  # the same (row, col) again under type 0: a multigraph
        row, col, etype = (np.concatenate([a, b]) for a, b in ((row, row[extra]), (col, col[extra]),
                                                              (etype, np.zeros(len(extra), np.int64))))
        order = np.lexsort((col, row))
        row, col, etype = row[order], col[order], etype[order]
        assert np.bincount(row).max() <= 120 and np.bincount(col).max() <= 12 and len(row) <= 500
        assert np.bincount(etype).max() <= 160
        assert len(np.unique(row // BM)) == TC + 1 and not (row // BM == EMPTY_TILE).any() and row.max() == M - 1
        assert ((row == HUB) & (etype == 3)).sum() > PASS and not (etype == 4).any() and len(np.unique(row)) < M // 10
    adj = ps.SparseTensor(row=cuda(row), col=cuda(col), sparse_sizes=(rows, M), is_sorted=True)
    return row, col, etype, rows, ps.BasisPlan(adj, cuda(etype), T)


@functools.lru_cache(maxsize=None)
def case(K, F, B, valued, bf16=False, head=False):
    """Operands, a cotangent and the float64 results of one shape; nothing here is written again."""
    row, col, etype, rows, _ = graph(head)
    rng = np.random.default_rng(1000 * K + 10 * F + B)
    x = rng.integers(-2, 3, (M, K)).astype(np.float32)
    V, comp = rng.choice(DYADIC, (B, K, F)), rng.choice(DYADIC, (T, B))
    g = rng.integers(-2, 3, (rows, F)).astype(np.float32)
    value = rng.integers(1, 3, len(row)).astype(np.float32) if valued else None
    out = ref.forward(row, col, etype, x, V, comp, value, rows, bf16)
    return (x, V, comp, g, value, out) + ref.backward(row, col, etype, x, V, comp, g, value, bf16)


def blank(shape, dtype):
    nbytes = tuple(shape[:-1]) + (shape[-1] * dtype.itemsize,)
    return torch.full(nbytes, 0xAB, dtype=torch.uint8, device="cuda").view(dtype)


def assert_exact(got, want, dtype):
    want = np.asarray(want, np.float32) if dtype == torch.float32 else round_bf16(want)
    assert np.array_equal(got.float().cpu().numpy(), want)


@pytest.mark.parametrize("valued", (False, True))
@pytest.mark.parametrize("trans", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", BASES)
@pytest.mark.parametrize("K,F", SHAPES)
def test_raw_forward(K, F, B, dtype, trans, valued):
    dt, plan = DTYPES[dtype], graph()[4]
    x, V, comp, _, value, want = case(K, F, B, valued, dtype == "bf16")[:6]
    out = blank(want.shape, dt)
    got = ops.basis_spmm(plan, cuda(x, dt), cuda(V.transpose(0, 2, 1) if trans else V, dt), cuda(comp), cuda(value),
                         trans=trans, out=out)
    assert got is out and plan.perm is None and plan.nnz == len(graph()[0])
    assert (plan.rowptr.dtype, plan.col.dtype, plan.etype.dtype) == (torch.int64, torch.int32, torch.int32)
    assert_exact(got, want, dt)


@pytest.mark.parametrize("head", (False, True))
@pytest.mark.parametrize("valued", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", BASES)
@pytest.mark.parametrize("K,F", ((3, 1), (33, KB + 1), (130, 130)))
def test_raw_basis_gradient(K, F, B, dtype, valued, head):
    dt, plan = DTYPES[dtype], graph(head)[4]
    x, _, comp, g, value, _, _, want = case(K, F, B, valued, dtype == "bf16", head)[:8]
    assert ops._lib.load().psa_basis_spmm_bw_chunks(plan.M) == (1 if head else 2)  # the direct route and the fold
    out = blank(want.shape, dt)
    ops.basis_spmm_bw_basis(plan, cuda(x, dt), cuda(g, dt), cuda(comp), cuda(value), out=out)
    assert_exact(out, want, dt)


@pytest.mark.parametrize("valued", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", BASES)
@pytest.mark.parametrize("K,F", SMALL)
def test_raw_comp_gradient(K, F, B, dtype, valued):
    dt, plan = DTYPES[dtype], graph()[4]
    x, V, _, g, value, _, _, _, _, want = case(K, F, B, valued, dtype == "bf16")
    out = blank(want.shape, torch.float32)
    ops.basis_spmm_bw_comp(plan, cuda(x, dt), cuda(g, dt), cuda(V, dt), cuda(value), out=out)
    assert_exact(out, want, torch.float32)


def run_public(plan, x, V, comp, g, dt, **kw):
    xd, Vd, cd = cuda(x, dt).requires_grad_(), cuda(V, dt).requires_grad_(), cuda(comp).requires_grad_()
    out = ps.basis_spmm(plan, xd, Vd, cd, **kw)
    out.backward(cuda(g, dt))
    return out.detach(), xd.grad, Vd.grad, cd.grad


@pytest.mark.parametrize("valued", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,F", ((33, KB + 1), (130, 33), (3, 130)))
def test_public_op_and_its_gradients(K, F, dtype, valued):
    dt, plan = DTYPES[dtype], graph()[4]
    x, V, comp, g, value, *want = case(K, F, G + 1, valued, dtype == "bf16")
    got = run_public(plan, x, V, comp, g, dt, value=cuda(value))
    for a, b, d in zip(got, want, (dt, dt, dt, torch.float32)):
        assert_exact(a, b, d)


def test_mean_is_the_sum_scaled_by_inv_count():
    row, _, etype, _, plan = graph()
    x, V, comp, g, value = case(33, KB + 1, G + 1, True)[:5]
    inv = plan.inv_count.cpu().numpy()
    assert np.array_equal(inv.view(np.uint32), ref.inv_count(row, etype).view(np.uint32))
    for v in (None, value):
        mean = run_public(plan, x, V, comp, g, torch.float32, value=cuda(v), reduce="mean")
        scaled = run_public(plan, x, V, comp, g, torch.float32, value=cuda(inv if v is None else v * inv))
        assert all(torch.equal(a, b) for a, b in zip(mean, scaled))


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_coefficients_give_typed_spmm(dtype):
    row, col, etype, _, plan = graph()
    dt = DTYPES[dtype]
    x, V, _, g, value = case(33, KB + 1, T, True)[:5]
    typed = ps.RelationalPlan(plan._adj, cuda(etype), T)
    xa, xb, Vd = cuda(x, dt).requires_grad_(), cuda(x, dt).requires_grad_(), cuda(V, dt)
    a = ps.basis_spmm(plan, xa, Vd, torch.eye(T, device="cuda"), cuda(value))
    b = ps.typed_spmm(typed, xb, Vd, cuda(value))
    a.backward(cuda(g, dt))
    b.backward(cuda(g, dt))
    assert torch.equal(a, b) and torch.equal(xa.grad, xb.grad)


def test_random_data_within_the_dot_product_bound_reproducible_and_capturable():
    """|got - ref| <= 2 (n_i + B K) 2^-23 sum |v| |comp| |x| |V|, n_i the entries of the row: Z_b is an fp32 sum of n_i
    products whose factor v * comp is itself rounded, out a dot product of B K terms over it; the first-order bound of
    both stages is (n_i + B K + 1) 2^-24 of the sum of the magnitudes, written with 2^-23 and doubled as for
    typed_spmm.  Two runs of every kernel give equal bits; a captured graph with a prebuilt plan replays to the eager
    result on changed x."""
    row, col, etype, _, plan = graph()
    rng = np.random.default_rng(7)
    K, F, B = 130, 65, G + 1
    x, V = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((B, K, F)).astype(np.float32)
    comp, v = rng.standard_normal((T, B)).astype(np.float32), rng.standard_normal(len(row)).astype(np.float32)
    xd, Vd, cd, vd = cuda(x), cuda(V), cuda(comp), cuda(v)
    got = ps.basis_spmm(plan, xd, Vd, cd, vd)
    n_i = np.bincount(row, minlength=M)[:, None]
    bound = 2 * (n_i + B * K) * 2.0 ** -23 * ref.forward(row, col, etype, np.abs(x), np.abs(V), np.abs(comp), np.abs(v), M)
    assert np.all(np.abs(got.cpu().numpy() - ref.forward(row, col, etype, x, V, comp, v, M)) <= bound)
    assert torch.equal(got, ps.basis_spmm(plan, xd, Vd, cd, vd))
    assert torch.equal(ops.basis_spmm(plan.t(), got, Vd, cd, trans=True), ops.basis_spmm(plan.t(), got, Vd, cd, trans=True))
    assert torch.equal(ops.basis_spmm_bw_basis(plan, xd, got, cd), ops.basis_spmm_bw_basis(plan, xd, got, cd))
    assert torch.equal(ops.basis_spmm_bw_comp(plan, xd, got, Vd), ops.basis_spmm_bw_comp(plan, xd, got, Vd))
    out = torch.empty_like(got)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out.copy_(ps.basis_spmm(plan, xd, Vd, cd, vd, reduce="mean"))  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_):
        out.copy_(ps.basis_spmm(plan, xd, Vd, cd, vd, reduce="mean"))
    for shift in (1.0, -3.0, 2.0):
        xd.add_(shift)
        graph_.replay()
        assert torch.equal(out, ps.basis_spmm(plan, xd, Vd, cd, vd, reduce="mean"))


def test_a_value_that_requires_grad_and_a_type_out_of_range_are_refused():
    row, col, etype, _, plan = graph()
    x, V, comp, _, value = case(3, 1, 1, True)[:5]
    with pytest.raises(NotImplementedError):
        ps.basis_spmm(plan, cuda(x), cuda(V), cuda(comp), cuda(value).requires_grad_())
    for bad in (-1, T):
        with pytest.raises(ops.IndexRangeError):
            ps.BasisPlan(plan._adj, cuda(np.where(np.arange(len(etype)) == 3, bad, etype)), T)
