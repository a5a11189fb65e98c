"""GPU suite for edge_spmm (csrc/edge_spmm.hip, edge_spmm.py) against a float64 CPU reference: m = op(x[col], edge),
an index_add_ over row, the division for mean, and torch autograd through that expression for both gradients.

Exact data are integers of magnitude <= 4: every message, every product with grad_out and every sum stays an integer
below 2^24 (mean patterns have power-of-two row lengths, so 1 / n and the division are exact too), hence fp32 results
equal the reference bit for bit in any summation order and bf16 results equal the reference rounded once.  The sums
of the long rows exceed 2^8, which an accumulator of bf16 precision cannot hold."""
import functools

import pytest
import torch

import paddle_sparse_amd as ps
from paddle_sparse_amd import SparseTensor, ops

pytestmark = pytest.mark.gpu

OPS = ("mul", "add", "add_relu")
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
# the element form (1, 3), one vector, a width that is no power of two, one vector past a tile of the 16-byte form
WIDTHS = {"fp32": (1, 3, 4, 68, ops.EDGE_SPMM_TILE[torch.float32] + 4),
          "bf16": (1, 3, 8, 72, ops.EDGE_SPMM_TILE[torch.bfloat16] + 8)}
CASES = [(d, k, False) for d in DTYPES for k in WIDTHS[d]] + [(d, WIDTHS[d][3], True) for d in DTYPES]
# rows: empty, one entry, either side of the 64-entry batch and of LONG_ROW, three chunks with a ragged last one
SUM_ROWS = (0, 1, 63, 64, 65, ops.LONG_ROW, ops.LONG_ROW + 1, 300, 0)
MEAN_ROWS = (0, 1, 2, 64, 128, 256, 0)
U24 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def pattern(lengths, N=12, width=None):
    """(M, N, row, col): row r holds lengths[r] entries over columns 0 .. width - 1 in turn (duplicate pairs, columns
    of more than LONG_ROW entries: the long-column plan of grad_x), the one-entry row sits in column 7, the other
    columns are empty."""
    width = width or sum(lengths) // 140  # about 150 entries per column: two chunks, the second one ragged
    row = torch.cat([torch.full((n,), r, dtype=torch.int64) for r, n in enumerate(lengths)])
    col = torch.cat([torch.sort(torch.arange(n) % width).values if n != 1 else torch.tensor([7]) for n in lengths])
    assert torch.bincount(col, minlength=N).max() > ops.LONG_ROW and N != len(lengths)
    return len(lengths), N, row, col


@functools.lru_cache(maxsize=None)
def data(lengths, K, exact, seed=0):
    """x, edge, grad_out (float32, CPU) for a pattern: small integers, x + edge on both sides of 0, or normals."""
    M, N, row, col = pattern(lengths)
    gen = torch.Generator().manual_seed(seed + K)
    if exact:
        draw = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).float()
        return draw(-1, 4, N, K), draw(-2, 4, len(col), K), draw(-4, 4, M, K)
    return tuple(torch.randn(*shape, generator=gen) for shape in ((N, K), (len(col), K), (M, K)))


def reference(row, col, M, x, edge, g, op, mean):
    """(out, grad_x, grad_edge, sum of |m| per output element), float64."""
    x, edge = x.double().requires_grad_(), edge.double().requires_grad_()
    m = {"mul": x[col] * edge, "add": x[col] + edge, "add_relu": torch.relu(x[col] + edge)}[op]
    out = torch.zeros(M, x.shape[1], dtype=torch.float64).index_add(0, row, m)
    mag = torch.zeros(M, x.shape[1], dtype=torch.float64).index_add(0, row, m.detach().abs())
    if mean:
        n = torch.bincount(row, minlength=M).clamp(min=1)[:, None]
        out, mag = out / n, mag / n
    out.backward(g.double())
    return out.detach(), x.grad, edge.grad, mag


@functools.lru_cache(maxsize=None)
def exact_reference(lengths, K, op, mean):
    M, N, row, col = pattern(lengths)
    return reference(row, col, M, *data(lengths, K, True), op, mean)


def run(lengths, x, edge, g, dtype, op, reduce, unaligned=False, stored=False):
    """(out, grad_x, grad_edge) of the op on the GPU, on the CPU in float64 for comparison."""
    M, N, row, col = pattern(lengths)
    xd = x.to(dtype).cuda()
    if unaligned:  # a storage offset of one element: no 16-byte access can be used
        flat = torch.empty(xd.numel() + 1, dtype=dtype, device="cuda")
        flat[1:].copy_(xd.reshape(-1))
        xd = flat[1:].view(xd.shape)
        assert xd.data_ptr() % 16 != 0
    xd, ed = xd.detach().requires_grad_(), edge.to(dtype).cuda().requires_grad_()
    adj = SparseTensor(row=row.cuda(), col=col.cuda(), sparse_sizes=(M, N), is_sorted=True, trust_data=True)
    out = adj.set_value(ed, layout="coo").edge_spmm(xd, op=op, reduce=reduce) if stored else ps.edge_spmm(adj, xd, ed, op, reduce)
    assert out.dtype == dtype and out.shape == (M, x.shape[1])
    out.backward(g.to(dtype).cuda())
    return tuple(t.detach().cpu().double() for t in (out, xd.grad, ed.grad))


def assert_exact(got, want, dtype):
    for name, a, b in zip(("out", "grad_x", "grad_edge"), got, want):
        assert torch.equal(a, b.to(dtype).double()), name


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dtype,K,unaligned", CASES, ids=lambda v: str(v))
def test_exact_sum(dtype, K, unaligned, op):
    want = exact_reference(SUM_ROWS, K, op, False)
    assert want[0][7].abs().max() > 2 ** 8 and (op != "add_relu" or (want[2] == 0).any())  # the data do what they are for
    assert_exact(run(SUM_ROWS, *data(SUM_ROWS, K, True), DTYPES[dtype], op, "sum", unaligned), want, DTYPES[dtype])


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dtype,K,unaligned", CASES, ids=lambda v: str(v))
def test_exact_mean(dtype, K, unaligned, op):
    want = exact_reference(MEAN_ROWS, K, op, True)
    got = run(MEAN_ROWS, *data(MEAN_ROWS, K, True), DTYPES[dtype], op, "mean", unaligned, stored=True)
    assert_exact(got, want, DTYPES[dtype])


def test_second_trip_of_every_capped_grid():
    """More listed rows and listed columns than the combine grids have waves (so more chunks than the chunk grids
    have), more entries than the grad_edge grid has lanes: the grid-stride loops of the chunk, combine and grad_edge
    kernels all take a second trip, in the forward and in grad_x.  A band matrix: row r holds 129, 130 or 131
    entries (two chunks, the second nearly empty) from column r on, so all but the first and last columns hold 129 to
    131 entries too; one short and one empty row behind them.  Sums stay below 16 * 131."""
    cap = ops.EDGE_SPMM_CHUNK_WAVES
    lengths = torch.tensor([ops.LONG_ROW + 1 + r % 3 for r in range(cap + cap // 25)] + [5, 0])
    M, N = len(lengths), len(lengths) + 100
    row = torch.repeat_interleave(torch.arange(M), lengths)
    col = (row + torch.arange(len(row)) - torch.repeat_interleave(lengths.cumsum(0) - lengths, lengths)) % N
    col = (row * N + col).sort().values % N
    nnz = len(col)
    assert (lengths > ops.LONG_ROW).sum() > cap and (torch.bincount(col, minlength=N) > ops.LONG_ROW).sum() > cap
    assert nnz > ops.EDGE_SPMM_ENTRY_LANES and N != M
    gen = torch.Generator().manual_seed(1)
    x, edge, g = (torch.randint(-4, 5, s, generator=gen).float() for s in ((N, 4), (nnz, 4), (M, 4)))
    want = reference(row, col, M, x, edge, g, "mul", False)
    xd, ed = x.cuda().requires_grad_(), edge.cuda().requires_grad_()
    adj = SparseTensor(row=row.cuda(), col=col.cuda(), sparse_sizes=(M, N), is_sorted=True, trust_data=True)
    out = adj.edge_spmm(xd, ed)
    out.backward(g.cuda())
    assert_exact([t.detach().cpu().double() for t in (out, xd.grad, ed.grad)], want, torch.float32)


@pytest.mark.parametrize("reduce", ("sum", "mean"))
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_general_values_within_the_derived_bound(dtype, op, reduce):
    """|out - ref| <= u |ref| + (n + 2) 2^-24 sum |m|: n fp32 additions, one product or addition and one division,
    each within 2^-24 relative of a quantity that sum |m| bounds, and for bf16 the one final rounding (u = 2^-8; 0 for
    fp32).  The reference takes the inputs as the kernel sees them: rounded to bf16 first."""
    K = WIDTHS[dtype][3]
    M, N, row, col = pattern(SUM_ROWS)
    x, edge, g = (t.to(DTYPES[dtype]).float() for t in data(SUM_ROWS, K, False))
    ref, _, _, mag = reference(row, col, M, x, edge, g, op, reduce == "mean")
    out = run(SUM_ROWS, x, edge, g, DTYPES[dtype], op, reduce)[0]
    n = torch.tensor(SUM_ROWS, dtype=torch.float64)[:, None]
    u = 0.0 if dtype == "fp32" else 2.0 ** -8
    assert torch.all((out - ref).abs() <= u * ref.abs() + (n + 2) * U24 * mag)


def test_non_finite_values_stay_where_they_are():
    M, N, row, col = pattern(SUM_ROWS)
    x, edge, g = (t.clone() for t in data(SUM_ROWS, 4, True))
    e0 = int((row == 4).nonzero()[3])  # 0 * inf in one entry of row 4
    edge[col == col[e0], 0] = 1.0  # the other entries that meet this x stay finite
    x[col[e0], 0], edge[e0, 0] = 0.0, float("inf")
    ref = reference(row, col, M, x, edge, g, "mul", False)[0]
    out = run(SUM_ROWS, x, edge, g, torch.float32, "mul", "sum")[0]
    nan = torch.zeros(M, 4, dtype=torch.bool)
    nan[4, 0] = True
    assert torch.equal(out.isnan(), nan) and torch.equal(ref.isnan(), nan) and torch.equal(out[~nan], ref[~nan])
    x, edge, g = (t.clone() for t in data(SUM_ROWS, 4, True))
    x[7, 1] = float("nan")  # column 7 holds the one-entry row only: relu(NaN) is NaN there
    ref = reference(row, col, M, x, edge, g, "add_relu", False)[0]
    out = run(SUM_ROWS, x, edge, g, torch.float32, "add_relu", "sum")[0]
    nan[:] = False
    nan[1, 1] = True
    assert torch.equal(out.isnan(), nan) and torch.equal(ref.isnan(), nan) and torch.equal(out[~nan], ref[~nan])
    assert not out[0].any() and not out[8].any()  # rows without entries


def test_same_bits_twice_and_in_a_captured_graph():
    M, N, row, col = pattern(SUM_ROWS)
    x, edge, g = data(SUM_ROWS, 68, False)
    first = run(SUM_ROWS, x, edge, g, torch.float32, "mul", "mean")
    assert all(torch.equal(a, b) for a, b in zip(first, run(SUM_ROWS, x, edge, g, torch.float32, "mul", "mean")))
    xd, ed, gd = x.cuda().requires_grad_(), edge.cuda().requires_grad_(), g.cuda()
    adj = SparseTensor(row=row.cuda(), col=col.cuda(), sparse_sizes=(M, N), is_sorted=True, trust_data=True)

    def step():
        return (out := adj.edge_spmm(xd, ed, "mul", "mean"),) + torch.autograd.grad(out, (xd, ed), gd)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up outside the capture: the storage builds its CSC view here
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    for _ in range(3):
        for t in held:
            t.detach().fill_(7.0)
        graph.replay()
        assert all(torch.equal(h.detach().cpu().double(), f) for h, f in zip(held, first))
