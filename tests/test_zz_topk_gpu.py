"""GPU suite for segment_topk and SparseTensor.topk (csrc/topk.hip).  A selection has no rounding:
every comparison is bit-exact against the numpy restatement of tests/topk_ref.py (held to torch.topk
and to the kernels' steps run on the host by test_zz_topk_ref.py), on the case list of that file:
the short regime at every group width the launch can choose with every length 0 .. TOPK_SHORT + 1,
the LDS and stream regimes at the lengths either side of a chunk, of TOPK_LDS and beyond, every k
either side of a length and of a chunk, both directions, all six dtypes, per-segment k with zeros,
negatives and values above the length, structured keys (all equal, one differing byte at every
byte of the key, two values, quota 1 and count - 1, NaN of both signs, infinities, signed zeros,
denormals, the integer limits, the half types' extremes), pointers that leave a head and a tail
uncovered or lie outside the arrays, and a random perm.  Every output starts as 0xAB bytes, so a
position that must not be written shows, and one that must be shows too.

Grids: the short kernel's grid covers the segments and is not capped.  The long kernel's is capped
at TOPK_GRID workgroups, each taking TOPK_CHUNK segments per trip: the second-trip test gives it
3 * TOPK_GRID // 2 chunks, with one long segment of TOPK_SHORT + 1 entries in each.

The file name sorts behind every other GPU file on purpose: the new tests are collected last."""
import numpy as np
import pytest
import torch

import topk_ref as tr
from paddle_sparse_amd import ops

pytestmark = pytest.mark.gpu

SHORT, LDS, GRID, CHUNK = ops.TOPK_SHORT, ops.TOPK_LDS, ops.TOPK_GRID, ops.TOPK_CHUNK
CASES = tr.all_cases(SHORT, LDS)
SENTINEL = 0xAB


def gpu_value(value, bf16):
    if bf16:
        return torch.from_numpy(value.view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(value).cuda()


def gpu_k(k):
    return k if isinstance(k, int) else torch.from_numpy(k).cuda()


def run_case(c):
    n = c["value"].size
    want = tr.topk_ref(c["value"], c["indptr"], c["k"], c["perm"], c["largest"], np.full(n, SENTINEL, np.uint8), c["bf16"])
    out = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
    perm = None if c["perm"] is None else torch.from_numpy(c["perm"]).cuda()
    got = ops.segment_topk(gpu_value(c["value"], c["bf16"]), torch.from_numpy(c["indptr"]).cuda(), gpu_k(c["k"]), perm,
                           c["largest"], out=out)
    assert got is out
    return got.cpu().numpy(), want


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_list_bit_exact(name):
    c = CASES[name]
    got, want = run_case(c)
    covered = np.zeros(got.size, bool)
    ptr = c["indptr"]
    for b, e in zip(ptr[:-1], ptr[1:]):
        if 0 <= b <= e <= got.size:
            covered[(np.arange(b, e) if c["perm"] is None else c["perm"][b:e])] = True
    assert np.isin(got[covered], (0, 1)).all() and (got[~covered] == SENTINEL).all()
    assert np.array_equal(got, want)


def test_all_equal_keeps_exactly_the_first_k_positions():
    c = CASES["all-equal-float32-max"]
    got, _ = run_case(c)
    for b, e in zip(c["indptr"][:-1], c["indptr"][1:]):
        assert got[b:b + 7].all() and not got[b + 7:e].any()


def test_the_head_and_the_tail_keep_their_sentinel():
    c = CASES["head-tail-max"]
    got, _ = run_case(c)
    lo, hi = c["indptr"][0], c["indptr"][-1]
    assert lo > 0 and hi < got.size and (got[:lo] == SENTINEL).all() and (got[hi:] == SENTINEL).all()
    assert np.isin(got[lo:hi], (0, 1)).all()


def test_default_output_is_zero_filled_and_repeats():
    c = CASES["head-tail-perm-min"]
    args = (gpu_value(c["value"], c["bf16"]), torch.from_numpy(c["indptr"]).cuda(), c["k"], torch.from_numpy(c["perm"]).cuda(),
            c["largest"])
    a, b = ops.segment_topk(*args), ops.segment_topk(*args)
    assert a.dtype == torch.uint8 and torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), tr.topk_ref(c["value"], c["indptr"], c["k"], c["perm"], c["largest"]))


def test_second_trip_of_the_long_kernel():
    """More chunks of segments than the long kernel has workgroups: every workgroup of the first half
    of the grid takes a second chunk.  One segment of TOPK_SHORT + 1 entries per chunk, the others
    empty; the output starts poisoned."""
    chunks = 3 * GRID // 2
    lengths = np.zeros(chunks * CHUNK, np.int64)
    lengths[np.arange(chunks) * CHUNK + (np.arange(chunks) * 37) % CHUNK] = SHORT + 1
    indptr = tr.ptr_of(lengths)
    nseg, n = lengths.size, int(indptr[-1])
    assert -(-nseg // CHUNK) > GRID and n == chunks * (SHORT + 1)  # the count exceeds the grid
    value, _ = tr.tied(np.random.default_rng(23), n, "float32")
    for k in (3, SHORT):
        want = tr.topk_ref(value, indptr, k, out=np.full(n, SENTINEL, np.uint8))
        out = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
        ops.segment_topk(torch.from_numpy(value).cuda(), torch.from_numpy(indptr).cuda(), k, out=out)
        got = out.cpu().numpy()
        assert np.isin(got, (0, 1)).all() and np.array_equal(got, want)
        assert got.reshape(chunks, SHORT + 1).sum(1).tolist() == [k] * chunks


# ---- through the surface -----------------------------------------------------------------------------
def random_adj(seed, M=70, N=90, nnz=2500, value="float32", heads=None):
    import paddle_sparse_amd as psa

    rng = np.random.default_rng(seed)
    key = np.unique(rng.integers(0, M * N, nnz))
    row, col = key // N, key % N
    if value is None:
        val = None
    elif heads:
        val = torch.from_numpy(rng.standard_normal((key.size, heads)).astype(value)).cuda()
    else:
        val = torch.from_numpy(rng.integers(-4, 5, key.size).astype(value)).cuda()
    adj = psa.SparseTensor(row=torch.from_numpy(row).cuda(), col=torch.from_numpy(col).cuda(), value=val,
                           sparse_sizes=(M, N), is_sorted=True)
    return adj, row, col


def ref_rows(score, row, col, M, N, k, dim, largest=True):
    """The kept storage positions by the restatement: per row in storage order, per column through the
    stable column order."""
    if dim == 1:
        ptr = np.searchsorted(row, np.arange(M + 1)).astype(np.int64)
        keep = tr.topk_ref(score, ptr, k, None, largest)
    else:
        perm = np.argsort(col, kind="stable").astype(np.int64)
        ptr = np.searchsorted(col[perm], np.arange(N + 1)).astype(np.int64)
        keep = tr.topk_ref(score, ptr, k, perm, largest)
    return np.flatnonzero(keep)


def check_storage(out, row, col, e_ref):
    """A valid sorted storage holding exactly the entries e_ref, whose handed-over and derived caches agree
    with those of a storage built fresh from its coo()."""
    import paddle_sparse_amd as psa

    r, c, v = out.coo()
    assert np.array_equal(r.cpu().numpy(), row[e_ref]) and np.array_equal(c.cpu().numpy(), col[e_ref])
    fresh = psa.SparseTensor(row=r.clone(), col=c.clone(), value=v, sparse_sizes=out.sparse_sizes(), is_sorted=False)
    for name in ("rowptr", "rowcount", "colptr", "colcount", "csr2csc", "csc2csr"):
        assert torch.equal(getattr(out.storage, name)(), getattr(fresh.storage, name)()), name
    assert torch.equal(fresh.storage.row(), r) and torch.equal(fresh.storage.col(), c)


@pytest.mark.parametrize("largest", (True, False))
@pytest.mark.parametrize("k", (0, 1, 3, 200, "tensor"))
def test_topk_rows_and_columns_against_the_reference_and_the_transpose(k, largest):
    import paddle_sparse_amd as psa

    adj, row, col = random_adj(31)
    M, N = adj.sparse_sizes()
    score = adj.storage.value().cpu().numpy()
    rng = np.random.default_rng(5)
    for dim in (1, 0, -1, -2):
        kk = rng.integers(-1, 6, M if dim in (1, -1) else N).astype(np.int64) if k == "tensor" else k
        e_ref = ref_rows(score, row, col, M, N, kk, dim % 2, largest)
        kg = gpu_k(kk)
        out, e_id = adj.topk(kg, dim=dim, largest=largest, return_e_id=True)
        assert e_id.dtype == torch.int64 and np.array_equal(e_id.cpu().numpy(), e_ref)
        assert torch.equal(out.storage.value(), adj.storage.value()[e_id])
        check_storage(out, row, col, e_ref)
        assert torch.equal(psa.topk(adj, kg, dim, largest).storage.col(), out.storage.col())
    # per column = per row of the transpose, entry for entry
    kk = rng.integers(-1, 6, N).astype(np.int64) if k == "tensor" else k
    a = adj.topk(gpu_k(kk), dim=0, largest=largest)
    b = adj.t().topk(gpu_k(kk), dim=1, largest=largest).t()
    for x, y in zip(a.coo(), b.coo()):
        assert torch.equal(x, y)


def test_by_selects_and_keeps_multi_head_values():
    adj, row, col = random_adj(37, value="float32", heads=3)
    M, N = adj.sparse_sizes()
    with pytest.raises(ValueError, match="by"):
        adj.topk(2)
    rng = np.random.default_rng(3)
    score = rng.integers(-3, 4, row.size).astype(np.float64)
    score[::17] = np.nan
    for dim in (1, 0):
        out, e_id = adj.topk(2, dim=dim, by=torch.from_numpy(score).cuda(), return_e_id=True)
        e_ref = ref_rows(score, row, col, M, N, 2, dim)
        assert np.array_equal(e_id.cpu().numpy(), e_ref)
        assert tuple(out.storage.value().shape) == (e_ref.size, 3)
        assert torch.equal(out.storage.value(), adj.storage.value()[e_id])
        check_storage(out, row, col, e_ref)
    with pytest.raises(ValueError):
        adj.topk(2, by=torch.zeros(row.size + 1, device="cuda"))


def test_without_values_the_first_k_entries_are_kept():
    adj, row, col = random_adj(41, value=None)
    M, N = adj.sparse_sizes()
    zeros = np.zeros(row.size, np.float32)
    for dim in (1, 0):
        out, e_id = adj.topk(3, dim=dim, return_e_id=True)
        e_ref = ref_rows(zeros, row, col, M, N, 3, dim)
        assert out.storage.value() is None and np.array_equal(e_id.cpu().numpy(), e_ref)
        check_storage(out, row, col, e_ref)
    first = np.concatenate([np.flatnonzero(row == r)[:3] for r in range(M)])
    assert np.array_equal(adj.topk(3, return_e_id=True)[1].cpu().numpy(), first)


def test_public_segment_topk_returns_the_kept_positions():
    import paddle_sparse_amd as psa

    rng = np.random.default_rng(43)
    sizes = np.array([0, 5, 70, 1, 300, 12], np.int64)
    ptr = tr.ptr_of(sizes)
    score, _ = tr.tied(rng, int(ptr[-1]), "float32")
    k = np.ceil(0.5 * sizes).astype(np.int64)
    for kk in (k, 4):
        got = psa.segment_topk(torch.from_numpy(score).cuda(), torch.from_numpy(ptr).cuda(), gpu_k(kk))
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), np.flatnonzero(tr.topk_ref(score, ptr, kk)))


def test_autograd_passes_through_the_kept_values_only():
    import paddle_sparse_amd as psa

    adj, row, col = random_adj(47)
    M, N = adj.sparse_sizes()
    for dim in (1, 0):
        w = adj.storage.value().clone().requires_grad_(True)
        out, e_id = adj.set_value(w, layout="coo").topk(3, dim=dim, return_e_id=True)
        assert out.storage.value().requires_grad
        out.storage.value().sum().backward()
        mask = torch.zeros_like(w)
        mask[e_id] = 1.0
        assert torch.equal(w.grad, mask)
        assert np.array_equal(np.flatnonzero(mask.cpu().numpy()), ref_rows(w.detach().cpu().numpy(), row, col, M, N, 3, dim))
    w = adj.storage.value().clone().requires_grad_(True)
    by = torch.randn(row.size, device="cuda", requires_grad=True)
    psa.topk(adj.set_value(w, layout="coo"), 2, by=by).storage.value().sum().backward()
    assert by.grad is None and w.grad is not None and int(w.grad.sum()) == int((w.grad != 0).sum())


def test_segment_topk_replays_from_a_hip_graph():
    """ops.segment_topk reads nothing back and allocates nothing it is not handed: captured on one stream,
    it replays to the same bits on new data written into the same buffers."""
    rng = np.random.default_rng(53)
    lengths = tr.mixed_lengths(SHORT, LDS)
    indptr = torch.from_numpy(tr.ptr_of(lengths)).cuda()
    n = sum(lengths)
    value = torch.zeros(n, device="cuda")
    perm = torch.from_numpy(rng.permutation(n).astype(np.int64)).cuda()
    out = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.segment_topk(value, indptr, 9, perm, out=out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.segment_topk(value, indptr, 9, perm, out=out)
    for trial in range(3):
        new, _ = tr.tied(rng, n, "float32")
        value.copy_(torch.from_numpy(new).cuda())
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        want = tr.topk_ref(new, indptr.cpu().numpy(), 9, perm.cpu().numpy())
        assert np.array_equal(out.cpu().numpy(), want)
        assert torch.equal(out, ops.segment_topk(value, indptr, 9, perm))
