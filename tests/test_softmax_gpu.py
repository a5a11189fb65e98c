"""GPU suite of the segmented softmax (csrc/softmax.hip) and SparseTensor.softmax.

Exact tests first: with one finite constant in L entries of a segment and -inf in the rest,
x - m is 0, exp is 1, the sum is the integer L and the result the correctly rounded 1 / L or
exactly 0, so segmentation, chunk combine, lane mapping and `perm` are held without any
tolerance; with L a power of two and integer upstream gradients the backward is exact too.
General values are held to bounds derived from the arithmetic (u = 2^-24):
    forward   |out - ref64|  <= (len + 64) u ref64
    backward  |grad - ref64| <= (len + 8) u y (|g| + sum |y g|)     (ref64 fed the same fp32 y)
The reference is tests/softmax_ref.py (float64 numpy)."""
import numpy as np
import pytest
import torch

import softmax_ref as sr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
INF = float("inf")
DEV = "cuda"

LAYOUTS = {
    # every length of the issue's set but the largest; an empty first and last segment
    "edges": [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1024, 4099, 0],
    # a long segment first, two long ones adjacent, a long one last; one above 65 535 entries
    "long": [70001, 3, 129, 4099, 0, 2, 1024],
    # short segments: the host picks narrower lane groups from n / nseg (8 or 16 lanes at D = 1 and 2, 32 at D = 4 for
    # "short"; 32 at D = 1 for "mid"), one segment above 128 entries among them
    "short": [0, 1, 2, 3, 5, 8, 13] * 6 + [129],
    "mid": [12, 20, 9, 17, 0, 11, 130, 16] * 3,
    "empty": [0, 0, 0],
    "none": [],
}
HEADS = [(1, "flat"), (1, "col"), (2, "col"), (3, "col"), (4, "col"), (8, "col"), (64, "col"), (65, "col")]


def layouts_for(D):
    return ["edges", "long", "short", "mid", "empty", "none"]


def indptr_of(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)


def shape_of(n, D, form):
    return (n,) if form == "flat" else (n, D)


def dev(a, dtype=None, misalign=False):
    """The array on the GPU; misalign: as a view one element into a larger allocation."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    if not misalign:
        return t.to(DEV)
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = base[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def exact_case(lens, D, form, rng, pow2):
    """(src fp32 in position order, expected fp32): per segment and head one constant in L entries
    (L a power of two when asked), -inf in the rest."""
    indptr = indptr_of(lens)
    n = int(indptr[-1])
    src = np.full((n, D), -INF, dtype=np.float32)
    want = np.zeros((n, D), dtype=np.float32)
    for s, ln in enumerate(lens):
        for h in range(D):
            if ln == 0:
                continue
            if pow2:
                L = 1 << int(rng.integers(0, min(int(np.log2(ln)), 16) + 1))
            else:
                L = int(rng.integers(1, ln + 1))
            live = indptr[s] + rng.choice(ln, size=L, replace=False)
            src[live, h] = np.float32(rng.integers(-50, 50)) / np.float32(4)
            want[live, h] = np.float32(1) / np.float32(L)
    return indptr, src.reshape(shape_of(n, D, form)), want.reshape(shape_of(n, D, form))


def to_rows(a, perm):
    """Position-ordered data -> row order: out[perm[j]] = a[j]."""
    if perm is None:
        return a
    out = np.empty_like(a)
    out[perm] = a
    return out


def variants(n, rng):
    """(perm | None, misalign) combinations every case runs in."""
    perm = rng.permutation(n).astype(np.int64)
    return [(None, False), (perm, False), (None, True), (perm, True)]


@pytest.mark.parametrize("D,form", HEADS)
def test_forward_exact(D, form):
    from paddle_sparse_amd import ops

    rng = np.random.default_rng(100 + D)
    for name in layouts_for(D):
        lens = LAYOUTS[name]
        indptr, src, want = exact_case(lens, D, form, rng, pow2=False)
        n = int(indptr[-1])
        for perm, mis in variants(n, rng):
            got = ops.segment_softmax(dev(to_rows(src, perm), misalign=mis and n > 0), dev(indptr),
                                      None if perm is None else dev(perm))
            assert got.shape == src.shape and got.dtype == torch.float32
            assert np.array_equal(got.cpu().numpy(), to_rows(want, perm)), (name, perm is not None, mis)


@pytest.mark.parametrize("D,form", HEADS)
def test_backward_exact(D, form):
    from paddle_sparse_amd import ops

    rng = np.random.default_rng(200 + D)
    for name in layouts_for(D):
        lens = LAYOUTS[name]
        indptr, src, y = exact_case(lens, D, form, rng, pow2=True)
        n = int(indptr[-1])
        g = rng.integers(-8, 9, size=y.shape).astype(np.float32)
        want = sr.softmax_bw_ref(y, g, indptr).astype(np.float32)
        assert np.array_equal(want.astype(np.float64), sr.softmax_bw_ref(y, g, indptr))  # exactly representable
        for perm, mis in variants(n, rng):
            p = None if perm is None else dev(perm)
            yd, gd = dev(to_rows(y, perm), misalign=mis and n > 0), dev(to_rows(g, perm), misalign=mis and n > 0)
            got = ops.segment_softmax_bw(yd, gd, dev(indptr), p)
            assert np.array_equal(got.cpu().numpy(), to_rows(want, perm)), (name, "raw", perm is not None, mis)
            x = dev(to_rows(src, perm), misalign=mis and n > 0).requires_grad_()
            out = ops.segment_softmax(x, dev(indptr), p)
            out.backward(gd)
            assert np.array_equal(out.detach().cpu().numpy(), to_rows(y, perm))
            assert np.array_equal(x.grad.cpu().numpy(), to_rows(want, perm)), (name, "autograd", perm is not None, mis)


@pytest.mark.parametrize("D,form", HEADS)
def test_general_values_within_the_derived_bounds(D, form):
    from paddle_sparse_amd import ops

    rng = np.random.default_rng(300 + D)
    for name in layouts_for(D)[:4]:
        lens = LAYOUTS[name]
        indptr = indptr_of(lens)
        n = int(indptr[-1])
        shape = shape_of(n, D, form)
        src = rng.uniform(-8, 8, size=shape).astype(np.float32)
        g = rng.normal(size=shape).astype(np.float32)
        for perm, mis in variants(n, rng)[1:3]:  # with perm aligned, without perm misaligned
            p = None if perm is None else dev(perm)
            xs, gs = to_rows(src, perm), to_rows(g, perm)
            got = ops.segment_softmax(dev(xs, misalign=mis), dev(indptr), p)
            y = got.cpu().numpy()
            ref = sr.softmax_ref(xs, indptr, perm)
            length = sr.segment_lengths(indptr, n, perm, shape[1:])
            err = np.abs(y.astype(np.float64) - ref)
            bound = (length + 64) * U * ref
            worst = float(np.max(err / np.maximum(bound, 1e-300)))
            print(f"forward D={D} {name} perm={perm is not None}: worst err / bound = {worst:.3f}")
            assert np.all(err <= bound)
            got_bw = ops.segment_softmax_bw(got, dev(gs, misalign=mis), dev(indptr), p).cpu().numpy()
            ref_bw = sr.softmax_bw_ref(y, gs, indptr, perm)  # the same fp32 y
            _, scale = sr.softmax_bw_bound_terms(y, gs, indptr, perm)
            err = np.abs(got_bw.astype(np.float64) - ref_bw)
            bound = (length + 8) * U * y.astype(np.float64) * scale
            worst = float(np.max(err / np.maximum(bound, 1e-300)))
            print(f"backward D={D} {name} perm={perm is not None}: worst err / bound = {worst:.3f}")
            assert np.all(err <= bound)


NONFINITE_SEGMENTS = {
    "nan": lambda v: v.__setitem__(1, np.nan),
    "plus_inf": lambda v: v.__setitem__(v.size // 2, INF),
    "all_minus_inf": lambda v: v.fill(-INF),
    "minus_inf_among_finite": lambda v: v.__setitem__(slice(0, None, 2), -INF),
    "nan_in_the_last_chunk": lambda v: v.__setitem__(v.size - 1, np.nan),
}


@pytest.mark.parametrize("D", [1, 3])
def test_nonfinite_rule(D):
    """Every case of the rule, per head, in a short segment (registers), one of 200 entries (chunks) and
    one of 1 entry; head 0 carries the case, the other heads stay finite.  NaN mask and finite entries
    against torch.softmax on the CPU dense row."""
    from paddle_sparse_amd import ops

    rng = np.random.default_rng(7)
    cases = sorted(NONFINITE_SEGMENTS)
    lens = []
    for _ in cases:
        lens += [5, 200, 2]
    indptr = indptr_of(lens)
    n = int(indptr[-1])
    src = rng.uniform(-8, 8, size=(n, D)).astype(np.float32)
    for i, case in enumerate(cases):
        for k in range(3):
            s = 3 * i + k
            NONFINITE_SEGMENTS[case](src[indptr[s]:indptr[s + 1], 0])
    got = ops.segment_softmax(dev(src), dev(indptr)).cpu().numpy()
    for s in range(len(lens)):
        sl = slice(indptr[s], indptr[s + 1])
        want = torch.softmax(torch.from_numpy(src[sl]), 0).numpy()
        assert np.array_equal(np.isnan(got[sl]), np.isnan(want)), cases[s // 3]
        ok = ~np.isnan(want)
        np.testing.assert_allclose(got[sl][ok], want[ok], rtol=(lens[s] + 64) * 2 * U, atol=0)
        assert np.array_equal(got[sl] == 0, want == 0)  # -inf among finite entries: exactly 0
    # backward: an entry with y = 0 gets gradient 0 when g is finite
    y = np.nan_to_num(got, nan=0.25)
    g = rng.normal(size=y.shape).astype(np.float32)
    grad = ops.segment_softmax_bw(dev(y), dev(g), dev(indptr)).cpu().numpy()
    assert (y == 0).any() and np.all(grad[y == 0] == 0)


def test_run_to_run_equality():
    from paddle_sparse_amd import ops

    rng = np.random.default_rng(11)
    indptr = dev(indptr_of(LAYOUTS["long"]))
    n = sum(LAYOUTS["long"])
    src = dev(rng.uniform(-8, 8, size=(n, 3)).astype(np.float32))
    g = dev(rng.normal(size=(n, 3)).astype(np.float32))
    perm = dev(rng.permutation(n).astype(np.int64))
    for p in (None, perm):
        a, b = ops.segment_softmax(src, indptr, p), ops.segment_softmax(src, indptr, p)
        assert torch.equal(a, b)
        ga, gb = ops.segment_softmax_bw(a, g, indptr, p), ops.segment_softmax_bw(a, g, indptr, p)
        assert torch.equal(ga, gb)


def test_wrapper_errors():
    from paddle_sparse_amd import ops

    ptr = torch.tensor([0, 3], device=DEV)
    with pytest.raises(TypeError):
        ops.segment_softmax(torch.zeros(3, dtype=torch.float64, device=DEV), ptr)
    with pytest.raises(TypeError):
        ops.segment_softmax(torch.zeros(3, dtype=torch.float16, device=DEV), ptr)
    with pytest.raises(TypeError):
        ops.segment_softmax(torch.zeros(3, device=DEV), ptr.int())
    with pytest.raises(RuntimeError):
        ops.segment_softmax(torch.zeros(3), ptr)
    with pytest.raises(ValueError):
        ops.segment_softmax(torch.zeros(3, device=DEV), ptr, torch.tensor([0, 1], device=DEV))
    with pytest.raises(ValueError):
        ops.segment_softmax_bw(torch.zeros(3, device=DEV), torch.zeros(4, device=DEV), ptr)
    with pytest.raises(TypeError):
        ops.segment_softmax_bw(torch.zeros(3, device=DEV), torch.zeros(3, dtype=torch.float64, device=DEV), ptr)


# ---- SparseTensor.softmax ---------------------------------------------------------------------------

def unsorted_matrix(rng, M, N, nnz, heads=None):
    """Distinct entries in random order, one hub row; (row, col, value) as numpy."""
    cells = rng.choice(M * N, size=nnz, replace=False)
    hub = np.arange(N, dtype=np.int64) + 3 * N  # row 3 is full: N > 128 entries
    cells = np.unique(np.concatenate([cells, hub]))
    rng.shuffle(cells)
    row, col = cells // N, cells % N
    shape = (cells.size,) if heads is None else (cells.size, heads)
    return row.astype(np.int64), col.astype(np.int64), rng.uniform(-8, 8, size=shape).astype(np.float32)


def sorted_view(row, col, value, M, N):
    order = np.lexsort((col, row))
    r, c, v = row[order], col[order], value[order]
    rowptr = np.searchsorted(r, np.arange(M + 1)).astype(np.int64)
    to_csc = np.argsort(c, kind="stable").astype(np.int64)
    colptr = np.searchsorted(c[to_csc], np.arange(N + 1)).astype(np.int64)
    return order, r, c, v, rowptr, to_csc, colptr


def within_forward_bound(got, ref, length):
    return np.all(np.abs(got.astype(np.float64) - ref) <= (length + 64) * U * ref)


@pytest.mark.parametrize("heads", [None, 4])
def test_sparse_tensor_softmax_rows_and_columns(heads):
    import paddle_sparse_amd as psa

    rng = np.random.default_rng(21)
    M, N = 150, 200
    row, col, value = unsorted_matrix(rng, M, N, 2500, heads)
    A = psa.SparseTensor(row=dev(row), col=dev(col), value=dev(value), sparse_sizes=(M, N))
    _, r, c, v, rowptr, to_csc, colptr = sorted_view(row, col, value, M, N)
    assert np.array_equal(A.storage.row().cpu().numpy(), r) and np.array_equal(A.storage.col().cpu().numpy(), c)
    tail = v.shape[1:]
    for dim, neg in ((1, -1), (0, -2)):
        B = A.softmax(dim)
        ref = sr.softmax_ref(v, rowptr) if dim == 1 else sr.softmax_ref(v, colptr, to_csc)
        length = sr.segment_lengths(rowptr, v.shape[0], None, tail) if dim == 1 else \
            sr.segment_lengths(colptr, v.shape[0], to_csc, tail)
        got = B.storage.value().cpu().numpy()
        assert got.shape == v.shape
        assert within_forward_bound(got, ref, length)
        assert torch.equal(B.storage.col(), A.storage.col()) and B.sparse_sizes() == A.sparse_sizes()
        assert torch.equal(psa.softmax(A, neg).storage.value(), B.storage.value())
    # dim = 0 is the row softmax of the transpose, bit for bit
    via_t = A.t().softmax(1).t()
    assert torch.equal(via_t.storage.col(), A.storage.col())
    assert torch.equal(via_t.storage.value(), A.softmax(0).storage.value())
    with pytest.raises(ValueError):
        A.softmax(2)


def test_sparse_tensor_softmax_without_values_is_one_over_the_degree():
    import paddle_sparse_amd as psa

    rng = np.random.default_rng(22)
    M, N = 150, 200
    row, col, _ = unsorted_matrix(rng, M, N, 2500)
    A = psa.SparseTensor(row=dev(row), col=dev(col), value=None, sparse_sizes=(M, N))
    r, c = A.storage.row().cpu().numpy(), A.storage.col().cpu().numpy()
    deg_r, deg_c = np.bincount(r, minlength=M), np.bincount(c, minlength=N)
    assert np.array_equal(A.softmax(1).storage.value().cpu().numpy(), np.float32(1) / deg_r[r].astype(np.float32))
    assert np.array_equal(A.softmax(0).storage.value().cpu().numpy(), np.float32(1) / deg_c[c].astype(np.float32))


def test_sparse_tensor_softmax_keeps_the_pattern_caches():
    import paddle_sparse_amd as psa

    rng = np.random.default_rng(23)
    row, col, value = unsorted_matrix(rng, 150, 200, 2500)
    A = psa.SparseTensor(row=dev(row), col=dev(col), value=dev(value), sparse_sizes=(150, 200))
    st = A.storage
    cached = {"rowptr": st.rowptr(), "csr2csc": st.csr2csc(), "colptr": st.colptr(), "rowcount": st.rowcount()}
    for dim in (1, 0):
        out = A.softmax(dim).storage
        for name, t in cached.items():
            kept = getattr(out, "_" + name)
            assert kept is not None, name
            assert kept is t or torch.equal(kept, t), name
        assert out.col() is st.col() or torch.equal(out.col(), st.col())


def test_sparse_tensor_softmax_tracked_values_get_the_reference_gradient():
    import paddle_sparse_amd as psa

    rng = np.random.default_rng(24)
    M, N = 150, 200
    row, col, value = unsorted_matrix(rng, M, N, 2500)
    coef = rng.normal(size=value.shape).astype(np.float32)  # per ORIGINAL entry, carried to the sorted order below
    order, r, c, v, rowptr, to_csc, colptr = sorted_view(row, col, value, M, N)
    for dim in (1, 0):
        val = dev(value).requires_grad_()
        A = psa.SparseTensor(row=dev(row), col=dev(col), value=val, sparse_sizes=(M, N))
        B = A.softmax(dim)
        y = B.storage.value()
        assert y.requires_grad
        (y * dev(coef[order])).sum().backward()
        ptr, perm = (rowptr, None) if dim == 1 else (colptr, to_csc)
        y32 = y.detach().cpu().numpy()
        ref_sorted = sr.softmax_bw_ref(y32, coef[order], ptr, perm)
        length = sr.segment_lengths(ptr, v.shape[0], perm)
        _, scale = sr.softmax_bw_bound_terms(y32, coef[order], ptr, perm)
        got_sorted = val.grad.cpu().numpy()[order]
        assert np.all(np.abs(got_sorted.astype(np.float64) - ref_sorted) <= (length + 8) * U * y32 * scale)


def test_forward_and_backward_replay_from_a_hip_graph():
    """One capture of forward + backward on a single stream (the matrix with the 1024-entry segment,
    so the long-segment launches and their scratch are in the graph), replayed on new data."""
    from paddle_sparse_amd import ops

    rng = np.random.default_rng(31)
    lens = LAYOUTS["edges"]
    indptr = dev(indptr_of(lens))
    n = sum(lens)
    src = dev(rng.uniform(-8, 8, size=(n, 2)).astype(np.float32))
    g = dev(rng.normal(size=(n, 2)).astype(np.float32))
    perm = dev(rng.permutation(n).astype(np.int64))

    def step():
        y = ops.segment_softmax(src, indptr, perm)
        return y, ops.segment_softmax_bw(y, g, indptr, perm)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_g, grad_g = step()
    for trial in range(2):
        src.copy_(dev(rng.uniform(-8, 8, size=(n, 2)).astype(np.float32)))
        g.copy_(dev(rng.normal(size=(n, 2)).astype(np.float32)))
        graph.replay()
        y_e, grad_e = step()
        assert torch.equal(y_g, y_e) and torch.equal(grad_g, grad_e), trial
