"""GPU: the grouped reductions against the exact reference (tests/reduce_ref.py), bit for bit, on every
route: segment_csr (thread-per-element and wave-per-segment kernels and the switch between them),
scatter, unique_sorted_reduce, coalesce (one launch, two-call chain, above the chain),
SparseTensor.sum / mean / min / max over dim 1 and dim 0, and the compress step of spspmm.

Every comparison is equality of values and indices with NaNs matched by position (reduce_ref.same):
the data are small integers under the bound that `assert_exact` checks, so any summation order gives
the same bits, plus +inf / -inf / NaN (`specials`) and the integer type limits (`extremes`).  The rule
under test: min / max give NaN for a group that holds one in that column, wherever it sits; sum /
mean are IEEE; an empty group gives 0.

Each test names its route and proves it: `spy` records the C entry points a call went through (and
the arguments that select a kernel inside one), or the test calls the entry point itself."""
import math
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from reduce_ref import (HALF_TYPES, REDUCES, SHAPES, assert_exact, coalesce_ref, group_lengths, group_reduce,
                        make_case, same, scatter_ref, segment_ref, shuffled, spspmm_ref, spspmm_terms)

pytestmark = pytest.mark.gpu

F32, F64, I32, I64, F16, BF16 = (torch.float32, torch.float64, torch.int32, torch.int64, torch.float16,
                                 torch.bfloat16)
ALL = [F32, F64, I32, I64, F16, BF16]
WORD = [F32, F64, I32, I64]


def _modes(dtypes, extremes=True):
    """(dtype, mode) pairs: int everywhere, specials for floating types, extremes for integers."""
    out = []
    for dt in dtypes:
        out.append(pytest.param(dt, "int", id=f"{str(dt)[6:]}-int"))
        if dt.is_floating_point:
            out.append(pytest.param(dt, "specials", id=f"{str(dt)[6:]}-specials"))
        elif extremes:
            out.append(pytest.param(dt, "extremes", id=f"{str(dt)[6:]}-extremes"))
    return out


def _reduces(mode):
    return ("min", "max") if mode == "extremes" else REDUCES  # sums of type limits overflow


def _lengths(shape):
    return group_lengths(shape, total=60_000 if shape == "powerlaw" else None, seed=3)


@contextmanager
def spy(*names):
    """Records (name, args) of the calls to the named C entry points for as long as it is open."""
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    calls, saved = [], {}
    for name in names:
        fn = saved[name] = getattr(lib, name)

        def wrapped(*args, _fn=fn, _name=name):
            calls.append((_name, args))
            return _fn(*args)

        setattr(lib, name, wrapped)
    try:
        yield calls
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)


def _names(calls):
    return [c[0] for c in calls]


def _segment_kernels(calls):
    """'wave' / 'thread' for every psa_segment_reduce call: launch_segment takes the wave-per-segment
    kernel when D == 1 and n_hint >= 32 * nseg (args: reduce, dtype, src, perm, ptr, nseg, D, n_hint, ...)."""
    return ["wave" if a[6] == 1 and a[7] >= 32 * a[5] else "thread" for name, a in calls if name == "psa_segment_reduce"]


def _segment_direct(src, indptr, reduce, perm, n_hint):
    """psa_segment_reduce with the caller's n_hint: the hint alone picks the kernel."""
    from paddle_sparse_amd import _lib, ops

    nseg = indptr.numel() - 1
    out = torch.empty((nseg,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    D = math.prod(src.shape[1:])
    _lib.check(_lib.load().psa_segment_reduce(_lib.REDUCE_ID[reduce], ops._DTYPE_ID[src.dtype], src.data_ptr(),
                                              None if perm is None else perm.data_ptr(), indptr.data_ptr(), nseg, D,
                                              int(n_hint), out.data_ptr(), ops._stream()))
    return out


def _coo_of(group, n):
    """Group g at the matrix position (g // n * 2, g % n): distinct groups, distinct positions."""
    return torch.stack([group // n * 2, group % n])


# ---------------------------------------------------------------------------------------------
# ops.segment_csr
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,mode", _modes(ALL))
@pytest.mark.parametrize("shape", SHAPES)
def test_segment_reduce_thread_and_wave_kernels(shape, dtype, mode):
    """Both kernels on the same scalar data, with and without perm, by the hint that selects them."""
    case = make_case(_lengths(shape), mode, dtype, seed=1)
    case.check(_reduces(mode))
    n, nseg = case.values.shape[0], case.ngroups
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(2))
    src, indptr, perm_d = case.values.cuda(), case.indptr.cuda(), perm.cuda()
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n)
    src_for_perm = case.values[inv].cuda()  # src_for_perm[perm] is the case's own order
    for reduce in _reduces(mode):
        ref = segment_ref(case.values, case.indptr, reduce)
        for route, hint in (("thread", 0), ("wave", 32 * nseg)):
            with spy("psa_segment_reduce") as calls:
                got = _segment_direct(src, indptr, reduce, None, hint)
                got_p = _segment_direct(src_for_perm, indptr, reduce, perm_d, hint)
            assert _segment_kernels(calls) == [route, route]
            assert same(got, ref), (route, reduce)
            assert same(got_p, ref), (route, reduce, "perm")


@pytest.mark.parametrize("dtype,mode", _modes(ALL))
def test_segment_csr_picks_the_kernel_by_size_and_both_agree(dtype, mode):
    """ops.segment_csr itself: few long segments go to the wave kernel, many short ones to the
    thread kernel, and a perm changes nothing."""
    from paddle_sparse_amd import ops

    for shape, route in (("edges", "wave"), ("long", "wave"), ("powerlaw", "thread")):
        case = make_case(_lengths(shape), mode, dtype, seed=3)
        case.check(_reduces(mode))
        perm = torch.randperm(case.values.shape[0], generator=torch.Generator().manual_seed(4))
        for reduce in _reduces(mode):
            with spy("psa_segment_reduce") as calls:
                got = ops.segment_csr(case.values.cuda(), case.indptr.cuda(), reduce)
                got_p = ops.segment_csr(case.values.cuda(), case.indptr.cuda(), reduce, perm=perm.cuda())
            assert _segment_kernels(calls) == [route, route], shape
            assert same(got, segment_ref(case.values, case.indptr, reduce)), (shape, reduce)
            assert same(got_p, segment_ref(case.values, case.indptr, reduce, perm=perm)), (shape, reduce, "perm")


@pytest.mark.parametrize("dtype,mode", _modes(ALL))
def test_segment_csr_on_the_switch_between_the_kernels(dtype, mode):
    """n == 32 * nseg exactly (wave kernel) and one segment more for the same entries (thread kernel),
    through ops.segment_csr; and the same data under n_hint = 32 * nseg and 32 * nseg - 1."""
    from paddle_sparse_amd import ops

    extra = {"specials": 5, "extremes": 5}.get(mode, 0)
    extra_len = {"specials": 222, "extremes": 142}.get(mode, 0)
    base = [0, 1, 2, 63, 64, 65, 0, 33, 31, 32, 1, 0]
    nseg = len(base) + 1 + extra
    base.insert(6, 32 * nseg - sum(base) - extra_len)  # one filler segment makes n == 32 * nseg
    assert base[6] > 0
    case = make_case(np.array(base), mode, dtype, seed=5)
    case.check(_reduces(mode))
    assert case.ngroups == nseg and case.values.shape[0] == 32 * nseg
    src, indptr = case.values.cuda(), case.indptr.cuda()
    longer = torch.cat([case.indptr, case.indptr[-1:]]).cuda()  # one more (empty) segment: n < 32 * nseg
    for reduce in _reduces(mode):
        ref = segment_ref(case.values, case.indptr, reduce)
        with spy("psa_segment_reduce") as calls:
            at = ops.segment_csr(src, indptr, reduce)
            below = ops.segment_csr(src, longer, reduce)
            hint_at = _segment_direct(src, indptr, reduce, None, 32 * nseg)
            hint_below = _segment_direct(src, indptr, reduce, None, 32 * nseg - 1)
        assert _segment_kernels(calls) == ["wave", "thread", "wave", "thread"]
        assert same(at, ref) and same(hint_at, ref) and same(hint_below, ref), reduce
        assert same(below[:-1], ref) and bool((below[-1] == 0).all()), reduce


@pytest.mark.parametrize("dtype,mode", _modes(ALL))
@pytest.mark.parametrize("tail", [(1,), (2,), (3,), (5,), (64,)], ids=str)
def test_segment_csr_trailing_dims(tail, dtype, mode):
    """Trailing dims: D > 1 always takes the thread-per-element kernel; (1,) is D == 1 and may take the
    wave kernel.  Deliberate non-finite entries sit in one column; the others must stay finite."""
    from paddle_sparse_amd import ops

    case = make_case(_lengths("edges"), mode, dtype, tail, seed=6)
    case.check(_reduces(mode))
    perm = torch.randperm(case.values.shape[0], generator=torch.Generator().manual_seed(7))
    for reduce in _reduces(mode):
        with spy("psa_segment_reduce") as calls:
            got = ops.segment_csr(case.values.cuda(), case.indptr.cuda(), reduce)
            got_p = ops.segment_csr(case.values.cuda(), case.indptr.cuda(), reduce, perm=perm.cuda())
        assert _segment_kernels(calls) == (["wave"] * 2 if tail == (1,) else ["thread"] * 2)
        assert same(got, segment_ref(case.values, case.indptr, reduce)), reduce
        assert same(got_p, segment_ref(case.values, case.indptr, reduce, perm=perm)), reduce


# ---------------------------------------------------------------------------------------------
# ops.scatter
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,mode", _modes(WORD))
@pytest.mark.parametrize("tail", [(), (3,), (64,)], ids=str)
def test_scatter(tail, dtype, mode):
    """Atomics by destination row: untouched rows give 0, indices outside [0, dim_size) are ignored,
    a NaN anywhere in a group reaches its min / max, a group of nothing but the type's limit keeps it."""
    from paddle_sparse_amd import ops

    for shape in (("edges",) if tail == (64,) else SHAPES):
        case = make_case(_lengths(shape), mode, dtype, tail, seed=8)
        case.check(_reduces(mode))
        values, group = shuffled(case, 9)
        wild = group.clone()
        wild[5::97] = -1
        wild[11::89] = case.ngroups
        wild[17::83] = case.ngroups + 12345
        keep = (wild >= 0) & (wild < case.ngroups)
        assert_exact(values[keep], wild[keep], case.ngroups, sums=mode != "extremes")
        for reduce in _reduces(mode):
            with spy("psa_scatter_reduce") as calls:
                got = ops.scatter(values.cuda(), group.cuda(), case.ngroups, reduce)
                got_w = ops.scatter(values.cuda(), wild.cuda(), case.ngroups, reduce)
            assert _names(calls) == ["psa_scatter_reduce"] * 2
            assert same(got, scatter_ref(values, group, case.ngroups, reduce)), (shape, reduce)
            assert same(got_w, scatter_ref(values, wild, case.ngroups, reduce)), (shape, reduce, "out of range")


# ---------------------------------------------------------------------------------------------
# ops.unique_sorted_reduce
# ---------------------------------------------------------------------------------------------

def _short_and_edges(seed):
    """Short runs with the edge lengths among them: runs of 2047 / 2048 / 2049 entries cross the 2048-key
    tiles of unique_write_reduce_kernel whatever their offset, and runs average well under 32."""
    short = group_lengths("short", total=20_000, seed=seed)
    edges = group_lengths("edges")
    return np.concatenate([short[:3000], edges, short[3000:]])


@pytest.mark.parametrize("dtype,mode", _modes([F32, I32]))
def test_unique_sorted_reduce_fused_write_and_wave_reducer(dtype, mode):
    from paddle_sparse_amd import ops

    N = 1000
    for lengths, route in ((_short_and_edges(1), "fused"), (_lengths("long"), "wave"), (_lengths("one"), "wave")):
        case = make_case(lengths, mode, dtype, seed=10)
        case.check(_reduces(mode))
        present = case.indptr.diff() > 0
        keys = (case.group * 7 + 3)  # sorted, distinct per group, with gaps
        for reduce in _reduces(mode):
            with spy("psa_unique_write_reduce", "psa_segment_reduce") as calls:
                count, row, col, value = ops.unique_sorted_reduce(keys.cuda(), N, case.values.cuda(), reduce)
            if route == "fused":
                assert _names(calls) == ["psa_unique_write_reduce"]
            else:
                assert _names(calls) == ["psa_segment_reduce"] and _segment_kernels(calls) == ["wave"]
            ukeys = torch.arange(case.ngroups)[present] * 7 + 3
            assert count == ukeys.numel()
            assert torch.equal(row.cpu(), ukeys // N) and torch.equal(col.cpu(), ukeys % N)
            assert same(value, segment_ref(case.values, case.indptr, reduce)[present]), (route, reduce)


# ---------------------------------------------------------------------------------------------
# coalesce
# ---------------------------------------------------------------------------------------------

_CHAIN = ("psa_coalesce_small_fused", "psa_coalesce_count", "psa_coalesce_write", "psa_unique_write_reduce",
          "psa_unique_write", "psa_segment_reduce")


def _coalesce_all_ops(case, route_names, n_cols=37, seed=11, sorted_too=True):
    """coalesce of the case's groups as matrix entries, sorted and shuffled, all four ops, against the
    reference; `route_names` are the C entry points the call has to go through, in order."""
    import paddle_sparse_amd as ps

    m = (case.ngroups // n_cols + 1) * 2
    for order, (values, group) in (("sorted", (case.values, case.group)), ("shuffled", shuffled(case, seed))):
        if order == "sorted" and not sorted_too:
            continue
        index = _coo_of(group, n_cols)
        ref_index = None
        for op in ("add", "mean", "min", "max"):
            if ref_index is None:
                ref_index, _ = coalesce_ref(index, None, m, n_cols, op)
                _, inverse = torch.unique(index[0] * n_cols + index[1], sorted=True, return_inverse=True)
            ref_value = group_reduce(values, inverse, ref_index.shape[1], op)
            with spy(*_CHAIN) as calls:
                got_index, got_value = ps.coalesce(index.cuda(), values.cuda(), m, n_cols, op)
            expected = route_names(order) if callable(route_names) else route_names
            assert _names(calls) == list(expected), (order, op, _names(calls))
            assert torch.equal(got_index.cpu(), ref_index), (order, op)
            assert same(got_value, ref_value), (order, op)
        yield order, calls


@pytest.mark.parametrize("dtype,mode", _modes([F32, I32], extremes=False))
def test_coalesce_one_launch_form(dtype, mode):
    """Up to 10 240 fp32 / int32 scalar entries: sort, run lengths and the reduction in one launch."""
    from paddle_sparse_amd import ops

    case = make_case(_lengths("edges"), mode, dtype, seed=12)
    case.check()
    assert case.values.shape[0] <= ops._FUSED_SMALL
    list(_coalesce_all_ops(case, ["psa_coalesce_small_fused"]))


@pytest.mark.parametrize("dtype,mode", _modes(WORD, extremes=False) + [pytest.param(F32, "tail3", id="float32-tail3")])
def test_coalesce_two_call_chain(dtype, mode):
    """The two-call chain: up to 10 240 entries its own pack-and-reduce kernel (8-byte and vector
    values), above that the fused write (4-byte scalars) or the thread-per-element reducer."""
    from paddle_sparse_amd import ops

    tail = (3,) if mode == "tail3" else ()
    mode = "specials" if mode == "tail3" else mode
    shapes = ["long", "powerlaw"]
    if dtype in (F64, I64) or tail:
        shapes.append("edges")  # 4-byte scalars of this size take the one-launch form, tested above
    for shape in shapes:
        case = make_case(_lengths(shape), mode, dtype, tail, seed=13)
        case.check()
        n = case.values.shape[0]
        assert (n <= ops._FUSED_SMALL) == (shape == "edges") and n <= (1 << 20)
        for order, calls in _coalesce_all_ops(case, ["psa_coalesce_count", "psa_coalesce_write"]):
            pass


@pytest.mark.parametrize("dtype,mode,runs", [
    pytest.param(F32, "specials", "short", id="float32-specials-short"),
    pytest.param(F32, "specials", "long", id="float32-specials-long"),
    pytest.param(F32, "int", "short", id="float32-int-short"),
    pytest.param(F32, "int", "long", id="float32-int-long"),
    pytest.param(I32, "int", "short", id="int32-int-short"),
    pytest.param(I32, "int", "long", id="int32-int-long"),
    pytest.param(F64, "specials", "short", id="float64-specials-short"),
    pytest.param(F64, "int", "long", id="float64-int-long"),
    pytest.param(I64, "int", "short", id="int64-int-short"),
])
def test_coalesce_above_the_chain(dtype, mode, runs):
    """1.2 M entries.  4-byte scalars ride the sort (or are in order already) and take the fused write
    while runs are short, unique_write + the wave reducer when they are long; 8-byte values go through
    the permutation into the segmented reducer.  The fp32 add / mean legs are the exact counterpart of
    test_coalesce_above_the_chain_limit_equals_the_oracle's tolerance branch."""
    total = 1_200_000
    if runs == "short":
        lengths = np.concatenate([group_lengths("short", total=total - 110_000, seed=2), group_lengths("edges"),
                                  group_lengths("long")])
    else:
        lengths = np.concatenate([group_lengths("powerlaw", total=total - 110_000, seed=2)[:20_000],
                                  group_lengths("edges"), group_lengths("long")])
        lengths = np.concatenate([lengths, group_lengths("one", total=total - int(lengths.sum()))])
    case = make_case(lengths, mode, dtype, seed=14)
    case.check()
    n, groups = case.values.shape[0], int((case.indptr.diff() > 0).sum())
    assert n > (1 << 20) and (groups * 32 > n) == (runs == "short")
    if dtype in (F32, I32):
        names = ["psa_unique_write_reduce"] if runs == "short" else ["psa_unique_write", "psa_segment_reduce"]
    else:
        names = ["psa_unique_write", "psa_segment_reduce"]
    want_kernel = [] if names == ["psa_unique_write_reduce"] else (
        ["wave"] if runs == "long" else ["thread"])
    for order, calls in _coalesce_all_ops(case, names, n_cols=1009, sorted_too=dtype == F32):
        assert _segment_kernels(calls) == want_kernel, order


# ---------------------------------------------------------------------------------------------
# SparseTensor.sum / mean / min / max
# ---------------------------------------------------------------------------------------------

def _tensor_by_groups(case, dim):
    """A SparseTensor whose rows (dim == 1) or columns (dim == 0) are the case's groups, entry p of a
    group at position p of the other axis, so the order inside a group is the case's order."""
    from paddle_sparse_amd import SparseTensor

    within = torch.arange(case.group.numel()) - case.indptr[case.group]
    size = max(int(within.max()) + 1, 1)
    if dim == 1:
        return SparseTensor(row=case.group.cuda(), col=within.cuda(), value=case.values.cuda(),
                            sparse_sizes=(case.ngroups, size), is_sorted=True)
    return SparseTensor(row=within.cuda(), col=case.group.cuda(), value=case.values.cuda(),
                        sparse_sizes=(size, case.ngroups), is_sorted=False)


@pytest.mark.parametrize("dtype,mode", _modes(ALL, extremes=False))
def test_sparse_tensor_reductions_over_dim_1(dtype, mode):
    for shape in SHAPES:
        case = make_case(_lengths(shape), mode, dtype, seed=15)
        case.check()
        t = _tensor_by_groups(case, 1)
        for reduce in REDUCES:
            with spy("psa_segment_reduce", "psa_scatter_reduce") as calls:
                got = getattr(t, reduce)(dim=1)
            assert _names(calls) == ["psa_segment_reduce"]
            assert same(got, segment_ref(case.values, case.indptr, reduce)), (shape, reduce)


@pytest.mark.parametrize("dtype,mode", _modes(ALL, extremes=False))
def test_sparse_tensor_reductions_over_dim_0_before_and_after_the_csc_cache(dtype, mode):
    """Below 2^20 entries dim 0 is a scatter by column (fp16 / bf16: CSC segments, which accumulate in
    fp32) until the storage holds csr2csc, then a segmented reduction in CSC order: the same tensor
    gives the same bits on both sides of storage.csr2csc()."""
    for shape in SHAPES:
        case = make_case(_lengths(shape), mode, dtype, seed=16)
        case.check()
        ref = {r: segment_ref(case.values, case.indptr, r) for r in REDUCES}
        t = _tensor_by_groups(case, 0)
        assert not t.storage.has_csr2csc()
        before = {}
        first = ["psa_segment_reduce"] if dtype in HALF_TYPES else ["psa_scatter_reduce"]
        for reduce in REDUCES:
            with spy("psa_segment_reduce", "psa_scatter_reduce") as calls:
                before[reduce] = getattr(t, reduce)(dim=0)
            assert _names(calls) == first, (shape, reduce)
            assert same(before[reduce], ref[reduce]), (shape, reduce, "before")
        t.storage.csr2csc()
        assert t.storage.has_csr2csc() and t.storage.has_colptr()
        for reduce in REDUCES:
            with spy("psa_segment_reduce", "psa_scatter_reduce") as calls:
                after = getattr(t, reduce)(dim=0)
            assert _names(calls) == ["psa_segment_reduce"], (shape, reduce)
            assert same(after, ref[reduce]), (shape, reduce, "after")
            assert same(after, before[reduce]), (shape, reduce, "before vs after")


@pytest.mark.parametrize("dtype,mode", [
    pytest.param(F32, "specials", id="float32-specials"), pytest.param(I32, "int", id="int32-int"),
    pytest.param(F64, "int", id="float64-int"), pytest.param(I64, "int", id="int64-int"),
    pytest.param(F16, "specials", id="float16-specials"), pytest.param(BF16, "int", id="bfloat16-int"),
])
def test_sparse_tensor_reductions_over_dim_0_by_size(dtype, mode):
    """2^20 + 5 entries: dim 0 goes through the CSC segments without anybody asking for the cache."""
    total = (1 << 20) + 5
    lengths = np.concatenate([group_lengths("powerlaw", total=total - 110_000, seed=4), group_lengths("edges"),
                              group_lengths("long")])
    lengths[0] += total - int(lengths.sum()) - (222 if mode == "specials" else 0)
    case = make_case(lengths, mode, dtype, seed=17)
    case.check()
    assert case.values.shape[0] == total
    t = _tensor_by_groups(case, 0)
    assert not t.storage.has_csr2csc()
    for reduce in REDUCES:
        with spy("psa_segment_reduce", "psa_scatter_reduce") as calls:
            got = getattr(t, reduce)(dim=0)
        assert _names(calls) == ["psa_segment_reduce"]
        assert same(got, segment_ref(case.values, case.indptr, reduce)), reduce


# ---------------------------------------------------------------------------------------------
# spspmm
# ---------------------------------------------------------------------------------------------

def _coo(m, n, nnz, seed, dtype, extra=()):
    """Coalesced COO with integer values in [-3, 3]; `extra` keys (row * n + col) are entries for sure."""
    g = torch.Generator().manual_seed(seed)
    key = torch.unique(torch.cat([torch.randint(0, m * n, (nnz,), generator=g), torch.as_tensor(list(extra), dtype=torch.int64)]))
    value = torch.randint(-3, 4, (key.numel(),), generator=g).to(dtype)
    return torch.stack([key // n, key % n]), value


def _spspmm_operands(kind, dtype):
    if kind == "short":  # a random product: runs of a few terms
        m, k, n = 3000, 2500, 3500
        return _coo(m, k, 30_000, 1, dtype), _coo(k, n, 30_000, 2, dtype), (m, k, n)
    if kind == "long":  # two dense blocks: every entry of C sums 400 products
        m, k, n = 20, 400, 24
        full = lambda r, c: range(r * c)  # noqa: E731
        return _coo(m, k, 0, 3, dtype, full(m, k)), _coo(k, n, 0, 4, dtype, full(k, n)), (m, k, n)
    # hub: row 0 of A and column 0 of B are full, so C[0, 0] is one run of 12 000 products
    m, k, n = 200, 12_000, 150
    a = _coo(m, k, 20_000, 5, dtype, range(k))
    b = _coo(k, n, 20_000, 6, dtype, (r * n for r in range(k)))
    return a, b, (m, k, n)


_SPSPMM = ("psa_sort_pairs_u32_field", "psa_index_sort", "psa_sort_pairs_u32", "psa_unique_write_reduce",
           "psa_unique_write", "psa_segment_reduce")


@pytest.mark.parametrize("dtype", WORD, ids=str)
@pytest.mark.parametrize("kind", ["short", "long", "hub"])
def test_spspmm_compress_step(kind, dtype):
    """4-byte values walk B by column and sort on the row field; 8-byte values walk the CSR and sort
    the full key.  Runs averaging under 32 products are summed by the fused write (4-byte) or the
    thread reducer, over 32 by the wave reducer.  Cancelled entries stay (structural product).
    The long legs are the exact counterpart of test_bit_exact_vs_oracle's tolerance branch."""
    import paddle_sparse_amd as ps

    (iA, vA), (iB, vB), (m, k, n) = _spspmm_operands(kind, dtype)
    key, prod = spspmm_terms(iA, vA, iB, vB, m, k, n)
    uniq, inverse, counts = torch.unique(key, return_inverse=True, return_counts=True)
    assert_exact(prod, inverse, uniq.numel(), dtype, products=True)
    over = key.numel() >= 32 * uniq.numel()
    assert over == (kind == "long")
    if kind == "hub":
        assert int(counts.max()) > 10_000
    ref_i, ref_v = spspmm_ref(iA, vA, iB, vB, m, k, n)
    with spy(*_SPSPMM) as calls:
        got_i, got_v = ps.spspmm(iA.cuda(), vA.cuda(), iB.cuda(), vB.cuda(), m, k, n)
    names = _names(calls)
    if dtype in (F32, I32):  # the by-column walk is the only caller of the field sort
        assert "psa_sort_pairs_u32_field" in names, names
        assert names[-1] == ("psa_segment_reduce" if over else "psa_unique_write_reduce"), names
    else:
        assert "psa_sort_pairs_u32_field" not in names and "psa_index_sort" in names, names
        assert names[-2:] == ["psa_unique_write", "psa_segment_reduce"], names
    if names[-1] == "psa_segment_reduce":
        assert _segment_kernels(calls) == ["wave" if over else "thread"]
    assert torch.equal(got_i.cpu(), ref_i)
    assert same(got_v, ref_v)
    assert kind != "short" or bool((ref_v == 0).any())


@pytest.mark.parametrize("dtype", [F32, F64], ids=str)
def test_spspmm_specials(dtype):
    """inf * 0 and inf - inf give NaN, a NaN operand reaches every entry it takes part in."""
    import paddle_sparse_amd as ps

    inf, nan = float("inf"), float("nan")
    # A = [[inf, 1, 0], [inf, inf, 0], [2, 0, nan]]     B = [[0, 1, 1], [1, -1, 0], [0, 0, 3]]
    iA = torch.tensor([[0, 0, 1, 1, 2, 2], [0, 1, 0, 1, 0, 2]])
    vA = torch.tensor([inf, 1, inf, inf, 2, nan], dtype=dtype)
    iB = torch.tensor([[0, 0, 0, 1, 1, 2], [0, 1, 2, 0, 1, 2]])
    vB = torch.tensor([0, 1, 1, 1, -1, 3], dtype=dtype)
    ref_i, ref_v = spspmm_ref(iA, vA, iB, vB, 3, 3, 3)
    got_i, got_v = ps.spspmm(iA.cuda(), vA.cuda(), iB.cuda(), vB.cuda(), 3, 3, 3)
    assert torch.equal(got_i.cpu(), ref_i) and same(got_v, ref_v)
    out = torch.zeros(3, 3, dtype=dtype)
    out[ref_i[0], ref_i[1]] = ref_v
    assert bool(torch.isnan(out[0, 0]))                      # inf * 0 + 1 * 1
    assert bool(torch.isnan(out[1, 1]))                      # inf * 1 + inf * -1
    assert float(out[0, 1]) == inf and float(out[1, 2]) == inf
    assert bool(torch.isnan(out[2, 2])) and float(out[2, 1]) == 2.0
