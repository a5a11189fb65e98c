"""The exact grouped-reduction reference (tests/reduce_ref.py) against the numpy oracle, the C spspmm
oracle and the framework's own reducers, CPU only.

On integer data below the `assert_exact` bound the oracle's arithmetic in the values' own dtype is
exact too, so the two agree bit for bit in every dtype; on the `specials` data the reference equals
amin / amax / sum taken group by group; and `assert_exact` rejects data that breaks its bound."""
import numpy as np
import pytest
import torch

import oracle
from oracle import storage_oracle as so
from reduce_ref import (HALF_TYPES, REDUCES, SHAPES, assert_exact, coalesce_ref, group_lengths, group_reduce,
                        make_case, same, scatter_ref, segment_ref, shuffled, spspmm_ref, spspmm_terms)

NP_DTYPES = [torch.float32, torch.float64, torch.int32, torch.int64]
ALL_DTYPES = NP_DTYPES + list(HALF_TYPES)


def _lengths(shape):
    return group_lengths(shape, total=20_000 if shape == "powerlaw" else None, seed=3)


def _via_numpy(fn, values: torch.Tensor, *args):
    """The numpy oracle on `values`; half-width dtypes go through fp32, where the integer data is exact,
    and are rounded once at the end as the kernels round."""
    wide = values.to(torch.float32) if values.dtype in HALF_TYPES else values
    return torch.from_numpy(np.asarray(fn(wide.numpy(), *args))).to(values.dtype)


@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES)
def test_segment_ref_equals_the_oracle(shape, dtype, reduce):
    tail = (3,) if shape == "edges" else ()
    case = make_case(_lengths(shape), "int", dtype, tail, seed=1)
    case.check()
    ref = segment_ref(case.values, case.indptr, reduce)
    fast = _via_numpy(so.segment_csr_fast, case.values, case.indptr.numpy(), reduce)
    assert same(ref, fast)
    if shape != "long":  # the sequential oracle is a Python loop over the entries
        assert same(ref, _via_numpy(so.segment_csr, case.values, case.indptr.numpy(), reduce))
    perm = torch.randperm(case.values.shape[0], generator=torch.Generator().manual_seed(2))
    assert same(segment_ref(case.values, case.indptr, reduce, perm=perm),
                _via_numpy(so.segment_csr_fast, case.values[perm], case.indptr.numpy(), reduce))


@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("dtype", NP_DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES)
def test_scatter_ref_equals_the_oracle(shape, dtype, reduce):
    case = make_case(_lengths(shape), "int", dtype, (2,), seed=4)
    case.check()
    values, group = shuffled(case, 5)
    ref = scatter_ref(values, group, case.ngroups, reduce)
    assert same(ref, _via_numpy(so.scatter, values, group.numpy(), case.ngroups, reduce))
    # indices outside [0, dim_size) are ignored
    wild = group.clone()
    wild[::7] = -1
    wild[3::11] = case.ngroups
    keep = (wild >= 0) & (wild < case.ngroups)
    assert same(scatter_ref(values, wild, case.ngroups, reduce), scatter_ref(values[keep], wild[keep], case.ngroups, reduce))


def _coo_of(group: torch.Tensor, n: int):
    """Group g as the matrix position (g // n * 2, g % n): distinct groups, distinct positions."""
    return torch.stack([group // n * 2, group % n])


@pytest.mark.parametrize("op", ["add", "mean", "min", "max"])
@pytest.mark.parametrize("dtype", NP_DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES)
def test_coalesce_ref_equals_the_oracle(shape, dtype, op):
    tail = (3,) if shape == "powerlaw" else ()
    case = make_case(_lengths(shape), "int", dtype, tail, seed=6)
    case.check()
    n = 37
    m = (case.ngroups // n + 1) * 2
    for values, group in ((case.values, case.group), shuffled(case, 7)):
        index = _coo_of(group, n)
        ref_i, ref_v = coalesce_ref(index, values, m, n, op)
        o_i, o_v = so.coalesce(index.numpy(), values.numpy(), m, n, op)
        assert np.array_equal(ref_i.numpy(), o_i)
        assert same(ref_v, torch.from_numpy(np.asarray(o_v)))
    assert coalesce_ref(index, None, m, n, op)[1] is None


def _random_coo(m, n, nnz, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    key = torch.unique(torch.randint(0, m * n, (nnz,), generator=g))
    value = torch.randint(-3, 4, (key.numel(),), generator=g).to(dtype)
    return torch.stack([key // n, key % n]), value


@pytest.mark.parametrize("dtype", NP_DTYPES, ids=str)
def test_spspmm_ref_equals_the_oracle(dtype):
    m, k, n = 60, 50, 70
    iA, vA = _random_coo(m, k, 500, 1, dtype)
    iB, vB = _random_coo(k, n, 600, 2, dtype)
    key, prod = spspmm_terms(iA, vA, iB, vB, m, k, n)
    uniq, inverse = torch.unique(key, return_inverse=True)
    assert_exact(prod, inverse, uniq.numel(), dtype, products=True)
    ref_i, ref_v = spspmm_ref(iA, vA, iB, vB, m, k, n)
    o_i, o_v = oracle.spspmm(iA.numpy(), vA.to(torch.float32).numpy(), iB.numpy(), vB.to(torch.float32).numpy(), m, k, n)
    assert np.array_equal(ref_i.numpy(), o_i)
    assert ref_v.dtype == dtype and np.array_equal(ref_v.to(torch.float32).numpy(), o_v)
    assert bool((ref_v == 0).any()), "no cancelled entry in this product: the structural rule is not exercised"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("shape", SHAPES)
def test_specials_equal_the_frameworks_reducers_group_by_group(shape, dtype):
    case = make_case(_lengths(shape), "specials", dtype, (2,), seed=8)
    case.check()
    wide = torch.float64 if dtype == torch.float64 else torch.float32
    out = {r: segment_ref(case.values, case.indptr, r) for r in REDUCES}
    for g in range(case.ngroups):
        b, e = int(case.indptr[g]), int(case.indptr[g + 1])
        if e == b:
            assert all(bool((out[r][g] == 0).all()) for r in REDUCES)
            continue
        seg = case.values[b:e].to(wide)
        assert same(out["min"][g], seg.amin(0).to(dtype)) and same(out["max"][g], seg.amax(0).to(dtype))
        total = seg.to(torch.float64).sum(0)
        assert same(out["sum"][g], total.to(dtype))
        assert same(out["mean"][g], (total.to(wide) / torch.tensor(e - b, dtype=wide)).to(dtype))
    # the deliberate groups give what the rule says, in the column that holds them
    mk, col = case.marks, 1
    for name in ("nan_first", "nan_last", "nan_at_64_of_200", "all_nan"):
        for r in REDUCES:
            assert bool(torch.isnan(out[r][mk[name], col])), (name, r)
            assert name == "all_nan" or bool(torch.isfinite(out[r][mk[name], 0])), (name, r)
    g = mk["both_inf"]
    assert bool(torch.isnan(out["sum"][g, col])) and bool(torch.isnan(out["mean"][g, col]))
    assert float(out["min"][g, col]) == float("-inf") and float(out["max"][g, col]) == float("inf")
    # and the same through the scatter form of the reference, in any entry order
    values, group = shuffled(case, 9)
    for r in REDUCES:
        assert same(scatter_ref(values, group, case.ngroups, r), out[r])


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=str)
def test_extremes_mode(dtype):
    case = make_case(group_lengths("edges"), "extremes", dtype, (2,), seed=10)
    case.check(("min", "max"))
    lo, hi = torch.iinfo(dtype).min, torch.iinfo(dtype).max
    mn, mx = segment_ref(case.values, case.indptr, "min"), segment_ref(case.values, case.indptr, "max")
    mk = case.marks
    assert mn[mk["only_min"]].tolist() == [lo, lo] and mx[mk["only_min"]].tolist() == [lo, lo]
    assert mn[mk["only_max"]].tolist() == [hi, hi] and mx[mk["only_max"]].tolist() == [hi, hi]
    assert mn[mk["all_max"]].tolist() == [hi, hi] and mx[mk["all_min"]].tolist() == [lo, lo]
    assert int(mn[mk["min_and_max"], 1]) == lo and int(mx[mk["min_and_max"], 1]) == hi
    assert abs(int(mn[mk["min_and_max"], 0])) <= 4 and abs(int(mx[mk["min_and_max"], 0])) <= 4
    assert same(mn, _via_numpy(so.segment_csr_fast, case.values, case.indptr.numpy(), "min"))
    assert same(mx, _via_numpy(so.segment_csr_fast, case.values, case.indptr.numpy(), "max"))
    assert bool((mn[case.indptr.diff() == 0] == 0).all())


def test_int_mode_marks_both_ends_of_every_group():
    """Cutting the first or the last entry off any group of two or more changes its sum, min or max."""
    for dtype in (torch.float32, torch.bfloat16, torch.int64):
        case = make_case(group_lengths("edges"), "int", dtype, seed=11)
        for g in range(case.ngroups):
            b, e = int(case.indptr[g]), int(case.indptr[g + 1])
            if e - b >= 2:
                seg = case.values[b:e].to(torch.float64)
                assert float(seg[0]) == -4 and float(seg[-1]) == 4
                assert float(seg[1:].min()) > -4 and float(seg[:-1].max()) < 4


def test_assert_exact_rejects_data_that_breaks_its_bound():
    group = torch.zeros(4, dtype=torch.int64)
    ok = torch.tensor([1.0, -2.0, float("nan"), float("inf")])
    assert_exact(ok, group, 1)
    with pytest.raises(AssertionError, match="non-integer"):
        assert_exact(torch.tensor([1.0, 0.5, 0.0, 0.0]), group, 1)
    with pytest.raises(AssertionError, match="-0.0"):
        assert_exact(torch.tensor([1.0, -0.0, 0.0, 0.0]), group, 1)
    big = torch.full((4,), float(1 << 22))
    with pytest.raises(AssertionError, match="sum"):
        assert_exact(big, group, 1)
    assert_exact(big, torch.arange(4), 4)  # the same values in groups of their own stay below the bound
    assert_exact(big, group, 1, sums=False)  # min / max only: no sum is taken
    assert_exact(big.to(torch.float64), group, 1)
    with pytest.raises(AssertionError, match="sum"):
        assert_exact(torch.full((4,), 100.0, dtype=torch.bfloat16), group, 1)
    assert_exact(torch.full((4,), 100.0, dtype=torch.float16), group, 1)
    with pytest.raises(AssertionError, match="sum"):
        assert_exact(torch.full((4,), 600.0, dtype=torch.float16), group, 1)
    with pytest.raises(AssertionError, match="integer sums"):
        assert_exact(torch.full((4,), 1 << 30, dtype=torch.int32), group, 1)
    assert_exact(torch.full((4,), 1 << 30, dtype=torch.int64), group, 1)
    # entries that a scatter ignores do not count
    assert_exact(big, torch.tensor([0, -1, 5, 1]), 2)


def test_group_reduce_ignores_nothing_it_should_keep():
    v = torch.tensor([[1.0, float("nan")], [2.0, 3.0], [float("inf"), 4.0], [float("-inf"), 5.0]])
    g = torch.tensor([0, 0, 2, 2])
    assert same(group_reduce(v, g, 4, "min"), torch.tensor([[1.0, float("nan")], [0, 0], [float("-inf"), 4.0], [0, 0]]))
    assert same(group_reduce(v, g, 4, "max"), torch.tensor([[2.0, float("nan")], [0, 0], [float("inf"), 5.0], [0, 0]]))
    assert same(group_reduce(v, g, 4, "sum"), torch.tensor([[3.0, float("nan")], [0, 0], [float("nan"), 9.0], [0, 0]]))
    i = torch.tensor([-7, 2, -1], dtype=torch.int32)
    assert group_reduce(i, torch.zeros(3, dtype=torch.int64), 1, "mean").tolist() == [-2]  # floor(-6 / 3)
    assert group_reduce(i[:2], torch.zeros(2, dtype=torch.int64), 1, "mean").tolist() == [-3]  # floor(-5 / 2)
