"""The reference of the index-range tests, checked on the CPU: phi is strictly increasing and hits every band
edge, and the Python-int dict-of-keys oracle applied to injected operands equals phi applied to the references
the suite already uses (oracle.spspmm, oracle.storage_oracle, reduce_ref.coalesce_ref) on the small operands —
the property tests/test_index_range_gpu.py relies on, confirmed without phi in the loop."""
import numpy as np
import pytest
import torch

import index_range_ref as ir
import oracle
import reduce_ref as rr
from oracle import storage_oracle as so

BIG = [pytest.param(b, id=str(b)) for b in ir.BIG_DIMS]


@pytest.mark.parametrize("big", BIG)
@pytest.mark.parametrize("small", [40, 41, 97, 300])
def test_phi_is_strictly_increasing_and_hits_every_band_edge(small, big):
    ids = np.arange(small, dtype=np.int64)
    img = ir.inject(ids, small, big)
    assert img.dtype == np.int64 and img.shape == ids.shape
    as_ints = [int(x) for x in img]
    assert all(b > a for a, b in zip(as_ints, as_ints[1:])), "phi is not strictly increasing"
    assert as_ints[0] == 0 and as_ints[-1] == big - 1
    for edge in ir.EDGE_VALUES + (big - 1,):
        if edge < big:
            assert edge in as_ints, f"{edge} is not hit for big_dim = {big}"
    # blocks tile the small range, their images are disjoint and ordered
    blocks = ir.band_blocks(small, big)
    assert blocks[0][0] == 0 and blocks[-1][1] == small
    for (f0, s0, i0), (f1, s1, i1) in zip(blocks, blocks[1:]):
        assert s0 == f1 and i0 + (s0 - f0) <= i1
    # a permutation of the ids maps elementwise
    perm = np.random.default_rng(small).permutation(small)
    assert np.array_equal(ir.inject(perm, small, big), img[perm])


def test_phi_single_band_is_a_shift_and_bad_input_is_refused():
    ids = np.array([0, 5, 49], dtype=np.int64)
    assert np.array_equal(ir.inject(ids, 50, ir.LIMIT, bands=("end",)), ids + (ir.LIMIT - 50))
    assert np.array_equal(ir.inject(ids, 50, ir.LIMIT, bands=("zero",)), ids)
    with pytest.raises(AssertionError):
        ir.inject(np.array([50]), 50, ir.LIMIT)
    with pytest.raises(ValueError):
        ir.inject(ids, 50, 49)
    with pytest.raises(ValueError):
        ir.band_blocks(39, ir.LIMIT)


def test_covering_index_reaches_every_edge_value():
    rng = np.random.default_rng(3)
    index = ir.coalesced_index(rng, 200, 120, 900)
    key = index[0] * 120 + index[1]
    assert index.shape == (2, 900) and bool((key[1:] > key[:-1]).all())
    for big in ir.BIG_DIMS:
        for d, small in ((0, 200), (1, 120)):
            img = set(int(x) for x in ir.inject(index[d], small, big))
            for edge in ir.EDGE_VALUES + (big - 1,):
                assert edge >= big or edge in img, (big, d, edge)


def _case(seed, m, n, nnz):
    rng = np.random.default_rng(seed)
    index = ir.coalesced_index(rng, m, n, nnz)
    return index, ir.nonzero_integers(rng, nnz).astype(np.float32)


@pytest.mark.parametrize("big", BIG)
def test_oracle_spspmm_equals_phi_of_the_reference(big):
    m, k, n = 90, 50, 70
    index_a, value_a = _case(1, m, k, 400)
    index_b, value_b = _case(2, k, n, 350)
    ref_index, ref_value = oracle.spspmm(index_a, value_a, index_b, value_b, m, k, n)
    big_a = ir.inject_index(index_a, (m, k), (big, None))
    big_b = ir.inject_index(index_b, (k, n), (None, big))
    got_index, got_value = ir.dok_spspmm(big_a, value_a, big_b, value_b)
    assert np.array_equal(got_index, ir.inject_index(ref_index, (m, n), (big, big)))
    assert np.array_equal(np.array(got_value, dtype=np.float64), ref_value.astype(np.float64))
    # value-less operands count as ones
    ones_a = np.ones_like(value_a)
    ref_index, ref_value = oracle.spspmm(index_a, ones_a, index_b, value_b, m, k, n)
    got_index, got_value = ir.dok_spspmm(big_a, None, big_b, value_b)
    assert np.array_equal(got_index, ir.inject_index(ref_index, (m, n), (big, big)))
    assert np.array_equal(np.array(got_value, dtype=np.float64), ref_value.astype(np.float64))


@pytest.mark.parametrize("big", BIG)
@pytest.mark.parametrize("op", ["add", "mul"])
def test_oracle_union_and_intersection_equal_phi_of_the_reference(op, big):
    m, n = 80, 60
    index_a, value_a = _case(3, m, n, 700)
    index_b, value_b = _case(4, m, n, 650)
    a = so.Storage(index_a[0], index_a[1], value_a, (m, n), True)
    b = so.Storage(index_b[0], index_b[1], value_b, (m, n), True)
    ref = so.add(a, b) if op == "add" else so.mul(a, b)
    assert 0 < ref.row.size < 1350
    big_a, big_b = ir.inject_index(index_a, (m, n), (big, big)), ir.inject_index(index_b, (m, n), (big, big))
    fn = ir.dok_union if op == "add" else ir.dok_intersection
    got_index, got_value = fn(big_a, value_a, big_b, value_b)
    assert np.array_equal(got_index, ir.inject_index(np.stack([ref.row, ref.col]), (m, n), (big, big)))
    assert np.array_equal(np.array(got_value, dtype=np.float64), ref.value.astype(np.float64))


@pytest.mark.parametrize("big", BIG)
@pytest.mark.parametrize("op", ["add", "max"])
def test_oracle_coalesce_equals_phi_of_the_reference(op, big):
    m, n, nnz = 70, 90, 1500
    rng = np.random.default_rng(5)
    base = ir.coalesced_index(rng, m, n, 600)
    index = base[:, rng.integers(0, 600, nnz)]  # duplicates, shuffled
    index[:, :600] = base[:, rng.permutation(600)]
    value = ir.nonzero_integers(rng, nnz, (2,)).astype(np.float32)
    ref_index, ref_value = rr.coalesce_ref(torch.from_numpy(index), torch.from_numpy(value), m, n, op)
    assert ref_index.shape[1] == 600
    got_index, got_value = ir.dok_coalesce(ir.inject_index(index, (m, n), (big, big)), value, op)
    assert np.array_equal(got_index, ir.inject_index(ref_index.numpy(), (m, n), (big, big)))
    assert np.array_equal(np.array(got_value, dtype=np.float64), ref_value.numpy().astype(np.float64))
