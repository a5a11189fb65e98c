"""CPU suite for segment_topk: holds the numpy restatement (tests/topk_ref.py) to torch.topk and to
properties recomputed from the data alone, and the host export psa_segment_topk_host (the kernels' own
steps of csrc/topk_select.h, run serially) to the restatement bit for bit, over the case list that
test_zz_topk_gpu.py runs through the kernels, for all six dtypes.  No GPU is needed.

The file name sorts behind every other CPU file on purpose: the new tests are collected last."""
import ctypes

import numpy as np
import pytest
import torch

import topk_ref as tr
from paddle_sparse_amd import _lib, ops

SHORT, LDS = ops.TOPK_SHORT, ops.TOPK_LDS
CASES = tr.all_cases(SHORT, LDS)
SENTINEL = 0xAB
OK, INVALID = 0, 1


def host(c, out=None):
    return ops.segment_topk_host(c["value"], c["indptr"], c["k"], c["perm"], c["largest"], out,
                                 "bfloat16" if c["bf16"] else None)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_export_equals_the_restatement(name):
    c = CASES[name]
    n = c["value"].size
    want = tr.topk_ref(c["value"], c["indptr"], c["k"], c["perm"], c["largest"], np.full(n, SENTINEL, np.uint8), c["bf16"])
    got = host(c, np.full(n, SENTINEL, np.uint8))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", sorted(CASES)[::5])
def test_the_two_restatements_agree(name):
    c = CASES[name]
    args = (c["value"], c["indptr"], c["k"], c["perm"], c["largest"], None, c["bf16"])
    assert np.array_equal(tr.topk_ref(*args), tr.topk_ref_loop(*args))


def test_the_case_list_covers_every_dtype_regime_and_width():
    names = sorted(CASES)
    for dtype in tr.DTYPES:
        assert any(n.startswith(dtype) for n in names)
    for width in (8, 16, 32, 64):
        lengths = tr.short_lengths(width, SHORT)
        assert sorted(set(lengths)) == list(range(SHORT + 2))
        mean, w = -(-sum(lengths) // len(lengths)), 8
        while w < 64 and w < mean:  # the launch's choice (csrc/topk.hip, run)
            w <<= 1
        assert w == width
    assert tr.long_lengths(SHORT, LDS) == [SHORT + 1, 255, 256, 257, 511, 513, LDS - 1, LDS, LDS + 1, 3 * LDS + 17]


@pytest.mark.parametrize("name", sorted(CASES)[::3])
def test_properties_from_the_data_alone(name):
    """Per valid segment: the kept count is min(max(k, 0), len); the smallest kept key is >= the largest
    dropped key; among the keys equal to the smallest kept key, the kept entries are the earliest."""
    c = CASES[name]
    keep = host(c)
    key = tr.key_of(c["value"], c["largest"], c["bf16"])
    ptr, n = c["indptr"], key.size
    for s, (b, e) in enumerate(zip(ptr[:-1], ptr[1:])):
        if not 0 <= b <= e <= n:
            continue
        at = np.arange(b, e) if c["perm"] is None else c["perm"][b:e]
        k = c["k"] if isinstance(c["k"], int) else int(c["k"][s])
        kept, keys = keep[at].astype(bool), key[at]
        assert kept.sum() == min(max(k, 0), e - b)
        if kept.any() and not kept.all():
            t = keys[kept].min()
            assert t >= keys[~kept].max()
            at_t = np.flatnonzero(keys == t)
            q = kept[at_t].sum()
            assert kept[at_t[:q]].all() and not kept[at_t[q:]].any()


def _special_floats(rng, n, dtype):
    x = rng.integers(-3, 4, n).astype(np.float64)
    spots = rng.random(n) < 0.3
    x[spots] = rng.choice([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0], int(spots.sum()))
    return x.astype(dtype)


@pytest.mark.parametrize("dtype", ("float32", "float64", "float16"))
def test_restatement_keeps_the_multiset_torch_topk_keeps(dtype):
    """torch.topk does not say which of several equal values it keeps, so the comparison is by the
    multiset of kept keys: random segments with heavy ties, NaN of both signs, infinities and signed
    zeros, both directions."""
    rng = np.random.default_rng(101)
    for trial in range(300):
        n = int(rng.integers(1, 90))
        x = _special_floats(rng, n, dtype)
        k = int(rng.integers(1, n + 1))
        for largest in (True, False):
            keep = tr.topk_ref(x, np.array([0, n], np.int64), k, None, largest).astype(bool)
            want = torch.topk(torch.from_numpy(x).to(torch.float64), k, largest=largest).values.numpy()
            got_keys = np.sort(tr.key_of(x[keep].astype(np.float64), largest))
            assert np.array_equal(got_keys, np.sort(tr.key_of(want, largest)))


def test_integer_restatement_against_torch_topk():
    rng = np.random.default_rng(103)
    for dtype in ("int32", "int64"):
        info = np.iinfo(dtype)
        for trial in range(100):
            n = int(rng.integers(1, 90))
            x = rng.choice(np.array([info.min, -2, -1, 0, 1, 2, info.max], np.int64), n).astype(dtype)
            k = int(rng.integers(1, n + 1))
            for largest in (True, False):
                keep = tr.topk_ref(x, np.array([0, n], np.int64), k, None, largest).astype(bool)
                want = torch.topk(torch.from_numpy(x), k, largest=largest).values.numpy()
                assert np.array_equal(np.sort(x[keep]), np.sort(want))


def test_key_mapping_by_hand():
    f = lambda *v: tr.key_of(np.array(v, np.float32)).tolist()  # noqa: E731
    assert f(0.0, -0.0) == [0x80000000, 0x80000000]
    assert f(np.nan, -np.nan) == [0xFFFFFFFF, 0xFFFFFFFF]
    assert f(np.inf, -np.inf) == [0xFF800000, 0x007FFFFF]
    keys = f(-np.inf, -2.0, -1e-45, 0.0, 1e-45, 2.0, np.inf, np.nan)
    assert keys == sorted(keys) and len(set(keys)) == 8
    assert tr.key_of(np.array([np.nan], np.float32), largest=False).tolist() == [0]
    assert tr.key_of(np.array([-2**31, -1, 0, 2**31 - 1], np.int32)).tolist() == [0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
    assert tr.key_of(np.array([-2**63, 2**63 - 1], np.int64)).tolist() == [0, 2**64 - 1]
    assert tr.key_of(np.array([0x7FC0, 0xFFC1, 0x8000, 0x0000, 0x3F80], np.uint16), bf16=True).tolist() == [
        0xFFFFFFFF, 0xFFFFFFFF, 0x80000000, 0x80000000, 0xBF800000]
    h = tr.key_of(np.array([np.nan, 0.0, -0.0, 65504.0, -65504.0], np.float16)).tolist()
    assert h == [0xFFFFFFFF, 0x8000, 0x8000, 0xFBFF, 0x0400]


def test_tie_rule_by_hand():
    x = np.array([1, 3, 3, 2, 3, 1], np.float32)
    ptr = np.array([0, 6], np.int64)
    assert ops.segment_topk_host(x, ptr, 2).tolist() == [0, 1, 1, 0, 0, 0]
    assert ops.segment_topk_host(x, ptr, 4).tolist() == [0, 1, 1, 1, 1, 0]
    assert ops.segment_topk_host(x, ptr, 1, largest=False).tolist() == [1, 0, 0, 0, 0, 0]
    assert ops.segment_topk_host(x, ptr, 5, perm=np.array([5, 4, 3, 2, 1, 0], np.int64)).tolist() == [0, 1, 1, 1, 1, 1]
    x = np.array([np.nan, 5, -np.nan, np.inf], np.float32)
    assert ops.segment_topk_host(x, np.array([0, 4], np.int64), 1).tolist() == [1, 0, 0, 0]
    assert ops.segment_topk_host(x, np.array([0, 4], np.int64), 3).tolist() == [1, 0, 1, 1]
    assert ops.segment_topk_host(x, np.array([0, 4], np.int64), 2, largest=False).tolist() == [0, 1, 0, 1]


def test_public_names_and_symbols():
    import paddle_sparse_amd as psa
    from test_abi import declared_functions

    import importlib

    module = importlib.import_module("paddle_sparse_amd.topk")
    for name in ("topk", "segment_topk"):
        assert name in psa.__all__ and getattr(psa, name) is getattr(module, name)
    assert psa.SparseTensor.topk is module.topk
    declared = declared_functions()
    for name in ("psa_segment_topk", "psa_segment_topk_host"):
        assert name in declared and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["psa_segment_topk"][1]) == len(_lib.SIGNATURES["psa_segment_topk_host"][1]) + 1
    assert not [n for n in _lib.SIGNATURES if "topk" in n and n.endswith("_workspace_bytes")]  # no scratch
    assert (ops.TOPK_SHORT, ops.TOPK_LDS, ops.TOPK_GRID, ops.TOPK_CHUNK) == (64, 4096, 2048, 256)


def test_argument_errors_and_zero_counts():
    lib = _lib.load()
    value = np.arange(6, dtype=np.float32)
    ptr = np.array([0, 2, 6], np.int64)
    keep = np.full(6, SENTINEL, np.uint8)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def call(value_=p(value), dtype=0, ptr_=p(ptr), nseg=2, n=6, keep_=p(keep)):
        return lib.psa_segment_topk_host(value_, dtype, None, ptr_, nseg, n, 1, None, 1, keep_)

    assert call() == OK and keep.tolist() == [0, 1, 0, 0, 0, 1]
    for kw in (dict(dtype=6), dict(dtype=-1), dict(nseg=-1), dict(n=-1), dict(value_=None), dict(ptr_=None),
               dict(keep_=None)):
        keep[:] = SENTINEL
        assert call(**kw) == INVALID, kw
        assert b"psa_segment_topk_host" in lib.psa_last_error()
        assert (keep == SENTINEL).all()
    for kw in (dict(nseg=0), dict(n=0), dict(nseg=0, value_=None, ptr_=None, keep_=None)):
        assert call(**kw) == OK and (keep == SENTINEL).all(), kw
    # the device entry point refuses the same arguments before it launches anything
    assert lib.psa_segment_topk(1, 9, None, 1, 2, 6, 1, None, 1, 1, None) == INVALID
    assert lib.psa_segment_topk(1, 0, None, 1, -2, 6, 1, None, 1, 1, None) == INVALID
    assert lib.psa_segment_topk(1, 0, None, 1, 2, -6, 1, None, 1, 1, None) == INVALID
    assert lib.psa_segment_topk(None, 0, None, 1, 2, 6, 1, None, 1, 1, None) == INVALID
    assert lib.psa_segment_topk(1, 0, None, None, 2, 6, 1, None, 1, 1, None) == INVALID
    assert lib.psa_segment_topk(1, 0, None, 1, 2, 6, 1, None, 1, None, None) == INVALID
    assert b"psa_segment_topk" in lib.psa_last_error()
    assert lib.psa_segment_topk(None, 0, None, None, 0, 6, 1, None, 1, None, None) == OK
    assert lib.psa_segment_topk(None, 0, None, None, 2, 0, 1, None, 1, None, None) == OK
    assert isinstance(lib, ctypes.CDLL)


def test_ops_argument_checks():
    x = torch.zeros(4)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.segment_topk(x, torch.tensor([0, 4]), 1)
    with pytest.raises(TypeError):
        ops.segment_topk_host(np.zeros(4, np.int8), [0, 4], 1)
    with pytest.raises(TypeError):
        ops.segment_topk_host(np.zeros(4, np.float32), [0, 4], 1.5)
    with pytest.raises(ValueError):
        ops.segment_topk_host(np.zeros(4, np.float32), [0, 4], np.array([1, 2], np.int64))
    with pytest.raises(ValueError):
        ops.segment_topk_host(np.zeros(4, np.float32), [0, 4], 1, perm=np.arange(3))
    with pytest.raises(ValueError):
        ops.segment_topk_host(np.zeros((2, 2), np.float32), [0, 4], 1)


def test_surface_argument_checks_need_no_gpu():
    import paddle_sparse_amd as psa

    with pytest.raises(TypeError):
        psa.topk(object(), 1)
    with pytest.raises(ValueError):
        psa.segment_topk(torch.zeros(2, 2), torch.tensor([0, 2]), 1)
    with pytest.raises(TypeError):
        psa.segment_topk(torch.zeros(4), torch.tensor([0, 4]), 1.5)
    with pytest.raises(ValueError):
        psa.segment_topk(torch.zeros(4), torch.tensor([0, 4]), torch.tensor([1, 2]))
