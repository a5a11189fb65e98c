"""The float64 reference of the attention path (tests/softmax_ref.py) against hand-worked
answers and torch on the CPU, and the presence of the new public names and C-ABI symbols.
No kernel runs here."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import softmax_ref as sr

ROOT = Path(__file__).resolve().parent.parent
INF = float("inf")
NAN = float("nan")

# 5 rows: [0, 0] | [ln 1, ln 3] | (empty) | [5] | [ln 1, ln 2, ln 5]
INDPTR = np.array([0, 2, 4, 4, 5, 8])
SRC = np.array([0.0, 0.0, math.log(1.0), math.log(3.0), 5.0, math.log(1.0), math.log(2.0), math.log(5.0)])
WANT = np.array([0.5, 0.5, 0.25, 0.75, 1.0, 0.125, 0.25, 0.625])


def test_forward_by_hand():
    np.testing.assert_allclose(sr.softmax_ref(SRC, INDPTR), WANT, rtol=1e-15)


def test_forward_heads_and_perm_by_hand():
    two = np.stack([SRC, SRC[::-1].copy()], axis=1)  # head 1: other numbers, same segments
    got = sr.softmax_ref(two, INDPTR)
    np.testing.assert_allclose(got[:, 0], WANT, rtol=1e-15)
    np.testing.assert_allclose(got[:2, 1], [5 / 7, 2 / 7], rtol=1e-15)  # [ln 5, ln 2]
    # perm: position j is row perm[j]; the result stays in row order
    perm = np.array([7, 3, 0, 5, 1, 2, 6, 4])
    src = np.empty(8)
    src[perm] = SRC
    want = np.empty(8)
    want[perm] = WANT
    np.testing.assert_allclose(sr.softmax_ref(src, INDPTR, perm), want, rtol=1e-15)


def test_backward_by_hand():
    y = np.array([0.25, 0.75, 1.0])
    g = np.array([1.0, 2.0, 7.0])
    # dot = 0.25 + 1.5 = 1.75 -> [0.25 * (1 - 1.75), 0.75 * (2 - 1.75)]; a single entry gets 0
    got = sr.softmax_bw_ref(y, g, np.array([0, 2, 2, 3]))
    assert got.tolist() == [-0.1875, 0.1875, 0.0]
    perm = np.array([2, 0, 1])
    yp, gp = np.empty(3), np.empty(3)
    yp[perm], gp[perm] = y, g
    want = np.empty(3)
    want[perm] = got
    assert sr.softmax_bw_ref(yp, gp, np.array([0, 2, 2, 3]), perm).tolist() == want.tolist()


@pytest.mark.parametrize("shape", [(0,), (0, 1), (0, 3)])
@pytest.mark.parametrize("indptr", [[0], [0, 0, 0, 0]])
def test_no_entries(shape, indptr):
    z, ptr, perm = np.zeros(shape), np.array(indptr), np.zeros(0, dtype=np.int64)
    for p in (None, perm):
        assert sr.softmax_ref(z, ptr, p).shape == shape
        assert sr.softmax_bw_ref(z, z, ptr, p).shape == shape
        length, scale = sr.softmax_bw_bound_terms(z, z, ptr, p)
        assert length.shape == shape and scale.shape == shape
    assert sr.segment_lengths(ptr, 0, None, shape[1:]).shape == shape


def test_sddmm_by_hand():
    rowptr, col = np.array([0, 2, 2, 3]), np.array([0, 2, 1])
    x = np.array([[1.0, 2.0], [9.0, 9.0], [-1.0, 3.0]])
    y = np.array([[4.0, 0.0], [2.0, 2.0], [1.0, -1.0], [7.0, 7.0]])
    assert sr.sddmm_ref(rowptr, col, x, y).tolist() == [4.0, -1.0, 4.0]


def _dense_rows(src, indptr):
    """The segments as rows of a dense matrix, missing entries at -inf."""
    nseg, width = indptr.size - 1, int(np.diff(indptr).max())
    dense = torch.full((nseg, width), -INF, dtype=torch.float64)
    for s in range(nseg):
        dense[s, :indptr[s + 1] - indptr[s]] = torch.from_numpy(src[indptr[s]:indptr[s + 1]])
    return dense


def test_forward_and_backward_against_torch_float64():
    rng = np.random.default_rng(5)
    lens = [3, 1, 7, 2, 40]  # no empty row: torch gives NaN for a row of nothing but -inf
    indptr = np.concatenate([[0], np.cumsum(lens)])
    src = rng.uniform(-8, 8, indptr[-1])
    g = rng.normal(size=indptr[-1])
    dense = _dense_rows(src, indptr).requires_grad_()
    out = torch.softmax(dense, dim=1)
    gd = torch.zeros_like(out)
    for s in range(len(lens)):
        gd[s, :lens[s]] = torch.from_numpy(g[indptr[s]:indptr[s + 1]])
    out.backward(gd)
    got = sr.softmax_ref(src, indptr)
    got_bw = sr.softmax_bw_ref(got, g, indptr)
    for s in range(len(lens)):
        sl = slice(indptr[s], indptr[s + 1])
        np.testing.assert_allclose(got[sl], out[s, :lens[s]].detach().numpy(), rtol=1e-14)
        np.testing.assert_allclose(got_bw[sl], dense.grad[s, :lens[s]].numpy(), rtol=1e-12, atol=1e-16)


NONFINITE = {
    "nan": ([1.0, NAN, 3.0], [NAN, NAN, NAN]),
    "plus_inf": ([1.0, INF, 3.0], [NAN, NAN, NAN]),
    "two_plus_inf": ([INF, INF], [NAN, NAN]),
    "all_minus_inf": ([-INF, -INF], [NAN, NAN]),
    "one_minus_inf": ([-INF], [NAN]),
    "minus_inf_among_finite": ([0.0, -INF, 0.0, -INF], [0.5, 0.0, 0.5, 0.0]),
    "nan_and_minus_inf": ([-INF, NAN], [NAN, NAN]),
}


@pytest.mark.parametrize("case", sorted(NONFINITE))
def test_nonfinite_rule(case):
    """The rule as the issue states it; torch.softmax on the CPU agrees except that it gives NaN,
    not a crash, for +inf — compared where both are defined the same way."""
    src, want = (np.array(a) for a in NONFINITE[case])
    got = sr.softmax_ref(src, np.array([0, src.size]))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])
    ref = torch.softmax(torch.from_numpy(src), 0).numpy()
    assert np.array_equal(np.isnan(ref), np.isnan(want))
    np.testing.assert_array_equal(ref[~np.isnan(ref)], want[~np.isnan(want)])


def test_nonfinite_rule_is_per_head():
    src = np.array([[1.0, NAN], [2.0, 0.0]])
    got = sr.softmax_ref(src, np.array([0, 2]))
    assert not np.isnan(got[:, 0]).any() and np.isnan(got[:, 1]).all()


def test_backward_zero_output_gets_zero_gradient():
    y = sr.softmax_ref(np.array([0.0, -INF, 0.0]), np.array([0, 3]))
    got = sr.softmax_bw_ref(y, np.array([3.0, 100.0, -1.0]), np.array([0, 3]))
    assert got[1] == 0.0 and got[0] == -got[2] == 1.0  # 0.5 * (3 - 1)


def test_public_names_are_the_modules_functions():
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import sddmm as sddmm_mod
    from paddle_sparse_amd import softmax as softmax_mod

    assert "softmax" in psa.__all__ and "sddmm" in psa.__all__
    import importlib

    assert psa.softmax is importlib.import_module("paddle_sparse_amd.softmax").softmax
    assert psa.sddmm is importlib.import_module("paddle_sparse_amd.sddmm").sddmm
    assert callable(softmax_mod) and callable(sddmm_mod)
    assert callable(psa.SparseTensor.softmax) and callable(psa.SparseTensor.sddmm)


NEW_SYMBOLS = ("psa_segment_softmax_workspace_bytes", "psa_segment_softmax", "psa_segment_softmax_bw")


def test_new_symbols_are_exported_and_bound():
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    header = (ROOT / "include" / "paddle_sparse_hip.h").read_text()
    shim = (ROOT / "integration" / "paddle_shim" / "paddle_sparse_hip_ops.cc").read_text()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
        assert re.search(rf"\b{name}\s*\(", header)
        assert re.search(rf"\b{name}\s*\(", shim)
    assert lib.psa_abi_version() == 1
    # no segment above 128 entries is possible: no scratch; otherwise list + partials
    assert lib.psa_segment_softmax_workspace_bytes(128, 8) == 0
    assert lib.psa_segment_softmax_workspace_bytes(129, 8) > 0


def test_wrappers_reject_cpu_tensors_and_other_dtypes():
    from paddle_sparse_amd import ops

    with pytest.raises(RuntimeError):
        ops.segment_softmax(torch.zeros(3), torch.tensor([0, 3]))
    with pytest.raises(RuntimeError):
        ops.sddmm(torch.tensor([0, 1]), torch.tensor([0]), torch.zeros(1, 2), torch.zeros(1, 2))
