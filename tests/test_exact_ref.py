"""The exact SpMM reference (tests/exact_ref.py) against the fp32 C oracle, CPU only.

On integer data whose sums stay below 2^24 the oracle's fp32 arithmetic is exact too, so the two
must agree bit for bit: forward out and arg_out, and every backward entry point, for every
reduction — on graphs with empty rows, hubs, long rows and many ties, and on the README answer."""
import numpy as np
import pytest
import torch

import oracle
from exact_ref import (EXACT, FLT_MAX, assert_exact_preconditions, csr_with_col_degrees, csr_with_degrees, int_data,
                       integers, pow2_degrees, spmm_backward_ref, spmm_ref, with_specials)

REDUCES = ["sum", "mean", "min", "max"]


def _np(x):
    return None if x is None else x.numpy()


def _graphs():
    rng = np.random.default_rng(0)
    deg = rng.integers(0, 6, 300)
    deg[rng.random(300) < 0.25] = 0
    deg[[3, 150, 299]] = [129, 700, 65]  # long rows among short and empty ones
    yield "mixed", csr_with_degrees(deg, 90, seed=1), deg
    yield "hub_columns", csr_with_degrees(rng.integers(0, 40, 120), 500, seed=2, col_skew=6.0), None
    col_deg = rng.integers(0, 4, 200)
    col_deg[[0, 77]] = [300, 129]
    yield "hub_columns_exact", csr_with_col_degrees(col_deg, 150, seed=3), None
    yield "all_empty", csr_with_degrees([0] * 7, 5), None
    yield "one_row", csr_with_degrees([2000], 3, seed=4), None  # three columns: nearly every product ties


GRAPHS = list(_graphs())


@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("K", [1, 3, 8, 33])
@pytest.mark.parametrize("with_value", [True, False])
@pytest.mark.parametrize("graph", [g[0] for g in GRAPHS])
def test_forward_matches_the_oracle_bit_for_bit(reduce, K, with_value, graph):
    (rowptr, col), _ = next((g[1], g[2]) for g in GRAPHS if g[0] == graph)
    N = int(col.max()) + 1 if col.numel() else 5
    value, mat, _ = int_data(rowptr, N, K, seed=K, with_value=with_value)
    assert_exact_preconditions(rowptr, col, value, mat)
    out, arg = spmm_ref(reduce, rowptr, col, value, mat)
    want, want_arg = oracle.spmm(reduce, rowptr.numpy(), col.numpy(), _np(value), mat.numpy())
    assert out.dtype == torch.float32 and np.array_equal(out.numpy(), want)
    if reduce in ("min", "max"):
        assert np.array_equal(arg.numpy(), want_arg)
        if graph == "one_row":  # ties everywhere: the winner is the first edge that reaches the extreme
            p = (value if with_value else torch.ones(col.numel()))[:, None] * mat[col]
            first = torch.argmax((p == out).to(torch.int8), 0)
            assert torch.equal(arg[0], first)


@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("K", [1, 4, 17])
@pytest.mark.parametrize("graph", ["mixed", "hub_columns_exact", "one_row"])
def test_backward_matches_the_oracle_bit_for_bit(reduce, K, graph):
    (rowptr, col), deg = next((g[1], g[2]) for g in GRAPHS if g[0] == graph)
    if reduce == "mean":  # exact only on power-of-two row degrees: rebuild the graph with those
        deg = pow2_degrees(rowptr.diff().numpy())
        rowptr, col = csr_with_degrees(deg, int(col.max()) + 1, seed=K)
    N = int(col.max()) + 1
    value, mat, grad = int_data(rowptr, N, K, seed=10 + K)
    assert_exact_preconditions(rowptr, col, value, mat, grad, mean_backward=reduce == "mean")
    row = torch.repeat_interleave(torch.arange(rowptr.numel() - 1), rowptr.diff()).numpy()
    args = rowptr.numpy(), col.numpy()
    gv, gm = spmm_backward_ref(reduce, rowptr, col, value, mat, grad)
    if reduce in ("sum", "mean"):
        want_gv = oracle.spmm_value_bw(reduce, row, *args, mat.numpy(), grad.numpy())
        want_gm = oracle.spmm_mat_bw(reduce, row, *args, value.numpy(), grad.numpy(), N)
        want_gm_unweighted = oracle.spmm_mat_bw(reduce, row, *args, None, grad.numpy(), N)
        assert np.array_equal(spmm_backward_ref(reduce, rowptr, col, None, mat, grad)[1].numpy(), want_gm_unweighted)
    else:
        _, arg = oracle.spmm(reduce, *args, value.numpy(), mat.numpy())
        want_gv, want_gm = oracle.spmm_minmax_bw(col.numpy(), value.numpy(), mat.numpy(), grad.numpy(), arg)
        assert torch.equal(spmm_ref(reduce, rowptr, col, value, mat)[1], torch.from_numpy(arg))
    assert np.array_equal(gv.numpy(), want_gv)
    assert np.array_equal(gm.numpy(), want_gm)


@pytest.mark.parametrize("reduce", REDUCES)
def test_specials_follow_the_oracle(reduce):
    """inf and NaN in the dense operand: sums give NaN / +-inf where the oracle does, min / max never pick
    NaN, an infinite product wins only when it improves on the +-FLT_MAX init, and a row without a winner keeps
    the sentinel (and the init, or 0 when it is empty)."""
    rowptr, col = csr_with_degrees([0, 1, 2, 3, 40, 200, 5, 1], 30, seed=5)
    value, mat, _ = int_data(rowptr, 30, 16, seed=6)
    mat = with_specials(mat, seed=7, frac=0.03)
    mat[3, :] = float("nan")  # rows made of NaN only: a row reading nothing else has no winner
    col[rowptr[1]] = 3
    assert_exact_preconditions(rowptr, col, value, mat)
    out, arg = spmm_ref(reduce, rowptr, col, value, mat)
    want, want_arg = oracle.spmm(reduce, rowptr.numpy(), col.numpy(), value.numpy(), mat.numpy())
    assert np.array_equal(out.numpy(), want, equal_nan=True)
    assert bool(torch.isnan(out).any() or torch.isinf(out).any()) or reduce in ("min", "max")
    if arg is not None:
        assert np.array_equal(arg.numpy(), want_arg)
        assert bool((arg[1] == col.numel()).all())  # the NaN-only row: no winner, sentinel, the init
        assert bool((out[1].abs() == FLT_MAX).all()) and bool((out[0] == 0).all())  # row 0 is empty


def test_readme_kat(kats):
    k = kats["spmm"]
    row, col = torch.tensor(k["index"], dtype=torch.int64)
    rowptr = torch.zeros(k["m"] + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(row, minlength=k["m"]), 0)
    out, _ = spmm_ref("sum", rowptr, col, torch.tensor(k["value"], dtype=torch.float32),
                      torch.tensor(k["matrix"], dtype=torch.float32))
    assert out.tolist() == k["out"]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_outputs_round_once(dtype):
    """Sums past the half types' exact range round once, to nearest even, from the exact value; fp16 overflows
    to +-inf.  (The fp32 oracle, rounded on its own, must give the same bits: its sums are exact.)"""
    rowptr, col = csr_with_degrees([1, 7, 300, 300, 1000], 4, seed=8)
    value = integers(col.numel(), 20, 30, torch.float32, seed=9)
    mat = integers((4, 8), -40, 40, dtype, seed=10)
    mat[:, 0] = 40
    assert_exact_preconditions(rowptr, col, value, mat)
    out, _ = spmm_ref("sum", rowptr, col, value, mat)
    want, _ = oracle.spmm("sum", rowptr.numpy(), col.numpy(), value.numpy(), mat.float().numpy())
    assert torch.equal(out, torch.from_numpy(want).to(dtype))
    assert out.dtype == dtype and bool((out.float().abs() > 2048).any())
    if dtype == torch.float16:
        assert bool(torch.isinf(out).any())


def test_preconditions_catch_an_inexact_test():
    rowptr, col = csr_with_degrees([4096], 2, seed=1)
    mat = torch.full((2, 4), 8.0)
    value = torch.full((4096,), 512.0)
    with pytest.raises(AssertionError):
        assert_exact_preconditions(rowptr, col, value, mat)  # 4096 * 512 * 8 = 2^24
    assert_exact_preconditions(rowptr, col, value / 2, mat)
    with pytest.raises(AssertionError):
        assert_exact_preconditions(rowptr, col, value + 0.5, mat)
    rowptr, col = csr_with_degrees([3, 4], 2, seed=1)
    with pytest.raises(AssertionError):
        assert_exact_preconditions(rowptr, col, None, mat[:, :1], torch.ones(2, 1), mean_backward=True)
    assert EXACT == 2.0 ** 24
