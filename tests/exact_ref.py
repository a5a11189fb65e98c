"""Exact SpMM reference on integer-valued data, in plain torch on the CPU (float64 / int64).

With small integers every product is an integer and every partial sum stays below 2^24, so fp32
arithmetic is exact in ANY summation order: a kernel must then match this reference bit for bit,
and a single dropped, duplicated or misrouted edge fails at any row length (a tolerance relative to
sum |w * b| cannot see one edge of a 10^5-entry row).  `assert_exact_preconditions` checks that
bound on the data a test generated, so a later edit cannot quietly make a test inexact.

Rules (oracle/spmm_oracle.c, upstream pytorch_sparse): sum / mean accumulate w_e * mat[col[e]];
mean divides by max(deg, 1); min / max start at +-FLT_MAX and take an edge only on a strict
improvement (NaN never wins), ties go to the first edge; a row without a winner gives the sentinel
arg = nnz and out = 0 when it is empty, +-FLT_MAX (the untouched init) when it is not.  The expected value is computed in float64 and rounded once to the output dtype
(round to nearest even); mean rounds the quotient to fp32 first, as the kernels divide in fp32.

The mean backward folds a rounded 1 / deg into the weights: it is exact only where every non-empty
row degree is a power of two (terms are then multiples of 2^-j and each sum must stay below
2^(24 - j)); `assert_exact_preconditions(..., mean_backward=True)` checks that too.

Independent of the package and of the oracle: tests/test_exact_ref.py pins the two to each other.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

FLT_MAX = float(np.finfo(np.float32).max)
EXACT = float(1 << 24)
HALF_TYPES = (torch.float16, torch.bfloat16)


# ---------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------

def integers(shape, lo: int, hi: int, dtype=torch.float32, seed: int = 0) -> torch.Tensor:
    """Integer values in [lo, hi] as `dtype` (exact in fp32, bf16 and fp16 for |x| <= 256)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape) if not isinstance(shape, int) else (shape,), generator=g).to(dtype)


def int_data(rowptr: torch.Tensor, N: int, K: int, dtype=torch.float32, value_dtype=torch.float32,
             seed: int = 0, with_value: bool = True, vmax: int = 3, mmax: int = 8, gmax: int = 8):
    """(value, mat, grad_out) of the `int` mode: value in [-vmax, vmax], mat and grad in [-mmax, mmax] /
    [-gmax, gmax] — few distinct products, so min / max see many ties."""
    M, nnz = rowptr.numel() - 1, int(rowptr[-1])
    value = integers(nnz, -vmax, vmax, value_dtype, seed) if with_value else None
    mat = integers((N, K), -mmax, mmax, dtype, seed + 1)
    grad = integers((M, K), -gmax, gmax, dtype, seed + 2)
    return value, mat, grad


def with_specials(mat: torch.Tensor, seed: int = 0, frac: float = 0.002) -> torch.Tensor:
    """A copy of `mat` with a few +inf, -inf and NaN entries (the `specials` mode); the finite entries
    stay small integers, so no finite sum overflows in fp32 or fp64."""
    g = torch.Generator().manual_seed(seed)
    out = mat.clone()
    pick = torch.rand(mat.shape, generator=g)
    out[pick < frac] = float("inf")
    out[(pick >= frac) & (pick < 2 * frac)] = float("-inf")
    out[(pick >= 2 * frac) & (pick < 3 * frac)] = float("nan")
    return out


def csr_with_degrees(deg: Sequence[int], N: int, seed: int = 0, col_skew: float = 1.0):
    """(rowptr, col) int64 with the given row degrees; columns uniform in [0, N) (col_skew > 1
    crowds them towards column 0, for hub columns), in random order inside a row (duplicates allowed)."""
    deg = torch.as_tensor(np.asarray(deg, np.int64))
    rowptr = torch.zeros(deg.numel() + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    nnz = int(rowptr[-1])
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(nnz, generator=g, dtype=torch.float64)
    col = torch.clamp((u ** col_skew * N).to(torch.int64), max=N - 1)
    return rowptr, col


def csr_with_col_degrees(col_deg: Sequence[int], M: int, seed: int = 0):
    """(rowptr, col) int64 of an M-row CSR whose columns hold the given numbers of entries (the
    row degrees of the transpose, for the passes over the CSC view); rows uniform in [0, M)."""
    col_deg = torch.as_tensor(np.asarray(col_deg, np.int64))
    N = col_deg.numel()
    col = torch.repeat_interleave(torch.arange(N), col_deg)
    g = torch.Generator().manual_seed(seed)
    row = torch.randint(0, M, (col.numel(),), generator=g)
    order = torch.argsort(row * N + col, stable=True)
    row, col = row[order], col[order]
    rowptr = torch.zeros(M + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(row, minlength=M), 0)
    return rowptr, col


def pow2_degrees(deg: Sequence[int]) -> np.ndarray:
    """Each degree rounded down to a power of two (0 stays 0): graphs whose mean backward is exact."""
    d = np.asarray(deg, np.int64)
    return np.where(d > 0, 1 << np.floor(np.log2(np.maximum(d, 1))).astype(np.int64), 0)


# ---------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------

def _rows(rowptr: torch.Tensor) -> torch.Tensor:
    rowptr = rowptr.cpu().to(torch.int64)
    return torch.repeat_interleave(torch.arange(rowptr.numel() - 1), rowptr.diff())


def _f64(x: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if x is None else x.detach().cpu().to(torch.float64)


def _weights(value, nnz: int) -> torch.Tensor:
    return torch.ones(nnz, dtype=torch.float64) if value is None else _f64(value)


def round_to(x64: torch.Tensor, dtype) -> torch.Tensor:
    """One rounding of float64 to `dtype` (nearest even, overflow to +-inf)."""
    return x64.to(dtype)


def spmm_ref(reduce: str, rowptr, col, value, mat, out_dtype=None):
    """(out in out_dtype (default mat's dtype), arg_out int64 [M, K] or None) of reduce-SpMM."""
    rowptr, col = rowptr.cpu().to(torch.int64), col.cpu().to(torch.int64)
    out_dtype = out_dtype or mat.dtype
    M, (N, K), nnz = rowptr.numel() - 1, mat.shape, col.numel()
    rows = _rows(rowptr)
    p = _weights(value, nnz)[:, None] * _f64(mat)[col]  # [nnz, K] products, exact for the data here
    deg = rowptr.diff()
    if reduce in ("sum", "mean", "add"):
        acc = torch.zeros(M, K, dtype=torch.float64).index_add_(0, rows, p)
        if reduce == "mean":
            acc = (acc / deg.clamp(min=1).to(torch.float64)[:, None]).to(torch.float32).to(torch.float64)
        return round_to(acc, out_dtype), None
    if reduce not in ("min", "max"):
        raise ValueError(reduce)
    mn = reduce == "min"
    valid = (p < FLT_MAX) if mn else (p > -FLT_MAX)  # strict improvement over the init; NaN never wins
    key = torch.where(valid, p, torch.full_like(p, float("inf") if mn else float("-inf")))
    idx = rows[:, None].expand(nnz, K)
    fill = float("inf") if mn else float("-inf")
    best = torch.full((M, K), fill, dtype=torch.float64).scatter_reduce_(0, idx, key, "amin" if mn else "amax")
    hit = valid & (p == best[rows])  # edges reaching the row's extreme
    e = torch.arange(nnz)[:, None].expand(nnz, K)
    arg = torch.full((M, K), nnz, dtype=torch.int64).scatter_reduce_(0, idx, torch.where(hit, e, nnz), "amin")
    # no winner: an empty row gives 0, a non-empty one keeps the init +-FLT_MAX (arg_out = nnz either way)
    lost = torch.where(deg > 0, FLT_MAX if mn else -FLT_MAX, 0.0).to(torch.float64)[:, None].expand(M, K)
    out = torch.where(arg < nnz, best, lost)
    return round_to(out, out_dtype), arg


def spmm_backward_ref(reduce: str, rowptr, col, value, mat, grad, arg=None, out_dtype=None,
                      value_dtype=torch.float32):
    """(grad_value [nnz] in value_dtype, grad_mat [N, K] in out_dtype (default grad's dtype)).  min / max
    route through `arg` (spmm_ref's arg_out; computed when not given)."""
    rowptr, col = rowptr.cpu().to(torch.int64), col.cpu().to(torch.int64)
    out_dtype = out_dtype or grad.dtype
    M, (N, K), nnz = rowptr.numel() - 1, mat.shape, col.numel()
    rows = _rows(rowptr)
    w, b, g = _weights(value, nnz), _f64(mat), _f64(grad)
    if reduce in ("sum", "mean", "add"):
        scale = torch.ones(nnz, dtype=torch.float64)
        if reduce == "mean":
            scale = 1.0 / rowptr.diff().clamp(min=1).to(torch.float64)[rows]
        gv = (b[col] * g[rows]).sum(1) * scale
        gm = torch.zeros(N, K, dtype=torch.float64).index_add_(0, col, (w * scale)[:, None] * g[rows])
        return round_to(gv, value_dtype), round_to(gm, out_dtype)
    if arg is None:
        arg = spmm_ref(reduce, rowptr, col, value, mat)[1]
    live = arg < nnz
    i, k = live.nonzero(as_tuple=True)
    e = arg[live]
    gik = g[i, k]
    gv = torch.zeros(nnz, dtype=torch.float64).index_add_(0, e, b[col[e], k] * gik)
    gm = torch.zeros(N * K, dtype=torch.float64).index_add_(0, col[e] * K + k, w[e] * gik).view(N, K)
    return round_to(gv, value_dtype), round_to(gm, out_dtype)


def _top(x: torch.Tensor) -> float:
    return float(x.max()) if x.numel() else 0.0


def assert_exact_preconditions(rowptr, col, value, mat, grad=None, mean_backward: bool = False):
    """Every fp32 sum the forward (and, with `grad`, the backward) adds stays exact in any order:
    all inputs are integers (finite ones; inf / NaN entries of the specials mode aside), and the
    largest sum |term| of an output element is below 2^24.  mean_backward: non-empty row degrees
    are powers of two 2^j_r and sum |term| * 2^j stays below 2^24 (j = the largest j_r)."""
    rowptr, col = rowptr.cpu().to(torch.int64), col.cpu().to(torch.int64)
    M, (N, K), nnz = rowptr.numel() - 1, mat.shape, col.numel()
    rows = _rows(rowptr)
    w, b = _weights(value, nnz), _f64(mat)
    for name, x in (("value", w), ("mat", b), ("grad", _f64(grad) if grad is not None else None)):
        if x is None:
            continue
        fin = x[torch.isfinite(x)]
        assert torch.equal(fin, fin.round()), f"{name} holds non-integers"
    bf = torch.where(torch.isfinite(b), b, torch.zeros_like(b)).abs()
    fwd = torch.zeros(M, K, dtype=torch.float64).index_add_(0, rows, w.abs()[:, None] * bf[col])
    assert _top(fwd) < EXACT, f"forward sums reach {_top(fwd)} >= 2^24"
    if grad is None:
        return
    g = _f64(grad).abs()
    gv = (bf[col] * g[rows]).sum(1)  # grad_value: an integer sum per edge (mean scales it once afterwards)
    wt = w.abs()
    unit = 1.0
    if mean_backward:  # grad_mat adds w * g / deg(row): multiples of 2^-j, exact below 2^(24 - j)
        deg = rowptr.diff()
        nz = deg[deg > 0]
        assert bool(((nz & (nz - 1)) == 0).all()), "mean backward needs power-of-two row degrees"
        unit = float(nz.max()) if nz.numel() else 1.0
        wt = wt / deg.clamp(min=1).to(torch.float64)[rows]
    gm = torch.zeros(N, K, dtype=torch.float64).index_add_(0, col, wt[:, None] * g[rows])
    assert _top(gv) < EXACT, f"grad_value sums reach {_top(gv)} >= 2^24"
    assert _top(gm) * unit < EXACT, f"grad_mat sums reach {_top(gm)} * {unit} >= 2^24"
