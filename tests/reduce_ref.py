"""Exact reference for the grouped reductions (segment_csr, scatter, coalesce, the compress step of
spspmm), in plain torch on the CPU with float64 / int64 inside.

Independent of the package and of oracle/ (tests/test_reduce_ref.py pins it to the oracle and to the
framework's reducers).  The rule, a function of a group's contents alone:

  sum    float64 / int64 accumulation, rounded once to the output dtype; IEEE for non-finite values
         (+inf and -inf in one group give NaN)
  mean   that exact sum, then ONE division in the kernels' accumulator type — fp32 for fp32 / fp16 /
         bf16 values, fp64 for fp64, floor division for integers — then one rounding for half types
  min / max   NaN when the group holds a NaN in that output column, whatever its position; else the
         extreme (infinities included)
  a group without entries gives 0.

With integer-valued finite data whose per-group sum |term| stays below 2^24 every fp32 partial sum is
exact in ANY order, so a kernel has to match this reference bit for bit: `assert_exact` checks that
bound on the data a test generated.  No generator produces -0.0 (which zero min / max return on a
+0 / -0 tie is not pinned).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from exact_ref import integers, with_specials

EXACT = float(1 << 24)
HALF_TYPES = (torch.float16, torch.bfloat16)
FLOAT_TYPES = (torch.float32, torch.float64) + HALF_TYPES
INT_TYPES = (torch.int32, torch.int64)
HALF_SUM_MAX = {torch.float16: 2048.0, torch.bfloat16: 256.0}  # every integer up to here is representable
REDUCES = ("sum", "mean", "min", "max")
_OP = {"add": "sum", "sum": "sum", "mean": "mean", "min": "min", "max": "max"}


# ---------------------------------------------------------------------------------------------
# the reduction itself
# ---------------------------------------------------------------------------------------------

def _wide(x: torch.Tensor) -> torch.Tensor:
    """[n, D] in float64 (floating dtypes) or int64 (integers)."""
    x = x.detach().cpu()
    x = x.reshape(x.shape[0], -1)
    return x.to(torch.float64 if x.dtype.is_floating_point else torch.int64)


def group_reduce(src: torch.Tensor, group: torch.Tensor, ngroups: int, reduce: str) -> torch.Tensor:
    """out[g] = reduce of src[i] over group[i] == g, along dim 0; out has src's dtype and trailing
    dims.  Entries whose group lies outside [0, ngroups) are ignored."""
    reduce = _OP[reduce]
    dtype, tail = src.dtype, tuple(src.shape[1:])
    v = _wide(src)
    group = group.cpu().to(torch.int64)
    keep = (group >= 0) & (group < ngroups)
    v, group = v[keep], group[keep]
    D = v.shape[1]
    is_float = dtype.is_floating_point
    count = torch.zeros(ngroups, dtype=torch.int64).index_add_(0, group, torch.ones_like(group))
    if reduce in ("sum", "mean"):
        acc = torch.zeros(ngroups, D, dtype=v.dtype).index_add_(0, group, v)
        if reduce == "mean":
            c = count.clamp(min=1)[:, None]
            if not is_float:
                acc = torch.div(acc, c, rounding_mode="floor")
            elif dtype == torch.float64:
                acc = acc / c.to(torch.float64)
            else:  # one fp32 division of the exactly representable sum
                acc = (acc.to(torch.float32) / c.to(torch.float32)).to(torch.float64)
        out = acc
    else:
        mn = reduce == "min"
        idx = group[:, None].expand(-1, D)
        if is_float:
            nan = torch.isnan(v)
            far = float("inf") if mn else float("-inf")
            clean = torch.where(nan, torch.full_like(v, far), v)
            out = torch.full((ngroups, D), far, dtype=torch.float64)
            out.scatter_reduce_(0, idx, clean, "amin" if mn else "amax", include_self=True)
            has_nan = torch.zeros(ngroups, D, dtype=torch.int64).index_add_(0, group, nan.to(torch.int64)) > 0
            out[has_nan] = float("nan")
        else:
            far = torch.iinfo(torch.int64).max if mn else torch.iinfo(torch.int64).min
            out = torch.full((ngroups, D), far, dtype=torch.int64)
            out.scatter_reduce_(0, idx, v, "amin" if mn else "amax", include_self=True)
        out[count == 0] = 0
    return out.to(dtype).reshape((ngroups,) + tail)


def groups_of(indptr: torch.Tensor) -> torch.Tensor:
    indptr = indptr.cpu().to(torch.int64)
    return torch.repeat_interleave(torch.arange(indptr.numel() - 1), indptr.diff())


def segment_ref(src: torch.Tensor, indptr: torch.Tensor, reduce: str, perm: Optional[torch.Tensor] = None):
    """segment_csr along dim 0: out[s] = reduce of src[perm][indptr[s]:indptr[s + 1]]."""
    indptr = indptr.cpu().to(torch.int64)
    src = src.detach().cpu()
    if perm is not None:
        src = src[perm.cpu().to(torch.int64)]
    lo, hi = int(indptr[0]), int(indptr[-1])
    return group_reduce(src[lo:hi], groups_of(indptr), indptr.numel() - 1, reduce)


def scatter_ref(src: torch.Tensor, index: torch.Tensor, dim_size: int, reduce: str):
    """scatter along dim 0: untouched rows 0, indices outside [0, dim_size) ignored."""
    return group_reduce(src, index, dim_size, reduce)


def coalesce_ref(index: torch.Tensor, value: Optional[torch.Tensor], m: int, n: int, op: str = "add"):
    """(index int64[2, nnz'] in row-major order without duplicates, value' | None)."""
    index = index.cpu().to(torch.int64)
    assert int(index[0].min()) >= 0 and int(index[0].max()) < m and int(index[1].min()) >= 0 and int(index[1].max()) < n
    key = index[0] * n + index[1]
    uniq, inverse = torch.unique(key, sorted=True, return_inverse=True)
    out_index = torch.stack([uniq // n, uniq % n])
    if value is None:
        return out_index, None
    return out_index, group_reduce(value, inverse, uniq.numel(), op)


def spspmm_terms(indexA, valueA, indexB, valueB, m: int, k: int, n: int):
    """(key = i * n + j, product a * b in float64 / int64) of every partial product of A @ B."""
    indexA, indexB = indexA.cpu().to(torch.int64), indexB.cpu().to(torch.int64)
    a, b = _wide(valueA)[:, 0], _wide(valueB)[:, 0]
    orderB = torch.argsort(indexB[0], stable=True)
    rowB, colB, b = indexB[0][orderB], indexB[1][orderB], b[orderB]
    rowptrB = torch.zeros(k + 1, dtype=torch.int64)
    rowptrB[1:] = torch.cumsum(torch.bincount(rowB, minlength=k), 0)
    counts = rowptrB[indexA[1] + 1] - rowptrB[indexA[1]]
    owner = torch.repeat_interleave(torch.arange(indexA.shape[1]), counts)
    start = torch.cumsum(counts, 0) - counts
    within = torch.arange(owner.numel()) - start[owner]
    e = rowptrB[indexA[1][owner]] + within
    return indexA[0][owner] * n + colB[e], a[owner] * b[e]


def spspmm_ref(indexA, valueA, indexB, valueB, m: int, k: int, n: int):
    """Structural product of two coalesced COO matrices: every (i, j) reached by a product is an
    entry, also where its terms cancel to 0.  Returns (index int64[2, nnz'], value' in valueA's dtype)."""
    key, prod = spspmm_terms(indexA, valueA, indexB, valueB, m, k, n)
    uniq, inverse = torch.unique(key, sorted=True, return_inverse=True)
    total = torch.zeros(uniq.numel(), dtype=prod.dtype).index_add_(0, inverse, prod)
    return torch.stack([uniq // n, uniq % n]), total.to(valueA.dtype)


# ---------------------------------------------------------------------------------------------
# the precondition of bit-exactness
# ---------------------------------------------------------------------------------------------

def assert_exact(terms: torch.Tensor, group: torch.Tensor, ngroups: int, dtype=None, sums: bool = True,
                 products: bool = False):
    """The data makes every summation order give the same bits: all finite terms are integers and,
    for the additive reductions (`sums`), every group's sum |term| is below 2^24 where the kernels
    accumulate in fp32 (fp32 / fp16 / bf16 values) and 2^53 in fp64, |sum| <= 2048 (fp16) / 256
    (bf16) so that the result is representable, and integer sums stay inside their type.
    `dtype`: the values' dtype where `terms` are products computed wider (spspmm; `products` then
    allows -0.0, which 0 * -3 gives and which no input may hold)."""
    dtype = dtype or terms.dtype
    v = _wide(terms)
    group = group.cpu().to(torch.int64)
    keep = (group >= 0) & (group < ngroups)
    v, group = v[keep], group[keep]
    if dtype.is_floating_point:
        fin = torch.isfinite(v)
        assert torch.equal(v[fin], v[fin].round()), "non-integer values"
        assert products or not bool(((v == 0) & torch.signbit(v)).any()), "-0.0 in the data"
        v = torch.where(fin, v, torch.zeros_like(v))
    if not sums:
        return
    D = v.shape[1]
    mag = torch.zeros(ngroups, D, dtype=torch.float64).index_add_(0, group, v.abs().to(torch.float64))
    top = float(mag.max()) if mag.numel() else 0.0
    if dtype.is_floating_point:
        bound = float(1 << 53) if dtype == torch.float64 else EXACT
        assert top < bound, f"a group's sum |term| reaches {top} >= {bound}"
        if dtype in HALF_TYPES:
            tot = torch.zeros(ngroups, D, dtype=torch.float64).index_add_(0, group, v).abs()
            t = float(tot.max()) if tot.numel() else 0.0
            assert t <= HALF_SUM_MAX[dtype], f"|sum| reaches {t}: not every such integer is a {dtype}"
    else:
        assert top <= float(torch.iinfo(dtype).max), f"integer sums may leave {dtype}: {top}"


# ---------------------------------------------------------------------------------------------
# group-length shapes
# ---------------------------------------------------------------------------------------------

def _power_law(ngroups: int, total: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    w = (1.0 / np.arange(1, ngroups + 1)) ** 1.1
    rng.shuffle(w)
    deg = np.floor(w / w.sum() * total).astype(np.int64)
    deg[int(np.argmax(deg))] += total - int(deg.sum())
    return deg


def group_lengths(shape: str, total: Optional[int] = None, seed: int = 0) -> np.ndarray:
    """The group-length shapes every test shares.  `total` sizes the power-law mix."""
    if shape == "edges":  # empty groups at the start, in the middle and at the end
        return np.array([0, 0, 1, 2, 63, 64, 65, 0, 127, 128, 129, 0, 0, 2047, 2048, 2049, 1, 0, 0], np.int64)
    if shape == "long":
        return np.array([3, 100_000, 0, 5], np.int64)
    if shape == "one":
        return np.array([total or 5000], np.int64)
    if shape == "powerlaw":
        return _power_law(max(8, (total or 60_000) // 20), total or 60_000, seed)
    if shape == "short":  # runs of 1 .. 4, for the routes that serve short runs
        rng = np.random.default_rng(seed)
        deg = rng.integers(1, 5, max(1, (total or 60_000) // 2))
        return deg[np.cumsum(deg) <= (total or 60_000)].astype(np.int64)
    raise ValueError(shape)


SHAPES = ("edges", "long", "one", "powerlaw")
# deliberate groups appended (before the trailing empty ones) by the modes below
_SPECIAL_GROUPS = (("nan_first", 5), ("nan_last", 7), ("nan_at_64_of_200", 200), ("all_nan", 4), ("both_inf", 6))
_EXTREME_GROUPS = (("only_min", 1), ("only_max", 1), ("all_max", 5), ("all_min", 5), ("min_and_max", 130))


@dataclass
class Case:
    """Grouped data: values[i] belongs to group[i]; groups are contiguous (indptr) in this order."""
    values: torch.Tensor
    indptr: torch.Tensor
    group: torch.Tensor
    mode: str
    marks: Dict[str, int] = field(default_factory=dict)  # name of a deliberate group -> its id

    @property
    def ngroups(self) -> int:
        return self.indptr.numel() - 1

    def check(self, reduces: Sequence[str] = REDUCES):
        """assert_exact on this data for the reductions a test is going to run."""
        assert_exact(self.values, self.group, self.ngroups, sums=any(_OP[r] in ("sum", "mean") for r in reduces))


def _with_extra(lengths: np.ndarray, extra) -> Tuple[np.ndarray, Dict[str, int]]:
    lengths = np.asarray(lengths, np.int64)
    cut = lengths.size
    while cut > 0 and lengths[cut - 1] == 0:
        cut -= 1
    marks = {name: cut + i for i, (name, _) in enumerate(extra)}
    return np.concatenate([lengths[:cut], np.array([ln for _, ln in extra], np.int64), lengths[cut:]]), marks


def make_case(lengths, mode: str, dtype, tail: Tuple[int, ...] = (), seed: int = 0) -> Case:
    """Values of `mode` for groups of the given lengths.

    int       integers in [-3, 3] (many ties); the first entry of every group of two or more is -4,
              its only minimum, and the last is 4, its only maximum, so a run cut short at either
              end changes sum, min or max.  Half-width dtypes get the interior in (v, -v) pairs, which
              keeps |sum| of a 100 000-entry group within what bf16 holds exactly.
    specials  int, plus about 0.2 % each of +inf, -inf and NaN, plus the deliberate groups of
              _SPECIAL_GROUPS (in column min(1, D - 1) of a trailing dim; the other columns stay finite)
    extremes  (integers, min / max only) int, plus about 1 % each of the type's minimum and maximum and
              the deliberate groups of _EXTREME_GROUPS."""
    marks: Dict[str, int] = {}
    if mode == "specials":
        assert dtype.is_floating_point
        lengths, marks = _with_extra(lengths, _SPECIAL_GROUPS)
    elif mode == "extremes":
        assert not dtype.is_floating_point
        lengths, marks = _with_extra(lengths, _EXTREME_GROUPS)
    elif mode != "int":
        raise ValueError(mode)
    lengths = torch.as_tensor(np.asarray(lengths, np.int64))
    indptr = torch.zeros(lengths.numel() + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(lengths, 0)
    n = int(indptr[-1])
    group = groups_of(indptr)
    v = integers((n,) + tuple(tail), -3, 3, torch.float64, seed)
    if dtype in HALF_TYPES and n > 1:
        v[1::2] = -v[0:n - (n % 2):2]
    v = v + 0.0  # -0.0 from the negation above becomes +0.0
    many = lengths >= 2
    v[indptr[:-1][many]] = -4.0
    v[indptr[1:][many] - 1] = 4.0
    flat = v.reshape(n, -1)
    col = min(1, flat.shape[1] - 1)
    if mode == "specials":
        flat = with_specials(flat, seed + 7)
        for name in marks:  # the deliberate groups start finite
            b, e = int(indptr[marks[name]]), int(indptr[marks[name] + 1])
            flat[b:e] = torch.nan_to_num(flat[b:e], nan=1.0, posinf=2.0, neginf=-2.0)
        span = {name: (int(indptr[g]), int(indptr[g + 1])) for name, g in marks.items()}
        flat[span["nan_first"][0], col] = float("nan")
        flat[span["nan_last"][1] - 1, col] = float("nan")
        flat[span["nan_at_64_of_200"][0] + 64, col] = float("nan")
        flat[span["all_nan"][0]:span["all_nan"][1], col] = float("nan")
        flat[span["both_inf"][0] + 1, col] = float("inf")
        flat[span["both_inf"][1] - 2, col] = float("-inf")
        values = flat.reshape(v.shape).to(dtype)
    elif mode == "extremes":
        lo, hi = torch.iinfo(dtype).min, torch.iinfo(dtype).max
        w = flat.to(torch.int64)
        pick = torch.rand(w.shape, generator=torch.Generator().manual_seed(seed + 7))
        w[pick < 0.01] = lo
        w[(pick >= 0.01) & (pick < 0.02)] = hi
        span = {name: (int(indptr[g]), int(indptr[g + 1])) for name, g in marks.items()}
        w[span["only_min"][0]] = lo
        w[span["only_max"][0]] = hi
        w[span["all_max"][0]:span["all_max"][1]] = hi
        w[span["all_min"][0]:span["all_min"][1]] = lo
        b, e = span["min_and_max"]
        w[b:e] = torch.clamp(w[b:e], -4, 4)
        w[b + 64, col] = lo
        w[e - 1, col] = hi
        values = w.reshape(v.shape).to(dtype)
    else:
        values = flat.reshape(v.shape).to(dtype)
    return Case(values, indptr, group, mode, marks)


def shuffled(case: Case, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(values, group) of the case in a random entry order (scatter and unsorted coalesce inputs)."""
    p = torch.randperm(case.group.numel(), generator=torch.Generator().manual_seed(seed + 13))
    return case.values[p], case.group[p]


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal shape, dtype and bits up to the payload of a NaN: NaNs have to sit at the same places."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])
