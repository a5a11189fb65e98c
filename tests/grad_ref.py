"""Reference for the "value in, value out" ops and their gradients: float64 on the CPU, plain torch
indexing (`index_put_(accumulate=True)`, `sum`, division, dense `@`), and torch's OWN autograd for the
gradient of `(out * coef).sum()`.  It shares no code with the package.

Every function takes the values in their dtype and returns `(..., out, grads)`: `out` is the float64
result rounded once to that dtype, `grads` holds d/d(operand) of `(out64 * coef).sum()` rounded the
same way, one per operand (None for an operand without values).  Half types are rounded through
fp32, as kernels that accumulate in fp32 round.

A matrix is never built m x n: the keys row * n + col are ranked (`torch.unique`) and the "dense"
matrix is the vector of the distinct keys, so an index past 2^32 costs nothing.  Only the sparse
product builds real dense operands (`@`), on the small shapes its tests use.

Exactness.  Values are integers in [-3, 3], coefficients and dense operands in [-8, 8]; with every
group's sum |term| below 2^24 (fp32) / a result within HALF_SUM_MAX (half types) each sum is exact
in any order, forward and backward (`check_values`, `check_sums` on top of reduce_ref.assert_exact).
A mean contributes ONE division per element — the fp64 quotient of two such integers rounded to
fp32 is the correctly rounded fp32 quotient (53 >= 2 * 24 + 2 bits) — so where a mean's gradient
is added up again (a repeated selection) every divisor has to be a power of two
(`check_pow2`; exact_ref.pow2_degrees makes such run lengths).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from exact_ref import integers
from reduce_ref import HALF_TYPES, assert_exact

VALUE_MAX, COEF_MAX = 3, 8


# ---------------------------------------------------------------------------------------------
# data and preconditions
# ---------------------------------------------------------------------------------------------

def values(n: int, dtype, tail: Tuple[int, ...] = (), seed: int = 0) -> torch.Tensor:
    """Integers in [-3, 3] as `dtype`; half types get (v, -v) pairs so that no run's sum leaves the
    integers the type holds exactly.  No -0.0."""
    v = integers((n,) + tuple(tail), -VALUE_MAX, VALUE_MAX, torch.float64, seed)
    if dtype in HALF_TYPES and n > 1:
        v[1::2] = -v[0:n - (n % 2):2]
    return (v + 0.0).to(dtype)


def coefs(shape, seed: int = 0) -> torch.Tensor:
    """float64 integers in [-8, 8]: the weights of the scalar loss."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return integers(shape, -COEF_MAX, COEF_MAX, torch.float64, seed + 1000)


def check_values(x: Optional[torch.Tensor], bound: int) -> None:
    """x holds integers of magnitude <= bound, and no -0.0."""
    if x is None:
        return
    x = x.detach().cpu().to(torch.float64)
    assert bool(torch.isfinite(x).all()), "non-finite data"
    assert torch.equal(x, x.round()), "non-integer data"
    assert x.numel() == 0 or float(x.abs().max()) <= bound, f"|x| above {bound}"
    assert not bool(((x == 0) & torch.signbit(x)).any()), "-0.0 in the data"


def check_sums(terms: torch.Tensor, group: torch.Tensor, ngroups: int, dtype) -> None:
    """The sums of `terms` (float64, computed wide) over `group` are exact in `dtype` in any order."""
    assert_exact(terms.detach().cpu().to(torch.float64), group, ngroups, dtype=dtype, products=True)


def check_pow2(counts: torch.Tensor) -> None:
    """Every non-zero divisor is a power of two: quotients by them add up exactly."""
    c = counts.cpu().to(torch.int64)
    c = c[c > 0]
    assert bool(((c & (c - 1)) == 0).all()), "a mean that is added up again needs power-of-two run lengths"


# ---------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------

def _leaf(v: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if v is None else v.detach().cpu().to(torch.float64).clone().requires_grad_(True)


def _round(x64: torch.Tensor, dtype) -> torch.Tensor:
    x64 = x64.detach()
    return x64.to(torch.float32).to(dtype) if dtype in HALF_TYPES else x64.to(dtype)


def _finish(out64: torch.Tensor, coef: Optional[torch.Tensor], leaves: Sequence[Optional[torch.Tensor]], dtypes):
    """(out rounded to dtypes[0], [d (out64 * coef).sum() / d leaf, rounded to that leaf's dtype])."""
    coef = torch.ones_like(out64) if coef is None else coef.cpu().to(torch.float64)
    assert coef.shape == out64.shape, f"coef {tuple(coef.shape)} for a result {tuple(out64.shape)}"
    live = [x for x in leaves if x is not None]
    got = iter(torch.autograd.grad((out64 * coef).sum(), live, allow_unused=True)) if out64.requires_grad else iter(())
    grads: List[Optional[torch.Tensor]] = []
    for x, dt in zip(leaves, dtypes):
        if x is None:
            grads.append(None)
            continue
        g = next(got, None)
        grads.append(_round(torch.zeros_like(x) if g is None else g, dt))
    return _round(out64, dtypes[0]), grads


def _keys(index: torch.Tensor, n: int) -> torch.Tensor:
    index = index.cpu().to(torch.int64)
    return index[0] * n + index[1]


def _counts(inverse: torch.Tensor, size: int) -> torch.Tensor:
    return torch.zeros(size, dtype=torch.float64).index_put_((inverse,), torch.ones(inverse.numel(), dtype=torch.float64),
                                                             accumulate=True)


def _accumulate(v: torch.Tensor, inverse: torch.Tensor, size: int, mean: bool) -> torch.Tensor:
    acc = torch.zeros((size,) + tuple(v.shape[1:]), dtype=torch.float64).index_put_((inverse,), v, accumulate=True)
    if mean:
        c = _counts(inverse, size).clamp(min=1)
        acc = acc / c.view((-1,) + (1,) * (v.dim() - 1))
    return acc


def _additive(op: str) -> bool:
    if op not in ("add", "sum", "mean"):
        raise ValueError(f"{op!r} has no gradient reference (min / max are not differentiable in the package)")
    return op != "mean"


# ---------------------------------------------------------------------------------------------
# the ops
# ---------------------------------------------------------------------------------------------

def select_ref(value: torch.Tensor, sel: torch.Tensor, coef: Optional[torch.Tensor] = None):
    """out = value[sel] along dim 0 (permutations, CSC order, index_select, narrow); repeats add up
    in the gradient.  Returns (out, [grad])."""
    v = _leaf(value)
    return _finish(v[sel.cpu().to(torch.int64)], coef, [v], [value.dtype])


def select_reduce_grad_ref(value: torch.Tensor, sel: torch.Tensor, group: torch.Tensor, ngroups: int, reduce: str,
                           coef: Optional[torch.Tensor] = None):
    """A selection followed by a grouped sum / mean: out[g] = reduce of value[sel][i] over group[i] == g
    (index_select and then a reduction over rows).  Returns (out, [grad])."""
    v = _leaf(value)
    out = _accumulate(v[sel.cpu().to(torch.int64)], group.cpu().to(torch.int64), ngroups, mean=not _additive(reduce))
    return _finish(out, coef, [v], [value.dtype])


def coalesce_grad_ref(index: torch.Tensor, value: torch.Tensor, m: int, n: int, op: str = "add",
                      coef: Optional[torch.Tensor] = None):
    """Row-major sort, duplicates reduced with add / mean.  Returns (index', out, [grad])."""
    key = _keys(index, n)
    uniq, inverse = torch.unique(key, sorted=True, return_inverse=True)
    v = _leaf(value)
    out = _accumulate(v, inverse, uniq.numel(), mean=not _additive(op))
    out_v, grads = _finish(out, coef, [v], [value.dtype])
    return torch.stack([uniq // n, uniq % n]), out_v, grads


def reduce_grad_ref(index: torch.Tensor, value: torch.Tensor, m: int, n: int, dim: Optional[int], reduce: str,
                    coef: Optional[torch.Tensor] = None):
    """SparseTensor.sum / mean: over the stored entries of every column (dim 0) or row (dim 1) — the
    mean divides by their number, at least 1 —, over everything (None) or over a value dim (>= 2).
    Returns (out, [grad])."""
    index = index.cpu().to(torch.int64)
    v = _leaf(value)
    mean = not _additive(reduce)
    if dim is None:
        out = v.mean() if mean else v.sum()
    elif dim in (0, 1):
        out = _accumulate(v, index[1 - dim], (n, m)[dim], mean)
    else:
        out = v.mean(dim - 1) if mean else v.sum(dim - 1)
    return _finish(out, coef, [v], [value.dtype])


def add_grad_ref(index_a, value_a, index_b, value_b, m: int, n: int, coef: Optional[torch.Tensor] = None):
    """A + B: union of the entries, shared ones added.  Returns (index', out, [grad_a, grad_b])."""
    key = torch.cat([_keys(index_a, n), _keys(index_b, n)])
    uniq, inverse = torch.unique(key, sorted=True, return_inverse=True)
    a, b = _leaf(value_a), _leaf(value_b)
    out = _accumulate(torch.cat([a, b]), inverse, uniq.numel(), mean=False)
    out_v, grads = _finish(out, coef, [a, b], [value_a.dtype, value_b.dtype])
    return torch.stack([uniq // n, uniq % n]), out_v, grads


def mul_grad_ref(index_a, value_a, index_b, value_b, m: int, n: int, coef: Optional[torch.Tensor] = None):
    """A * B of two coalesced matrices: the entries both hold.  Returns (index', out, [grad_a, grad_b])."""
    ka, kb = _keys(index_a, n), _keys(index_b, n)
    uniq, inverse = torch.unique(torch.cat([ka, kb]), sorted=True, return_inverse=True)
    ia, ib = inverse[:ka.numel()], inverse[ka.numel():]
    a, b = _leaf(value_a), _leaf(value_b)
    U = uniq.numel()
    shape = (U,) + tuple(value_a.shape[1:])
    da = torch.zeros(shape, dtype=torch.float64).index_put_((ia,), a, accumulate=True)
    db = torch.zeros(shape, dtype=torch.float64).index_put_((ib,), b, accumulate=True)
    assert int(_counts(ia, U).max()) <= 1 and int(_counts(ib, U).max()) <= 1, "operands must be coalesced"
    both = (_counts(ia, U) > 0) & (_counts(ib, U) > 0)
    out_v, grads = _finish((da * db)[both], coef, [a, b], [value_a.dtype, value_b.dtype])
    return torch.stack([uniq[both] // n, uniq[both] % n]), out_v, grads


def symmetric_grad_ref(index, value, size: int, reduce: str = "sum", coef: Optional[torch.Tensor] = None):
    """to_symmetric: A and A^T laid over each other on a size x size grid.  Returns (index', out, [grad])."""
    index = index.cpu().to(torch.int64)
    key = torch.cat([index[0] * size + index[1], index[1] * size + index[0]])
    uniq, inverse = torch.unique(key, sorted=True, return_inverse=True)
    v = _leaf(value)
    out = _accumulate(torch.cat([v, v]), inverse, uniq.numel(), mean=not _additive(reduce))
    out_v, grads = _finish(out, coef, [v], [value.dtype])
    return torch.stack([uniq // size, uniq % size]), out_v, grads


def broadcast_grad_ref(index, value, vec: torch.Tensor, kind: str, coef: Optional[torch.Tensor] = None):
    """A + vec / A * vec for vec of shape (M, 1) (one operand per row) or (1, N) (per column).
    Returns (out, [grad_value, grad_vec])."""
    index = index.cpu().to(torch.int64)
    v, w = _leaf(value), _leaf(vec)
    which = index[0] if vec.shape[1] == 1 else index[1]
    spread = w.reshape(-1)[which]
    out = v + spread if kind == "add" else v * spread
    return _finish(out, coef, [v, w], [value.dtype, vec.dtype])


def spspmm_grad_ref(index_a, value_a, index_b, value_b, m: int, k: int, n: int, coef: Optional[torch.Tensor] = None,
                    dtype=None):
    """A @ B through dense float64 operands; the result's entries are the STRUCTURAL ones (every
    (i, j) a product reaches, cancelled or not) in row-major order.  An operand without values counts
    as ones.  Returns (index', out, [grad_a | None, grad_b | None])."""
    assert m * k <= (1 << 24) and k * n <= (1 << 24) and m * n <= (1 << 24), "dense operands: keep the shapes small"
    index_a, index_b = index_a.cpu().to(torch.int64), index_b.cpu().to(torch.int64)
    dtype = dtype or (value_a.dtype if value_a is not None else value_b.dtype)
    a, b = _leaf(value_a), _leaf(value_b)
    ones_a, ones_b = torch.ones(index_a.shape[1], dtype=torch.float64), torch.ones(index_b.shape[1], dtype=torch.float64)
    put = lambda index, v, r, c: torch.zeros(r, c, dtype=torch.float64).index_put_((index[0], index[1]), v, accumulate=True)
    dense = put(index_a, ones_a if a is None else a, m, k) @ put(index_b, ones_b if b is None else b, k, n)
    reached = (put(index_a, ones_a, m, k) @ put(index_b, ones_b, k, n)) > 0
    out_index = reached.nonzero().t().contiguous()
    out_v, grads = _finish(dense[reached], coef, [a, b], [dtype, dtype])
    return out_index, out_v, grads
