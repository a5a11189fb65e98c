"""Reference for the index-range tests: an order-preserving injection of a small index range into a
huge one, and a dict-of-keys oracle in Python ints.  CPU only: numpy and the standard library.

THE PROPERTY (it is the whole reference).  `inject(ids, small_dim, big_dim)` applies a STRICTLY
INCREASING map phi from [0, small_dim) into [0, big_dim).  Every sparse op of this package that is
tested with it depends on its row and column ids only through their ORDER and their EQUALITY
(sorting by (row, col), merging equal keys, matching A's columns with B's rows, run boundaries),
never through their magnitude.  A strictly increasing phi keeps both, so when the ids of the
operands are mapped through phi

  * the (row, col) order of the entries, which entries coalesce, every run boundary and the order
    of the terms inside every sum are unchanged;
  * hence the result is the small result with its ids mapped through phi: the same number of
    entries in the same order, VALUES BIT FOR BIT (also for floats and whatever the summation
    order, because it is the same summation), and every pointer / count / permutation array that
    belongs to a dimension that was NOT mapped is unchanged.

A kernel that truncates an id to 32 bits, sign-extends 2^31, wraps a key product past 2^63 or derives
a radix pass count from a wrong bound breaks the order or the equality of some mapped ids and fails
the comparison.  phi therefore places consecutive blocks of the small ids in bands around the values
where such faults live:

  "zero"   starting at 0
  "2^31"   straddling 2^31 - 1 | 2^31
  "2^32"   straddling 2^32 - 1 | 2^32
  "end"    ending at big_dim - 1

A straddling band is left out when its edge pair does not fit under big_dim, and also when the "end"
band already covers that pair (big_dim = 2^31 + 5, say): the pair is hit either way.

The dict-of-keys oracle (`dok_*`) computes product, union, intersection and coalesce on (row, col)
TUPLES of Python ints: no key row * n + col is ever formed, so nothing can overflow, and the CPU test
uses it to confirm the property independently of phi.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

INT64_MAX = (1 << 63) - 1
LIMIT = 3_037_000_499  # the largest d with d * d < 2^63
BIG_DIMS = ((1 << 31) - 1, 1 << 31, (1 << 31) + 5, (1 << 32) - 1, (1 << 32) + 7, LIMIT)
BANDS = ("zero", "2^31", "2^32", "end")
_EDGE = {"2^31": 1 << 31, "2^32": 1 << 32}
MIN_SMALL_DIM = 40  # four blocks of at least 10 ids: the "end" block then covers the edge pair of 2^31 + 5 and 2^32 + 7


def band_blocks(small_dim: int, big_dim: int, bands: Sequence[str] = BANDS) -> List[Tuple[int, int, int]]:
    """The blocks of phi as (first small id, one past the last small id, image of the first): block b maps
    s -> image + (s - first).  Blocks tile [0, small_dim) in order and their images are disjoint and increasing."""
    small_dim, big_dim = int(small_dim), int(big_dim)
    bands = tuple(bands)
    assert bands and all(b in BANDS for b in bands) and list(bands) == [b for b in BANDS if b in bands], bands
    if small_dim > big_dim:
        raise ValueError(f"cannot inject {small_dim} ids into {big_dim}")
    if small_dim < MIN_SMALL_DIM and len(bands) > 1:
        raise ValueError(f"small_dim must be at least {MIN_SMALL_DIM} for more than one band")
    assert big_dim - 1 <= INT64_MAX
    share = small_dim // len(bands)  # every block but the last; the last takes the remainder too
    end_len = small_dim - share * (len(bands) - 1)
    end_start = big_dim - end_len if "end" in bands else big_dim
    kept = []
    for b in bands:
        if b in _EDGE:
            edge = _EDGE[b]
            if edge >= big_dim:
                continue  # the pair (edge - 1, edge) does not fit under big_dim
            if "end" in bands and end_start <= edge - 1:
                continue  # the "end" band covers the pair already
            if edge - share // 2 + share > end_start:
                raise ValueError(f"band {b} collides with the end band for big_dim = {big_dim}")
        kept.append(b)
    share = small_dim // len(kept)
    blocks, first, floor = [], 0, 0
    for i, b in enumerate(kept):
        last = i == len(kept) - 1
        length = small_dim - first if last else share
        if b == "zero":
            image = 0
        elif b == "end":
            image = big_dim - length
        else:
            image = _EDGE[b] - length // 2
            assert length >= 2 and image <= _EDGE[b] - 1 and image + length > _EDGE[b]
        if image < floor:
            raise ValueError(f"band {b} does not fit above the previous one for big_dim = {big_dim}")
        assert image + length <= big_dim and image + length - 1 <= INT64_MAX
        blocks.append((first, first + length, image))
        first, floor = first + length, image + length
    assert first == small_dim
    return blocks


def inject(ids, small_dim: int, big_dim: int, bands: Sequence[str] = BANDS) -> np.ndarray:
    """phi(ids) as int64; ids must lie in [0, small_dim).  The arithmetic is done in numpy int64 on values
    asserted to stay at or below 2^63 - 1."""
    ids = np.asarray(ids, dtype=np.int64)
    assert ids.size == 0 or (int(ids.min()) >= 0 and int(ids.max()) < small_dim), "an id outside [0, small_dim)"
    out = np.empty_like(ids)
    done = np.zeros(ids.shape, dtype=bool)
    for first, stop, image in band_blocks(small_dim, big_dim, bands):
        assert image + (stop - first) - 1 <= INT64_MAX
        sel = (ids >= first) & (ids < stop)
        out[sel] = ids[sel] + np.int64(image - first)
        done |= sel
    assert bool(done.all())
    assert out.size == 0 or (int(out.min()) >= 0 and int(out.max()) < big_dim)
    return out


def inject_index(index, small_sizes: Tuple[int, int], big_sizes: Tuple[Optional[int], Optional[int]],
                 bands: Sequence[str] = BANDS) -> np.ndarray:
    """A [2, nnz] index with row and / or column ids mapped (None in big_sizes: that dimension stays)."""
    index = np.asarray(index, dtype=np.int64)
    out = index.copy()
    for d in (0, 1):
        if big_sizes[d] is not None:
            out[d] = inject(index[d], small_sizes[d], big_sizes[d], bands)
    return out


# ---------------------------------------------------------------------------------------------
# dict-of-keys oracle: (row, col) tuples of Python ints, integer values
# ---------------------------------------------------------------------------------------------

Dok = Dict[Tuple[int, int], object]


def _entries(index, value):
    index = np.asarray(index)
    rows, cols = [int(r) for r in index[0]], [int(c) for c in index[1]]
    if value is None:
        vals = [1] * len(rows)
    else:
        value = np.asarray(value)
        vals = [tuple(int(x) for x in np.atleast_1d(v).ravel()) if value.ndim > 1 else int(v) for v in value]
        flat = np.asarray(value, dtype=np.float64)
        assert np.array_equal(flat, np.round(flat)), "the oracle takes integer-valued data"
    return rows, cols, vals


def dok_result(d: Dok):
    """(index int64[2, nnz] in (row, col) order, values as a list in that order)."""
    keys = sorted(d)
    for r, c in keys:
        assert 0 <= r <= INT64_MAX and 0 <= c <= INT64_MAX
    index = np.array([[r for r, _ in keys], [c for _, c in keys]], dtype=np.int64).reshape(2, len(keys))
    return index, [d[k] for k in keys]


def _combine(a, b, op: str):
    if isinstance(a, tuple):
        return tuple(_combine(x, y, op) for x, y in zip(a, b))
    return {"add": a + b, "sum": a + b, "min": min(a, b), "max": max(a, b)}[op]


def dok_coalesce(index, value, op: str = "add"):
    """Duplicates of (row, col) reduced with op ("add" / "sum" / "min" / "max")."""
    rows, cols, vals = _entries(index, value)
    d: Dok = {}
    for r, c, v in zip(rows, cols, vals):
        d[(r, c)] = _combine(d[(r, c)], v, op) if (r, c) in d else v
    index, out = dok_result(d)
    return index, (None if value is None else out)


def dok_union(index_a, value_a, index_b, value_b):
    """A + B: the entries of either, values of shared entries added; values only when both have them."""
    has = value_a is not None and value_b is not None
    d: Dok = {}
    for index, value in ((index_a, value_a if has else None), (index_b, value_b if has else None)):
        rows, cols, vals = _entries(index, value)
        for r, c, v in zip(rows, cols, vals):
            d[(r, c)] = _combine(d[(r, c)], v, "add") if (r, c) in d else v
    index, out = dok_result(d)
    return index, (out if has else None)


def dok_intersection(index_a, value_a, index_b, value_b):
    """A * B elementwise: the entries of both (coalesced) operands, values multiplied."""
    ra, ca, va = _entries(index_a, value_a)
    rb, cb, vb = _entries(index_b, value_b)
    a = dict(zip(zip(ra, ca), va))
    b = dict(zip(zip(rb, cb), vb))
    assert len(a) == len(ra) and len(b) == len(rb), "operands must be coalesced"
    d: Dok = {k: a[k] * b[k] for k in a if k in b}
    return dok_result(d)


def dok_spspmm(index_a, value_a, index_b, value_b):
    """A @ B structurally: every (i, j) a partial product reaches is an entry, cancelled or not.  An operand
    without values counts as ones; the result has values when either operand has."""
    ra, ca, va = _entries(index_a, value_a)
    rb, cb, vb = _entries(index_b, value_b)
    rows_of_b: Dict[int, List[Tuple[int, int]]] = {}
    for r, c, v in zip(rb, cb, vb):
        rows_of_b.setdefault(r, []).append((c, v))
    d: Dok = {}
    for i, c, a in zip(ra, ca, va):
        for j, b in rows_of_b.get(c, ()):
            d[(i, j)] = d.get((i, j), 0) + a * b
    index, out = dok_result(d)
    return index, (None if value_a is None and value_b is None else out)


# ---------------------------------------------------------------------------------------------
# small cases
# ---------------------------------------------------------------------------------------------

def nonzero_integers(rng: np.random.Generator, n: int, tail: Tuple[int, ...] = (), bound: int = 8) -> np.ndarray:
    """int64 values with 1 <= |v| <= bound: every product and sum of them is an exact integer in any of the
    value dtypes, in any order, and no product is -0.0."""
    v = rng.integers(1, bound + 1, (n,) + tuple(tail), dtype=np.int64)
    return v * rng.choice(np.array([-1, 1], dtype=np.int64), v.shape)


def coalesced_index(rng: np.random.Generator, m: int, n: int, nnz: int, cover: bool = True,
                    must: Sequence[Tuple[int, int]] = ()) -> np.ndarray:
    """nnz distinct cells of an m x n matrix in (row, col) order.  cover: the first and last row and column
    and the ids next to every block boundary of the four-band phi are among them, so that every band edge
    value occurs in the injected index.  must: cells that have to be among them."""
    assert nnz <= m * n
    cells = set((int(r), int(c)) for r, c in must)
    if cover:
        rows, cols = _edge_ids(m), _edge_ids(n)
        for i in range(max(len(rows), len(cols))):
            cells.add((rows[i % len(rows)], cols[i % len(cols)]))
    assert len(cells) <= nnz
    while len(cells) < nnz:
        need = nnz - len(cells)
        for r, c in zip(rng.integers(0, m, need), rng.integers(0, n, need)):
            cells.add((int(r), int(c)))
    cells = sorted(cells)
    return np.array(cells, dtype=np.int64).T.reshape(2, len(cells))


def _edge_ids(dim: int) -> List[int]:
    """Small ids whose image is a band edge value for one of BIG_DIMS (0, 2^31 - 1, 2^31, 2^32 - 1, 2^32,
    big_dim - 1), and the first and last id of every block."""
    ids = {0, dim - 1}
    if dim >= MIN_SMALL_DIM:
        for big in BIG_DIMS:
            for first, stop, image in band_blocks(dim, big):
                ids.update((first, stop - 1))
                for target in EDGE_VALUES + (big - 1,):
                    if image <= target < image + (stop - first):
                        ids.add(first + target - image)
    return sorted(ids)


EDGE_VALUES = (0, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32)
