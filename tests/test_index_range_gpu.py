"""Hypersparse index-range tests: the sparse ops with row / column ids at 2^31, 2^32 and the int64 key limit.

A metamorphic suite (tests/index_range_ref.py states the property): every case is first run at its small size and
checked against the reference the suite already uses for that op; then its ids are mapped through a strictly
increasing phi into a dimension of BIG_DIMS = {2^31 - 1, 2^31, 2^31 + 5, 2^32 - 1, 2^32 + 7, 3 037 000 499} and the
result must be the small RESULT with its ids mapped through phi — indices, sparse sizes, values bit for bit, and every
cache the op fills (pointer, count and permutation arrays of the dimension that was not mapped are unchanged).
Values are non-zero integers of magnitude <= 8, so every sum is exact in any order and in every dtype.  No tolerance
anywhere: torch.equal / np.array_equal only.

MEMORY RULE.  No test lets the device allocate an array whose length is a sparse dimension above 2^24: the huge
value goes only to a dimension the op does not turn into a pointer array, read from the code:

  op                              huge-able                    pointer array on the other dimension
  ------------------------------  ---------------------------  -----------------------------------------------------
  spspmm (COO function form)      m: always                    rowptrB[k + 1] (row walk); colptrA[k + 1] (column walk)
                                  n: 8-byte / no / tracked     the column walk (4-byte values, m, n < 2^31) builds
                                     values, or n >= 2^31      colptrB[n + 1]: n = 2^31 - 1 with fp32 / int32 values
                                                               is EXCLUDED (a 16 GB pointer array; see the summary)
  coalesce, ops.coalesce_chain,   m and n                      none (keys only)
    ops.coalesce_small
  ops.make_keys / _checked,       multiplier / divisor         none
    split_keys, unique_sorted(_reduce)
  add, mul                        both                         none (coo() only)
  to_symmetric (sort route)       both, up to 3 037 000 499    none (the result is N x N with N = max(M, N): larger
                                                               sizes are refused, see below)
  to_symmetric (merge route)      rows, up to 3 037 000 499    colptr[n + 1] of csc()
  cat dim 0 / 1 / (0, 1)          both (row-built operands)    none; a rowptr is chained only when the operands have one
  __narrow_diag__                 columns                      rowptr[M + 1]
  narrow / select, dim 1          both                         none (mask over col; colptr sliced only when cached)
  index_select / masked_select    dim 0: columns               rowptr[M + 1], rowcount[M]
                                  dim 1: rows                  colptr[N + 1], colcount[N]
  remove_diag / set_diag /        columns, and with them k     rowptr[M + 1], rowcount[M] (colcount[N] only when the
    fill_diag / get_diag          up to N - 1 > 2^31           operand has it cached: never here).  k below -2^31 needs
                                                               M > 2^31 rows, i.e. rowptr[M + 1]: EXCLUDED
  t()                             rows                         colptr[N + 1] (it becomes the result's rowptr)
  transpose (function form)       both                         none (the coalesce chain on swapped ids)

EXCLUDED by the rule, whole ops:
  ops.sample_adj    `newid` is sized max(num_rows, num_cols) and rowptr by num_rows: neither dimension can be huge.
                    Its keys owner * n_out + id are bounded by the lengths of two device arrays (S * n_out), so the
                    product cannot come near 2^63 either: there is no refusal to test.
  saint_subgraph    a square matrix: rowptr[N + 1] and a workspace sized by N.
  ops.make_keys     takes one multiplier and no row bound: it has no pair of dimensions to refuse (make_keys_checked
                    has, and refuses).
Dense operands are never sized by a huge dimension, so SpMM, sddmm, softmax and attention are not here.

Every test runs inside `bounded_memory()`: after a reset_peak_memory_stats(), torch.cuda.max_memory_allocated() stays
under 256 MB above what was live at the reset, so a route that silently builds a pointer array over a huge dimension
(8 bytes x 2^31 = 16 GB) fails.

REFUSALS.  Wherever an op forms a key row * n + col from two dimensions, dims whose product is >= 2^63
(3 037 000 500 squared, 2^32 x 2^31) must raise ValueError naming the two dimensions before anything is launched.
"""
import functools
import importlib
import inspect
import itertools
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import grad_ref as gr
import index_range_ref as ir
import reduce_ref as rr
import storage_ref as sr
from oracle import storage_oracle as so

pytestmark = pytest.mark.gpu

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
P31, P32, LIMIT = 1 << 31, 1 << 32, ir.LIMIT
BIG = [pytest.param(b, id=str(b)) for b in ir.BIG_DIMS]
PEAK_BYTES = 256 << 20
FIELDS = ("_row", "_rowptr", "_col", "_value", "_rowcount", "_colptr", "_colcount", "_csr2csc", "_csc2csr")
OVER = [pytest.param(LIMIT + 1, LIMIT + 1, id="3037000500^2"), pytest.param(P32, P31, id="2^32x2^31")]


# ---------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------

def ps():
    import paddle_sparse_amd

    return paddle_sparse_amd


def ops():
    from paddle_sparse_amd import ops as o

    return o


def cuda(x):
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.cuda()


def cpu(x):
    return None if x is None else x.detach().cpu()


@contextmanager
def bounded_memory():
    """The peak of device memory inside the block stays under 256 MB above the level at its start.  The level at the
    start is subtracted because max_memory_allocated() counts what is live already: in a run of the whole suite the
    operands that earlier modules keep cached (more than 256 MB of them) would fail every test here before it
    allocates a byte.  Run alone the level is a few MB and this is the plain bound on max_memory_allocated()."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    assert peak < PEAK_BYTES, f"peak device memory {peak} bytes: an array sized by a huge dimension was built"


def over(**folded):
    """The test body run once per combination of the given values INSIDE one test case; a failure names the
    combination.  Sizes and dtypes that only repeat the same few launches are folded this way, so that the suite
    gains a hundred-odd cases instead of five hundred; the checks are the same.  A key "a,b" takes pairs."""
    names = [tuple(k.split(",")) for k in folded]
    flat = [n for group in names for n in group]

    def wrap(fn):
        def run(**kw):
            for combo in itertools.product(*folded.values()):
                args = {}
                for group, value in zip(names, combo):
                    args.update(zip(group, value if len(group) > 1 else (value,)))
                try:
                    fn(**kw, **args)
                except Exception as e:
                    raise AssertionError(f"[{', '.join(f'{k}={v}' for k, v in args.items())}] "
                                         f"{type(e).__name__}: {e}") from e

        sig = inspect.signature(fn)
        run.__signature__ = sig.replace(parameters=[p for p in sig.parameters.values() if p.name not in flat])
        run.__name__, run.__qualname__, run.__doc__, run.__module__ = fn.__name__, fn.__qualname__, fn.__doc__, fn.__module__
        return run

    return wrap


class Phi:
    """phi of index_range_ref on torch / numpy ids; identity when big is None."""

    def __init__(self, small, big, bands=ir.BANDS):
        self.small, self.big, self.bands = small, big, bands

    def __call__(self, ids):
        ids = np.asarray(cpu(ids) if torch.is_tensor(ids) else ids, dtype=np.int64)
        if self.big is None:
            return torch.from_numpy(ids.copy())
        return torch.from_numpy(ir.inject(ids, self.small, self.big, self.bands))

    @property
    def size(self):
        return self.small if self.big is None else self.big


def map_index(index, phi_row, phi_col):
    return torch.stack([phi_row(index[0]), phi_col(index[1])])


def same(got, want, what):
    got, want = cpu(got), cpu(want)
    assert (got is None) == (want is None), f"{what}: {'missing' if got is None else 'unexpected'}"
    if got is None:
        return
    assert got.dtype == want.dtype and got.shape == want.shape, \
        f"{what}: {got.dtype}{tuple(got.shape)} for {want.dtype}{tuple(want.shape)}"
    if not torch.equal(got, want):
        bad = (got != want).reshape(got.shape[0], -1).any(1).nonzero().flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {got.shape[0]} rows differ, first at {i}: "
                             f"{got[i].tolist()} for {want[i].tolist()}")


def values_of(ints, dtype):
    return None if dtype is None else torch.from_numpy(ints).to(dtype)


def tensor(index, value, sizes):
    """A SparseTensor over row-major sorted entries, built from `row` alone: no pointer array exists until an op
    asks for one."""
    return ps().SparseTensor(row=cuda(index[0]), col=cuda(index[1]), value=cuda(value), sparse_sizes=tuple(sizes),
                             is_sorted=True)


def check_small(t, ref_index, ref_value, sizes, what):
    """A small result against its reference: entries, values, sizes, and every cache it carries against the plain
    definition (storage_ref) from its own entries."""
    st = t.storage
    assert tuple(st.sparse_sizes()) == tuple(sizes), f"{what}: sizes {st.sparse_sizes()} for {sizes}"
    row, col = cpu(st.row()), cpu(st.col())
    same(torch.stack([row, col]), torch.as_tensor(ref_index), f"{what} index")
    same(st.value(), None if ref_value is None else torch.as_tensor(ref_value), f"{what} value")
    d = sr.derived(row.numpy(), col.numpy(), sizes[0], sizes[1])
    assert d.sorted, f"{what}: entries not in (row, col) order"
    for name in ("rowptr", "rowcount", "colptr", "colcount", "csr2csc", "csc2csr"):
        got = getattr(st, "_" + name)
        if got is not None:
            same(got, torch.from_numpy(getattr(d, name)), f"{what} cache {name}")


def check_embedded(big_t, small_t, phi_row, phi_col, what, sizes=None):
    """The embedded result is the small one mapped: same caches present, row / col through phi, the rest unchanged.
    `row` is derived state where a rowptr exists (check_small has expanded it on the small side): compared through
    row() then, which the small row count keeps cheap."""
    b, s = big_t.storage, small_t.storage
    want_sizes = tuple(sizes) if sizes is not None else (phi_row.size if phi_row.big is not None else s.sparse_size(0),
                                                         phi_col.size if phi_col.big is not None else s.sparse_size(1))
    assert tuple(b.sparse_sizes()) == want_sizes, f"{what}: sizes {b.sparse_sizes()} for {want_sizes}"
    for f in FIELDS:
        x, y = getattr(b, f), getattr(s, f)
        if f == "_row":
            if x is None or y is None:
                assert b._rowptr is not None and s._rowptr is not None, f"{what}: neither row nor rowptr"
                x, y = b.row(), s.row()
            y = phi_row(y)
        if f == "_col":
            y = phi_col(y)
        same(x, y, f"{what} {f[1:]}")


class Spy:
    """Records the names of the `ops.<name>` called while active."""

    def __init__(self, *names):
        self.ops, self.names, self.calls = ops(), names, []
        self.real = {n: getattr(self.ops, n) for n in names}

    def __enter__(self):
        for n in self.names:
            setattr(self.ops, n, (lambda n_: lambda *a, **k: self.calls.append(n_) or self.real[n_](*a, **k))(n))
        return self

    def __exit__(self, *exc):
        for n, f in self.real.items():
            setattr(self.ops, n, f)


LAUNCHES = ("ind2ptr", "ptr2ind", "spspmm_count", "count2ptr", "spspmm_expand", "gather_rows", "index_sort",
            "sort_pairs", "sort_pairs_field", "make_keys", "make_keys_checked", "split_keys", "merge_sorted",
            "unique_sorted", "unique_sorted_reduce", "coalesce_chain", "coalesce_small", "segment_csr", "bincount")


def refused(fn, rows, cols, direct=None):
    """fn() raises ValueError naming both dimensions before any launching op of `ops` is called (`direct`: the one
    fn calls itself, which must call no other), and allocates nothing sized by them."""
    with bounded_memory(), Spy(*LAUNCHES) as spy, pytest.raises(ValueError, match=rf"{rows} x {cols}"):
        fn()
    assert spy.calls == ([direct] if direct else []), f"launched {spy.calls} before raising"


# ---------------------------------------------------------------------------------------------
# spspmm
# ---------------------------------------------------------------------------------------------

M_, K_, N_ = 200, 60, 150


def walk(dtype, m, n):
    return "column" if dtype in (F32, I32) and m < P31 and n < P31 else "row"


@functools.lru_cache(maxsize=None)
def product_case():
    rng = np.random.default_rng(11)
    # the last row of A meets the last column of B: the product holds the cell (m - 1, n - 1), the largest key
    index_a = ir.coalesced_index(rng, M_, K_, 900, must=[(M_ - 1, K_ - 1)])
    index_b = ir.coalesced_index(rng, K_, N_, 600, must=[(K_ - 1, N_ - 1)])
    return index_a, ir.nonzero_integers(rng, 900), index_b, ir.nonzero_integers(rng, 600)


def run_product(index_a, va, index_b, vb, m, k, n):
    index, value = ps().spspmm(cuda(index_a), cuda(va), cuda(index_b), cuda(vb), m, k, n)
    return cpu(index), cpu(value)


@functools.lru_cache(maxsize=None)
def small_product(dtype, has_a=True, has_b=True):
    """The small product on the device, checked against reduce_ref.spspmm_ref (a value-less operand is ones)."""
    index_a, ia, index_b, ib = product_case()
    va, vb = values_of(ia, dtype if has_a else None), values_of(ib, dtype if has_b else None)
    index, value = run_product(index_a, va, index_b, vb, M_, K_, N_)
    ones = lambda v: torch.ones(v.shape[0], dtype=dtype)
    ref_index, ref_value = rr.spspmm_ref(torch.from_numpy(index_a), va if has_a else ones(ia), torch.from_numpy(index_b),
                                         vb if has_b else ones(ib), M_, K_, N_)
    same(index, ref_index, "small product index")
    same(value, ref_value if (has_a or has_b) else None, "small product value")
    return index, value


def embedded_product(dtype, big_m, big_n, has_a=True, has_b=True, route=None):
    index_a, ia, index_b, ib = product_case()
    phi_m, phi_n = Phi(M_, big_m), Phi(N_, big_n)
    small_index, small_value = small_product(dtype, has_a, has_b)
    big_a = map_index(torch.from_numpy(index_a), phi_m, Phi(K_, None))
    big_b = map_index(torch.from_numpy(index_b), Phi(K_, None), phi_n)
    va, vb = values_of(ia, dtype if has_a else None), values_of(ib, dtype if has_b else None)
    with bounded_memory(), Spy("sort_pairs_field") as spy:
        index, value = run_product(big_a, va, big_b, vb, phi_m.size, K_, phi_n.size)
    if route is not None:
        assert bool(spy.calls) == (route == "column"), f"took the {'column' if spy.calls else 'row'} walk"
    same(index, map_index(small_index, phi_m, phi_n), "product index")
    same(value, small_value, "product value")
    return index, value


@pytest.mark.parametrize("big", BIG)
@over(dtype=[F32, F64, I32, I64])
def test_spspmm_with_huge_m(big, dtype):
    """Rows of A (and of C) up to 2^63 / n.  m = 2^31 - 1 with 4-byte values is the column walk with every bit of the
    31-bit row field in use; 8-byte values, and any m >= 2^31, take the row-order walk."""
    embedded_product(dtype, big, None, route=walk(dtype, big, N_))


@pytest.mark.parametrize("big", BIG)
@over(dtype=[F32, F64, I32, I64])
def test_spspmm_with_huge_n(big, dtype):
    """Columns of B (and of C).  The column walk builds colptrB[n + 1], so 4-byte values with n < 2^31 are excluded
    by the memory rule (see the table): those combinations are not run."""
    if walk(dtype, M_, big) == "row":
        embedded_product(dtype, None, big, route="row")


@pytest.mark.parametrize("dtype", [F32, F64], ids=str)
def test_spspmm_with_keys_just_under_2_63(dtype):
    """m = n = 3 037 000 499: the keys i * n + j reach m * n - 1 < 2^63, all eight radix passes."""
    index, _ = embedded_product(dtype, LIMIT, LIMIT, route="row")
    assert int(index[0, -1]) * LIMIT + int(index[1, -1]) == LIMIT * LIMIT - 1, "the case must reach the last key"


@pytest.mark.parametrize("dtype", [F32, I32], ids=str)
def test_spspmm_one_past_the_column_walk_equals_it(dtype):
    """m = 2^31 takes the row-order walk, m = 2^31 - 1 the column walk: the same ids give the same product."""
    index_a, ia, index_b, ib = product_case()
    phi_m = Phi(M_, P31 - 1)
    big_a = map_index(torch.from_numpy(index_a), phi_m, Phi(K_, None))
    va, vb = values_of(ia, dtype), values_of(ib, dtype)
    out = {}
    for m in (P31 - 1, P31):
        with bounded_memory(), Spy("sort_pairs_field") as spy:
            out[m] = run_product(big_a, va, index_b, vb, m, K_, N_)
        assert bool(spy.calls) == (m < P31)
    same(out[P31][0], out[P31 - 1][0], "index at m = 2^31")
    same(out[P31][1], out[P31 - 1][1], "value at m = 2^31")
    same(out[P31][0], map_index(small_product(dtype)[0], phi_m, Phi(N_, None)), "index")


@pytest.mark.parametrize("missing", ["a", "b", "both"])
@pytest.mark.parametrize("big", [pytest.param(P31 - 1, id="2^31-1"), pytest.param(P32 + 7, id="2^32+7")])
def test_spspmm_of_value_less_operands(big, missing):
    has_a, has_b = missing == "b", missing == "a"
    embedded_product(F32, big, None, has_a, has_b)
    embedded_product(F64, None, big, has_a, has_b)


@pytest.mark.parametrize("track", ["a", "b", "both"])
@pytest.mark.parametrize("big", [pytest.param(P31 - 1, id="2^31-1"), pytest.param(LIMIT, id="limit")])
@over(dtype=[F32, F64])
def test_spspmm_tracked_route(big, track, dtype):
    """requires_grad on either operand: forward bits and both gradients equal the small case's, which equal
    grad_ref.spspmm_grad_ref."""
    index_a, ia, index_b, ib = product_case()
    ta, tb = track in ("a", "both"), track in ("b", "both")
    coef = None

    def run(ia_index, ib_index, m, n):
        va, vb = cuda(values_of(ia, dtype)).requires_grad_(ta), cuda(values_of(ib, dtype)).requires_grad_(tb)
        index, value = ps().spspmm(cuda(ia_index), va, cuda(ib_index), vb, m, K_, n)
        (value * cuda(coef[:value.shape[0]].to(dtype))).sum().backward()
        return cpu(index), cpu(value), cpu(va.grad), cpu(vb.grad)

    ref_index, _, _ = gr.spspmm_grad_ref(torch.from_numpy(index_a), values_of(ia, dtype), torch.from_numpy(index_b),
                                          values_of(ib, dtype), M_, K_, N_)
    coef = gr.coefs(ref_index.shape[1], seed=5)
    ref_index, ref_value, (ga, gb) = gr.spspmm_grad_ref(torch.from_numpy(index_a), values_of(ia, dtype),
                                                         torch.from_numpy(index_b), values_of(ib, dtype), M_, K_, N_,
                                                         coef=coef)
    index, value, grad_a, grad_b = run(torch.from_numpy(index_a), torch.from_numpy(index_b), M_, N_)
    same(index, ref_index, "small tracked index")
    same(value, ref_value, "small tracked value")
    same(grad_a, ga if ta else None, "small grad A")
    same(grad_b, gb if tb else None, "small grad B")
    phi_m, phi_n = Phi(M_, big), Phi(N_, big)
    with bounded_memory():
        big_index, big_value, big_ga, big_gb = run(map_index(torch.from_numpy(index_a), phi_m, Phi(K_, None)),
                                                   map_index(torch.from_numpy(index_b), Phi(K_, None), phi_n), big, big)
    same(big_index, map_index(index, phi_m, phi_n), "tracked index")
    same(big_value, value, "tracked value")
    same(big_ga, grad_a, "grad A")
    same(big_gb, grad_b, "grad B")


# ---------------------------------------------------------------------------------------------
# coalesce
# ---------------------------------------------------------------------------------------------

CM, CN, CDISTINCT, CNNZ = 150, 130, 700, 2500
COALESCE_DIMS = [(b, None) for b in ir.BIG_DIMS] + [(None, b) for b in ir.BIG_DIMS] + [(LIMIT, LIMIT)]


@functools.lru_cache(maxsize=None)
def coalesce_case():
    """Shuffled entries with duplicates: every distinct cell at least once."""
    rng = np.random.default_rng(21)
    base = ir.coalesced_index(rng, CM, CN, CDISTINCT)
    pick = np.concatenate([rng.permutation(CDISTINCT), rng.integers(0, CDISTINCT, CNNZ - CDISTINCT)])
    rng.shuffle(pick)
    return base[:, pick], ir.nonzero_integers(rng, CNNZ, (3,))


def coalesce_values(kind):
    _, ints = coalesce_case()
    return {"none": None, "f32": values_of(ints[:, 0], F32), "i32": values_of(ints[:, 0], I32),
            "f64": values_of(ints[:, 0], F64), "i64": values_of(ints[:, 0], I64), "f32x3": values_of(ints, F32)}[kind]


@functools.lru_cache(maxsize=None)
def small_coalesce(kind, op):
    index, _ = coalesce_case()
    value = coalesce_values(kind)
    out_index, out_value = ps().coalesce(cuda(index), cuda(value), CM, CN, op)
    ref_index, ref_value = rr.coalesce_ref(torch.from_numpy(index), value, CM, CN, op)
    same(out_index, ref_index, "small coalesce index")
    same(out_value, ref_value, "small coalesce value")
    return cpu(out_index), cpu(out_value)


@pytest.mark.parametrize("kind,op", [("f32", "add"), ("none", "add"), ("f64", "add"), ("f32x3", "add"), ("i32", "max"),
                                     ("i64", "min"), ("f32", "mean")])
@over(**{"big_m,big_n": COALESCE_DIMS})
def test_coalesce_function(big_m, big_n, kind, op):
    """ps.coalesce: the one-launch form (fp32 / int32 / no values), the two-call chain (the rest) and, from
    m * n >= 2^62, the stream route (make_keys_checked + sort + unique)."""
    index, _ = coalesce_case()
    phi_m, phi_n = Phi(CM, big_m), Phi(CN, big_n)
    small_index, small_value = small_coalesce(kind, op)
    with bounded_memory():
        out_index, out_value = ps().coalesce(cuda(map_index(torch.from_numpy(index), phi_m, phi_n)),
                                             cuda(coalesce_values(kind)), phi_m.size, phi_n.size, op)
    same(out_index, map_index(small_index, phi_m, phi_n), "coalesce index")
    same(out_value, small_value, "coalesce value")


@pytest.mark.parametrize("big_m,big_n", [pytest.param(P31 + 5, None, id="2^31+5xsmall"),
                                         pytest.param(None, P32 + 7, id="smallx2^32+7"),
                                         pytest.param(P31 + 5, P31 - 1, id="2^31+5x2^31-1"),
                                         pytest.param(LIMIT, LIMIT, id="limit^2")])
@over(kind=["f32", "f64"])
def test_coalesce_chain_reading_the_count_first(big_m, big_n, kind):
    """ops.coalesce_chain(read_first=True): exactly sized outputs.  At 3 037 000 499 squared the chain's own bound
    (M * N < 9.0e18) refuses, with the library's checked error and before a launch."""
    from paddle_sparse_amd._lib import HipCoreError

    index, _ = coalesce_case()
    phi_m, phi_n = Phi(CM, big_m), Phi(CN, big_n)
    small_index, small_value = small_coalesce(kind, "add")
    args = (cuda(phi_m(index[0])), cuda(phi_n(index[1])), cuda(coalesce_values(kind)), phi_m.size, phi_n.size, "add")
    if phi_m.size * phi_n.size >= 9.0e18:
        with pytest.raises(HipCoreError, match="does not fit"):
            ops().coalesce_chain(*args, read_first=True)
        return
    with bounded_memory():
        out_index, out_value, was_sorted = ops().coalesce_chain(*args, read_first=True)
    assert not was_sorted
    same(out_index, map_index(small_index, phi_m, phi_n), "chain index")
    same(out_value, small_value, "chain value")


@over(**{"big_m,big_n": COALESCE_DIMS})
def test_coalesce_small(big_m, big_n):
    """ops.coalesce_small: count, run pointer, distinct (row, col) and the stable sorting permutation."""
    index, _ = coalesce_case()
    assert CNNZ <= ops().coalesce_small_max()
    phi_m, phi_n = Phi(CM, big_m), Phi(CN, big_n)
    count, ptr, row, col, perm = ops().coalesce_small(cuda(index[0]), cuda(index[1]), CM, CN)
    key = index[0] * CN + index[1]
    order = np.argsort(key, kind="stable")
    heads = np.nonzero(np.concatenate([[True], key[order][1:] != key[order][:-1]]))[0]
    assert count == heads.size == CDISTINCT
    same(perm, torch.from_numpy(order), "small perm")
    same(ptr, torch.from_numpy(np.concatenate([heads, [CNNZ]])), "small ptr")
    same(row, torch.from_numpy(index[0][order][heads]), "small row")
    same(col, torch.from_numpy(index[1][order][heads]), "small col")
    with bounded_memory():
        big = ops().coalesce_small(cuda(phi_m(index[0])), cuda(phi_n(index[1])), phi_m.size, phi_n.size)
    assert big[0] == count
    same(big[1], ptr, "ptr")
    same(big[2], phi_m(row), "row")
    same(big[3], phi_n(col), "col")
    same(big[4], perm, "perm")


# ---------------------------------------------------------------------------------------------
# keys: make_keys, make_keys_checked, split_keys, unique_sorted, unique_sorted_reduce
# ---------------------------------------------------------------------------------------------

WIDTHS = BIG + [pytest.param(P32, id="2^32")]


def key_case(width, n=1500, seed=31):
    """(a, b) as lists of Python ints with b < width and a * width + b <= 2^63 - 1, the extremes included."""
    rows = ((1 << 63) - 1) // width  # a < rows keeps every key of a rows x width matrix inside int64
    rng = np.random.default_rng(seed)
    a = [0, 0, rows - 1, rows - 1, min(rows - 1, P31 - 1), min(rows - 1, P31), 1]
    b = [0, width - 1, width - 1, 0, min(width - 1, P31 - 1), min(width - 1, P31), width - 1]
    a += [int(x) for x in rng.integers(0, rows, n - len(a))]
    b += [int(x) for x in rng.integers(0, width, n - len(b))]
    return rows, a, b


def i64(values):
    return torch.tensor(values, dtype=I64)


@pytest.mark.parametrize("width", WIDTHS)
def test_make_and_split_keys(width):
    rows, a, b = key_case(width)
    keys = [x * width + y for x, y in zip(a, b)]
    assert max(keys) == (rows - 1) * width + width - 1 <= (1 << 63) - 1
    unsorted = any(k1 < k0 for k0, k1 in zip(keys, keys[1:]))
    assert unsorted
    with bounded_memory():
        got, flag = ops().make_keys(cuda(i64(a)), cuda(i64(b)), width, check_sorted=True)
        same(got, i64(keys), "make_keys")
        assert int(flag.item()) == 1
        order = sorted(range(len(keys)), key=keys.__getitem__)
        got, flag = ops().make_keys(cuda(i64([a[i] for i in order])), cuda(i64([b[i] for i in order])), width,
                                    check_sorted=True)
        same(got, i64(sorted(keys)), "make_keys of sorted input")
        assert int(flag.item()) == 0
        got, status = ops().make_keys_checked(cuda(i64(a)), cuda(i64(b)), rows, width)
        same(got, i64(keys), "make_keys_checked")
        assert int(status[1].item()) == 2, "in range, not sorted"
        got, status = ops().make_keys_checked(cuda(i64([a[i] for i in order])), cuda(i64([b[i] for i in order])), rows,
                                              width)
        same(got, i64(sorted(keys)), "make_keys_checked of sorted input")
        assert int(status[1].item()) == 0, "in range and sorted"
        hi, lo = ops().split_keys(cuda(i64(keys)), width)
        same(hi, i64([k // width for k in keys]), "split_keys hi")
        same(lo, i64([k % width for k in keys]), "split_keys lo")
        # keys that fit 32 bits beside ones that do not, under a divisor that does or does not
        mixed = [0, 1, width - 1, width, P32 - 1, P32, P32 + 1, (1 << 63) - 1]
        hi, lo = ops().split_keys(cuda(i64(mixed)), width)
        same(hi, i64([k // width for k in mixed]), "split_keys hi (mixed)")
        same(lo, i64([k % width for k in mixed]), "split_keys lo (mixed)")


@pytest.mark.parametrize("width", WIDTHS)
@over(runs=["short", "long", "distinct"])
def test_unique_sorted_and_reduce(width, runs):
    """Run heads, (key // N, key % N) of every distinct key, and the fused reduce in its one-launch form (short runs),
    its two-launch form (long runs) and without duplicates."""
    rows, a, b = key_case(width, n=60 if runs == "long" else 1500)
    distinct = sorted(set(x * width + y for x, y in zip(a, b)))
    rng = np.random.default_rng(41)
    repeat = {"short": rng.integers(1, 4, len(distinct)), "long": rng.integers(40, 90, len(distinct)),
              "distinct": np.ones(len(distinct), dtype=np.int64)}[runs]
    keys = [k for k, r in zip(distinct, repeat) for _ in range(int(r))]
    n, count = len(keys), len(distinct)
    assert {"short": count < n and count * 32 > n, "long": count * 32 <= n, "distinct": count == n}[runs]
    ptr = np.concatenate([[0], np.cumsum(repeat)])
    payload = ir.nonzero_integers(rng, n)
    with bounded_memory():
        got = ops().unique_sorted(cuda(i64(keys)), width)
        assert got[0] == count
        same(got[1], torch.from_numpy(ptr), "ptr")
        same(got[2], i64([k // width for k in distinct]), "row")
        same(got[3], i64([k % width for k in distinct]), "col")
        for dtype in (F32, I32):
            for reduce in ("sum", "max"):
                value = values_of(payload, dtype)
                want = rr.segment_ref(value, torch.from_numpy(ptr), reduce)
                got = ops().unique_sorted_reduce(cuda(i64(keys)), width, cuda(value), reduce)
                assert got[0] == count
                same(got[1], i64([k // width for k in distinct]), f"reduce row {dtype} {reduce}")
                same(got[2], i64([k % width for k in distinct]), f"reduce col {dtype} {reduce}")
                same(got[3], want, f"reduce value {dtype} {reduce}")


# ---------------------------------------------------------------------------------------------
# add, mul, to_symmetric
# ---------------------------------------------------------------------------------------------

AM, AN = 160, 140
# (sizes of A, sizes of B, dimension phi maps into) with None for a dimension that stays small
PAIR_DIMS = ([((b, None), (b, None)) for b in ir.BIG_DIMS] + [((None, b), (None, b)) for b in ir.BIG_DIMS]
             + [((LIMIT, LIMIT), (LIMIT, LIMIT)), ((P32 + 7, None), (LIMIT, None)), ((None, P31 + 5), (None, P32 - 1)),
                ((1 << 30, P32 + 7), ((1 << 30) + 9, P31))])


@functools.lru_cache(maxsize=None)
def pair_case():
    rng = np.random.default_rng(51)
    index_a = ir.coalesced_index(rng, AM, AN, 1400)
    shared = index_a[:, rng.permutation(1400)[:500]]
    fresh = ir.coalesced_index(rng, AM, AN, 900)
    cells = sorted(set(map(tuple, shared.T.tolist())) | set(map(tuple, fresh.T.tolist())))
    index_b = np.array(cells, dtype=np.int64).T
    return index_a, ir.nonzero_integers(rng, 1400, (3,)), index_b, ir.nonzero_integers(rng, index_b.shape[1], (3,))


def pair_values(kind):
    _, ia, _, ib = pair_case()
    if kind == "none":
        return None, None
    if kind == "f32x3":
        return values_of(ia, F32), values_of(ib, F32)
    dtype = {"f32": F32, "f64": F64, "i32": I32}[kind]
    return values_of(ia[:, 0], dtype), values_of(ib[:, 0], dtype)


@contextmanager
def threshold(module, name, value):
    """A route threshold of the package lowered, so that inputs of a few thousand entries take the route of large ones."""
    mod = importlib.import_module(f"paddle_sparse_amd.{module}")
    old = getattr(mod, name)
    setattr(mod, name, value)
    try:
        yield
    finally:
        setattr(mod, name, old)


def pair_op(op, route):
    fn = ps().add if op == "add" else ps().mul
    if op == "add" and route == "merge":
        def merged(a, b):
            with threshold("add", "_ONE_WORKGROUP_BELOW", 0), Spy("merge_sorted") as spy:
                out = fn(a, b)
            assert spy.calls, "add did not take the merge route"
            return out
        return merged
    return fn


@functools.lru_cache(maxsize=None)
def small_pair(op, route, kind):
    index_a, _, index_b, _ = pair_case()
    va, vb = pair_values(kind)
    out = pair_op(op, route)(tensor(index_a, va, (AM, AN)), tensor(index_b, vb, (AM, AN)))
    np_ = lambda v: None if v is None else v.numpy()
    a = so.Storage(index_a[0], index_a[1], np_(va), (AM, AN), True)
    b = so.Storage(index_b[0], index_b[1], np_(vb), (AM, AN), True)
    ref = so.add(a, b) if op == "add" else so.mul(a, b)
    assert 0 < ref.row.size < index_a.shape[1] + index_b.shape[1]
    check_small(out, np.stack([ref.row, ref.col]), ref.value, (AM, AN), f"small {op}")
    return out


@pytest.mark.parametrize("op,route,kind", [("add", "auto", "f32"), ("add", "merge", "f32"), ("add", "merge", "f64"),
                                           ("add", "merge", "f32x3"), ("add", "auto", "f32x3"), ("add", "merge", "none"),
                                           ("mul", "merge", "f32"), ("mul", "merge", "f64"), ("mul", "merge", "f32x3")])
@over(**{"sizes_a,sizes_b": PAIR_DIMS})
def test_add_and_mul_of_sparse_tensors(sizes_a, sizes_b, op, route, kind):
    """sparse + sparse and sparse * sparse: the chain on the concatenation (small add), the stable merge with the
    values riding (fp32) and with the source index (fp64, [nnz, 3]).  Operands of different huge shapes share phi
    (into the smaller shape); the result takes the larger."""
    index_a, _, index_b, _ = pair_case()
    va, vb = pair_values(kind)
    small = small_pair(op, route, kind)
    into = [None if x is None else min(x, y) for x, y in zip(sizes_a, sizes_b)]
    phi_m, phi_n = Phi(AM, into[0]), Phi(AN, into[1])
    full = lambda s: (AM if s[0] is None else s[0], AN if s[1] is None else s[1])
    with bounded_memory():
        a = tensor(map_index(torch.from_numpy(index_a), phi_m, phi_n), va, full(sizes_a))
        b = tensor(map_index(torch.from_numpy(index_b), phi_m, phi_n), vb, full(sizes_b))
        out = pair_op(op, route)(a, b)
    shape = tuple(max(x, y) for x, y in zip(full(sizes_a), full(sizes_b)))
    check_embedded(out, small, phi_m, phi_n, op, sizes=shape)


SYM_M, SYM_N = 200, 40  # the columns lie inside phi's first block, where phi is the identity


@functools.lru_cache(maxsize=None)
def symmetric_case():
    rng = np.random.default_rng(61)
    assert ir.band_blocks(SYM_M, LIMIT)[0][1] >= SYM_N and ir.band_blocks(SYM_M, P31)[0][1] >= SYM_N
    square = ir.coalesced_index(rng, SYM_M, SYM_M, 1800)
    tall = ir.coalesced_index(rng, SYM_M, SYM_N, 1500)
    return square, tall, ir.nonzero_integers(rng, 1800, (3,))


def symmetric_values(kind, nnz):
    ints = symmetric_case()[2][:nnz]
    return {"none": None, "f32": values_of(ints[:, 0], F32), "f64": values_of(ints[:, 0], F64),
            "f32x3": values_of(ints, F32)}[kind]


def symmetric_run(index, value, sizes, route, reduce):
    t = tensor(index, value, sizes)
    if route == "merge":
        with threshold("tensor", "_MERGE_ABOVE", 0), Spy("merge_sorted") as spy:
            out = t.to_symmetric(reduce)
        assert spy.calls, "to_symmetric did not take the merge route"
        return out
    return t.to_symmetric(reduce)


@functools.lru_cache(maxsize=None)
def small_symmetric(shape, route, reduce, kind):
    square, tall, _ = symmetric_case()
    index, sizes = (square, (SYM_M, SYM_M)) if shape == "square" else (tall, (SYM_M, SYM_N))
    value = symmetric_values(kind, index.shape[1])
    out = symmetric_run(index, value, sizes, route, reduce)
    ref = so.to_symmetric(so.Storage(index[0], index[1], None if value is None else value.numpy(), sizes, True), reduce)
    check_small(out, np.stack([ref.row, ref.col]), ref.value, (SYM_M, SYM_M), "small to_symmetric")
    return out


@pytest.mark.parametrize("shape,route,reduce,kind", [
    ("square", "sort", "sum", "f32"), ("square", "sort", "max", "f32"), ("square", "sort", "sum", "f64"),
    ("square", "sort", "sum", "f32x3"), ("square", "sort", "sum", "none"), ("tall", "sort", "sum", "f32"),
    ("tall", "merge", "sum", "f32"), ("tall", "merge", "max", "f32"), ("tall", "merge", "sum", "f64"),
    ("tall", "merge", "sum", "f32x3")])
@over(big=[b for b in ir.BIG_DIMS if b <= LIMIT])  # the result is big x big: its keys must fit
def test_to_symmetric(big, shape, route, reduce, kind):
    """The union of A and its transpose over keys r * N + c with N = max(M, N) huge: the sort route on a square and
    on a tall matrix, the merge route (A and its CSC view, both sorted) on the tall one, whose column count stays
    small.  phi is the identity on the tall matrix's columns, so one map serves rows and columns of the result."""
    square, tall, _ = symmetric_case()
    index = square if shape == "square" else tall
    small = small_symmetric(shape, route, reduce, kind)
    phi = Phi(SYM_M, big)
    sizes = (big, big) if shape == "square" else (big, SYM_N)
    with bounded_memory():
        out = symmetric_run(map_index(torch.from_numpy(index), phi, phi), symmetric_values(kind, index.shape[1]), sizes,
                            route, reduce)
    check_embedded(out, small, phi, phi, "to_symmetric")


# ---------------------------------------------------------------------------------------------
# cat and its inverse
# ---------------------------------------------------------------------------------------------

CAT = ((100, 90, 700), (80, 110, 600))  # (rows, cols, entries) of the two operands


@functools.lru_cache(maxsize=None)
def cat_case():
    rng = np.random.default_rng(71)
    return tuple((ir.coalesced_index(rng, m, n, nnz), values_of(ir.nonzero_integers(rng, nnz), F32)) for m, n, nnz in CAT)


class Chain:
    """The increasing map of a concatenated dimension: operand i's ids go through its own phi, shifted by the sizes
    of the operands before it (identity shift by the small sizes when nothing is huge)."""

    def __init__(self, smalls, big):
        self.smalls, self.big = smalls, big
        self.phis = [Phi(s, big) for s in smalls]

    def __call__(self, ids):
        ids = np.asarray(cpu(ids) if torch.is_tensor(ids) else ids, dtype=np.int64)
        out, lo, shift = np.empty_like(ids), 0, 0
        for s, phi in zip(self.smalls, self.phis):
            sel = (ids >= lo) & (ids < lo + s)
            out[sel] = phi(ids[sel] - lo).numpy() + shift
            lo, shift = lo + s, shift + phi.size
        return torch.from_numpy(out)

    @property
    def size(self):
        return sum(p.size for p in self.phis)


def small_cat(dim):
    (ia, va), (ib, vb) = cat_case()
    (ma, na, _), (mb, nb, _) = CAT
    out = ps().cat([tensor(ia, va, (ma, na)), tensor(ib, vb, (mb, nb))], dim)
    r0, c0 = (ma if dim in (0, (0, 1)) else 0), (na if dim in (1, (0, 1)) else 0)
    row, col = np.concatenate([ia[0], ib[0] + r0]), np.concatenate([ia[1], ib[1] + c0])
    order = np.lexsort((col, row))
    sizes = (ma + mb if r0 else max(ma, mb), na + nb if c0 else max(na, nb))
    check_small(out, np.stack([row[order], col[order]]), torch.cat([va, vb])[torch.from_numpy(order)], sizes, "small cat")
    return out


@pytest.mark.parametrize("huge", ["rows", "cols", "both"])
@pytest.mark.parametrize("dim", [0, 1, (0, 1)], ids=["dim0", "dim1", "diag"])
@over(big=ir.BIG_DIMS)
def test_cat(big, dim, huge):
    """Stacked rows, stacked columns (the constructor re-sorts on keys row * (N1 + N2) + col) and the block diagonal:
    the second operand's ids are shifted by the first one's huge size."""
    if dim == 1 and huge == "both" and 2 * big * big >= (1 << 63):
        return  # the keys of the re-sort do not fit: the refusal tests have this shape
    (ia, va), (ib, vb) = cat_case()
    (ma, na, _), (mb, nb, _) = CAT
    big_r, big_c = (big if huge != "cols" else None), (big if huge != "rows" else None)
    small = small_cat(dim)
    # a dimension that is concatenated chains the operands' maps; one that is shared maps both through one phi
    rows = Chain((ma, mb), big_r) if dim in (0, (0, 1)) else Phi(max(ma, mb), big_r)
    cols = Chain((na, nb), big_c) if dim in (1, (0, 1)) else Phi(max(na, nb), big_c)
    op_rows = rows.phis if isinstance(rows, Chain) else (rows, rows)
    op_cols = cols.phis if isinstance(cols, Chain) else (cols, cols)
    size = lambda phi, s: s if phi.big is None else phi.big
    with bounded_memory():
        a = tensor(map_index(torch.from_numpy(ia), op_rows[0], op_cols[0]), va, (size(op_rows[0], ma), size(op_cols[0], na)))
        b = tensor(map_index(torch.from_numpy(ib), op_rows[1], op_cols[1]), vb, (size(op_rows[1], mb), size(op_cols[1], nb)))
        out = ps().cat([a, b], dim)
    want_sizes = (rows.size if isinstance(rows, Chain) else max(a.sparse_size(0), b.sparse_size(0)),
                  cols.size if isinstance(cols, Chain) else max(a.sparse_size(1), b.sparse_size(1)))
    assert tuple(out.sparse_sizes()) == want_sizes
    s = small.storage
    for f in FIELDS:
        y = getattr(s, f)
        if f == "_row" and y is not None:
            y = rows(y) if big_r is not None else y
        if f == "_col":
            y = cols(y) if big_c is not None else y
        same(getattr(out.storage, f), y, f"cat {f[1:]}")


@pytest.mark.parametrize("big", BIG)
def test_narrow_diag_inverts_the_block_diagonal(big):
    """__narrow_diag__ hands back each block of cat(dim=(0, 1)) with its caches: rows stay small (it slices the
    rowptr), columns and the column offset of the second block are huge."""
    (ia, va), (ib, vb) = cat_case()
    (ma, na, _), (mb, nb, _) = CAT
    pa, pb = Phi(na, big), Phi(nb, big)
    with bounded_memory():
        a = tensor(map_index(torch.from_numpy(ia), Phi(ma, None), pa), va, (ma, big))
        b = tensor(map_index(torch.from_numpy(ib), Phi(mb, None), pb), vb, (mb, big))
        both = ps().cat([a, b], (0, 1))
        assert tuple(both.sparse_sizes()) == (ma + mb, 2 * big)
        blocks = (both.__narrow_diag__((0, 0), (ma, big)), both.__narrow_diag__((ma, big), (mb, big)))
    for got, src, index, value, m in ((blocks[0], a, ia, va, ma), (blocks[1], b, ib, vb, mb)):
        assert tuple(got.sparse_sizes()) == (m, big)
        same(got.storage._row, torch.from_numpy(index[0]), "block row")
        same(got.storage._col, src.storage._col, "block col")
        same(got.storage._value, value, "block value")
        same(got.storage._rowptr, torch.from_numpy(sr.derived(index[0], index[1], m, max(na, nb)).rowptr), "block rowptr")
        for f in ("_rowcount", "_colptr", "_colcount", "_csr2csc", "_csc2csr"):
            assert getattr(got.storage, f) is None, f"{f} appeared"


# ---------------------------------------------------------------------------------------------
# narrow / select on dim 1, index_select / masked_select, t / transpose
# ---------------------------------------------------------------------------------------------

SM, SN = 100, 120


@functools.lru_cache(maxsize=None)
def slice_case():
    rng = np.random.default_rng(81)
    return ir.coalesced_index(rng, SM, SN, 2400), values_of(ir.nonzero_integers(rng, 2400, (2,)), F64)


@pytest.mark.parametrize("big", [pytest.param(P32 + 7, id="2^32+7"), pytest.param((1 << 40) + 3, id="2^40+3")])
def test_narrow_and_select_columns_beyond_2_32(big):
    """narrow / select on dim 1 with start beyond 2^32: a window inside phi's last block gives the small window's
    result unchanged (columns are relative to start); a window that begins below 2^31 and ends above 2^32 gives the
    masked entries with col - start."""
    index, value = slice_case()
    phi = Phi(SN, big)
    first, stop, image = ir.band_blocks(SN, big)[-1]
    lo = first + max(0, P32 - image)  # the small id whose image is the first at or beyond 2^32
    assert lo + 3 < stop and int(phi(np.array([lo]))[0]) >= P32
    small = tensor(index, value, (SM, SN))
    with bounded_memory():
        t = tensor(map_index(torch.from_numpy(index), Phi(SM, None), phi), value, (SM, big))
        for s, length in ((lo, stop - lo), (lo + 1, 2), (stop - 1, 1)):
            want = small.narrow(1, s, length)
            ref, _ = so.narrow(so.Storage(index[0], index[1], value.numpy(), (SM, SN), True), 1, s, length)
            assert ref.row.size > 0
            check_small(want, np.stack([ref.row, ref.col]), ref.value, (SM, length), "small narrow")
            start = int(phi(np.array([s]))[0])
            got = t.narrow(1, start, length)
            check_embedded(got, want, Phi(SM, None), Phi(length, None), f"narrow({start}, {length})")
            if length == 1:
                check_embedded(t.select(1, start), want, Phi(SM, None), Phi(1, None), f"select({start})")
                check_embedded(t[:, start], want, Phi(SM, None), Phi(1, None), f"[:, {start}]")
        # a window over the band edges: [2^31 - 2, 2^32 + 2)
        start, length = P31 - 2, P32 + 2 - (P31 - 2)
        got = t.narrow(1, start, length)
        cols = phi(index[1])
        keep = (cols >= start) & (cols < start + length)
        assert 0 < int(keep.sum()) < index.shape[1]
        assert tuple(got.sparse_sizes()) == (SM, length)
        same(got.storage.row(), torch.from_numpy(index[0])[keep], "wide narrow row")
        same(got.storage.col(), cols[keep] - start, "wide narrow col")
        same(got.storage.value(), value[keep], "wide narrow value")


@pytest.mark.parametrize("how", ["index", "mask"])
@pytest.mark.parametrize("dim", [0, 1])
@over(big=ir.BIG_DIMS)
def test_index_and_masked_select_on_the_pointered_dimension(big, dim, how):
    """Rows gathered (dim 0) from a matrix with huge columns, columns gathered (dim 1, re-sorted on keys
    row * len(idx) + col) from one with huge rows."""
    index, value = slice_case()
    rng = np.random.default_rng(91)
    size = (SM, SN)[dim]
    if how == "index":
        pick = torch.from_numpy(rng.integers(0, size, 70))  # repeats, any order
        ref, ref_caches = so.index_select(so.Storage(index[0], index[1], value.numpy(), (SM, SN), True), dim, pick.numpy())
    else:
        pick = torch.from_numpy(rng.random(size) < 0.6)
        ref, ref_caches = so.masked_select(so.Storage(index[0], index[1], value.numpy(), (SM, SN), True), dim, pick.numpy())
    run = lambda t: t.index_select(dim, cuda(pick)) if how == "index" else t.masked_select(dim, cuda(pick))
    small = run(tensor(index, value, (SM, SN)))
    kept = int(pick.numel() if how == "index" else pick.sum())
    check_small(small, np.stack([ref.row, ref.col]), ref.value, (kept, SN) if dim == 0 else (SM, kept), "small select")
    for name, want in ref_caches.items():
        same(getattr(small.storage, "_" + name), torch.from_numpy(want), f"small select cache {name}")
    phi_m, phi_n = Phi(SM, big if dim == 1 else None), Phi(SN, big if dim == 0 else None)
    with bounded_memory():
        got = run(tensor(map_index(torch.from_numpy(index), phi_m, phi_n), value, (phi_m.size, phi_n.size)))
    out_m, out_n = (Phi(kept, None), phi_n) if dim == 0 else (phi_m, Phi(kept, None))
    check_embedded(got, small, out_m, out_n, "select")


@pytest.mark.parametrize("big", BIG)
def test_t_and_transpose(big):
    """t() of a matrix with huge rows (its colptr becomes the rowptr of the result) and the function form, which
    coalesces the swapped ids and takes huge sizes on both sides."""
    index, value = slice_case()
    value = value[:, 0].contiguous()
    ref = so.t(so.Storage(index[0], index[1], value.numpy(), (SM, SN), True))
    small = tensor(index, value, (SM, SN)).t()
    check_small(small, np.stack([ref.row, ref.col]), ref.value, (SN, SM), "small t")
    phi = Phi(SM, big)
    with bounded_memory():
        got = tensor(map_index(torch.from_numpy(index), phi, Phi(SN, None)), value, (big, SN)).t()
    check_embedded(got, small, Phi(SN, None), phi, "t")
    for big_m, big_n in ((big, None), (None, big)) + (((big, big),) if big * big < (1 << 63) else ()):
        phi_m, phi_n = Phi(SM, big_m), Phi(SN, big_n)
        with bounded_memory():
            out_index, out_value = ps().transpose(cuda(map_index(torch.from_numpy(index), phi_m, phi_n)), cuda(value),
                                                  phi_m.size, phi_n.size)
        same(out_index, map_index(torch.from_numpy(np.stack([ref.row, ref.col])), phi_n, phi_m), "transpose index")
        same(out_value, torch.from_numpy(ref.value), "transpose value")


# ---------------------------------------------------------------------------------------------
# diagonal ops
# ---------------------------------------------------------------------------------------------

DM, DN = 90, 120


@functools.lru_cache(maxsize=None)
def diag_case():
    """Entries on and around the diagonals 0, 7 and 31, and elsewhere."""
    rng = np.random.default_rng(101)
    cells = set(map(tuple, ir.coalesced_index(rng, DM, DN, 900).T.tolist()))
    for k in (0, 7, 31):
        for r in range(0, DM, 2):
            if 0 <= r + k < DN:
                cells.add((r, r + k))
    index = np.array(sorted(cells), dtype=np.int64).T
    return index, values_of(ir.nonzero_integers(rng, index.shape[1], (2,)), F32)


def ref_diag(index, value, M, N, k, insert, diag_values):
    """remove_diag / set_diag restated: drop (r, r + k), then one entry per cell of the diagonal."""
    row, col = index
    keep = col != row + k
    start, nd = max(-k, 0), max(min(M, N - k) if k >= 0 else min(M + k, N), 0)
    d_rows = np.arange(start, start + nd, dtype=np.int64) if insert else np.zeros(0, np.int64)
    all_row, all_col = np.concatenate([row[keep], d_rows]), np.concatenate([col[keep], d_rows + k])
    order = np.lexsort((all_col, all_row))
    out_value = None
    if value is not None:
        parts = [value[torch.from_numpy(keep)]] + ([diag_values] if insert else [])
        out_value = torch.cat(parts)[torch.from_numpy(order)]
    return np.stack([all_row[order], all_col[order]]), out_value


@pytest.mark.parametrize("with_value", [True, False], ids=["values", "value-less"])
@pytest.mark.parametrize("k", [0, 7, 31])
@over(big=ir.BIG_DIMS[2:])
def test_diagonal_ops_with_offsets_beyond_2_31(big, k, with_value):
    """Columns shifted by S = big - N (phi with the single band "end"), so the k-th diagonal of the small matrix is the
    (k + S)-th of the embedded one, k + S up to 2^32 - 82.  Only k >= 0 embeds this way (a diagonal below the main
    one gains cells left of the shifted block), and an offset beyond -2^31 would need as many rows, i.e. a rowptr
    of that length: excluded by the memory rule."""
    index, value = diag_case()
    value = value if with_value else None
    shift = big - DN
    phi = Phi(DN, big, bands=("end",))
    assert int(phi(np.array([0]))[0]) == shift
    diag_rows = max(min(DM, DN - k) if k >= 0 else min(DM + k, DN), 0)
    dv = values_of(ir.nonzero_integers(np.random.default_rng(7), diag_rows, (2,)), F32)
    small_t = tensor(index, value, (DM, DN))
    with bounded_memory():
        big_t = tensor(map_index(torch.from_numpy(index), Phi(DM, None), phi), value, (DM, big))
        for name, insert, call in (("remove_diag", False, lambda t, kk: t.remove_diag(kk)),
                                   ("set_diag", True, lambda t, kk: t.set_diag(cuda(dv) if with_value else None, kk)),
                                   ("fill_diag", True, lambda t, kk: t.fill_diag(3, kk))):
            fill = dv if name == "set_diag" else torch.full_like(dv, 3)
            ref_index, ref_value = ref_diag(index, value, DM, DN, k, insert, fill)
            small = call(small_t, k)
            check_small(small, ref_index, ref_value, (DM, DN), f"small {name}")
            got = call(big_t, k + shift)
            check_embedded(got, small, Phi(DM, None), phi, name)
        # an offset past the last column has no cell: nothing changes
        same(big_t.remove_diag(big).storage.col(), big_t.storage.col(), "remove_diag(k = N)")


@pytest.mark.parametrize("big", BIG)
def test_get_diag_of_a_matrix_with_huge_columns(big):
    """The main diagonal of an M x N matrix, N huge: entry (r, c') lies on it only when phi(c) == r."""
    index, value = diag_case()
    phi = Phi(DN, big)
    cols = phi(index[1])
    want = torch.zeros((DM,) + tuple(value.shape[1:]), dtype=value.dtype)
    hit = torch.from_numpy(index[0]) == cols
    assert 0 < int(hit.sum()) < int((torch.from_numpy(index[0]) == torch.from_numpy(index[1])).sum())
    want[torch.from_numpy(index[0])[hit]] = value[hit]
    with bounded_memory():
        t = tensor(torch.stack([torch.from_numpy(index[0]), cols]), value, (DM, big))
        same(t.get_diag(), want, "get_diag")
        bare = tensor(torch.stack([torch.from_numpy(index[0]), cols]), None, (DM, big))
        same(bare.get_diag(), (want[:, 0] != 0).to(F32), "get_diag of a value-less matrix")


# ---------------------------------------------------------------------------------------------
# refusals at the int64 limit
# ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tiny():
    """A handful of entries that lie inside every refused shape (and every part of one)."""
    index = torch.tensor([[0, 1, 1, 5, 7], [3, 0, 2, 2, 9]], dtype=I64)
    return cuda(index), cuda(torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0]))


@pytest.mark.parametrize("m,n", OVER)
def test_refusals_of_the_functions(m, n):
    index, value = tiny()
    shuffled = index[:, [3, 0, 4, 1, 2]].contiguous()
    refused(lambda: ps().coalesce(shuffled, value, m, n), m, n)
    refused(lambda: ps().coalesce(shuffled, None, m, n, "max"), m, n)
    refused(lambda: ps().transpose(index, value, n, m), m, n)
    refused(lambda: ops().coalesce_chain(shuffled[0].contiguous(), shuffled[1].contiguous(), value, m, n), m, n,
            "coalesce_chain")
    refused(lambda: ops().coalesce_small(shuffled[0].contiguous(), shuffled[1].contiguous(), m, n), m, n,
            "coalesce_small")
    refused(lambda: ops().make_keys_checked(index[0].contiguous(), index[1].contiguous(), m, n), m, n,
            "make_keys_checked")
    small_b = torch.tensor([[0, 2, 3], [0, 1, 9]], dtype=I64).cuda()
    b_value = torch.tensor([1.0, 2.0, 3.0]).cuda()
    for va, vb in ((value, b_value), (value.double(), b_value.double()), (None, None),
                   (value.clone().requires_grad_(True), b_value)):
        refused(lambda: ps().spspmm(index[:, :4].contiguous(), None if va is None else va[:4], small_b, vb, m, 4, n), m, n)


@pytest.mark.parametrize("m,n", OVER)
def test_refusals_of_the_tensor_ops(m, n):
    index, value = tiny()
    a = ps().SparseTensor(row=index[0], col=index[1], value=value, sparse_sizes=(m, n), is_sorted=True)
    b = ps().SparseTensor(row=index[0, :3], col=index[1, :3], value=value[:3], sparse_sizes=(5, n), is_sorted=True)
    with threshold("add", "_ONE_WORKGROUP_BELOW", 0):
        refused(lambda: ps().add(a, b), m, n)
    refused(lambda: ps().add(b, a), m, n)
    refused(lambda: ps().mul(a, b), m, n)
    refused(lambda: a.is_coalesced(), m, n)
    refused(lambda: a.coalesce(), m, n)
    side = max(m, n)
    refused(lambda: a.to_symmetric(), side, side)
    if n * n >= (1 << 63):  # the merge route, on a matrix whose column count alone is too large
        with threshold("tensor", "_MERGE_ABOVE", 0):
            refused(lambda: b.to_symmetric("max"), n, n)
    # the constructor's own sort
    refused(lambda: ps().SparseTensor(row=index[0].flip(0), col=index[1].flip(0), value=value, sparse_sizes=(m, n)), m, n)
    # cat along dim 1 re-sorts on keys row * (N1 + N2) + col
    half = ps().SparseTensor(row=index[0], col=index[1], value=value, sparse_sizes=(m, n - n // 2), is_sorted=True)
    other = ps().SparseTensor(row=index[0, :3], col=index[1, :3], value=value[:3], sparse_sizes=(5, n // 2), is_sorted=True)
    refused(lambda: ps().cat([half, other], 1), m, n)


def test_index_select_refuses_keys_past_2_63():
    """index_select(dim=1) re-sorts on keys row * len(idx) + col: 2^31 rows and 2^32 selected columns.  The index is
    a zero-stride view of one element, so that the refusal has to come before anything of its length is built."""
    index, value = tiny()
    t = ps().SparseTensor(row=index[0], col=index[1], value=value, sparse_sizes=(P31, P31), is_sorted=True)
    idx = torch.zeros(1, dtype=I64, device="cuda").expand(P32)
    assert idx.numel() == P32
    refused(lambda: t.index_select(1, idx), P31, P32)
