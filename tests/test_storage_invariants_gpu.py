"""Audit of every derived cache and private memo of SparseStorage after every op that hands them over.

Many ops do not let their result rebuild its caches lazily: they slice, shift, swap or concatenate the
operand's caches and construct the result with is_sorted=True, trust_data=True, so nothing validates
them — and a wrong cache does not crash, it is read later by t(), csc(), sum(dim=0) and the SpMM
backward over the CSC view.  `audit` compares, for the result of an op,

  1. every field the op LEFT (public caches and private memos, read as attributes before any accessor
     runs) with the plain numpy reference of tests/storage_ref.py, np.array_equal;
  2. the set of public caches present with the set the op's code says it keeps (EXPECT below, per op and
     operand state) — set equality, so no comparison of step 1 is skipped because a field is absent
     unless the table says it is absent;
  3. the same fields again after every lazy builder has run on top of what the op left;
  4. the downstream consumers (csc(), t(), sum / max over a dim, SpMM forward and both gradients for
     sum / mean / max at K = 32) against a `cold` tensor built from copies of the result's coo() —
     torch.equal on exact integer data — with `cold` itself checked against tests/exact_ref.py.

Every op runs with its operand(s) cold (no caches), warm (fill_cache_()) and hot (warm + every private
memo built), and the result must be the same entries and values in all three.

Operand values are small integers, so every fp32 sum is exact in any order (the bound is asserted as in
test_exact_spmm_gpu.py).  The one inexact consumer is the mean backward on rows whose degree is not a
power of two: `t` against `cold` is still bit for bit (same kernels, same structure, same plan state),
`cold` against the float64 reference is held to the rounding bound written out in `_mean_backward_bound` —
and compared exactly wherever every row degree is a power of two (test_mean_backward_exact_on_power_of_two_degrees).

Above 2^20 entries the hand-over ops run with cold, warm and hot operands through steps 1 - 3 and the equality of
the results; step 4 runs there for the hot operand only (the one whose memos an op could have mishandled) and
without the float64 reference except once, on the operand itself: the small size has already held the same code
to it, and a CPU reference of a 10^6-entry SpMM costs seconds per case.
"""
import numpy as np
import pytest
import scipy.sparse
import torch

from exact_ref import assert_exact_preconditions, integers, pow2_degrees, spmm_backward_ref, spmm_ref
from storage_ref import derived

pytestmark = pytest.mark.gpu

CACHES = ("rowcount", "colptr", "colcount", "csr2csc", "csc2csr")
ALL = frozenset(CACHES)
NONE = frozenset()
STATES = ("cold", "warm", "hot")
KINDS = ("f32", "f32x3", "i64", None)
K = 32


@pytest.fixture(scope="module", autouse=True)
def _small_hot_columns():
    """storage.HOT_COLUMNS lowered for this module, so that the power-law test matrices get a `_hot_memo`."""
    import paddle_sparse_amd.storage as st_mod

    old, st_mod.HOT_COLUMNS = st_mod.HOT_COLUMNS, 64
    yield
    st_mod.HOT_COLUMNS = old


def host(x):
    return x.detach().cpu().numpy()


def dev(a, dtype=torch.int64):
    return torch.as_tensor(np.asarray(a), dtype=dtype).cuda()


# ---------------------------------------------------------------------------------------------
# matrices
# ---------------------------------------------------------------------------------------------

def power_law(M, N, special=(0, 1, 129, 300), seed=0, tail=6, hole=(200, 216), typical=4, pow2=False):
    """(row, col) int64 numpy of a coalesced M x N matrix in row-major order: the first rows have
    `special` entries (0, 1, 129, 300: one- and two-byte edge tags both occur), the last `tail` rows none,
    the rest 0 .. typical (mostly 0 - 2, so the matrix takes the edge-range SpMM); columns are drawn with
    Zipf weights (hub columns), none from [hole) and none from the last `tail` columns."""
    rng = np.random.default_rng(seed)
    allowed = np.array([c for c in range(N - tail) if not hole[0] <= c < hole[1]])
    p = 1.0 / (1.0 + rng.permutation(allowed.size))
    p /= p.sum()
    deg = rng.choice(typical + 1, M, p=np.array([4, 3, 2] + [1] * (typical - 2), float) / (9 + typical - 2))
    deg[:len(special)] = special
    deg[M - tail:] = 0
    if pow2:  # every degree rounded down to a power of two: the mean backward is then exact as well
        deg = pow2_degrees(deg)
    rows, cols = [], []
    for r in range(M):
        if deg[r]:
            rows.append(np.full(deg[r], r))
            cols.append(np.sort(rng.choice(allowed, deg[r], replace=False, p=p)))
    return np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64)


def big_power_law(M=1 << 18, N=1 << 17, nnz=(1 << 20) + 4096, seed=0, huge_row=0, at_least=1 << 20):
    """Vectorised power-law matrix just above 2^20 entries (duplicates removed, so slightly fewer are drawn
    and `nnz` is over-asked): Zipf-like rows and columns; `huge_row` > 0 makes row 5 that long."""
    rng = np.random.default_rng(seed)
    n = int(nnz * 1.35)
    r = np.minimum((M * rng.random(n) ** 3).astype(np.int64), M - 1)
    c = np.minimum((N * rng.random(n) ** 3).astype(np.int64), N - 1)
    key = r * N + c
    if huge_row:
        key = np.concatenate([key, 5 * N + rng.choice(N, huge_row, replace=False)])
    key = np.unique(key)
    if key.size > nnz and not huge_row:
        key = np.sort(rng.choice(key, nnz, replace=False))
    assert key.size >= at_least
    return key // N, key % N


def values(kind, nnz, seed=0):
    if kind is None:
        return None
    if kind == "f32":
        return integers(nnz, -3, 3, torch.float32, seed)
    if kind == "f32x3":
        return integers((nnz, 3), -3, 3, torch.float32, seed)
    return integers(nnz, -3, 3, torch.int64, seed)


def heat(t):
    """Every private memo of t.storage built: SpMM forward + backward with tracked values for sum, mean and max
    on the storage itself, then csc() and t()."""
    from paddle_sparse_amd.matmul import _SpMM

    st = t.storage
    M, N = st.sparse_sizes()
    if M > 0 and N > 0:
        for i, reduce in enumerate(("sum", "mean", "max")):
            v = integers(st.col().numel(), -3, 3, torch.float32, 40 + i).cuda().requires_grad_()
            B = integers((N, K), -8, 8, torch.float32, 50 + i).cuda().requires_grad_()
            _SpMM.apply(v, B, st, reduce, True).backward(integers((M, K), -8, 8, torch.float32, 60 + i).cuda())
    t.csc()
    t.t()
    st._csc_view()
    st._mean_scale_per_entry()
    st._csc_edge_tags(1)
    st._csc_edge_tags(2)
    return t


def make(row, col, sizes, kind=None, state="cold", seed=0, layout="row", value=None):
    """SparseTensor over copies of (row, col) in the given state.  layout: built from `row`, from `rowptr`
    alone, or from both."""
    from paddle_sparse_amd import SparseTensor

    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    value = values(kind, row.size, seed) if value is None else value
    rowptr = np.searchsorted(row, np.arange(sizes[0] + 1), side="left")
    t = SparseTensor(row=dev(row) if layout in ("row", "both") else None,
                     rowptr=dev(rowptr) if layout in ("rowptr", "both") else None, col=dev(col),
                     value=None if value is None else value.clone().cuda(), sparse_sizes=tuple(sizes), is_sorted=True)
    if state in ("warm", "hot"):
        t.fill_cache_()
    if state == "hot":
        heat(t)
    return t


# ---------------------------------------------------------------------------------------------
# the audit
# ---------------------------------------------------------------------------------------------

def present(st):
    return frozenset(k for k in CACHES if getattr(st, "_" + k) is not None)


def _entries(st):
    """(row, col) of a storage on the host WITHOUT calling an accessor: `_row` as left, or expanded from `_rowptr`."""
    col = host(st._col)
    if st._row is not None:
        return host(st._row), col
    rowptr = host(st._rowptr)
    return np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr)), col


def check_fields(st, d, where, depth=0):
    """Every non-None derived field and memo of `st` against the reference `d`.  Reads attributes only."""
    from paddle_sparse_amd import ops

    def same(name, got, want):
        got = host(got)
        assert got.dtype == want.dtype, f"{where}: {name} is {got.dtype}, expected {want.dtype}"
        assert got.shape == want.shape, f"{where}: {name} has shape {got.shape}, expected {want.shape}"
        assert np.array_equal(got, want), f"{where}: {name} differs from the reference at {np.flatnonzero(got != want)[:5]}"

    assert tuple(st._sparse_sizes) == (d.M, d.N), where
    for name, want in (("_row", d.row), ("_rowptr", d.rowptr), ("_col", d.col), ("_rowcount", d.rowcount),
                       ("_colptr", d.colptr), ("_colcount", d.colcount), ("_csr2csc", d.csr2csc),
                       ("_csc2csr", d.csc2csr), ("_row_csc", d.row_csc), ("_mean_scale_memo", d.mean_scale)):
        got = getattr(st, name, None)
        if got is not None:
            same(name, got, want)
    if st._edge_tags:
        for width, tag in st._edge_tags.items():
            same(f"_edge_tags[{width}]", tag, d.edge_tags(width))
    if st._max_rowcount is not None:
        assert st._max_rowcount == d.longest_row, f"{where}: _max_rowcount"
    if st._spmm_algo_memo is not None:
        # storage._spmm_algo: edge ranges once rows of at most two entries are more than 40 % of the rows
        want = "edge_ranges" if 5 * int((d.rowcount <= 2).sum()) > 2 * d.M else "row_waves"
        assert st._spmm_algo_memo == want, f"{where}: _spmm_algo_memo"
    memo = st._value_csc_memo
    if memo is not None and memo[0] is st._value and memo[1] == st._value._version and memo[2]._version == memo[3]:
        same("_value_csc_memo", memo[2], host(st._value)[d.csr2csc])
    view = st._csc_view_memo
    if view is not None:
        # the CSR storage of the transpose: rowptr = colptr, col = row[csr2csc], colcount = rowcount
        assert view._rowptr is not None and view._colcount is not None, f"{where}: _csc_view_memo lost its arrays"
        assert depth == 0, f"{where}: a CSC view with a CSC view of its own"
        check_fields(view, derived(d.col_csc, d.row_csc, d.N, d.M), where + " / _csc_view_memo", depth + 1)
    for direction, plan in (getattr(st, "_perm_plans", None) or {}).items():
        if isinstance(direction, str):
            ids = torch.arange(d.nnz, dtype=torch.int32, device=st._col.device)
            want = d.csr2csc if direction == "to_csc" else d.csc2csr
            same(f"_perm_plans[{direction}]", ops.permute_apply(ids, plan), want.astype(np.int32))
    hot = st._hot_memo
    if hot:
        ids, col_eff = host(hot[0]), host(hot[1])
        assert np.unique(ids).size == ids.size and (ids >= 0).all() and (ids < d.N).all(), f"{where}: _hot_memo ids"
        back = np.where(col_eff >= d.N, ids[np.clip(col_eff - d.N, 0, ids.size - 1)], col_eff)
        assert col_eff.shape == d.col.shape and (col_eff < d.N + ids.size).all(), f"{where}: _hot_memo range"
        assert np.array_equal(back, d.col), f"{where}: _hot_memo does not map back to col"
        assert not np.isin(col_eff[col_eff < d.N], ids).any(), f"{where}: a reference to a hot column was not redirected"
    huge = getattr(st, "_huge_memo", None)
    if huge:
        cut = ops.ARG_WORDS_EXACT_ROW
        rows = np.flatnonzero(d.rowcount > cut)
        same("_huge_memo.rows", huge["rows"], rows)
        same("_huge_memo.start", huge["start"], d.rowptr[rows])
        ids = np.concatenate([np.arange(d.rowptr[r], d.rowptr[r + 1]) for r in rows]).astype(np.int64)
        same("_huge_memo.ids", huge["ids"], ids)
        same("_huge_memo.col", huge["col"], d.col[ids])
        per = (d.rowcount[rows] + cut - 1) // cut
        same("_huge_memo.piece_ptr", huge["piece_ptr"], np.concatenate([[0], np.cumsum(per)]).astype(np.int64))
        same("_huge_memo.piece_row", huge["piece_row"], np.repeat(np.arange(rows.size, dtype=np.int64), per))
        lens = np.concatenate([np.minimum(cut, d.rowcount[r] - cut * np.arange(n)) for r, n in zip(rows, per)])
        same("_huge_memo.rowptr", huge["rowptr"], np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    bw = getattr(st, "_huge_bw_memo", None)
    if bw:
        # (ids_ext, row_eff, tags, P): a CSC entry of a huge row points at its piece, the others at their row or
        # at a hub-row copy; every id in ids_ext names the row a reference M + j stands for
        ids_ext, row_eff, tags, P = host(bw[0]), host(bw[1]), host(bw[2]), bw[3]
        cut = ops.ARG_WORDS_EXACT_ROW
        back = np.where(row_eff >= d.M, ids_ext[np.clip(row_eff - d.M, 0, ids_ext.size - 1)], row_eff)
        assert np.array_equal(back, d.row_csc), f"{where}: _huge_bw_memo does not map back to row[csr2csc]"
        local = d.csr2csc - d.rowptr[d.row_csc]
        is_huge = d.rowcount[d.row_csc] > cut
        want = np.where(is_huge, local % cut, local & 0xffff).astype(np.uint16).view(np.int16)
        assert np.array_equal(tags, want), f"{where}: _huge_bw_memo tags"
        # an entry of a huge row points at ITS piece: behind the M rows and the h hub rows, piece local // cut of the row
        rows = np.flatnonzero(d.rowcount > cut)
        per = (d.rowcount[rows] + cut - 1) // cut
        piece_ptr = np.concatenate([[0], np.cumsum(per)])
        slot = np.searchsorted(rows, d.row_csc[is_huge])
        h = ids_ext.size - P
        assert np.array_equal(row_eff[is_huge], d.M + h + piece_ptr[slot] + local[is_huge] // cut), \
            f"{where}: _huge_bw_memo sends an entry of a huge row to the wrong piece"
        assert np.array_equal(ids_ext[h:], np.repeat(rows, per)), f"{where}: _huge_bw_memo piece rows"
        assert P == int(((d.rowcount[d.rowcount > cut] + cut - 1) // cut).sum()), f"{where}: _huge_bw_memo pieces"


def _top(x):
    return float(x.max()) if x.numel() else 0.0


def _spmm_all(x, w, mat, grad, reduce):
    v = w.clone().cuda().requires_grad_()
    B = mat.clone().cuda().requires_grad_()
    out = x.set_value(v, layout="coo").matmul(B, reduce)
    out.backward(grad.cuda())
    return out.detach(), v.grad, B.grad


def _mean_backward_bound(d, w, mat, grad):
    """|kernel - float64 reference| allowed for the mean backward.  The kernels multiply by fl(1 / deg) (relative
    error u = 2^-24) where the reference divides, and round every product and partial sum to fp32; the terms
    themselves are exact integers.  grad_value[e] = (sum_k mat[col, k] grad[row, k]) / deg is a K-term sum:
    (K + 4) u sum |terms| / deg covers it in any association; grad_mat[c, k] = sum over the n_c entries of column c
    of w grad[row, k] / deg: (n_c + 4) u sum |terms| likewise (Higham, Accuracy and Stability, (3.5), n u bound)."""
    u = 2.0 ** -24
    row, col = torch.from_numpy(d.row), torch.from_numpy(d.col)
    inv = 1.0 / torch.from_numpy(np.maximum(d.rowcount, 1)).double()[row]
    b, g = mat.double().abs(), grad.double().abs()
    gv = (K + 4) * u * (b[col] * g[row]).sum(1) * inv
    terms = torch.zeros(d.N, K, dtype=torch.float64).index_add_(0, col, (w.double().abs() * inv)[:, None] * g[row])
    gm = (torch.from_numpy(d.colcount).double()[:, None] + 4) * u * terms
    return gv, gm


def downstream(t, d, where, check_ref=True, seed=0):
    """Step 4: `t` (with whatever the op and the lazy builders left) against `cold`, a tensor built from copies
    of its coo() with no caches; `cold` against the exact reference."""
    from paddle_sparse_amd import SparseTensor

    row, col, value = t.coo()
    cold = SparseTensor(row=row.clone(), col=col.clone(), value=None if value is None else value.detach().clone(),
                        sparse_sizes=t.sparse_sizes())
    assert present(cold.storage) == NONE

    def eq(name, a, b):
        assert (a is None) == (b is None), f"{where}: {name}: one side has no values"
        if a is not None:
            assert a.dtype == b.dtype and torch.equal(a, b), f"{where}: {name} differs between the result and a cold rebuild"

    for name, a, b in zip(("row", "col", "value"), t.coo(), cold.coo()):
        eq(f"coo {name}", a, b)
    for name, a, b in zip(("colptr", "row", "value"), t.csc(), cold.csc()):
        eq(f"csc() {name}", a, b)
    for name, a, b in zip(("row", "col", "value"), t.t().coo(), cold.t().coo()):
        eq(f"t().coo() {name}", a, b)
    eq("t().csr() rowptr", t.t().csr()[0], cold.t().csr()[0])
    # reference of the reductions: every sum is an integer far below 2^24
    dense_v = None if value is None else value.detach().cpu().double()
    for dim, index, size in ((0, d.col, d.N), (1, d.row, d.M)):
        got = t.sum(dim=dim)
        eq(f"sum(dim={dim})", got, cold.sum(dim=dim))
        if dense_v is None:
            want = torch.from_numpy(np.bincount(index, minlength=size)[:size]).double()
        else:
            shape = (size,) + tuple(dense_v.shape[1:])
            want = torch.zeros(shape, dtype=torch.float64).index_add_(0, torch.from_numpy(index), dense_v)
            top = torch.zeros(shape, dtype=torch.float64).index_add_(0, torch.from_numpy(index), dense_v.abs())
            assert _top(top) < 2 ** 24, "the reduction's sums must stay exact in fp32"
        assert torch.equal(got.cpu().double(), want), f"{where}: sum(dim={dim}) differs from the reference"
    if value is not None:
        eq("max(dim=0)", t.max(dim=0), cold.max(dim=0))
    M, N = d.M, d.N
    if M == 0 or N == 0:
        return  # a product with an empty dimension has no dense operand or no output
    w = integers(d.nnz, -3, 3, torch.float32, seed + 1)
    mat = integers((N, K), -8, 8, torch.float32, seed + 2)
    grad = integers((M, K), -8, 8, torch.float32, seed + 3)
    rowptr, colh = torch.from_numpy(d.rowptr), torch.from_numpy(d.col)
    nz = d.rowcount[d.rowcount > 0]
    pow2 = bool(((nz & (nz - 1)) == 0).all())  # then the mean backward is exact too (tests/exact_ref.py)
    if check_ref:
        assert_exact_preconditions(rowptr, colh, w, mat, grad)
        if pow2:
            assert_exact_preconditions(rowptr, colh, w, mat, grad, mean_backward=True)
    # same plan state on both sides: above ops.PERMUTE_PLAN_FROM the mean backward folds 1 / deg into the weights
    # only when both planned routes exist, and step 3 has built them on `t`
    for direction in ("to_csc", "to_csr"):
        cold.storage._permute_plan(direction, force=True)
    for reduce in ("sum", "mean", "max"):
        got, ref = _spmm_all(t, w, mat, grad, reduce), _spmm_all(cold, w, mat, grad, reduce)
        for name, a, b in zip(("out", "grad_value", "grad_mat"), got, ref):
            eq(f"SpMM {reduce} {name}", a, b)
        if not check_ref:
            continue
        out, arg = spmm_ref(reduce, rowptr, colh, w, mat)
        assert torch.equal(ref[0].cpu(), out), f"{where}: cold SpMM {reduce} forward differs from the exact reference"
        if reduce == "mean" and not pow2:
            # rows whose degree is not a power of two: 1 / deg is rounded, the float64 reference is met within the bound
            w64, m64, g64 = w.double(), mat.double(), grad.double()
            rows = torch.from_numpy(d.row)
            inv = 1.0 / torch.from_numpy(np.maximum(d.rowcount, 1)).double()[rows]
            gv64 = (m64[colh] * g64[rows]).sum(1) * inv
            gm64 = torch.zeros(N, K, dtype=torch.float64).index_add_(0, colh, (w64 * inv)[:, None] * g64[rows])
            tv, tm = _mean_backward_bound(d, w, mat, grad)
            ev, em = (ref[1].cpu().double() - gv64).abs(), (ref[2].cpu().double() - gm64).abs()
            assert bool((ev <= tv).all()) and bool((em <= tm).all()), \
                f"{where}: cold SpMM mean backward outside the bound: grad_value {_top(ev):.3e}, grad_mat {_top(em):.3e}"
        else:
            gv, gm = spmm_backward_ref(reduce, rowptr, colh, w, mat, grad, arg)
            assert torch.equal(ref[1].cpu(), gv), f"{where}: cold SpMM {reduce} grad_value differs from the exact reference"
            assert torch.equal(ref[2].cpu(), gm), f"{where}: cold SpMM {reduce} grad_mat differs from the exact reference"


def audit(t, expect_present, where, check_ref=True, run_downstream=True):
    st = t.storage
    row, col = _entries(st)  # as left: no accessor has run
    M, N = st._sparse_sizes
    d = derived(row, col, M, N)
    assert d.sorted, f"{where}: the result is not in row-major order"
    if st._value is not None:
        assert st._value.shape[0] == d.nnz, where
    check_fields(st, d, where + " [as left]")                                   # 1
    assert present(st) == frozenset(expect_present), \
        f"{where}: caches present {sorted(present(st))}, the op keeps {sorted(expect_present)}"  # 2
    t.fill_cache_()                                                               # 3
    st._row_in_csc_order()
    st._csc_edge_tags(1)
    st._csc_edge_tags(2)
    st._longest_row()
    st._csc_view()
    st._mean_scale_per_entry()
    st._spmm_algo()
    for direction in ("to_csc", "to_csr"):
        st._permute_plan(direction, force=True)
    assert st._row is not None and st._rowptr is not None and present(st) == ALL and st._row_csc is not None
    assert set(st._edge_tags) == {1, 2} and st._csc_view_memo is not None and st._mean_scale_memo is not None
    check_fields(st, d, where + " [after the lazy builders]")
    if run_downstream:
        downstream(t, d, where, check_ref=check_ref)                              # 4
    return d


def same_result(results, where):
    """The op's result over the operand states: same sizes, entries and values."""
    first = results[0]
    for other in results[1:]:
        assert other.sparse_sizes() == first.sparse_sizes(), where
        for name, a, b in zip(("row", "col", "value"), first.coo(), other.coo()):
            assert (a is None) == (b is None), f"{where}: {name}"
            if a is not None:
                assert a.dtype == b.dtype and torch.equal(a, b), f"{where}: {name} depends on the operand's caches"


def run(op, operand, expect, where, kinds=KINDS, states=STATES, downstream_kinds=("f32", None)):
    """op(t) for the operand in every state and with every kind of value; expect[state] = the caches the op keeps.
    Steps 1 - 3 run for every combination; step 4 for the kinds in `downstream_kinds` (the consumers read the
    structure, and values of each kind through csc() / t() / the reductions), the exact reference once per op."""
    for kind in kinds:
        results = []
        for state in states:
            out = op(operand(kind, state))
            tag = f"{where} [{kind}, {state}]"
            audit(out, expect[state], tag, check_ref=(kind == kinds[0] and state == "hot"),
                  run_downstream=kind in downstream_kinds or state == "hot")
            results.append(out)
        same_result(results, f"{where} [{kind}]")


def by_state(cold, warm, hot=None):
    return {"cold": frozenset(cold), "warm": frozenset(warm), "hot": frozenset(warm if hot is None else hot)}


# ---------------------------------------------------------------------------------------------
# small size: the whole op list
# ---------------------------------------------------------------------------------------------

M0, N0 = 400, 1200


@pytest.fixture(scope="module")
def base():
    return power_law(M0, N0, seed=3)


def operand_of(base, sizes=(M0, N0), layout="row"):
    row, col = base
    return lambda kind, state: make(row, col, sizes, kind, state, seed=7, layout=layout)


def test_operand_states_themselves(base):
    """The three operand states pass the audit before any op: cold has nothing, warm has the five caches, hot
    has every memo (and the small matrix takes the edge-range SpMM with a hub-column copy)."""
    op = operand_of(base)
    for kind in KINDS:
        for state in STATES:
            t = op(kind, state)
            st = t.storage
            if state == "hot":
                assert st._row_csc is not None and set(st._edge_tags) == {1, 2} and st._max_rowcount == 300
                assert st._spmm_algo_memo == "edge_ranges" and st._hot_memo, "the test matrix must have hub columns"
                assert st._csc_view_memo is not None and st._mean_scale_memo is not None
            audit(t, NONE if state == "cold" else ALL, f"operand [{kind}, {state}]", check_ref=(state == "hot" and kind == "f32"))


def test_mean_backward_exact_on_power_of_two_degrees():
    """Every row degree a power of two (0, 1, 128, 256 and 0 - 4): 1 / deg is exact, so the cold rebuild's mean
    backward is compared with the float64 reference bit for bit (downstream takes that branch by itself), on the
    operand and on the ops that keep whole rows."""
    p2 = power_law(M0, N0, special=(0, 1, 128, 256), seed=5, pow2=True)
    deg = np.bincount(p2[0], minlength=M0)
    assert np.array_equal(deg, pow2_degrees(deg)) and deg.max() == 256
    op = operand_of(p2)
    for state in STATES:
        audit(op("f32", state), NONE if state == "cold" else ALL, f"power-of-two operand [{state}]")
    run(lambda t: t.narrow(0, 1, 300), op, by_state(NONE, {"rowcount"}), "narrow(0) of power-of-two rows", kinds=("f32",))
    sel = np.concatenate([np.arange(M0)[::-1], [2, 3, 3]])
    run(lambda t: t.index_select(0, dev(sel)), op, by_state({"rowcount"}, {"rowcount"}), "index_select(0) of power-of-two rows",
        kinds=("f32",))
    run(lambda t: t.set_value(values("f32", t.nnz(), 3).cuda(), layout="csc"), op,
        by_state({"colptr", "csr2csc", "csc2csr"}, ALL), "set_value of power-of-two rows", kinds=("f32",))
    run(lambda t: t.sparse_resize((M0 + 9, N0 + 9)), op, by_state(NONE, ALL), "sparse_resize of power-of-two rows", kinds=("f32",))


@pytest.mark.parametrize("layout", ["row", "rowptr"])
def test_t(base, layout):
    # A^T keeps rowcount <- colcount, colptr <- rowptr, colcount <- rowcount, csr2csc <- csc2csr; csc2csr is the
    # sort t() itself runs.  A cold operand built from `row` has no rowptr to hand over, one built from `rowptr` has.
    cold = {"csc2csr"} | ({"colptr"} if layout == "rowptr" else set())
    run(lambda t: t.t(), operand_of(base, layout=layout), by_state(cold, ALL), f"t() of a {layout}-built operand")
    # t().t(): the first t() leaves csc2csr and the implicit rowptr; the second swaps them and sorts again
    run(lambda t: t.t().t(), operand_of(base, layout=layout), by_state({"colptr", "csr2csc", "csc2csr"}, ALL),
        f"t().t() of a {layout}-built operand")


NARROW0 = [(0, 0, 50), (0, 120, 100), (0, 330, 70), (0, 17, 0), (0, M0 - 6, 6), (0, 2, 2), (0, 0, M0)]
NARROW1 = [(1, 0, 300), (1, 100, 500), (1, 900, 300), (1, 40, 0), (1, 200, 16), (1, N0 - 6, 6), (1, 0, N0)]


@pytest.mark.parametrize("dim,start,length", NARROW0 + NARROW1)
def test_narrow(base, dim, start, length):
    # start 0, interior, to the end, length 0, a range of only empty rows / columns, rows 2 - 3 (129 and 300 entries)
    keeps = {"rowcount"} if dim == 0 else {"colptr", "colcount"}
    run(lambda t: t.narrow(dim, start, length), operand_of(base), by_state(NONE, keeps),
        f"narrow({dim}, {start}, {length})")


def test_narrow_of_a_rowptr_built_operand(base):
    run(lambda t: t.narrow(0, 1, 150), operand_of(base, layout="rowptr"), by_state(NONE, {"rowcount"}), "narrow(0) rowptr-built")


@pytest.mark.parametrize("dim,idx", [(0, 3), (0, 0), (0, M0 - 1), (1, 0), (1, 205), (1, N0 - 1)])
def test_select(base, dim, idx):
    keeps = {"rowcount"} if dim == 0 else {"colptr", "colcount"}
    run(lambda t: t.select(dim, idx), operand_of(base), by_state(NONE, keeps), f"select({dim}, {idx})")


def _selections(size, hole, seed):
    rng = np.random.default_rng(seed)
    some = rng.integers(0, size, 150)
    return {"duplicates": np.concatenate([some, some[:40], [2, 3, 3, 2]]), "reversed": np.arange(size)[::-1].copy(),
            "empty": np.zeros(0, np.int64), "only empty": np.arange(*hole), "all": np.arange(size)}


@pytest.mark.parametrize("name", ["duplicates", "reversed", "empty", "only empty", "all"])
@pytest.mark.parametrize("dim", [0, 1])
def test_index_select(base, dim, name):
    # dim 0 hands over rowcount, dim 1 colptr, colcount and the csc2csr of its sort — whatever the operand holds
    idx = _selections((M0, N0)[dim], ((M0 - 6, M0), (200, 216))[dim], 5)[name]
    keeps = {"rowcount"} if dim == 0 else {"colptr", "colcount", "csc2csr"}
    run(lambda t: t.index_select(dim, dev(idx)), operand_of(base), by_state(keeps, keeps),
        f"index_select({dim}, {name})")


@pytest.mark.parametrize("which", ["none", "all", "some"])
@pytest.mark.parametrize("dim", [0, 1])
def test_masked_select(base, dim, which):
    size = (M0, N0)[dim]
    mask = {"none": np.zeros(size, bool), "all": np.ones(size, bool), "some": np.random.default_rng(2).random(size) < 0.4}[which]
    keeps = {"rowcount"} if dim == 0 else {"colptr", "colcount", "csc2csr"}
    run(lambda t: t.masked_select(dim, torch.from_numpy(mask).cuda()), operand_of(base), by_state(keeps, keeps),
        f"masked_select({dim}, {which})")


def _blocks(seed=0):
    """Three operands for cat: different heights and widths, the middle one without entries."""
    a = power_law(120, 300, special=(0, 1, 129), seed=seed, hole=(50, 60))
    b = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    c = power_law(90, 400, special=(300, 0, 2), seed=seed + 1, hole=(100, 140))
    return [(a, (120, 300)), (b, (40, 70)), (c, (90, 400))]


def _cat_operands(blocks, kind, states, layouts):
    return [make(r, c, s, kind, state, seed=11 + i, layout=layout)
            for i, (((r, c), s), state, layout) in enumerate(zip(blocks, states, layouts))]


@pytest.mark.parametrize("count", [1, 2, 3])
@pytest.mark.parametrize("dim", [0, 1, (0, 1)])
def test_cat(dim, count):
    from paddle_sparse_amd import cat

    keeps = {0: {"rowcount"}, 1: {"colptr", "colcount"}, (0, 1): ALL}[dim]
    blocks = _blocks()[:count] if count != 2 else [_blocks()[0], _blocks()[2]]
    for kind in KINDS:
        results = []
        for state in STATES:
            for layout in ("row", "rowptr"):
                ops_ = _cat_operands(blocks, kind, [state] * count, [layout] * count)
                out = cat(ops_, dim)
                audit(out, keeps if state != "cold" else NONE, f"cat(dim={dim}, {count} x {state}, {layout}-built) [{kind}]",
                      check_ref=(state == "hot" and kind == "f32" and layout == "row"),
                      run_downstream=(layout == "row"))
                results.append(out)
        same_result(results, f"cat(dim={dim}, {count}) [{kind}]")


@pytest.mark.parametrize("dim", [0, 1, (0, 1)])
def test_cat_of_mixed_operands(dim):
    """A cache of the result is kept exactly when every operand carries it: one cold operand drops them all;
    operands built from `row` only and from `rowptr` only meet (the missing rows are expanded)."""
    from paddle_sparse_amd import cat

    blocks = _blocks(4)
    for states, layouts, expect in ((("warm", "cold", "hot"), ("row", "rowptr", "both"), NONE),
                                    (("hot", "warm", "warm"), ("rowptr", "row", "rowptr"),
                                     {0: {"rowcount"}, 1: {"colptr", "colcount"}, (0, 1): ALL}[dim]),
                                    (("cold", "cold", "cold"), ("row", "rowptr", "row"), NONE)):
        for kind in KINDS:
            out = cat(_cat_operands(blocks, kind, states, layouts), dim)
            audit(out, expect, f"cat(dim={dim}) of {states} built from {layouts} [{kind}]", check_ref=(kind == "f32"))


def test_narrow_diag_of_a_block_diagonal():
    """__narrow_diag__ on cat(..., (0, 1)) of three blocks, one of them without entries: every cache of a block is
    a shifted slice of the whole's."""
    from paddle_sparse_amd import cat

    blocks = _blocks(8)
    for kind in KINDS:
        for state in STATES:
            whole = cat(_cat_operands(blocks, kind, [state] * 3, ["row"] * 3), (0, 1))
            if state == "hot":
                heat(whole)
            r0 = c0 = 0
            for i, (_, (nr, nc)) in enumerate(blocks):
                part = whole.__narrow_diag__((r0, c0), (nr, nc))
                d = audit(part, NONE if state == "cold" else ALL, f"__narrow_diag__ block {i} [{kind}, {state}]")
                assert np.array_equal(d.row, blocks[i][0][0]) and np.array_equal(d.col, blocks[i][0][1])
                r0, c0 = r0 + nr, c0 + nc


@pytest.mark.parametrize("sizes", [(M0 + 37, N0), (M0, N0 + 50), (M0 + 1, N0 + 1), (M0 - 6, N0), (M0, N0 - 6), (M0 - 6, N0 - 6)])
def test_sparse_resize(base, sizes):
    # grow and shrink (to the tight size: the last 6 rows and columns are empty) in each dim; everything is kept
    run(lambda t: t.sparse_resize(sizes), operand_of(base), by_state(NONE, ALL), f"sparse_resize({sizes})")


@pytest.mark.parametrize("M,N", [(5, 9), (7, 7), (9, 5), (1, 1), (300, 2)])
def test_eye_with_caches(M, N):
    from paddle_sparse_amd import SparseTensor

    for has_value in (True, False):
        t = SparseTensor.eye(M, N, has_value=has_value, dtype=torch.float32, device="cuda", fill_cache=True)
        d = audit(t, ALL, f"eye({M}, {N}, fill_cache=True)")
        assert np.array_equal(d.row, np.arange(min(M, N))) and np.array_equal(d.col, np.arange(min(M, N)))
        audit(SparseTensor.eye(M, N, has_value=has_value, dtype=torch.float32, device="cuda"), NONE, f"eye({M}, {N})")


@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_from_scipy(base, fmt):
    from paddle_sparse_amd import SparseTensor

    row, col = base
    data = values("f32", row.size, 3).numpy()
    mat = scipy.sparse.coo_matrix((data, (row, col)), shape=(M0, N0))
    mat = mat.tocsr() if fmt == "csr" else mat.tocsc()
    for has_value in (True, False):
        t = SparseTensor.from_scipy(mat, has_value=has_value, device="cuda")
        d = audit(t, {"colptr"} if fmt == "csc" else NONE, f"from_scipy({fmt})")  # a csc matrix forwards its colptr
        assert np.array_equal(d.row, row) and np.array_equal(d.col, col)
        if has_value:
            assert np.array_equal(host(t.storage.value()), data)


@pytest.mark.parametrize("k", [-2, 0, 3])
@pytest.mark.parametrize("op", ["set_diag", "remove_diag", "fill_diag"])
def test_diag_ops(base, op, k):
    # rowptr and rowcount come from the kernels, colcount is adjusted iff the operand had it
    row, col = base
    extra = np.arange(0, 380, 3)  # some entries ON each diagonal, so that removing and replacing both happen
    keep = (extra + k >= 0) & (extra + k < N0 - 6)
    key = np.unique(np.concatenate([row * N0 + col, extra[keep] * N0 + extra[keep] + k]))
    with_diag = (key // N0, key % N0)
    fn = {"set_diag": lambda t: t.set_diag(None, k), "remove_diag": lambda t: t.remove_diag(k),
          "fill_diag": lambda t: t.fill_diag(2, k)}[op]
    run(fn, operand_of(with_diag), by_state({"rowcount"}, {"rowcount", "colcount"}), f"{op}(k={k})")


# ---- value-only replacements: the memos are carried and must still be right ------------------------

def _memo_names(st):
    names = {n for n in ("_row_csc", "_max_rowcount", "_spmm_algo_memo", "_csc_view_memo", "_mean_scale_memo")
             if getattr(st, n, None) is not None}
    if st._edge_tags:
        names.add("_edge_tags")
    if st._hot_memo:
        names.add("_hot_memo")
    return names


def _like(t, seed):
    """One integer operand entry per stored entry, in the shape of t's values ([nnz] for a value-less t)."""
    v = t.storage.value()
    return values("f32x3" if v is not None and v.dim() == 2 else "f32", t.nnz(), seed).cuda()


VALUE_OPS = {
    "set_value coo": (lambda t: t.set_value(values("f32", t.nnz(), 90).cuda(), layout="coo"), NONE),
    "set_value csc": (lambda t: t.set_value(values("f32", t.nnz(), 91).cuda(), layout="csc"), {"colptr", "csr2csc", "csc2csr"}),
    "set_value None": (lambda t: t.set_value(None, layout="coo"), NONE),
    "set_value_": (lambda t: t.copy().set_value_(values("f32x3", t.nnz(), 92).cuda(), layout="coo"), NONE),
    "type": (lambda t: t.type(torch.float64) if t.has_value() else t.copy(), NONE),
    "detach": (lambda t: t.detach(), NONE),
    "fill_value": (lambda t: t.fill_value(2.0, dtype=torch.float32), NONE),
    "mul_nnz": (lambda t: t.mul_nnz(_like(t, 93), layout="coo"), NONE),
    "add_nnz": (lambda t: t.add_nnz(_like(t, 94), layout="coo"), NONE),
    "copy": (lambda t: t.copy(), NONE),
}


@pytest.mark.parametrize("name", sorted(VALUE_OPS))
def test_value_only_replacements_carry_the_memos(base, name):
    fn, cold_keeps = VALUE_OPS[name]
    run(fn, operand_of(base), by_state(cold_keeps, ALL), name)
    hot = operand_of(base)("f32", "hot")
    had = _memo_names(hot.storage)
    assert {"_row_csc", "_edge_tags", "_max_rowcount", "_spmm_algo_memo", "_csc_view_memo", "_mean_scale_memo", "_hot_memo"} <= had
    out = fn(hot)
    assert _memo_names(out.storage) >= had, f"{name}: memos lost: {sorted(had - _memo_names(out.storage))}"


@pytest.mark.parametrize("name", ["narrow", "index_select"])
def test_dim_2_slicing_is_a_value_replacement(base, name):
    # only [nnz, 3] values have a dimension 2 (the other kinds raise: there is nothing to slice)
    fn = {"narrow": lambda t: t.narrow(2, 1, 2), "index_select": lambda t: t.index_select(2, dev([2, 0, 2]))}[name]
    run(fn, operand_of(base), by_state(NONE, ALL), f"{name}(dim=2)", kinds=("f32x3",), downstream_kinds=("f32x3",))


def test_clone_and_clear_cache(base):
    """clone copies the caches and drops the memos; clear_cache_ drops both; neither touches the hot operand,
    and ops on the clone leave the operand's arrays alone."""
    for kind in KINDS:
        hot = operand_of(base)(kind, "hot")
        had = _memo_names(hot.storage)
        before = {n: host(getattr(hot.storage, "_" + n)).copy() for n in CACHES + ("row", "rowptr", "col")}
        c = hot.clone()
        assert _memo_names(c.storage) == set() and not c.storage._perm_plans and c.storage._value_csc_memo is None
        for n in CACHES + ("row", "rowptr", "col"):
            assert getattr(c.storage, "_" + n).data_ptr() != getattr(hot.storage, "_" + n).data_ptr() or hot.nnz() == 0, n
        audit(c, ALL, f"clone [{kind}]")
        if kind is not None:
            c.storage.value().mul_(5)
            c.set_value_(c.storage.value() + 1, layout="coo")
        c.storage.col().add_(0)  # an in-place write on the clone's own arrays
        cleared = hot.clone()
        heat(cleared)
        cleared.clear_cache_()
        assert _memo_names(cleared.storage) == set() and cleared.storage._value_csc_memo is None
        assert not cleared.storage._perm_plans and getattr(cleared.storage, "_huge_memo", None) is None
        audit(cleared, NONE, f"clear_cache_ [{kind}]")
        assert _memo_names(hot.storage) == had
        for n, want in before.items():
            assert np.array_equal(host(getattr(hot.storage, "_" + n)), want), n
        audit(hot, ALL, f"hot operand after ops on its clone [{kind}]")


# ---- fresh structures ----------------------------------------------------------------------------

def test_coalesce_of_a_storage_with_duplicates(base):
    row, col = base
    rng = np.random.default_rng(6)
    again = rng.integers(0, row.size, 300)
    key = np.sort(np.concatenate([row * N0 + col, (row * N0 + col)[again]]))
    dup = (key // N0, key % N0)
    for reduce in ("sum", "max"):
        run(lambda t: t.coalesce(reduce), operand_of(dup), by_state(NONE, NONE), f"coalesce({reduce})")
    d = derived(*_entries(operand_of(dup)("f32", "cold").coalesce().storage), M0, N0)
    assert np.array_equal(d.row, row) and np.array_equal(d.col, col)


def test_to_symmetric_below_and_above_the_merge_threshold(base, monkeypatch):
    import paddle_sparse_amd.tensor as tensor_mod

    run(lambda t: t.to_symmetric(), operand_of(base), by_state(NONE, NONE), "to_symmetric (sorted halves)")
    monkeypatch.setattr(tensor_mod, "_MERGE_ABOVE", 64)  # the small matrix then takes the merge of A and its CSC view
    assert 2 * base[0].size > 64
    run(lambda t: t.to_symmetric(), operand_of(base), by_state(NONE, NONE), "to_symmetric (merged halves)")


def test_sparse_binary_ops(base):
    """A + B with every kind of value (the result has values only when both operands do); A * B and A @ B multiply
    the values of matching entries, which they take as fp32 scalars."""
    other = power_law(M0, N0, seed=21)
    for kind in KINDS:
        results = []
        for state in STATES:
            a, b = operand_of(base)(kind, state), make(*other, (M0, N0), kind, state, seed=9)
            results.append(a + b)
            audit(results[-1], NONE, f"A + B [{kind}, {state}]", check_ref=(kind == "f32" and state == "hot"))
        same_result(results, f"A + B [{kind}]")
    prod, mm = [], []
    for state in STATES:
        a, b = operand_of(base)("f32", state), make(*other, (M0, N0), "f32", state, seed=9)
        prod.append(a * b)
        audit(prod[-1], NONE, f"A * B [{state}]")
        mm.append(a @ b.t())
        audit(mm[-1], NONE, f"A @ B^T [{state}]", check_ref=False)
    same_result(prod, "A * B")
    same_result(mm, "A @ B^T")
    a, b = operand_of(base)(None, "hot"), make(*other, (M0, N0), "f32", "warm")
    audit(a + b, NONE, "A + B, one side without values")


def test_permute_reshape_and_sampling(base):
    sq = power_law(500, 500, seed=13, hole=(100, 110))
    perm = np.random.default_rng(1).permutation(500)
    square = lambda kind, state: make(*sq, (500, 500), kind, state, seed=2)  # noqa: E731
    # permute = index_select(0) then index_select(1): the caches of the second
    run(lambda t: t.permute(dev(perm)), square, by_state({"colptr", "colcount", "csc2csr"}, {"colptr", "colcount", "csc2csr"}),
        "permute")
    run(lambda t: t.sparse_reshape(250, 1000), square, by_state(NONE, NONE), "sparse_reshape(250, 1000)")
    run(lambda t: t.sparse_reshape(1000, -1), square, by_state(NONE, NONE), "sparse_reshape(1000, -1)")
    subset = dev([3, 2, 499, 7, 0, 250, 1])
    for k in (-1, 3):
        run(lambda t: t.sample_adj(subset, k, seed=5)[0], square, by_state(NONE, NONE), f"sample_adj(k={k})")
    nodes = dev(np.random.default_rng(2).permutation(500)[:200])
    run(lambda t: t.saint_subgraph(nodes)[0], square, by_state(NONE, NONE), "saint_subgraph")


def test_nnz_selections_with_an_ascending_selection(base):
    """index_select_nnz / masked_select_nnz mark their result sorted: that holds for an ascending selection,
    the documented contract (the result of any other order is unspecified)."""
    nnz = base[0].size
    rng = np.random.default_rng(3)
    pick = np.sort(rng.choice(nnz, nnz // 3, replace=False))
    keep = rng.random(nnz) < 0.5
    run(lambda t: t.index_select_nnz(dev(pick), layout="coo"), operand_of(base), by_state(NONE, NONE), "index_select_nnz")
    run(lambda t: t.masked_select_nnz(torch.from_numpy(keep).cuda(), layout="coo"), operand_of(base), by_state(NONE, NONE),
        "masked_select_nnz")


# ---- the value memo --------------------------------------------------------------------------------

def test_value_in_csc_order_follows_every_change_of_the_values(base):
    """_value_in_csc_order() == value[csr2csc] after set_value_ in place, after value.mul_(2) in place and after a
    write into the tensor csc() returned — on a hot storage and on its _replace'd descendants, which share
    `_perm_plans` with it."""
    d = derived(*base, M0, N0)
    hot = operand_of(base)("f32", "hot")
    family = [hot, hot.set_value(values("f32", d.nnz, 70).cuda(), layout="coo"), hot.copy(), hot.detach()]
    family.append(family[1].mul_nnz(values("f32", d.nnz, 71).cuda(), layout="coo"))

    def ok(t, where):
        got, want = host(t.storage._value_in_csc_order()), host(t.storage.value())[d.csr2csc]
        assert np.array_equal(got, want), where
        assert np.array_equal(host(t.csc()[2]), want), where

    for i, t in enumerate(family):
        ok(t, f"member {i}")
        t.set_value_(values("f32", d.nnz, 80 + i).cuda(), layout="coo")
        ok(t, f"member {i} after set_value_")
        t.storage.value().mul_(2)
        ok(t, f"member {i} after value.mul_(2)")
        t.csc()[2].zero_()  # a caller scribbling on what csc() gave it
        ok(t, f"member {i} after a write into csc()'s values")
        t.set_value_(values("f32", d.nnz, 85 + i).cuda(), layout="csc")
        assert np.array_equal(host(t.storage.value())[d.csr2csc], values("f32", d.nnz, 85 + i).numpy())
        ok(t, f"member {i} after set_value_(layout=csc)")
    for i, t in enumerate(family):  # and no member's change reached another
        ok(t, f"member {i} at the end")
        check_fields(t.storage, d, f"member {i} at the end")


# ---------------------------------------------------------------------------------------------
# just above 2^20 entries: colptr() through the column sort, planned permutations, hub columns
# ---------------------------------------------------------------------------------------------

BIG_M, BIG_N = 1 << 18, 1 << 17


@pytest.fixture(scope="module")
def big():
    return big_power_law(BIG_M, BIG_N)


@pytest.fixture
def hub_columns_4096():
    """The 64 hot columns of the small matrices draw 7 % of the large one's entries; 4096 draw 31 % of them (and
    4096 hub rows 25 % of the transpose's), above the fifth `_hot_columns` asks for."""
    import paddle_sparse_amd.storage as st_mod

    old, st_mod.HOT_COLUMNS = st_mod.HOT_COLUMNS, 4096
    yield
    st_mod.HOT_COLUMNS = old


def big_operand(big, state, kind="f32"):
    from paddle_sparse_amd import ops
    from paddle_sparse_amd import storage as st_mod

    assert big[0].size >= st_mod._SORT_BEATS_ATOMICS and big[0].size >= ops.PERMUTE_PLAN_FROM
    return make(*big, (BIG_M, BIG_N), kind, state, seed=17)


def test_big_operand_takes_the_large_routes(big, hub_columns_4096):
    hot = big_operand(big, "hot")
    st = hot.storage
    assert st._spmm_algo_memo == "edge_ranges" and st._hot_memo, "hub columns expected on the large power-law matrix"
    assert {"to_csc", "to_csr"} & set(st._perm_plans), "a planned permutation expected after three training steps"
    audit(hot, ALL, "big hot operand")
    cold = big_operand(big, "cold")
    cold.storage.colcount()  # from 2^20 entries: through the column sort, which leaves csr2csc and colptr behind
    audit(cold, {"colptr", "colcount", "csr2csc"}, "colcount() of a big cold operand", run_downstream=False)


BIG_OPS = {
    "t": (lambda t: t.t(), {"csc2csr"}, ALL),
    "narrow 0": (lambda t: t.narrow(0, 1000, BIG_M // 2), NONE, {"rowcount"}),
    "narrow 1": (lambda t: t.narrow(1, 7, BIG_N // 2), NONE, {"colptr", "colcount"}),
    "index_select 0": (lambda t: t.index_select(0, dev(np.random.default_rng(0).integers(0, BIG_M // 8, BIG_M // 2))),
                       {"rowcount"}, {"rowcount"}),
    "index_select 1": (lambda t: t.index_select(1, dev(np.random.default_rng(1).integers(0, BIG_N // 8, BIG_N // 2))),
                       {"colptr", "colcount", "csc2csr"}, {"colptr", "colcount", "csc2csr"}),
    "sparse_resize": (lambda t: t.sparse_resize((BIG_M + 3, BIG_N + 5)), NONE, ALL),
    "set_diag": (lambda t: t.set_diag(None, 3), {"rowcount"}, {"rowcount", "colcount"}),
    "set_value": (lambda t: t.set_value(values("f32", t.nnz(), 33).cuda(), layout="csc"), {"colptr", "csr2csc", "csc2csr"}, ALL),
    "to_symmetric": (lambda t: t.to_symmetric(), NONE, NONE),
    "masked_select 0": (lambda t: t.masked_select(0, torch.from_numpy(np.random.default_rng(2).random(BIG_M) < 0.9).cuda()),
                        {"rowcount"}, {"rowcount"}),
    "masked_select 1": (lambda t: t.masked_select(1, torch.from_numpy(np.random.default_rng(3).random(BIG_N) < 0.9).cuda()),
                        {"colptr", "colcount", "csc2csr"}, {"colptr", "colcount", "csc2csr"}),
    "select 0": (lambda t: t.select(0, 0), NONE, {"rowcount"}),  # the longest row
    "select 1": (lambda t: t.select(1, 0), NONE, {"colptr", "colcount"}),  # the longest column
    "remove_diag": (lambda t: t.remove_diag(0), {"rowcount"}, {"rowcount", "colcount"}),
    "fill_diag": (lambda t: t.fill_diag(2.0, -2), {"rowcount"}, {"rowcount", "colcount"}),
}
BIG_STATES = ("cold", "warm", "hot")


@pytest.mark.parametrize("name", sorted(BIG_OPS))
def test_big(big, name, hub_columns_4096):
    fn, cold_keeps, warm_keeps = BIG_OPS[name]
    results = []
    for state in BIG_STATES:
        out = fn(big_operand(big, state))
        audit(out, cold_keeps if state == "cold" else warm_keeps, f"big {name} [{state}]",
              check_ref=False, run_downstream=(state == "hot"))
        results.append(out)
    same_result(results, f"big {name}")


@pytest.mark.parametrize("dim", [0, 1, (0, 1)])
def test_big_cat(big, dim, hub_columns_4096):
    from paddle_sparse_amd import cat

    small = power_law(M0, N0, seed=3)
    keeps = {0: {"rowcount"}, 1: {"colptr", "colcount"}, (0, 1): ALL}[dim]
    results = []
    for state in BIG_STATES:
        parts = [big_operand(big, state), make(*small, (M0, N0), "f32", state, seed=1)]
        out = cat(parts, dim)
        if dim == (0, 1):
            # and back: each block of the block diagonal is a shifted slice of every cache, the permutations
            # included (taken before the audit's lazy builders fill the whole's caches)
            r0 = c0 = 0
            for i, ((row, col), (nr, nc)) in enumerate(((big, (BIG_M, BIG_N)), (small, (M0, N0)))):
                part = out.__narrow_diag__((r0, c0), (nr, nc))
                d = audit(part, NONE if state == "cold" else ALL, f"big __narrow_diag__ block {i} [{state}]",
                          check_ref=False, run_downstream=(state == "hot"))
                assert np.array_equal(d.row, row) and np.array_equal(d.col, col)
                assert torch.equal(part.storage.value(), parts[i].storage.value())
                r0, c0 = r0 + nr, c0 + nc
        audit(out, NONE if state == "cold" else keeps, f"big cat(dim={dim}) [{state}]", check_ref=False,
              run_downstream=(state == "hot"))
        results.append(out)
    same_result(results, f"big cat(dim={dim})")


def test_big_eye(hub_columns_4096):
    from paddle_sparse_amd import SparseTensor, ops

    M, N = ops.PERMUTE_PLAN_FROM + 5, ops.PERMUTE_PLAN_FROM + 3
    t = SparseTensor.eye(M, N, dtype=torch.float32, device="cuda", fill_cache=True)
    d = audit(t, ALL, "big eye(fill_cache=True)", check_ref=False)
    assert d.nnz == N and np.array_equal(d.row, np.arange(N)) and np.array_equal(d.col, np.arange(N))


@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_big_from_scipy(big, fmt, hub_columns_4096):
    """A csc matrix forwards its colptr — the array storage.colptr() would otherwise take from the column sort."""
    from paddle_sparse_amd import SparseTensor

    row, col = big
    data = values("f32", row.size, 3).numpy()
    indptr = np.searchsorted(row, np.arange(BIG_M + 1), side="left")
    mat = scipy.sparse.csr_matrix((data, col, indptr), shape=(BIG_M, BIG_N))
    t = SparseTensor.from_scipy(mat if fmt == "csr" else mat.tocsc(), device="cuda")
    d = audit(t, {"colptr"} if fmt == "csc" else NONE, f"big from_scipy({fmt})", check_ref=False)
    assert np.array_equal(d.row, row) and np.array_equal(d.col, col) and np.array_equal(host(t.storage.value()), data)


def test_row_above_the_two_byte_limit():
    """One row above ops.ARG_WORDS_EXACT_ROW entries: `_huge_memo` / `_huge_bw_memo` are built by the max training
    step, kept by set_value, and not carried by a narrow(0, ...) that cuts through the matrix (the result
    builds its own, for the rows it kept)."""
    from paddle_sparse_amd import ops

    M, N = 1 << 12, 1 << 17
    row, col = big_power_law(M, N, nnz=1 << 18, seed=5, huge_row=ops.ARG_WORDS_EXACT_ROW + 4000, at_least=1 << 17)
    hot = make(row, col, (M, N), "f32", "hot", seed=4)
    st = hot.storage
    assert st._max_rowcount > ops.ARG_WORDS_EXACT_ROW and st._huge_memo and st._huge_bw_memo
    audit(hot, ALL, "hot operand with a huge row", check_ref=False)
    kept = hot.set_value(values("f32", hot.nnz(), 8).cuda(), layout="coo")
    assert kept.storage._huge_memo is st._huge_memo and kept.storage._huge_bw_memo is st._huge_bw_memo
    audit(kept, ALL, "set_value of a storage with a huge row", check_ref=False)
    for start, length in ((3, 200), (6, 100), (0, 6)):  # with row 5 inside, without it, ending at it
        cut = hot.narrow(0, start, length)
        assert getattr(cut.storage, "_huge_memo", None) is None and getattr(cut.storage, "_huge_bw_memo", None) is None
        heat(cut.fill_cache_())  # warm first: the training steps alone never ask for colcount
        assert bool(getattr(cut.storage, "_huge_memo", None)) == (start <= 5 < start + length)
        audit(cut, ALL, f"narrow(0, {start}, {length}) through a matrix with a huge row", check_ref=False)
