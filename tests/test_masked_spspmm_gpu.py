"""GPU suite for the pair-intersection kernel and the ops built on it (masked_spspmm, common_neighbors,
triangle_count).  The raw op is held bit for bit to the ordered restatement of tests/intersect_ref.py
(pinned by test_intersect_ref.py) in float32 and float64 and to the mathematical one in the counting form;
the public functions to dense float64 products of integer-valued data, where every order gives the same bits."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from intersect_ref import (GROUP, T, WAVE, common_neighbors_ref, csc_of, pair_intersect_math, pair_intersect_ordered,
                           triangle_count_ref)
from test_intersect_ref import KAT_GRAPHS, W3_A, W3_B, W3_C, W3_W, csr_arrays

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
NP_OF = {torch.float32: np.float32, torch.float64: np.float64, torch.int64: np.int64}
BITS = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64, np.dtype(np.int64): np.int64}


def gpu(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def fam_gpu(fam, dtype=None):
    return gpu(fam[0]), gpu(fam[1]), gpu(fam[2], dtype)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(BITS[a.dtype])


def run(x, y, px, py, weight=None, dtype=torch.float32):
    """ops.pair_intersect on host arrays, values and weight cast to dtype; the result on the host.  The op is
    told the dtype only when nothing it is given carries one."""
    from paddle_sparse_amd import ops

    vd = None if dtype == torch.int64 else dtype
    bare = x[2] is None and y[2] is None and weight is None
    out = ops.pair_intersect(fam_gpu(x, vd), fam_gpu(y, vd), gpu(np.asarray(px, np.int64)), gpu(np.asarray(py, np.int64)),
                             gpu(weight, vd), dtype=dtype if bare and dtype != torch.int64 else None)
    assert out.dtype == dtype
    return out.cpu().numpy()


def assert_bits(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


# ---- the kernel's constants ------------------------------------------------------------------------------------------
def test_the_restatement_uses_the_kernels_constants():
    src = (ROOT / "paddle_sparse_amd" / "csrc" / "intersect.hip").read_text()
    assert int(re.search(r"#define PSA_INTERSECT_T (\d+)", src).group(1)) == T
    assert int(re.search(r"constexpr int kGroup = (\d+);", src).group(1)) == GROUP
    assert "kLongFrom = PSA_INTERSECT_T" in src and "np > kLongFrom" in src  # longer than T, not from T on
    assert WAVE == 64
    design = (ROOT / "DESIGN.md").read_text()
    assert re.search(r"`T = %d`" % T, design)


# ---- the list-length grid --------------------------------------------------------------------------------------------
LENGTHS = sorted({0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, T, T + 1, 2 * T + 3, 3000})
PLACEMENTS = ("none", "all", "first", "last", "ends", "interleaved")
UNIVERSE = 10 * 3000 + 16  # searched lists hold multiples of 10 from 10 on


def make_lists(a, b, placement, rng):
    """(probe list of length a, searched list of length b), a <= b, ascending and free of duplicates.  The searched
    list is 10, 20, ..., 10 b; values 5 mod 10 never match."""
    searched = 10 * np.arange(1, b + 1, dtype=np.int64)
    miss = lambda lo, hi, n: 10 * np.sort(rng.choice(np.arange(lo, hi), n, replace=False)).astype(np.int64) + 5
    if a == 0:
        return np.zeros(0, np.int64), searched
    if placement == "none":
        probe = miss(0, b + 1, a)
    elif placement == "all":
        probe = np.sort(rng.choice(searched, a, replace=False))
    elif placement == "first":  # only the first probe element, at the first position of the searched list
        probe = np.concatenate([searched[:1], miss(1, b + 1, a - 1)])
    elif placement == "last":  # only the last probe element, at the last position of the searched list
        probe = np.concatenate([miss(0, b, a - 1), searched[-1:]])
    elif placement == "ends":  # first and last position of the searched list, nothing between
        probe = np.concatenate([searched[:1], miss(1, b, a - 2), searched[-1:]]) if a >= 2 else searched[-1:].copy()
    else:  # neighbours k - 1 and k + 1 of stored values among exact ones
        cand = np.concatenate([searched - 1, searched, searched + 1])
        probe = np.sort(rng.choice(cand, a, replace=False))
    assert len(probe) == a and np.all(np.diff(probe) > 0) and np.all(np.diff(searched) > 0)
    return probe, searched


@functools.lru_cache(maxsize=None)
def grid():
    """One X list and one Y list per (len x, len y, placement); pair i of the grid is (i, i), in a shuffled order
    so that every wave mixes short and deferred pairs."""
    rng = np.random.default_rng(2024)
    xs, ys, meta = [], [], []
    for nx in LENGTHS:
        for ny in LENGTHS:
            for placement in PLACEMENTS:
                probe, searched = make_lists(min(nx, ny), max(nx, ny), placement, rng)
                xl, yl = (probe, searched) if nx <= ny else (searched, probe)  # a tie: X probes
                assert (len(xl), len(yl)) == (nx, ny)
                xs.append(xl), ys.append(yl), meta.append((nx, ny, placement))

    def family(lists):
        ptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64)
        idx = np.concatenate(lists)
        val = rng.standard_normal(len(idx)) * 10.0 ** rng.integers(-2, 3, len(idx))  # sums whose order shows
        return ptr, idx, val

    x, y = family(xs), family(ys)
    weight = rng.standard_normal(UNIVERSE) + 2.0
    order = rng.permutation(len(meta))
    return x, y, weight, order, meta


@functools.lru_cache(maxsize=None)
def grid_reference(dtype_name):
    x, y, weight, order, _ = grid()
    if dtype_name == "int64":
        return pair_intersect_math((x[0], x[1], None), (y[0], y[1], None), order, order)
    return pair_intersect_ordered(x, y, order, order, weight, np.dtype(dtype_name))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_length_grid_has_the_restatements_bits(dtype):
    x, y, weight, order, meta = grid()
    want = grid_reference(np.dtype(NP_OF[dtype]).name)
    got = run(x, y, order, order, weight, dtype)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, [(meta[order[i]], got[i], want[i]) for i in bad[:6]]
    # the sums are not trivial: the ordered bits differ from the float64 answer rounded once, somewhere
    exact = pair_intersect_math((x[0], x[1], x[2].astype(NP_OF[dtype])), (y[0], y[1], y[2].astype(NP_OF[dtype])),
                                order, order, weight.astype(NP_OF[dtype]))
    assert np.any(want != 0) and (dtype == torch.float64 or np.any(want != exact.astype(np.float32)))


def test_length_grid_counts():
    x, y, _, order, meta = grid()
    want = grid_reference("int64")
    got = run((x[0], x[1], None), (y[0], y[1], None), order, order, dtype=torch.int64)
    assert got.dtype == np.int64
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(meta[order[i]], got[i], want[i]) for i in bad[:6]]
    by = {m: want[np.flatnonzero(order == i)[0]] for i, m in enumerate(meta)}
    assert by[(3000, 3000, "all")] == 3000 and by[(3000, 3000, "none")] == 0 and by[(T + 1, 3000, "ends")] == 2
    assert by[(17, 64, "first")] == 1 and by[(64, 17, "last")] == 1 and by[(0, 9, "all")] == 0


# ---- pair counts, mixed waves, the grid tail ---------------------------------------------------------------------------
def pair_of(nx, ny, placement="interleaved"):
    return grid()[4].index((nx, ny, placement))


def test_pair_counts_and_mixed_waves():
    x, y, weight, _, _ = grid()
    rng = np.random.default_rng(5)
    short = [pair_of(9, 17), pair_of(T, T, "all"), pair_of(1, 3000, "all"), pair_of(0, 65), pair_of(63, 8)]
    long_ = [pair_of(T + 1, T + 1, "all"), pair_of(2 * T + 3, 3000), pair_of(3000, 3000), pair_of(3000, 65, "ends")]
    cases = []
    for P in (0, 1, 7, 8, 9, 63, 64, 65, 513):  # partial groups, partial waves, more than one block
        cases.append((rng.choice(short + long_, P), rng.choice(short + long_, P)))  # X and Y lists chosen apart
    waves = [[pos == d for pos in range(8)] for d in range(8)]  # one deferred group, in every position
    waves += [[True] * 8, [False] * 8, [pos % 2 == 0 for pos in range(8)], [pos >= 4 for pos in range(8)]]
    mixed = np.array([long_[(i + j) % len(long_)] if d else short[(i + j) % len(short)]
                      for i, w in enumerate(waves) for j, d in enumerate(w)])
    cases.append((mixed, mixed))
    cases.append((mixed[:-3], mixed[:-3]))  # the last wave partial, its last group deferred before the cut
    for px, py in cases:
        for dtype in (torch.float32, torch.float64):
            want = pair_intersect_ordered(x, y, px, py, weight, NP_OF[dtype])
            assert_bits(run(x, y, px, py, weight, dtype), want, (len(px), dtype))
        pat = ((x[0], x[1], None), (y[0], y[1], None))
        assert np.array_equal(run(*pat, px, py, dtype=torch.int64), pair_intersect_math(*pat, px, py)), len(px)


def test_more_pairs_than_one_sweep_of_the_grid():
    """The launch is capped at 65536 blocks of 32 pairs and the waves stride: pairs past 2^21."""
    x, y, weight, _, meta = grid()
    src = (ROOT / "paddle_sparse_amd" / "csrc" / "intersect.hip").read_text()
    cap = int(re.search(r"kMaxBlocks = (\d+);", src).group(1)) * 32
    base = np.array([i for i, (nx, ny, _) in enumerate(meta) if max(nx, ny) <= 2 * T + 3])
    P = cap + 65
    px = np.resize(base, P)
    py = np.resize(base[::-1], P)
    want = np.resize(pair_intersect_ordered(x, y, px[:len(base)], py[:len(base)], weight, np.float32), P)
    from paddle_sparse_amd import ops

    out = ops.pair_intersect(fam_gpu(x, torch.float32), fam_gpu(y, torch.float32), gpu(px), gpu(py),
                             gpu(weight, torch.float32))
    assert torch.equal(out.view(torch.int32), gpu(want).view(torch.int32))


# ---- index and value edges -------------------------------------------------------------------------------------------
def small_family(rng, lists, n_max, universe):
    lens = rng.integers(0, n_max + 1, lists)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(universe, n, replace=False)) for n in lens] + [np.zeros(0, np.int64)])
    return ptr, idx.astype(np.int64), rng.standard_normal(len(idx)) * 10.0 ** rng.integers(-2, 3, len(idx))


def test_bad_pair_indices_write_zero_and_duplicates_agree():
    rng = np.random.default_rng(1)
    x, y = small_family(rng, 40, 90, 200), small_family(rng, 30, 90, 200)
    weight = rng.standard_normal(200)
    px = np.array([-1, 40, 2**40, -2**63, 3, 3, 0, 39, 3, 41, 5, 2**63 - 1], np.int64)
    py = np.array([0, 0, 1, 2, -1, 30, 29, 29, 7, 31, 5, 2**63 - 1], np.int64)
    inside = (px >= 0) & (px < 40) & (py >= 0) & (py < 30)
    px, py = np.concatenate([px, px]), np.concatenate([py, py])  # every pair twice
    for dtype in (torch.float32, torch.float64):
        got = run(x, y, px, py, weight, dtype)
        assert_bits(got, pair_intersect_ordered(x, y, px, py, weight, NP_OF[dtype]), dtype)
        assert np.all(got[~np.concatenate([inside, inside])] == 0) and np.any(got != 0)
        assert_bits(got[:len(got) // 2], got[len(got) // 2:])
    got = run((x[0], x[1], None), (y[0], y[1], None), px, py, dtype=torch.int64)
    assert np.all(got[~np.concatenate([inside, inside])] == 0) and np.any(got != 0)


def test_index_values_above_32_bits():
    """Compared as int64: values that agree in their low 32 bits are different values."""
    hi = 2**32
    x = (np.array([0, 3, 5], np.int64), np.array([5, 5 + hi, 7 + 2 * hi, 1, 9 + 2**40], np.int64), np.array([2., 3., 5., 7., 11.]))
    y = (np.array([0, 3, 6], np.int64), np.array([7, 5 + hi, 7 + 2 * hi, 9, 1 + hi, 9 + 2**40], np.int64),
         np.array([17., 13., 19., 29., 23., 31.]))
    assert all(np.all(np.diff(f[1][f[0][i]:f[0][i + 1]]) > 0) for f in (x, y) for i in (0, 1))  # ascending lists
    px, py = [0, 0, 1, 1], [0, 1, 0, 1]
    assert run((x[0], x[1], None), (y[0], y[1], None), px, py, dtype=torch.int64).tolist() == [2, 0, 0, 1]
    for dtype in (torch.float32, torch.float64):
        assert run(x, y, px, py, dtype=dtype).tolist() == [3. * 13 + 5 * 19, 0, 0, 11. * 31]
    # long lists far above 2^32 (both modes), against the restatement
    rng = np.random.default_rng(3)
    fx, fy = small_family(rng, 12, 200, 400), small_family(rng, 12, 200, 400)
    fx, fy = (fx[0], fx[1] * hi + 3, fx[2]), (fy[0], fy[1] * hi + 3, fy[2])
    p = np.arange(12)
    assert_bits(run(fx, fy, p, p[::-1]), pair_intersect_ordered(fx, fy, p, p[::-1]))
    assert pair_intersect_math(fx, fy, p, p[::-1]).any()


def test_value_and_weight_combinations():
    rng = np.random.default_rng(4)
    x, y = small_family(rng, 50, 150, 300), small_family(rng, 50, 150, 300)
    weight = rng.standard_normal(300)
    px, py = rng.integers(0, 50, 200), rng.integers(0, 50, 200)
    for dtype in (torch.float32, torch.float64):
        for xv in (x[2], None):
            for yv in (y[2], None):
                for w in (weight, None):
                    fx, fy = (x[0], x[1], xv), (y[0], y[1], yv)
                    want = pair_intersect_ordered(fx, fy, px, py, w, NP_OF[dtype])
                    got = run(fx, fy, px, py, w, dtype)
                    assert_bits(got, want, (dtype, xv is None, yv is None, w is None))
    # without anything the default is the counting form; with a float dtype the counts come as floats
    pat = ((x[0], x[1], None), (y[0], y[1], None))
    counts = pair_intersect_math(*pat, px, py)
    assert np.array_equal(run(*pat, px, py, dtype=torch.int64), counts) and counts.any()
    assert np.array_equal(run(*pat, px, py, dtype=torch.float32), counts.astype(np.float32))


def test_a_stored_zero_is_not_skipped():
    ptr = np.array([0, 2], np.int64)
    idx = np.array([3, 8], np.int64)
    x, y = (ptr, idx, np.array([np.inf, 1.0])), (ptr, idx, np.array([0.0, 2.0]))
    for dtype in (torch.float32, torch.float64):
        assert np.isnan(run(x, y, [0], [0], dtype=dtype)[0])  # inf * 0
        assert np.isnan(run(y, x, [0], [0], dtype=dtype)[0])
        w = np.zeros(9)
        assert np.isnan(run(x, (ptr, idx, None), [0], [0], w, dtype)[0])  # inf * weight 0
        assert run(y, (ptr, idx, None), [0], [0], dtype=dtype)[0] == 2.0


def test_operands_are_checked_before_any_launch():
    from paddle_sparse_amd import ops

    ptr, idx = gpu(np.array([0, 2], np.int64)), gpu(np.array([1, 4], np.int64))
    val, p = torch.ones(2, device="cuda"), gpu(np.array([0], np.int64))
    fam = (ptr, idx, val)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.pair_intersect((ptr.cpu(), idx, val), fam, p, p)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.pair_intersect(fam, fam, p.cpu(), p)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.pair_intersect(fam, fam, p, p, weight=torch.ones(5))
    with pytest.raises(TypeError):
        ops.pair_intersect((ptr.int(), idx, val), fam, p, p)
    with pytest.raises(TypeError):
        ops.pair_intersect(fam, (ptr, idx, val.double()), p, p)  # mixed value dtypes
    with pytest.raises(TypeError):
        ops.pair_intersect(fam, fam, p, p, dtype=torch.int64)  # values with the counting form
    with pytest.raises(TypeError):
        ops.pair_intersect((ptr, idx, None), (ptr, idx, None), p, p, dtype=torch.float16)
    with pytest.raises(ValueError):
        ops.pair_intersect((ptr, idx, torch.ones(3, device="cuda")), fam, p, p)  # one value per index
    with pytest.raises(ValueError):
        ops.pair_intersect((ptr, idx, torch.ones(4, device="cuda")[::2]), fam, p, p)  # contiguous
    with pytest.raises(ValueError):
        ops.pair_intersect(fam, fam, p, gpu(np.array([0, 0], np.int64)))
    with pytest.raises(TypeError):
        ops.pair_intersect((ptr, idx), fam, p, p)
    # families without entries: nothing to intersect, nothing to point at
    empty = (gpu(np.zeros(3, np.int64)), gpu(np.zeros(0, np.int64)), None)
    assert ops.pair_intersect(empty, (ptr, idx, None), gpu(np.array([0, 1], np.int64)),
                              gpu(np.array([0, 0], np.int64))).tolist() == [0, 0]
    assert ops.pair_intersect(fam, fam, p[:0], p[:0]).shape == (0,)


# ---- the public surface ----------------------------------------------------------------------------------------------
def int_matrix(M, N, density, seed, empty_rows=(), empty_cols=()):
    """Coalesced scipy CSR with small non-zero integer values (float64)."""
    rng = np.random.default_rng(seed)
    m = sp.random(M, N, density=density, random_state=rng, format="lil")
    for r in empty_rows:
        m[r, :] = 0
    for c in empty_cols:
        m[:, c] = 0
    m = sp.csr_matrix(m)
    m.data = (rng.integers(1, 4, m.nnz) * rng.choice([-1, 1], m.nnz)).astype(np.float64)
    m.sort_indices()
    return m


def tensor_of(m, dtype=torch.float32, has_value=True):
    from paddle_sparse_amd import SparseTensor

    t = SparseTensor.from_scipy(sp.csr_matrix(m), has_value=has_value, device="cuda")
    return t.set_value(t.storage.value().to(dtype), layout="coo") if has_value else t


def dense_of(m):
    return torch.from_numpy(np.asarray(sp.csr_matrix(m).todense(), np.float64)).cuda()


@functools.lru_cache(maxsize=None)
def product_case():
    M, K, N = 70, 300, 45  # rectangular; a has a hub row, b a hub column: both modes of the kernel
    a = int_matrix(M, K, 0.05, 1, empty_rows=(3, 69)).tolil()
    b = int_matrix(K, N, 0.05, 2, empty_cols=(0, 7)).tolil()
    a[1, :] = 1
    b[:, 2] = 2
    a[5, :100] = -1
    mask = int_matrix(M, N, 0.5, 3, empty_rows=(10,)).tolil()  # denser than the product: entries outside its pattern
    mask[1, 2] = mask[5, 2] = 1  # hub row against hub column
    return (sp.csr_matrix(a), sp.csr_matrix(b), sp.csr_matrix(mask),
            np.random.default_rng(9).integers(1, 4, K).astype(np.float64))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_masked_spspmm_is_the_dense_product_at_the_mask(dtype):
    import paddle_sparse_amd as psa

    a, b, mask, w = product_case()
    ta, tb, tm = tensor_of(a, dtype), tensor_of(b, dtype), tensor_of(mask, dtype)
    row, col, mval = tm.coo()
    for weight in (None, w):
        dense = (dense_of(a) * (1 if weight is None else gpu(weight))) @ dense_of(b)
        out = psa.masked_spspmm(ta, tb, tm, None if weight is None else gpu(weight, dtype))
        assert out.sparse_sizes() == tm.sparse_sizes() and out.storage.value().dtype == dtype
        assert out.storage.row().data_ptr() == row.data_ptr() and out.storage.col().data_ptr() == col.data_ptr()
        assert torch.equal(out.storage.value().double(), dense[row, col])
        assert out.storage.value() is not mval and torch.equal(tm.storage.value(), mval)  # the mask's values: not read
        assert bool((dense[row, col] == 0).any()) and bool((dense[row, col] != 0).any())
        assert torch.equal(ta.masked_matmul(tb, tm, None if weight is None else gpu(weight, dtype)).storage.value(),
                           out.storage.value())
    # a mask without values gives the same; an empty mask an empty result
    bare = tensor_of(mask, has_value=False)
    assert torch.equal(psa.masked_spspmm(ta, tb, bare).storage.value().double(), (dense_of(a) @ dense_of(b))[row, col])
    none = psa.SparseTensor(row=row[:0], col=col[:0], sparse_sizes=tm.sparse_sizes(), is_sorted=True)
    out = psa.masked_spspmm(ta, tb, none)
    assert out.nnz() == 0 and out.sparse_sizes() == tm.sparse_sizes() and out.storage.value().dtype == dtype
    # one operand without values counts as ones; neither: int64 counts
    ones_a, ones_b = tensor_of(a, has_value=False), tensor_of(b, has_value=False)
    pat_a, pat_b = (dense_of(a) != 0).double(), (dense_of(b) != 0).double()
    assert torch.equal(psa.masked_spspmm(ones_a, tb, tm).storage.value().double(), (pat_a @ dense_of(b))[row, col])
    assert torch.equal(psa.masked_spspmm(ta, ones_b, tm).storage.value().double(), (dense_of(a) @ pat_b)[row, col])
    counts = psa.masked_spspmm(ones_a, ones_b, tm).storage.value()
    assert counts.dtype == torch.int64 and torch.equal(counts, (pat_a @ pat_b)[row, col].long())
    assert int(counts.max()) > T  # the hub row against the hub column


def test_masked_spspmm_refuses_wrong_sizes_and_dtypes():
    import paddle_sparse_amd as psa

    a, b, mask, w = product_case()
    ta, tb, tm = tensor_of(a), tensor_of(b), tensor_of(mask)
    with pytest.raises(ValueError, match="inner sizes"):
        psa.masked_spspmm(ta, ta, tm)
    with pytest.raises(ValueError, match="mask must be"):
        psa.masked_spspmm(ta, tb, tm.t())
    with pytest.raises(TypeError, match="mixed dtypes"):
        psa.masked_spspmm(ta, tensor_of(b, torch.float64), tm)
    with pytest.raises(TypeError, match="mixed dtypes"):
        psa.masked_spspmm(ta, tb, tm, gpu(w, torch.float64))
    with pytest.raises(TypeError):
        psa.masked_spspmm(tensor_of(a, torch.float16), tb, tm)
    with pytest.raises(ValueError, match="weight must have"):
        psa.masked_spspmm(ta, tb, tm, gpu(w[:-1], torch.float32))
    with pytest.raises(NotImplementedError):
        psa.masked_spspmm(ta, tb, tm, gpu(w, torch.float32).requires_grad_())
    with pytest.raises(TypeError):
        psa.masked_spspmm(ta, dense_of(b), tm)


def storage_snapshot(t):
    st = t.storage
    return {k: (getattr(st, "_" + k).data_ptr(), getattr(st, "_" + k).clone()) for k in st.cached_keys()
            + ["col"] + (["row"] if st.has_row() else []) + (["rowptr"] if st.has_rowptr() else [])}


def test_operand_caches_are_unchanged():
    import paddle_sparse_amd as psa

    a, b, mask, w = product_case()
    ts = [tensor_of(m).fill_cache_() for m in (a, b, mask)]
    before = [storage_snapshot(t) for t in ts]
    values = [t.storage.value().clone() for t in ts]
    va, vb = (t.storage.value().clone().requires_grad_() for t in ts[:2])
    out = psa.masked_spspmm(ts[0].set_value(va, layout="coo"), ts[1].set_value(vb, layout="coo"), ts[2],
                            gpu(w, torch.float32))
    out.storage.value().sum().backward()
    psa.common_neighbors(ts[0], gpu(np.array([1, 5])), gpu(np.array([5, 2])))
    for t, snap, v in zip(ts, before, values):
        after = storage_snapshot(t)
        assert sorted(after) == sorted(snap)
        for k in snap:
            assert after[k][0] == snap[k][0] and torch.equal(after[k][1], snap[k][1]), k
        assert torch.equal(t.storage.value(), v)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_value_gradients_are_the_dense_gradients(dtype):
    """Integer-valued operands, weight and upstream gradient: every sum is exact in any order, so the sparse
    gradients equal dense float64 autograd bit for bit."""
    import paddle_sparse_amd as psa

    a, b, mask, w = product_case()
    rng = np.random.default_rng(12)
    ta, tb, tm = tensor_of(a, dtype), tensor_of(b, dtype), tensor_of(mask, dtype)
    row, col, _ = tm.coo()
    g = gpu(rng.integers(-3, 4, tm.nnz()).astype(np.float64))
    for weight in (None, w):
        for track_a, track_b in ((True, True), (True, False), (False, True)):
            va = ta.storage.value().clone().requires_grad_(track_a)
            vb = tb.storage.value().clone().requires_grad_(track_b)
            out = psa.masked_spspmm(ta.set_value(va, layout="coo"), tb.set_value(vb, layout="coo"), tm,
                                    None if weight is None else gpu(weight, dtype))
            out.storage.value().backward(g.to(dtype))
            da, db = dense_of(a).requires_grad_(), dense_of(b).requires_grad_()
            dense = (da * (1 if weight is None else gpu(weight))) @ db
            assert torch.equal(out.storage.value().detach().double(), dense[row, col].detach())
            dense[row, col].backward(g)
            ra, ca, _ = ta.coo()
            rb, cb, _ = tb.coo()
            assert (va.grad is not None) == track_a and (vb.grad is not None) == track_b
            if track_a:
                assert va.grad.dtype == dtype and torch.equal(va.grad.double(), da.grad[ra, ca])
                assert bool((va.grad != 0).any())
            if track_b:
                assert vb.grad.dtype == dtype and torch.equal(vb.grad.double(), db.grad[rb, cb])
                assert bool((vb.grad != 0).any())
    # an operand without values beside a tracked one
    vb = tb.storage.value().clone().requires_grad_()
    out = psa.masked_spspmm(tensor_of(a, has_value=False), tb.set_value(vb, layout="coo"), tm)
    out.storage.value().backward(g.to(dtype))
    db = dense_of(b).requires_grad_()
    ((dense_of(a) != 0).double() @ db)[row, col].backward(g)
    assert torch.equal(vb.grad.double(), db.grad[tb.storage.row(), tb.storage.col()])


def adjacency_tensor(rowptr, col, value=None):
    from paddle_sparse_amd import SparseTensor

    n = len(rowptr) - 1
    return SparseTensor(rowptr=gpu(rowptr), col=gpu(col), value=gpu(value), sparse_sizes=(n, n), is_sorted=True)


@functools.lru_cache(maxsize=None)
def random_symmetric(n=600, seed=21):
    rng = np.random.default_rng(seed)
    m = sp.random(n, n, density=0.02, random_state=rng, format="csr")
    m = sp.lil_matrix(((m + m.T) != 0).astype(np.float64))
    m[7, :] = 1  # a hub: lists above T
    m[:, 7] = 1
    m.setdiag(0)
    m = sp.csr_matrix(m)
    m.eliminate_zeros()
    rowptr, col, _ = csr_arrays(m)
    return rowptr, col


def test_common_neighbors_and_triangle_count():
    import paddle_sparse_amd as psa

    for name, ((rowptr, col), per_edge, triangles) in KAT_GRAPHS.items():
        adj = adjacency_tensor(rowptr, col)
        row = adj.storage.row()
        got = psa.common_neighbors(adj, row, adj.storage.col())
        assert got.dtype == torch.int64 and got.tolist() == [per_edge] * len(col), name
        assert psa.triangle_count(adj).tolist() == triangles and adj.triangle_count().tolist() == triangles, name
    star = adjacency_tensor(*KAT_GRAPHS["star"][0])
    assert star.common_neighbors(gpu(np.array([1, 1, 0, 3])), gpu(np.array([2, 1, 4, 4], np.int32))).tolist() == [1, 1, 0, 1]
    # the weighted 3 x 3: rows of A against rows of B^T
    rp, c, v = csr_arrays(W3_A)
    a3 = adjacency_tensor(rp, c, v.astype(np.float32))
    b3 = adjacency_tensor(*csr_arrays(W3_B)[:2], csr_arrays(W3_B)[2].astype(np.float32))
    full = adjacency_tensor(np.arange(0, 10, 3), np.tile(np.arange(3), 3))
    assert psa.masked_spspmm(a3, b3, full, gpu(W3_W, torch.float32)).storage.value().tolist() == W3_C.reshape(-1).tolist()
    # a random symmetric graph with a hub, arbitrary query pairs, with and without values and weight
    rowptr, col = random_symmetric()
    n = len(rowptr) - 1
    rng = np.random.default_rng(2)
    u, v = rng.integers(0, n, 3000), rng.integers(0, n, 3000)
    u[:3], v[:3] = 7, (7, 8, 9)
    adj = adjacency_tensor(rowptr, col)
    assert np.array_equal(adj.common_neighbors(gpu(u), gpu(v)).cpu().numpy(), common_neighbors_ref(rowptr, col, None, u, v))
    assert np.array_equal(psa.triangle_count(adj).cpu().numpy(), triangle_count_ref(rowptr, col))
    assert int(psa.triangle_count(adj).sum()) % 3 == 0 and int(psa.triangle_count(adj).sum()) > 0
    val = rng.integers(1, 4, len(col)).astype(np.float32)
    w = rng.integers(1, 4, n).astype(np.float32)
    got = adjacency_tensor(rowptr, col, val).common_neighbors(gpu(u), gpu(v), gpu(w))
    assert got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().astype(np.float64), common_neighbors_ref(rowptr, col, val, u, v, w))
    with pytest.raises(NotImplementedError):
        adjacency_tensor(rowptr, col, val).requires_grad_().common_neighbors(gpu(u), gpu(v))
    with pytest.raises(ValueError):
        psa.triangle_count(tensor_of(product_case()[0]))


def test_adamic_adar_by_the_readme_recipe():
    rowptr, col = random_symmetric()
    n = len(rowptr) - 1
    adj = adjacency_tensor(rowptr, col)
    rng = np.random.default_rng(6)
    u, v = rng.integers(0, n, 500), rng.integers(0, n, 500)
    deg = adj.storage.rowcount()
    weight = 1.0 / torch.log(deg.clamp(min=2).double())  # the README's recipe
    got = adj.common_neighbors(gpu(u), gpu(v), weight).cpu().numpy()
    degree = np.diff(rowptr)
    want = np.zeros(500)
    for p in range(500):
        common = np.intersect1d(col[rowptr[u[p]]:rowptr[u[p] + 1]], col[rowptr[v[p]]:rowptr[v[p] + 1]])
        want[p] = sum(1.0 / np.log(max(degree[k], 2)) for k in common.tolist())
    # positive float64 terms, each within 2 eps of the loop's (log and the division, on either side), summed in
    # another order: at most (terms - 1) eps more.  The terms of a pair number at most the largest degree.
    assert np.all(np.abs(got - want) <= (degree.max() + 2) * np.finfo(np.float64).eps * want) and want.any()
    text = (ROOT / "README.md").read_text()
    assert "1.0 / torch.log(deg.clamp(min=2)" in text
    # the README's other two recipes: resource allocation and Jaccard from the count and the two degrees
    assert "1.0 / deg.clamp(min=1)" in text and "cn / (deg[u] + deg[v] - cn).clamp(min=1)" in text
    tu, tv = gpu(u), gpu(v)
    cn = adj.common_neighbors(tu, tv)
    ra = adj.common_neighbors(tu, tv, 1.0 / deg.clamp(min=1).double()).cpu().numpy()
    jaccard = (cn / (deg[tu] + deg[tv] - cn).clamp(min=1)).cpu().numpy()
    cn = cn.cpu().numpy()
    for p in range(500):
        nu, nv = set(col[rowptr[u[p]]:rowptr[u[p] + 1]].tolist()), set(col[rowptr[v[p]]:rowptr[v[p] + 1]].tolist())
        want_ra = sum(1.0 / degree[k] for k in sorted(nu & nv))
        assert abs(ra[p] - want_ra) <= (degree.max() + 2) * np.finfo(np.float64).eps * want_ra
        assert cn[p] == len(nu & nv) and abs(jaccard[p] - len(nu & nv) / max(len(nu | nv), 1)) <= 1e-6  # a float32 quotient


def test_the_range_check_reads_once_and_trust_data_never(monkeypatch):
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import masked

    rowptr, col = random_symmetric()
    n = len(rowptr) - 1
    adj = adjacency_tensor(rowptr, col)
    adj.storage.rowptr()
    reads = []
    real = masked._host_read
    monkeypatch.setattr(masked, "_host_read", lambda t: (reads.append(1), real(t))[1])
    u, v = gpu(np.array([0, 5, n - 1])), gpu(np.array([3, 2, 1]))
    want = adj.common_neighbors(u, v)
    assert len(reads) == 1
    for bad_u, bad_v in ((n, 0), (0, n), (-1, 0), (0, -1)):
        with pytest.raises(IndexError):
            adj.common_neighbors(gpu(np.array([1, bad_u])), gpu(np.array([2, bad_v])))
    reads.clear()
    bad_u, bad_v = gpu(np.array([1, n, -1])), gpu(np.array([2, 0, 0]))
    with monkeypatch.context() as m:  # no read by any other way either
        for k in ("item", "tolist", "cpu", "numpy", "__bool__", "__int__"):
            m.setattr(torch.Tensor, k, lambda *a, _k=k, **kw: pytest.fail(f"host read through Tensor.{_k}"))
        got = psa.common_neighbors(adj, u, v, trust_data=True)
        bad = psa.common_neighbors(adj, bad_u, bad_v, trust_data=True)
    assert not reads and torch.equal(got, want) and bad.tolist()[1:] == [0, 0]


def test_two_runs_are_bit_equal():
    import paddle_sparse_amd as psa

    a, b, mask, w = product_case()
    ta, tb, tm = tensor_of(a), tensor_of(b), tensor_of(mask)
    rng = np.random.default_rng(8)
    ta = ta.set_value(gpu(rng.standard_normal(ta.nnz()), torch.float32), layout="coo")
    tb = tb.set_value(gpu(rng.standard_normal(tb.nnz()), torch.float32), layout="coo")
    weight = gpu(rng.standard_normal(a.shape[1]), torch.float32)
    first = psa.masked_spspmm(ta, tb, tm, weight).storage.value()
    for _ in range(3):
        assert torch.equal(psa.masked_spspmm(ta, tb, tm, weight).storage.value().view(torch.int32), first.view(torch.int32))
    # and they are the restatement's bits, through the views the public function picks
    x = csr_arrays(a)[:2] + (ta.storage.value().cpu().numpy(),)
    vb = tb.storage.value().cpu().numpy()
    y = csc_of(*csr_arrays(b)[:2], vb, b.shape[1])
    mr, mc, _ = (t.cpu().numpy() for t in tm.coo())
    assert_bits(first.cpu().numpy(), pair_intersect_ordered(x, y, mr, mc, weight.cpu().numpy()))


def test_capture_and_replay():
    import paddle_sparse_amd as psa

    a, b, mask, w = product_case()
    ta, tb, tm = (tensor_of(m).fill_cache_() for m in (a, b, mask))
    weight = gpu(w, torch.float32)
    rowptr, col = random_symmetric()
    n = len(rowptr) - 1
    adj = adjacency_tensor(rowptr, col).fill_cache_()
    u, v = gpu(np.arange(0, 512) % n), gpu((np.arange(0, 512) * 7 + 3) % n)
    g = torch.Generator(device="cuda").manual_seed(0)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        psa.masked_spspmm(ta, tb, tm, weight)
        psa.common_neighbors(adj, u, v, trust_data=True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = psa.masked_spspmm(ta, tb, tm, weight).storage.value()
        cn = psa.common_neighbors(adj, u, v, trust_data=True)
    for _ in range(2):  # new data in the captured buffers, replay
        ta.storage.value().copy_(torch.randn(ta.nnz(), generator=g, device="cuda"))
        tb.storage.value().copy_(torch.randn(tb.nnz(), generator=g, device="cuda"))
        weight.copy_(torch.randn(weight.numel(), generator=g, device="cuda"))
        u.copy_(torch.randint(0, n, (512,), generator=g, device="cuda"))
        v.copy_(torch.randint(0, n, (512,), generator=g, device="cuda"))
        graph.replay()
        torch.cuda.synchronize()
        eager = psa.masked_spspmm(ta, tb, tm, weight).storage.value()
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32)) and bool((out != 0).any())
        assert torch.equal(cn, psa.common_neighbors(adj, u, v, trust_data=True)) and bool((cn != 0).any())
