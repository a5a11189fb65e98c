"""tests/index_ref.py held to hand-written answers, and its case generators to the structure they claim
(no GPU).  A generator that lost its edge would leave tests/test_index_kernels_gpu.py green and blind."""
import numpy as np
import pytest

import index_ref as ir


def i64(*x):
    return np.array(x, np.int64)


# ---------------------------------------------------------------------------------------------
# restatements against hand-written answers
# ---------------------------------------------------------------------------------------------

def test_count2ptr_by_hand():
    assert ir.count2ptr(i64()).tolist() == [0]
    assert ir.count2ptr(i64(3)).tolist() == [0, 3]
    assert ir.count2ptr(i64(2, 0, 5, 1)).tolist() == [0, 2, 2, 7, 8]
    big = ir.count2ptr(i64(1 << 40, 0, (1 << 31) + 1, 1 << 62))
    assert big.dtype == np.int64
    assert big.tolist() == [0, 1 << 40, 1 << 40, (1 << 40) + (1 << 31) + 1, (1 << 62) + (1 << 40) + (1 << 31) + 1]


def test_gather_bytes_by_hand():
    src = np.arange(12, dtype=np.uint8)  # three rows of four bytes
    assert ir.gather_bytes(src, i64(2, 0, 2), 4).tolist() == [[8, 9, 10, 11], [0, 1, 2, 3], [8, 9, 10, 11]]
    # rows six bytes apart, window [1, 3): two rows
    assert ir.gather_bytes(src, i64(1, 0), 2, stride=6, first=1).tolist() == [[7, 8], [1, 2]]
    assert ir.gather_bytes(src, i64(), 4).shape == (0, 4)
    assert ir.gather_bytes(src, i64(1), 0, stride=4, first=4).shape == (1, 0)


def test_make_and_split_keys_by_hand():
    keys, flag = ir.make_keys(i64(0, 0, 1, 2), i64(3, 9, 0, 0), 10)
    assert keys.tolist() == [3, 9, 10, 20] and flag == 0
    keys, flag = ir.make_keys(i64(0, 1, 0), i64(3, 0, 9), 10)
    assert keys.tolist() == [3, 10, 9] and flag == 1
    assert ir.make_keys(i64(1, 1), i64(4, 4), 10)[1] == 0      # equal neighbours are sorted
    assert ir.make_keys(i64(5), i64(1), 10) == (i64(51), 0)
    hi, lo = ir.split_keys(i64(0, 9, 10, 29, (1 << 40) + 7), 10)
    assert hi.tolist() == [0, 0, 1, 2, 109951162778] and lo.tolist() == [0, 9, 0, 9, 3]   # 2^40 + 7 = 1099511627783
    hi, lo = ir.split_keys(i64(1 << 62, (1 << 32) + 1), (1 << 32) + 1)
    assert hi.tolist() == [(1 << 62) // ((1 << 32) + 1), 1] and lo.tolist() == [(1 << 62) % ((1 << 32) + 1), 0]


def test_bincount_and_inverse_by_hand():
    assert ir.bincount(i64(1, 1, 3, -1, 4, 1 << 40, ir.INT64_MIN, 0), 4).tolist() == [1, 2, 0, 1]
    assert ir.bincount(i64(1, 2), 0).tolist() == []
    assert ir.invert_permutation(i64(2, 0, 3, 1)).tolist() == [1, 3, 0, 2]


def test_merge_sorted_by_hand():
    merged, source = ir.merge_sorted(i64(1, 3, 3, 7), i64(0, 3, 8))
    assert merged.tolist() == [0, 1, 3, 3, 3, 7, 8]
    assert source.tolist() == [4, 0, 1, 2, 5, 3, 6]      # the 3s: a's two first, then b's
    merged, source = ir.merge_sorted(i64(), i64(5, 5))
    assert merged.tolist() == [5, 5] and source.tolist() == [0, 1]
    merged, source = ir.merge_sorted(i64(ir.INT64_MAX), i64(ir.INT64_MIN, ir.INT64_MAX))
    assert source.tolist() == [1, 0, 2]


def test_spspmm_products_by_hand():
    # A = [[0 a0 a1], [a2 0 0]] (entries (0,1), (0,2), (1,0)); B rows: 0 -> {(0,1): 5}, 1 -> {}, 2 -> {(2,0): 7, (2,3): 9}
    rowA, colA, valA = i64(0, 0, 1), i64(1, 2, 0), np.array([2., 3., 4.], np.float32)
    rowptrB, colB, valB = i64(0, 1, 1, 3), i64(1, 0, 3), np.array([5., 7., 9.], np.float32)
    p = ir.spspmm_products(rowA, colA, valA, rowptrB, colB, valB, 4)
    assert p.counts.tolist() == [0, 2, 1] and p.offsets.tolist() == [0, 0, 2, 3] and p.owner.tolist() == [1, 1, 2]
    assert p.keys.tolist() == [0 * 4 + 0, 0 * 4 + 3, 1 * 4 + 1]
    assert p.vals.dtype == np.float32 and p.vals.tolist() == [21., 27., 20.]
    packed = ir.spspmm_products(rowA, colA, None, rowptrB, colB, valB, -1)
    assert packed.keys.tolist() == [(0 << 32) | 0, (3 << 32) | 0, (1 << 32) | 1]
    assert packed.vals.tolist() == [7., 9., 5.]
    assert ir.spspmm_products(rowA, colA, valA, rowptrB, colB, None, 4).vals.tolist() == [3., 3., 4.]
    assert ir.spspmm_products(rowA, colA, None, rowptrB, colB, None, 4).vals is None
    ints = ir.spspmm_products(rowA, colA, valA.astype(np.int64), rowptrB, colB, valB.astype(np.int64), 4)
    assert ints.vals.dtype == np.int64 and ints.vals.tolist() == [21, 27, 20]


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.int64])
def test_spspmm_readme_known_answer(kats, dtype):
    k = kats["spspmm"]
    idx, val = ir.spspmm(np.array(k["indexA"]), np.array(k["valueA"], dtype), np.array(k["indexB"]),
                         np.array(k["valueB"], dtype), k["m"], k["k"], k["n"])
    assert idx.tolist() == k["indexC"] and val.dtype == dtype and val.tolist() == k["valueC"]
    idx, val = ir.spspmm(np.array(k["indexA"]), None, np.array(k["indexB"]), None, k["m"], k["k"], k["n"])
    assert idx.tolist() == k["indexC"] and val is None


def test_spspmm_matches_dense_product():
    iA, iB = ir.random_coo(30, 20, 150, 1), ir.random_coo(20, 25, 120, 2)
    vA, vB = ir.small_int_values(iA.shape[1], np.float64, 3), ir.small_int_values(iB.shape[1], np.float64, 4)
    A, B = np.zeros((30, 20)), np.zeros((20, 25))
    A[iA[0], iA[1]], B[iB[0], iB[1]] = vA, vB
    idx, val = ir.spspmm(iA, vA, iB, vB, 30, 20, 25)
    C = np.zeros((30, 25))
    C[idx[0], idx[1]] = val
    assert np.array_equal(C, A @ B)
    SA, SB = np.zeros((30, 20), int), np.zeros((20, 25), int)
    SA[iA[0], iA[1]], SB[iB[0], iB[1]] = 1, 1
    assert idx.shape[1] == int((SA @ SB != 0).sum())  # structural product: zero and cancelled entries stay stored
    key = idx[0] * 25 + idx[1]
    assert np.all(key[1:] > key[:-1])
    ones_idx, ones_val = ir.spspmm(iA, None, iB, vB, 30, 20, 25)
    assert np.array_equal(ones_idx, idx) and ones_val.dtype == np.float64


# ---------------------------------------------------------------------------------------------
# count2ptr cases
# ---------------------------------------------------------------------------------------------

def test_scan_sizes_sit_at_the_edges():
    s = set(ir.SCAN_SIZES)
    for edge in (ir.WAVE, ir.SCAN_WAVE, ir.SCAN_TILE, 2 * ir.SCAN_TILE, ir.SCAN_TILE * ir.SCAN_SPLIT):
        assert {edge - 1, edge, edge + 1} <= s
    assert (ir.SCAN_WAVE, ir.SCAN_TILE, ir.SCAN_SPLIT) == (512, 2048, 1024)
    per = {n: ir.scan_per(n) for n in ir.SCAN_SIZES}
    assert per[ir.SCAN_TILE * ir.SCAN_SPLIT] == 1 and per[ir.SCAN_TILE * ir.SCAN_SPLIT + 1] == 2
    assert per[ir.SCAN_TILE * (ir.SCAN_SPLIT + 1) + 1] == 2 and ir.scan_blocks(ir.SCAN_TILE * (ir.SCAN_SPLIT + 1) + 1) == 1026
    assert max(ir.SCAN_SIZES) == 2048 * 2049 + 5 and per[max(ir.SCAN_SIZES)] == 3
    assert max(ir.SCAN_SIZES) * 8 < 35_000_000                      # 34 MB, the largest array
    assert ir.SCAN_LARGE == tuple(sorted(ir.SCAN_SIZES)[-3:])
    # the tests the suite had stop below per = 2
    assert ir.scan_per(2_000_000) == 1 and ir.scan_blocks(2_000_000) == 977


@pytest.mark.parametrize("n", ir.SCAN_SIZES)
def test_scan_cases_have_the_structure_they_claim(n):
    labels = [label for label, _ in ir.scan_cases(n)]
    assert len(set(labels)) == len(labels)
    want = {"ones", "random"} | ({"zeros", "alternating"} if n not in ir.SCAN_LARGE else set())
    assert {x for x in labels if not x.startswith("carry@")} == want
    pos = ir.scan_carry_positions(n)
    assert [f"carry@{p}" for p in pos] == [x for x in labels if x.startswith("carry@")]
    cand = (0, 63, 64, 511, 512, 2047, 2048, 2048 * 1023 + 2047, 2048 * 1024, n - 1)
    assert pos == sorted({p for p in cand if 0 <= p < n}) and 0 in pos and n - 1 in pos
    for label, kw in ir.scan_cases(n):
        c = ir.scan_counts(n, **kw)
        assert c.dtype == np.int64 and c.shape == (n,) and c.min() >= 0
        total = ir.exact_sum(c)
        assert total < 1 << 63
        ptr = ir.count2ptr(c)
        assert int(ptr[0]) == 0 and int(ptr[-1]) == total           # so the int64 cumsum never wrapped
        if label.startswith("carry@"):
            p = kw["p"]
            assert total == 1 << 40 > 1 << 32 and int(c[p]) == 1 << 40 and np.count_nonzero(c) == 1
            assert np.all(ptr[:p + 1] == 0) and np.all(ptr[p + 1:] == 1 << 40)
        elif label == "ones":
            assert np.array_equal(ptr, np.arange(n + 1))
        elif label == "zeros":
            assert total == 0
        elif label == "alternating":
            assert np.all(c[0::2] == 0) and np.all(c[1::2] == (1 << 31) + 1)
            assert n < 4 or total > 1 << 32
        elif label == "random":
            assert c.max() < 1 << 33
            assert n < 64 or (total > 1 << 32 and c.max() >= 1 << 32)


# ---------------------------------------------------------------------------------------------
# gather cases
# ---------------------------------------------------------------------------------------------

def test_gather_sweep_reaches_every_width_both_ways_and_both_index_forms():
    assert ir.GATHER_ROW_BYTES == (1, 2, 3, 4, 6, 8, 12, 16, 24, 40, 48, 64, 80, 512, 520)
    assert ir.GATHER_OFFSETS == (0, 1, 2, 4, 8) and ir.GATHER_N == (1, 255, 257, 1000)
    by_size, by_alignment, chunks = set(), set(), set()
    for rb in ir.GATHER_ROW_BYTES:
        by_size.add(ir.gather_width(rb, 0, 0))
        for so in ir.GATHER_OFFSETS:
            for oo in ir.GATHER_OFFSETS:
                w = ir.gather_width(rb, so, oo)
                if w < ir.gather_width(rb, 0, 0):
                    by_alignment.add(w)
                chunks.add(rb // w)
    assert by_size == {16, 8, 4, 2, 1}
    assert by_alignment == {8, 4, 2, 1}          # 16 is never a narrowing
    assert {1, 2, 4, 8, 16, 32} <= chunks        # shift form
    assert {3, 5, 65} <= chunks                  # division form


@pytest.mark.parametrize("n", ir.GATHER_N)
def test_gather_perm_has_repeats_and_both_ends(n):
    R = ir.gather_rows_of(n)
    perm = ir.gather_perm(n, R, n)
    assert perm.dtype == np.int64 and perm.shape == (n,) and perm.min() == 0 and perm.max() == R - 1
    assert n == 1 or np.unique(perm).size < n


@pytest.mark.parametrize("name", sorted(ir.WINDOW_CASES))
def test_window_cases_cover_every_class_the_dtype_allows(name):
    size = ir.WINDOW_ITEMSIZE[name]
    cases = ir.WINDOW_CASES[name]
    for cls, W, col0, width in cases:
        assert 0 <= col0 and 0 < width and col0 + width <= W
        assert ir.window_class(size, W, col0, width) == cls, (cls, W, col0, width)
    allowed = {8: {"16", "4"}, 4: {"16", "4", "8row"}, 2: {"16", "4", "8row", "2"}, 1: {"16", "4", "8row", "2", "1"}}[size]
    assert {c[0] for c in cases} == allowed
    for cls in allowed - {"8row"}:
        mine = [c[1:] for c in cases if c[0] == cls]
        assert any(col0 == 0 and width < W for W, col0, width in mine)
        assert any(col0 > 0 and col0 + width == W for W, col0, width in mine)
        assert any(width == W for W, col0, width in mine)
    # a chunk count that is no power of two, in the 16-byte and in the 4-byte kernel
    for kernel in (16, 4):
        counts = [width * size // kernel for cls, W, col0, width in cases
                  if ir.window_width(W * size, col0 * size, width * size) == kernel]
        assert any(c & (c - 1) for c in counts), (name, kernel, counts)
    assert ir.window_width(64, 16, 32, src_off=4) == 4 and ir.window_width(64, 16, 32, src_off=1) == 1


# ---------------------------------------------------------------------------------------------
# key cases
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", ir.KEY_N)
def test_key_streams(n):
    assert ir.inversion_positions(n) == [1, 63, 64, 65, 255, 256, 257, 511, 512, n - 1]
    a, b = ir.sorted_stream(n, n)
    keys, flag = ir.make_keys(a, b, ir.KEY_MUL)
    assert flag == 0 and np.all(keys[1:] > keys[:-1]) and b.min() >= 0 and b.max() < ir.KEY_MUL and a.max() > 1000
    for i in ir.inversion_positions(n):
        ai, bi = ir.inversion_stream(n, i, n)
        ki, fi = ir.make_keys(ai, bi, ir.KEY_MUL)
        assert fi == 1 and np.flatnonzero(ki[1:] < ki[:-1]).tolist() == [i - 1]   # key i below key i - 1, nowhere else
        assert np.array_equal(np.sort(ki), keys)
    a, b = ir.sorted_stream(n, n, equal_runs=True)
    keys, flag = ir.make_keys(a, b, ir.KEY_MUL)
    assert flag == 0
    for lo, hi in ir.EQUAL_RUNS:
        assert np.all(keys[lo:hi] == keys[lo]) and keys[lo - 1] < keys[lo] < keys[hi]
    assert any(lo < 64 < hi for lo, hi in ir.EQUAL_RUNS) and any(lo < 256 < hi for lo, hi in ir.EQUAL_RUNS)


def test_single_key_stream():
    a, b = ir.sorted_stream(1)
    assert a.shape == b.shape == (1,) and ir.make_keys(a, b, ir.KEY_MUL)[1] == 0


def test_split_stream_mixes_both_division_paths_in_every_wave():
    assert ir.SPLIT_KEYS == (0, 1, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 1, 2**40 + 7, 2**62)
    assert ir.SPLIT_DIVS == (1, 3, 2**32 - 1, 2**32, 2**32 + 1) and ir.SPLIT_N == (255, 256, 257)
    for n in ir.SPLIT_N:
        keys = ir.split_stream(n)
        assert keys.shape == (n,) and set(keys.tolist()) == set(ir.SPLIT_KEYS)
        for w in range(0, n, 64):
            wave = keys[w:w + 64]
            assert wave.size < 8 or ((wave < 2**32).any() and (wave >= 2**32).any())
        for div in ir.SPLIT_DIVS:
            hi, lo = ir.split_keys(keys, div)
            assert [int(h) * div + int(l) for h, l in zip(hi, lo)] == keys.tolist() and lo.max() < div and lo.min() >= 0


@pytest.mark.parametrize("n", ir.PERM_N)
@pytest.mark.parametrize("kind", ir.PERM_KINDS)
def test_permutations(n, kind):
    perm = ir.permutation(n, kind)
    assert np.array_equal(np.sort(perm), np.arange(n))
    inv = ir.invert_permutation(perm)
    assert np.array_equal(inv[perm], np.arange(n)) and np.array_equal(perm[inv], np.arange(n))
    if kind == "stride257" and n > 257:
        assert perm[1] == 257 and not np.array_equal(perm, inv)


# ---------------------------------------------------------------------------------------------
# merge cases
# ---------------------------------------------------------------------------------------------

def test_merge_case_list():
    names = list(ir.MERGE_CASES)
    assert len(names) == len(ir.merge_cases())
    T = ir.MERGE_TILE
    assert ir.MERGE_TOTALS == (1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 64 * T + 1)
    for total in ir.MERGE_TOTALS:
        for na in {0, 1, total // 2, total - 1, total}:
            if 0 <= na <= total:
                assert f"total{total}-na{na}" in names
    assert ir.MERGE_RUNS == (1, 63, 64, 65, T - 1, T, T + 1) and all(f"runs{L}" in names for L in ir.MERGE_RUNS)
    for other in ("alternating", "alternating-reverse", "identical-distinct", "identical-equal-runs", "sparse-in-dense",
                  "dense-in-sparse", "extremes"):
        assert other in names
    for where in ("below", "middle", "above"):
        assert f"long-short-{where}" in names and f"short-long-{where}" in names


@pytest.mark.parametrize("name", list(ir.MERGE_CASES))
def test_merge_cases_are_sorted_and_shaped_as_named(name):
    a, b = ir.MERGE_CASES[name]()
    for x in (a, b):
        assert x.dtype == np.int64 and x.ndim == 1 and np.all(x[1:] >= x[:-1])
    merged, source = ir.merge_sorted(a, b)
    assert np.all(merged[1:] >= merged[:-1]) and np.array_equal(np.sort(source), np.arange(a.size + b.size))
    from_b = source >= a.size
    edges = np.flatnonzero(from_b[1:] != from_b[:-1]) + 1
    runs = np.diff(np.concatenate([[0], edges, [source.size]]))   # lengths of the single-source runs of the merge
    if name.startswith("total"):
        total, na = (int(x[len(p):]) for x, p in zip(name.split("-"), ("total", "na")))
        assert (a.size, b.size) == (na, total - na)
        if total > 100:
            assert np.unique(merged).size < total          # ties
    elif name.startswith("alternating"):
        assert a.size == b.size == 5000 and np.all(runs == 1) and bool(from_b[0]) == (name == "alternating-reverse")
    elif name.startswith("runs"):
        L = int(name[4:])
        assert np.all(runs[:-1] == L) and runs.size >= 4 and merged.size > 3 * ir.MERGE_TILE and not from_b[0]
    elif name == "identical-distinct":
        assert np.array_equal(a, b) and np.unique(a).size == a.size and np.all(runs == 1) and not from_b[0]
    elif name == "identical-equal-runs":
        assert np.array_equal(a, b) and np.all(runs[:-2] == 3 * ir.MERGE_TILE) and not from_b[0]
        # ties resolve to a first: inside one key, all of a's entries precede all of b's
        assert np.array_equal(merged[::2 * 3 * ir.MERGE_TILE], np.unique(a))
    elif name in ("sparse-in-dense", "dense-in-sparse"):
        few = from_b if name == "dense-in-sparse" else ~from_b
        assert np.array_equal(np.flatnonzero(few), np.arange(ir.MERGE_TILE - 1, merged.size, ir.MERGE_TILE))
        assert int(few.sum()) == 10
    elif name.startswith(("long-short", "short-long")):
        long, short = (a, b) if name.startswith("long") else (b, a)
        assert long.size == 300_000 and short.size == 3
        at = np.flatnonzero(from_b if name.startswith("long") else ~from_b)
        where = name.rsplit("-", 1)[1]
        if where == "below":
            assert at.tolist() == [0, 1, 2]
        elif where == "above":
            assert at.tolist() == [300_000, 300_001, 300_002]
        else:
            assert 100_000 < at[0] and at[-1] < 200_003 and np.isin(short[:2], long).all() and not np.isin(short[2], long)
    elif name == "extremes":
        for x in (a, b):
            assert {ir.INT64_MIN, -1, 0, ir.INT64_MAX} <= set(x.tolist())
            assert x[0] == ir.INT64_MIN and x[-1] == ir.INT64_MAX
    else:
        raise AssertionError(name)


# ---------------------------------------------------------------------------------------------
# expand cases
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ir.EXPAND_CASES)
def test_expand_cases(name):
    c = ir.expand_case(name)
    deg = np.diff(c.rowptrB)
    assert c.rowptrB.size == c.k + 1 and int(c.rowptrB[-1]) == c.colB.size and c.colB.max() < c.n
    assert c.colA.min() >= 0 and c.colA.max() < c.k and c.rowA.max() < c.m and c.rowA.size == c.colA.size
    assert deg[0] == 0 and deg[-1] == 0 and 0 in c.colA and c.k - 1 in c.colA   # A points at both empty rows
    p = ir.spspmm_products(c.rowA, c.colA, None, c.rowptrB, c.colB, None, c.n)
    assert int(p.offsets[-1]) == p.keys.size == p.owner.size
    if name == "big":
        assert deg.max() == 5000 and int((deg[c.colA] == 1).sum()) == 5000 and int((deg[c.colA] == 5000).sum()) == 3
        assert p.keys.size == 5000 + 3 * 5000
    else:
        assert p.keys.size == int(name[5:]) and p.keys.size in (255, 256, 257)
    # products of an A entry are contiguous, in B's storage order
    for e in (0, c.colA.size // 2, c.colA.size - 1):
        lo, hi = int(p.offsets[e]), int(p.offsets[e + 1])
        cols = c.colB[c.rowptrB[c.colA[e]]:c.rowptrB[c.colA[e] + 1]]
        assert np.array_equal(p.keys[lo:hi], c.rowA[e] * c.n + cols) and np.all(p.owner[lo:hi] == e)


def test_small_int_values_are_exact_in_every_type():
    for dtype in (np.float32, np.float64, np.int32, np.int64):
        v = ir.small_int_values(1000, dtype, 1)
        assert v.dtype == dtype and v.min() == -4 and v.max() == 4
    # 5000 products of magnitude <= 16 stay far below 2^24, where fp32 stops holding every integer
    assert 5000 * 16 < 1 << 24
