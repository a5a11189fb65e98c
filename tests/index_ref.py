"""Plain numpy restatements of the index kernels every sparse op is stitched from, and the structured
inputs their tests run.  CPU only: numpy and the standard library, no GPU, no package import.

The kernels (csrc/util.hip, csrc/merge.hip, csrc/spspmm.hip) and the one-line statement each is held to:

    count2ptr            [0, cumsum(counts)] in int64
    gather_rows(_window) out[i, :] = the bytes [first, first + row_bytes) of source row perm[i]
    make_keys            a * mul + b, and "some key is smaller than its predecessor"
    split_keys           divmod(keys, div)
    bincount             occurrences of every index inside [0, size); the others are ignored
    invert_permutation   inv[perm[i]] = i
    merge_sorted         np.argsort(concat(a, b), kind="stable"): a's entry first on equal keys
    spspmm_count/expand  one (key, value) per product, A's storage order, then B's inside one A entry

The generators below place sizes, carries, inversions and run lengths AT the edges of the kernels' tiles:

    scan   (count2ptr)   a wave scans 512 counts, a workgroup 2048 (SCAN_TILE); the block sums are scanned
                         by ONE workgroup of 1024 threads, `per = ceil(blocks / 1024)` sums each
    keys   (make_keys)   the predecessor of element i lives in another lane (any i), another wave
                         (i % 64 == 0) or another workgroup (i % 256 == 0)
    merge  (merge_sorted) a workgroup produces 2048 merged keys (MERGE_TILE); its split is searched 64 probes
                         a round
    gather               the element width (16, 8, 4, 2, 1 bytes) follows the row size AND the alignment of
                         both operands; a power-of-two chunk count takes a shift, any other a division

tests/test_index_ref.py pins the restatements to hand-written answers and asserts that every generator has the
structure it claims; tests/test_index_kernels_gpu.py draws the same inputs for the kernels.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

WAVE = 64
BLOCK = 256           # threads of the one-element-per-thread kernels
SCAN_ITEMS = 8
SCAN_WAVE = WAVE * SCAN_ITEMS     # 512 counts per wave
SCAN_TILE = BLOCK * SCAN_ITEMS    # 2048 counts per workgroup
SCAN_SPLIT = 1024                 # threads of the second-level scan
MERGE_TILE = 2048
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


# ---------------------------------------------------------------------------------------------
# restatements
# ---------------------------------------------------------------------------------------------

def count2ptr(counts: np.ndarray) -> np.ndarray:
    """[0, counts[0], counts[0] + counts[1], ...] as int64[n + 1]."""
    counts = np.asarray(counts, np.int64)
    out = np.zeros(counts.size + 1, np.int64)
    np.cumsum(counts, out=out[1:])
    return out


def gather_bytes(src_bytes: np.ndarray, perm: np.ndarray, row_bytes: int, stride: Optional[int] = None,
                 first: int = 0) -> np.ndarray:
    """uint8[n, row_bytes]: row i holds the bytes [first, first + row_bytes) of source row perm[i], the rows of
    the flat uint8 array `src_bytes` being `stride` bytes apart (default: row_bytes, rows back to back)."""
    src_bytes = np.asarray(src_bytes, np.uint8).reshape(-1)
    perm = np.asarray(perm, np.int64)
    stride = row_bytes if stride is None else stride
    assert 0 <= first and first + row_bytes <= stride
    at = perm[:, None] * stride + first + np.arange(row_bytes, dtype=np.int64)[None, :]
    return src_bytes[at]


def make_keys(a: np.ndarray, b: np.ndarray, mul: int) -> Tuple[np.ndarray, int]:
    """(a * mul + b, 1 if some key is smaller than its predecessor else 0)."""
    keys = np.asarray(a, np.int64) * np.int64(mul) + np.asarray(b, np.int64)
    return keys, int(bool(np.any(keys[1:] < keys[:-1])))


def split_keys(keys: np.ndarray, div: int) -> Tuple[np.ndarray, np.ndarray]:
    """divmod(keys, div) for non-negative keys and a positive divisor."""
    keys = np.asarray(keys, np.int64)
    assert div > 0 and (keys.size == 0 or keys.min() >= 0)
    hi, lo = np.divmod(keys, np.int64(div))
    return hi, lo


def bincount(index: np.ndarray, size: int) -> np.ndarray:
    """int64[size]: occurrences of every value of [0, size) in index; values outside are ignored."""
    index = np.asarray(index, np.int64)
    inside = index[(index >= 0) & (index < size)]
    return np.bincount(inside, minlength=size).astype(np.int64)[:size]


def invert_permutation(perm: np.ndarray) -> np.ndarray:
    perm = np.asarray(perm, np.int64)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size, dtype=np.int64)
    return inv


def merge_sorted(a: np.ndarray, b: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(merged keys, source): source indexes concat(a, b); equal keys keep concatenation order, so a's come first."""
    both = np.concatenate([np.asarray(a, np.int64), np.asarray(b, np.int64)])
    source = np.argsort(both, kind="stable").astype(np.int64)
    return both[source], source


class Products(NamedTuple):
    keys: np.ndarray              # int64[total]
    vals: Optional[np.ndarray]    # dtype[total], None when neither operand has values
    counts: np.ndarray            # int64[nnzA]: entries of B's row colA[e]
    offsets: np.ndarray           # int64[nnzA + 1]: count2ptr(counts)
    owner: np.ndarray             # int64[total]: the A entry of product p


def spspmm_products(rowA, colA, valA, rowptrB, colB, valB, n: int) -> Products:
    """Every partial product of A @ B in the expand kernel's order: A's storage order and, inside one A entry
    e = (i, c, a), B's storage order over the entries (c, j, b) of B's row c.  Key i * n + j, or for n < 0 the
    packed (j << 32) | i.  An operand without values counts as ones; the value dtype is the given operand's."""
    rowA, colA = np.asarray(rowA, np.int64), np.asarray(colA, np.int64)
    rowptrB, colB = np.asarray(rowptrB, np.int64), np.asarray(colB, np.int64)
    counts = rowptrB[colA + 1] - rowptrB[colA]
    offsets = count2ptr(counts)
    total = int(offsets[-1])
    owner = np.repeat(np.arange(colA.size, dtype=np.int64), counts)
    q = rowptrB[colA[owner]] + (np.arange(total, dtype=np.int64) - offsets[owner])
    i, j = rowA[owner], colB[q]
    keys = ((j << np.int64(32)) | i) if n < 0 else i * np.int64(n) + j
    vals = None
    if valA is not None or valB is not None:
        dtype = (valA if valA is not None else valB).dtype
        va = np.ones(total, dtype) if valA is None else np.asarray(valA)[owner]
        vb = np.ones(total, dtype) if valB is None else np.asarray(valB)[q]
        assert va.dtype == vb.dtype == dtype
        vals = va * vb
    return Products(keys, vals, counts, offsets, owner)


def spspmm(indexA, valA, indexB, valB, m: int, k: int, n: int):
    """(index int64[2, nnzC], value | None) of A @ B for coalesced COO operands: the products of
    `spspmm_products` brought into key order by a stable sort (so every entry adds its terms in the order a
    row-by-row Gustavson product meets them) and summed run by run, left to right, in the value dtype."""
    indexA, indexB = np.asarray(indexA, np.int64), np.asarray(indexB, np.int64)
    assert indexA.shape[0] == 2 and indexB.shape[0] == 2
    assert indexA.size == 0 or (indexA[0].max() < m and indexA[1].max() < k)
    rowptrB = count2ptr(bincount(indexB[0], k))
    p = spspmm_products(indexA[0], indexA[1], valA, rowptrB, indexB[1], valB, n)
    order = np.argsort(p.keys, kind="stable")
    keys = p.keys[order]
    head = np.ones(keys.size, bool)
    head[1:] = keys[1:] != keys[:-1]
    starts = np.flatnonzero(head)
    uniq = keys[starts]
    index = np.stack([uniq // n, uniq % n]).astype(np.int64)
    if p.vals is None:
        return index, None
    vals = p.vals[order]
    out = np.zeros(starts.size, vals.dtype)
    ends = np.append(starts[1:], keys.size)
    for s, (lo, hi) in enumerate(zip(starts, ends)):
        acc = vals[lo]
        for t in range(lo + 1, hi):
            acc = acc + vals[t]
        out[s] = acc
    return index, out


# ---------------------------------------------------------------------------------------------
# count2ptr cases
# ---------------------------------------------------------------------------------------------

SCAN_SIZES = (1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097,
              SCAN_TILE * SCAN_SPLIT - 1, SCAN_TILE * SCAN_SPLIT, SCAN_TILE * SCAN_SPLIT + 1,
              SCAN_TILE * (SCAN_SPLIT + 1) + 1,   # 1026 blocks: per = 2, the last threads of the second level idle
              SCAN_TILE * 2049 + 5)               # 2050 blocks: per = 3
SCAN_LARGE = SCAN_SIZES[-3:]   # these run "ones", the single carries and "random" only
SCAN_CARRY = 1 << 40
SCAN_ALT = (1 << 31) + 1
SCAN_RANDOM_BOUND = 1 << 33


def scan_blocks(n: int) -> int:
    return -(-n // SCAN_TILE)


def scan_per(n: int) -> int:
    """Block sums each thread of the second-level scan takes."""
    return -(-scan_blocks(n) // SCAN_SPLIT)


def scan_carry_positions(n: int) -> List[int]:
    """Where the single 2^40 sits: first and last element of a wave's item, of a wave, of a tile, the last
    element a second-level thread owns alone (block 1023) and the first of block 1024, and the end."""
    cand = (0, 63, 64, 511, 512, 2047, 2048, SCAN_TILE * (SCAN_SPLIT - 1) + 2047, SCAN_TILE * SCAN_SPLIT, n - 1)
    return sorted({p for p in cand if 0 <= p < n})


def scan_counts(n: int, pattern: str, p: int = 0, seed: int = 0) -> np.ndarray:
    """int64[n] of one pattern: "zeros", "ones", "carry" (2^40 at p, zeros elsewhere: every later pointer must
    carry it over each wave, tile and second-level edge behind p), "alternating" (0, 2^31 + 1, 0, ...: sums pass
    2^32 after four elements) and "random" (seeded, uniform in [0, 2^33))."""
    if pattern == "zeros":
        return np.zeros(n, np.int64)
    if pattern == "ones":
        return np.ones(n, np.int64)
    if pattern == "carry":
        c = np.zeros(n, np.int64)
        c[p] = SCAN_CARRY
        return c
    if pattern == "alternating":
        return (np.arange(n, dtype=np.int64) & 1) * SCAN_ALT
    if pattern == "random":
        return np.random.default_rng(seed).integers(0, SCAN_RANDOM_BOUND, n, dtype=np.int64)
    raise KeyError(pattern)


def scan_cases(n: int) -> List[Tuple[str, dict]]:
    """(label, scan_counts keyword arguments) of every pattern size n runs."""
    cases = [("ones", {"pattern": "ones"})]
    cases += [(f"carry@{p}", {"pattern": "carry", "p": p}) for p in scan_carry_positions(n)]
    cases += [("random", {"pattern": "random", "seed": n % 1000})]
    if n not in SCAN_LARGE:
        cases += [("zeros", {"pattern": "zeros"}), ("alternating", {"pattern": "alternating"})]
    return cases


def exact_sum(x: np.ndarray) -> int:
    """Sum of non-negative int64 as a Python int (no wrap)."""
    x = np.asarray(x, np.int64)
    return (int((x >> 32).sum()) << 32) + int((x & 0xffffffff).sum())


# ---------------------------------------------------------------------------------------------
# gather cases
# ---------------------------------------------------------------------------------------------

GATHER_ROW_BYTES = (1, 2, 3, 4, 6, 8, 12, 16, 24, 40, 48, 64, 80, 512, 520)
GATHER_OFFSETS = (0, 1, 2, 4, 8)     # start of an operand, in bytes past a 16-byte boundary
GATHER_N = (1, 255, 257, 1000)
GATHER_WIDTHS = (16, 8, 4, 2, 1)


def gather_rows_of(n: int) -> int:
    """Source rows R for a gather of n rows: one for n = 1 (row 0 is also row R - 1), else 97."""
    return 1 if n == 1 else 97


def gather_perm(n: int, R: int, seed: int = 0) -> np.ndarray:
    """int64[n] in [0, R) with rows 0 (last) and R - 1 (first) present (n = 1 and R > 1: row R - 1 only); n > R
    makes repeats certain."""
    perm = np.random.default_rng(seed).integers(0, R, n, dtype=np.int64)
    perm[-1], perm[0] = 0, R - 1
    return perm


def gather_width(row_bytes: int, src_off: int, out_off: int) -> int:
    """Element width psa_gather_rows picks: the largest of 16, 8, 4, 2, 1 that divides the row size and both
    start addresses."""
    for w in GATHER_WIDTHS:
        if row_bytes % w == 0 and src_off % w == 0 and out_off % w == 0:
            return w
    raise AssertionError


def window_width(row_bytes: int, offset_bytes: int, width_bytes: int, src_off: int = 0, out_off: int = 0) -> int:
    """Element width psa_gather_rows_window picks (16, 4 or 1): by the OR of row size, offset and width, and
    both start addresses."""
    every = row_bytes | offset_bytes | width_bytes
    for w in (16, 4, 1):
        if every % w == 0 and src_off % w == 0 and out_off % w == 0:
            return w
    raise AssertionError


WINDOW_R = 300
WINDOW_N = (1, 257, 1000)
WINDOW_ITEMSIZE = {"float32": 4, "bfloat16": 2, "uint8": 1, "float64": 8}
# the classes of (row bytes | offset bytes | width bytes): "16" a multiple of 16; "4" of 4, not of 16; "8row" a row
# size that is a multiple of 8 while the offset is a multiple of 4 only (and the width of 4 only); "2" of 2 only;
# "1" odd.  A dtype runs the classes its element size allows (float64: every byte count is a multiple of 8).
# (W, col0, width) in ELEMENTS.
WINDOW_CASES: Dict[str, List[Tuple[str, int, int, int]]] = {
    "float32": [("16", 16, 4, 8), ("16", 16, 0, 4), ("16", 16, 4, 12), ("16", 16, 0, 16), ("16", 20, 8, 12),
                ("4", 7, 2, 3), ("4", 7, 0, 5), ("4", 7, 4, 3), ("4", 7, 0, 7), ("4", 9, 1, 4),
                ("8row", 6, 1, 3), ("8row", 10, 3, 5)],
    "bfloat16": [("16", 32, 8, 16), ("16", 32, 0, 8), ("16", 32, 8, 24), ("16", 32, 0, 32),
                 ("4", 14, 4, 6), ("4", 14, 0, 10), ("4", 14, 8, 6), ("4", 14, 0, 14),
                 ("8row", 12, 2, 6),
                 ("2", 7, 1, 3), ("2", 7, 0, 5), ("2", 7, 4, 3), ("2", 7, 0, 7)],
    "uint8": [("16", 64, 16, 32), ("16", 64, 0, 48), ("16", 64, 16, 48), ("16", 64, 0, 64),
              ("4", 28, 8, 12), ("4", 28, 0, 20), ("4", 28, 16, 12), ("4", 28, 0, 28),
              ("8row", 24, 4, 12),
              ("2", 14, 2, 6), ("2", 14, 0, 10), ("2", 14, 8, 6), ("2", 14, 0, 14),
              ("1", 7, 1, 3), ("1", 7, 0, 5), ("1", 7, 4, 3), ("1", 7, 0, 7), ("1", 16, 0, 5)],
    "float64": [("16", 8, 2, 4), ("16", 8, 0, 2), ("16", 8, 2, 6), ("16", 8, 0, 8),
                ("4", 3, 1, 1), ("4", 3, 0, 2), ("4", 3, 1, 2), ("4", 3, 0, 3), ("4", 7, 2, 3)],
}


def window_class(itemsize: int, W: int, col0: int, width: int) -> str:
    rb, ob, wb = W * itemsize, col0 * itemsize, width * itemsize
    every = rb | ob | wb
    if every % 16 == 0:
        return "16"
    if every % 4 == 0:
        return "8row" if rb % 8 == 0 and ob % 8 != 0 and wb % 8 != 0 else "4"
    return "2" if every % 2 == 0 else "1"


# ---------------------------------------------------------------------------------------------
# make_keys / split_keys cases
# ---------------------------------------------------------------------------------------------

KEY_MUL = 1 << 20
KEY_N = (1000, 100_003)
EQUAL_RUNS = ((60, 70), (250, 262))   # [first, last) of the stretches of equal keys: across i = 64 and i = 256


def inversion_positions(n: int) -> List[int]:
    return sorted({i for i in (1, 63, 64, 65, 255, 256, 257, 511, 512, n - 1) if 0 < i < n})


def sorted_stream(n: int, seed: int = 0, equal_runs: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """(a, b) with b < KEY_MUL whose keys a * KEY_MUL + b increase strictly (gaps in [1, 2^22)); with
    `equal_runs` the keys of EQUAL_RUNS are equal instead (sorted still: the flag must stay 0)."""
    gaps = np.random.default_rng(seed).integers(1, 1 << 22, n, dtype=np.int64)
    if equal_runs:
        for lo, hi in EQUAL_RUNS:
            gaps[lo + 1:hi] = 0
    keys = np.cumsum(gaps)
    return keys >> 20, keys & (KEY_MUL - 1)


def inversion_stream(n: int, i: int, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """The strictly increasing stream with entries i - 1 and i exchanged: key i is smaller than key i - 1, and
    that is the only such place (key i + 1 is above both, key i - 2 below both)."""
    a, b = sorted_stream(n, seed)
    for x in (a, b):
        x[i - 1], x[i] = x[i], x[i - 1]
    return a, b


SPLIT_KEYS = (0, 1, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) + 7, 1 << 62)
SPLIT_DIVS = (1, 3, (1 << 32) - 1, 1 << 32, (1 << 32) + 1)
SPLIT_N = (255, 256, 257)


def split_stream(n: int) -> np.ndarray:
    """SPLIT_KEYS over and over: keys below and above 2^32 alternate inside every wave."""
    return np.resize(np.array(SPLIT_KEYS, np.int64), n)


# ---------------------------------------------------------------------------------------------
# invert_permutation cases
# ---------------------------------------------------------------------------------------------

PERM_N = (1, 255, 256, 257, 100_003)
PERM_KINDS = ("identity", "reversal", "stride257")


def permutation(n: int, kind: str) -> np.ndarray:
    idx = np.arange(n, dtype=np.int64)
    if kind == "identity":
        return idx
    if kind == "reversal":
        return idx[::-1].copy()
    if kind == "stride257":  # the transpose-like order of tests/test_sort_gpu.py
        w = 257
        return np.argsort((idx % w) * (n // w + 1) + idx // w, kind="stable").astype(np.int64)
    raise KeyError(kind)


# ---------------------------------------------------------------------------------------------
# merge cases
# ---------------------------------------------------------------------------------------------

MERGE_TOTALS = (1, 2047, 2048, 2049, 4095, 4096, 4097, 64 * MERGE_TILE + 1)
MERGE_RUNS = (1, 63, 64, 65, 2047, 2048, 2049)
MERGE_LONG, MERGE_SHORT = 300_000, 3
MERGE_EQUAL_RUN = 3 * MERGE_TILE


def merge_splits(total: int) -> List[int]:
    return sorted({0, 1, total // 2, total - 1, total} & set(range(total + 1)))


def _split(keys: np.ndarray, na: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    pick = np.zeros(keys.size, bool)
    pick[np.random.default_rng(seed).choice(keys.size, na, replace=False)] = True
    return keys[pick], keys[~pick]


def merge_split(total: int, na: int, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """`total` sorted keys drawn from [0, total / 4] (ties everywhere, between the streams and inside each), a
    random na of them to a, the rest to b."""
    rng = np.random.default_rng(seed)
    keys = np.sort(rng.integers(0, total // 4 + 1, total, dtype=np.int64))
    return _split(keys, na, seed + 1)


def merge_alternating(n: int, reverse: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """a the even numbers below 2 n, b the odd ones (reverse: the other way round): the merge takes one key from
    each stream in turn."""
    even, odd = np.arange(0, 2 * n, 2, dtype=np.int64), np.arange(1, 2 * n, 2, dtype=np.int64)
    return (odd, even) if reverse else (even, odd)


def merge_runs(L: int) -> Tuple[np.ndarray, np.ndarray]:
    """The keys 0 .. N - 1 in blocks of L: even blocks to a, odd ones to b.  N covers four blocks and three
    tiles, plus 17."""
    N = max(4 * L, 3 * MERGE_TILE) + 17
    keys = np.arange(N, dtype=np.int64)
    to_b = (keys // L) % 2 == 1
    return keys[~to_b], keys[to_b]


def merge_identical(equal_runs: bool) -> Tuple[np.ndarray, np.ndarray]:
    """a == b: distinct keys (3 i), or runs of 3 * 2048 equal keys (a tie of 6 * 2048 entries over six tiles, all
    of a's before all of b's)."""
    if equal_runs:
        a = np.arange(3 * MERGE_EQUAL_RUN + 100, dtype=np.int64) // MERGE_EQUAL_RUN
    else:
        a = 3 * np.arange(5000, dtype=np.int64)
    return a, a.copy()


def merge_sparse_in_dense(mirror: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """One key of a per 2047 keys of b: the keys 0 .. N - 1, every 2048th (2047, 4095, ...) to a."""
    keys = np.arange(10 * MERGE_TILE + 5, dtype=np.int64)
    to_a = keys % MERGE_TILE == MERGE_TILE - 1
    return (keys[~to_a], keys[to_a]) if mirror else (keys[to_a], keys[~to_a])


def merge_long_short(where: str, mirror: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """300 000 keys (10 + 2 i) against 3: "below" all of them, in the "middle" (two equal to a long key, one
    between two) or "above" all."""
    long = 10 + 2 * np.arange(MERGE_LONG, dtype=np.int64)
    mid = int(long[MERGE_LONG // 2])
    short = {"below": [0, 1, 9], "middle": [mid, mid, mid + 1], "above": [int(long[-1]) + 1] * 2 + [INT64_MAX]}[where]
    short = np.array(short, np.int64)
    return (short, long) if mirror else (long, short)


def merge_extremes(seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """int64 min, -1, 0 and int64 max in both streams, among 3000 keys each from the whole int64 range."""
    rng = np.random.default_rng(seed)
    fixed = np.array([INT64_MIN, -1, 0, INT64_MAX], np.int64)
    out = []
    for _ in range(2):
        body = rng.integers(INT64_MIN, INT64_MAX, 3000, dtype=np.int64, endpoint=True)
        out.append(np.sort(np.concatenate([fixed, fixed[:2], body])))
    return out[0], out[1]


def merge_cases() -> List[Tuple[str, Tuple[np.ndarray, np.ndarray]]]:
    """(name, thunk) of every merge case; call the thunk for (a, b)."""
    cases = []
    for t, total in enumerate(MERGE_TOTALS):
        for na in merge_splits(total):
            cases.append((f"total{total}-na{na}", (lambda total=total, na=na, t=t: merge_split(total, na, 10 * t))))
    cases.append(("alternating", lambda: merge_alternating(5000)))
    cases.append(("alternating-reverse", lambda: merge_alternating(5000, True)))
    for L in MERGE_RUNS:
        cases.append((f"runs{L}", (lambda L=L: merge_runs(L))))
    cases.append(("identical-distinct", lambda: merge_identical(False)))
    cases.append(("identical-equal-runs", lambda: merge_identical(True)))
    cases.append(("sparse-in-dense", lambda: merge_sparse_in_dense()))
    cases.append(("dense-in-sparse", lambda: merge_sparse_in_dense(True)))
    for where in ("below", "middle", "above"):
        cases.append((f"long-short-{where}", (lambda where=where: merge_long_short(where))))
        cases.append((f"short-long-{where}", (lambda where=where: merge_long_short(where, True))))
    cases.append(("extremes", lambda: merge_extremes()))
    return cases


MERGE_CASES = dict(merge_cases())


# ---------------------------------------------------------------------------------------------
# spspmm_count / spspmm_expand cases
# ---------------------------------------------------------------------------------------------

class ExpandCase(NamedTuple):
    rowA: np.ndarray
    colA: np.ndarray
    rowptrB: np.ndarray
    colB: np.ndarray
    m: int
    k: int
    n: int


EXPAND_BIG_ROW = 5000
EXPAND_SMALL_TOTALS = (255, 256, 257)
EXPAND_CASES = ("big",) + tuple(f"total{t}" for t in EXPAND_SMALL_TOTALS)


def _csr(lengths, n: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """rowptr and sorted distinct columns below n for rows of the given lengths."""
    rng = np.random.default_rng(seed)
    cols = [np.sort(rng.choice(n, int(d), replace=False)).astype(np.int64) for d in lengths]
    return count2ptr(np.array(lengths, np.int64)), (np.concatenate(cols) if cols else np.zeros(0, np.int64))


def expand_case(name: str) -> ExpandCase:
    """"big": B has 14 rows, the first and the last empty, row 6 with 5000 entries, the other eleven with one; A
    (500 x 14) has 5000 entries in ten of the one-entry columns, its rows 0 .. 2 also meet row 6 of B, and rows 0 and
    499 point at B's two empty rows.  "total255" / "total256" / "total257": B has 6 rows of 0, 1, 2, 50, 3, 0
    entries and A's entries are chosen so that exactly that many products exist (the last workgroup of the
    expand kernel is full but for one, full, or one over); A points at both empty rows."""
    if name == "big":
        k, n, m = 14, EXPAND_BIG_ROW, 500
        lengths = [0] + [1] * 5 + [EXPAND_BIG_ROW] + [1] * 6 + [0]
        rowptrB, colB = _csr(lengths, n, 1)
        one = [1, 2, 3, 4, 5, 7, 8, 9, 10, 11]
        rows = []
        for i in range(m):
            cols = list(one) + ([6] if i < 3 else []) + ([0, 13] if i in (0, m - 1) else [])
            rows += [(i, c) for c in sorted(cols)]
        ic = np.array(rows, np.int64)
        return ExpandCase(ic[:, 0].copy(), ic[:, 1].copy(), rowptrB, colB, m, k, n)
    total = int(name[len("total"):])
    k, n = 6, 64
    lengths = [0, 1, 2, 50, 3, 0]
    rowptrB, colB = _csr(lengths, n, 2)
    cols, need = [0], total          # the first A entry points at the empty first row
    for c in (3, 4, 2, 1):
        while need >= lengths[c]:
            cols.append(c)
            need -= lengths[c]
    assert need == 0
    cols.insert(len(cols) // 2, 5)   # and one in the middle at the empty last row
    colA = np.array(cols, np.int64)
    rowA = np.arange(colA.size, dtype=np.int64) // 2
    return ExpandCase(rowA, colA, rowptrB, colB, int(rowA[-1]) + 1, k, n)


def small_int_values(count: int, dtype, seed: int) -> np.ndarray:
    """Integers of [-4, 4] in `dtype`: every product and every sum of them is exact in any of the value types."""
    return np.random.default_rng(seed).integers(-4, 5, count).astype(dtype)


def small_nonzero_values(count: int, dtype, seed: int) -> np.ndarray:
    """Integers of [-4, 4] without 0 (no product is a signed zero, so "the sum of one term" has one spelling)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 5, count) * rng.choice([-1, 1], count)).astype(dtype)


def random_coo(m: int, n: int, nnz: int, seed: int) -> np.ndarray:
    """int64[2, <= nnz]: distinct (row, col) of an m x n matrix in row-major order."""
    key = np.unique(np.random.default_rng(seed).integers(0, m * n, nnz))
    return np.stack([key // n, key % n]).astype(np.int64)
