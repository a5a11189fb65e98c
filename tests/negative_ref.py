"""Edge lookup and negative sampling restated serially in Python integers (csrc/edge_lookup.h,
csrc/negative.hip), built on weighted_ref's mix64, with the graphs and the case tables that the
CPU suite (host exports) and the GPU suite (kernels) both run.  Both compare bit for bit with
ref_edge_lookup and ref_negative_sample; tests/test_zz_negative_ref.py pins them to hand-checked
answers.  Not a test module."""
import bisect
import functools

import numpy as np

import weighted_ref as wr

M64 = wr.M64
RANGE, FAILED = 1, 2  # bits of flags


def mulhi(r, n):
    return (r * n) >> 64


def rand_stream(seed, i):
    return wr.mix64((seed & M64) ^ wr.mix64(i & M64))


def edge_find(col, lo, hi, x):
    """Position of the first entry of the non-decreasing list col[lo:hi] equal to x, or -1."""
    p = bisect.bisect_left(col, x, lo, hi)
    return p if p < hi and col[p] == x else -1


def _lists(rowptr, col):
    """Python lists of the two arrays (the fastest to bisect), or the int64 arrays themselves when they are too
    long to turn into lists (the bench tool's graphs): bisect reads either."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    return (rowptr, col) if col.size > 1 << 22 else (rowptr.tolist(), col.tolist())


def ref_edge_lookup(rowptr, col, M, N, row_q, col_q):
    """(pos int64[Q], flags)."""
    rowptr, col = _lists(rowptr, col)
    pos, flags = [], 0
    for r, c in zip(np.asarray(row_q, np.int64).tolist(), np.asarray(col_q, np.int64).tolist()):
        if not (0 <= r < M and 0 <= c < N):
            flags |= RANGE
            pos.append(-1)
        else:
            pos.append(edge_find(col, rowptr[r], rowptr[r + 1], c))
    return np.array(pos, np.int64).reshape(-1), flags


def ref_negative_sample(rowptr, col, M, N, src, count, no_self_loops, max_tries, seed, stats=None):
    """src None: `count` samples with the row drawn, (row, col, flags).  src given: `count`
    samples for each of its rows, (None, col int64[len(src) * count], flags).  stats, a dict,
    gets the number of tries made ("tries") added."""
    rowptr, col = _lists(rowptr, col)
    given = src is not None
    src = np.asarray(src, np.int64).tolist() if given else None
    n, k = (len(src) * count, count) if given else (count, 1)
    rows, cols, flags, tries = [-1] * n, [-1] * n, 0, 0
    for i in range(n):
        r = src[i // k] if given else -1
        if given and not 0 <= r < M:
            flags |= RANGE
            continue
        done = False
        if M > 0 and N > 0:
            stream = rand_stream(seed, i)
            for j in range(max_tries):
                tries += 1
                c = (stream + j) & M64
                cc = mulhi(wr.mix64(c), N)
                if not given:
                    r = mulhi(wr.mix64((c + (1 << 63)) & M64), M)
                if no_self_loops and r == cc:
                    continue
                if edge_find(col, rowptr[r], rowptr[r + 1], cc) < 0:
                    rows[i], cols[i], done = r, cc, True
                    break
        if not done:
            flags |= FAILED
    if stats is not None:
        stats["tries"] = stats.get("tries", 0) + tries
    return (None if given else np.array(rows, np.int64).reshape(-1)), np.array(cols, np.int64).reshape(-1), flags


def sorted_csr(row, col, M):
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    order = np.lexsort((col, row))
    return np.searchsorted(row[order], np.arange(M + 1), side="left").astype(np.int64), col[order]


def coo_rows(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


# ---- small matrices with answers that need no random number ---------------------------------------
def tiny():
    """(rowptr, col, M, N): 5 x 8, row 0 = [1, 3, 3, 3, 6] (a triple), row 1 = [0, 7] (the first and
    the last column), row 2 empty, row 3 = [2, 2], the last row 4 = [4]."""
    return sorted_csr([0, 0, 0, 0, 0, 1, 1, 3, 3, 4], [1, 3, 3, 3, 6, 0, 7, 2, 2, 4], 5) + (5, 8)


def one_free(free=5, N=8):
    """(rowptr, col, N, N): row r of an N x N matrix stores every column but `free`, with the next
    column twice; row N - 1 stores every column (a full row)."""
    rows, cols = [], []
    for r in range(N):
        c = [x for x in range(N) if x != free or r == N - 1] + [(free + 1) % N]
        rows += [r] * len(c)
        cols += c
    return sorted_csr(rows, cols, N) + (N, N)


# ---- the case tables ------------------------------------------------------------------------------
DEGS = (0, 1, 2, 3, 63, 64, 65)
BIG_ROW, BIG_DEG = 2047, 1000  # the last row of "degs"
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
HUGE_N = 1 << 40
GRAPHS = ("degs", "rect", "huge", "empty")


@functools.lru_cache(maxsize=None)
def case_graph(name):
    """(rowptr, col, M, N), read-only.
    degs:  2048 x 2048, rows of DEGS entries in turn, columns drawn with repeats (duplicated entries), the
           diagonal stored on every fifth row; the last row has 1000 distinct columns.
    rect:  40 x 70 at density 0.3, no duplicates.
    huge:  6 x 2^40, a dozen entries with column ids either side of 2^32, one of them twice; row 2 empty.
    empty: 50 x 50 without entries."""
    rng = np.random.default_rng(20)
    if name == "degs":
        M = N = BIG_ROW + 1
        rows, cols = [], []
        for i in range(BIG_ROW):
            c = rng.integers(0, N, DEGS[i % len(DEGS)])
            if len(c) > 2:
                c[1] = c[0]  # a duplicate in every row of three entries or more
            if i % 5 == 0 and len(c):
                c[-1] = i
            rows.append(np.full(len(c), i))
            cols.append(c)
        rows.append(np.full(BIG_DEG, BIG_ROW))
        cols.append(rng.choice(N, BIG_DEG, replace=False))
        row, col = np.concatenate(rows), np.concatenate(cols)
    elif name == "rect":
        M, N = 40, 70
        row, col = np.nonzero(rng.random((M, N)) < 0.3)
    elif name == "huge":
        M, N = 6, HUGE_N
        B = 1 << 32
        row = [0, 0, 0, 1, 1, 1, 3, 3, 4, 5, 5, 5]
        col = [3, B + 3, HUGE_N - 1, B - 1, B, B + 1, 5 * B + 7, 5 * B + 7, 0, 7, (1 << 39) + 7, (1 << 33)]
    else:
        M = N = 50
        row, col = [], []
    rowptr, col = sorted_csr(row, col, M)
    for a in (rowptr, col):
        a.setflags(write=False)
    return rowptr, col, M, N


def stored_pairs(name):
    rowptr, col, _, _ = case_graph(name)
    return set(zip(coo_rows(rowptr).tolist(), col.tolist()))


def case_queries(name, Q):
    """(row, col) int64[Q], all inside the matrix: about half stored entries (duplicates, first and last
    entries of rows among them), the rest their neighbours in the column direction, the same column
    modulo 2^32 or plus 2^32 (what a 32-bit index would confuse) and random pairs."""
    rowptr, col, M, N = case_graph(name)
    rng = np.random.default_rng(1000 + Q)
    r, c = rng.integers(0, M, Q), rng.integers(0, N, Q)
    nnz = len(col)
    if nnz and Q:
        e = rng.integers(0, nnz, Q)
        e[:2] = (0, nnz - 1)[:Q]
        kind = rng.integers(0, 8, Q)
        kind[:2] = 0
        er, ec = coo_rows(rowptr)[e], col[e]
        alt = np.select([kind < 4, kind == 4, kind == 5, kind == 6],
                        [ec, ec - 1, ec + 1, np.where(ec >= 1 << 32, ec % (1 << 32), ec + (1 << 32))], c)
        use = kind < 7
        r, c = np.where(use, er, r), np.where(use, np.clip(alt, 0, N - 1), c)
    return r.astype(np.int64), c.astype(np.int64)


LOOKUP_CASES = tuple((g, Q) for g in GRAPHS for Q in COUNTS if g != "empty" or Q in (0, 65))


def _sample_cases():
    """(graph, given rows?, S, k, no_self_loops): in global mode S is the number of samples.  Every count
    with k = 1 in both modes, k = 3 with S * k of 0, 63, 255, 258 and 1002; on the square graph each with
    no_self_loops off and on."""
    out = []
    for g in GRAPHS:
        for loops in ((False, True) if g in ("degs", "empty") else (False,)):
            counts = COUNTS if g != "empty" else (0, 65)
            out += [(g, given, S, 1, loops) for S in counts for given in (False, True)]
            out += [(g, True, S, 3, loops) for S in ((0, 21, 85, 86, 334) if g != "empty" else (21,))]
    return tuple(out)


SAMPLE_CASES = _sample_cases()
CASE_SEED = 2**63 + 29  # a seed with the top bit set
CASE_MAX_TRIES = 64


def case_src(name, S):
    _, _, M, _ = case_graph(name)
    src = np.random.default_rng(7 * S + 1).integers(0, M, S)
    if S:
        src[0] = M - 1  # the last row; the 1000-entry row of "degs"
    return src.astype(np.int64)


@functools.lru_cache(maxsize=None)
def lookup_ref(k):
    name, Q = LOOKUP_CASES[k]
    rowptr, col, M, N = case_graph(name)
    pos, flags = ref_edge_lookup(rowptr, col, M, N, *case_queries(name, Q))
    pos.setflags(write=False)
    return pos, flags


@functools.lru_cache(maxsize=None)
def sample_ref(k):
    """(row or None, col, flags) of SAMPLE_CASES[k], computed once per process."""
    name, given, S, kk, loops = SAMPLE_CASES[k]
    rowptr, col, M, N = case_graph(name)
    row, cols, flags = ref_negative_sample(rowptr, col, M, N, case_src(name, S) if given else None,
                                           kk if given else S, loops, CASE_MAX_TRIES, CASE_SEED + k)
    for a in (row, cols):
        if a is not None:
            a.setflags(write=False)
    return row, cols, flags


# ---- uniformity -----------------------------------------------------------------------------------
UNIFORM_S = 100_000
ROW16 = (0, 2, 3, 7, 11, 15)  # the stored columns of the one row, N = 16
ROW16_SEED, SQUARE12_SEED = 5, 9


def row16():
    return sorted_csr([0] * len(ROW16), ROW16, 1) + (1, 16)


@functools.lru_cache(maxsize=None)
def square12():
    """12 x 12 with exactly half of the 144 pairs stored."""
    stored = np.sort(np.random.default_rng(3).choice(144, 72, replace=False))
    rowptr, col = sorted_csr(stored // 12, stored % 12, 12)
    return rowptr, col, 12, 12


def sigmas(counts, n):
    """Largest |count - n / len(counts)| / sigma of a uniform draw of n over len(counts) cells."""
    p = 1.0 / len(counts)
    return float((np.abs(np.asarray(counts) - n * p) / np.sqrt(n * p * (1 - p))).max())


def row16_sigmas(cols):
    free = [c for c in range(16) if c not in ROW16]
    assert np.isin(cols, free).all()
    return sigmas([(cols == c).sum() for c in free], len(cols))


def square12_sigmas(rows, cols):
    rowptr, col, _, _ = square12()
    stored = set((coo_rows(rowptr) * 12 + col).tolist())
    free = [x for x in range(144) if x not in stored]
    keys = rows * 12 + cols
    assert np.isin(keys, free).all()
    return sigmas(np.bincount(keys, minlength=144)[free], len(keys))
