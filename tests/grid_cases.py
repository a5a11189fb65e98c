"""Graphs that drive every capped-grid kernel past its grid, and the arithmetic that proves they do.

Many kernels here run a fixed or capped number of workgroups over a device-side work list with a
grid-stride loop (`for (c = wave; c < total; c += num_waves)`), so the loop body runs a second time
only when the list is longer than the grid.  `GRIDS` restates those grids from the sources
(tests/test_grid_cases.py parses the constants back out of the .hip / .h text and fails when the two
disagree); the builders make lists one and a half times as long, so that the second trip is partial:
some waves take two items, some one.  `listed` and `saint_blocks` recompute from a graph alone what
the device will list, with the rules of csrc/long_rows.h (deg > 128, ceil(deg / 128) chunks) and of
csrc/walk.hip (block_range, stage_tile), so that every test can assert the property its case exists
for on the very data it runs.  Numpy only: no torch, no GPU."""
import numpy as np

LONG_ROW = 128    # csrc/long_rows.h kLongRow: rows with more entries are listed
LONG_CHUNK = 128  # csrc/long_rows.h kLongChunk: entries per chunk wave

# launch family -> the constants its grid is made of (source file under paddle_sparse_amd/csrc, name, value) and
# the number of items one sweep of the grid takes: waves for the chunk / combine / write loops, pairs or
# elements for the two flat loops, workgroups for saint (whose range is split over the blocks instead)
GRIDS = {
    "spmm_long": {"constants": [("long_rows.h", "kLongBlocks", 512), ("long_rows.h", "kLongThreads", 1024)],
                  "sweep": 512 * 1024 // 64},
    "spmm_fused": {"constants": [("spmm.hip", "kFusedChunkBlocksDefault", 768), ("spmm.hip", "kThreads", 256)],
                   "sweep": 768 * 4},
    "spmm_masked": {"constants": [("spmm.hip", "kMaskedChunkBlocks", 384), ("spmm.hip", "kThreads", 256)],
                    "sweep": 384 * 4},
    "spmm_half_bw": {"constants": [("spmm_half_bw.hip", "kHalfChunkBlocks", 768),
                                   ("spmm_half_bw.hip", "kThreads", 256)],
                     "sweep": 768 * 4},
    "heads": {"constants": [("spmm_heads.hip", "kMaxChunkBlocks", 4096), ("spmm_heads.hip", "kThreads", 256)],
              "sweep": 4096 * 4},
    "heads_half": {"constants": [("spmm_heads_half.hip", "kMaxChunkBlocks", 4096),
                                 ("spmm_heads_half.hip", "kThreads", 256)],
                   "sweep": 4096 * 4},
    "softmax": {"constants": [("softmax.hip", "kMaxChunkBlocks", 4096), ("softmax.hip", "kThreads", 256)],
                "sweep": 4096 * 4},
    "attention": {"constants": [("attention_kernels.h", "kMaxChunkBlocks", 4096),
                                ("attention_kernels.h", "kThreads", 256)],
                  "sweep": 4096 * 4},
    "pair_intersect": {"constants": [("intersect.hip", "kMaxBlocks", 65536), ("intersect.hip", "kThreads", 256),
                                     ("intersect.hip", "kGroup", 8)],
                       "sweep": 65536 * 4 * 8},
    # (this cap is a literal in the launch, not a named constant: the guard looks for the expression)
    "dropout_mask": {"constants": [("attention.hip", "literal:blocks > 65536 ? 65536 : blocks", 65536),
                                   ("attention_kernels.h", "kThreads", 256)],
                     "sweep": 65536 * 256},
    "saint": {"constants": [("walk.hip", "kBlocks", 2048), ("walk.hip", "kThreads", 256), ("walk.hip", "kPer", 4),
                            ("walk.hip", "kRows", 512)],
              "sweep": 2048},
    "long_rule": {"constants": [("long_rows.h", "kLongRow", LONG_ROW), ("long_rows.h", "kLongChunk", LONG_CHUNK)],
                  "sweep": None},
}

SAINT_BLOCKS = 2048      # csrc/walk.hip kBlocks
SAINT_TILE = 256 * 4     # csrc/walk.hip kTile = kThreads * kPer
SAINT_ROWS = 512         # csrc/walk.hip kRows


def second_trip(waves):
    """Items of a list one and a half grids long (+1): every wave takes one, half of them take two."""
    return waves + waves // 2 + 1


def listed(rowptr):
    """(long rows, chunks) the device lists for these row pointers: deg > 128, ceil(deg / 128) each."""
    deg = np.diff(np.asarray(rowptr, np.int64))
    long = deg[deg > LONG_ROW]
    return int(long.size), int(((long + LONG_CHUNK - 1) // LONG_CHUNK).sum())


def launched_waves(nnz, family="heads"):
    """Waves of the chunk (and write) launch of the heads / softmax / attention families for `nnz` entries:
    min(ceil(max_long_chunks(nnz) / 4), kMaxChunkBlocks) workgroups of 4 waves (long_rows.h: max_long_rows,
    max_long_chunks).  The combine launch is sized the same way from max_long_rows."""
    max_rows = nnz // (LONG_ROW + 1) + 1
    max_chunks = nnz // LONG_CHUNK + max_rows + 1
    cap = GRIDS[family]["sweep"] // 4
    return 4 * min(-(-max_chunks // 4), cap), 4 * min(-(-max_rows // 4), cap)


# chunk counts 33, 9, 6, 3, 2; 1025 and 129 end in a chunk of ONE entry, the others in ragged ones
RAGGED_DEGREES = (4099, 1025, 700, 300, 129)
# the uniform regime of the attention tests needs power-of-two row lengths (4 and 2 full chunks).  No longer rows:
# dS of a row of 2^j entries is a multiple of 2^-2j, and the sums of 2^j of them that grad_q adds must stay within
# 24 bits — at 1024 entries they do not (tests/test_zz_second_trip_gpu.py asserts the bound on its data)
POW2_DEGREES = (512, 256)


def _interleave(long_deg, rng, pow2, short_per_long):
    """The long rows in the given order, each followed by `short_per_long` rows of 0 - 4 entries (0, 1, 2, 4 under
    pow2; about a third of them empty) — but the first row and the last row are long."""
    short = rng.choice(np.array([0, 0, 1, 2, 4] if pow2 else [0, 0, 1, 2, 3, 4]), (len(long_deg), short_per_long))
    deg = np.concatenate([np.asarray(long_deg, np.int64)[:, None], short], axis=1).reshape(-1)
    return deg[:deg.size - short_per_long]


def _csr(deg, N, rng):
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    return rowptr, rng.integers(0, N, int(rowptr[-1])).astype(np.int64)


def many_chunks(waves, seed, pow2=False, N=600):
    """(rowptr, col): long rows whose chunks add up to second_trip(waves) exactly, of at least three different
    degrees, none a multiple of 128 (every row ends in a ragged chunk, some in a chunk of one entry; under pow2:
    512 and 256, the lengths the uniform attention regime allows, whose even chunk counts may end one above an odd
    sum), interleaved with rows of 0 - 4 entries and empty rows, a long row first and a long row last; columns uniform
    in [0, N), duplicates allowed."""
    rng = np.random.default_rng(seed)
    palette = POW2_DEGREES if pow2 else RAGGED_DEGREES
    chunks = [-(-d // LONG_CHUNK) for d in palette]
    left, long_deg, i = second_trip(waves), [], 0
    while left > 2 * chunks[0]:  # the palette in turn ...
        long_deg.append(palette[i % len(palette)])
        left -= chunks[i % len(palette)]
        i += 1
    if left % 2 and not pow2:  # ... then one row of 3 chunks and rows of 2 chunks to the exact sum
        long_deg.append(palette[-2])
        left -= chunks[-2]
    long_deg += [palette[-1]] * -(-left // 2)  # (pow2 has even chunk counts only: an odd sum ends one above)
    long_deg = np.array(long_deg, np.int64)
    long_deg = long_deg[rng.permutation(long_deg.size)]
    return _csr(_interleave(long_deg, rng, pow2, 3), N, rng)


def many_long_rows(waves, seed, pow2=False, N=600):
    """(rowptr, col): second_trip(waves) rows of 129, 130 or 131 entries (256 under pow2) — just above kLongRow, two
    chunks each — shuffled among as many rows of 0 - 4 entries and empty rows: the combine loops take a second
    trip, and the list pre-pass reserves list space from many workgroups."""
    rng = np.random.default_rng(seed)
    n = second_trip(waves)
    long_deg = np.full(n, 256, np.int64) if pow2 else rng.integers(129, 132, n)
    deg = _interleave(long_deg, rng, pow2, 1)
    inner = deg[1:-1]
    deg[1:-1] = inner[rng.permutation(inner.size)]  # long rows in runs of random length; the ends stay long
    return _csr(deg, N, rng)


# ---- saint_subgraph --------------------------------------------------------------------------------

def saint_blocks(rowptr, node_idx):
    """What the two candidate passes of saint_subgraph (csrc/walk.hip) do with this selection, from the graph
    alone: dict(C, per_block [2048], tiles_per_block [2048], rows_per_tile [tiles]) with block_range's split of
    [0, C) and stage_tile's row span (the rows between the one holding the tile's first candidate and the one
    holding its last, empty rows in between included)."""
    rowptr, node_idx = np.asarray(rowptr, np.int64), np.asarray(node_idx, np.int64)
    in_ptr = np.concatenate([[0], np.cumsum(rowptr[node_idx + 1] - rowptr[node_idx])]).astype(np.int64)
    C, S = int(in_ptr[-1]), node_idx.size
    b = np.arange(SAINT_BLOCKS + 1, dtype=np.int64)
    edge = C // SAINT_BLOCKS * b + (C % SAINT_BLOCKS) * b // SAINT_BLOCKS
    lo, hi = edge[:-1], edge[1:]
    tiles = -(-(hi - lo) // SAINT_TILE)
    p0 = np.concatenate([l + SAINT_TILE * np.arange(t) for l, t in zip(lo, tiles)]) if C else np.zeros(0, np.int64)
    p1 = np.minimum(p0 + SAINT_TILE, np.repeat(hi, tiles))
    first = np.minimum(np.searchsorted(in_ptr, p0, side="right") - 1, S - 1)
    last = np.minimum(np.searchsorted(in_ptr, p1 - 1, side="right") - 1, S - 1)
    return {"C": C, "per_block": hi - lo, "tiles_per_block": tiles, "rows_per_tile": last - first + 1,
            "tile_block": np.repeat(np.arange(SAINT_BLOCKS), tiles)}


def saint_ref(rowptr, col, node_idx, N):
    """(rowptr', col', edge_index) of saint_subgraph: tests/test_walk_saint.py's ref_saint_subgraph without its Python
    loop over the entries (tests/test_grid_cases.py holds the two to each other on the small cases)."""
    rowptr, col, node_idx = (np.asarray(a, np.int64) for a in (rowptr, col, node_idx))
    S = node_idx.size
    assoc = np.full(N, -1, np.int64)
    assoc[node_idx] = np.arange(S)  # the last duplicate wins (numpy assigns in order)
    deg = rowptr[node_idx + 1] - rowptr[node_idx]
    in_ptr = np.concatenate([[0], np.cumsum(deg)])
    row = np.repeat(np.arange(S), deg)
    e = np.arange(int(in_ptr[-1])) - in_ptr[row] + rowptr[node_idx][row]
    c = assoc[col[e]]
    keep = c >= 0
    row, c, e = row[keep], c[keep], e[keep]
    order = np.lexsort((c, row))  # stable: ties keep candidate order
    return np.searchsorted(row[order], np.arange(S + 1), side="left").astype(np.int64), c[order], e[order]


def _sorted_rows(rowptr, col):
    """Columns sorted inside every row (the storage order of a SparseTensor)."""
    row = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    return col[np.lexsort((col, row))]


def saint_cases():
    """name -> (rowptr, col, node_idx, N) for saint_subgraph:
    a_*        more than 2048 * (2 * 1024 + 300) candidates, so every block walks two full tiles and a ragged
               third (q0 carried across tiles, every sub-tile, every wave's prefix); one hub row longer than three
               tiles.  a_all: every node selected, everything kept; a_subset: a strict subset holding nearly all
               entries, half of whose columns fall outside the selection (mixed keep / drop); a_unsorted: that
               subset shuffled (candidate order is no longer (row, col) order: the caller re-sorts).
    b_runs     runs of 600 and 1100 selected rows without entries between non-empty ones: the tiles around them
               span more than 512 rows (searched in global memory, not staged), with staged tiles right behind.
    c_small    C < 2048 and C % 2048 != 0: most blocks have an empty range."""
    rng = np.random.default_rng(2048)
    cases = {}
    # a: nodes 0 .. S-1 hold the entries (the hub is node 7), nodes S .. N-1 hold 0 - 2 each
    S, N = 3000, 6000
    want = SAINT_BLOCKS * (2 * SAINT_TILE + 300) + 7
    deg = rng.integers(0, 2 * want // S, S)
    deg[7] = 3 * SAINT_TILE + 500
    deg[S - 1] += max(0, want - int(deg.sum()))
    deg = np.concatenate([deg, rng.integers(0, 3, N - S)]).astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.integers(0, N, int(rowptr[-1])).astype(np.int64)  # half of them >= S: not in the subset
    col = _sorted_rows(rowptr, col)
    subset = np.arange(S, dtype=np.int64)
    cases["a_all"] = (rowptr, col, np.arange(N, dtype=np.int64), N)
    cases["a_subset"] = (rowptr, col, subset, N)
    cases["a_unsorted"] = (rowptr, col, rng.permutation(subset), N)
    # b: about 48 candidates per block; every node selected, in order
    runs = [rng.integers(1, 60, 900), np.zeros(600), rng.integers(1, 60, 700), np.zeros(1100), rng.integers(1, 60, 900)]
    deg = np.concatenate(runs).astype(np.int64)
    N = deg.size
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = _sorted_rows(rowptr, rng.integers(0, N, int(rowptr[-1])).astype(np.int64))
    cases["b_runs"] = (rowptr, col, np.arange(N, dtype=np.int64), N)
    # c: 1500-odd candidates
    deg = rng.integers(0, 7, 500).astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = _sorted_rows(rowptr, rng.integers(0, 500, int(rowptr[-1])).astype(np.int64))
    cases["c_small"] = (rowptr, col, np.sort(rng.choice(500, 400, replace=False)).astype(np.int64), 500)
    return cases
