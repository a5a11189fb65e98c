"""CPU suite of tests/grid_cases.py: the table of grids agrees with the sources, and every builder has,
computed from the graph alone, the property its case exists for.  No kernel runs.

The guard sends whoever changes a cap (kLongBlocks, kFusedChunkBlocksDefault, kMaxChunkBlocks, walk.hip's
kBlocks, ...) here: the second-trip GPU tests size their graphs from GRIDS, and must not quietly lose
their coverage when a grid grows."""
import re
from pathlib import Path

import numpy as np
import pytest

import grid_cases as gc

CSRC = Path(__file__).resolve().parents[1] / "paddle_sparse_amd" / "csrc"


def constant_in(text, name):
    """The value of `constexpr int NAME = value;` (or int64_t) in a source text; products of literals and of
    `kThreads`-style names already defined in the same text are not followed: the table names plain constants."""
    m = re.search(r"constexpr\s+(?:int|int64_t|unsigned)\s+" + re.escape(name) + r"\s*=\s*(\d+)\s*;", text)
    return None if m is None else int(m.group(1))


@pytest.mark.parametrize("family", sorted(gc.GRIDS))
def test_the_table_agrees_with_the_sources(family):
    for file, name, value in gc.GRIDS[family]["constants"]:
        text = (CSRC / file).read_text()
        if name.startswith("literal:"):
            assert name[len("literal:"):] in text, f"{file}: the launch no longer reads `{name[8:]}`"
            assert str(value) in name
        else:
            assert constant_in(text, name) == value, f"{file}: {name} is {constant_in(text, name)}, the table says {value}"


def test_the_guard_sees_an_edited_cap():
    """The parser on edited copies of the texts: a changed kLongBlocks, kFusedChunkBlocksDefault, kMaxChunkBlocks or
    kBlocks no longer equals the table."""
    for file, name in (("long_rows.h", "kLongBlocks"), ("spmm.hip", "kFusedChunkBlocksDefault"),
                       ("softmax.hip", "kMaxChunkBlocks"), ("attention_kernels.h", "kMaxChunkBlocks"),
                       ("walk.hip", "kBlocks")):
        text = (CSRC / file).read_text()
        old = constant_in(text, name)
        assert old is not None
        edited = re.sub(r"(constexpr\s+int\s+" + name + r"\s*=\s*)\d+", lambda m: m.group(1) + str(2 * old), text)
        assert constant_in(edited, name) == 2 * old != old


def test_sweeps_follow_from_the_constants():
    g = {f: {n: v for _, n, v in e["constants"]} for f, e in gc.GRIDS.items()}
    assert gc.GRIDS["spmm_long"]["sweep"] == g["spmm_long"]["kLongBlocks"] * g["spmm_long"]["kLongThreads"] // 64 == 8192
    assert gc.GRIDS["spmm_fused"]["sweep"] == g["spmm_fused"]["kFusedChunkBlocksDefault"] * g["spmm_fused"]["kThreads"] // 64
    assert gc.GRIDS["spmm_half_bw"]["sweep"] == g["spmm_half_bw"]["kHalfChunkBlocks"] * g["spmm_half_bw"]["kThreads"] // 64
    assert gc.GRIDS["spmm_masked"]["sweep"] == g["spmm_masked"]["kMaskedChunkBlocks"] * g["spmm_masked"]["kThreads"] // 64
    for f in ("heads", "heads_half", "softmax", "attention"):
        assert gc.GRIDS[f]["sweep"] == g[f]["kMaxChunkBlocks"] * g[f]["kThreads"] // 64 == 16384
    p = g["pair_intersect"]
    assert gc.GRIDS["pair_intersect"]["sweep"] == p["kMaxBlocks"] * (p["kThreads"] // 64) * (64 // p["kGroup"]) == 2097152
    assert gc.GRIDS["dropout_mask"]["sweep"] == 65536 * g["dropout_mask"]["kThreads"] == 16777216
    s = g["saint"]
    assert (s["kBlocks"], s["kThreads"] * s["kPer"], s["kRows"]) == (gc.SAINT_BLOCKS, gc.SAINT_TILE, gc.SAINT_ROWS)
    assert (g["long_rule"]["kLongRow"], g["long_rule"]["kLongChunk"]) == (gc.LONG_ROW, gc.LONG_CHUNK)


WAVES = sorted({gc.GRIDS[f]["sweep"] for f in ("spmm_long", "spmm_fused", "spmm_masked", "spmm_half_bw", "heads")})


@pytest.mark.parametrize("pow2", [False, True])
@pytest.mark.parametrize("waves", WAVES)
def test_many_chunks(waves, pow2):
    rowptr, col = gc.many_chunks(waves, seed=waves, pow2=pow2)
    deg = np.diff(rowptr)
    rows, chunks = gc.listed(rowptr)
    want = gc.second_trip(waves)
    assert chunks > waves and chunks < 2 * waves  # a second trip, and a partial one
    assert chunks == want or (pow2 and want % 2 == 1 and chunks == want + 1)
    long = deg[deg > gc.LONG_ROW]
    assert np.unique(long).size >= (2 if pow2 else 3)
    assert deg[0] > gc.LONG_ROW and deg[-1] > gc.LONG_ROW
    short = deg[deg <= gc.LONG_ROW]
    assert short.max() <= 4 and (short == 0).any() and set(np.unique(short)) >= {0, 1, 2, 4}
    if pow2:
        assert np.all(deg[deg > 0] & (deg[deg > 0] - 1) == 0)
    else:
        assert np.all(long % gc.LONG_CHUNK != 0) and np.any(long % gc.LONG_CHUNK == 1)
    assert col.size == rowptr[-1] and col.min() >= 0 and col.max() < 600
    # the capped launches of the heads / softmax / attention families are in fact capped at this size
    if waves == gc.GRIDS["heads"]["sweep"]:
        assert gc.launched_waves(col.size) == (waves, waves)


@pytest.mark.parametrize("pow2", [False, True])
@pytest.mark.parametrize("waves", WAVES)
def test_many_long_rows(waves, pow2):
    rowptr, col = gc.many_long_rows(waves, seed=waves + 1, pow2=pow2)
    deg = np.diff(rowptr)
    rows, chunks = gc.listed(rowptr)
    assert rows == gc.second_trip(waves) > waves and chunks == 2 * rows
    long = deg[deg > gc.LONG_ROW]
    assert set(np.unique(long)) == ({256} if pow2 else {129, 130, 131})
    assert deg[0] > gc.LONG_ROW and deg[-1] > gc.LONG_ROW and (deg == 0).any()
    # long rows and short rows are mixed, not alternating: runs of long rows of several lengths
    is_long = deg > gc.LONG_ROW
    assert (is_long[1:] & is_long[:-1]).any() and (~is_long[1:] & ~is_long[:-1]).any()
    # the list pre-pass (1024 rows per workgroup) reserves from many workgroups
    assert deg.size > 16 * 1024 or waves < 8192
    if waves == gc.GRIDS["heads"]["sweep"]:
        assert gc.launched_waves(col.size) == (waves, waves)


@pytest.fixture(scope="module")
def saint():
    return gc.saint_cases()


def test_saint_blocks_restates_block_range():
    """Hand-checked: 5000 candidates over 2048 blocks — 2 or 3 each, contiguous, summing to C."""
    rowptr = np.array([0, 4000, 4000, 5000])
    b = gc.saint_blocks(rowptr, np.array([0, 1, 2]))
    assert b["C"] == 5000 and b["per_block"].sum() == 5000 and set(b["per_block"]) == {2, 3}
    assert b["tiles_per_block"].max() == 1 and b["rows_per_tile"].max() == 3  # the tile across the empty row
    assert b["per_block"][0] == 5000 // 2048 * 1 + (5000 % 2048) * 1 // 2048


@pytest.mark.parametrize("name", ["a_all", "a_subset", "a_unsorted"])
def test_saint_a_every_block_walks_three_tiles(saint, name):
    rowptr, col, idx, N = saint[name]
    b = gc.saint_blocks(rowptr, idx)
    assert b["C"] >= 2048 * (2 * 1024 + 300) + 7
    assert b["tiles_per_block"].min() >= 3
    assert np.all(b["per_block"] % gc.SAINT_TILE != 0)  # the last tile of every block is ragged
    deg = rowptr[idx + 1] - rowptr[idx]
    assert deg.max() > 3 * gc.SAINT_TILE
    sel = np.zeros(N, bool)
    sel[idx] = True
    kept = sel[col[np.concatenate([np.arange(rowptr[v], rowptr[v + 1]) for v in idx[:50]])]].mean()
    if name == "a_all":
        assert idx.size == N and kept == 1.0
    else:
        assert idx.size < N and 0.4 < kept < 0.6  # mixed keep and drop decisions
        assert (np.diff(idx) < 0).any() == (name == "a_unsorted")


def test_saint_b_a_tile_spans_more_than_512_rows(saint):
    rowptr, col, idx, N = saint["b_runs"]
    deg = rowptr[idx + 1] - rowptr[idx]
    empty_runs = sorted(len(r) for r in "".join("e" if d == 0 else " " for d in deg).split())
    assert empty_runs == [600, 1100]
    b = gc.saint_blocks(rowptr, idx)
    wide = np.flatnonzero(b["rows_per_tile"] > gc.SAINT_ROWS)
    assert wide.size == 2 and b["rows_per_tile"].max() > 1100  # both runs sit inside a tile
    assert np.all(b["rows_per_tile"][wide + 1] <= gc.SAINT_ROWS)  # a staged tile directly behind each
    assert np.all(b["rows_per_tile"][wide + 1] >= 1) and np.all(b["per_block"][b["tile_block"][wide + 1]] > 0)


def test_saint_c_some_blocks_are_empty(saint):
    rowptr, col, idx, N = saint["c_small"]
    b = gc.saint_blocks(rowptr, idx)
    assert 0 < b["C"] < gc.SAINT_BLOCKS and b["C"] % gc.SAINT_BLOCKS != 0
    assert (b["per_block"] == 0).any() and (b["per_block"] == 1).any() and b["per_block"].max() == 1


def test_vectorised_saint_restatement_matches_the_scalar_one(saint):
    """gc.saint_ref against test_walk_saint.ref_saint_subgraph on the small cases, and on a selection with duplicates."""
    from test_walk_saint import ref_saint_subgraph

    for name in ("b_runs", "c_small"):
        rowptr, col, idx, N = saint[name]
        for a, b in zip(gc.saint_ref(rowptr, col, idx, N), ref_saint_subgraph(rowptr, col, idx, N)):
            assert np.array_equal(a, b), name
    rowptr, col, idx, N = saint["c_small"]
    dup = np.random.default_rng(3).choice(idx, 300)
    for a, b in zip(gc.saint_ref(rowptr, col, dup, N), ref_saint_subgraph(rowptr, col, dup, N)):
        assert np.array_equal(a, b)
    unsorted = np.random.default_rng(4).permutation(idx)
    for a, b in zip(gc.saint_ref(rowptr, col, unsorted, N), ref_saint_subgraph(rowptr, col, unsorted, N)):
        assert np.array_equal(a, b)
