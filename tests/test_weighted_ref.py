"""CPU suite for the edge-weighted samplers: the numpy restatement (tests/weighted_ref.py)
pinned to hand-checked answers, the host export of the pick against it (the tie and clamp
branches included, which no seed search reaches on the GPU), the statistics of the restated
draws, and the public surface / C-ABI entry points.  No kernel runs."""
import ctypes

import numpy as np
import pytest
import torch

import weighted_ref as wr
from paddle_sparse_amd import EdgeCDF  # noqa: F401  (the restatement is pinned to a feature that must exist)
from test_walk_saint import KAT_COL, KAT_ROWPTR, ref_random_walk

SYMBOLS = ("psa_row_cdf", "psa_weighted_pick_host", "psa_random_walk_weighted", "psa_sample_count_weighted",
           "psa_sample_select_weighted")

# The KAT graph of test_walk_saint.py with weights: row 1 starts with a zero weight, row 2
# has one inside, node 5 has no entries.
KAT_W = [1, 3, 0, 2, 1, 0, 1, 4, 4, 0.5]
KAT_CUM = [1, 4, 0, 2, 1, 1, 2, 4, 8, 0.5]
# seed 12345: u of (walk, step) = .3344 .3176 .8432 .4244 | .3017 .4257 .7593 .0850 | .8446 .2568 .0812 .2221
# | (node 5 never draws) | .3414 .3681 .3120 .1369 | .7079 .1237 .6904 .3529; e.g. walk 1 at node 2 (cum 1 1 2)
# with u = .7593: target 1.52, the first cum above it is entry 6 -> node 3.
KAT_WALK = dict(start=[0, 2, 4, 5, 3, 1], L=4, seed=12345,
                nodes=[[0, 2, 0, 2, 0], [2, 0, 2, 3, 2], [4, 3, 2, 0, 1], [5, 5, 5, 5, 5], [3, 2, 0, 2, 0],
                       [1, 2, 0, 2, 0]],
                e_id=[[1, 4, 1, 4], [4, 1, 6, 7], [9, 7, 4, 0], [-1, -1, -1, -1], [7, 4, 1, 4], [3, 4, 1, 4]])
# subset [2, 0, 5, 1], k = 3: row 0 (node 2) picks entries 4 4 6 (columns 0 0 3), row 1 (node 0) entry 1
# three times, node 5 nothing, node 1 entry 3 three times (never its zero-weight entry 2); column 3 is new.
KAT_SELECT = dict(idx=[2, 0, 5, 1], k=3, seed=12345, n_id=[2, 0, 5, 1, 3], rowptr=[0, 3, 6, 6, 9],
                  col=[1, 1, 4, 0, 0, 0, 0, 0, 0], e_id=[4, 4, 6, 1, 1, 1, 3, 3, 3])


def host_pick(cum_row, r):
    from paddle_sparse_amd import ops

    return ops.weighted_pick_host(cum_row, r)


# ---- the restatement -----------------------------------------------------------------
def test_row_cdf_restatement_kat():
    assert wr.row_cdf(KAT_ROWPTR, KAT_W).tolist() == KAT_CUM


def test_weighted_walk_restatement_kat():
    k = KAT_WALK
    nodes, e_id = wr.ref_weighted_walk(KAT_ROWPTR, KAT_COL, np.array(KAT_CUM, np.float64), k["start"], k["L"], k["seed"])
    assert nodes.tolist() == k["nodes"] and e_id.tolist() == k["e_id"]


def test_vectorised_picks_match_the_scalar_pick():
    k = KAT_WALK
    cum = np.array(KAT_CUM, np.float64)
    for n, cur in enumerate(k["start"]):
        for l in range(k["L"]):
            s, deg = KAT_ROWPTR[cur], KAT_ROWPTR[cur + 1] - KAT_ROWPTR[cur]
            p = wr.pick(cum[s:s + deg], wr.word(k["seed"], n, l))
            assert (s + p if p >= 0 else -1) == k["e_id"][n][l]
            cur = KAT_COL[s + p] if p >= 0 else cur


def test_uniform_restatement_is_random_walks():
    nodes, e_id = wr.ref_weighted_walk(KAT_ROWPTR, KAT_COL, None, [0, 2, 4, 5, 3], 5, 12345)
    assert np.array_equal(nodes, ref_random_walk(KAT_ROWPTR, KAT_COL, [0, 2, 4, 5, 3], 5, 12345))
    moved = e_id >= 0
    assert np.array_equal(np.array(KAT_COL)[e_id[moved]], nodes[:, 1:][moved]) and not moved[3].any()


def test_weighted_select_restatement_kat():
    k = KAT_SELECT
    n_id, rowptr, col, e_id = wr.ref_weighted_select(KAT_ROWPTR, KAT_COL, np.array(KAT_CUM, np.float64), k["idx"],
                                                     k["k"], k["seed"])
    assert n_id.tolist() == k["n_id"] and rowptr.tolist() == k["rowptr"]
    assert col.tolist() == k["col"] and e_id.tolist() == k["e_id"]


# ---- the host export of the pick ---------------------------------------------------------
def test_host_pick_equals_the_restatement_on_random_rows():
    rng = np.random.default_rng(2024)
    n = 0
    for _ in range(100):
        deg = int(rng.integers(1, 200))
        w = rng.random(deg) * (rng.random(deg) >= 0.3)
        if rng.random() < 0.1:
            w[:] = 0
        cum = np.cumsum(w)
        for r in rng.integers(0, 1 << 64, 100, dtype=np.uint64).tolist():
            want = wr.pick(cum, r)
            assert host_pick(cum, r) == want
            assert want == -1 or w[want] > 0
            n += 1
    assert n == 10_000


R_MAX = (1 << 64) - 1
CRAFTED = [
    ([1.0, 2.0, 2.0, 4.0], 0, 0),
    ([1.0, 2.0, 2.0, 4.0], R_MAX, 3),
    ([1.0, 2.0, 2.0, 4.0], 1 << 63, 3),            # target == cum[1] == cum[2]: the next positive weight
    ([1.0, 2.0, 2.0, 4.0], 1 << 62, 1),            # target == cum[0]: entry 1
    ([0.0, 0.0, 3.0, 5.0], 0, 2),                  # leading zeros are never taken, not even at u = 0
    ([3.0, 5.0, 5.0, 5.0], R_MAX, 1),              # trailing zeros
    ([2.0, 2.0, 2.0, 8.0], 1 << 62, 3),            # interior zeros: target == 2 exactly
    ([2.0, 2.0, 2.0, 8.0], (1 << 62) - (1 << 11), 0),  # one ulp of u below it
    ([7.0], 0, 0), ([7.0], R_MAX, 0), ([7.0], 1 << 63, 0),   # deg = 1
    ([0.0, 0.0, 0.0], 12345, -1), ([0.0], 0, -1),  # all-zero rows
    ([0.0, 5e-324, 5e-324], R_MAX, 1),             # the product rounds up to the total: the clamp branch
    ([5e-324], R_MAX, 0),
]


@pytest.mark.parametrize("cum,r,want", CRAFTED)
def test_host_pick_on_crafted_rows(cum, r, want):
    assert wr.pick(cum, r) == want
    assert host_pick(cum, r) == want


def test_crafted_targets_are_what_the_comments_say():
    u = np.float64((1 << 63) >> 11) * 2.0 ** -53
    assert u == 0.5 and u * 4.0 == 2.0
    u = np.float64(R_MAX >> 11) * 2.0 ** -53
    assert u < 1.0 and u * 5e-324 == 5e-324 and u * 4.0 < 4.0
    u = np.float64((1 << 62) >> 11) * 2.0 ** -53
    assert u == 0.25 and u * 8.0 == 2.0
    assert np.float64(((1 << 62) - (1 << 11)) >> 11) * 2.0 ** -53 * 8.0 < 2.0


def test_host_pick_of_no_row_is_no_pick():
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    assert lib.psa_weighted_pick_host(None, 3, 1) == -1
    assert host_pick([], 5) == -1


# ---- the draws, restated ------------------------------------------------------------------
S_STAR = 370_000


def star_counts(weights, seed=31337):
    rowptr, col, w = wr.star(weights)
    nodes, e_id = wr.ref_weighted_walk(rowptr, col, wr.row_cdf(rowptr, w), np.zeros(S_STAR, np.int64), 1, seed)
    assert np.array_equal(e_id[:, 0] + 1, nodes[:, 1])
    return np.bincount(nodes[:, 1], minlength=len(weights) + 1)[1:]


def test_restated_draws_follow_the_weights_on_a_star():
    w = np.arange(1, 38, dtype=np.float64)
    sigma, chi2 = wr.star_bounds(star_counts(w), w, S_STAR)
    assert sigma < 5 and chi2 < 80  # 2.19 sigma, chi^2 35.3 at 36 degrees of freedom


def test_restated_draws_never_take_a_zero_weight():
    w = [0, 1, 0, 2, 4, 0, 8, .5, .25, 0]
    counts = star_counts(w)
    assert counts[np.array(w) == 0].tolist() == [0, 0, 0, 0] and counts.sum() == S_STAR
    assert wr.star_bounds(counts, w, S_STAR)[0] < 5  # 1.89 sigma


# ---- the surface ----------------------------------------------------------------------------
def test_new_names_are_exported_attached_and_bound():
    import inspect

    from test_abi import declared_functions

    import paddle_sparse_amd as psa
    from paddle_sparse_amd import SparseTensor, _lib, ops, weighted

    assert "EdgeCDF" in psa.__all__ and psa.EdgeCDF is weighted.EdgeCDF
    for fn in (psa.random_walk, SparseTensor.random_walk):
        params = inspect.signature(fn).parameters
        assert params["weighted"].default is False and params["return_edge_ids"].default is False
    assert inspect.signature(psa.sample_adj).parameters["weighted"].default is False
    assert inspect.signature(ops.sample_adj).parameters["cum"].default is None
    for name in ("row_cdf", "random_walk_weighted", "weighted_pick_host"):
        assert callable(getattr(ops, name))
    declared = declared_functions()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert not [name for name in declared if "weighted" in name and "workspace" in name]  # they need none


def _cpu_csr(M=3, N=3, value=None):
    from paddle_sparse_amd import SparseTensor

    rowptr = torch.tensor([0, 2, 3, 3])
    col = torch.tensor([0, 2, 1])
    return SparseTensor(rowptr=rowptr, col=col, value=torch.ones(3) if value is None else value, sparse_sizes=(M, N),
                        is_sorted=True, trust_data=True)


def test_cpu_tensors_are_refused():
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import ops

    a = _cpu_csr()
    with pytest.raises(RuntimeError, match="GPU tensor"):
        psa.EdgeCDF(a)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        psa.random_walk(a, torch.tensor([0, 1]), 3, seed=1, weighted=True)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        psa.random_walk(a, torch.tensor([0, 1]), 3, seed=1, return_edge_ids=True)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        a.sample_adj(torch.tensor([0, 1]), 2, replace=True, seed=1, weighted=True)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.row_cdf(torch.tensor([0, 1]), torch.ones(1, dtype=torch.float64))


def test_bad_arguments_raise_before_any_launch():
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import SparseTensor

    a = _cpu_csr()
    rowptr, col = torch.tensor([0, 2, 3, 3]), torch.tensor([0, 2, 1])
    no_value = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(3, 3), is_sorted=True, trust_data=True)
    with pytest.raises(ValueError, match="values"):
        psa.EdgeCDF(no_value)
    with pytest.raises(ValueError, match="values"):
        psa.random_walk(no_value, torch.tensor([0]), 2, seed=1, weighted=True)
    with pytest.raises(ValueError, match="1-D"):
        psa.EdgeCDF(_cpu_csr(value=torch.ones(3, 2)))
    with pytest.raises(ValueError, match="floating, int32 or int64"):
        psa.EdgeCDF(_cpu_csr(value=torch.ones(3, dtype=torch.uint8)))
    with pytest.raises(TypeError):
        psa.EdgeCDF(rowptr)
    with pytest.raises(TypeError, match="EdgeCDF"):
        psa.random_walk(a, torch.tensor([0]), 2, seed=1, weighted="yes")
    with pytest.raises(TypeError, match="EdgeCDF"):
        a.sample_adj(torch.tensor([0]), 2, replace=True, seed=1, weighted=3.5)
    with pytest.raises(ValueError, match="square"):
        psa.random_walk(_cpu_csr(3, 4), torch.tensor([0]), 2, seed=1, weighted=True)
    with pytest.raises(TypeError):
        psa.random_walk(a, torch.tensor([0.0]), 2, seed=1, weighted=True)
    with pytest.raises(ValueError):
        psa.random_walk(a, torch.tensor([0]), -1, seed=1, return_edge_ids=True)
    # weighted picks without replacement: refused before anything looks at the tensors
    with pytest.raises(NotImplementedError, match="without replacement"):
        a.sample_adj(torch.tensor([0, 1]), 1, replace=False, seed=1, weighted=True)
    with pytest.raises(NotImplementedError, match="without replacement"):
        psa.sample_adj(a, torch.tensor([0, 1]), 0, seed=1, weighted=True)
