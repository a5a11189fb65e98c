"""CPU suite for weighted neighbor_sample: the host export of the successive
weighted picks without replacement against the serial restatement of
tests/weighted_neighbor_ref.py bit for bit, hand-picked random words that reach the two
rounding fallbacks, the invariants of the contract, the law of the draws, and the errors
the public surface raises before anything is launched.  No kernel runs."""
import ctypes
import inspect
import itertools

import numpy as np
import pytest
import torch

import weighted_neighbor_ref as nr

R_MAX = (1 << 64) - 1
TINY = 5e-324  # the smallest subnormal


def host(cum, k, words_entry, words_gap):
    from paddle_sparse_amd import ops

    return ops.weighted_pick_without_host(cum, k, words_entry, words_gap)


def host_pick(cum, r):
    from paddle_sparse_amd import ops

    return ops.weighted_pick_host(cum, r)


def row_weights(kind, deg, rng):
    w = rng.random(deg)
    if kind == "uniform":
        return w
    if kind == "half_zeros":
        w[rng.random(deg) < 0.5] = 0.0
    elif kind == "one_huge":
        w = np.ones(deg)
        w[rng.integers(deg)] = 1e18
    elif kind == "subnormal":
        w = TINY * rng.integers(0, 4, deg)
    elif kind == "small_integers":
        w = rng.integers(0, 3, deg).astype(np.float64)
    elif kind == "heavy_ends":  # the heaviest entries first and last: taken early, they leave empty edge gaps
        w[0] = w[-1] = 1e6
    elif kind == "few_positive":  # P < k <= deg for most k
        w[:] = 0.0
        w[rng.choice(deg, size=min(deg, int(rng.integers(0, 4))), replace=False)] = rng.random() + 0.5
    else:
        raise KeyError(kind)
    return w


KINDS = ["uniform", "half_zeros", "one_huge", "subnormal", "small_integers", "heavy_ends", "few_positive"]


def check_invariants(cum, k, words_entry, picks):
    P = nr.positive_entries(list(cum))
    assert len(picks) == min(k, P), (picks, k, P)
    assert len(set(picks)) == len(picks)
    for e in picks:
        assert 0 <= e < len(cum) and cum[e] > (cum[e - 1] if e > 0 else 0.0)  # a positive weight
    if picks:
        assert picks[0] == host_pick(cum, words_entry[0])
    else:
        assert host_pick(cum, words_entry[0]) == -1


@pytest.mark.parametrize("kind", KINDS)
def test_host_export_equals_the_restatement(kind):
    """Rows of 1 to 40 entries, k = 1 .. 12, the words of a stream: bit for bit, and the
    invariants of the contract on every row."""
    rng = np.random.default_rng(KINDS.index(kind))
    seen_short = seen_full = 0
    for deg in range(1, 41):
        w = row_weights(kind, deg, rng)
        cum = np.cumsum(w).tolist()
        for k in range(1, 13):
            we, wg = nr.stream_words(1000 + deg, k, k)
            want = nr.picks_without_words(cum, k, we, wg)
            got = host(cum, k, we, wg)
            assert got == want, (kind, deg, k)
            check_invariants(cum, k, we, got)
            seen_short += len(got) < k
            seen_full += len(got) == k
    assert seen_full > 0 and seen_short > 0  # deg < k at the least


@pytest.mark.parametrize("k", [8, 9, 16, 17, 32, 33, 40])
def test_host_export_at_every_register_width(k):
    """The walk is compiled for up to 8, 16 and 32 draws in registers and for any number in
    memory: both sides of every boundary, rows shorter and longer than k."""
    rng = np.random.default_rng(k)
    for deg in (1, k - 1, k, k + 1, 2 * k, 90):
        for kind in ("uniform", "half_zeros", "one_huge", "small_integers"):
            cum = np.cumsum(row_weights(kind, deg, rng)).tolist()
            we, wg = nr.stream_words(77, deg, k)
            got = host(cum, k, we, wg)
            assert got == nr.picks_without_words(cum, k, we, wg), (k, deg, kind)
            check_invariants(cum, k, we, got)


def test_rows_without_a_positive_weight_and_rows_of_one_entry():
    for deg in (1, 2, 7):
        for k in (1, 3, 9):
            zeros = [0.0] * deg
            assert host(zeros, k, [R_MAX] * k, [0] * k) == [] == nr.picks_without_words(zeros, k, [R_MAX] * k, [0] * k)
    for k in (1, 2, 5):
        for r in (0, R_MAX, 1 << 63):
            assert host([7.0], k, [r] * k, [r] * k) == [0] == nr.picks_without_words([7.0], k, [r] * k, [r] * k)
    assert host([], 3, [1, 2, 3], [4, 5, 6]) == []
    assert host([1.0, 2.0], 0, [], []) == []


# (cum, k, words_entry, words_gap, picks)
CRAFTED = [
    # u = 0 in both stages: the first entry of positive weight of the first gap that has any
    ([1.0, 3.0, 6.0, 10.0], 4, [0] * 4, [0] * 4, [0, 1, 2, 3]),
    # the largest words: the last entry, then the last entry of the last gap with mass
    ([1.0, 3.0, 6.0, 10.0], 4, [R_MAX] * 4, [R_MAX] * 4, [3, 2, 1, 0]),
    # zeros at both ends and inside are never taken: P = 2 < k
    ([0.0, 2.0, 2.0, 5.0, 5.0], 4, [0] * 4, [R_MAX] * 4, [1, 3]),
    ([0.0, 2.0, 2.0, 5.0, 5.0], 4, [R_MAX] * 4, [0] * 4, [3, 1]),
    # a subnormal total: u * T rounds up to T.  Draw 0 takes the stage-2 fallback (the smallest
    # e with cum[e] == top); from draw 1 on stage 1 finds no S_g > target and falls back to
    # the last gap of positive mass, and stage 2 falls back again
    ([TINY, 2 * TINY, 3 * TINY, 4 * TINY], 4, [R_MAX] * 4, [R_MAX] * 4, [3, 2, 1, 0]),
    ([0.0, TINY, TINY], 3, [R_MAX] * 3, [R_MAX] * 3, [1]),
    # stage 1 alone falls back: masses TINY | taken | 0, the gap word at its largest, entry word 0
    ([TINY, 2 * TINY, 2 * TINY], 3, [R_MAX, 0, 0], [0, R_MAX, R_MAX], [1, 0]),
    # normal numbers: base + u * mass rounds up to top in the ADD (1e18 + 256 - 2^-45): draw 1 takes the
    # stage-2 fallback inside the gap behind the taken entry 0
    ([1e18, 1e18 + 128, 1e18 + 256], 2, [0, R_MAX], [0, 0], [0, 2]),
]


@pytest.mark.parametrize("cum,k,we,wg,want", CRAFTED)
def test_hand_picked_words(cum, k, we, wg, want):
    assert nr.picks_without_words(cum, k, we, wg) == want
    assert host(cum, k, we, wg) == want
    check_invariants(cum, k, we, want)


def test_crafted_roundings_are_what_the_comments_say():
    u = nr.unit(R_MAX)
    assert u < 1.0 and nr.unit(0) == 0.0
    for m in (1, 2, 3, 4):
        assert u * (m * TINY) == m * TINY  # rounds up to the total: no S_g, no cum[e] above it
    assert u * 10.0 < 10.0 and u * 256.0 < 256.0
    assert 1e18 + 128 == np.nextafter(1e18, np.inf) and 1e18 + u * 256.0 == 1e18 + 256  # the add rounds up to top


def test_the_law_of_two_draws():
    """w = [1, 2, 3, 4], k = 2, streams 0 .. 199 999 of one seed through the host export: the
    12 ordered pairs against w_a / 10 * w_b / (10 - w_a).  chi^2 below 45 (p about 1e-5 at 11
    degrees of freedom); the bits are fixed, so is the outcome."""
    w = [1.0, 2.0, 3.0, 4.0]
    cum = np.cumsum(w).tolist()
    T = 200_000
    counts = {}
    for i in range(T):
        pair = tuple(host(cum, 2, *nr.stream_words(4242, i, 2)))
        counts[pair] = counts.get(pair, 0) + 1
    pairs = list(itertools.permutations(range(4), 2))
    assert sorted(counts) == pairs
    chi2 = sum((counts[a, b] - T * w[a] / 10 * w[b] / (10 - w[a])) ** 2 / (T * w[a] / 10 * w[b] / (10 - w[a]))
               for a, b in pairs)
    print(f"chi^2 of the ordered pairs: {chi2:.2f}")
    assert chi2 < 45


def test_the_law_of_one_draw():
    """k = 1: single draws against w / 10; chi^2 below 26 (p about 1e-5 at 3 degrees of freedom)."""
    w = [1.0, 2.0, 3.0, 4.0]
    cum = np.cumsum(w).tolist()
    T = 200_000
    counts = np.zeros(4)
    for i in range(T):
        (e,) = host(cum, 1, *nr.stream_words(4242, i, 1))
        counts[e] += 1
    mean = T * np.array(w) / 10
    chi2 = float(((counts - mean) ** 2 / mean).sum())
    print(f"chi^2 of the single draws: {chi2:.2f}")
    assert chi2 < 26


def test_restated_sampler_with_unit_weights_keeps_the_structure():
    """The restated sampler on the KAT graph: every hop's picks are distinct entries of
    positive weight of the expanded row, and a fan-out of -1 takes every entry."""
    from test_walk_saint import KAT_COL, KAT_ROWPTR
    from test_weighted_ref import KAT_CUM, KAT_W

    n_id, rowptr, col, e_id, nodes, edges = nr.neighbor_sample_ref(KAT_ROWPTR, KAT_COL, KAT_CUM, [0, 2], [2, 2], False, 7)
    assert len(set(e_id.tolist())) == len(e_id) == sum(edges) and all(KAT_W[e] > 0 for e in e_id)
    assert np.array_equal(np.asarray(KAT_COL)[e_id], n_id[col]) and sum(nodes) == len(n_id)
    import neighbor_ref

    all_uniform = neighbor_ref.neighbor_sample_ref(KAT_ROWPTR, KAT_COL, [0, 2], [-1], False, 7)
    all_weighted = nr.neighbor_sample_ref(KAT_ROWPTR, KAT_COL, KAT_CUM, [0, 2], [-1], False, 7)
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(all_uniform, all_weighted))


# ---- the surface ------------------------------------------------------------------------------
def test_new_names_are_declared_exported_and_bound():
    from test_abi import declared_functions

    import paddle_sparse_amd as psa
    from paddle_sparse_amd import SparseTensor, _lib, ops

    for fn in (psa.neighbor_sample, SparseTensor.neighbor_sample, psa.NeighborSampler.__init__):
        assert inspect.signature(fn).parameters["weighted"].default is None
    assert inspect.signature(ops.neighbor_sample).parameters["cum"].default is None
    assert callable(ops.weighted_pick_without_host)
    declared = declared_functions()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("psa_weighted_pick_without_host", "psa_neighbor_hop_pick_weighted"):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["psa_neighbor_hop_pick_weighted"][1]) == len(_lib.SIGNATURES["psa_neighbor_hop_pick"][1]) + 1
    assert not [name for name in declared if "weighted" in name and "workspace" in name]  # the hop's workspace serves


def _cpu_csr(value=None):
    from paddle_sparse_amd import SparseTensor

    return SparseTensor(rowptr=torch.tensor([0, 2, 3, 3]), col=torch.tensor([0, 2, 1]),
                        value=torch.ones(3) if value is None else value, sparse_sizes=(3, 3), is_sorted=True,
                        trust_data=True)


def test_bad_arguments_raise_before_any_launch():
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import ops

    a = _cpu_csr()
    seeds = torch.tensor([0])
    for bad in ("yes", 3.5, 1, torch.ones(3, dtype=torch.float64)):
        with pytest.raises(TypeError, match="EdgeCDF"):
            psa.neighbor_sample(a, seeds, [2], weighted=bad)
        with pytest.raises(TypeError, match="EdgeCDF"):
            psa.NeighborSampler(a, [2], weighted=bad)
        with pytest.raises(TypeError, match="EdgeCDF"):
            a.neighbor_sample(seeds, [2], weighted=bad)
    # an EdgeCDF of another matrix (put together by hand: building one runs a kernel)
    other = psa.EdgeCDF.__new__(psa.EdgeCDF)
    other.rowptr, other.cum = _cpu_csr().storage.rowptr(), torch.ones(3, dtype=torch.float64)
    with pytest.raises(ValueError, match="another matrix"):
        psa.neighbor_sample(a, seeds, [2], weighted=other)
    with pytest.raises(ValueError, match="another matrix"):
        psa.NeighborSampler(a, [2], replace=True, directed=False, weighted=other)
    # the uniform checks still come first
    with pytest.raises(ValueError, match=">= -1"):
        psa.NeighborSampler(a, [-2], weighted=other)
    with pytest.raises(ValueError, match="values"):
        psa.neighbor_sample(psa.SparseTensor(rowptr=torch.tensor([0, 2, 3, 3]), col=torch.tensor([0, 2, 1]),
                                             sparse_sizes=(3, 3), is_sorted=True, trust_data=True), seeds, [2], weighted=True)
    # ops.neighbor_sample: cum of the wrong length, dtype or kind
    rowptr, col, _ = a.csr()
    with pytest.raises(ValueError, match="cum"):
        ops.neighbor_sample(rowptr, col, seeds, [2], cum=torch.ones(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="cum"):
        ops.neighbor_sample(rowptr, col, seeds, [2], cum=torch.ones(3, 1, dtype=torch.float64))
    with pytest.raises(TypeError, match="float64"):
        ops.neighbor_sample(rowptr, col, seeds, [2], cum=torch.ones(3, dtype=torch.float32))
    with pytest.raises(TypeError, match="cum"):
        ops.neighbor_sample(rowptr, col, seeds, [2], cum=[1.0, 2.0, 3.0])
    # a well-formed cum on CPU tensors: refused as every CPU tensor is
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.neighbor_sample(rowptr, col, seeds, [2], cum=torch.ones(3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        a.neighbor_sample(seeds, [2], weighted=True)
    with pytest.raises(ValueError):
        ops.weighted_pick_without_host([1.0, 2.0], 2, [1], [1, 2])


def test_weighted_sample_adj_without_replacement_still_raises():
    a = _cpu_csr()
    with pytest.raises(NotImplementedError, match="without replacement"):
        a.sample_adj(torch.tensor([0, 1]), 1, replace=False, seed=1, weighted=True)
