"""CPU suite for temporal_neighbor_sample: hand answers that pin the restatement of
tests/temporal_ref.py, the host export of the kernels' pick rule against it bit for bit,
properties of the picks computed without the pick code, the law of the exact Floyd walk, and
the argument errors raised before any launch.  No kernel runs."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

from neighbor_ref import picks_of_row
from temporal_ref import (eligible_ref, ranks_ref, temporal_neighbor_sample_ref, temporal_walk_ref, time_of_entries,
                          time_order_ref)

SYMBOLS = ("psa_temporal_hop_count", "psa_temporal_hop_pick", "psa_temporal_total", "psa_temporal_finish",
           "psa_temporal_pick_host")

# ---- the hand graph: 8 nodes, 14 entries ------------------------------------------------------------
# row 0: 1@5 2@3 3@9 4@3 | row 1: 0@2 2@7 | row 2: 0@4 3@1 3@6 (a stored duplicate, two times) | row 3: none
# row 4: 0@8 5@0 | row 5: 6@-1 | row 6: 7@2 | row 7: 5@10
HAND_ROWPTR = [0, 4, 6, 9, 9, 11, 12, 13, 14]
HAND_COL = [1, 2, 3, 4, 0, 2, 0, 3, 3, 0, 5, 6, 7, 5]
HAND_TIME = [5, 3, 9, 3, 2, 7, 4, 1, 6, 8, 0, -1, 2, 10]
HAND_ORDER = [1, 3, 0, 2, 4, 5, 7, 6, 8, 10, 9, 11, 12, 13]
HAND_SORTED_TIME = [3, 3, 5, 9, 2, 7, 1, 4, 6, 0, 8, -1, 2, 10]
HAND_NODE_TIME = [4, 1, 7, 2, 9, 0, 3, 5]
HAND_SEEDS, HAND_SEED_TIME = [0, 0, 4], [5, 3, 8]  # node 0 twice, under two bounds

# strategy "last", fan-outs [2, 2], worked by hand:
#  hop 1  ego 0 (node 0, T 5): c = 3, ranks 2 1 -> entries 0 (col 1), 3 (col 4)
#         ego 1 (node 0, T 3): c = 2, ranks 1 0 -> entries 3 (col 4), 1 (col 2)
#         ego 2 (node 4, T 8): c = 2, ranks 1 0 -> entries 9 (col 0), 10 (col 5)
#  hop 2  (1, ego 0): c = 1 -> entry 4 (col 0)     (4, ego 0): c = 1 -> entry 10 (col 5)
#         (4, ego 1): c = 1 -> entry 10 (col 5)    (2, ego 1): c = 1 -> entry 7 (col 3)
#         (0, ego 2): c = 3 -> entries 0, 3        (5, ego 2): c = 1 -> entry 11 (col 6)
HAND_LAST_22 = ([0, 1, 4, 5, 0, 2, 3, 4, 5, 0, 1, 4, 5, 6], [0, 4, 9, 14], [0, 4, 11],
                [0, 2, 3, 4, 4, 6, 7, 7, 8, 8, 10, 10, 12, 13, 13], [1, 2, 0, 3, 5, 7, 6, 8, 10, 11, 9, 12, 13],
                [0, 3, 4, 10, 1, 3, 7, 10, 0, 3, 9, 10, 11])
# fan-outs [-1]: every eligible entry of the seeds' rows
HAND_ALL = ([0, 1, 2, 4, 0, 2, 4, 0, 4, 5], [0, 4, 7, 10], [0, 4, 8], [0, 3, 3, 3, 3, 5, 5, 5, 5, 7, 7],
            [1, 2, 3, 5, 6, 7, 9], [0, 1, 3, 1, 3, 9, 10])


def as_lists(out):
    return tuple(x.tolist() for x in out)


def test_time_order_of_the_hand_graph():
    order, sorted_time = time_order_ref(HAND_ROWPTR, HAND_TIME)
    assert order == HAND_ORDER and sorted_time == HAND_SORTED_TIME
    assert time_of_entries(HAND_COL, node_time=HAND_NODE_TIME) == [1, 7, 2, 9, 4, 7, 4, 2, 2, 4, 0, 3, 5, 0]
    assert time_of_entries(HAND_COL, edge_time=HAND_TIME) == HAND_TIME


def test_hand_answers():
    got = temporal_neighbor_sample_ref(HAND_ROWPTR, HAND_COL, HAND_TIME, HAND_SEEDS, HAND_SEED_TIME, [2, 2], "last")
    assert as_lists(got) == HAND_LAST_22
    for strategy, replace in (("uniform", False), ("last", False)):
        got = temporal_neighbor_sample_ref(HAND_ROWPTR, HAND_COL, HAND_TIME, HAND_SEEDS, HAND_SEED_TIME, [-1], strategy,
                                           replace, seed=9)
        assert as_lists(got) == HAND_ALL
    # c <= k everywhere: "uniform" without replacement takes all eligible entries, as [-1] does
    got = temporal_neighbor_sample_ref(HAND_ROWPTR, HAND_COL, HAND_TIME, HAND_SEEDS, HAND_SEED_TIME, [3], "uniform")
    assert as_lists(got) == HAND_ALL
    # no fan-outs, and a zero fan-out: each ego is its seed alone
    for fanouts in ([], [0, 2]):
        got = temporal_neighbor_sample_ref(HAND_ROWPTR, HAND_COL, HAND_TIME, HAND_SEEDS, HAND_SEED_TIME, fanouts)
        assert as_lists(got) == ([0, 0, 4], [0, 1, 2, 3], [0, 1, 2], [0, 0, 0, 0], [], [])
    # nothing is eligible before time -1
    got = temporal_neighbor_sample_ref(HAND_ROWPTR, HAND_COL, HAND_TIME, [0, 5], [2, -2], [2, 2])
    assert as_lists(got) == ([0, 5], [0, 1, 2], [0, 1], [0, 0, 0], [], [])


def test_hand_walk_has_empty_slots_that_stay_empty():
    hops, parents = temporal_walk_ref(HAND_ROWPTR, HAND_COL, HAND_TIME, HAND_SEEDS, HAND_SEED_TIME, [2, 2], "last")
    assert [len(h) for h in hops] == [3, 6, 12]
    assert hops[1] == [(1, 0, 0), (4, 0, 3), (4, 1, 3), (2, 1, 1), (0, 2, 9), (5, 2, 10)]
    assert hops[2] == [(0, 0, 4), (-1, 0, -1), (5, 0, 10), (-1, 0, -1), (5, 1, 10), (-1, 1, -1), (3, 1, 7), (-1, 1, -1),
                       (1, 2, 0), (4, 2, 3), (6, 2, 11), (-1, 2, -1)]
    assert [c for c, _ in parents] == [3, 2, 2, 1, 1, 1, 1, 3, 1]
    hops3, _ = temporal_walk_ref(HAND_ROWPTR, HAND_COL, HAND_TIME, HAND_SEEDS, HAND_SEED_TIME, [2, 2, 1], "last")
    assert hops3[:3] == hops and len(hops3[3]) == 12
    assert [hops3[3][i] for i in (1, 3, 5, 7, 11)] == [(-1, 0, -1), (-1, 0, -1), (-1, 1, -1), (-1, 1, -1), (-1, 2, -1)]


# ---- the host export against the restatement ---------------------------------------------------------
def host_picks(sorted_time, start, deg, bound, k, replace, strategy, seed, stream):
    from paddle_sparse_amd import ops

    return ops.temporal_pick_host(sorted_time, start, deg, bound, k, replace, strategy, seed, stream)


MODES = (("uniform", False), ("uniform", True), ("last", False))
SEEDS = (0, 12345, 2**63 + 11)


def properties(ranks, c, k, replace):
    """What the picks must satisfy, whatever the rule that made them."""
    assert all(0 <= r < c for r in ranks)  # eligible
    if k < 0:
        assert ranks == list(range(c))
    elif replace:
        assert len(ranks) == (k if c > 0 else 0)
    else:
        assert len(ranks) == min(k, c) and len(set(ranks)) == len(ranks)


@pytest.mark.parametrize("deg", [0, 1, 2, 33, 300])
def test_host_export_equals_the_restatement_over_the_grid(deg):
    pad = [99, 98, 97]
    row = [2 * i - 7 for i in range(deg)]  # distinct, some negative
    sorted_time = pad + row + [-99, -98]
    stream = 5
    for k in (1, 5, 32, 33):
        for c in sorted({x for x in (0, 1, k - 1, k, k + 1, deg) if 0 <= x <= deg}):
            bound = row[c - 1] if c > 0 else -100
            assert eligible_ref(sorted_time, 3, deg, bound) == c
            for (strategy, replace), seed in itertools.product(MODES, SEEDS):
                stream += 1
                got = host_picks(sorted_time, 3, deg, bound, k, replace, strategy, seed, stream)
                assert got == ranks_ref(c, k, replace, strategy, seed, stream), (deg, k, c, strategy, replace, seed)
                properties(got, c, k, replace)
    for c in {0, deg // 2, deg}:  # k < 0: all eligible, ascending
        bound = row[c - 1] if c > 0 else -100
        assert host_picks(sorted_time, 3, deg, bound, -1, False, "uniform", 1, 2) == list(range(c))


def test_ties_at_the_boundary():
    sorted_time = [1, 1, 4, 4, 4, 4, 9, 9]
    for bound, c in ((0, 0), (1, 2), (3, 2), (4, 6), (5, 6), (8, 6), (9, 8), (2**62, 8), (-2**62, 0)):
        assert eligible_ref(sorted_time, 0, 8, bound) == c
        assert host_picks(sorted_time, 0, 8, bound, -1, False, "uniform", 0, 0) == list(range(c))
        assert host_picks(sorted_time, 0, 8, bound, 3, False, "last", 0, 0) == [c - 1 - t for t in range(min(3, c))]
        for k, replace in ((2, False), (5, False), (7, True)):
            got = host_picks(sorted_time, 0, 8, bound, k, replace, "uniform", 4, 17)
            assert got == ranks_ref(c, k, replace, "uniform", 4, 17)
            properties(got, c, k, replace)
    # a segment inside a longer array: the search never leaves [start, start + deg)
    assert host_picks([0, 0, 5, 6, 7, 0, 0], 2, 3, 6, -1, False, "uniform", 0, 0) == [0, 1]
    assert host_picks([0, 0, 5, 6, 7, 0, 0], 2, 3, 0, -1, False, "uniform", 0, 0) == []


def test_floyd_in_registers_and_in_memory_agree_on_the_rule():
    """k = 32 runs the register walk, k = 33 the walk in memory: both are the restatement's."""
    sorted_time = list(range(300))
    for k in (31, 32, 33, 64, 299):
        for seed in SEEDS:
            got = host_picks(sorted_time, 0, 300, 299, k, False, "uniform", seed, k)
            assert got == ranks_ref(300, k, False, "uniform", seed, k)
            properties(got, 300, k, False)


def test_host_export_refuses_bad_arguments():
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    arr = (ctypes.c_int64 * 4)(1, 2, 3, 4)
    out = (ctypes.c_int64 * 2)()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    assert lib.psa_temporal_pick_host(p(arr), 0, 4, 4, -1, 0, 0, 0, 0, p(out), 2) == -1  # 4 ranks, room for 2
    assert lib.psa_temporal_pick_host(p(arr), 0, 4, 4, 2, 1, 1, 0, 0, p(out), 2) == -1  # last with replacement
    assert lib.psa_temporal_pick_host(p(arr), 0, 4, 4, 2, 0, 7, 0, 0, p(out), 2) == -1  # unknown strategy
    assert lib.psa_temporal_pick_host(p(arr), 0, 4, 2, 2, 0, 1, 0, 0, p(out), 2) == 2 and list(out) == [1, 0]


# ---- the law ---------------------------------------------------------------------------------------
LAW_C, LAW_K, LAW_STREAMS = 25, 5, 20_000
LAW_BOUND = 283  # 5 sigma of Binomial(20000, 0.2): 5 * sqrt(20000 * 0.2 * 0.8) = 282.8


@functools.lru_cache(maxsize=None)
def law_counts(replace):
    sorted_time = list(range(LAW_C))
    counts = np.zeros(LAW_C, np.int64)
    for i in range(LAW_STREAMS):
        for r in host_picks(sorted_time, 0, LAW_C, LAW_C, LAW_K, replace, "uniform", 0, i):
            counts[r] += 1
    return counts


@pytest.mark.parametrize("replace", [False, True])
def test_every_rank_is_picked_with_probability_k_over_c(replace):
    counts = law_counts(replace)
    assert counts.sum() == LAW_STREAMS * LAW_K
    worst = int(np.abs(counts - LAW_STREAMS * LAW_K // LAW_C).max())
    print(f"replace={replace}: largest deviation from 4000 = {worst}")
    assert worst <= LAW_BOUND, counts.tolist()


def test_the_law_test_tells_the_two_floyd_rules_apart():
    """The walk of sample_adj (draw in [0, j), upstream's rule) fails the same bound: its last k
    ranks are under-sampled.  temporal_neighbor_sample must not reuse it."""
    counts = np.zeros(LAW_C, np.int64)
    for i in range(LAW_STREAMS):
        for e in picks_of_row(0, LAW_C, LAW_K, False, 0, i):
            counts[e] += 1
    dev = np.abs(counts - 4000)
    assert dev.max() > 2 * LAW_BOUND and dev[LAW_C - LAW_K:].min() > LAW_BOUND, counts.tolist()


# ---- the surface and the argument errors that need no GPU --------------------------------------------
def test_the_op_is_exported_attached_and_bound():
    from test_abi import declared_functions

    import paddle_sparse_amd as psa
    from paddle_sparse_amd import SparseTensor, _lib, temporal

    assert "temporal_neighbor_sample" in psa.__all__ and "EdgeTimeOrder" in psa.__all__
    assert psa.temporal_neighbor_sample is temporal.temporal_neighbor_sample
    assert psa.EdgeTimeOrder is temporal.EdgeTimeOrder
    assert SparseTensor.temporal_neighbor_sample is temporal.temporal_neighbor_sample
    declared = declared_functions()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in SYMBOLS:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert not name.endswith("_workspace_bytes")


def cpu_adj(M=8, N=8):
    from paddle_sparse_amd import SparseTensor

    return SparseTensor(rowptr=torch.tensor(HAND_ROWPTR[:M + 1]), col=torch.tensor(HAND_COL[:HAND_ROWPTR[M]]),
                        sparse_sizes=(M, N), is_sorted=True, trust_data=True)


def test_edge_time_order_argument_errors():
    from paddle_sparse_amd import EdgeTimeOrder

    adj = cpu_adj()
    t = torch.tensor(HAND_TIME)
    with pytest.raises(TypeError):
        EdgeTimeOrder(adj)
    with pytest.raises(TypeError):
        EdgeTimeOrder(adj, edge_time=t, node_time=torch.tensor(HAND_NODE_TIME))
    with pytest.raises(TypeError):
        EdgeTimeOrder("adj", edge_time=t)
    for bad in (t.float(), t > 0, t.double()):
        with pytest.raises(TypeError):
            EdgeTimeOrder(adj, edge_time=bad)
        with pytest.raises(TypeError):
            EdgeTimeOrder(adj, node_time=bad[:8])
    with pytest.raises(ValueError):
        EdgeTimeOrder(adj, edge_time=t[:-1])
    with pytest.raises(ValueError):
        EdgeTimeOrder(adj, node_time=torch.tensor(HAND_NODE_TIME + [0]))
    with pytest.raises(ValueError):
        EdgeTimeOrder(adj, edge_time=t.view(2, 7))
    wide = t.clone()
    wide[0], wide[1] = -2**61, 2**61  # a span of exactly 2^62
    with pytest.raises(ValueError, match="span"):
        EdgeTimeOrder(adj, edge_time=wide)
    wide[1] = 2**61 - 1  # 2^62 - 1 passes the check and goes on to the device, which a CPU tensor is not on
    with pytest.raises(RuntimeError, match="GPU tensor"):
        EdgeTimeOrder(adj, edge_time=wide)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        EdgeTimeOrder(adj, edge_time=t.to(torch.int32))


def fake_order(adj):
    """An EdgeTimeOrder filled in by hand: its constructor needs the device."""
    from paddle_sparse_amd import EdgeTimeOrder

    order = object.__new__(EdgeTimeOrder)
    order.rowptr = adj.storage.rowptr()
    order.order, order.sorted_time = torch.tensor(HAND_ORDER), torch.tensor(HAND_SORTED_TIME)
    return order


def test_sample_argument_errors_before_any_launch():
    import paddle_sparse_amd as psa

    adj = cpu_adj()
    order = fake_order(adj)
    seeds, times = torch.tensor(HAND_SEEDS), torch.tensor(HAND_SEED_TIME)
    with pytest.raises(ValueError, match="square"):
        psa.temporal_neighbor_sample(cpu_adj(7, 8), seeds, times, [2], time=order)
    with pytest.raises(TypeError):
        adj.temporal_neighbor_sample(seeds, times, [2])  # no order
    with pytest.raises(TypeError):
        adj.temporal_neighbor_sample(seeds, times, [2], time=torch.tensor(HAND_TIME))
    with pytest.raises(TypeError):
        adj.temporal_neighbor_sample(seeds, times, 2, time=order)
    with pytest.raises(TypeError):
        adj.temporal_neighbor_sample(seeds, times, [2.0], time=order)
    with pytest.raises(ValueError):
        adj.temporal_neighbor_sample(seeds, times, [-2], time=order)
    with pytest.raises(ValueError, match="strategy"):
        adj.temporal_neighbor_sample(seeds, times, [2], time=order, strategy="first")
    with pytest.raises(ValueError, match="last"):
        adj.temporal_neighbor_sample(seeds, times, [2], time=order, strategy="last", replace=True)
    with pytest.raises(TypeError):
        adj.temporal_neighbor_sample(seeds.float(), times, [2], time=order)
    with pytest.raises(TypeError):
        adj.temporal_neighbor_sample(seeds, times.float(), [2], time=order)
    with pytest.raises(ValueError):
        adj.temporal_neighbor_sample(seeds.view(1, 3), times, [2], time=order)
    with pytest.raises(ValueError, match="seed_time"):
        adj.temporal_neighbor_sample(seeds, times[:2], [2], time=order)
    with pytest.raises(ValueError, match="another matrix"):
        cpu_adj().temporal_neighbor_sample(seeds, times, [2], time=order)
    with pytest.raises(RuntimeError, match="GPU tensor"):  # everything checked: the device is next
        adj.temporal_neighbor_sample(seeds, times, [2], time=order, seed=1)
