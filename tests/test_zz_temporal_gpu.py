"""GPU suite for temporal_neighbor_sample and EdgeTimeOrder.  The op is index work, so every
comparison is bit-exact against the serial restatement of tests/temporal_ref.py (pinned by
test_zz_temporal_ref.py), on all six outputs and on the index; values ride on e_id and are
compared exactly too.  Every result is also held to the property the op exists for: no entry
of ego g is newer than seed_time[g].

The file name sorts behind every other GPU file on purpose: the new tests are collected last, so
the tests that were there before keep their positions in a run of the whole suite."""
import functools

import numpy as np
import pytest
import torch

from temporal_ref import temporal_neighbor_sample_ref, time_of_entries, time_order_ref
from test_walk_saint_gpu import adj_of, gpu, sorted_csr
from test_zz_temporal_ref import (HAND_ALL, HAND_COL, HAND_LAST_22, HAND_NODE_TIME, HAND_ORDER, HAND_ROWPTR, HAND_SEED_TIME,
                                  HAND_SEEDS, HAND_SORTED_TIME, HAND_TIME)

pytestmark = pytest.mark.gpu

BIG_SEED = 2**63 + 11
NAMES = ("n_id", "ptr", "root", "rowptr", "col", "e_id")
MODES = (("uniform", False), ("uniform", True), ("last", False))


def unpack(res):
    sub, n_id, e_id, ptr, root = res
    st = sub.storage
    got = tuple(x.cpu().numpy() for x in (n_id, ptr, root, st.rowptr(), st.col(), e_id))
    assert sub.sparse_sizes() == (n_id.numel(), n_id.numel())
    return got, sub


def assert_same(got, want, what=""):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w), (what, name)


def assert_time_property(got, time, seed_time):
    """Every returned entry of ego g has time_of(e_id) <= seed_time[g]; the ego of an entry is the
    block its row lies in."""
    n_id, ptr, _, rowptr, col, e_id = got
    rows = np.repeat(np.arange(len(n_id)), np.diff(rowptr))
    ego = np.searchsorted(ptr, rows, side="right") - 1
    assert np.array_equal(ego, np.searchsorted(ptr, col, side="right") - 1)  # block-diagonal
    assert all(time[e] <= seed_time[g] for e, g in zip(e_id.tolist(), ego.tolist()))


class Case:
    """A matrix on the device with its time order, and the same graph for the restatement."""

    def __init__(self, rowptr, col, edge_time=None, node_time=None, value=None):
        from paddle_sparse_amd import EdgeTimeOrder

        self.rowptr, self.col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
        self.time = time_of_entries(self.col, edge_time, node_time)
        self.adj = adj_of(self.rowptr, self.col, value)
        if edge_time is not None:
            self.order = EdgeTimeOrder(self.adj, edge_time=gpu(np.asarray(edge_time, np.int64)))
        else:
            self.order = EdgeTimeOrder(self.adj, node_time=gpu(np.asarray(node_time, np.int64)))

    def check(self, seeds, seed_time, fanouts, strategy="uniform", replace=False, seed=0, want=None):
        res = self.adj.temporal_neighbor_sample(gpu(seeds), gpu(seed_time), list(fanouts), time=self.order,
                                                strategy=strategy, replace=replace, seed=seed)
        got, sub = unpack(res)
        if want is None:
            want = temporal_neighbor_sample_ref(self.rowptr, self.col, self.time, seeds, seed_time, fanouts, strategy,
                                                replace, seed)
        assert_same(got, want, (list(fanouts), strategy, replace, seed))
        assert_time_property(got, self.time, [int(t) for t in seed_time])
        return got, sub


def assert_index(case):
    order, sorted_time = time_order_ref(case.rowptr, case.time)
    assert case.order.order.dtype == torch.int64 and case.order.sorted_time.dtype == torch.int64
    assert case.order.order.cpu().tolist() == order and case.order.sorted_time.cpu().tolist() == sorted_time


# ---- the hand graph -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hand():
    return Case(HAND_ROWPTR, HAND_COL, edge_time=HAND_TIME)


def test_hand_graph_index_and_known_answers():
    import paddle_sparse_amd as psa

    case = hand()
    assert case.order.order.cpu().tolist() == HAND_ORDER and case.order.sorted_time.cpu().tolist() == HAND_SORTED_TIME
    a = lambda xs: tuple(np.array(x, np.int64) for x in xs)
    case.check(HAND_SEEDS, HAND_SEED_TIME, [2, 2], "last", want=a(HAND_LAST_22))
    case.check(HAND_SEEDS, HAND_SEED_TIME, [-1], "uniform", seed=9, want=a(HAND_ALL))
    case.check(HAND_SEEDS, HAND_SEED_TIME, [3], "uniform", seed=4, want=a(HAND_ALL))
    # the function form, int32 seeds and bounds
    res = psa.temporal_neighbor_sample(case.adj, gpu(HAND_SEEDS, torch.int32), gpu(HAND_SEED_TIME, torch.int32), [2, 2],
                                       case.order, "last")
    assert_same(unpack(res)[0], a(HAND_LAST_22))


@pytest.mark.parametrize("strategy,replace", MODES)
def test_hand_graph_one_node_under_two_bounds(strategy, replace):
    case = hand()
    for seed in (0, 3, BIG_SEED):
        got, _ = case.check(HAND_SEEDS, HAND_SEED_TIME, [2, 2], strategy, replace, seed)
        n_id, ptr = got[0], got[1]
        assert n_id[ptr[0]] == 0 and n_id[ptr[1]] == 0  # egos 0 and 1 are both node 0's
    node = Case(HAND_ROWPTR, HAND_COL, node_time=HAND_NODE_TIME)
    assert_index(node)
    node.check(HAND_SEEDS, [4, 2, 9], [2, 2], strategy, replace, 5)
    node.check([4], [-5], [2], strategy, replace, 5)  # the seed's own time (9) is not checked; nothing is eligible


# ---- a hub: ties, a time order unlike the storage order, Floyd in registers and in memory ------------
@functools.lru_cache(maxsize=None)
def hub():
    """N = 300.  Row 0 holds 300 entries with times (p * 7) % 97, entry 0 moved to -1 so that one
    entry is the oldest alone; rows 1 .. 299 have 0 to 3 entries."""
    rng = np.random.default_rng(11)
    N = 300
    degs = np.concatenate([[300], np.arange(1, N) % 4])
    cols = [np.arange(N)] + [np.sort(rng.choice(N, d, replace=False)) for d in degs[1:]]
    rowptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int64)
    col = np.concatenate(cols).astype(np.int64)
    time = np.concatenate([(np.arange(300) * 7) % 97, rng.integers(0, 97, len(col) - 300)]).astype(np.int64)
    time[0] = -1
    return Case(rowptr, col, edge_time=time)


HUB_SEEDS, HUB_BOUNDS = [0, 0, 0, 0, 7, 0], [-2, -1, 48, 96, 50, 48]


def test_hub_index_and_eligible_counts():
    case = hub()
    assert_index(case)
    t = np.array(case.time[:300])
    assert [(t <= b).sum() for b in HUB_BOUNDS[:4]] == [0, 1, 154, 300] and (t == 48).sum() == 3  # 48 is a tie
    assert not np.array_equal(case.order.order[:300].cpu().numpy(), np.arange(300))


@pytest.mark.parametrize("k", [1, 5, 32, 33, 299, 300, 301, -1])
def test_hub_fanouts(k):
    case = hub()
    for strategy, replace in MODES:
        for seed in (1, BIG_SEED):
            got, _ = case.check(HUB_SEEDS, HUB_BOUNDS, [k], strategy, replace, seed)
        ptr = got[1]
        assert ptr[1] - ptr[0] == 1  # c = 0: the ego is its seed alone
        if k < 33:
            case.check(HUB_SEEDS, HUB_BOUNDS, [k, 2], strategy, replace, 2)


def test_hub_same_seed_same_bits_another_seed_differs():
    case = hub()
    for strategy, replace in MODES[:2]:
        a, _ = case.check(HUB_SEEDS, HUB_BOUNDS, [5, 2], strategy, replace, 7)
        b, _ = case.check(HUB_SEEDS, HUB_BOUNDS, [5, 2], strategy, replace, 7)
        c, _ = case.check(HUB_SEEDS, HUB_BOUNDS, [5, 2], strategy, replace, 8)
        assert_same(a, b)
        assert not all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, c))
    res = [case.adj.temporal_neighbor_sample(gpu(HUB_SEEDS), gpu(HUB_BOUNDS), [5], time=case.order) for _ in range(2)]
    assert not torch.equal(res[0][2], res[1][2]) or not torch.equal(res[0][1], res[1][1])  # seed=None: drawn per call


# ---- a random graph ---------------------------------------------------------------------------------
R_N = 200
R_FANOUTS = ([3, 2, 2], [-1, 2], [2, -1], [5, 0, 3], [0], [])


@functools.lru_cache(maxsize=None)
def random_graph():
    """N = 200, mean degree 6, rows 150 .. 199 empty, 200 stored duplicates (their times differ)."""
    rng = np.random.default_rng(21)
    row = rng.integers(0, 150, 1000)
    col = rng.integers(0, R_N, 1000)
    row, col = np.concatenate([row, row[:200]]), np.concatenate([col, col[:200]])
    rowptr, col = sorted_csr(row, col, R_N)
    edge_time = rng.integers(-50, 50, len(col))
    node_time = rng.integers(-50, 50, R_N)
    seeds = rng.integers(0, R_N, 64)
    seeds[40:48] = seeds[:8]  # repeats
    seeds[63] = 199  # an empty row
    seed_time = rng.integers(-60, 60, 64)
    return rowptr, col, edge_time, node_time, seeds, seed_time


@functools.lru_cache(maxsize=None)
def random_case(mode):
    rowptr, col, edge_time, node_time, _, _ = random_graph()
    value = torch.arange(1, len(col) + 1, dtype=torch.float32).cuda()
    return Case(rowptr, col, value=value, **({"edge_time": edge_time} if mode == "edge" else {"node_time": node_time}))


def test_random_graph_covers_what_it_is_for():
    rowptr, col, edge_time, _, seeds, seed_time = random_graph()
    assert np.diff(rowptr).min() == 0 and len(set(seeds.tolist())) < 64
    pairs = np.stack([np.repeat(np.arange(R_N), np.diff(rowptr)), col])
    dup = np.flatnonzero((pairs[:, 1:] == pairs[:, :-1]).all(0))
    assert len(dup) >= 100 and (edge_time[dup] != edge_time[dup + 1]).any()
    (_, hops, parents) = temporal_neighbor_sample_ref(rowptr, col, edge_time.tolist(), seeds, seed_time, [3, 2, 2],
                                                      with_walk=True)
    assert any(c == 0 for c, _ in parents) and any(0 < c < k for c, k in parents) and any(c > k for c, k in parents)
    slots = [(g, e) for hop in hops for _, g, e in hop if e >= 0]
    assert len(set(slots)) < len(slots)  # some (ego, entry) is emitted by two slots
    egos_of = {}
    for g, e in slots:
        egos_of.setdefault(e, set()).add(g)
    assert any(len(s) > 1 for s in egos_of.values())  # some entry lands in two egos


@pytest.mark.parametrize("mode", ["edge", "node"])
@pytest.mark.parametrize("strategy,replace", MODES)
def test_random_graph_fanout_lists(mode, strategy, replace):
    case = random_case(mode)
    _, _, _, _, seeds, seed_time = random_graph()
    if (strategy, replace) == MODES[0]:
        assert_index(case)
    for fanouts in R_FANOUTS:
        got, sub = case.check(seeds, seed_time, fanouts, strategy, replace, 13)
        e_id = got[5]
        assert torch.equal(sub.storage.value().cpu(), torch.from_numpy(e_id + 1).float())  # value[e_id]
        if fanouts in ([0], []):
            assert got[0].tolist() == seeds.tolist() and got[1].tolist() == list(range(65)) and len(e_id) == 0
        if fanouts == [5, 0, 3]:
            first, _ = case.check(seeds, seed_time, [5], strategy, replace, 13)
            assert_same(got, first, "a zero fan-out ends the sampling")
    case.check(seeds, seed_time, [3, 2], strategy, replace, BIG_SEED)


def test_against_ego_k_hop_sample_when_nothing_is_in_the_future():
    case = random_case("edge")
    _, _, _, _, seeds, _ = random_graph()
    got, _ = case.check(seeds, np.full(64, 50), [-1, -1])
    _, n_id, _, ptr, root = case.adj.ego_k_hop_sample(gpu(seeds), [-1, -1])
    assert np.array_equal(got[0], n_id.cpu().numpy()) and np.array_equal(got[1], ptr.cpu().numpy())
    assert np.array_equal(got[2], root.cpu().numpy())


# ---- negative times and the span limit ----------------------------------------------------------------
def test_negative_times_and_a_span_just_under_two_to_the_62():
    from paddle_sparse_amd import EdgeTimeOrder

    lo, hi = -2**61, 2**61 - 1  # a span of 2^62 - 1
    scale = {-1: lo, 10: hi}
    time = [scale.get(t, t * 2**50 - 7) for t in HAND_TIME]
    case = Case(HAND_ROWPTR, HAND_COL, edge_time=time)
    assert_index(case)
    assert (case.order.min_time, case.order.max_time) == (lo, hi)
    bounds = [5 * 2**50, lo, hi]
    for strategy, replace in MODES:
        case.check([0, 5, 7], bounds, [2, 2], strategy, replace, 3)
    case.check([0, 5, 7], [lo - 1, lo - 1, hi - 1], [-1])  # below every time of rows 0 and 5; row 7's is hi
    time[11] = lo - 1  # a span of exactly 2^62
    with pytest.raises(ValueError, match="span"):
        EdgeTimeOrder(case.adj, edge_time=gpu(np.array(time, np.int64)))


# ---- argument errors, empty inputs, the input is untouched -------------------------------------------------
def test_empty_inputs_and_argument_errors():
    from paddle_sparse_amd import EdgeTimeOrder

    case = hand()
    got, _ = case.check([], [], [2, 2])
    assert [len(x) for x in got] == [0, 1, 0, 1, 0, 0]
    with pytest.raises(IndexError):
        case.adj.temporal_neighbor_sample(gpu([0, 8]), gpu([5, 5]), [2], time=case.order, seed=1)
    with pytest.raises(IndexError):
        case.adj.temporal_neighbor_sample(gpu([-1]), gpu([5]), [], time=case.order, seed=1)
    other = adj_of(np.array(HAND_ROWPTR), np.array(HAND_COL))
    with pytest.raises(ValueError, match="another matrix"):
        other.temporal_neighbor_sample(gpu([0]), gpu([5]), [2], time=case.order, seed=1)
    with pytest.raises(ValueError, match="seed_time"):
        case.adj.temporal_neighbor_sample(gpu([0, 1]), gpu([5]), [2], time=case.order, seed=1)
    empty = Case(np.zeros(6, np.int64), np.zeros(0, np.int64), edge_time=np.zeros(0, np.int64))
    assert empty.order.order.numel() == 0 and empty.order.sorted_time.numel() == 0
    got, _ = empty.check([3, 3, 0], [1, 2, 3], [2, -1])
    assert got[0].tolist() == [3, 3, 0] and got[2].tolist() == [0, 1, 2] and len(got[5]) == 0
    with pytest.raises(ValueError):
        EdgeTimeOrder(case.adj, edge_time=gpu(HAND_TIME[:-1]))
    with pytest.raises(TypeError):
        EdgeTimeOrder(case.adj, edge_time=gpu(HAND_TIME).float())


def test_the_input_is_untouched():
    from paddle_sparse_amd import EdgeTimeOrder

    rowptr, col, edge_time, _, seeds, seed_time = random_graph()
    value = torch.arange(len(col), dtype=torch.float32).cuda()
    adj = adj_of(rowptr, col, value)
    r, c, v = adj.csr()
    before = (r.data_ptr(), c.data_ptr(), v.data_ptr(), r.clone(), c.clone(), v.clone())
    t = gpu(edge_time, torch.int32)
    t_before = t.clone()
    order = EdgeTimeOrder(adj, edge_time=t)
    adj.temporal_neighbor_sample(gpu(seeds), gpu(seed_time), [3, -1], time=order, seed=1)
    r, c, v = adj.csr()
    assert (r.data_ptr(), c.data_ptr(), v.data_ptr()) == before[:3]
    assert torch.equal(r, before[3]) and torch.equal(c, before[4]) and torch.equal(v, before[5])
    assert torch.equal(t, t_before) and t.dtype == torch.int32


def test_gradient_is_the_count_of_every_entry():
    rowptr, col, edge_time, _, seeds, seed_time = random_graph()
    value = torch.ones(len(col), dtype=torch.float32, device="cuda", requires_grad=True)
    case = Case(rowptr, col, edge_time=edge_time, value=value)
    sub, _, e_id, _, _ = case.adj.temporal_neighbor_sample(gpu(seeds), gpu(seed_time), [3, 2], time=case.order, seed=2)
    sub.storage.value().sum().backward()
    want = torch.bincount(e_id, minlength=len(col)).float()
    assert want.max() > 1 and torch.equal(value.grad, want)
