"""GPU suite for ego_k_hop_sample.  The op is index work, so every comparison is bit-exact
against the serial restatement of tests/ego_ref.py (pinned by test_ego_ref.py), on all six
outputs; values ride on e_id and are compared exactly too.

The file name sorts behind every other GPU file on purpose: the new tests are collected last, so
the tests that were there before keep their positions in a run of the whole suite."""
import functools

import numpy as np
import pytest
import torch

from ego_ref import ego_k_hop_sample_ref
from test_ego_ref import KAT_EGO
from test_walk_saint_gpu import adj_of, gpu, kat_adj, sorted_csr
from test_walk_saint_gpu import graph as _graph

pytestmark = pytest.mark.gpu

BIG_SEED = 2**63 + 11
NAMES = ("n_id", "ptr", "root", "rowptr", "col", "e_id")
FANOUTS = ([3], [2, 2], [-1], [-1, 2], [3, -1], [2, 0, 5], [])


def unpack(res):
    sub, n_id, e_id, ptr, root = res
    st = sub.storage
    got = tuple(x.cpu().numpy() for x in (n_id, ptr, root, st.rowptr(), st.col(), e_id))
    assert sub.sparse_sizes() == (n_id.numel(), n_id.numel())
    return got, sub


def assert_same(got, want, what=""):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w), (what, name)


def check(rowptr, col, seeds, fanouts, replace=False, seed=0, adj=None, want=None):
    adj = adj_of(rowptr, col) if adj is None else adj
    got, sub = unpack(adj.ego_k_hop_sample(gpu(seeds), list(fanouts), replace=replace, seed=seed))
    want = ego_k_hop_sample_ref(rowptr, col, seeds, fanouts, replace, seed) if want is None else want
    assert_same(got, want, (list(fanouts), replace, seed))
    assert not sub.has_value()
    return got


@functools.lru_cache(maxsize=None)
def graph(name):
    return _graph(name)


# ---- known answers ------------------------------------------------------------------------------
def test_known_answers_function_method_and_int32_seeds():
    import paddle_sparse_amd as psa

    adj = kat_adj()
    for (seeds, fanouts, replace, seed), want in KAT_EGO:
        got, _ = unpack(adj.ego_k_hop_sample(gpu(seeds), fanouts, replace=replace, seed=seed))
        assert tuple(x.tolist() for x in got) == tuple(want)
        got, _ = unpack(psa.ego_k_hop_sample(adj, gpu(seeds, torch.int32), fanouts, replace, seed))
        assert tuple(x.tolist() for x in got) == tuple(want)


# ---- row degrees around the group and the wave ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def degree_graph():
    """Rows of 0, 1, 7, 8, 9, 63, 64 and 65 entries in turn, distinct columns, plus a self loop on
    every fifth node that has entries."""
    rng = np.random.default_rng(3)
    N = 240
    degs = np.tile([0, 1, 7, 8, 9, 63, 64, 65], N // 8)
    cols = []
    for v, d in enumerate(degs):
        c = rng.choice(N, d, replace=False)
        if d and v % 5 == 0 and v not in c:
            c[0] = v
        cols.append(c)
    return sorted_csr(np.repeat(np.arange(N), degs), np.concatenate(cols).astype(np.int64), N)


@pytest.mark.parametrize("replace", [False, True])
def test_fanout_lists_on_every_row_degree(replace):
    rowptr, col = degree_graph()
    assert sorted(set(np.diff(rowptr).tolist())) == [0, 1, 7, 8, 9, 63, 64, 65]
    adj = adj_of(rowptr, col)
    seeds = np.concatenate([np.arange(16), [5, 5, 239, 0]])  # every degree twice, a seed three times, an isolated one
    for fanouts in FANOUTS:
        for seed in (5, BIG_SEED):
            got = check(rowptr, col, seeds, fanouts, replace, seed, adj=adj)
            if not fanouts or fanouts == [2, 0, 5]:
                first = check(rowptr, col, seeds, fanouts[:1], replace, seed, adj=adj)
                assert_same(got, first, "a zero fan-out ends the sampling")
    n_id, ptr = check(rowptr, col, seeds, [], replace, 1, adj=adj)[:2]
    assert n_id.tolist() == seeds.tolist() and ptr.tolist() == list(range(len(seeds) + 1))


def test_floyd_in_registers_and_outside():
    """Rows of 40 entries: [32] is the largest fan-out whose Floyd picks stay in registers, [33]
    the first that walks in memory; [33, 2] expands 33 children per seed."""
    rng = np.random.default_rng(4)
    N = 120
    col = np.concatenate([np.sort(rng.choice(N, 40, replace=False)) for _ in range(N)]).astype(np.int64)
    rowptr = np.arange(N + 1, dtype=np.int64) * 40
    adj = adj_of(rowptr, col)
    seeds = np.arange(0, N, 7)
    for fanouts in ([32], [33], [33, 2], [1, 33], [39], [40], [41]):
        for seed in (1, BIG_SEED):
            got = check(rowptr, col, seeds, fanouts, False, seed, adj=adj)
        assert np.all(np.diff(got[1]) >= min(fanouts[0], 40) // 2), fanouts
    check(rowptr, col, seeds, [33], True, 2, adj=adj)


# ---- both probe directions, both lane counts, the tie, stored duplicates ---------------------------------
H, A, B, Z = 10, 20, 30, 40


@functools.lru_cache(maxsize=None)
def probe_graph():
    """N = 6000.  H has 5000 entries: A three times, B, H itself and distinct others.  A = [H, B];
    B = [A, A, B] (3 entries).  Z has 3000 entries: A twice, H and 2997 distinct others.  The rest
    have 0 .. 5 entries, duplicates allowed.  So with fan-out -1:
      seed A   ego {H, A, B}, 3 nodes: row H (5000) is probed BY the list, 8 lanes, and the run of
               three A's comes out; row B has deg == n_g == 3, the tie: the row probes, with its
               duplicate; row A probes
      seed Z   ego of 3000 nodes = Z's 3000 entries: deg == n_g, the tie on a whole wave, the row
               probes with its duplicate; row H (5000 > 3000) is probed by the list on a whole wave
      seed H   ego of 4998 nodes < 5000 entries: the list probes on a whole wave, duplicates in the row"""
    rng = np.random.default_rng(6)
    N = 6000
    others = np.arange(100, N)
    rows = {
        H: np.concatenate([[A, A, A, B, H], rng.choice(others, 4995, replace=False)]),
        A: np.array([H, B]),
        B: np.array([A, A, B]),
        Z: np.concatenate([[A, A, H], rng.choice(others, 2997, replace=False)]),
    }
    row, col = [], []
    for v in range(N):
        c = rows[v] if v in rows else rng.integers(0, N, rng.integers(0, 6))
        row.append(np.full(len(c), v))
        col.append(c)
    return sorted_csr(np.concatenate(row), np.concatenate(col).astype(np.int64), N)


PROBE_SEEDS = (A, Z, H, A, 5999, B)


@functools.lru_cache(maxsize=None)
def probe_reference(fanouts):
    rowptr, col = probe_graph()
    return ego_k_hop_sample_ref(rowptr, col, PROBE_SEEDS, list(fanouts))


def test_probe_directions_lane_counts_tie_and_stored_duplicates():
    rowptr, col = probe_graph()
    deg = np.diff(rowptr)
    assert deg[H] == 5000 and deg[Z] == 3000 and deg[B] == 3
    n_id, ptr, root, p, c, e = check(rowptr, col, PROBE_SEEDS, [-1], want=probe_reference((-1,)))
    sizes = np.diff(ptr)
    assert sizes[0] == 3 and sizes[1] == 3000 == deg[Z] and sizes[2] == 4998 < deg[H] and sizes[3] == 3
    assert n_id[ptr[0]:ptr[1]].tolist() == [H, A, B] and deg[B] == sizes[0]  # the tie
    counts = np.diff(p)
    assert counts[0] == 5 and e[p[0]:p[1]].tolist() == list(range(rowptr[H], rowptr[H] + 5))  # A, A, A, B, H in a row
    assert c[p[0]:p[1]].tolist() == [0, 1, 1, 1, 2]
    z_row = ptr[1] + int(np.searchsorted(n_id[ptr[1]:ptr[2]], Z))
    assert n_id[z_row] == Z and counts[z_row] == 3000  # every entry of Z's row lies in its ego
    h_row = ptr[1] + int(np.searchsorted(n_id[ptr[1]:ptr[2]], H))
    assert n_id[h_row] == H and 5 <= counts[h_row] < 5000  # the list's 3000 nodes probed H's row


def test_probe_graph_deeper_fanouts():
    rowptr, col = probe_graph()
    check(rowptr, col, PROBE_SEEDS, [-1, 2], seed=3)
    check(rowptr, col, PROBE_SEEDS, [4, -1], replace=True, seed=BIG_SEED)


def test_every_threshold_gives_the_same_bits():
    """T moves rows between the 8-lane and the 64-lane pass; the result may not notice."""
    from paddle_sparse_amd import ops

    rowptr, col = probe_graph()
    adj = adj_of(rowptr, col)
    old = ops.ego_set_threshold(32)
    try:
        for T in (1, 2, 3, 8, 64, 2999, 3000, 10**6):
            ops.ego_set_threshold(T)
            check(rowptr, col, PROBE_SEEDS, [-1], adj=adj, want=probe_reference((-1,)))
    finally:
        assert ops.ego_set_threshold(old) == 10**6


def test_hub_row_and_many_egos():
    """The 70 000-entry row of graph("hub"), as a seed and as a neighbour, among 300 egos."""
    rowptr, col = graph("hub")
    N = len(rowptr) - 1
    seeds = np.concatenate([[17, 17], np.random.default_rng(2).integers(0, N, 298)])
    check(rowptr, col, seeds, [-1], seed=1)
    check(rowptr, col, seeds, [5, 3], seed=2)
    check(rowptr, col, seeds, [5, 3], replace=True, seed=2)


# ---- segment isolation -----------------------------------------------------------------------------------------
def test_a_search_never_leaves_its_egos_segment():
    """Ego 0 = {5, 6}, ego 1 = {7, 8}, ego 2 = {5, 9}, neighbours in n_id.  Row 6 holds 7, the first
    node of ego 1's list, right behind ego 0's: a lower bound that ran past the segment's end would
    find it; and 9, a node of ego 2.  Row 7 holds 5 and 6, the nodes of ego 0's list in front of its
    own, and 9.  Row 5 of ego 2 holds 6, which ego 0 has.  None of them may be emitted."""
    N = 12
    rows = {5: [6], 6: [7, 9], 7: [5, 6, 9], 8: [7, 8], 9: [5]}
    row = np.concatenate([np.full(len(c), v) for v, c in rows.items()])
    col = np.concatenate([np.array(c) for c in rows.values()])
    rowptr, col = sorted_csr(row, col, N)
    n_id, ptr, root, p, c, e = check(rowptr, col, [5, 8, 9], [-1])
    assert n_id.tolist() == [5, 6, 7, 8, 5, 9] and ptr.tolist() == [0, 2, 4, 6] and root.tolist() == [0, 3, 5]
    assert np.diff(p).tolist() == [1, 0, 0, 2, 0, 1] and c.tolist() == [1, 2, 3, 4]
    for g in range(3):
        inside = c[p[ptr[g]]:p[ptr[g + 1]]]
        assert np.all((inside >= ptr[g]) & (inside < ptr[g + 1]))


# ---- a seed listed twice ---------------------------------------------------------------------------------------
def test_a_seed_listed_twice_is_two_egos():
    rowptr, col = graph("uniform")
    adj = adj_of(rowptr, col)
    n_id, ptr, *_ = check(rowptr, col, [9, 9, 9, 9], [3, 3], True, 5, adj=adj)
    egos = [n_id[ptr[g]:ptr[g + 1]].tolist() for g in range(4)]
    assert any(egos[0] != other for other in egos[1:])  # streams differ
    n_id, ptr, root, p, c, e = check(rowptr, col, [9, 9], [-1, -1], adj=adj)
    half = ptr[1]
    assert np.array_equal(n_id[:half], n_id[half:]) and np.array_equal(c[:p[half]] + half, c[p[half]:])
    assert np.array_equal(e[:p[half]], e[p[half]:]) and root[1] - root[0] == half


def test_self_loops_isolated_seeds_and_repeated_entries():
    rowptr, col = graph("loops_multi_isolated")
    seeds = np.concatenate([np.arange(0, 60), [300, 301, 499]])  # nodes from 250 on have no entries
    for fanouts in ([3, 2], [-1, -1], [2, -1]):
        for replace in (False, True):
            n_id, ptr, root, p, _, _ = check(rowptr, col, seeds, fanouts, replace, 8)
            assert np.diff(ptr)[-3:].tolist() == [1, 1, 1] and np.all(np.diff(p)[-3:] == 0)
    check(np.zeros(11, np.int64), np.zeros(0, np.int64), [3, 1, 3], [2, -1])  # a matrix without entries
    check(np.arange(51), np.arange(50), [7, 3, 49, 7], [2, 2])               # self loops only


# ---- empty inputs ---------------------------------------------------------------------------------------------
def test_no_seeds():
    rowptr, col = graph("uniform")
    for fanouts in ([3, 2], [-1], []):
        got = check(rowptr, col, np.zeros(0, np.int64), fanouts)
        assert got[1].tolist() == [0] and got[3].tolist() == [0] and all(got[i].size == 0 for i in (0, 2, 4, 5))


# ---- keys past 32 bits ------------------------------------------------------------------------------------------
def test_keys_past_32_bits():
    """N = 2^20 and 4096 egos: the keys ego * N + node reach 2^32.  Most seeds are nodes without
    entries; the last egos, whose keys are the largest, have neighbourhoods."""
    rng = np.random.default_rng(12)
    N, S = 2**20, 4096
    busy = rng.choice(N, 400, replace=False)
    row = np.repeat(busy, 8)
    col = rng.choice(busy, len(row))
    col[::5] = rng.integers(0, N, len(col[::5]))  # and some columns that lead nowhere
    rowptr, col = sorted_csr(row, col, N)
    assert len(col) == 3200
    seeds = rng.integers(0, N, S)
    seeds[-64:] = busy[:64]
    seeds[0], seeds[1] = N - 1, busy[0]
    assert (S - 1) * N + int(seeds[-1]) >= 2**32 - N
    got = check(rowptr, col, seeds, [3, 2], seed=7)
    assert np.diff(got[1])[-64:].min() > 1 and got[0].max() <= N - 1
    check(rowptr, col, seeds, [-1, -1])


# ---- host reads -----------------------------------------------------------------------------------------------
def test_host_reads_follow_the_formula_whatever_S():
    """2 + the number of hops with k < 0 that run: the node count (with the sort's fault word) and
    nnz' (with the flags), plus the slot count of every -1 hop.  Conditions of the design."""
    from paddle_sparse_amd import ops

    rowptr, col = graph("uniform")
    busy = np.flatnonzero(np.diff(rowptr) >= 3)  # so that every hop has slots
    rowptr, col = gpu(rowptr), gpu(col)
    for fanouts in FANOUTS + ([33], [32], [-1, -1, -1]):
        run = fanouts[:fanouts.index(0)] if 0 in fanouts else fanouts
        want = 2 + sum(k < 0 for k in run)
        assert want <= 3 + sum(k < 0 for k in fanouts)
        for S in (1, 300):
            stats = {}
            seeds = gpu(busy[np.random.default_rng(S).integers(0, len(busy), S)])
            ops.ego_k_hop_sample(rowptr, col, seeds, fanouts, False, 1, stats=stats)
            assert stats["host_reads"] == want and stats["hops_run"] == len(run), (fanouts, S)
        ops.ego_k_hop_sample(rowptr, col, gpu([]), fanouts, False, 1, stats=stats)
        assert stats["host_reads"] == 0 and stats["hops_run"] == 0, fanouts


# ---- errors ---------------------------------------------------------------------------------------------------
def test_errors():
    rowptr, col = graph("uniform")
    adj = adj_of(rowptr, col)
    N = len(rowptr) - 1
    for bad in (-1, N, 2**40):
        for fanouts in ([2], [-1], [], [2, -1]):
            with pytest.raises(IndexError):
                adj.ego_k_hop_sample(gpu([5, bad, 7]), fanouts)
    with pytest.raises(ValueError, match="square"):
        adj_of(rowptr, col, N=N + 1).ego_k_hop_sample(gpu([1]), [2])
    with pytest.raises(TypeError):
        adj.ego_k_hop_sample(gpu([1.0], torch.float32), [2])
    with pytest.raises(ValueError):
        adj.ego_k_hop_sample(gpu([[1, 2]]), [2])
    with pytest.raises(ValueError):
        adj.ego_k_hop_sample(gpu([1]), [2, -2])
    check(rowptr, col, [5, 7], [2], seed=1, adj=adj)  # and the next call is sound


def test_the_slot_limit_is_refused_before_anything_is_allocated():
    rowptr, col = graph("uniform")
    adj = adj_of(rowptr, col)
    seeds = gpu(np.arange(300))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    for fanouts in ([3000, 3000], [10, 10, 10, 10, 10, 10, 10], [2**31], [40000, 200, -1]):
        with pytest.raises(ValueError, match=r"hop \d+ has \d+ slots"):
            adj.ego_k_hop_sample(seeds, fanouts, seed=1)
    assert torch.cuda.max_memory_allocated() == before
    with pytest.raises(ValueError, match="walk list"):  # every hop fits, their sum does not
        adj.ego_k_hop_sample(seeds, [3_000_000, 1, 1], seed=1)
    assert torch.cuda.max_memory_allocated() == before


# ---- values and their gradient -----------------------------------------------------------------------------------
def test_values_are_gathered_by_e_id():
    rowptr, col = graph("loops_multi_isolated")
    seeds = gpu(np.arange(0, 64))
    for dtype, width in ((torch.float64, None), (torch.float32, None), (torch.int64, None), (torch.float32, 3)):
        shape = (len(col),) if width is None else (len(col), width)
        value = torch.randint(-50, 50, shape, device="cuda").to(dtype)
        adj = adj_of(rowptr, col, value)
        for fanouts, replace in (([4, 3], False), ([2, 2], True), ([-1], False)):
            sub, _, e_id, _, _ = adj.ego_k_hop_sample(seeds, fanouts, replace=replace, seed=1)
            got = sub.storage.value()
            assert got.dtype == dtype and got.shape[1:] == value.shape[1:] and e_id.numel() > 0
            assert torch.equal(got, value[e_id]), (dtype, width, fanouts)


def test_value_gradient_is_exact_and_repeatable():
    """Integer-valued fp64 data: every sum is exact, so the gradient equals index_add over e_id
    bit for bit; one edge sits in several egos, so the sums have work to do."""
    rowptr, col = graph("loops_multi_isolated")
    g = torch.Generator(device="cuda").manual_seed(3)
    value = torch.randint(-8, 9, (len(col),), generator=g, device="cuda").double()
    seeds = gpu(np.concatenate([np.arange(0, 64), np.arange(0, 64)]))
    grads, outs = [], []
    for _ in range(2):
        v = value.clone().requires_grad_()
        sub, n_id, e_id, ptr, root = adj_of(rowptr, col, v).ego_k_hop_sample(seeds, [4, 3], seed=1)
        weight = torch.randint(-8, 9, (e_id.numel(),), generator=torch.Generator(device="cuda").manual_seed(4),
                               device="cuda").double()
        (sub.storage.value() * weight).sum().backward()
        grads.append(v.grad)
        outs.append((n_id, e_id, ptr, root, sub.storage.rowptr(), sub.storage.col(), sub.storage.value().detach()))
    assert torch.equal(grads[0], grads[1])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    assert torch.unique(e_id).numel() < e_id.numel()
    want = torch.zeros_like(value).index_add_(0, e_id, weight)
    assert torch.equal(grads[0], want) and bool(grads[0].abs().sum() > 0)


# ---- the result and the source -------------------------------------------------------------------------------------
def test_the_result_is_a_sound_storage_and_the_source_is_untouched():
    from storage_ref import derived

    rowptr, col = graph("loops_multi_isolated")
    value = torch.arange(len(col), dtype=torch.float32, device="cuda")
    adj = adj_of(rowptr, col, value)
    adj.fill_cache_()
    st = adj.storage
    names = ("_row", "_rowptr", "_col", "_value", "_rowcount", "_colptr", "_colcount", "_csr2csc", "_csc2csr")
    before = {k: (getattr(st, k), getattr(st, k).clone()) for k in names if getattr(st, k, None) is not None}
    assert {"_rowptr", "_col", "_value", "_colptr", "_csr2csc"} <= set(before)
    sub, n_id, e_id, ptr, root = adj.ego_k_hop_sample(gpu(np.arange(0, 80)), [3, -1], seed=4)
    for k, (obj, copy) in before.items():
        assert getattr(st, k) is obj and torch.equal(obj, copy), k
    n = n_id.numel()
    sst = sub.storage
    row = np.repeat(np.arange(n), np.diff(sst.rowptr().cpu().numpy()))
    d = derived(row, sst.col().cpu().numpy(), n, n)
    assert d.sorted and d.nnz == e_id.numel() > 0
    for got, want in ((sst.rowptr(), d.rowptr), (sst.row(), d.row), (sst.rowcount(), d.rowcount),
                      (sst.colptr(), d.colptr), (sst.colcount(), d.colcount), (sst.csr2csc(), d.csr2csc),
                      (sst.csc2csr(), d.csc2csr)):
        assert np.array_equal(got.cpu().numpy(), want)
    # block-diagonal: an entry never leaves its ego
    ego_of = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr.cpu().numpy()))
    assert np.array_equal(ego_of[d.row], ego_of[d.col])
    # and it multiplies: the root rows of sub @ x are the egos' aggregates
    x = torch.ones(n, 2, device="cuda")
    out = sub @ x
    assert torch.equal(out[:, 0], torch.from_numpy(np.bincount(d.row, weights=value[e_id].cpu().numpy(),
                                                                minlength=n)).float().cuda())


# ---- determinism ---------------------------------------------------------------------------------------------------
def test_a_second_stream_returns_the_same_bits():
    rowptr, col = graph("uniform")
    adj = adj_of(rowptr, col)
    seeds = gpu(np.random.default_rng(1).integers(0, 3000, 257))
    for fanouts, replace in (([5, 3], False), ([-1, 2], True)):
        first, _ = unpack(adj.ego_k_hop_sample(seeds, fanouts, replace=replace, seed=BIG_SEED))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            second, _ = unpack(adj.ego_k_hop_sample(seeds, fanouts, replace=replace, seed=BIG_SEED))
        side.synchronize()
        assert_same(second, first, ("second stream", fanouts))
        other, _ = unpack(adj.ego_k_hop_sample(seeds, fanouts, replace=replace, seed=BIG_SEED + 1))
        assert not all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(other, first))


def test_seed_none_draws_from_torchs_cpu_generator():
    rowptr, col = graph("uniform")
    adj = adj_of(rowptr, col)
    seeds = gpu(np.arange(100))
    torch.manual_seed(5)
    a, _ = unpack(adj.ego_k_hop_sample(seeds, [3, 2]))
    torch.manual_seed(5)
    b, _ = unpack(adj.ego_k_hop_sample(seeds, [3, 2]))
    assert_same(a, b, "same generator state")
    torch.manual_seed(5)
    s = int(torch.randint(0, 2**62, (1,)).item())
    assert_same(a, ego_k_hop_sample_ref(rowptr, col, np.arange(100), [3, 2], False, s), "the drawn seed")
