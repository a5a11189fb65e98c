"""GPU suite for weighted neighbor_sample.  Index work: every comparison is
bit-exact against the serial restatement of tests/weighted_neighbor_ref.py (pinned, with the
host export of the pick, by test_zz_weighted_neighbor_ref.py).  Shapes are the smallest that
reach each kernel: the walks in registers for up to 8, 16 and 32 draws, the walk in memory
beyond, the slot kernel with replacement."""
import functools

import numpy as np
import pytest
import torch

import neighbor_ref
import weighted_neighbor_ref as nr
import weighted_ref as wr
from test_neighbor_sample_gpu import BIG_SEED, GRAPHS, assert_same, graph, seeds_of, unpack
from test_walk_saint_gpu import adj_of, gpu

pytestmark = pytest.mark.gpu


def f64(x):
    return torch.as_tensor(np.asarray(x, np.float64)).cuda()


class Case:
    """A graph with float64 weights: the numpy form, the restated cum, the matrix and its EdgeCDF."""

    def __init__(self, rowptr, col, w):
        import paddle_sparse_amd as psa

        self.rowptr, self.col, self.w = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(w, np.float64)
        self.cum = wr.row_cdf(self.rowptr, self.w)
        self.adj = adj_of(self.rowptr, self.col, f64(self.w))
        self.cdf = psa.EdgeCDF(self.adj)
        assert np.array_equal(self.cdf.cum.cpu().numpy().view(np.int64), self.cum.view(np.int64))  # the same bits
        self.N = len(self.rowptr) - 1

    def ref(self, seeds, fanouts, replace=False, seed=0):
        return nr.neighbor_sample_ref(self.rowptr, self.col, self.cum, seeds, list(fanouts), replace, seed)

    def run(self, seeds, fanouts, replace=False, seed=0, **kw):
        return unpack(self.adj.neighbor_sample(gpu(seeds), list(fanouts), replace=replace, seed=seed,
                                               weighted=self.cdf, **kw))

    def check(self, seeds, fanouts, replace=False, seed=0):
        (got, sub), want = self.run(seeds, fanouts, replace, seed), self.ref(seeds, fanouts, replace, seed)
        assert_same(got, want, (fanouts, replace, seed))
        assert np.array_equal(sub.storage.value().cpu().numpy(), self.w[want[3]])  # the values, gathered by e_id
        if all(k >= 0 for k in fanouts):
            assert np.all(self.w[want[3]] > 0)
        return got


@functools.lru_cache(maxsize=None)
def weighted_case(name):
    """A graph of test_neighbor_sample_gpu.py with random float64 weights, 30 % of them zero."""
    rowptr, col = graph(name)
    rng = np.random.default_rng(23)
    w = rng.random(len(col))
    w[rng.random(len(col)) < 0.3] = 0.0
    return Case(rowptr, col, w)


# ---- the restatement grid --------------------------------------------------------------------------
FANOUTS = [(3,), (5, 3), (4, 2, 2), (-1, 3)]


@pytest.mark.parametrize("name", GRAPHS)
def test_grid_matches_the_restatement(name):
    """All six outputs, four fan-out shapes, both replace settings, two seeds (one above 2^63),
    257 seeds with the hub's id first."""
    case = weighted_case(name)
    seeds = seeds_of(name, 257)
    for fanouts in FANOUTS:
        for replace in (False, True):
            for seed in (5, BIG_SEED):
                case.check(seeds, fanouts, replace, seed)


# ---- degree boundaries -------------------------------------------------------------------------------
KS = [1, 2, 31, 32, 33, 40]


@functools.lru_cache(maxsize=None)
def stars(k):
    """Stars with leaves of their own, one per (degree, weights): degrees k - 1, k, k + 1, 2 k;
    every weight positive, or P = 0, 1, k - 1 positive among zeros.  Centres first; no leaf is
    shared, so new local ids are handed out in slot order and a row's entries of the result
    stand in draw order."""
    rng = np.random.default_rng(100 + k)
    rows = []
    for deg in (k - 1, k, k + 1, 2 * k):
        for P in (None, 0, 1, k - 1):
            w = rng.random(deg) + 0.25
            if P is not None:
                keep = rng.choice(deg, size=min(P, deg), replace=False)
                z = np.zeros(deg)
                z[keep] = w[keep]
                w = z
            rows.append(w)
    C = len(rows)
    total = sum(len(w) for w in rows)
    rowptr = np.zeros(C + total + 1, np.int64)
    rowptr[1:C + 1] = np.cumsum([len(w) for w in rows])
    rowptr[C + 1:] = total
    return Case(rowptr, C + np.arange(total, dtype=np.int64), np.concatenate(rows) if total else np.zeros(0)), C


@pytest.mark.parametrize("k", KS)
def test_degree_boundaries_on_stars(k):
    from paddle_sparse_amd import ops

    case, C = stars(k)
    seeds = np.arange(C)
    got = case.check(seeds, [k])
    n_id, rowptr, col, e_id, nodes, edges = got
    for i in range(C):
        s, deg = case.rowptr[i], case.rowptr[i + 1] - case.rowptr[i]
        P = int((case.w[s:s + deg] > 0).sum())
        picks = e_id[rowptr[i]:rowptr[i + 1]] - s
        assert len(picks) == min(k, P) and len(set(picks.tolist())) == len(picks), (k, deg, P)
        # the host export, fed with the words of the row's stream: the same picks in the same order
        words = nr.stream_words(0, i, k)
        assert picks.tolist() == ops.weighted_pick_without_host(case.cum[s:s + deg], k, *words), (k, deg, P)
    assert edges == [sum(min(k, int((case.w[case.rowptr[i]:case.rowptr[i + 1]] > 0).sum())) for i in range(C))]
    case.check(seeds, [k], replace=True, seed=3)


def test_slot_zero_in_draw_order_is_the_weighted_walks_step():
    case, C = stars(32)
    seeds = np.arange(C)
    (n_id, rowptr, col, e_id, _, _), _ = case.run(seeds, [32], seed=77)
    _, e_walk = case.adj.random_walk(gpu(seeds), 1, seed=77, weighted=case.cdf, return_edge_ids=True)
    e_walk = e_walk[:, 0].cpu().numpy()
    for i in range(C):
        assert (e_id[rowptr[i]] if rowptr[i + 1] > rowptr[i] else -1) == e_walk[i]


# ---- a dominating weight ---------------------------------------------------------------------------------
def dominated(R, D, N, lowest, rng):
    """R rows of D entries, one weight of 1e18 among ones, at a position >= lowest."""
    col = np.concatenate([np.sort(rng.choice(N, D, replace=False)) for _ in range(R)])
    rowptr = np.concatenate([np.arange(R + 1) * D, np.full(N - R, R * D)]).astype(np.int64)
    w = np.ones(R * D)
    heavy = np.arange(R) * D + rng.integers(lowest, D, R)
    w[heavy] = 1e18
    return Case(rowptr, col, w), heavy


def test_one_dominating_weight_per_row():
    """300 rows of 64 entries, one weight of 1e18 among 63 ones, k = 8: rejection would spin;
    here every row returns 8 distinct entries, the heavy one among them.  The heavy entry
    stands behind at least 7 ones: float64 prefix sums absorb a 1 added to 1e18, so the
    entries BEHIND the heavy one weigh nothing in the row CDF (a limit of EdgeCDF, DESIGN
    3.17, that the picks inherit: see the next test)."""
    rng = np.random.default_rng(5)
    R = 300
    case, heavy = dominated(R, 64, 2400, 7, rng)
    n_id, p, c, e_id, nodes, edges = case.check(rng.permutation(R), [8], seed=12)
    assert edges == [R * 8]
    for i in range(R):
        mine = e_id[p[i]:p[i + 1]]
        assert len(set(mine.tolist())) == 8 and np.isin(mine, heavy).sum() == 1
    case.check(np.arange(R), [8, 8], seed=13)


def test_weights_the_prefix_sum_absorbs_count_as_zero():
    """The heavy entry anywhere in the row: the picks are the heavy entry and entries in front
    of it, min(8, position + 1) of them, exactly what the row's cum holds."""
    rng = np.random.default_rng(15)
    R, D = 300, 64
    case, heavy = dominated(R, D, 2400, 0, rng)
    n_id, p, c, e_id, nodes, edges = case.check(np.arange(R), [8], seed=12)
    for i in range(R):
        mine = e_id[p[i]:p[i + 1]]
        assert len(mine) == min(8, heavy[i] - i * D + 1) == min(8, nr.positive_entries(case.cum[i * D:(i + 1) * D].tolist()))
        assert heavy[i] in mine and mine.max() == heavy[i]


# ---- a long row ----------------------------------------------------------------------------------------------
def test_a_row_of_70000_entries():
    """Node 0 holds 70 000 entries, columns 1 .. 70 000, the heavy weights past position 2^16: 17
    halvings per search, picks at positions and columns past 2^16; k = 5 in registers, k = 40
    in memory, and with replacement."""
    D = 70_000
    rng = np.random.default_rng(6)
    rowptr = np.concatenate([[0], np.full(D + 1, D)]).astype(np.int64)
    w = rng.random(D) * np.where(np.arange(D) >= 2**16, 100.0, 1.0)
    w[rng.random(D) < 0.2] = 0.0
    case = Case(rowptr, np.arange(1, D + 1, dtype=np.int64), w)
    for k, replace in ((5, False), (40, False), (5, True)):
        n_id, p, c, e_id, _, _ = case.check([0], [k], replace, seed=21)
        assert len(e_id) == k and e_id.max() > 2**16 and n_id.max() > 2**16


# ---- frontier sizes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 255, 256, 257, 1000])
def test_frontier_sizes_around_the_workgroup(S):
    """One thread per frontier row, 256 per workgroup; the second hop's stream index is the
    local id, not the position in the frontier."""
    case = weighted_case("uniform")
    seeds = seeds_of("uniform", S)
    got = case.check(seeds, [4, 3], seed=BIG_SEED)
    assert got[4][1] > 0 and got[5][1] > 0  # the second hop drew
    case.check(seeds, [2, 2], replace=True, seed=8)


# ---- ties to the existing ops ------------------------------------------------------------------------------------
def test_hop_one_with_replacement_is_weighted_sample_adj():
    from paddle_sparse_amd import ops

    case = weighted_case("uniform")
    S = 300
    seeds = seeds_of("uniform", S)
    for k in (1, 4, 33):
        (n_id, p, c, e_id, nodes, edges), _ = case.run(seeds, [k], replace=True, seed=BIG_SEED)
        raw = ops.sample_adj(gpu(case.rowptr), gpu(case.col), gpu(seeds), k, True, seed=BIG_SEED, cum=case.cdf.cum)
        p1, e1 = raw[0].cpu().numpy(), raw[3].cpu().numpy()
        assert np.array_equal(p[:S + 1], p1) and np.array_equal(n_id, raw[2].cpu().numpy())
        for i in range(S):
            assert sorted(e_id[p[i]:p[i + 1]].tolist()) == sorted(e1[p1[i]:p1[i + 1]].tolist()), (k, i)


def test_draw_zero_is_step_zero_of_the_weighted_walk():
    case = weighted_case("hub")
    seeds = seeds_of("hub", 500)
    _, e_walk = case.adj.random_walk(gpu(seeds), 1, seed=321, weighted=case.cdf, return_edge_ids=True)
    e_walk = e_walk[:, 0].cpu().numpy()
    (_, p, _, e_id, _, _), _ = case.run(seeds, [1], seed=321)  # one slot per row: slot 0
    one = np.full(len(seeds), -1)
    one[np.diff(p[:len(seeds) + 1]) > 0] = e_id
    assert np.array_equal(one, e_walk) and (e_walk >= 0).sum() > 300
    (_, p, _, e_id, _, _), _ = case.run(seeds, [6], seed=321)  # the same word opens a longer walk
    for i in np.flatnonzero(e_walk >= 0):
        assert e_walk[i] in e_id[p[i]:p[i + 1]]


def test_without_weights_nothing_changes():
    case = weighted_case("loops_multi_isolated")
    seeds = seeds_of("loops_multi_isolated", 100)
    for fanouts, replace in (([5, 3], False), ([3, 3], True), ([-1, 2], False)):
        today, _ = unpack(case.adj.neighbor_sample(gpu(seeds), fanouts, replace=replace, seed=4))
        none, _ = unpack(case.adj.neighbor_sample(gpu(seeds), fanouts, replace=replace, seed=4, weighted=None))
        assert_same(none, today)
        assert_same(none, neighbor_ref.neighbor_sample_ref(case.rowptr, case.col, seeds, fanouts, replace, 4))
    # all entries whatever their weight, as weighted sample_adj with k < 0
    every, _ = unpack(case.adj.neighbor_sample(gpu(seeds), [-1], seed=4))
    got, _ = case.run(seeds, [-1], seed=4)
    assert_same(got, every)


def test_true_builds_the_cdf_and_another_matrix_is_refused():
    import paddle_sparse_amd as psa

    case = weighted_case("uniform")
    seeds = seeds_of("uniform", 64)
    want, _ = case.run(seeds, [3, 2], seed=2)
    got, _ = unpack(psa.neighbor_sample(case.adj, gpu(seeds), [3, 2], seed=2, weighted=True))
    assert_same(got, want)
    got, _ = unpack(psa.NeighborSampler(case.adj, [3, 2], weighted=True)(gpu(seeds), seed=2))
    assert_same(got, want)
    with pytest.raises(ValueError, match="another matrix"):
        weighted_case("hub").adj.neighbor_sample(gpu(seeds), [3], weighted=case.cdf)
    from paddle_sparse_amd import ops

    with pytest.raises(ValueError, match="cum"):
        ops.neighbor_sample(gpu(case.rowptr), gpu(case.col), gpu(seeds), [3], cum=case.cdf.cum[:-1])
    with pytest.raises(ValueError, match="cum lies on"):
        ops.neighbor_sample(gpu(case.rowptr), gpu(case.col), gpu(seeds), [3], cum=case.cdf.cum.cpu())


# ---- the claim race -------------------------------------------------------------------------------------------------
def test_many_rows_claim_the_same_few_columns():
    """2000 frontier rows whose entries all point at the same 6 columns: every new id is
    fought over by hundreds of slots, the smallest slot wins whatever the arrival order."""
    rng = np.random.default_rng(9)
    R, hot = 2000, np.array([2000, 2001, 2002, 2003, 2004, 2005])
    rowptr = np.concatenate([np.arange(R + 1) * 6, np.full(6, R * 6)]).astype(np.int64)
    case = Case(rowptr, np.tile(hot, R), rng.random(R * 6) * (rng.random(R * 6) > 0.2))
    seeds = rng.permutation(R)
    for replace in (False, True):
        first = case.check(seeds, [3], replace, seed=41)
        assert first[4] == [R, 6]
        for _ in range(3):
            again, _ = case.run(seeds, [3], replace, seed=41)
            assert_same(again, first)


# ---- the sampler object ------------------------------------------------------------------------------------------------
def test_a_reused_weighted_sampler_equals_fresh_calls_also_after_an_error():
    import paddle_sparse_amd as psa

    case = weighted_case("uniform")
    for fanouts, replace in (([5, 3, 2], False), ([-1, 2], False), ([3, 3], True)):
        sampler = psa.NeighborSampler(case.adj, fanouts, replace, weighted=case.cdf)
        batches = [np.random.default_rng(s).permutation(case.N)[:size] for s, size in ((1, 300), (2, 64), (3, 300))]
        for i, seeds in enumerate(batches):
            got, _ = unpack(sampler(gpu(seeds), seed=i))
            fresh, _ = case.run(seeds, fanouts, replace, seed=i)
            assert_same(got, fresh, ("reuse", i))
            if i == 0:
                assert_same(got, case.ref(seeds, fanouts, replace, i), "restatement")
        for bad, error in ((np.concatenate([batches[0], batches[0][:1]]), ValueError),
                           (np.concatenate([batches[1], [case.N]]), IndexError)):
            with pytest.raises(error):
                sampler(gpu(bad), seed=9)
            got, _ = unpack(sampler(gpu(batches[2]), seed=2))
            fresh, _ = case.run(batches[2], fanouts, replace, seed=2)
            assert_same(got, fresh, ("after", error.__name__))
        local = sampler._workspace.buf[:4 * case.N].view(torch.int32)
        assert sampler._workspace.clean and bool((local == -2**31).all())


def test_undirected_is_the_induced_subgraph_of_the_weighted_node_set():
    case = weighted_case("loops_multi_isolated")
    seeds = gpu(seeds_of("loops_multi_isolated", 60))
    for fanouts in ([4, 2], [-1, 3]):
        _, n_id, _, (nodes, _) = case.adj.neighbor_sample(seeds, fanouts, seed=6, weighted=case.cdf)
        sub, n_id2, e_id, (nodes2, edges2) = case.adj.neighbor_sample(seeds, fanouts, directed=False, seed=6,
                                                                      weighted=case.cdf)
        assert torch.equal(n_id, n_id2) and nodes == nodes2 and edges2 is None
        want, want_e = case.adj.saint_subgraph(n_id)
        assert torch.equal(e_id, want_e) and all(torch.equal(a, b) for a, b in zip(sub.csr(), want.csr()))
        _, uniform, _, _ = case.adj.neighbor_sample(seeds, fanouts, seed=6)
        assert not torch.equal(uniform, n_id)  # the weights chose other nodes


# ---- values and their gradient ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("replace", [False, True])
def test_values_follow_e_id_and_the_gradient_is_exact(replace):
    import paddle_sparse_amd as psa

    case = weighted_case("uniform")
    seeds = gpu(seeds_of("uniform", 200))
    grads = []
    for _ in range(2):
        v = f64(case.w).requires_grad_()
        adj = adj_of(case.rowptr, case.col, v)
        sub, n_id, e_id, _ = adj.neighbor_sample(seeds, [4, 3], replace=replace, seed=1, weighted=psa.EdgeCDF(adj))
        picked = sub.storage.value()
        assert torch.equal(picked.detach(), v.detach()[e_id])
        g = torch.arange(1, picked.numel() + 1, dtype=torch.float64, device="cuda")  # integers: any order adds exactly
        picked.backward(g)
        assert torch.equal(v.grad, torch.zeros_like(v).index_add_(0, e_id, g))
        grads.append(v.grad)
    assert torch.equal(grads[0], grads[1]) and bool(grads[0].abs().sum() > 0)
    want = case.ref(seeds.cpu().numpy(), [4, 3], replace, 1)
    assert np.array_equal(e_id.cpu().numpy(), want[3])
    if not replace:
        assert len(set(want[3].tolist())) == len(want[3])  # every entry at most once: the backward is a scatter
