"""GPU suite for neighbor_sample.  The op is index work, so every comparison is bit-exact
against the serial restatement of tests/neighbor_ref.py (pinned by test_neighbor_ref.py);
the loader-size case checks vectorised properties instead."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from neighbor_ref import neighbor_sample_ref
from test_neighbor_ref import KAT_NEIGHBOR
from test_walk_saint import ref_saint_subgraph
from test_walk_saint_gpu import adj_of, gpu, kat_adj, sorted_csr
from test_walk_saint_gpu import graph as _graph
from util import random_csr

pytestmark = pytest.mark.gpu

GRAPHS = ["uniform", "hub", "loops_multi_isolated"]
HUB = 17  # the 70 000-entry row of graph("hub")
BIG_SEED = 2**63 + 11


@functools.lru_cache(maxsize=None)
def graph(name):
    return _graph(name)


@functools.lru_cache(maxsize=None)
def reference(name, S, fanouts, replace, seed):
    rowptr, col = graph(name)
    return neighbor_sample_ref(rowptr, col, seeds_of(name, S), list(fanouts), replace, seed)


def seeds_of(name, S):
    """S distinct nodes, the hub's id first."""
    N = len(graph(name)[0]) - 1
    perm = np.random.default_rng(11).permutation(N)
    return np.concatenate([[HUB], perm[perm != HUB]])[:S].astype(np.int64)


def unpack(res):
    sub, n_id, e_id, (nodes, edges) = res
    st = sub.storage
    return (n_id.cpu().numpy(), st.rowptr().cpu().numpy(), st.col().cpu().numpy(), e_id.cpu().numpy(), nodes, edges), sub


def assert_same(got, want, what=""):
    for g, w, name in zip(got, want, ("n_id", "rowptr", "col", "e_id", "nodes_per_hop", "edges_per_hop")):
        if isinstance(w, np.ndarray):
            assert g.dtype == np.int64 and np.array_equal(g, w), (what, name)
        else:
            assert list(g) == list(w), (what, name)


def check(rowptr, col, seeds, fanouts, replace=False, seed=0, adj=None):
    adj = adj_of(rowptr, col) if adj is None else adj
    got, sub = unpack(adj.neighbor_sample(gpu(seeds), fanouts, replace=replace, seed=seed))
    want = neighbor_sample_ref(rowptr, col, seeds, fanouts, replace, seed)
    assert_same(got, want, (fanouts, replace, seed))
    n = len(want[0])
    assert sub.sparse_sizes() == (n, n) and not sub.has_value()
    return got


# ---- known answers ------------------------------------------------------------------------------
def test_known_answers_functions_methods_and_int32_seeds():
    import paddle_sparse_amd as psa

    adj = kat_adj()
    for (seeds, fanouts, replace, seed), want in KAT_NEIGHBOR:
        got, _ = unpack(adj.neighbor_sample(gpu(seeds), fanouts, replace=replace, seed=seed))
        assert tuple(np.asarray(x).tolist() for x in got) == tuple(want)
    (seeds, fanouts, replace, seed), want = KAT_NEIGHBOR[1]
    got, _ = unpack(psa.neighbor_sample(adj, gpu(seeds, torch.int32), fanouts, replace, True, seed))
    assert tuple(np.asarray(x).tolist() for x in got) == tuple(want)
    got, _ = unpack(psa.NeighborSampler(adj, fanouts, replace)(gpu(seeds), seed=seed))
    assert tuple(np.asarray(x).tolist() for x in got) == tuple(want)


# ---- one hop is sample_adj ------------------------------------------------------------------------
def test_one_hop_equals_sample_adj():
    from paddle_sparse_amd import ops

    rowptr, col = graph("uniform")
    S = 257
    seeds = gpu(seeds_of("uniform", S))
    adj = adj_of(rowptr, col)
    for k, replace in ((3, False), (3, True), (-1, False), (30, True)):
        sub, n_id, e_id, (nodes, edges) = adj.neighbor_sample(seeds, [k], replace=replace, seed=BIG_SEED)
        one, n_id1 = adj.sample_adj(seeds, k, replace=replace, seed=BIG_SEED)
        p1, c1, _ = one.csr()
        p, c, _ = sub.csr()
        assert torch.equal(n_id, n_id1) and torch.equal(c, c1) and torch.equal(p[:S + 1], p1), (k, replace)
        assert int(p[-1]) == int(p1[-1]) == edges[0] and nodes == [S, n_id.numel() - S], (k, replace)
        # sample_adj's e_id, through the oracle-checked raw op
        raw = ops.sample_adj(gpu(rowptr), gpu(col), seeds, k, replace, seed=BIG_SEED, num_cols=3000)
        assert torch.equal(e_id, raw[3]), (k, replace)


# ---- grid and tile edges ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
def test_grid_matches_the_restatement(name):
    """S around the workgroup size, the three fan-out shapes, both replace settings, two
    seeds (one at or above 2^63), the hub's id first among the seeds: 48 calls per graph."""
    rowptr, col = graph(name)
    adj = adj_of(rowptr, col)
    for S in (1, 255, 256, 257):
        seeds = gpu(seeds_of(name, S))
        for fanouts in ((5, 3, 2), (-1, 2), (3, -1)):
            for replace in (False, True):
                for seed in (5, BIG_SEED):
                    got, _ = unpack(adj.neighbor_sample(seeds, list(fanouts), replace=replace, seed=seed))
                    assert_same(got, reference(name, S, fanouts, replace, seed), (name, S, fanouts, replace, seed))
    if name == "hub":  # hop 1 with fan-out -1 held the hub's 70 000 entries: 68 tiles of 1024 slots that find one row
        assert rowptr[HUB + 1] - rowptr[HUB] == 70_000 and reference("hub", 257, (-1, 2), False, 5)[5][0] > 70_000


def rows_per_tile(deg, tile=1024):
    """Frontier rows that each tile of `tile` slots spans (first to last row with a slot in it),
    as neighbor_pick_all_kernel counts them, from the frontier's degrees."""
    ptr = np.concatenate([[0], np.cumsum(deg)])
    out = []
    for p0 in range(0, int(ptr[-1]), tile):
        p1 = min(p0 + tile, int(ptr[-1]))
        out.append(int(np.searchsorted(ptr, p1 - 1, side="right") - np.searchsorted(ptr, p0, side="right")) + 1)
    return out


def test_tiles_that_span_more_rows_than_the_stage_holds():
    """Fan-out -1 over a frontier of mostly one-entry nodes with long runs of nodes without
    entries: a tile of 1024 slots then spans more than the 512 rows staged in LDS and
    searches the scanned degrees in global memory.  Seeds, in order: 1024 one-entry nodes (tile
    0, one row per slot), 600 empty (tile 1 starts right behind the run), 500 one-entry, 700
    empty (a run inside tile 1), 524 one-entry (tile 1 ends with them), 10 empty, 300 nodes of
    3 entries (a staged tile behind the others).  Their targets have one entry or none in
    turn, so hop 2 of [-1, -1] is a tile of the same kind."""
    rng = np.random.default_rng(17)
    segments = [(1024, 1), (600, 0), (500, 1), (700, 0), (524, 1), (10, 0), (300, 3)]
    seed_deg = np.concatenate([np.full(n, d) for n, d in segments])
    S, T = len(seed_deg), 2400
    N = S + T
    target_deg = (np.arange(T) % 3 != 0).astype(np.int64)  # a third of the targets has no entry
    deg = np.concatenate([seed_deg, target_deg])
    row = np.repeat(np.arange(N), deg)
    col = np.concatenate([S + rng.integers(0, T, int(seed_deg.sum())),  # seeds point at targets
                          rng.integers(0, N, int(target_deg.sum()))])   # targets point anywhere
    rowptr, col = sorted_csr(row, col, N)
    relabel = rng.permutation(N)  # the node ids carry no order
    inv = np.argsort(relabel)
    rowptr2, col2 = sorted_csr(relabel[np.repeat(np.arange(N), np.diff(rowptr))], relabel[col], N)
    seeds = relabel[np.arange(S)]
    tiles = rows_per_tile(np.diff(rowptr2)[seeds])
    assert tiles[0] == 1024 and tiles[1] == 1724 and tiles[2] <= 512 and len(tiles) == 3
    adj = adj_of(rowptr2, col2)
    for fanouts in ([-1], [-1, -1], [-1, -1, 2]):
        for replace in (False, True):
            got = check(rowptr2, col2, seeds, fanouts, replace, 9, adj=adj)
    hop2 = got[0][S:S + got[4][1]]
    assert max(rows_per_tile(np.diff(rowptr2)[hop2])) > 512 and inv[hop2].min() >= S


# ---- Floyd boundary -----------------------------------------------------------------------------------
def test_floyd_boundary_degrees():
    for k in (1, 2, 8, 32, 33):
        floyd_boundary(k)


def floyd_boundary(k):
    """Rows with deg in k - 1, k, k + 1, k + 2 and 0: at deg = k + 1 the walk's last step
    draws from k values of which k - 1 are taken.  Between k = 32 and 33 the walk changes
    kernels (up to 32 picks stay in registers, more go through memory)."""
    rng = np.random.default_rng(k)
    N = 300
    degs = np.repeat([0, max(k - 1, 0), k, k + 1, k + 2], N // 5)
    rng.shuffle(degs)
    row = np.repeat(np.arange(N), degs)
    col = np.concatenate([rng.choice(N, d, replace=False) for d in degs]).astype(np.int64)
    rowptr, col = sorted_csr(row, col, N)
    seeds = np.arange(0, N, 2)  # hop 2 walks the other half
    for fanouts in ([k], [k, k]):
        for seed in (1, BIG_SEED):
            got = check(rowptr, col, seeds, fanouts, False, seed)
    deg_of = np.diff(rowptr)[got[0]]
    counts = np.diff(got[1])
    expanded = len(seeds) + got[4][1]
    assert np.array_equal(counts[:expanded], np.minimum(deg_of[:expanded], k)), k


# ---- claim race -----------------------------------------------------------------------------------------
def test_claim_race_on_a_star():
    """2000 frontier nodes all pick node 0 and one private neighbour each: node 0 gets the
    id of its first slot whatever the arrival order of the 2000 claims."""
    F = 2000
    row = np.repeat(np.arange(1, F + 1), 2)
    col = np.stack([np.zeros(F, np.int64), np.arange(F + 1, 2 * F + 1)], 1).reshape(-1)
    rowptr, col = sorted_csr(row, col, 2 * F + 1)
    seeds = np.arange(1, F + 1)
    adj = adj_of(rowptr, col)
    for fanouts in ([2], [-1], [2, 1]):
        first = check(rowptr, col, seeds, fanouts, False, 3, adj=adj)
        second, _ = unpack(adj.neighbor_sample(gpu(seeds), fanouts, seed=3))
        assert_same(second, first, ("second run", fanouts))
        assert first[0][F] == 0 and np.array_equal(first[0][F + 1:2 * F + 1], np.arange(F + 1, 2 * F + 1)), fanouts


# ---- seen nodes --------------------------------------------------------------------------------------------
def ring_with_chords(N=64):
    i = np.arange(N)
    row = np.repeat(i, 3)
    col = np.stack([(i + 1) % N, (i - 1) % N, (i + 8) % N], 1).reshape(-1)
    return sorted_csr(row, col, N)


def test_seen_nodes_keep_their_ids():
    """Hop 2 picks seeds, hop-1 nodes and nodes that a smaller slot of the same hop claimed."""
    rowptr, col = ring_with_chords()
    for fanouts in ([-1, -1, -1], [2, 2, 2], [3, -1, 2]):
        for replace in (False, True):
            got = check(rowptr, col, [0, 1, 9, 63], fanouts, replace, 21)
            if fanouts[0] == -1:
                hop2 = got[2][got[5][0]:got[5][0] + got[5][1]]
                assert (hop2 < 4).any() and ((hop2 >= 4) & (hop2 < 4 + got[4][1])).any() and (hop2 >= 4 + got[4][1]).any()


def test_self_loops_only():
    N = 50
    rowptr, col = np.arange(N + 1), np.arange(N)
    for replace in (False, True):
        for fanouts in ([2, 2], [-1, -1]):
            got = check(rowptr, col, [7, 3, 49], fanouts, replace, 2)
            assert got[0].tolist() == [7, 3, 49] and got[4] == [3, 0, 0], (fanouts, replace)


# ---- empty cases ---------------------------------------------------------------------------------------------
def test_empty_cases():
    rowptr, col = graph("loops_multi_isolated")
    adj = adj_of(rowptr, col)
    none = np.zeros(0, np.int64)
    got = check(rowptr, col, none, [3, 2], adj=adj)
    assert got[4] == [0, 0, 0] and got[5] == [0, 0] and got[1].tolist() == [0]
    got = check(rowptr, col, [4, 2, 9], [], adj=adj)
    assert got[0].tolist() == [4, 2, 9] and got[1].tolist() == [0, 0, 0, 0] and got[4] == [3] and got[5] == []
    got = check(rowptr, col, np.arange(40), [3, 0, 3], adj=adj)
    assert got[4][2:] == [0, 0] and got[5][1:] == [0, 0] and got[5][0] > 0
    for fanouts in ([3, 2], [-1, -1]):
        got = check(rowptr, col, np.arange(300, 340), fanouts, adj=adj)  # nodes from 250 on have no entries
        assert got[4] == [40, 0, 0] and got[3].size == 0
    check(np.zeros(11, np.int64), none, [3, 1], [2, -1])
    check(np.zeros(11, np.int64), none, [3, 1], [2], replace=True)


# ---- sampler reuse ------------------------------------------------------------------------------------------------
def test_a_reused_sampler_equals_fresh_calls_also_after_an_error():
    import paddle_sparse_amd as psa

    rowptr, col = graph("uniform")
    adj = adj_of(rowptr, col)
    N = len(rowptr) - 1
    for fanouts, replace in (([5, 3, 2], False), ([-1, 2], False), ([3, 3], True)):
        sampler = psa.NeighborSampler(adj, fanouts, replace)
        batches = [np.random.default_rng(s).permutation(N)[:size] for s, size in ((1, 300), (2, 64), (3, 300))]
        for i, seeds in enumerate(batches):
            got, _ = unpack(sampler(gpu(seeds), seed=i))
            fresh, _ = unpack(adj.neighbor_sample(gpu(seeds), fanouts, replace=replace, seed=i))
            assert_same(got, fresh, ("reuse", i))
            if i == 0:
                assert_same(got, neighbor_sample_ref(rowptr, col, seeds, fanouts, replace, i), "restatement")
        for bad, error in ((np.concatenate([batches[0], batches[0][:1]]), ValueError),
                           (np.concatenate([batches[1], [N]]), IndexError)):
            with pytest.raises(error):
                sampler(gpu(bad), seed=9)
            got, _ = unpack(sampler(gpu(batches[2]), seed=2))
            fresh, _ = unpack(adj.neighbor_sample(gpu(batches[2]), fanouts, replace=replace, seed=2))
            assert_same(got, fresh, ("after", error.__name__))
        # the map is clean again: every entry is the "unseen" word
        local = sampler._workspace.buf[:4 * N].view(torch.int32)
        assert sampler._workspace.clean and bool((local == -2**31).all())


# ---- errors ----------------------------------------------------------------------------------------------------------
def test_errors():
    rowptr, col = graph("uniform")
    adj = adj_of(rowptr, col)
    N = len(rowptr) - 1
    with pytest.raises(ValueError, match="distinct"):
        adj.neighbor_sample(gpu([5, 9, 5]), [2])
    for bad in (-1, N):
        for fanouts in ([2], [-1], []):
            with pytest.raises(IndexError):
                adj.neighbor_sample(gpu([5, bad, 7]), fanouts)
    with pytest.raises(ValueError, match="square"):
        adj_of(rowptr, col, N=N + 1).neighbor_sample(gpu([1]), [2])
    with pytest.raises(TypeError):
        adj.neighbor_sample(gpu([1.0], torch.float32), [2])
    with pytest.raises(ValueError):
        adj.neighbor_sample(gpu([[1, 2]]), [2])
    with pytest.raises(ValueError):
        adj.neighbor_sample(gpu([1]), [2, -2])


# ---- host reads ------------------------------------------------------------------------------------------------------
def test_host_reads_are_bounded_by_the_design():
    """One read per hop plus the one behind the sort; a fan-out of -1 adds the read that sizes
    its slots.  Conditions of the design, not measurements."""
    from paddle_sparse_amd import ops

    rowptr, col = graph("uniform")
    rowptr, col, seeds = gpu(rowptr), gpu(col), gpu(seeds_of("uniform", 257))
    for fanouts in ([5, 3, 2], [-1, 2], [3, -1], [-1, -1, -1], [4, 0, 4], []):
        stats = {}
        ops.neighbor_sample(rowptr, col, seeds, fanouts, False, 1, stats=stats)
        L = len(fanouts)
        assert stats["host_reads"] <= (L + 1 if all(k >= 0 for k in fanouts) else 2 * L + 1), fanouts
        assert stats["hops_run"] == (1 if fanouts == [4, 0, 4] else L), fanouts
        ops.neighbor_sample(rowptr, col, gpu([]), fanouts, False, 1, stats=stats)
        assert stats["host_reads"] == 0 and stats["hops_run"] == 0, fanouts


# ---- properties at loader size ---------------------------------------------------------------------------------------
def test_properties_at_loader_size():
    N, S, fanouts = 200_000, 1024, [15, 10, 5]
    row, rowptr, col, _ = random_csr(N, N, 2_000_000, seed=8, sort_cols=True)
    adj = adj_of(rowptr, col)
    seeds = gpu(np.random.default_rng(8).permutation(N)[:S])
    sub, n_id, e_id, (nodes, edges) = adj.neighbor_sample(seeds, fanouts, seed=4)
    n, E = n_id.numel(), e_id.numel()
    assert torch.equal(n_id[:S], seeds) and torch.unique(n_id).numel() == n
    assert nodes[0] == S and sum(nodes) == n and sum(edges) == E and len(nodes) == 4 and len(edges) == 3
    p, c, _ = sub.csr()
    r = sub.storage.row()
    assert int(p[-1]) == E and sub.sparse_sizes() == (n, n)
    assert torch.equal(gpu(row)[e_id], n_id[r]) and torch.equal(gpu(col)[e_id], n_id[c])
    node_lo = np.concatenate([[0], np.cumsum(nodes)]).tolist()
    edge_lo = np.concatenate([[0], np.cumsum(edges)]).tolist()
    for hop in range(3):  # each hop's targets lie in the previous hop's id range
        rr = r[edge_lo[hop]:edge_lo[hop + 1]]
        assert int(rr.min()) >= node_lo[hop] and int(rr.max()) < node_lo[hop + 1]
        assert int(c[edge_lo[hop]:edge_lo[hop + 1]].max()) < node_lo[hop + 2]
    assert bool((p[node_lo[3]:] == E).all())
    # picks within a row are distinct storage positions, k at most, all of a short row
    key = r * (2 * 10**6) + e_id
    assert torch.unique(key).numel() == E
    deg = torch.diff(gpu(rowptr))[n_id]
    k_of = torch.repeat_interleave(torch.tensor(fanouts + [0], device="cuda"), torch.tensor(nodes, device="cuda"))
    assert torch.equal(torch.diff(p), torch.minimum(deg, k_of))
    # the storage's own validation: bounds, and (row, col) order without a re-sort
    from paddle_sparse_amd import SparseStorage, ops

    _, unsorted = ops.make_keys(r, c, n, check_sorted=True)
    assert int(unsorted.item()) == 0
    st = SparseStorage(row=r, rowptr=p, col=c, sparse_sizes=(n, n))
    assert st.col().data_ptr() == c.data_ptr() and torch.equal(st.rowptr(), ops.ind2ptr(r, n))


# ---- directed=False ----------------------------------------------------------------------------------------------------
def test_undirected_is_the_induced_subgraph():
    rowptr, col = graph("loops_multi_isolated")
    value = torch.arange(len(col), dtype=torch.float32, device="cuda")
    adj = adj_of(rowptr, col, value)
    seeds = gpu(seeds_of("loops_multi_isolated", 64))
    for fanouts in ([5, 3, 2], [-1, 2]):
        _, n_id, _, (nodes, _) = adj.neighbor_sample(seeds, fanouts, seed=6)
        sub, n_id2, e_id, (nodes2, edges2) = adj.neighbor_sample(seeds, fanouts, directed=False, seed=6)
        assert torch.equal(n_id, n_id2) and nodes == nodes2 and edges2 is None, fanouts
        want, want_e = adj.saint_subgraph(n_id)
        assert torch.equal(e_id, want_e) and all(torch.equal(a, b) for a, b in zip(sub.csr(), want.csr())), fanouts
        p, c, e = ref_saint_subgraph(rowptr, col, n_id.cpu().numpy(), len(rowptr) - 1)
        assert np.array_equal(sub.storage.rowptr().cpu().numpy(), p) and np.array_equal(e_id.cpu().numpy(), e), fanouts


# ---- values --------------------------------------------------------------------------------------------------------------
def test_values_are_gathered_by_e_id():
    rowptr, col = graph("loops_multi_isolated")
    seeds = gpu(seeds_of("loops_multi_isolated", 64))
    for dtype, width in ((torch.float32, None), (torch.bfloat16, None), (torch.int64, None), (torch.float32, 3)):
        shape = (len(col),) if width is None else (len(col), width)
        value = torch.randint(-50, 50, shape, device="cuda").to(dtype)
        adj = adj_of(rowptr, col, value)
        for replace in (False, True):
            sub, _, e_id, _ = adj.neighbor_sample(seeds, [4, 3], replace=replace, seed=1)
            got = sub.storage.value()
            assert got.dtype == dtype and torch.equal(got, value[e_id]) and e_id.numel() > 0, (dtype, width, replace)


def test_value_gradient_is_exact_and_repeatable():
    for replace in (False, True):
        value_gradient(replace)


def value_gradient(replace):
    """Integer-valued data: every sum is exact, so the gradient equals float64 autograd of
    value[e_id] bit for bit, whatever the order of the additions."""
    rowptr, col = graph("loops_multi_isolated")
    g = torch.Generator(device="cuda").manual_seed(3)
    value = torch.randint(-8, 9, (len(col),), generator=g, device="cuda").float()
    x = torch.randint(-8, 9, (len(rowptr) - 1, 4), generator=g, device="cuda").float()
    seeds = gpu(seeds_of("loops_multi_isolated", 64))
    grads = []
    for _ in range(2):
        v = value.clone().requires_grad_()
        sub, n_id, e_id, _ = adj_of(rowptr, col, v).neighbor_sample(seeds, [4, 3], replace=replace, seed=1)
        (sub @ x[n_id]).sum().backward()
        grads.append(v.grad)
    assert torch.equal(grads[0], grads[1])
    if replace:
        assert torch.unique(e_id).numel() < e_id.numel()  # the sort + segment-sum route has work to do
    v64 = value.double().requires_grad_()
    p, c, _ = sub.csr()
    r = sub.storage.row()
    dense = torch.zeros(n_id.numel(), n_id.numel(), dtype=torch.float64, device="cuda").index_put(
        (r, c), v64[e_id], accumulate=True)
    (dense @ x[n_id].double()).sum().backward()
    assert torch.equal(grads[0].double(), v64.grad) and bool(grads[0].abs().sum() > 0)


# ---- README ----------------------------------------------------------------------------------------------------------------
def test_the_readme_usage_line_runs_as_written():
    text = (Path(__file__).resolve().parent.parent / "README.md").read_text()
    line = next(l for l in text.splitlines() if "adj.neighbor_sample(" in l and "=" in l and not l.lstrip().startswith("|"))
    assert re.match(r"^sub, n_id, e_id, counts = adj\.neighbor_sample\(batch, \[\d+(, \d+)*\]\)", line.strip()), line
    rowptr, col = graph("uniform")
    scope = {"adj": adj_of(rowptr, col, torch.ones(len(col), device="cuda")), "batch": torch.arange(0, 64, device="cuda"),
             "torch": torch}
    exec(line.strip(), scope)
    sub, n_id, counts = scope["sub"], scope["n_id"], scope["counts"]
    assert torch.equal(n_id[:64], scope["batch"]) and sub.sparse_sizes() == (n_id.numel(),) * 2
    assert sum(counts[0]) == n_id.numel() and sum(counts[1]) == scope["e_id"].numel() == sub.nnz()
