"""CPU suite for the node2vec (p, q) walk: pins the restatement of tests/node2vec_ref.py to
the existing walks and to answers that need no random number, holds the host export
psa_node2vec_walk_host (the kernel's own step, csrc/node2vec_step.h) to it bit for bit on the
GPU suite's case table, and checks the argument rules of the C entry point and of
random_walk(p=, q=).  No GPU needed.

The kite statistics: the largest deviation over the five cases is 1.62 sigma (bound: 5)."""
import numpy as np
import pytest

import node2vec_ref as nr
import weighted_ref as wr

ONE = nr.ONE


# ---- the restatement ---------------------------------------------------------------------------
def test_bias_constants():
    assert nr.bias(1, 1) == ((ONE, ONE, ONE), 32)
    assert nr.bias(0.25, 4) == ((ONE, ONE // 4, ONE // 16), 32 * 16)
    assert nr.bias(4, 0.25) == ((ONE // 16, ONE // 4, ONE), 32 * 16)
    assert nr.bias(2, 1) == ((ONE // 2, ONE, ONE), 64)
    assert nr.bias(1 / 32, 32) == ((ONE, ONE // 32, ONE // 1024), 32768)
    thr, max_tries = nr.bias(3, 0.7)
    assert max(thr) == ONE and max_tries == 32 * 5  # ceil((1/0.7) / (1/3)) = ceil(4.29)


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("weighted", [False, True])
def test_with_every_threshold_at_one_it_is_the_existing_walk(symmetric, weighted):
    rowptr, col, _, cum = nr.case_graph(symmetric)
    cum = cum if weighted else None
    start = np.concatenate([nr.case_start(257), np.arange(0, nr.N_NODES, 5)])  # some without entries
    want = wr.ref_weighted_walk(rowptr, col, cum, start, 17, 99)
    got = nr.ref_node2vec_walk(rowptr, col, cum, start, 17, 99, (ONE,) * 3, 32)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (want[1] < 0).any() and (want[1] >= 0).any()


def test_a_path_walk_that_never_returns_until_the_end_of_the_path():
    """thr = (0, 1, 1): a proposal back to the previous node is always refused, so on a path
    the walk goes straight on; at the end node every proposal leads back, all 64 tries are
    refused and the last one is taken."""
    rowptr, col = nr.path_graph(10)
    nodes, e_id = nr.ref_node2vec_walk(rowptr, col, None, [0], 12, 5, (0, ONE, ONE), 64)
    assert nodes.tolist() == [[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 8, 7, 6]]
    assert np.array_equal(col[e_id[0]], nodes[0, 1:])
    stats = {}
    nr.ref_node2vec_walk(rowptr, col, None, [0], 10, 5, (0, ONE, ONE), 64, stats)
    assert stats["steps"] == 10 and stats["tries"] >= 9 + 64  # step 9, at node 9, ran out of tries


def test_with_one_try_every_step_is_the_plain_walks_step():
    rowptr, col = nr.path_graph(10)
    start = np.arange(10)
    want = wr.ref_weighted_walk(rowptr, col, None, start, 12, 5)
    for thr in ((0, ONE, ONE), (0, 0, 0), (ONE, 0, ONE // 3)):
        got = nr.ref_node2vec_walk(rowptr, col, None, start, 12, 5, thr, 1)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("p,q,weighted,seed", nr.KITE_CASES)
def test_kite_third_nodes_follow_the_bias(p, q, weighted, seed):
    rowptr, col, w = nr.kite_graph()
    cum = wr.row_cdf(rowptr, w) if weighted else None
    thr, max_tries = nr.bias(p, q)
    nodes, _ = nr.ref_node2vec_walk(rowptr, col, cum, np.zeros(nr.KITE_WALKS, np.int64), 2, seed, thr, max_tries)
    sigma, n = nr.kite_sigmas(nodes, p, q, weighted)
    print(f"kite p={p} q={q} weighted={weighted}: {n} walks through node 2, largest deviation {sigma:.2f} sigma")
    assert n > nr.KITE_WALKS // 3 and sigma < 5


# ---- the host export ---------------------------------------------------------------------------
def host(rowptr, col, cum, start, L, seed, thr, max_tries):
    from paddle_sparse_amd import ops

    nodes, e_id, flags = ops.node2vec_walk_host(rowptr, col, cum, start, L, seed, thr, max_tries)
    assert flags == 0
    return nodes, e_id


@pytest.mark.parametrize("k", range(len(nr.CASES)))
def test_host_export_equals_the_restatement_on_the_case_table(k):
    symmetric, S, L, pq, mode, _ = nr.CASES[k]
    rowptr, col, _, cum = nr.case_graph(symmetric)
    thr, max_tries = nr.bias(*pq)
    nodes, e_id = host(rowptr, col, None if mode == "uniform" else cum, nr.case_start(S), L, nr.CASE_SEED + k, thr,
                       max_tries)
    want = nr.case_ref(k)
    assert nodes.shape == (S, L + 1) and e_id.shape == (S, L)
    assert np.array_equal(nodes, want[0]) and np.array_equal(e_id, want[1])


def test_the_case_table_covers_what_it_names():
    cases = nr.CASES
    assert {c[1] for c in cases} == set(nr.SIZES) and {c[2] for c in cases} == set(nr.LENGTHS)
    for a, b in ((3, 4), (3, 5), (4, 5), (0, 3), (0, 4), (0, 5)):
        assert len({(c[a], c[b]) for c in cases}) == len({c[a] for c in cases}) * len({c[b] for c in cases})
    deg = np.diff(nr.case_graph(False)[0])
    assert deg[:nr.DENSE].tolist() == [nr.DEGS[i % 9] for i in range(nr.DENSE)] and deg[nr.HUB] == nr.HUB_DEG
    for symmetric in (True, False):
        rowptr, col, w, cum = nr.case_graph(symmetric)
        row = np.repeat(np.arange(nr.N_NODES), np.diff(rowptr))
        assert len(np.unique(col[rowptr[nr.HUB]:rowptr[nr.HUB + 1]])) >= nr.HUB_DEG
        assert (row == col).sum() >= 50 and (np.diff(rowptr) == 0).any()
        assert ((row[1:] == row[:-1]) & (col[1:] == col[:-1])).any()  # duplicated entries
        assert rowptr[nr.ZERO_ROW + 1] > rowptr[nr.ZERO_ROW] and cum[rowptr[nr.ZERO_ROW + 1] - 1] == 0
        assert (w == 0).mean() > 0.2


def test_host_export_on_raw_thresholds_and_the_path():
    rowptr, col, _, cum = nr.case_graph(True)
    start = nr.case_start(65)
    for thr in ((0, ONE, ONE), (ONE, 0, ONE), (ONE, ONE, 0), (0, 0, 0)):
        for max_tries in (1, 2, 64):
            for c in (None, cum):
                got = host(rowptr, col, c, start, 9, 3, thr, max_tries)
                want = nr.ref_node2vec_walk(rowptr, col, c, start, 9, 3, thr, max_tries)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    rowptr, col = nr.path_graph(10)
    nodes, _ = host(rowptr, col, None, [0], 12, 5, (0, ONE, ONE), 64)
    assert nodes.tolist() == [[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 8, 7, 6]]


def test_host_export_flags_a_start_outside_the_matrix():
    from paddle_sparse_amd import ops

    rowptr, col = nr.path_graph(10)
    nodes, e_id, flags = ops.node2vec_walk_host(rowptr, col, None, [3, 10, -1, 4], 2, 1, (ONE,) * 3, 32)
    assert flags == 1
    assert (nodes[[1, 2]] == -7).all() and (e_id[[1, 2]] == -7).all()  # left unwritten
    assert nodes[0, 0] == 3 and nodes[3, 0] == 4 and (e_id[[0, 3]] >= 0).all()


def test_argument_errors_of_the_c_entry_points():
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    rowptr, col = nr.path_graph(10)
    start = np.zeros(4, np.int64)
    out, e_id, flags = np.zeros((4, 4), np.int64), np.zeros((4, 3), np.int64), np.zeros(1, np.int64)
    p = lambda a: a.ctypes.data  # noqa: E731

    def call(rowptr_=p(rowptr), start_=p(start), out_=p(out), flags_=p(flags), N=10, S=4, L=3, thr=(ONE,) * 3,
             max_tries=32):
        return lib.psa_node2vec_walk_host(rowptr_, p(col), None, N, start_, S, L, 1, *thr, max_tries, out_, p(e_id),
                                          flags_)

    OK, INVALID = 0, 1
    assert call() == OK and out[:, 1].tolist() == [1] * 4
    assert call(S=0, rowptr_=None, start_=None, out_=None, flags_=None) == OK
    for bad in (dict(rowptr_=None), dict(start_=None), dict(out_=None), dict(flags_=None), dict(N=-1), dict(S=-1),
                dict(L=-1), dict(max_tries=0), dict(max_tries=-5), dict(max_tries=32769), dict(thr=(ONE + 1, ONE, ONE)),
                dict(thr=(ONE, ONE + 1, ONE)), dict(thr=(0, 0, 2**64 - 1)), dict(S=0, max_tries=0)):
        assert call(**bad) == INVALID, bad
        assert b"psa_node2vec_walk_host" in lib.psa_last_error()
    assert call(max_tries=32768, thr=(0, 0, 0)) == OK
    # the device entry point refuses the same arguments before it touches the GPU
    none = (None,) * 4
    assert lib.psa_node2vec_walk(None, None, None, 10, None, 4, 3, 1, ONE, ONE, ONE, 32, *none) == INVALID
    assert lib.psa_node2vec_walk(1, 1, None, 10, 1, 4, 3, 1, ONE, ONE, ONE + 1, 32, 1, None, 1, None) == INVALID
    assert lib.psa_node2vec_walk(1, 1, None, 10, 1, 4, 3, 1, ONE, ONE, ONE, 0, 1, None, 1, None) == INVALID


# ---- random_walk(p=, q=) -------------------------------------------------------------------------
def test_python_bias_equals_the_restatements():
    from paddle_sparse_amd import rw

    for p, q in nr.PQS + ((3, 0.7), (1, 1024), (1 / 1024, 1), (1 / 32, 32), (1e-3, 1e-3), (7, 7)):
        assert rw._node2vec_bias(p, q) == nr.bias(p, q), (p, q)
        thr, max_tries = rw._node2vec_bias(p, q)
        assert max(thr) == ONE and min(thr) > 0 and 32 <= max_tries <= 32768


class _Stop(Exception):
    pass


def _cpu_adj(N=4, M=None):
    import torch
    from paddle_sparse_amd import SparseTensor

    return SparseTensor(rowptr=torch.arange(N + 1), col=torch.arange(N), sparse_sizes=(N, N if M is None else M),
                        is_sorted=True, trust_data=True)


@pytest.mark.parametrize("bad", [dict(p=0), dict(p=-1), dict(q=0), dict(q=-2.5), dict(p=float("inf")),
                                 dict(q=float("inf")), dict(p=float("nan")), dict(q=float("nan")),
                                 dict(p=1025), dict(q=1 / 1025), dict(p=1 / 33, q=32), dict(p=64, q=1 / 32)])
def test_bad_p_and_q_are_refused_before_anything_runs(bad, monkeypatch):
    import torch
    from paddle_sparse_amd import ops

    def never(*a, **k):
        raise AssertionError("reached an op")

    for name in ("node2vec_walk", "random_walk", "random_walk_weighted"):
        monkeypatch.setattr(ops, name, never)
    with pytest.raises(ValueError, match="random_walk"):
        _cpu_adj().random_walk(torch.arange(4), 3, seed=1, **bad)


def test_p_q_arguments_and_their_routes(monkeypatch):
    import torch
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import ops

    seen = []

    def stop(name):
        def f(*a, **k):
            seen.append((name, a))
            raise _Stop

        return f

    for name in ("node2vec_walk", "random_walk", "random_walk_weighted"):
        monkeypatch.setattr(ops, name, stop(name))
    adj, start = _cpu_adj(), torch.arange(4, dtype=torch.int32)
    # p = q = 1, in any spelling, takes today's route
    for kw in (dict(), dict(p=1, q=1), dict(p=1.0, q=1.0)):
        with pytest.raises(_Stop):
            adj.random_walk(start, 3, seed=1, **kw)
        assert seen.pop()[0] == "random_walk"
        with pytest.raises(_Stop):
            psa.random_walk(adj, start, 3, 1, False, True, **kw)
        assert seen.pop()[0] == "random_walk_weighted"
    # anything else reaches the new op with the thresholds of the definition, keyword or positional
    for call in (lambda: adj.random_walk(start, 3, seed=1, p=0.25, q=4),
                 lambda: adj.random_walk(start, 3, 1, False, False, 0.25, 4),
                 lambda: psa.random_walk(adj, start, 3, 1, False, False, 0.25, 4),
                 lambda: psa.random_walk(adj, start, 3, seed=1, q=4, p=0.25)):
        with pytest.raises(_Stop):
            call()
        name, args = seen.pop()
        assert name == "node2vec_walk" and args[2] is None and args[3].dtype == torch.int64
        assert args[4:] == (3, 1, (ONE, ONE // 4, ONE // 16), 512, False)
    with pytest.raises(_Stop):
        adj.random_walk(start, 3, seed=1, q=1024, return_edge_ids=True)
    assert seen.pop()[1][6:] == ((ONE, ONE, ONE // 1024), 32768, True)
    assert not seen
    # the checks of random_walk come first, as before
    with pytest.raises(ValueError, match="square"):
        _cpu_adj(4, 5).random_walk(start, 3, seed=1, p=2)
    with pytest.raises(TypeError):
        adj.random_walk(start.float(), 3, seed=1, p=2)


def test_ops_node2vec_walk_checks_its_thresholds():
    import torch
    from paddle_sparse_amd import ops

    x = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.node2vec_walk(x, x, None, x, 2, 1, (ONE,) * 3, 32)
    assert ops._node2vec_args((0, ONE, 5), 32768) == ((0, ONE, 5), 32768)
    for thr, max_tries in (((ONE + 1, 0, 0), 32), ((0, -1, 0), 32), ((ONE, ONE), 32), ((ONE,) * 3, 0),
                           ((ONE,) * 3, 32769)):
        with pytest.raises(ValueError):
            ops._node2vec_args(thr, max_tries)
