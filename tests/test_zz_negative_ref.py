"""CPU suite for edge lookup and negative sampling: pins the restatement of tests/negative_ref.py
and the host exports psa_edge_lookup_host / psa_negative_sample_host (the kernels' own steps,
csrc/edge_lookup.h) to answers that need no random number, holds the two together bit for bit on
the GPU suite's case tables, and checks the argument rules of the C entry points and of the public
functions.  No GPU needed.

Every hand-checked answer is asked of the restatement and of the host export alike (lookup(),
sample()), so that neither can drift alone.

Uniformity, S = 100 000 samples, seeds fixed: the largest deviation of a free cell's count from
S / cells is 1.14 sigma for the one row of N = 16 (10 free columns, seed 5) and 3.06 sigma for the
12 x 12 matrix at density 0.5 (72 free pairs, seed 9); the bound is 5."""
import numpy as np
import pytest

import negative_ref as nr
import weighted_ref as wr


def lookup(rowptr, col, M, N, row_q, col_q):
    """(pos, flags) of the restatement, which the host export must equal."""
    from paddle_sparse_amd import ops

    want = nr.ref_edge_lookup(rowptr, col, M, N, row_q, col_q)
    got = ops.edge_lookup_host(rowptr, col, N, row_q, col_q)
    assert len(rowptr) == M + 1
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    return want[0].tolist(), want[1]


def sample(rowptr, col, M, N, src, count, loops, max_tries, seed):
    """(row or None, col, flags) of the restatement, which the host export must equal."""
    from paddle_sparse_amd import ops

    row, cols, flags = nr.ref_negative_sample(rowptr, col, M, N, src, count, loops, max_tries, seed)
    got = ops.negative_sample_host(rowptr, col, N, src, count, loops, max_tries, seed)
    assert len(rowptr) == M + 1
    if src is None:
        assert np.array_equal(got[0], row)
    assert np.array_equal(got[-2], cols) and got[-1] == flags
    return row, cols, flags


# ---- lookup: hand answers ---------------------------------------------------------------------------
def test_lookup_on_a_tiny_matrix_with_duplicates():
    rowptr, col, M, N = nr.tiny()
    assert rowptr.tolist() == [0, 5, 7, 7, 9, 10] and col.tolist() == [1, 3, 3, 3, 6, 0, 7, 2, 2, 4]
    # the first of a triple and of a pair; the first and the last entry of a row
    assert lookup(rowptr, col, M, N, [0, 3, 0, 0], [3, 2, 1, 6]) == ([1, 7, 0, 4], 0)
    # the first and the last column of the matrix, stored (row 1) and not (row 0)
    assert lookup(rowptr, col, M, N, [1, 1, 0, 0], [0, 7, 0, 7]) == ([5, 6, -1, -1], 0)
    # below the first, between two and above the last column of a row
    assert lookup(rowptr, col, M, N, [0, 0, 0, 3, 3], [0, 2, 7, 1, 3]) == ([-1, -1, -1, -1, -1], 0)
    # the empty row, at every column, and its neighbours' columns
    assert lookup(rowptr, col, M, N, [2] * 8, list(range(8))) == ([-1] * 8, 0)
    # the last row
    assert lookup(rowptr, col, M, N, [4, 4, 4], [4, 3, 5]) == ([9, -1, -1], 0)
    assert lookup(rowptr, col, M, N, [], []) == ([], 0)


def test_lookup_flags_pairs_outside_the_matrix_and_reads_nothing_through_them():
    rowptr, col, M, N = nr.tiny()
    for r, c in ((-1, 0), (5, 0), (0, -1), (0, 8), (2**62, 1), (1, -2**63), (-2**63, 2**63 - 1)):
        assert lookup(rowptr, col, M, N, [0, r, 4], [1, c, 4]) == ([0, -1, 9], 1), (r, c)
    assert lookup(rowptr, col, M, N, [0, 4], [1, 4]) == ([0, 9], 0)


def test_lookup_with_column_ids_above_2_to_the_32():
    rowptr, col, M, N = nr.case_graph("huge")
    B = 1 << 32
    assert lookup(rowptr, col, M, N, [0, 0, 0, 1, 1, 1, 3], [3, B + 3, N - 1, B - 1, B, B + 1, 5 * B + 7]) \
        == ([0, 1, 2, 3, 4, 5, 6], 0)
    # what a 32-bit column would confuse with a stored entry
    assert lookup(rowptr, col, M, N, [1, 1, 3, 5, 4], [0, 1, 7, (1 << 33) + 7, B]) == ([-1] * 5, 0)
    assert lookup(rowptr, col, M, N, [0], [N]) == ([-1], 1)


# ---- sampling: hand answers ---------------------------------------------------------------------------
@pytest.mark.parametrize("free", [0, 5, 7])
def test_a_row_with_exactly_one_free_column_returns_it(free):
    rowptr, col, M, N = nr.one_free(free)
    src = np.arange(N - 1).repeat(3)
    _, cols, flags = sample(rowptr, col, M, N, src, 2, False, 32768, 11)
    assert cols.tolist() == [free] * (len(src) * 2) and flags == 0


def test_a_full_row_gives_minus_one_and_flag_two():
    rowptr, col, M, N = nr.one_free(5)
    stats = {}
    nr.ref_negative_sample(rowptr, col, M, N, [N - 1], 2, False, 100, 3, stats)
    assert stats["tries"] == 200
    _, cols, flags = sample(rowptr, col, M, N, [N - 1, 0, N - 1], 2, False, 100, 3)
    assert cols.tolist() == [-1, -1, 5, 5, -1, -1] and flags == 2


def test_a_row_whose_only_free_column_is_the_diagonal_gives_minus_one_without_self_loops():
    rows = [(r, c) for r in range(8) for c in range(8) if c != r or r >= 4]  # rows 0 .. 3 lack their diagonal only
    rowptr, col = nr.sorted_csr(*zip(*rows), 8)
    _, cols, flags = sample(rowptr, col, 8, 8, [0, 1, 2, 3], 1, False, 32768, 1)
    assert cols.tolist() == [0, 1, 2, 3] and flags == 0
    _, cols, flags = sample(rowptr, col, 8, 8, [0, 1, 2, 3], 1, True, 512, 1)
    assert cols.tolist() == [-1] * 4 and flags == 2
    # global mode on the same matrix: the four free pairs are the diagonal's
    row, cols, flags = sample(rowptr, col, 8, 8, None, 40, False, 32768, 1)
    assert flags == 0 and np.array_equal(row, cols) and set(row.tolist()) == {0, 1, 2, 3}
    row, cols, flags = sample(rowptr, col, 8, 8, None, 5, True, 512, 1)
    assert flags == 2 and row.tolist() == [-1] * 5 and cols.tolist() == [-1] * 5


def test_a_matrix_without_rows_or_columns_fails_every_sample_and_is_not_read():
    for M, N in ((0, 0), (0, 5), (5, 0)):
        rowptr = np.zeros(M + 1, np.int64)
        row, cols, flags = sample(rowptr, [], M, N, None, 3, False, 64, 1)
        assert row.tolist() == [-1] * 3 and cols.tolist() == [-1] * 3 and flags == 2
    _, cols, flags = sample(np.zeros(6, np.int64), [], 5, 0, [0, 4], 2, False, 64, 1)
    assert cols.tolist() == [-1] * 4 and flags == 2
    # no rows: every given source is outside the matrix
    _, cols, flags = sample(np.zeros(1, np.int64), [], 0, 5, [0], 2, False, 64, 1)
    assert cols.tolist() == [-1] * 2 and flags == 1
    assert lookup(np.zeros(1, np.int64), [], 0, 0, [0], [0]) == ([-1], 1)


def test_given_rows_outside_the_matrix_are_flagged_and_the_others_sampled():
    rowptr, col, M, N = nr.tiny()
    _, cols, flags = sample(rowptr, col, M, N, [2, -1, 5, 2**40, 4], 2, False, 64, 4)
    assert flags == 1 and cols[2:8].tolist() == [-1] * 6 and (cols[:2] >= 0).all() and (cols[8:] >= 0).all()
    assert 4 not in cols[8:].tolist()


@pytest.mark.parametrize("seed", [0, 1, 2**63 + 5, 2**64 - 1])
def test_on_an_empty_matrix_with_one_try_the_sample_is_the_streams_first_word(seed):
    M, N, n = 12, 1000, 70
    rowptr = np.zeros(M + 1, np.int64)
    want_col = [(wr.mix64(nr.rand_stream(seed, i)) * N) >> 64 for i in range(n)]
    want_row = [(wr.mix64((nr.rand_stream(seed, i) + 2**63) & wr.M64) * M) >> 64 for i in range(n)]
    assert wr.mix64(nr.rand_stream(seed, 3)) == wr.word(seed, 3, 0)  # the walks' stream, draw 0
    row, cols, flags = sample(rowptr, [], M, N, None, n, False, 1, seed)
    assert cols.tolist() == want_col and row.tolist() == want_row and flags == 0
    # given rows: the same columns, sample i belonging to src[i // k]
    _, cols, flags = sample(rowptr, [], M, N, np.arange(35) % M, 2, False, 1, seed)
    assert cols.tolist() == want_col and flags == 0
    # try j reads stream + j: with the first column refused everywhere the second word decides
    second = [(wr.mix64((nr.rand_stream(seed, i) + 1) & wr.M64) * N) >> 64 for i in range(n)]
    full = nr.sorted_csr(np.arange(M).repeat(n), np.tile(want_col, M), M)
    _, cols, _ = sample(*full, M, N, np.zeros(n, np.int64), 1, False, 2, seed)
    hit = np.isin(second, want_col)
    assert np.array_equal(cols[~hit], np.array(second)[~hit]) and (cols[hit] == -1).all() and (~hit).sum() > n // 2


# ---- the case tables: host exports against the restatement --------------------------------------------
@pytest.mark.parametrize("k", range(len(nr.LOOKUP_CASES)))
def test_lookup_host_export_equals_the_restatement_on_the_case_table(k):
    from paddle_sparse_amd import ops

    name, Q = nr.LOOKUP_CASES[k]
    rowptr, col, _, N = nr.case_graph(name)
    pos, flags = ops.edge_lookup_host(rowptr, col, N, *nr.case_queries(name, Q))
    want = nr.lookup_ref(k)
    assert pos.shape == (Q,) and flags == want[1] == 0 and np.array_equal(pos, want[0])


@pytest.mark.parametrize("k", range(len(nr.SAMPLE_CASES)))
def test_sample_host_export_equals_the_restatement_on_the_case_table(k):
    from paddle_sparse_amd import ops

    name, given, S, kk, loops = nr.SAMPLE_CASES[k]
    rowptr, col, M, N = nr.case_graph(name)
    got = ops.negative_sample_host(rowptr, col, N, nr.case_src(name, S) if given else None, kk if given else S, loops,
                                   nr.CASE_MAX_TRIES, nr.CASE_SEED + k)
    row, cols, flags = nr.sample_ref(k)
    assert got[-2].shape == (S * kk,) and np.array_equal(got[-2], cols) and got[-1] == flags
    if not given:
        assert np.array_equal(got[0], row)
    # on the table's graphs (density <= 0.5 in every row but one, 64 tries) no sample fails
    assert flags == 0 and (cols >= 0).all()
    # and what comes back is not stored, the pairs checked against a Python set
    stored = nr.stored_pairs(name)
    rows = np.repeat(nr.case_src(name, S), kk) if given else row
    pairs = list(zip(rows.tolist(), cols.tolist()))
    assert not stored.intersection(pairs)
    if loops:
        assert all(r != c for r, c in pairs)


def test_the_case_tables_cover_what_they_name():
    from paddle_sparse_amd import ops

    assert 1 <= nr.CASE_MAX_TRIES <= ops.NEGATIVE_MAX_TRIES  # the tables' tries are tries the ops accept
    rowptr, col, M, N = nr.case_graph("degs")
    deg = np.diff(rowptr)
    assert deg[:-1].tolist() == [nr.DEGS[i % 7] for i in range(M - 1)] and deg[-1] == nr.BIG_DEG
    row = nr.coo_rows(rowptr)
    assert ((row[1:] == row[:-1]) & (col[1:] == col[:-1])).sum() > 500 and (row == col).sum() > 100
    assert (np.diff(col)[row[1:] == row[:-1]] >= 0).all()
    assert deg.max() / N <= 0.5
    rowptr, col, M, N = nr.case_graph("rect")
    assert (M, N) == (40, 70) and 0.2 < len(col) / (M * N) < 0.4 and np.diff(rowptr).max() / N <= 0.5
    rowptr, col, M, N = nr.case_graph("huge")
    assert N == 2**40 and len(col) == 12 and (col > 2**32).sum() >= 6 and (col < 2**32).sum() >= 4
    assert {Q for _, Q in nr.LOOKUP_CASES} == set(nr.COUNTS)
    assert {S * k for _, _, S, k, _ in nr.SAMPLE_CASES} >= set(nr.COUNTS)
    assert {(given, k, loops) for g, given, S, k, loops in nr.SAMPLE_CASES if g == "degs"} \
        == {(False, 1, False), (False, 1, True), (True, 1, False), (True, 1, True), (True, 3, False), (True, 3, True)}
    assert {g for g, *_ in nr.SAMPLE_CASES} == set(nr.GRAPHS) == {g for g, _ in nr.LOOKUP_CASES}
    for k, (name, Q) in enumerate(nr.LOOKUP_CASES):
        pos = nr.lookup_ref(k)[0]
        if Q >= 63 and name != "empty":
            assert (pos >= 0).sum() > Q // 4 and (pos < 0).sum() > Q // 8, (name, Q)
            r, c = nr.case_queries(name, Q)
            rowptr, col, _, _ = nr.case_graph(name)
            found = pos >= 0
            assert np.array_equal(nr.coo_rows(rowptr)[pos[found]], r[found])
            assert np.array_equal(col[pos[found]], c[found])
            assert not nr.stored_pairs(name).intersection(zip(r[~found].tolist(), c[~found].tolist()))


# ---- uniformity -------------------------------------------------------------------------------------------
def test_structured_samples_are_uniform_over_the_free_columns_of_a_row():
    rowptr, col, M, N = nr.row16()
    _, cols, flags = sample(rowptr, col, M, N, np.zeros(nr.UNIFORM_S, np.int64), 1, False, 64, nr.ROW16_SEED)
    sigma = nr.row16_sigmas(cols)
    print(f"row of 16 with 6 stored: largest deviation {sigma:.2f} sigma")
    assert flags == 0 and sigma < 5


def test_global_samples_are_uniform_over_the_free_pairs():
    rowptr, col, M, N = nr.square12()
    assert len(col) == 72
    row, cols, flags = sample(rowptr, col, M, N, None, nr.UNIFORM_S, False, 64, nr.SQUARE12_SEED)
    sigma = nr.square12_sigmas(row, cols)
    print(f"12 x 12 at density 0.5: largest deviation {sigma:.2f} sigma")
    assert flags == 0 and sigma < 5


# ---- argument rules of the C entry points -------------------------------------------------------------------
OK, INVALID = 0, 1


def test_argument_errors_of_the_lookup_entry_points():
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    rowptr, col, M, N = nr.tiny()
    rq, cq = np.array([0, 1], np.int64), np.array([1, 7], np.int64)
    pos, flags = np.full(2, -7, np.int64), np.zeros(1, np.int64)
    p = lambda a: a.ctypes.data  # noqa: E731

    def call(rowptr_=p(rowptr), rq_=p(rq), cq_=p(cq), pos_=p(pos), flags_=p(flags), M=M, N=N, Q=2):
        return lib.psa_edge_lookup_host(rowptr_, p(col), M, N, rq_, cq_, Q, pos_, flags_)

    assert call() == OK and pos.tolist() == [0, 6] and flags[0] == 0
    assert call(Q=0, rowptr_=None, rq_=None, cq_=None, pos_=None, flags_=None) == OK
    for bad in (dict(rowptr_=None), dict(rq_=None), dict(cq_=None), dict(pos_=None), dict(flags_=None), dict(M=-1),
                dict(N=-1), dict(Q=-1), dict(Q=0, N=-1)):
        assert call(**bad) == INVALID, bad
        assert b"psa_edge_lookup_host" in lib.psa_last_error()
    # the device entry point refuses the same arguments before it touches the GPU
    assert lib.psa_edge_lookup(None, None, M, N, None, None, 2, None, None, None) == INVALID
    assert lib.psa_edge_lookup(1, 1, M, N, 1, 1, -1, 1, 1, None) == INVALID
    assert lib.psa_edge_lookup(1, 1, -1, N, 1, 1, 2, 1, 1, None) == INVALID
    assert lib.psa_edge_lookup(None, None, M, N, None, None, 0, None, None, None) == OK


def test_argument_errors_of_the_sampling_entry_points():
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    rowptr, col, M, N = nr.tiny()
    src = np.array([0, 2], np.int64)
    row, cols, flags = np.full(6, -7, np.int64), np.full(6, -7, np.int64), np.zeros(1, np.int64)
    p = lambda a: a.ctypes.data  # noqa: E731

    def call(rowptr_=p(rowptr), src_=p(src), row_=None, cols_=p(cols), flags_=p(flags), M=M, N=N, S=2, k=3, loops=0,
             max_tries=64):
        return lib.psa_negative_sample_host(rowptr_, p(col), M, N, src_, S, k, loops, max_tries, 1, row_, cols_, flags_)

    assert call() == OK and (cols >= 0).all() and flags[0] == 0
    assert call(src_=None, row_=p(row), S=6, k=1) == OK and (row >= 0).all()
    assert call(S=0, rowptr_=None, src_=None, cols_=None, flags_=None) == OK
    assert call(max_tries=1) == OK and call(max_tries=32768) == OK
    for bad in (dict(rowptr_=None), dict(cols_=None), dict(flags_=None), dict(src_=None), dict(M=-1), dict(N=-1),
                dict(S=-1), dict(k=0), dict(k=-3), dict(max_tries=0), dict(max_tries=-1), dict(max_tries=32769),
                dict(S=2**62, k=4), dict(S=2**32, k=2**32), dict(loops=1), dict(S=0, k=0), dict(S=0, max_tries=0),
                dict(S=0, loops=1)):
        assert call(**bad) == INVALID, bad
        assert b"psa_negative_sample_host" in lib.psa_last_error()
    assert call(loops=1, N=M) == OK  # square: allowed
    # the device entry point refuses the same arguments before it touches the GPU
    none = (None,) * 4
    assert lib.psa_negative_sample(None, None, M, N, None, 2, 3, 0, 64, 1, *none) == INVALID
    assert lib.psa_negative_sample(1, 1, M, N, 1, 2, 0, 0, 64, 1, None, 1, 1, None) == INVALID
    assert lib.psa_negative_sample(1, 1, M, N, 1, 2, 3, 0, 32769, 1, None, 1, 1, None) == INVALID
    assert lib.psa_negative_sample(1, 1, M, N, 1, 2, 3, 1, 64, 1, None, 1, 1, None) == INVALID
    assert lib.psa_negative_sample(1, 1, M, N, 1, 2**62, 4, 0, 64, 1, None, 1, 1, None) == INVALID
    assert lib.psa_negative_sample(None, None, M, N, None, 0, 1, 0, 64, 1, *none) == OK


# ---- the public functions ---------------------------------------------------------------------------------------
def _cpu_adj(M=4, N=None):
    import torch
    from paddle_sparse_amd import SparseTensor

    return SparseTensor(rowptr=torch.arange(M + 1), col=torch.arange(M), sparse_sizes=(M, M if N is None else N),
                        is_sorted=True, trust_data=True)


def test_the_public_surface():
    import paddle_sparse_amd as psa

    for name in ("edge_ids", "has_edge", "negative_sampling", "structured_negative_sampling"):
        assert name in psa.__all__ and getattr(psa, name) is getattr(psa.negative, name)
        assert getattr(psa.SparseTensor, name) is getattr(psa, name)


def test_type_and_shape_errors_of_the_public_functions():
    import torch
    import paddle_sparse_amd as psa

    adj, ids = _cpu_adj(), torch.arange(4)
    for f in (psa.edge_ids, psa.has_edge):
        with pytest.raises(TypeError, match="SparseTensor"):
            f(ids, ids, ids)
        for bad in (ids.float(), ids.bool(), [0, 1, 2, 3], None):
            with pytest.raises(TypeError, match="integer tensor"):
                f(adj, bad, ids)
            with pytest.raises(TypeError, match="integer tensor"):
                f(adj, ids, bad)
        with pytest.raises(ValueError, match="1-D"):
            f(adj, ids.view(2, 2), ids)
        with pytest.raises(ValueError, match="differ in length"):
            f(adj, ids, ids[:3])
        with pytest.raises(RuntimeError, match="GPU tensor"):  # CPU tensors are rejected, as everywhere else
            f(adj, ids, ids)
    with pytest.raises(TypeError, match="SparseTensor"):
        psa.negative_sampling(ids, 3)
    with pytest.raises(TypeError, match="SparseTensor"):
        psa.structured_negative_sampling(ids, ids)
    for bad in (ids.float(), ids.bool(), [0, 1], None):
        with pytest.raises(TypeError, match="integer tensor"):
            adj.structured_negative_sampling(bad)
    with pytest.raises(ValueError, match="1-D"):
        adj.structured_negative_sampling(ids.view(2, 2))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        adj.structured_negative_sampling(ids, seed=1)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        adj.negative_sampling(3, seed=1)


@pytest.mark.parametrize("bad", [dict(max_tries=0), dict(max_tries=-1), dict(max_tries=32769), dict(count=-1),
                                 dict(no_self_loops=True, wide=True)])
def test_bad_sampler_arguments_are_refused_before_anything_runs(bad, monkeypatch):
    import torch
    from paddle_sparse_amd import ops

    def never(*a, **k):
        raise AssertionError("reached an op")

    monkeypatch.setattr(ops, "negative_sample", never)
    bad = dict(bad)
    adj = _cpu_adj(4, 5) if bad.pop("wide", False) else _cpu_adj()
    count = bad.pop("count", None)
    with pytest.raises(ValueError, match="negative_sampling"):
        adj.negative_sampling(3 if count is None else count, seed=1, **bad)
    with pytest.raises(ValueError, match="structured_negative_sampling"):
        adj.structured_negative_sampling(torch.arange(4), 1 if count is None else 0, seed=1, **bad)


def test_the_public_functions_reach_the_ops_with_the_arguments_of_the_definition(monkeypatch):
    import torch
    from paddle_sparse_amd import ops

    seen = []

    class _Stop(Exception):
        pass

    def stop(name):
        def f(*a, **k):
            seen.append((name, a))
            raise _Stop

        return f

    monkeypatch.setattr(ops, "negative_sample", stop("negative_sample"))
    monkeypatch.setattr(ops, "edge_lookup", stop("edge_lookup"))
    adj, ids = _cpu_adj(4, 6), torch.arange(4, dtype=torch.int32)
    with pytest.raises(_Stop):
        adj.negative_sampling(7, max_tries=5, seed=3)
    name, a = seen.pop()
    assert name == "negative_sample" and a[2:] == (6, None, 7, False, 5, 3)
    with pytest.raises(_Stop):
        adj.structured_negative_sampling(ids, 2, False, 9, 2**64 - 1)
    name, a = seen.pop()
    assert a[2] == 6 and a[3].dtype == torch.int64 and a[3].tolist() == [0, 1, 2, 3]
    assert a[4:] == (2, False, 9, 2**64 - 1)
    # seed=None draws from torch's CPU generator, as random_walk does
    drawn = []
    for _ in range(2):
        torch.manual_seed(123)
        with pytest.raises(_Stop):
            adj.negative_sampling(1)
        drawn.append(seen.pop()[1][-1])
    with pytest.raises(_Stop):
        adj.negative_sampling(1)
    drawn.append(seen.pop()[1][-1])
    assert drawn[0] == drawn[1] != drawn[2] and all(0 <= s < 2**62 for s in drawn)
    with pytest.raises(_Stop):
        adj.has_edge(ids, ids.to(torch.uint8))
    name, a = seen.pop()
    assert name == "edge_lookup" and a[2] == 6 and a[3].dtype == a[4].dtype == torch.int64 and not seen


def test_ops_check_their_arguments_without_a_device():
    import torch
    from paddle_sparse_amd import ops

    x = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.edge_lookup(x, x, 2, x, x)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.negative_sample(x, x, 2, None, 4, False, 64, 1)
    assert ops._negative_args(4, 4, 3, True, 32768) == (3, 32768)
    for args in ((4, 4, 0, False, 64), (4, 4, 1, False, 0), (4, 4, 1, False, 32769), (4, 5, 1, True, 64)):
        with pytest.raises(ValueError):
            ops._negative_args(*args)
    with pytest.raises(ValueError):
        ops.edge_lookup_host([0, 1], [0], 1, [0, 0], [0])
    with pytest.raises(RuntimeError, match="max_tries"):
        ops.negative_sample_host([0, 1], [0], 1, None, 4, False, 0, 1)
    assert (ops.LOOKUP_RANGE, ops.NEGATIVE_FAILED) == (nr.RANGE, nr.FAILED)
