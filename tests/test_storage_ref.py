"""CPU: the plain reference of a storage's derived state (tests/storage_ref.py) against hand-written
matrices, scipy.sparse and — once — the oracle's restatement of the reference class.  No GPU."""
import numpy as np
import pytest
import scipy.sparse

from storage_ref import derived


def eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b)


def test_hand_written_matrix_with_empty_row_empty_column_and_duplicate():
    #      c0 c1 c2 c3
    # r0 [  .  a  .  b ]
    # r1 [  .  .  .  . ]      empty row; column 2 is empty; (2, 1) is stored twice
    # r2 [  c d,e .  . ]
    # r3 [  f  .  .  g ]
    row = [0, 0, 2, 2, 2, 3, 3]
    col = [1, 3, 0, 1, 1, 0, 3]
    d = derived(row, col, 4, 4)
    assert d.sorted
    assert eq(d.rowcount, [2, 0, 3, 2]) and eq(d.rowptr, [0, 2, 2, 5, 7])
    assert eq(d.colcount, [2, 3, 0, 2]) and eq(d.colptr, [0, 2, 5, 5, 7])
    # CSC order: column 0 = entries 2 (r2), 5 (r3); column 1 = 0 (r0), 3, 4 (r2, in CSR order); column 3 = 1, 6
    assert eq(d.csr2csc, [2, 5, 0, 3, 4, 1, 6])
    assert eq(d.csc2csr, [2, 5, 0, 3, 4, 1, 6])  # this permutation happens to be an involution
    assert eq(d.row_csc, [2, 3, 0, 2, 2, 0, 3]) and eq(d.col_csc, [0, 0, 1, 1, 1, 3, 3])
    # position inside the CSR row: entry 2 is the first of row 2, entry 5 the first of row 3, ...
    assert eq(d.edge_tags(1), np.array([0, 0, 0, 1, 2, 1, 1], np.uint8)) and d.edge_tags(1).dtype == np.uint8
    assert eq(d.edge_tags(2), np.array([0, 0, 0, 1, 2, 1, 1], np.int16)) and d.edge_tags(2).dtype == np.int16
    assert d.longest_row == 3
    assert eq(d.mean_scale, np.float32(1) / np.array([2, 2, 3, 3, 3, 2, 2], np.float32)) and d.mean_scale.dtype == np.float32


def test_non_involutive_permutation_and_its_inverse():
    # r0: c2 ; r1: c0, c1 ; r2: c0   -> CSC order: (r1,c0)=1, (r2,c0)=3, (r1,c1)=2, (r0,c2)=0
    d = derived([0, 1, 1, 2], [2, 0, 1, 0], 3, 3)
    assert eq(d.csr2csc, [1, 3, 2, 0])
    assert eq(d.csc2csr, [3, 0, 2, 1])
    assert eq(d.csr2csc[d.csc2csr], np.arange(4)) and eq(d.csc2csr[d.csr2csc], np.arange(4))


def test_unsorted_input_is_reported():
    assert not derived([1, 0], [0, 0], 2, 1).sorted
    assert not derived([0, 0], [1, 0], 1, 2).sorted
    assert derived([0, 0], [1, 1], 1, 2).sorted  # duplicates are non-decreasing


@pytest.mark.parametrize("M,N", [(0, 0), (0, 5), (5, 0), (3, 4)])
def test_no_entries_and_zero_sizes(M, N):
    d = derived([], [], M, N)
    assert d.sorted and d.nnz == 0 and d.longest_row == 0
    assert eq(d.rowptr, np.zeros(M + 1, np.int64)) and eq(d.colptr, np.zeros(N + 1, np.int64))
    assert eq(d.rowcount, np.zeros(M, np.int64)) and eq(d.colcount, np.zeros(N, np.int64))
    for a in (d.csr2csc, d.csc2csr, d.row_csc, d.col_csc, d.edge_tags(1), d.edge_tags(2), d.mean_scale):
        assert a.size == 0
    assert d.rowptr.dtype == np.int64 and d.csr2csc.dtype == np.int64


def test_edge_tags_of_rows_around_the_one_byte_limit():
    # row 0: 128 entries (one byte exact, no flag), row 1: 129 (flagged, index mod 128), row 2: 300
    deg = [128, 129, 300]
    row = np.repeat(np.arange(3), deg)
    col = np.concatenate([np.arange(n) for n in deg])
    d = derived(row, col, 3, 300)
    t1, t2 = d.edge_tags(1), d.edge_tags(2)
    local = col[d.csr2csc]  # col == position inside the row here
    r = d.row_csc
    assert eq(t2, local.astype(np.int16))
    assert eq(t1[r == 0], local[r == 0])
    assert eq(t1[r == 1], (local[r == 1] % 128) | 0x80)
    assert eq(t1[r == 2], (local[r == 2] % 128) | 0x80)
    assert int(t1[(r == 1) & (local == 128)][0]) == 0x80  # the 129th entry wraps to 0, flag kept
    assert d.longest_row == 300


def test_two_byte_tags_wrap_as_a_bit_pattern():
    n = 40000
    d = derived(np.zeros(n, np.int64), np.arange(n), 1, n)
    t2 = d.edge_tags(2)
    assert int(t2[32767]) == 32767 and int(t2[32768]) == -32768 and int(t2[n - 1]) == n - 1 - 65536


@pytest.mark.parametrize("seed", range(6))
def test_against_scipy(seed):
    rng = np.random.default_rng(seed)
    M, N = int(rng.integers(1, 40)), int(rng.integers(1, 40))
    nnz = int(rng.integers(0, 3 * M * N // 2 + 1))  # with duplicates
    key = np.sort(rng.integers(0, M * N, nnz))
    row, col = key // N, key % N
    d = derived(row, col, M, N)
    assert d.sorted
    # scipy's CSR -> CSC conversion is a stable counting sort by column that keeps duplicates (COO -> CSC
    # would add them up): with the entry id as data it returns csr2csc itself
    indptr = np.searchsorted(row, np.arange(M + 1), side="left")
    csr = scipy.sparse.csr_matrix((np.arange(nnz, dtype=np.int64), col, indptr), shape=(M, N))
    csc = csr.tocsc()
    assert csc.nnz == nnz
    assert eq(d.colptr, csc.indptr) and eq(d.row_csc, csc.indices) and eq(d.csr2csc, csc.data)
    assert eq(d.rowptr, csr.indptr)
    assert eq(d.rowcount, np.diff(csr.indptr)) and eq(d.colcount, np.diff(csc.indptr))
    assert eq(np.sort(d.csc2csr), np.arange(nnz)) and eq(d.csr2csc[d.csc2csr], np.arange(nnz))


def test_against_the_oracle_once():
    """Second opinion: oracle/storage_oracle.py restates the reference class (its csr2csc sorts the
    key M * col + row, its csc2csr sorts csr2csc); both must describe the same state."""
    from oracle import storage_oracle as so

    rng = np.random.default_rng(99)
    M, N = 37, 23
    key = np.sort(rng.integers(0, M * N, 700))  # duplicates included
    row, col = key // N, key % N
    d, o = derived(row, col, M, N), so.Storage(row, col, None, (M, N), is_sorted=True)
    assert eq(d.rowptr, o.rowptr()) and eq(d.rowcount, o.rowcount())
    assert eq(d.colptr, o.colptr()) and eq(d.colcount, o.colcount())
    assert eq(d.csr2csc, o.csr2csc()) and eq(d.csc2csr, o.csc2csr())
