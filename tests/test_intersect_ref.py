"""CPU: the two restatements of the pair-intersection kernel (tests/intersect_ref.py) against scipy, against
each other and against hand-checked answers; the public names of masked.py.  The GPU suite
(test_masked_spspmm_gpu.py) holds the kernel to these restatements."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from intersect_ref import (GROUP, T, WAVE, abs_term_sum, common_neighbors_ref, csc_of, pair_intersect_math,
                           pair_intersect_ordered, triangle_count_ref)


def csr_arrays(m):
    m = sp.csr_matrix(m)
    m.sum_duplicates()
    m.sort_indices()
    return m.indptr.astype(np.int64), m.indices.astype(np.int64), m.data.copy()


def adjacency(n, edges):
    """Symmetric 0/1 adjacency of an undirected edge list as (rowptr, col)."""
    r = np.array([e[0] for e in edges] + [e[1] for e in edges])
    c = np.array([e[1] for e in edges] + [e[0] for e in edges])
    rowptr, col, _ = csr_arrays(sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n)))
    return rowptr, col


def random_sparse(M, N, density, seed, integer):
    rng = np.random.default_rng(seed)
    m = sp.random(M, N, density=density, random_state=rng, format="csr", dtype=np.float64)
    if integer:  # small and never 0, so that the stored pattern is the pattern of the non-zeros
        m.data = (rng.integers(1, 5, m.nnz) * rng.choice([-1, 1], m.nnz)).astype(np.float64)
    else:
        m.data = rng.standard_normal(m.nnz)
    return m


# a structured pair: a hub row / hub column (long lists against short ones) and empty rows and columns
def structured(M, K, N, seed):
    rng = np.random.default_rng(seed)
    a = random_sparse(M, K, 0.05, seed, True).tolil()
    b = random_sparse(K, N, 0.05, seed + 1, True).tolil()
    a[1, :] = rng.integers(1, 4, K)      # hub row of A
    b[:, 2] = rng.integers(1, 4, (K, 1))  # hub column of B
    a[3, :] = 0
    b[:, 4] = 0
    return sp.csr_matrix(a), sp.csr_matrix(b)


CASES = [
    ("random 40x30x50", lambda integer: (random_sparse(40, 30, 0.2, 1, integer), random_sparse(30, 50, 0.2, 2, integer))),
    ("random 7x300x9", lambda integer: (random_sparse(7, 300, 0.6, 3, integer), random_sparse(300, 9, 0.6, 4, integer))),
    ("square 64", lambda integer: (random_sparse(64, 64, 0.1, 5, integer), random_sparse(64, 64, 0.1, 6, integer))),
    ("structured", lambda integer: structured(20, 200, 25, 7)),
]


def sampled_case(name, make, integer, with_weight):
    a, b = make(integer)
    M, K = a.shape
    N = b.shape[1]
    rng = np.random.default_rng(len(name))
    w = None
    if with_weight:
        w = rng.integers(1, 4, K).astype(np.float64) if integer else rng.standard_normal(K)
    mask = sp.random(M, N, density=0.4, random_state=rng, format="coo")
    mr, mc = mask.row.astype(np.int64), mask.col.astype(np.int64)
    x = csr_arrays(a)
    y = csc_of(*csr_arrays(b), N)
    mid = a if w is None else a @ sp.diags(w)
    want = np.asarray((mid @ b).todense())[mr, mc]
    return x, y, mr, mc, w, want


@pytest.mark.parametrize("with_weight", [False, True])
@pytest.mark.parametrize("name,make", CASES)
def test_math_restatement_is_the_sampled_product(name, make, with_weight):
    x, y, mr, mc, w, want = sampled_case(name, make, True, with_weight)
    got = pair_intersect_math(x, y, mr, mc, w)
    assert got.dtype == np.float64 and np.array_equal(got, want)  # integer-valued: exact in any order
    x, y, mr, mc, w, want = sampled_case(name, make, False, with_weight)
    got = pair_intersect_math(x, y, mr, mc, w)
    mag, cnt = abs_term_sum(x, y, mr, mc, w)
    assert np.all(np.abs(got - want) <= (cnt + 2) * np.finfo(np.float64).eps * mag)
    # the counting form is the pattern product
    pa, pb = (x[0], x[1], None), (y[0], y[1], None)
    counts = pair_intersect_math(pa, pb, mr, mc)
    a, b = make(True)
    pattern = (sp.csr_matrix(a != 0).astype(np.int64) @ sp.csr_matrix(b != 0).astype(np.int64)).todense()
    assert counts.dtype == np.int64 and np.array_equal(counts, np.asarray(pattern)[mr, mc])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name,make", CASES)
def test_ordered_restatement_against_the_math(name, make, dtype):
    for with_weight in (False, True):
        x, y, mr, mc, w, want = sampled_case(name, make, True, with_weight)
        got = pair_intersect_ordered(x, y, mr, mc, w, dtype)
        assert got.dtype == dtype and np.array_equal(got.astype(np.float64), want)
        x, y, mr, mc, w, _ = sampled_case(name, make, False, with_weight)
        # the operands as the ordered form sees them: rounded to dtype first
        x, y = (x[0], x[1], x[2].astype(dtype)), (y[0], y[1], y[2].astype(dtype))
        w = None if w is None else w.astype(dtype)
        got = pair_intersect_ordered(x, y, mr, mc, w, dtype)
        ref = pair_intersect_math(x, y, mr, mc, w)
        mag, cnt = abs_term_sum(x, y, mr, mc, w)
        # two multiplies per term and at most cnt adds on its way to the result
        assert np.all(np.abs(got.astype(np.float64) - ref) <= (cnt + 2) * np.finfo(dtype).eps * mag)
    x, y, mr, mc, _, _ = sampled_case(name, make, True, False)
    pa, pb = (x[0], x[1], None), (y[0], y[1], None)
    assert np.array_equal(pair_intersect_ordered(pa, pb, mr, mc, dtype=np.int64), pair_intersect_math(pa, pb, mr, mc))


def test_ordered_restatement_takes_both_modes_and_the_tie_rule():
    """Lists around T: the long mode differs from the short one in bits on data chosen to show it, and on
    a tie X probes (which decides the order of the partial sums when the lists differ)."""
    assert (T, GROUP, WAVE) == (32, 8, 64)
    rng = np.random.default_rng(0)
    for n in (T, T + 1):
        idx = np.arange(n, dtype=np.int64)
        ptr = np.array([0, n], np.int64)
        v = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
        x, y = (ptr, idx, v), (ptr, idx, np.ones(n, np.float32))
        got = pair_intersect_ordered(x, y, [0], [0])[0]
        W = GROUP if n <= T else WAVE
        lanes = [np.float32(0)] * W
        for i in range(n):
            lanes[i % W] = np.float32(lanes[i % W] + v[i])
        off = 1
        while off < W:
            lanes = [np.float32(lanes[l] + lanes[l ^ off]) for l in range(W)]
            off *= 2
        assert got == lanes[0]
    # out-of-range pairs are 0, in every form
    x = (np.array([0, 2], np.int64), np.array([1, 5], np.int64), None)
    for bad in (-1, 1, 2**40):
        assert pair_intersect_math(x, x, [bad, 0], [0, bad]).tolist() == [0, 0]
        assert pair_intersect_ordered(x, x, [bad, 0], [0, bad], dtype=np.int64).tolist() == [0, 0]


# ---- hand-checked answers --------------------------------------------------------------------------------
TRIANGLE = adjacency(3, [(0, 1), (1, 2), (0, 2)])
STAR = adjacency(5, [(0, 1), (0, 2), (0, 3), (0, 4)])
CLIQUE4 = adjacency(4, [(i, j) for i in range(4) for j in range(i + 1, 4)])
# weighted 3 x 3:  A = [[1, 2, 0], [0, 3, 4], [5, 0, 6]],  B = [[1, 0, 2], [0, 3, 0], [4, 0, 5]],  w = [1, 2, 3]
#   A diag(w) B = [[1, 12, 2], [48, 18, 60], [77, 0, 100]]
W3_A = np.array([[1, 2, 0], [0, 3, 4], [5, 0, 6]], np.float64)
W3_B = np.array([[1, 0, 2], [0, 3, 0], [4, 0, 5]], np.float64)
W3_W = np.array([1, 2, 3], np.float64)
W3_C = np.array([[1, 12, 2], [48, 18, 60], [77, 0, 100]], np.float64)

KAT_GRAPHS = {
    # name: ((rowptr, col), common neighbours of every stored edge, triangles per node)
    "triangle": (TRIANGLE, 1, [1, 1, 1]),
    "star": (STAR, 0, [0, 0, 0, 0, 0]),
    "clique4": (CLIQUE4, 2, [3, 3, 3, 3]),
}


@pytest.mark.parametrize("name", sorted(KAT_GRAPHS))
def test_known_graphs(name):
    (rowptr, col), per_edge, triangles = KAT_GRAPHS[name]
    row = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    assert common_neighbors_ref(rowptr, col, None, row, col).tolist() == [per_edge] * len(col)
    assert triangle_count_ref(rowptr, col).tolist() == triangles
    fam = (rowptr, col, None)
    assert pair_intersect_ordered(fam, fam, row, col, dtype=np.int64).tolist() == [per_edge] * len(col)


def test_known_graphs_beyond_the_edges():
    rowptr, col = STAR
    # two leaves of a star share the centre; the centre shares nothing with a leaf
    assert common_neighbors_ref(rowptr, col, None, [1, 1, 0, 3], [2, 1, 4, 4]).tolist() == [1, 1, 0, 1]


def test_weighted_three_by_three():
    assert np.array_equal(W3_A @ np.diag(W3_W) @ W3_B, W3_C)
    x = csr_arrays(W3_A)
    y = csc_of(*csr_arrays(W3_B), 3)
    r, c = np.divmod(np.arange(9), 3)
    assert pair_intersect_math(x, y, r, c, W3_W).tolist() == W3_C.reshape(-1).tolist()
    for dtype in (np.float32, np.float64):
        assert pair_intersect_ordered(x, y, r, c, W3_W, dtype).tolist() == W3_C.reshape(-1).tolist()
    assert pair_intersect_math(x, y, r, c).tolist() == (W3_A @ W3_B).reshape(-1).tolist()


# ---- the surface ---------------------------------------------------------------------------------
def test_the_ops_are_exported_attached_and_bound():
    from test_abi import declared_functions

    import paddle_sparse_amd as psa
    from paddle_sparse_amd import SparseTensor, _lib, masked, ops

    for name in ("masked_spspmm", "common_neighbors", "triangle_count"):
        assert name in psa.__all__ and getattr(psa, name) is getattr(masked, name)
    assert SparseTensor.common_neighbors is masked.common_neighbors
    assert SparseTensor.triangle_count is masked.triangle_count
    assert callable(SparseTensor.masked_matmul) and callable(ops.pair_intersect)
    assert "psa_pair_intersect" in declared_functions() and "psa_pair_intersect" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), "psa_pair_intersect")
    assert not [n for n in _lib.SIGNATURES if "intersect" in n and n.endswith("_workspace_bytes")]  # no scratch


def test_the_c_abi_refuses_bad_arguments_before_any_launch():
    """Argument checks return before a device is touched: they run without a GPU."""
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    one = ctypes.c_int64(0)
    p = ctypes.addressof(one)
    F32, I64, I32 = 0, 3, 2

    def call(dtype=F32, x_ptr=p, x_idx=p, x_val=None, xl=1, y_ptr=p, y_idx=p, y_val=None, yl=1, weight=None,
             px=p, py=p, P=1, out=p):
        return lib.psa_pair_intersect(dtype, x_ptr, x_idx, x_val, xl, y_ptr, y_idx, y_val, yl, weight, px, py, P, out,
                                      None)

    for kw in (dict(x_ptr=None), dict(x_idx=None), dict(y_ptr=None), dict(y_idx=None), dict(px=None), dict(py=None),
               dict(out=None), dict(P=-1), dict(xl=-1), dict(yl=-1), dict(dtype=I32), dict(dtype=7),
               dict(dtype=I64, x_val=p), dict(dtype=I64, y_val=p), dict(dtype=I64, weight=p)):
        assert call(**kw) == 1, kw
        assert b"psa_pair_intersect" in lib.psa_last_error(), kw
    assert call(P=0, x_ptr=None, x_idx=None, y_ptr=None, y_idx=None, px=None, py=None, out=None) == 0  # nothing to do
