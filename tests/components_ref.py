"""Weakly connected components restated serially in numpy (csrc/union_find.h, csrc/components.hip),
with the graphs and the case table that the CPU suite (the host export) and the GPU suite (the
kernels) both run.  Both compare bit for bit with ref_components; tests/test_zz_components_ref.py
pins it to hand-checked answers and to scipy.  Not a test module.

A case is (N, row, col): an edge list in the order it was written down, as data.  case_graph puts
it into the order a SparseTensor stores, sorted by (row, col) — except the case "unsorted", which
is sorted by row only: a SparseTensor built from (rowptr, col) with is_sorted=True holds the
columns of a row in whatever order they were given (rows out of order it cannot hold: rowptr would
not describe them), and the components must not depend on it."""
import functools

import numpy as np

RANGE = 1  # bit of flags
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1000)


# ---- the restatement -------------------------------------------------------------------------------
def ref_roots(N, row, col):
    """(root int64[N], flags): union by smaller root over the entries in order, then flatten.  An
    entry with an end outside [0, N) is skipped and sets RANGE."""
    parent, flags = list(range(N)), 0

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for u, v in zip(np.asarray(row, np.int64).tolist(), np.asarray(col, np.int64).tolist()):
        if not (0 <= u < N and 0 <= v < N):
            flags |= RANGE
            continue
        a, b = find(u), find(v)
        if a != b:
            parent[max(a, b)] = min(a, b)
    for v in range(N):  # ascending: parent[v] < v is flat already
        parent[v] = parent[parent[v]]
    return np.array(parent, np.int64).reshape(-1), flags


def ref_components(N, row, col):
    """(n, labels int64[N], root int64[N], flags): labels[i] = the rank of i's root among the roots."""
    root, flags = ref_roots(N, row, col)
    is_root = root == np.arange(N)
    rank = np.concatenate([[0], np.cumsum(is_root)]).astype(np.int64)
    return int(rank[N]), rank[root], root, flags


def ref_largest(n, labels, k):
    """The ascending nodes of the k largest components; of two of one size the smaller label first."""
    sizes = np.bincount(labels, minlength=n)
    keep = sorted(range(n), key=lambda c: (-int(sizes[c]), c))[:k]
    return np.flatnonzero(np.isin(labels, keep)).astype(np.int64)


# ---- the graphs --------------------------------------------------------------------------------------
def _path(order):
    return order[:-1], order[1:]


def _grid(side, rng):
    ids = rng.permutation(side * side).reshape(side, side)
    row = np.concatenate([ids[:, :-1].ravel(), ids[:-1, :].ravel()])
    col = np.concatenate([ids[:, 1:].ravel(), ids[1:, :].ravel()])
    return row, col


def _clique(nodes):
    u, v = np.meshgrid(nodes, nodes, indexing="ij")
    keep = u != v
    return u[keep], v[keep]


def _edges(name):
    """(N, row, col) as written down: directed entries, any order."""
    rng = np.random.default_rng(sum(name.encode()) + 1000 * len(name))
    e = lambda *pairs: (np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64))  # noqa: E731
    if name.startswith("size_"):  # N nodes and nnz random entries, both from SIZES
        N, nnz = (int(x) for x in name.split("_")[1:])
        return N, rng.integers(0, max(N, 1), nnz), rng.integers(0, max(N, 1), nnz)
    if name == "no_edges":
        return 70, *e()
    if name == "self_loops":
        return 70, np.arange(70), np.arange(70)
    if name == "duplicates":
        return 9, *e((1, 5), (1, 5), (5, 1), (1, 5), (7, 8), (7, 8), (3, 3), (3, 3), (8, 7))
    if name == "hi_lo":  # one directed edge, stored only as (hi, lo)
        return 6, *e((4, 1))
    if name == "lo_hi":
        return 6, *e((1, 4))
    if name == "triangles":  # two triangles and four isolated nodes: a tie in size
        return 10, *e((1, 3), (3, 8), (8, 1), (2, 6), (6, 7), (2, 7))
    if name == "path_identity":
        return 20000, *_path(np.arange(20000))
    if name == "path_reversed":
        return 20000, *_path(np.arange(20000)[::-1])
    if name == "path_shuffled":
        return 20000, *_path(rng.permutation(20000))
    if name == "star_hub_first":
        return 3000, np.zeros(2999, np.int64), np.arange(1, 3000)
    if name == "star_hub_last":
        return 3000, np.full(2999, 2999), np.arange(2999)
    if name == "matching":
        p = rng.permutation(2000)
        return 2000, p[:1000], p[1000:]
    if name == "grid":
        return 4096, *_grid(64, rng)
    if name == "cliques":  # {0 .. 39, 80} and {40 .. 79}; (80, 79) is the last entry of the storage and the only join
        a, b = _clique(np.r_[np.arange(40), 80]), _clique(np.arange(40, 80))
        return 81, np.r_[a[0], b[0], 80], np.r_[a[1], b[1], 79]
    if name == "random":  # about N / 2 components, the largest of about a thousand nodes
        N = 20000
        return N, rng.integers(0, N, N // 2), rng.integers(0, N, N // 2)
    if name == "unsorted":  # three entries per row on average, their columns left in the order drawn
        return 3000, rng.integers(0, 3000, 9000), rng.integers(0, 3000, 9000)
    raise KeyError(name)


CASES = tuple(f"size_{k}_{k}" for k in SIZES) + tuple(f"size_1000_{k}" for k in SIZES[:-1]) + (
    "size_257_1000", "no_edges", "self_loops", "duplicates", "hi_lo", "lo_hi", "triangles", "path_identity",
    "path_reversed", "path_shuffled", "star_hub_first", "star_hub_last", "matching", "grid", "cliques", "random",
    "unsorted")

# hand answers: name -> (n, labels)
TINY = {
    "duplicates": (7, [0, 1, 2, 3, 4, 1, 5, 6, 6]),
    "hi_lo": (5, [0, 1, 2, 3, 1, 4]),
    "lo_hi": (5, [0, 1, 2, 3, 1, 4]),
    "triangles": (6, [0, 1, 2, 1, 3, 4, 2, 2, 1, 5]),
    "size_1_1": (1, [0]),
    "size_0_0": (0, []),
}


def _read_only(*arrays):
    out = tuple(np.ascontiguousarray(a, np.int64) for a in arrays)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case_edges(name):
    N, row, col = _edges(name)
    return (N,) + _read_only(row, col)


@functools.lru_cache(maxsize=None)
def case_graph(name):
    """(N, rowptr, row, col) in the order a SparseTensor stores."""
    N, row, col = case_edges(name)
    order = np.argsort(row, kind="stable") if name == "unsorted" else np.lexsort((col, row))
    row, col = row[order], col[order]
    rowptr = np.searchsorted(row, np.arange(N + 1), side="left")
    return (N,) + _read_only(rowptr, row, col)


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """ref_components of the case in storage order, computed once."""
    N, _, row, col = case_graph(name)
    n, labels, root, flags = ref_components(N, row, col)
    return (n,) + _read_only(labels, root) + (flags,)
