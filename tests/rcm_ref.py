"""Reference for reverse_cuthill_mckee, in numpy / plain Python, and the
graphs the CPU and GPU suites share.

Definition: deg[i] = rowptr[i+1] - rowptr[i] (stored duplicates and a stored diagonal
count).  Components one at a time; the seed of the next one is the unvisited node with
the smallest (deg, id); from the seed, nodes are taken in order and each appends its
not-yet-visited neighbours sorted by (deg, id), once.  perm is that order reversed.
"""
import numpy as np


def cuthill_mckee(rowptr, col):
    """The serial form: the order itself (not reversed), int64[N]."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    N = len(rowptr) - 1
    deg = np.diff(rowptr)
    seeds = np.lexsort((np.arange(N), deg))
    visited = np.zeros(N, bool)
    order = []
    si = 0
    while len(order) < N:
        while visited[seeds[si]]:
            si += 1
        s = int(seeds[si])
        visited[s] = True
        head = len(order)
        order.append(s)
        while head < len(order):
            v = order[head]
            head += 1
            nb = np.unique(col[rowptr[v]:rowptr[v + 1]])
            nb = nb[~visited[nb]]
            nb = nb[np.lexsort((nb, deg[nb]))]
            visited[nb] = True
            order.extend(nb.tolist())
    return np.asarray(order, np.int64)


def reverse_cuthill_mckee(rowptr, col):
    return cuthill_mckee(rowptr, col)[::-1].copy()


def cuthill_mckee_levels(rowptr, col):
    """The level-synchronous form, written independently of the serial one: the nodes found
    by one breadth-first level, ordered by (position of the earliest-placed parent, deg, id)."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    N = len(rowptr) - 1
    deg = [int(rowptr[i + 1] - rowptr[i]) for i in range(N)]
    by_degree = sorted(range(N), key=lambda i: (deg[i], i))
    rank = [-1] * N
    order = []
    for s in by_degree:
        if rank[s] >= 0:
            continue
        rank[s] = len(order)
        order.append(s)
        level = [s]
        while level:
            parent = {}
            for v in level:
                for c in col[rowptr[v]:rowptr[v + 1]].tolist():
                    if rank[c] < 0:
                        parent[c] = min(parent.get(c, rank[v]), rank[v])
            level = sorted(parent, key=lambda c: (parent[c], deg[c], c))
            for c in level:
                rank[c] = len(order)
                order.append(c)
    return np.asarray(order, np.int64)


def bandwidth(rowptr, col, perm=None):
    """max |row - col| over the stored entries of permute(A, perm) (of A itself without perm)."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    N = len(rowptr) - 1
    if len(col) == 0:
        return 0
    row = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))
    if perm is not None:
        inv = np.empty(N, np.int64)
        inv[np.asarray(perm, np.int64)] = np.arange(N, dtype=np.int64)
        row, col = inv[row], inv[col]
    return int(np.abs(row - col).max())


# ---- graphs ---------------------------------------------------------------------------

def csr_of(N, row, col):
    """Sorted CSR of the given entries (duplicates kept)."""
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    o = np.lexsort((col, row))
    row, col = row[o], col[o]
    return np.searchsorted(row, np.arange(N + 1), side="left").astype(np.int64), col


def undirected(N, edges, relabel=None):
    """Sorted CSR of the undirected edges (each stored both ways, duplicates removed);
    relabel: a permutation applied to the node ids."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    if relabel is not None:
        e = np.asarray(relabel, np.int64)[e]
    both = np.concatenate([e, e[:, ::-1]])
    both = np.unique(both, axis=0) if len(both) else both
    return csr_of(N, both[:, 0], both[:, 1])


KAT_N = 9
KAT_EDGES = [(0, 3), (0, 5), (1, 2), (1, 4), (1, 6), (2, 4), (3, 5), (3, 7), (5, 7), (6, 4)]
KAT_ROWPTR = [0, 2, 5, 7, 10, 13, 16, 18, 20, 20]
KAT_COL = [3, 5, 2, 4, 6, 1, 4, 0, 5, 7, 1, 2, 6, 0, 3, 7, 1, 4, 3, 5]
KAT_PERM = [6, 4, 1, 2, 7, 5, 3, 0, 8]


def path_graph(n, seed):
    lab = np.random.default_rng(seed).permutation(n)
    return undirected(n, [(i, i + 1) for i in range(n - 1)], lab)


def grid_graph(n, seed):
    """n x n five-point grid with shuffled labels."""
    lab = np.random.default_rng(seed).permutation(n * n)
    idx = np.arange(n * n).reshape(n, n)
    edges = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], 1),
                            np.stack([idx[:-1].ravel(), idx[1:].ravel()], 1)])
    return undirected(n * n, edges, lab)


def random_symmetric(N, per_row, seed):
    rng = np.random.default_rng(seed)
    m = N * per_row // 2
    return undirected(N, np.stack([rng.integers(0, N, m), rng.integers(0, N, m)], 1))


def symmetrised(rowptr, col):
    """Pattern of A + A^T, duplicates removed."""
    N = len(rowptr) - 1
    row = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))
    return undirected(N, np.stack([row, np.asarray(col, np.int64)], 1))
