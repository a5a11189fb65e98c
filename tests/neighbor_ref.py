"""neighbor_sample restated serially in numpy / Python integers: the GPU suite
compares the kernels with it bit for bit, tests/test_neighbor_ref.py pins it."""
import numpy as np

from test_walk_saint import randint


def picks_of_row(start, deg, k, replace, seed, i):
    """Storage positions picked by the node at local id i, in slot order: sample_adj's rules
    with stream i."""
    if k < 0 or (not replace and deg <= k):
        return list(range(start, start + deg))
    if replace:
        return [start + randint(seed, i, t, deg) for t in range(k)] if deg > 0 else []
    picks = []
    for t in range(k):  # Floyd's walk, deg > k
        j = deg - k + t
        e = start + randint(seed, i, t, j)
        picks.append(start + j if e in picks else e)
    return picks


def neighbor_sample_ref(rowptr, col, seeds, num_neighbors, replace=False, seed=0):
    """(n_id, rowptr', col', e_id, nodes_per_hop, edges_per_hop), entries sorted by
    (row', col'), ties in slot order."""
    rowptr, col = np.asarray(rowptr, np.int64).tolist(), np.asarray(col, np.int64).tolist()
    N = len(rowptr) - 1
    n_id, local = [], {}
    for s in np.asarray(seeds, np.int64).tolist():
        if s < 0 or s >= N:
            raise IndexError(s)
        if s in local:
            raise ValueError(s)
        local[s] = len(n_id)
        n_id.append(s)
    rows, cols, edges = [], [], []
    begin, end = 0, len(n_id)
    nodes_per_hop, edges_per_hop = [end], []
    for k in num_neighbors:
        before = len(edges)
        for i in range(begin, end):
            v = n_id[i]
            for e in picks_of_row(rowptr[v], rowptr[v + 1] - rowptr[v], k, replace, seed, i):
                c = col[e]
                j = local.get(c)
                if j is None:
                    j = local[c] = len(n_id)
                    n_id.append(c)
                rows.append(i)
                cols.append(j)
                edges.append(e)
        begin, end = end, len(n_id)
        nodes_per_hop.append(end - begin)
        edges_per_hop.append(len(edges) - before)
    rows, cols, edges = np.array(rows, np.int64), np.array(cols, np.int64), np.array(edges, np.int64)
    order = np.lexsort((cols, rows))  # stable
    new_rowptr = np.searchsorted(rows[order], np.arange(len(n_id) + 1), side="left").astype(np.int64)
    return np.array(n_id, np.int64), new_rowptr, cols[order], edges[order], nodes_per_hop, edges_per_hop
