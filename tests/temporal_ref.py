"""temporal_neighbor_sample restated serially in numpy / Python integers: the GPU
suite compares the kernels with it bit for bit, tests/test_zz_temporal_ref.py pins it.  It
never calls the package."""
import numpy as np

from test_walk_saint import randint

STRATEGIES = ("uniform", "last")


def time_of_entries(col, edge_time=None, node_time=None):
    """One time per stored entry: edge_time as it is, or the time of the entry's column."""
    assert (edge_time is None) != (node_time is None)
    if edge_time is not None:
        return [int(t) for t in edge_time]
    node_time = [int(t) for t in node_time]
    return [node_time[c] for c in np.asarray(col, np.int64).tolist()]


def time_order_ref(rowptr, time):
    """(order, sorted_time): inside every row the storage positions ascending by (time, position)."""
    rowptr = np.asarray(rowptr, np.int64).tolist()
    order = []
    for v in range(len(rowptr) - 1):
        order += sorted(range(rowptr[v], rowptr[v + 1]), key=lambda e: (time[e], e))
    return order, [time[e] for e in order]


def eligible_ref(sorted_time, start, deg, bound):
    """c: the entries of the row's segment that are not newer than bound (a prefix: the segment ascends)."""
    return sum(1 for t in sorted_time[start:start + deg] if t <= bound)


def ranks_ref(c, k, replace, strategy, seed, i):
    """Ranks into the eligible prefix picked by the parent at walk index i, in slot order."""
    assert strategy in STRATEGIES and not (strategy == "last" and replace)
    if k < 0:
        return list(range(c))
    if strategy == "last":
        return [c - 1 - t for t in range(min(k, c))]
    if replace:
        return [randint(seed, i, t, c) for t in range(k)] if c > 0 else []
    if c <= k:
        return list(range(c))
    picks = []
    for t in range(k):  # the exact Floyd walk: the draw includes j
        j = c - k + t
        r = randint(seed, i, t, j + 1)
        picks.append(j if r in picks else r)
    return picks


def temporal_walk_ref(rowptr, col, time, seeds, seed_time, num_neighbors, strategy="uniform", replace=False, seed=0):
    """The walk list as [(node or -1, ego, entry or -1)] per hop, empty slots included: hop 0 is
    the seeds (entry -1).  Also returns [(c, k)] of every parent that was expanded."""
    rowptr, col = np.asarray(rowptr, np.int64).tolist(), np.asarray(col, np.int64).tolist()
    N = len(rowptr) - 1
    seeds = np.asarray(seeds, np.int64).tolist()
    seed_time = [int(t) for t in seed_time]
    assert len(seed_time) == len(seeds)
    for s in seeds:
        if s < 0 or s >= N:
            raise IndexError(s)
    order, sorted_time = time_order_ref(rowptr, time)
    hops = [[(s, g, -1) for g, s in enumerate(seeds)]]
    parents_seen = []
    begin = 0
    for k in num_neighbors:
        parents = hops[-1]
        if k == 0 or not parents or not col:
            break
        slots = []
        for f, (v, g, _) in enumerate(parents):
            mine = []
            if v >= 0:
                start, deg = rowptr[v], rowptr[v + 1] - rowptr[v]
                c = eligible_ref(sorted_time, start, deg, seed_time[g])
                parents_seen.append((c, k))
                for r in ranks_ref(c, k, replace, strategy, seed, begin + f):
                    e = order[start + r]
                    mine.append((col[e], g, e))
            if k >= 0:
                assert len(mine) <= k
                mine += [(-1, g, -1)] * (k - len(mine))  # the slots past the picks keep their index
            slots += mine
        begin += len(parents)
        if not slots:
            break
        hops.append(slots)
    return hops, parents_seen


def temporal_neighbor_sample_ref(rowptr, col, time, seeds, seed_time, num_neighbors, strategy="uniform", replace=False,
                                 seed=0, with_walk=False):
    """(n_id, ptr, root, rowptr', col', e_id): the sampled entries, one per distinct (ego, entry)."""
    hops, parents_seen = temporal_walk_ref(rowptr, col, time, seeds, seed_time, num_neighbors, strategy, replace, seed)
    rowptr, col = np.asarray(rowptr, np.int64).tolist(), np.asarray(col, np.int64).tolist()
    seeds = np.asarray(seeds, np.int64).tolist()
    S = len(seeds)
    row_of = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)).tolist()
    nodes, entries = [set() for _ in range(S)], [set() for _ in range(S)]
    for hop in hops:
        for v, g, e in hop:
            if v >= 0:
                nodes[g].add(v)
            if e >= 0:
                entries[g].add(e)
    n_id, ptr, root = [], [0], []
    rows, cols, e_id = [], [], []
    for g in range(S):
        mine = sorted(nodes[g])
        rank = {v: ptr[-1] + j for j, v in enumerate(mine)}
        root.append(rank[seeds[g]])
        for e in sorted(entries[g]):
            rows.append(rank[row_of[e]])
            cols.append(rank[col[e]])
            e_id.append(e)
        n_id += mine
        ptr.append(len(n_id))
    a = lambda x: np.array(x, np.int64)
    new_rowptr = np.searchsorted(a(rows), np.arange(len(n_id) + 1), side="left").astype(np.int64)
    assert rows == sorted(rows) and all(rows[i] < rows[i + 1] or cols[i] <= cols[i + 1] for i in range(len(rows) - 1))
    out = a(n_id), a(ptr), a(root), new_rowptr, a(cols), a(e_id)
    return (out, hops, parents_seen) if with_walk else out
