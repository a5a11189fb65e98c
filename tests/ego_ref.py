"""ego_k_hop_sample restated serially in numpy / Python integers: the GPU suite
compares the kernels with it bit for bit, tests/test_ego_ref.py pins it.  It never calls the
package."""
import numpy as np

from neighbor_ref import picks_of_row


def ego_walk_ref(rowptr, col, seeds, num_neighbors, replace=False, seed=0):
    """The walk list as [(node or -1, ego)] per hop, empty slots included: hop 0 is the seeds."""
    rowptr, col = np.asarray(rowptr, np.int64).tolist(), np.asarray(col, np.int64).tolist()
    N = len(rowptr) - 1
    seeds = np.asarray(seeds, np.int64).tolist()
    for s in seeds:
        if s < 0 or s >= N:
            raise IndexError(s)
    hops = [[(s, g) for g, s in enumerate(seeds)]]
    begin = 0
    for k in num_neighbors:
        parents = hops[-1]
        if k == 0 or not parents:
            break
        slots = []
        for f, (v, g) in enumerate(parents):
            picks = []
            if v >= 0:
                picks = picks_of_row(rowptr[v], rowptr[v + 1] - rowptr[v], k, replace, seed, begin + f)
            mine = [(col[e], g) for e in picks]
            if k >= 0:
                assert len(mine) <= k
                mine += [(-1, g)] * (k - len(mine))  # the slots past the picks keep their index
            slots += mine
        begin += len(parents)
        if not slots:
            break
        hops.append(slots)
    return hops


def ego_k_hop_sample_ref(rowptr, col, seeds, num_neighbors, replace=False, seed=0):
    """(n_id, ptr, root, rowptr', col', e_id)."""
    hops = ego_walk_ref(rowptr, col, seeds, num_neighbors, replace, seed)
    rowptr, col = np.asarray(rowptr, np.int64).tolist(), np.asarray(col, np.int64).tolist()
    seeds = np.asarray(seeds, np.int64).tolist()
    S = len(seeds)
    sets = [set() for _ in range(S)]
    for hop in hops:
        for v, g in hop:
            if v >= 0:
                sets[g].add(v)
    n_id, ptr, root = [], [0], []
    new_rowptr, new_col, e_id = [0], [], []
    for g in range(S):
        nodes = sorted(sets[g])
        rank = {v: ptr[-1] + j for j, v in enumerate(nodes)}
        root.append(rank[seeds[g]])
        for v in nodes:
            for e in range(rowptr[v], rowptr[v + 1]):
                if col[e] in rank:
                    new_col.append(rank[col[e]])
                    e_id.append(e)
            new_rowptr.append(len(new_col))
        n_id += nodes
        ptr.append(len(n_id))
    a = lambda x: np.array(x, np.int64)
    return a(n_id), a(ptr), a(root), a(new_rowptr), a(new_col), a(e_id)
