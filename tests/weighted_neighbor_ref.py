"""Weighted neighbor_sample restated serially: the successive weighted picks
without replacement in plain Python float64 operations, in the order the contract states
them, and neighbor_ref.neighbor_sample_ref with the pick swapped.  The masses are read
afresh from cum at every draw (the kernels split them instead), so agreement bit for bit
also checks that.  Not a test module."""
from bisect import bisect_left, bisect_right

import numpy as np

import neighbor_ref
import weighted_ref as wr
from weighted_ref import M64, mix64


def stream(seed, i):
    return mix64((seed & M64) ^ mix64(i & M64))


def unit(r):
    return float(r >> 11) * 2.0 ** -53


def stream_words(seed, i, k):
    """(words_entry, words_gap) of stream i for a fan-out of k."""
    st = stream(seed, i)
    return [mix64((st + t) & M64) for t in range(k)], [mix64((st + k + t) & M64) for t in range(k)]


def gaps_of(cum, taken):
    """[(lo, hi, base, mass)] of the gaps that the ascending positions `taken` cut the row
    into: positions [lo, hi), base = cum just below, mass 0.0 for an empty gap."""
    bounds = [-1] + list(taken) + [len(cum)]
    out = []
    for g in range(len(bounds) - 1):
        lo, hi = bounds[g] + 1, bounds[g + 1]
        base = cum[lo - 1] if lo > 0 else 0.0
        out.append((lo, hi, base, cum[hi - 1] - base if hi > lo else 0.0))
    return out


def pick_in_gap(cum, lo, hi, base, mass, r):
    """Stage 2: the smallest e in [lo, hi) with cum[e] > base + u * mass, else the smallest
    with cum[e] == cum[hi - 1]."""
    part = unit(r) * mass
    target = base + part
    e = bisect_right(cum, target, lo, hi)
    if e < hi:
        return e
    return min(bisect_left(cum, cum[hi - 1], lo, hi), hi - 1)


def picks_without_words(cum, k, words_entry, words_gap):
    """The picks of one row (cum: a list of floats) in draw order."""
    cum = [float(x) for x in cum]
    taken, out = [], []
    if not cum:
        return out
    for t in range(k):
        gaps = gaps_of(cum, taken)
        run, sums = 0.0, []
        for _, _, _, m in gaps:
            run = run + m
            sums.append(run)
        total = sums[-1]
        if not total > 0.0:
            break
        if len(gaps) == 1:
            g = 0
        else:
            target = unit(words_gap[t]) * total
            g = next((j for j, s in enumerate(sums) if s > target), None)
            if g is None:
                g = max(j for j, gap in enumerate(gaps) if gap[3] > 0.0)
        lo, hi, base, mass = gaps[g]
        assert mass > 0.0
        e = pick_in_gap(cum, lo, hi, base, mass, words_entry[t])
        assert lo <= e < hi and e not in taken and cum[e] > (cum[e - 1] if e > 0 else 0.0)
        out.append(e)
        taken = sorted(taken + [e])
    return out


def picks_without(cum, k, seed, i):
    return picks_without_words(cum, k, *stream_words(seed, i, k))


def positive_entries(cum):
    return sum(1 for e in range(len(cum)) if cum[e] > (cum[e - 1] if e > 0 else 0.0))


def neighbor_sample_ref(rowptr, col, cum, seeds, num_neighbors, replace=False, seed=0):
    """neighbor_ref.neighbor_sample_ref with the picks of every hop with a fan-out >= 0 made
    by the weighted rules: (n_id, rowptr', col', e_id, nodes_per_hop, edges_per_hop)."""
    cum = np.asarray(cum, np.float64)

    def picks_of_row(start, deg, k, replace_, seed_, i):
        if k < 0:
            return list(range(start, start + deg))
        if deg == 0:
            return []
        row = cum[start:start + deg]
        if replace_:
            if not row[-1] > 0:
                return []
            return [start + wr.pick(row, wr.word(seed_, i, t)) for t in range(k)]
        return [start + e for e in picks_without(row.tolist(), k, seed_, i)]

    uniform = neighbor_ref.picks_of_row
    neighbor_ref.picks_of_row = picks_of_row
    try:
        return neighbor_ref.neighbor_sample_ref(rowptr, col, seeds, num_neighbors, replace, seed)
    finally:
        neighbor_ref.picks_of_row = uniform
