"""CPU suite for ppr: the host export psa_ppr_host (the kernel's own steps of csrc/ppr_step.h, run
serially) against the serial restatement of tests/ppr_ref.py, bit for bit, and the restatement against
dense float64 linear algebra.  No GPU is needed."""
import numpy as np
import pytest

import ppr_ref as pr


def table_rows(key, val):
    """[{node: value}] of the positive entries of every slab"""
    return [{int(k): int(x) for k, x in zip(ks, xs) if k >= 0 and x} for ks, xs in zip(key, val)]


@pytest.mark.parametrize("name", pr.CASES)
def test_host_export_is_the_restatement(name):
    from paddle_sparse_amd import ops
    from paddle_sparse_amd import ppr as _  # noqa: F401  (the function; the module is imported below)
    import sys

    ppr = sys.modules['paddle_sparse_amd.ppr']

    kind, N, sources, alpha, eps, max_rounds = pr.CASES[name]
    rowptr, col = pr.graph(kind, N)
    aq, eq = ppr.quantise(alpha, eps)
    assert (aq, eq) == pr.quantise(alpha, eps) and ppr.work_bound(aq, eq) == pr.bound(aq, eq)
    cap = ppr.table_cap(N, aq, eq)
    assert cap & (cap - 1) == 0 and cap >= 2 * min(N, 1 + pr.bound(aq, eq)) > cap // 2
    rounds = pr.bound(aq, eq) + 1 if max_rounds is None else max_rounds
    key, r, p, info = ops.ppr_host(rowptr, col, N, sources, cap, aq, eq, rounds)
    want = pr.case_ref(name)
    assert table_rows(key, p) == [w[0] for w in want]
    assert table_rows(key, r) == [w[1] for w in want]
    assert info[2].tolist() == [w[2] for w in want] and info[3].tolist() == [0] * len(sources)
    assert info[4].tolist() == [w[3] for w in want] and info[5].tolist() == [w[4] for w in want]
    assert info[0].tolist() == [len(w[0]) for w in want] and info[1].tolist() == [len(w[1]) for w in want]


def test_host_export_short_table_raises_the_flag():
    from paddle_sparse_amd import ops
    from paddle_sparse_amd import ppr as _  # noqa: F401  (the function; the module is imported below)
    import sys

    ppr = sys.modules['paddle_sparse_amd.ppr']

    rowptr, col = pr.graph("dir", 300)
    aq, eq = ppr.quantise(0.15, 1e-4)
    key, r, p, info = ops.ppr_host(rowptr, col, 300, [0, 17], 16, aq, eq, 100)
    assert info[3].tolist() == [ops.PPR_TABLE_FULL] * 2 and info[6].tolist() == [16, 16]
    with pytest.raises(ops.HipCoreError):
        ops.ppr_host(rowptr, col, 300, [0], 24, aq, eq, 100)  # no power of two


@pytest.mark.parametrize("name", [n for n, c in pr.CASES.items() if c[1] <= 300 and c[5] is None])
def test_restatement_against_dense_float64(name):
    """p + r @ Pi == Pi[s] up to (pushes + edges) * 2^-48 + 1e-13: the flooring of every push (one unit
    for keep, at most one per entry for share) plus float64 rounding at N <= 300.  On symmetric graphs
    also 0 <= Pi[s] - p <= eps * max(deg, 1) plus that slack.  alpha is the quantised one throughout."""
    kind, N, sources, alpha, eps, _ = pr.CASES[name]
    rowptr, col = pr.graph(kind, N)
    aq, eq = pr.quantise(alpha, eps)
    a = aq / 2**32  # the quantised alpha: exact in a double
    deg = np.diff(rowptr)
    P = np.zeros((N, N))
    np.add.at(P, (np.repeat(np.arange(N), deg), col), 1.0)
    P[deg == 0, np.flatnonzero(deg == 0)] = 1.0  # a dangling row is a self loop
    P /= np.maximum(deg, 1)[:, None]
    Pi = a * np.linalg.inv(np.eye(N) - (1 - a) * P)
    rows = pr.case_ref(name)
    p, r = pr.dense_rows(rows, N, 0), pr.dense_rows(rows, N, 1)
    for i, s in enumerate(sources):
        slack = (rows[i][3] + rows[i][4]) * 2.0**-48 + 1e-13
        err = np.abs(p[i] + r[i] @ Pi - Pi[s]).max()
        print(f"{name} source {s}: error {err:.3e}, bound {slack:.3e}")
        assert err <= slack
        if kind == "sym":
            gap = Pi[s] - p[i]
            print(f"  largest gap / (eps * deg) = {(gap / (eps * np.maximum(deg, 1))).max():.3f}")
            assert (gap >= -slack).all() and (gap <= eps * np.maximum(deg, 1) + slack).all()
