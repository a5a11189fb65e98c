"""GPU suite for ppr (csrc/ppr.hip).  Integer adds commute, so p and r do not depend on the schedule and
every comparison is bit-exact against the serial restatement of tests/ppr_ref.py (held to dense float64
algebra, and the kernel's steps run on the host held to it, by test_zz_ppr_ref.py), on the case list of
that file: symmetric and directed graphs with a row of N entries, a dangling node and a duplicated entry;
the hub, the dangling node and a repeated node as sources; four (alpha, eps); a source below its own
threshold; max_rounds 1 and 2; a table at the LDS limit and one twice as large, both with a frontier
larger than a chunk and a row longer than the workgroup."""
import numpy as np
import pytest
import torch

import ppr_ref as pr
from test_weighted_walk_gpu import adj_of, gpu

pytestmark = pytest.mark.gpu

_ADJ = {}


def case_adj(kind, N):
    if (kind, N) not in _ADJ:
        _ADJ[kind, N] = adj_of(*pr.graph(kind, N), N=N)
    return _ADJ[kind, N]


def dense(sp, S, N):
    """float64 [S, N] of a result, after checking that its entries are sorted by (row, col) and unique"""
    row, col, val = (x.cpu().numpy() for x in sp.coo())
    assert sp.sparse_sizes() == (S, N) and (np.diff(row * N + col) > 0).all()
    assert np.array_equal(sp.storage.rowcount().cpu().numpy(), np.bincount(row, minlength=S))
    out = np.zeros((S, N), val.dtype)
    out[row, col] = val
    return out


@pytest.mark.parametrize("name", pr.CASES)
def test_case_list_bit_exact(name):
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import ops

    kind, N, sources, alpha, eps, max_rounds = pr.CASES[name]
    want = pr.case_ref(name)
    want_p, want_r = pr.dense_rows(want, N, 0), pr.dense_rows(want, N, 1)
    adj, S, stats = case_adj(kind, N), len(sources), {}
    p, r = adj.ppr(gpu(sources), alpha, eps, return_residual=True, dtype=torch.float64, max_rounds=max_rounds,
                   stats=stats)
    assert np.array_equal(dense(p, S, N), want_p) and np.array_equal(dense(r, S, N), want_r)
    assert stats["rounds"].tolist() == [w[2] for w in want] and stats["pushes"].tolist() == [w[3] for w in want]
    assert stats["edges"].tolist() == [w[4] for w in want]
    assert stats["in_lds"].tolist() == [stats["cap"] <= ops.ppr_lds_cap()] * S
    # float32, the function form, a second run: the same bits, rounded once
    p32 = psa.ppr(adj, gpu(sources), alpha, eps, max_rounds=max_rounds)
    assert p32.storage.value().dtype == torch.float32
    assert np.array_equal(dense(p32, S, N), want_p.astype(np.float32))


def test_case_list_covers_both_builds_and_the_chunk_loop():
    from paddle_sparse_amd import ops
    from paddle_sparse_amd.ppr import quantise, table_cap

    caps = {name: table_cap(c[1], *quantise(c[3], c[4])) for name, c in pr.CASES.items()}
    assert caps["lds_limit"] == ops.ppr_lds_cap() and caps["twice_lds"] == 2 * ops.ppr_lds_cap()
    for name in ("lds_limit", "twice_lds"):  # round 2 of the hub source: more pending slots than its chunk holds
        kind, N, _, alpha, eps, _ = pr.CASES[name]
        aq, eq = pr.quantise(alpha, eps)
        deg = np.diff(pr.graph(kind, N)[0])
        share = (pr.ONE - ((pr.ONE * aq) >> 32)) // N
        assert deg[0] == N and ((deg > 0) & (share >= eq * deg)).sum() > (1024 if name == "lds_limit" else 2048)


def test_batches_reuse_the_slabs():
    kind, N, sources, alpha, eps, _ = pr.CASES["dir300a"]
    want = pr.dense_rows(pr.case_ref("dir300a"), N, 0)
    stats = {}
    p = case_adj(kind, N).ppr(gpu(sources), alpha, eps, dtype=torch.float64, concurrent=2, stats=stats)
    assert stats["batches"] == 3 and np.array_equal(dense(p, len(sources), N), want)


def test_short_table_raises_the_flag_inside_its_slabs():
    from paddle_sparse_amd import ops
    from paddle_sparse_amd.ppr import quantise

    rowptr, col = pr.graph("dir", 300)
    cap, S, guard, poison = 16, 2, 64, -(2**61) - 5
    bufs = [torch.full((guard + S * cap + guard,), poison, dtype=torch.int64, device="cuda") for _ in range(4)]
    tables = tuple(b[guard:guard + S * cap] for b in bufs)
    _, info = ops.ppr_push(gpu(rowptr), gpu(col), 300, gpu([0, 17]), cap, *quantise(0.15, 1e-4), 100, tables)
    info = info.cpu().numpy()
    assert info[3].tolist() == [ops.PPR_TABLE_FULL | ops.PPR_IN_LDS] * 2 and info[6].tolist() == [cap, cap]
    for b in bufs:
        assert (b[:guard] == poison).all() and (b[guard + S * cap:] == poison).all()
    key = tables[0].cpu().numpy()
    assert ((key >= 0) & (key < 300)).all()


@pytest.mark.parametrize("kwargs", [
    dict(alpha=2.0 ** -17), dict(alpha=1 - 2.0 ** -17), dict(eps=2.0 ** -33), dict(eps=1.5),
    dict(source=[0, 300]), dict(source=[-1]), dict(source=torch.zeros(2, dtype=torch.int32)),
])
def test_value_errors(kwargs):
    source = kwargs.pop("source", [0])
    source = source.cuda() if isinstance(source, torch.Tensor) else gpu(source)
    with pytest.raises(ValueError):
        case_adj("dir", 300).ppr(source, **kwargs)


def test_readme_line():
    N = 300
    adj = case_adj("sym", N)
    diffusion = adj.ppr(torch.arange(N, device="cuda"), 0.15, 1e-4)
    gdc = diffusion.topk(64, dim=0)
    sources = list(pr.CASES["sym300a"][2])
    want = pr.dense_rows(pr.case_ref("sym300a"), N, 0).astype(np.float32)
    assert np.array_equal(dense(diffusion, N, N)[sources], want)
    assert gdc.sparse_sizes() == (N, N)
    assert torch.equal(gdc.storage.colcount(), diffusion.storage.colcount().clamp(max=64))
