#!/usr/bin/env python3
"""edge_ids, structured_negative_sampling and negative_sampling against the torch-ops form a user
writes today, on the config-3 shape (2 M x 2 M, 20 M entries) and R-MAT 24 (bench.rmat_graph(24,
100 M)), both symmetrised (every entry stored both ways, coalesced) as in tools/node2vec_bench.py.

Workloads, each timed ALTERNATELY with its torch form on the same inputs, several rounds, so that
drift hits both alike; per form the median and the range of the rounds are printed:

  lookup, random pairs    edge_ids on 1 M uniform random pairs (nearly all absent)
  lookup, stored edges    edge_ids on 1 M stored entries drawn at random
  structured              structured_negative_sampling, every stored entry's row as src, k = 1
  global                  negative_sampling of nnz pairs

The torch form: the stored entries as linearised keys row * N + col (sorted; built ONCE, outside the
timed region, in the torch form's favour), a query as torch.searchsorted on the queries' keys and a
compare.  For the samplers it is ONE round of draw (torch.randint), lookup and mask, which leaves a
user with a boolean mask and the retries still to do; the kernels' time includes every retry.  The
linearised key overflows int64 once M * N passes 2^63; both graphs are far below that.

Next to each sampler: the mean tries per sample, from the serial restatement (tests/negative_ref.py)
on the first samples, which are first held to the kernel's output bit for bit; and the lookups are
held to the torch form on all queries.

Model of a lookup: the query pair (16 B, coalesced), the rowptr pair, about
ceil(log2(deg + 1)) dependent 8-byte loads in the row, 8 B out.

usage: python tools/negative_sample_bench.py [--quick]   (--quick: config 3 only)"""
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from bench import event_ms  # noqa: E402
import negative_ref as nr  # noqa: E402
from node2vec_bench import config3, rmat24  # noqa: E402
from paddle_sparse_amd import SparseTensor  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS, Q, SAMPLE = 3, 1_000_000, 2000
REPS_LOOKUP, REPS_SAMPLE = 200, 10  # launches per timed window: tens of milliseconds each


def torch_lookup(keys, N, row, col):
    """Position of (row, col) among the sorted keys, -1 where absent: what a user writes today."""
    q = row * N + col
    pos = torch.searchsorted(keys, q).clamp_(max=keys.numel() - 1)
    return torch.where(keys[pos] == q, pos, -1)


def run(name, make):
    N, rowptr, col = make()
    nnz = col.numel()
    a = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    deg = rowptr[1:] - rowptr[:-1]
    print(f"== {name}, symmetrised: {N} nodes, {nnz} entries, {int((deg == 0).sum())} without entries, "
          f"longest row {int(deg.max())}", flush=True)
    seed = 20261021
    g = torch.Generator(device=dev).manual_seed(7)
    with torch.no_grad():
        row = a.storage.row()
        keys = row * N + col  # sorted: the matrix is
        rq, cq = (torch.randint(0, N, (Q,), generator=g, device=dev) for _ in range(2))
        e = torch.randint(0, nnz, (Q,), generator=g, device=dev)
        rs, cs = row[e].contiguous(), col[e].contiguous()
        for r, c in ((rq, cq), (rs, cs)):
            assert torch.equal(a.edge_ids(r, c, trust_data=True), torch_lookup(keys, N, r, c))
        assert bool((a.edge_ids(rs, cs, trust_data=True) == e).all())  # coalesced: the position drawn
        depth = float(torch.ceil(torch.log2(deg[rs].double() + 1)).mean())
        depth_q = float(torch.ceil(torch.log2(deg[rq].double() + 1)).mean())

        # the samplers, held to the restatement on their first samples
        rowptr_np, col_np = rowptr.cpu().numpy(), col.cpu().numpy()
        stats_s, stats_g = {}, {}
        want = nr.ref_negative_sample(rowptr_np, col_np, N, N, row[:SAMPLE].cpu().numpy(), 1, False, 64, seed, stats_s)
        got = a.structured_negative_sampling(row[:SAMPLE], seed=seed, trust_data=True)
        assert np.array_equal(got.cpu().numpy().reshape(-1), want[1])
        want = nr.ref_negative_sample(rowptr_np, col_np, N, N, None, SAMPLE, False, 64, seed, stats_g)
        got = a.negative_sampling(nnz, seed=seed)
        assert np.array_equal(got[0][:SAMPLE].cpu().numpy(), want[0])
        assert np.array_equal(got[1][:SAMPLE].cpu().numpy(), want[1])
        failed = int((got[1] < 0).sum())
        del rowptr_np, col_np, got

        def torch_structured():
            c = torch.randint(0, N, (nnz,), generator=g, device=dev)
            return c, torch_lookup(keys, N, row, c) < 0

        def torch_global():
            r = torch.randint(0, N, (nnz,), generator=g, device=dev)
            c = torch.randint(0, N, (nnz,), generator=g, device=dev)
            return r, c, torch_lookup(keys, N, r, c) < 0

        work = {
            "lookup, random pairs": (Q, f"search depth {depth_q:5.2f}",
                                     lambda: a.edge_ids(rq, cq, trust_data=True), lambda: torch_lookup(keys, N, rq, cq)),
            "lookup, stored edges": (Q, f"search depth {depth:5.2f}",
                                     lambda: a.edge_ids(rs, cs, trust_data=True), lambda: torch_lookup(keys, N, rs, cs)),
            "structured": (nnz, f"tries/sample {stats_s['tries'] / SAMPLE:5.3f}",
                           lambda: a.structured_negative_sampling(row, seed=seed, trust_data=True), torch_structured),
            "global": (nnz, f"tries/sample {stats_g['tries'] / SAMPLE:5.3f}, {failed} of {nnz} failed",
                       lambda: a.negative_sampling(nnz, seed=seed), torch_global),
        }
        times = {(k, side): [] for k in work for side in ("hip", "torch")}
        for _ in range(ROUNDS):
            for k, (n, _, hip, ref) in work.items():
                for side, fn in (("hip", hip), ("torch", ref)):
                    fn()  # warm-up: the allocator has the blocks afterwards
                    times[(k, side)].append(event_ms(fn, REPS_LOOKUP if n == Q else REPS_SAMPLE))
        print(f"   ms per call over {ROUNDS} alternating rounds of {REPS_LOOKUP} (lookups) or {REPS_SAMPLE} (samplers) calls; "
              f"ratio = median of the HIP op over median of the torch form (samplers: ONE draw / lookup / mask round of it):",
              flush=True)
        for k, (n, note, _, _) in work.items():
            base = statistics.median(times[(k, "torch")])
            for side in ("hip", "torch"):
                ts = times[(k, side)]
                med = statistics.median(ts)
                print(f"     {k:22s} {side:6s} n = {n:10d}   median {med:9.3f}   range {min(ts):9.3f} .. {max(ts):9.3f}   "
                      f"x{med / base:6.2f}   {n / med / 1e6:8.3f} G/s   {note if side == 'hip' else ''}", flush=True)
    del a, rowptr, col, row, keys
    torch.cuda.empty_cache()


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}", flush=True)
    run("config-3 shape", config3)
    if "--quick" not in sys.argv:
        run("R-MAT 24", rmat24)
