#!/usr/bin/env python3
"""adj.ppr against dense power iteration through the package's own spmm, on the config-3 shape (2 M x 2 M)
and R-MAT 24, both symmetrised as in tools/node2vec_bench.py.

For S in {1024, 16384} random sources and (alpha, eps) in {(0.15, 1e-4), (0.25, 1e-4)} the op is timed by
the wall clock (it reads the host once per batch) ALTERNATELY with the dense form, several rounds, medians
and ranges printed.  The dense form pushes 256 sources at a time as an [N, 256] fp32 operand:
r <- (1 - alpha) * A (D^-1 r), p += alpha * r, until every column's residual mass is below eps (checked
every 4 products, one host read each); its time is scaled to S sources.  It is a different approximation
(a global stop on the mass, not a per-node threshold), so only the times are compared.

Per run the op's stats are printed: rounds, pushes and integer atomics per source, the share of sources
whose table ran in LDS, the table size, batches and host reads.

usage: python tools/ppr_bench.py [--quick]   (--quick: config 3, S = 1024 only)"""
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from node2vec_bench import config3, rmat24  # noqa: E402
from paddle_sparse_amd import SparseTensor  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS, WIDTH = 3, 256


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def power_iteration(a, inv_deg, source, alpha, eps):
    """(p [N, WIDTH], products): dense PPR columns of WIDTH sources"""
    N = inv_deg.numel()
    r = torch.zeros((N, source.numel()), device=dev)
    r[source, torch.arange(source.numel(), device=dev)] = 1.0
    p, products = alpha * r, 0
    while True:
        for _ in range(4):
            r = (1 - alpha) * (a @ (r * inv_deg[:, None]))
            p += alpha * r
            products += 1
        if float(r.sum(0).max()) < eps:
            return p, products


def run(name, make, sizes):
    N, rowptr, col = make()
    a = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    ones = SparseTensor(rowptr=rowptr, col=col, value=torch.ones(col.numel(), device=dev), sparse_sizes=(N, N),
                        is_sorted=True, trust_data=True)
    deg = (rowptr[1:] - rowptr[:-1]).float()
    inv_deg = torch.where(deg > 0, 1 / deg, torch.zeros_like(deg))
    print(f"== {name}, symmetrised: {N} nodes, {col.numel()} entries, longest row {int(deg.max())}", flush=True)
    gen = torch.Generator(device=dev).manual_seed(11)
    with torch.no_grad():
        for S in sizes:
            source = torch.randint(0, N, (S,), device=dev, generator=gen)
            for alpha, eps in ((0.15, 1e-4), (0.25, 1e-4)):
                stats, products = {}, []
                op = lambda: a.ppr(source, alpha, eps, stats=stats)  # noqa: E731
                ref = lambda: products.append(power_iteration(ones, inv_deg, source[:WIDTH], alpha, eps)[1])  # noqa: E731
                op(), ref()  # warm-up
                t_op, t_ref = [], []
                for _ in range(ROUNDS):
                    t_op.append(wall_ms(op))
                    t_ref.append(wall_ms(ref) * S / WIDTH)
                out = a.ppr(source, alpha, eps, stats=stats)
                m_op, m_ref = statistics.median(t_op), statistics.median(t_ref)
                mean = lambda k: float(stats[k].double().mean())  # noqa: E731
                print(f"   S = {S:6d} alpha = {alpha} eps = {eps}: ppr {m_op:9.2f} ms ({min(t_op):.2f} .. {max(t_op):.2f}), "
                      f"dense power iteration {m_ref:9.2f} ms ({min(t_ref):.2f} .. {max(t_ref):.2f}; {products[-1]} products "
                      f"per {WIDTH} sources, scaled), ratio x{m_op / m_ref:.3f}\n"
                      f"      per source: {out.nnz() / S:.1f} entries, {mean('rounds'):.1f} rounds, {mean('pushes'):.1f} pushes, "
                      f"{mean('edges'):.1f} atomics, {mean('touched'):.1f} slots used; in LDS {mean('in_lds'):.3f}; "
                      f"cap {stats['cap']}, {stats['batches']} batches, {stats['host_reads']} host reads", flush=True)
    del a, ones
    torch.cuda.empty_cache()


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}", flush=True)
    quick = "--quick" in sys.argv
    run("config-3 shape", config3, (1024,) if quick else (1024, 16384))
    if not quick:
        run("R-MAT 24", rmat24, (1024, 16384))
