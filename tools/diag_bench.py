#!/usr/bin/env python3
"""remove_diag / fill_diag / get_diag on the config-3 shape (2 M x 2 M, 20 M entries, columns
sorted inside rows) and on R-MAT 24 (bench.rmat_graph(24, 100 M)), against the same semantics
written with torch ops on the GPU (upstream torch_sparse/diag.py: masks over every entry,
boolean indexing, and for fill_diag a stable re-sort of the concatenated keys).  Both sides
are checked bit-equal first.  HIP-event means; the end-to-end calls include the one host
read of the output size.  Byte model (DESIGN.md "Diagonal ops"): rowptr, col and values read
once, rowptr', rowcount', col' and values' written once.

usage: python tools/diag_bench.py [--quick]   (--quick: config 3 only)"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bench import event_ms, rmat_graph  # noqa: E402
import paddle_sparse_amd as psa  # noqa: E402
from paddle_sparse_amd import SparseTensor, ops  # noqa: E402

dev = torch.device("cuda", 0)
REPS = 10


def torch_remove(rowptr, row, col, val, M, k=0):
    mask = col != row + k
    new_row = row[mask]
    ptr = torch.zeros(M + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(torch.bincount(new_row, minlength=M), 0)
    return ptr, col[mask], val[mask]


def torch_fill(rowptr, row, col, val, M, N, fill=1.0, k=0):
    start, nd = ops.diag_extent(M, N, k)
    mask = col != row + k
    d = torch.arange(start, start + nd, device=dev)
    keys = torch.cat([row[mask] * N + col[mask], d * N + d + k])
    vals = torch.cat([val[mask], torch.full((nd,), fill, dtype=val.dtype, device=dev)])
    keys, order = torch.sort(keys, stable=True)
    ptr = torch.zeros(M + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(torch.bincount(keys // N, minlength=M), 0)
    return ptr, keys % N, vals[order]


def torch_get_diag(row, col, val, M, N):
    out = torch.zeros(min(M, N), dtype=val.dtype, device=dev)
    mask = row == col
    out[row[mask]] = val[mask]  # upstream's index_put (its winner among duplicates is unspecified on a GPU)
    return out


def config3():
    M = N = 2_000_000
    g = torch.Generator(device=dev).manual_seed(3)
    keys = torch.sort(torch.randint(0, M, (20_000_000,), generator=g, device=dev) * N
                      + torch.randint(0, N, (20_000_000,), generator=g, device=dev))[0]
    row, col = keys // N, keys % N
    del keys
    return M, N, ops.ind2ptr(row, M), row, col, torch.randn(col.numel(), generator=g, device=dev)


def rmat24():
    N, rowptr, row, col, val = rmat_graph(24, 100_000_000, dev)
    return N, N, rowptr, row, col, val


def model_bytes(M, nnz, nnz_out, value_bytes=4):
    read = 8 * (M + 1) + (8 + value_bytes) * nnz
    written = 8 * (M + 1) + 8 * M + (8 + value_bytes) * nnz_out
    return read, written


def run(name, make):
    M, N, rowptr, row, col, val = make()
    nnz = col.numel()
    a = SparseTensor(rowptr=rowptr, col=col, value=val, sparse_sizes=(M, N), is_sorted=True, trust_data=True)
    rows_with_diag = int((col == row).sum().item())
    print(f"== {name}: {M} x {N}, {nnz} entries, {rows_with_diag} on the main diagonal, longest row "
          f"{int((rowptr[1:] - rowptr[:-1]).max().item())}", flush=True)

    f = psa.fill_diag(a, 1.0)
    p, c, v = torch_fill(rowptr, row, col, val, M, N)
    assert torch.equal(f.storage.rowptr(), p) and torch.equal(f.storage.col(), c) and torch.equal(f.storage.value(), v)
    r = psa.remove_diag(a)
    p, c, v = torch_remove(rowptr, row, col, val, M)
    assert torch.equal(r.storage.rowptr(), p) and torch.equal(r.storage.col(), c) and torch.equal(r.storage.value(), v)
    assert torch.equal(psa.get_diag(a), torch_get_diag(row, col, val, M, N))  # coalesced: one entry per cell
    nnz_fill, nnz_rm = f.nnz(), r.nnz()
    del f, r, p, c, v
    print("   results bit-equal to the torch composition", flush=True)

    def line(op, ours, theirs, nnz_out=None):
        extra = ""
        if nnz_out is not None:
            rd, wr = model_bytes(M, nnz, nnz_out)
            extra = (f"  model {rd / 1e9:.2f} GB read + {wr / 1e9:.2f} GB written -> {(rd + wr) / ours / 1e9:5.2f} TB/s "
                     f"({(rd + wr) / ours / 1e9 / 8 * 100:4.1f} % of 8 TB/s)")
        print(f"   {op:32s} {ours:8.3f} ms   torch ops {theirs:8.3f} ms   x{theirs / ours:5.1f}{extra}", flush=True)

    with torch.no_grad():
        line("fill_diag(A, 1) end to end", event_ms(lambda: psa.fill_diag(a, 1.0), REPS),
             event_ms(lambda: torch_fill(rowptr, row, col, val, M, N), REPS), nnz_fill)
        line("remove_diag(A) end to end", event_ms(lambda: psa.remove_diag(a), REPS),
             event_ms(lambda: torch_remove(rowptr, row, col, val, M), REPS), nnz_rm)
        line("get_diag(A)", event_ms(lambda: psa.get_diag(a), REPS),
             event_ms(lambda: torch_get_diag(row, col, val, M, N), REPS))
        # the two passes of fill_diag on their own (count + scan; the write pass alone)
        plan = ops.diag_count(rowptr, col, M, N, 0, True)
        ones = torch.ones(M, device=dev)
        lib = ops._lib.load()
        rc, rp_out = plan.rowcount, plan.rowptr

        def count_only():
            ops.check(lib.psa_diag_count(rowptr.data_ptr(), col.data_ptr(), M, N, 0, 1, None, rc.data_ptr(),
                                         rp_out.data_ptr(), None, plan.ws.data_ptr(), plan.ws.numel(), ops._stream()))

        t_count = event_ms(count_only, REPS)
        t_write = event_ms(lambda: ops.diag_write(plan, rowptr, col, val, ones), REPS)
        rd, wr = model_bytes(M, nnz, nnz_fill)
        print(f"   fill_diag passes: count + scan {t_count:.3f} ms, write {t_write:.3f} ms; kernel sum "
              f"{t_count + t_write:.3f} ms -> {(rd + wr) / (t_count + t_write) / 1e9:5.2f} TB/s on the model "
              f"({(rd + wr) / (t_count + t_write) / 1e9 / 8 * 100:4.1f} % of 8 TB/s)", flush=True)
    del a, rowptr, row, col, val, plan
    torch.cuda.empty_cache()


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}", flush=True)
    run("config-3 shape", config3)
    if "--quick" not in sys.argv:
        run("R-MAT 24", rmat24)
