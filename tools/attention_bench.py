#!/usr/bin/env python3
"""The attention path — SparseTensor.softmax, sddmm and one step softmax(sddmm(A, q, k)) @ v,
forward and backward — on the config-3 shape (2 M x 2 M, 20 M entries) and R-MAT 24
(bench.rmat_graph(24, 100 M)), each beside the cheapest restatement in torch ops on the GPU:

  softmax   m = zeros.scatter_reduce(row, "amax", include_self=False); e = exp(v - m[row]);
            out = e / zeros.index_add(row, e)[row]                      (backward: y * (g - index_add(y * g)[row]))
  sddmm     (x[row] * y[col]).sum(1)                                    (two nnz x K temporaries)
  step      the two above and torch.sparse.mm-free aggregation: zeros.index_add(row, a[:, None] * v[col])

The two sides of a line are timed alternately in one process: warm-up 3, then ROUNDS rounds of
one HIP-event-timed call each, medians reported.  Beside each of our timings the byte model of
DESIGN.md section 3.8 (forward nnz*4D read + nnz*4D written + (M+1)*8; backward 2*nnz*4D read + nnz*4D
written) as achieved bytes/s and as a fraction of 8 TB/s.  Results are compared where the restatement
is deterministic enough to (max relative difference printed; the torch side adds with atomics).

usage: python tools/attention_bench.py [--quick] [--once]
  --quick  config 3 only;  --once  one call of each of our ops and nothing else (for a kernel trace)"""
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bench import rmat_graph  # noqa: E402
import paddle_sparse_amd as psa  # noqa: E402
from paddle_sparse_amd import SparseTensor, ops  # noqa: E402

dev = torch.device("cuda", 0)
PEAK = 8e12
ROUNDS = 11


def one_ms(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(ours, theirs):
    """Median ms of each, the two alternating call by call after 3 warm-up calls of each."""
    for _ in range(3):
        ours()
        theirs()
    torch.cuda.synchronize()
    t_o, t_t = [], []
    for _ in range(ROUNDS):
        t_o.append(one_ms(ours))
        t_t.append(one_ms(theirs))
    return statistics.median(t_o), statistics.median(t_t)


def line(label, t_ours, t_theirs, model_bytes=None):
    tail = ""
    if model_bytes is not None:
        rate = model_bytes / (t_ours * 1e-3)
        tail = f"   model {model_bytes / 1e9:6.3f} GB  {rate / 1e12:5.2f} TB/s = {rate / PEAK:4.2f} of 8 TB/s"
    verdict = "" if t_ours <= t_theirs else "   SLOWER"
    print(f"   {label:40s} {t_ours:9.3f} ms   torch ops {t_theirs:9.3f} ms   x{t_theirs / t_ours:5.2f}{tail}{verdict}",
          flush=True)


def torch_softmax(v, row, M):
    shape = (M,) + tuple(v.shape[1:])
    m = torch.zeros(shape, device=dev).scatter_reduce(0, row.view((-1,) + (1,) * (v.dim() - 1)).expand_as(v), v, "amax",
                                                      include_self=False)
    e = torch.exp(v - m[row])
    return e / torch.zeros(shape, device=dev).index_add_(0, row, e)[row]


def torch_softmax_bw(y, g, row, M):
    yg = y * g
    dot = torch.zeros((M,) + tuple(y.shape[1:]), device=dev).index_add_(0, row, yg)
    return y * (g - dot[row])


def torch_sddmm(row, col, x, y):
    return (x[row] * y[col]).sum(1)


def config3():
    M = 2_000_000
    g = torch.Generator(device=dev).manual_seed(3)
    keys = torch.sort(torch.randint(0, M, (20_000_000,), generator=g, device=dev) * M
                      + torch.randint(0, M, (20_000_000,), generator=g, device=dev))[0]
    row, col = keys // M, keys % M
    del keys
    return M, ops.ind2ptr(row, M), col


def rmat24():
    N, rowptr, row, col, _ = rmat_graph(24, 100_000_000, dev)
    del row
    return N, rowptr, col


def run(name, make, once):
    N, rowptr, col = make()
    nnz = col.numel()
    row = ops.ptr2ind(rowptr, nnz)
    deg = rowptr[1:] - rowptr[:-1]
    print(f"== {name}: {N} x {N}, {nnz} entries, longest row {int(deg.max())}, "
          f"{int((deg > 128).sum())} rows above 128 entries", flush=True)
    gen = torch.Generator(device=dev).manual_seed(9)
    for D in (1, 8):
        shape = (nnz,) if D == 1 else (nnz, D)
        v = torch.randn(shape, generator=gen, device=dev)
        g = torch.randn(shape, generator=gen, device=dev)
        a = SparseTensor(rowptr=rowptr, col=col, value=v, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
        y = a.softmax(1).storage.value()
        gs = ops.segment_softmax_bw(y, g, rowptr)
        if once:
            continue
        ref = torch_softmax(v, row, N)
        print(f"   D = {D}: max |ours - torch| / torch = {float(((y - ref).abs() / ref).max()):.2e} (forward), "
              f"{float((gs - torch_softmax_bw(y, g, row, N)).abs().max()):.2e} absolute (backward)", flush=True)
        del ref
        t_o, t_t = alternate(lambda: a.softmax(1), lambda: torch_softmax(v, row, N))
        line(f"softmax forward, D = {D}", t_o, t_t, 2 * nnz * 4 * D + (N + 1) * 8)
        t_o, t_t = alternate(lambda: ops.segment_softmax_bw(y, g, rowptr), lambda: torch_softmax_bw(y, g, row, N))
        line(f"softmax backward, D = {D}", t_o, t_t, 3 * nnz * 4 * D)
        del a, y, gs
    del v, g
    K = 64
    q = torch.randn((N, K), generator=gen, device=dev) * 0.125
    k = torch.randn((N, K), generator=gen, device=dev)
    val = torch.randn((N, K), generator=gen, device=dev)
    go = torch.randn((N, K), generator=gen, device=dev)
    A = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    A.storage.csr2csc()  # the CSC view of the backward, built once as a training loop has it
    s = psa.sddmm(A, q, k).storage.value()

    def step_ours():
        qq, kk, vv = (t.detach().requires_grad_() for t in (q, k, val))
        out = psa.softmax(psa.sddmm(A, qq, kk), 1) @ vv
        out.backward(go)
        return out

    def step_torch():
        qq, kk, vv = (t.detach().requires_grad_() for t in (q, k, val))
        att = torch_softmax(torch_sddmm(row, col, qq, kk), row, N)
        out = torch.zeros((N, K), device=dev).index_add_(0, row, att[:, None] * vv[col])
        out.backward(go)
        return out

    step_ours()
    if not once:
        ref = torch_sddmm(row, col, q, k)
        print(f"   sddmm K = {K}: max |ours - torch| = {float((s - ref).abs().max()):.2e}", flush=True)
        del ref
        t_o, t_t = alternate(lambda: psa.sddmm(A, q, k), lambda: torch_sddmm(row, col, q, k))
        line(f"sddmm forward, K = {K}", t_o, t_t)
        t_o, t_t = alternate(step_ours, step_torch)
        line(f"attention step fwd + bwd, K = {K}", t_o, t_t)
    del A, q, k, val, go, s, rowptr, col, row
    torch.cuda.empty_cache()


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}", flush=True)
    once = "--once" in sys.argv
    run("config-3 shape", config3, once)
    if "--quick" not in sys.argv:
        run("R-MAT 24", rmat24, once)
