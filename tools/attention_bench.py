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

The multi-head lines (H = 8, K = F = 16 and 64: sddmm, the SpMM over per-head values forward and forward +
backward, the whole step) run the one-launch form beside (a) the per-head Python loop over the 2-D ops, slice
copies and the final stack included, and (b) the restatement in torch ops, the three alternating call by call;
each timing is the median with its [min .. max] over the rounds, the spread a difference has to exceed.  Byte
model of DESIGN.md section 3.9: the SpMM reads nnz*(8 + 4H + 4HF) and writes M*4HF, sddmm reads the same and
writes nnz*4H.  A side whose operands or temporaries would not fit the device's free memory is reported as not
run instead of being tried.

The fused lines (--fused: H = 8 with K = F = 16 and 64, H = 1 with K = F = 64) run SparseTensor.attention beside
the chain softmax(sddmm(A, q, k)) @ v it restates, forward and forward + backward, the two alternating call by
call, each with its [min .. max].  Byte model of DESIGN.md section 3.10: the fused forward reads
nnz*(8 + 4HK + 4HF) and writes M*(4HF + 8H); the chain moves nnz*(8*2 + 4H*6) more.  Under each pair the peak of
torch.cuda.max_memory_allocated over one forward + backward of each side, above what was allocated before it.

With --dtype bf16 the fused lines run SparseTensor.attention on bfloat16 q, k, v beside the same op on the fp32
values they were rounded from (the yardstick), the two alternating call by call in the same run, forward and
forward + backward, each with its [min .. max]: a difference counts only where it exceeds that spread.  Byte model
of DESIGN.md section 3.11 for the bf16 forward: reads nnz*(8 + 2HK + 2HF), writes M*(2HF + 8H).  Under each pair
the peak memory of one forward + backward of each side.

With --dropout P the fused lines run SparseTensor.attention(..., dropout_p=P) beside the same op without dropout
and beside the chain with a materialised mask, (att * mask * inv_keep) @ v with the mask of
ops.attention_dropout_mask, alternating call by call, and print the peak memory of one forward + backward of each;
with --dtype bf16 the two fused sides take bfloat16 operands (the chain stays fp32).  Dropout moves no extra bytes
(the mask is recomputed), so the byte model is that of the op without it.

The GAT lines (--gat: H = 8 with F = 16 and 64, H = 1 with F = 64) run SparseTensor.gat_attention beside (a) the
unfused chain it restates (torch indexing for z = a_row[row] + a_col[col], torch.where for the activation,
ops.segment_softmax, ops.spmm_heads; fp32) and (b) the dot-product fused op SparseTensor.attention at K = F on the
same pattern, which moves 4HK more bytes per entry and does the dot: the yardstick of the stage the two share.  The
three alternate call by call, forward and forward + backward, each with its [min .. max].  Byte model of DESIGN.md
section 3.13, e the element size: the forward reads nnz*(8 + e*H + e*H*F) + M*e*H and writes M*(e*H*F + 8H).  Under
each pair the peak memory of one forward + backward of each side.  --dtype bf16 gives the two fused sides bfloat16
operands, --dropout P gives all three the same dropout (the chain with the materialised mask of
ops.attention_dropout_mask).

usage: python tools/attention_bench.py [--quick] [--once] [--heads] [--fused | --gat [--dtype bf16] [--dropout P]]
  --quick  config 3 only;  --once  one call of each of our ops and nothing else (for a kernel trace);
  --heads  the multi-head lines only;  --fused  the fused-attention lines only;  --gat  the GAT lines only;
  --dtype bf16  (with --fused) the bf16 fused op beside the fp32 fused op; (with --gat) bf16 operands
  --dropout P   (with --fused) the fused op with dropout beside the op without and the chain with the same mask;
                (with --gat) dropout P on every side"""
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


def alternate_all(fns):
    """(median, min, max) ms of each callable, all alternating call by call after 3 warm-up calls of each."""
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(ROUNDS):
        for fn, t in zip(fns, times):
            t.append(one_ms(fn))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def fits(nbytes) -> bool:
    torch.cuda.empty_cache()
    return nbytes < 0.8 * torch.cuda.mem_get_info(dev)[0]


def heads_line(label, sides, model_bytes=None):
    """sides: [(name, callable or None)], ours first; a None side is printed as not run."""
    live = [(n, f) for n, f in sides if f is not None]
    res = dict(zip((n for n, _ in live), alternate_all([f for _, f in live])))
    ours = res[sides[0][0]][0]
    parts = []
    for name, fn in sides:
        if fn is None:
            parts.append(f"{name} not run (memory)")
            continue
        med, lo, hi = res[name]
        ratio = "" if name == sides[0][0] else f" x{med / ours:5.2f}" + (" SLOWER" if med < ours else "")
        parts.append(f"{name} {med:9.3f} ms [{lo:.3f} .. {hi:.3f}]{ratio}")
    tail = ""
    if model_bytes is not None:
        rate = model_bytes / (ours * 1e-3)
        tail = f"   model {model_bytes / 1e9:6.3f} GB  {rate / 1e12:5.2f} TB/s = {rate / PEAK:4.2f} of 8 TB/s"
    print(f"   {label:34s} " + "   ".join(parts) + tail, flush=True)


def run_heads(N, rowptr, col, row, gen, once):
    nnz, H = col.numel(), 8
    A = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    A.storage.csr2csc()  # the CSC view of the backward, built once as a training loop has it
    for K in (16, 64):
        F = K
        dense, edge, wide = N * H * K * 4, nnz * H * 4, nnz * H * K * 4
        if not fits(10 * dense + 8 * edge):  # q, k, v, the upstream gradient, three gradients, results of two sides
            print(f"   H = {H}, K = F = {K}: not run, the operands and gradients alone take {10 * dense / 1e9:.0f} GB", flush=True)
            continue
        q = torch.randn((N, H, K), generator=gen, device=dev) * 0.125
        k = torch.randn((N, H, K), generator=gen, device=dev)
        v = torch.randn((N, H, F), generator=gen, device=dev)
        go = torch.randn((N, H, F), generator=gen, device=dev)
        att = psa.sddmm(A, q, k).softmax(dim=1).storage.value()
        Aw = A.set_value(att, layout="coo")

        def per_head(h, qq=q, kk=k):  # one head's scores through the 2-D op (the slices are copied inside it)
            return psa.sddmm(A, qq[:, h], kk[:, h])

        def sddmm_loop():
            return torch.stack([per_head(h).storage.value() for h in range(H)], dim=1)

        def spmm_loop(w=att, vv=v):
            return torch.stack([A.set_value(w[:, h].contiguous(), layout="coo") @ vv[:, h] for h in range(H)], dim=1)

        def spmm_torch(w=att, vv=v):
            return torch.zeros((N, H, F), device=dev).index_add_(0, row, w[:, :, None] * vv[col])

        def with_grad(fn):
            def run():
                w, vv = att.detach().requires_grad_(), v.detach().requires_grad_()
                fn(w, vv).backward(go)
            return run

        def step(kind):
            def run():
                qq, kk, vv = (t.detach().requires_grad_() for t in (q, k, v))
                if kind == "ours":
                    out = psa.sddmm(A, qq, kk).softmax(dim=1) @ vv
                elif kind == "loop":
                    out = torch.stack([per_head(h, qq, kk).softmax(dim=1) @ vv[:, h] for h in range(H)], dim=1)
                else:
                    a = torch_softmax((qq[row] * kk[col]).sum(-1), row, N)
                    out = torch.zeros((N, H, F), device=dev).index_add_(0, row, a[:, :, None] * vv[col])
                out.backward(go)
            return run

        step("ours")()
        if once:
            continue
        print(f"   H = {H}, K = F = {K}: max |one launch - per-head loop| = "
              f"{float((psa.sddmm(A, q, k).storage.value() - sddmm_loop()).abs().max()):.2e} (sddmm), "
              f"{float(((Aw @ v) - spmm_loop()).abs().max()):.2e} (SpMM)", flush=True)
        spmm_bytes = nnz * (8 + 4 * H + 4 * H * F) + N * 4 * H * F
        heads_line(f"sddmm, H = {H}, K = {K}",
                   [("one launch", lambda: psa.sddmm(A, q, k)), ("per-head loop", sddmm_loop),
                    ("torch ops", (lambda: (q[row] * k[col]).sum(-1)) if fits(3 * wide) else None)],
                   nnz * (8 + 4 * H + 4 * H * K) + nnz * 4 * H)
        heads_line(f"SpMM heads forward, F = {F}",
                   [("one launch", lambda: Aw @ v), ("per-head loop", spmm_loop),
                    ("torch ops", spmm_torch if fits(3 * wide) else None)], spmm_bytes)
        heads_line(f"SpMM heads fwd + bwd, F = {F}",
                   [("one launch", with_grad(lambda w, vv: A.set_value(w, layout="coo") @ vv)),
                    ("per-head loop", with_grad(spmm_loop)),
                    ("torch ops", with_grad(spmm_torch) if fits(6 * wide) else None)])
        heads_line(f"attention step fwd + bwd, K = F = {K}",
                   [("one launch", step("ours")), ("per-head loop", step("loop")),
                    ("torch ops", step("torch") if fits(12 * wide) else None)])
        del q, k, v, go, att, Aw
        torch.cuda.empty_cache()


def peak_of(fn) -> float:
    """GB that one call of fn allocates at its peak above what is allocated now."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - base) / 1e9


def run_fused(N, rowptr, col, gen, once):
    nnz = col.numel()
    A = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    A.storage.csr2csc()  # the CSC view of the backward, built once as a training loop has it
    for H, K in ((8, 16), (8, 64), (1, 64)):
        F = K
        dense, edge = N * H * K * 4, nnz * H * 4
        tag = f"H = {H}, K = F = {K}"
        if not fits(8 * dense + 2 * edge):  # q, k, v, the upstream gradient, out, three gradients; p and dS
            print(f"   {tag}: not run, the operands and gradients alone take {8 * dense / 1e9:.0f} GB", flush=True)
            continue
        chain_fits = fits(8 * dense + 8 * edge)  # scores, weights, their gradients and the CSC-ordered copies
        q = torch.randn((N, H, K), generator=gen, device=dev) * 0.125
        k = torch.randn((N, H, K), generator=gen, device=dev)
        v = torch.randn((N, H, F), generator=gen, device=dev)
        go = torch.randn((N, H, F), generator=gen, device=dev)

        def forward(kind, qq=q, kk=k, vv=v):
            if kind == "fused":
                return A.attention(qq, kk, vv)
            return psa.sddmm(A, qq, kk).softmax(dim=1) @ vv

        def step(kind):
            def run():
                qq, kk, vv = (t.detach().requires_grad_() for t in (q, k, v))
                forward(kind, qq, kk, vv).backward(go)
            return run

        step("fused")()
        if once:
            continue
        if chain_fits:
            diff = float((forward("fused") - forward("chain")).abs().max())
            print(f"   {tag}: max |fused - chain| = {diff:.2e}", flush=True)
        fused_bytes = nnz * (8 + 4 * H * K + 4 * H * F) + N * (4 * H * F + 8 * H)
        heads_line(f"attention forward, {tag}",
                   [("fused", lambda: forward("fused")), ("chain", (lambda: forward("chain")) if chain_fits else None)],
                   fused_bytes)
        heads_line(f"attention fwd + bwd, {tag}",
                   [("fused", step("fused")), ("chain", step("chain") if chain_fits else None)])
        peak_c = f"{peak_of(step('chain')):7.3f} GB" if chain_fits else "not run (memory)"
        print(f"   {'peak memory of one fwd + bwd':34s} fused {peak_of(step('fused')):7.3f} GB   chain {peak_c}", flush=True)
        del q, k, v, go
        torch.cuda.empty_cache()


def run_fused_bf16(N, rowptr, col, gen, once):
    """The bf16 fused op ("ours" of each line) beside the fp32 fused op on the same shapes."""
    nnz = col.numel()
    A = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    A.storage.csr2csc()  # the CSC view of the backward, built once as a training loop has it
    for H, K in ((8, 16), (8, 64), (1, 64)):
        F = K
        dense, edge = N * H * K * 4, nnz * H * 4
        tag = f"H = {H}, K = F = {K}"
        if not fits(12 * dense + 2 * edge):  # both sides' operands, upstream gradient, out and gradients; p and dS
            print(f"   {tag}: not run, the operands and gradients alone take {12 * dense / 1e9:.0f} GB", flush=True)
            continue
        sides = {"bf16": tuple(t.to(torch.bfloat16) for t in (
            torch.randn((N, H, K), generator=gen, device=dev) * 0.125, torch.randn((N, H, K), generator=gen, device=dev),
            torch.randn((N, H, F), generator=gen, device=dev), torch.randn((N, H, F), generator=gen, device=dev)))}
        sides["fp32"] = tuple(t.float() for t in sides["bf16"])  # the same values on both sides

        def forward(name):
            q, k, v, _ = sides[name]
            return A.attention(q, k, v)

        def step(name):
            def run():
                q, k, v, go = sides[name]
                qq, kk, vv = (t.detach().requires_grad_() for t in (q, k, v))
                A.attention(qq, kk, vv).backward(go)
            return run

        step("bf16")()
        if once:
            continue
        ref = forward("fp32")
        diff = float(((forward("bf16").float() - ref).abs() / ref.abs().clamp_min(1e-3)).max())
        print(f"   {tag}: max |bf16 - fp32| / max(|fp32|, 1e-3) = {diff:.2e}", flush=True)
        del ref
        half_bytes = nnz * (8 + 2 * H * K + 2 * H * F) + N * (2 * H * F + 8 * H)
        heads_line(f"attention forward, {tag}", [("bf16", lambda: forward("bf16")), ("fp32", lambda: forward("fp32"))],
                   half_bytes)
        heads_line(f"attention fwd + bwd, {tag}", [("bf16", step("bf16")), ("fp32", step("fp32"))])
        print(f"   {'peak memory of one fwd + bwd':34s} bf16 {peak_of(step('bf16')):7.3f} GB   "
              f"fp32 {peak_of(step('fp32')):7.3f} GB", flush=True)
        del sides
        torch.cuda.empty_cache()


def run_fused_dropout(N, rowptr, col, gen, once, drop, half):
    """The fused op with dropout ("ours" of each line) beside the fused op without it and beside the chain with a
    materialised mask, (att * mask * inv_keep) @ v, the mask from ops.attention_dropout_mask under the same seed.
    The chain is fp32; with --dtype bf16 it is fed the fp32 copies of the same values."""
    nnz = col.numel()
    A = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    A.storage.csr2csc()  # the CSC view of the backward, built once as a training loop has it
    seed, inv_keep = 12345, float(torch.tensor(1.0 / (1.0 - drop), dtype=torch.float32))
    dt = torch.bfloat16 if half else torch.float32
    for H, K in ((8, 16), (8, 64), (1, 64)):
        F = K
        dense, edge = N * H * K * 4, nnz * H * 4
        tag = f"H = {H}, K = F = {K}, dropout {drop}"
        if not fits((12 if half else 8) * dense + 2 * edge):
            print(f"   {tag}: not run, the operands and gradients alone do not fit", flush=True)
            continue
        chain_fits = fits((12 if half else 8) * dense + 10 * edge)  # as --fused, plus the mask and the masked weights
        q, k, v, go = (t.to(dt) for t in (
            torch.randn((N, H, K), generator=gen, device=dev) * 0.125, torch.randn((N, H, K), generator=gen, device=dev),
            torch.randn((N, H, F), generator=gen, device=dev), torch.randn((N, H, F), generator=gen, device=dev)))
        q32, k32, v32, go32 = ((t.float() for t in (q, k, v, go)) if half else (q, k, v, go))

        def forward(kind, qq=None, kk=None, vv=None):
            if kind == "chain":
                qq, kk, vv = (q32, k32, v32) if qq is None else (qq, kk, vv)
                mask = ops.attention_dropout_mask(nnz, H, drop, seed)
                att = psa.sddmm(A, qq, kk).softmax(dim=1)
                return att.set_value(att.storage.value() * mask * inv_keep, layout="coo") @ vv
            qq, kk, vv = (q, k, v) if qq is None else (qq, kk, vv)
            return A.attention(qq, kk, vv, dropout_p=drop if kind == "dropout" else 0.0, seed=seed)

        def step(kind):
            def run():
                src = (q32, k32, v32) if kind == "chain" else (q, k, v)
                qq, kk, vv = (t.detach().requires_grad_() for t in src)
                forward(kind, qq, kk, vv).backward(go32 if kind == "chain" else go)
            return run

        step("dropout")()
        if once:
            continue
        if chain_fits:
            diff = float((forward("dropout").float() - forward("chain")).abs().max())
            print(f"   {tag}: max |fused - chain with the same mask| = {diff:.2e}", flush=True)
        width = 2 if half else 4
        model = nnz * (8 + width * H * K + width * H * F) + N * (width * H * F + 8 * H)  # dropout moves no extra bytes
        heads_line(f"attention forward, {tag}",
                   [("dropout", lambda: forward("dropout")), ("plain", lambda: forward("plain")),
                    ("masked chain", (lambda: forward("chain")) if chain_fits else None)], model)
        heads_line(f"attention fwd + bwd, {tag}",
                   [("dropout", step("dropout")), ("plain", step("plain")),
                    ("masked chain", step("chain") if chain_fits else None)])
        peak_c = f"{peak_of(step('chain')):7.3f} GB" if chain_fits else "not run (memory)"
        print(f"   {'peak memory of one fwd + bwd':34s} dropout {peak_of(step('dropout')):7.3f} GB   "
              f"plain {peak_of(step('plain')):7.3f} GB   masked chain {peak_c}", flush=True)
        del q, k, v, go, q32, k32, v32, go32
        torch.cuda.empty_cache()


def run_gat(N, rowptr, col, gen, once, half, drop):
    """gat_attention ("ours" of each line) beside the unfused chain and the dot-product fused op at K = F."""
    nnz = col.numel()
    A = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    st = A.storage
    csc = (st.colptr(), st._row_in_csc_order(), st.csr2csc())  # the CSC view of the backward, built once for every side
    row = None
    p_drop = 0.0 if drop is None else drop
    seed, inv_keep = 12345, float(torch.tensor(1.0 / (1.0 - p_drop), dtype=torch.float32))
    dt = torch.bfloat16 if half else torch.float32
    e = 2 if half else 4
    for H, F in ((8, 16), (8, 64), (1, 64)):
        K = F
        dense, edge = N * H * F * 4, nnz * H * 4
        tag = f"H = {H}, F = {F}" + ("" if drop is None else f", dropout {drop}") + (", bf16" if half else "")
        if not fits(5 * dense + 2 * edge):  # v, the upstream gradient, out, grad_v and a transient; p and dZ
            print(f"   {tag}: not run, the operands and gradients alone take {5 * dense / 1e9:.0f} GB", flush=True)
            continue
        dot_fits = fits(10 * dense + 2 * edge)  # q, k and their gradients on top
        chain_fits = fits((7 if half else 5) * dense + 10 * edge + nnz * 8)  # z, s, the weights, their gradients, row
        a_row = (torch.randn((N, H), generator=gen, device=dev)).to(dt)
        a_col = (torch.randn((N, H), generator=gen, device=dev)).to(dt)
        v = torch.randn((N, H, F), generator=gen, device=dev).to(dt)
        go = torch.randn((N, H, F), generator=gen, device=dev).to(dt)
        if dot_fits:
            q = (torch.randn((N, H, K), generator=gen, device=dev) * 0.125).to(dt)
            k = torch.randn((N, H, K), generator=gen, device=dev).to(dt)
        if chain_fits:
            if row is None:
                row = ops.ptr2ind(rowptr, nnz)
            r32, c32, v32, go32 = ((t.float() for t in (a_row, a_col, v, go)) if half else (a_row, a_col, v, go))

        def forward(kind, rr=None, cc=None, vv=None):
            if kind == "gat":
                rr, cc, vv = (a_row, a_col, v) if rr is None else (rr, cc, vv)
                return A.gat_attention(rr, cc, vv, dropout_p=p_drop, seed=seed)
            if kind == "dot":  # rr, cc stand for q, k
                rr, cc, vv = (q, k, v) if rr is None else (rr, cc, vv)
                return A.attention(rr, cc, vv, dropout_p=p_drop, seed=seed)
            rr, cc, vv = (r32, c32, v32) if rr is None else (rr, cc, vv)
            z = rr[row] + cc[col]
            att = ops.segment_softmax(torch.where(z > 0, z, 0.2 * z), rowptr)
            if drop is not None:
                att = att * ops.attention_dropout_mask(nnz, H, p_drop, seed) * inv_keep
            return ops.spmm_heads(rowptr, col, att, vv, csc=csc)

        def step(kind):
            def run():
                src = {"gat": lambda: (a_row, a_col, v), "dot": lambda: (q, k, v), "chain": lambda: (r32, c32, v32)}[kind]()
                rr, cc, vv = (t.detach().requires_grad_() for t in src)
                forward(kind, rr, cc, vv).backward(go32 if kind == "chain" else go)
            return run

        step("gat")()
        if once:
            continue
        if chain_fits:
            diff = float((forward("gat").float() - forward("chain")).abs().max())
            print(f"   {tag}: max |gat - chain| = {diff:.2e}", flush=True)
        model = nnz * (8 + e * H + e * H * F) + N * e * H + N * (e * H * F + 8 * H)
        heads_line(f"gat forward, {tag}",
                   [("gat", lambda: forward("gat")), ("chain", (lambda: forward("chain")) if chain_fits else None),
                    ("dot fused", (lambda: forward("dot")) if dot_fits else None)], model)
        heads_line(f"gat fwd + bwd, {tag}",
                   [("gat", step("gat")), ("chain", step("chain") if chain_fits else None),
                    ("dot fused", step("dot") if dot_fits else None)])
        peak_c = f"{peak_of(step('chain')):7.3f} GB" if chain_fits else "not run (memory)"
        peak_d = f"{peak_of(step('dot')):7.3f} GB" if dot_fits else "not run (memory)"
        print(f"   {'peak memory of one fwd + bwd':34s} gat {peak_of(step('gat')):7.3f} GB   chain {peak_c}   "
              f"dot fused {peak_d}", flush=True)
        del a_row, a_col, v, go
        if dot_fits:
            del q, k
        if chain_fits:
            del r32, c32, v32, go32
        torch.cuda.empty_cache()


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


def run(name, make, once, heads_only=False, fused_only=False, half=False, drop=None, gat_only=False):
    N, rowptr, col = make()
    nnz = col.numel()
    row = ops.ptr2ind(rowptr, nnz)
    deg = rowptr[1:] - rowptr[:-1]
    print(f"== {name}: {N} x {N}, {nnz} entries, longest row {int(deg.max())}, "
          f"{int((deg > 128).sum())} rows above 128 entries", flush=True)
    gen = torch.Generator(device=dev).manual_seed(9)
    if gat_only:
        del row
        run_gat(N, rowptr, col, gen, once, half, drop)
        return
    if fused_only:
        del row
        if drop is not None:
            run_fused_dropout(N, rowptr, col, gen, once, drop, half)
        else:
            (run_fused_bf16 if half else run_fused)(N, rowptr, col, gen, once)
        return
    if heads_only:
        run_heads(N, rowptr, col, row, gen, once)
        return
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
    del A, q, k, val, go, s
    torch.cuda.empty_cache()
    run_heads(N, rowptr, col, row, gen, once)
    del rowptr, col, row
    torch.cuda.empty_cache()


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}", flush=True)
    once = "--once" in sys.argv
    heads_only = "--heads" in sys.argv
    fused_only = "--fused" in sys.argv
    gat_only = "--gat" in sys.argv
    if gat_only and (fused_only or heads_only):
        sys.exit("--gat goes alone, with --dtype, --dropout, --quick and --once")
    half = False
    if "--dtype" in sys.argv:
        dtype = sys.argv[sys.argv.index("--dtype") + 1:][:1]
        if dtype not in (["bf16"], ["fp32"]) or not (fused_only or gat_only):
            sys.exit("--dtype takes bf16 or fp32 and goes with --fused or --gat")
        half = dtype == ["bf16"]
    drop = None
    if "--dropout" in sys.argv:
        arg = sys.argv[sys.argv.index("--dropout") + 1:][:1]
        try:
            drop = float(arg[0])
        except (IndexError, ValueError):
            drop = -1.0
        if not 0.0 < drop < 1.0 or not (fused_only or gat_only):
            sys.exit("--dropout takes a probability in (0, 1) and goes with --fused or --gat")
    run("config-3 shape", config3, once, heads_only, fused_only, half, drop, gat_only)
    if "--quick" not in sys.argv:
        run("R-MAT 24", rmat24, once, heads_only, fused_only, half, drop, gat_only)
