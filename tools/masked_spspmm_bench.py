#!/usr/bin/env python3
"""masked_spspmm / common_neighbors (csrc/intersect.hip) against what a user had before:

  (A @ A) . A      config-3 shape (2 M x 2 M, 20 M entries, uniform) and R-MAT 21: `masked_spspmm(A, A, A)` against
                   `A @ A` (spspmm: expand, sort, compress) followed by the selection of the mask's entries with
                   torch.searchsorted on the sorted keys.  Both arms of the baseline are ops the package had before
                   the intersection kernel.  The full product is skipped, and said to be, when its partial products
                   would not fit the device.
  tail             the same launch split by probe length: the pairs a group of 8 lanes runs (probe <= T) and the
                   pairs a whole wave runs (probe > T), each timed alone through ops.pair_intersect.
  R-MAT 24         (A @ A) . A alone (100 M generated entries), with the same split.
  common_neighbors 1 M uniformly random pairs and 1 M stored edges of R-MAT 21; on the host scipy's sampled form
                   A[u].multiply(A[v]).sum(1), which is (A @ A.T)[u, v] without forming the product.
  gradient         forward + backward of masked_spspmm with both operands' values tracked, config 3.
  --sweep-t DIR    every DIR/T<n>/libpaddle_sparse_hip.so (a build of csrc/intersect.hip with
                   PSA_EXTRA_HIPCC_FLAGS=-DPSA_INTERSECT_T=<n>; api.hip is all it needs beside it) runs the
                   R-MAT 21 and config-3 launches through ctypes, alternating with the shipped library.

Arms alternate call by call in one process; every figure is the median [min .. max] of ROUNDS whole calls on HIP
events after WARM warm-up calls.

usage: python tools/masked_spspmm_bench.py [--quick] [--no-rmat24 | --rmat24-only] [--sweep-t DIR]"""
import ctypes
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bench import make_workload, rmat_graph  # noqa: E402
import paddle_sparse_amd as psa  # noqa: E402
from paddle_sparse_amd import SparseTensor, _lib, ops  # noqa: E402

dev = torch.device("cuda", 0)
WARM, ROUNDS = 2, 7
T = 32


def call_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(arms, rounds=ROUNDS, warm=WARM):
    """{name: fn} -> {name: (median, min, max)} with the arms taking turns."""
    first = max(call_ms(fn) for fn in arms.values())
    if first > 1000.0:  # calls of seconds: fewer of them
        rounds, warm = 3, 1
    for _ in range(warm - 1):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            times[k].append(call_ms(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def show(label, t):
    print(f"   {label:58s} {t[0]:10.3f} ms  [{t[1]:.3f} .. {t[2]:.3f}]", flush=True)


def config3(M=2_000_000, nnz=20_000_000):
    rowptr, col, val = make_workload(M, M, nnz, 128, 3, dev)
    row = ops.ptr2ind(rowptr, col.numel())
    return SparseTensor(row=row, col=col, value=val, sparse_sizes=(M, M), is_sorted=False).coalesce()


def rmat(scale, n):
    N, rowptr, row, col, val = rmat_graph(scale, n, dev)
    return SparseTensor(rowptr=rowptr, row=row, col=col, value=val, sparse_sizes=(N, N), is_sorted=True, trust_data=True)


def product_then_select(a):
    """The route without the masked op: the whole product, then the mask's entries by their sorted keys."""
    N = a.size(1)
    c = a @ a
    rc, cc, vc = c.coo()
    rm, cm, _ = a.coo()
    kc, km = rc * N + cc, rm * N + cm
    pos = torch.searchsorted(kc, km).clamp_(max=max(kc.numel() - 1, 0))
    return torch.where(kc[pos] == km, vc[pos], torch.zeros((), dtype=vc.dtype, device=dev))


def split_by_probe(a):
    """Pairs of (A @ A) . A by the length of their probe list (the shorter of row i of A and column j of A)."""
    row, col, _ = a.coo()
    probe = torch.minimum(a.storage.rowcount()[row], a.storage.colcount()[col])
    return row, col, probe


def masked_block(name, a, with_product):
    a.fill_cache_()
    row, col, probe = split_by_probe(a)
    nnz = a.nnz()
    rc = a.storage.rowcount()
    print(f"== {name}: {a.size(0)} nodes, {nnz} entries, longest row {int(rc.max())}, longest column "
          f"{int(a.storage.colcount().max())}", flush=True)
    products = int(ops.spspmm_count(a.storage.col(), a.storage.rowptr()).sum())
    long_pairs = int((probe > T).sum())
    print(f"   partial products of A @ A: {products} ({products / max(nnz, 1):.1f} per entry of A); pairs with a probe "
          f"list above T = {T}: {long_pairs} ({100.0 * long_pairs / max(nnz, 1):.3f} %), longest probe {int(probe.max())}, "
          f"probe elements in short pairs {int(probe[probe <= T].sum())}, in long pairs {int(probe[probe > T].sum())}",
          flush=True)
    arms = {"masked_spspmm(A, A, A)": lambda: psa.masked_spspmm(a, a, a)}
    free = torch.cuda.mem_get_info(dev)[0]
    fits = with_product and products * 48 < free  # keys, values, owner, the sort's second buffers
    if fits:
        arms["A @ A (spspmm) alone"] = lambda: a @ a
        arms["A @ A, then the mask's entries"] = lambda: product_then_select(a)
    res = alternate(arms)
    for k, t in res.items():
        show(k, t)
    if fits:
        got, want = psa.masked_spspmm(a, a, a).storage.value(), product_then_select(a)
        scale = float(want.abs().max())
        print(f"   masked / (product + selection) = {res['masked_spspmm(A, A, A)'][0] / res[list(arms)[2]][0]:.4f}; "
              f"largest difference of the two results {float((got - want).abs().max()):.3e} at scale {scale:.3e}", flush=True)
    elif with_product:
        print(f"   A @ A NOT run: {products} partial products need about {products * 48 / 2**30:.0f} GiB, "
              f"{free / 2**30:.0f} GiB are free.  No figure is extrapolated.", flush=True)
    # the same launch, split by mode
    x = a.csr()
    y = a.csc()
    parts = {"all pairs (raw op)": torch.ones_like(probe, dtype=torch.bool), "pairs with probe <= T (8 lanes each)": probe <= T,
             "pairs with probe > T (a wave each)": probe > T}
    arms = {}
    for k, sel in parts.items():
        r, c = row[sel].contiguous(), col[sel].contiguous()
        if r.numel():
            arms[f"{k}: {r.numel()}"] = (lambda r=r, c=c: ops.pair_intersect(x, y, r, c))
    tail = alternate(arms)
    for k, t in tail.items():
        show(k, t)
    return a, (x, y, row, col)


def sweep_t(libdir, workloads):
    libs = {f"T = {T} (shipped)": _lib.load()}
    for p in sorted(Path(libdir).glob("T*/libpaddle_sparse_hip.so"), key=lambda p: int(p.parent.name[1:])):
        lib = ctypes.CDLL(str(p))
        lib.psa_pair_intersect.restype, lib.psa_pair_intersect.argtypes = _lib.SIGNATURES["psa_pair_intersect"]
        libs[f"T = {int(p.parent.name[1:])}"] = lib
    for name, (x, y, row, col) in workloads.items():
        print(f"== sweep of T on {name}: {row.numel()} pairs", flush=True)
        outs, arms = {}, {}
        for k, lib in libs.items():
            outs[k] = torch.empty(row.numel(), dtype=torch.float32, device=dev)

            def fn(lib=lib, out=outs[k]):
                ops.check(lib.psa_pair_intersect(0, x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), x[0].numel() - 1,
                                                 y[0].data_ptr(), y[1].data_ptr(), y[2].data_ptr(), y[0].numel() - 1, None,
                                                 row.data_ptr(), col.data_ptr(), row.numel(), out.data_ptr(), ops._stream()))
            arms[k] = fn
        for k, t in alternate(arms).items():
            show(k, t)
        # T only moves pairs between the two modes: the sums change order, nothing else
        ref = outs[f"T = {T} (shipped)"]
        worst = max(float((o - ref).abs().max()) for o in outs.values())
        print(f"   largest difference between any two settings {worst:.3e} at scale {float(ref.abs().max()):.3e}", flush=True)


def common_neighbors_block(a, pairs=1_000_000):
    N = a.size(0)
    g = torch.Generator(device=dev).manual_seed(1)
    row, col, _ = a.coo()
    e = torch.randint(0, a.nnz(), (pairs,), generator=g, device=dev)
    sets = {"uniformly random pairs": (torch.randint(0, N, (pairs,), generator=g, device=dev),
                                       torch.randint(0, N, (pairs,), generator=g, device=dev)),
            "stored edges": (row[e].contiguous(), col[e].contiguous())}
    pattern = a.set_value(None)
    print(f"== common_neighbors on {pairs} pairs of the same graph (counts; X = Y = the rows)", flush=True)
    try:
        import scipy.sparse as sp
    except ImportError:
        sp = None
    host = None if sp is None else sp.csr_matrix((torch.ones(a.nnz()).numpy(), a.storage.col().cpu().numpy(),
                                                  a.storage.rowptr().cpu().numpy()), shape=(N, N))
    for name, (u, v) in sets.items():
        res = alternate({"checked": lambda: pattern.common_neighbors(u, v),
                         "trust_data=True": lambda: pattern.common_neighbors(u, v, trust_data=True)})
        show(f"{name}, with the range check (one host read)", res["checked"])
        show(f"{name}, trust_data=True", res["trust_data=True"])
        got = pattern.common_neighbors(u, v)
        print(f"   mean count {float(got.double().mean()):.3f}, largest {int(got.max())}", flush=True)
        if host is not None:
            # the host form copies both rows of every pair: as many pairs as stay below 50 M copied entries
            deg = a.storage.rowcount()
            copied = torch.cumsum(deg[u] + deg[v], 0)
            H = int((copied <= 50_000_000).sum())
            uh, vh = u[:H].cpu().numpy(), v[:H].cpu().numpy()
            t = time.perf_counter()
            want = host[uh].multiply(host[vh]).sum(axis=1)
            ms = (time.perf_counter() - t) * 1e3
            same = bool((torch.from_numpy(want.A1 if hasattr(want, "A1") else want.ravel()).long() == got[:H].cpu()).all())
            print(f"   scipy on the host, A[u].multiply(A[v]).sum(1) on the first {H} pairs (one call, one thread, "
                  f"without the copies) {ms:10.1f} ms; same counts: {same}", flush=True)


def gradient_block(a):
    print("== gradient step of masked_spspmm(A, A', A) on the config-3 shape, both operands' values tracked", flush=True)
    va = a.storage.value().clone().requires_grad_()
    vb = a.storage.value().clone().requires_grad_()
    ta, tb = a.set_value(va, layout="coo"), a.set_value(vb, layout="coo")
    g = torch.randn(a.nnz(), device=dev, generator=torch.Generator(device=dev).manual_seed(2))

    def step():
        va.grad = vb.grad = None
        psa.masked_spspmm(ta, tb, a).storage.value().backward(g)

    res = alternate({"forward, untracked": lambda: psa.masked_spspmm(a, a, a),
                     "forward + backward (three launches of the kernel)": step})
    for k, t in res.items():
        show(k, t)


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    quick = "--quick" in sys.argv
    print(f"device: {torch.cuda.get_device_name(dev)}; T = {T}; median [min .. max] of {ROUNDS} alternating calls after "
          f"{WARM} warm-up calls", flush=True)
    workloads = {}
    if "--rmat24-only" in sys.argv:
        with torch.no_grad():
            masked_block("R-MAT 24", rmat(24, 100_000_000), False)
        sys.exit(0)
    with torch.no_grad():
        c3 = config3(20_000, 200_000) if quick else config3()
        c3, workloads["config 3"] = masked_block("config 3" + (" (a hundredth: --quick)" if quick else ""), c3, True)
    gradient_block(c3)
    del c3
    torch.cuda.empty_cache()
    with torch.no_grad():
        r21 = rmat(14, 200_000) if quick else rmat(21, 20_000_000)
        r21, workloads["R-MAT 21"] = masked_block("R-MAT 14 (--quick)" if quick else "R-MAT 21", r21, True)
        common_neighbors_block(r21, 10_000 if quick else 1_000_000)
        if "--sweep-t" in sys.argv:
            sweep_t(sys.argv[sys.argv.index("--sweep-t") + 1], workloads)
        del r21, workloads
        torch.cuda.empty_cache()
        if not quick and "--no-rmat24" not in sys.argv:
            masked_block("R-MAT 24", rmat(24, 100_000_000), False)
