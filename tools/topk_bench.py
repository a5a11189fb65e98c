#!/usr/bin/env python3
"""ops.segment_topk against the torch-ops form a user writes today, on the config-3 shape (2 M x 2 M,
20 M entries) and R-MAT 24 (bench.rmat_graph(24, 100 M)), both symmetrised (every entry stored both
ways, coalesced) as in tools/node2vec_bench.py, with uniform random fp32 scores.

For k in {1, 8, 32} and dim in {1, 0} (rows over rowptr; columns over colptr with perm = csr2csc, built
ONCE outside the timed region for both forms) the HIP op and the torch form are timed ALTERNATELY on the
same inputs, several rounds, so that drift hits both alike; per form the median and the range of the
rounds are printed.  Both produce the uint8 keep mask in storage order and are held to each other on
all entries before they are timed.

The torch form of the same semantics: a stable descending sort by the score, a stable sort of the
segment ids in that order (so the entries of a segment stand together, best first, ties by position),
rank = index - the segment's begin, keep = rank < k, scattered back.  (The padded dense torch.topk
cannot be built on R-MAT 24: its longest row alone would pad every row to 10^5 entries.)

Byte model: read 4 B per entry (plus 8 B of perm for dim = 0) and the pointers, write
1 B per entry; the fraction of 8 TB/s is printed next to the op.  Segments above TOPK_LDS entries read
their entries once per pass on top of that (5 passes for a 32-bit key); their share of the entries is
printed with the graph.

usage: python tools/topk_bench.py [--quick]   (--quick: config 3 only)"""
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from bench import event_ms  # noqa: E402
from node2vec_bench import config3, rmat24  # noqa: E402
from paddle_sparse_amd import SparseTensor, ops  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS, REPS_HIP, REPS_TORCH = 3, 20, 3


def torch_topk(score, ptr, seg, k, perm):
    """keep uint8[n] by two stable sorts; seg = the segment id of every position in segment order."""
    x = score if perm is None else score[perm]
    first = torch.sort(x, descending=True, stable=True).indices
    second = torch.sort(seg[first], stable=True).indices
    order = first[second]  # positions by (segment, score descending, position)
    rank = torch.arange(x.numel(), device=x.device) - ptr[seg[order]]
    keep = torch.zeros(x.numel(), dtype=torch.uint8, device=x.device)
    keep[order if perm is None else perm[order]] = (rank < k).to(torch.uint8)
    return keep


def run(name, make):
    N, rowptr, col = make()
    nnz = col.numel()
    score = torch.rand(nnz, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    a = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(N, N), is_sorted=True, trust_data=True)
    st = a.storage
    with torch.no_grad():
        perm, colptr = st.csr2csc(), st.colptr()
        sides = {1: (rowptr, st.row(), None), 0: (colptr, st.col()[perm].contiguous(), perm)}
        deg = rowptr[1:] - rowptr[:-1]
        lds = int(((deg > ops.TOPK_SHORT) & (deg <= ops.TOPK_LDS)).sum())
        stream = deg > ops.TOPK_LDS
        print(f"== {name}, symmetrised: {N} nodes, {nnz} entries, longest row {int(deg.max())}; rows above "
              f"{ops.TOPK_SHORT} entries: {lds} in LDS, {int(stream.sum())} streamed holding "
              f"{int(deg[stream].sum()) / nnz:.3f} of the entries", flush=True)
        work = {}
        for k in (1, 8, 32):
            for dim in (1, 0):
                ptr, seg, p = sides[dim]
                assert torch.equal(ops.segment_topk(score, ptr, k, p), torch_topk(score, ptr, seg, k, p)), (k, dim)
                nbytes = nnz * (5 + (8 if dim == 0 else 0)) + 8 * (N + 1)
                work[(k, dim)] = (nbytes, lambda ptr=ptr, p=p, k=k: ops.segment_topk(score, ptr, k, p),
                                  lambda ptr=ptr, seg=seg, p=p, k=k: torch_topk(score, ptr, seg, k, p))
        times = {(w, side): [] for w in work for side in ("hip", "torch")}
        for _ in range(ROUNDS):
            for w, (_, hip, ref) in work.items():
                for side, fn, reps in (("hip", hip, REPS_HIP), ("torch", ref, REPS_TORCH)):
                    fn()  # warm-up: the allocator has the blocks afterwards
                    times[(w, side)].append(event_ms(fn, reps))
        print(f"   ms per call over {ROUNDS} alternating rounds of {REPS_HIP} (HIP op) or {REPS_TORCH} (torch form) calls; "
              f"ratio = median over the median of the torch form:", flush=True)
        for (k, dim), (nbytes, _, _) in work.items():
            base = statistics.median(times[((k, dim), "torch")])
            for side in ("hip", "torch"):
                ts = times[((k, dim), side)]
                med = statistics.median(ts)
                model = f"{nbytes / 1e9:6.3f} GB, {nbytes / med / 1e9:6.3f} TB/s = {nbytes / med / 1e9 / 8:5.3f} of 8 TB/s"
                print(f"     k = {k:2d} dim = {dim} {side:6s} median {med:9.3f}   range {min(ts):9.3f} .. {max(ts):9.3f}   "
                      f"x{med / base:6.3f}   {model if side == 'hip' else ''}", flush=True)
    del a, st, sides, work
    torch.cuda.empty_cache()


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}", flush=True)
    run("config-3 shape", config3)
    if "--quick" not in sys.argv:
        run("R-MAT 24", rmat24)
