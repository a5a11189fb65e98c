"""Record the bits of fused attention: tests/golden/attention_bits.json, checked by tests/test_attention_bits_gpu.py.

    python tests/golden/make_attention_bits.py            # on the GPU; writes the fixture

The fixture pins the arithmetic of psa_attention_* and psa_gat_attention_* (fp32 and bf16, with and without dropout):
per case a SHA-256 (its first 64 bits, as 16 hex digits) of the raw bytes of every input and of out, stat and the
gradients of the three dense operands and of the bias.  Hashes only: a change of one rounding anywhere shows.  A pull
request that changes the arithmetic on purpose runs this tool again and says so; one that does not must leave the
fixture alone.  Only the public Python API is used (SparseTensor.attention / gat_attention, ops.attention_raw,
ops.gat_attention_raw, autograd), so the tool runs on any commit that has these.

One pattern serves all cases: 40 rows by 320 columns, rows of 0, 1, 64 (one tile), 65 (a tile boundary), 128 (kLongRow:
the last length that is not long), 129 (a long row of two chunks) and 300 (three chunks, the last one partial) entries,
the other rows short.  The long rows put every case through the row kernel and through the chunk / combine path.
Inputs are small integers over 64 from a seeded CPU torch.Generator (bf16: rounded on the CPU), the bias holds a few
-inf among finite values.  The shapes take every value of every template parameter of every entry-point family, for
both dtypes (forward VEC wide / 1, NR 4 / 0, NT 1 / 2 / 4; backward VEC wide / 1, NRK 4 / 0, NRF 4 / 0)."""
import hashlib
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent.parent
FIXTURE = Path(__file__).resolve().parent / "attention_bits.json"
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

DEV = "cuda"
M, N = 40, 320
LENGTHS = [0, 1, 64, 65, 128, 129, 300] + [2 + (5 * i) % 9 for i in range(M - 7)]
DROPOUT_P, SEED = 0.25, 20260711
# (H, K, F) and what it reaches in fp32 / bf16 (forward VEC, NR, NT; backward NRK, NRF)
SHAPES = [
    (1, 1, 1),        # element form, one tile
    (3, 5, 7),        # element form, nothing a power of two
    (8, 16, 16),      # 16-byte form, one tile, q in registers; backward (4, 4)
    (8, 64, 64),      # two tiles in fp32, one in bf16
    (16, 64, 64),     # four tiles in fp32, two in bf16
    (20, 4, 4),       # two head blocks, 16 + 4 (bf16: the element form)
    (1, 3, 261),      # element form, NT = 4 with the pass repeated; backward (4, 0)
    (1, 261, 3),      # element form, forward NR = 0; backward (0, 4)
    (1, 261, 261),    # element form; backward (0, 0)
    (1, 8, 2048),     # 16-byte form, one head wider than the tile budget: the pass is repeated
    (8, 512, 64),     # 16-byte form, forward NR = 0; backward (0, 4)
    (8, 16, 512),     # 16-byte form; backward (4, 0)
    (16, 256, 256),   # 16-byte form; backward (0, 0)
]
OFFSET_SHAPE = (8, 16, 16)  # once more one element into the allocation: divisible widths off 16 bytes
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def sha(t: torch.Tensor) -> str:
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def pattern():
    g = torch.Generator().manual_seed(7)
    cols = [torch.sort(torch.randperm(N, generator=g)[:n]).values for n in LENGTHS]
    rowptr = torch.tensor([0] + LENGTHS, dtype=torch.int64).cumsum(0)
    return rowptr, torch.cat(cols).to(torch.int64)


def cases():
    """Every case as a dict of plain values; its position in the list seeds its inputs."""
    out = []
    for family in ("attention", "gat"):
        shapes = [s + (False, 0.2) for s in SHAPES] + [OFFSET_SHAPE + (True, 0.2)]
        if family == "gat":  # K dropped: (H, F) once each, and negative_slope = 0 once
            seen, shapes = set(), []
            for H, _, F in SHAPES:
                if (H, F) not in seen:
                    seen.add((H, F))
                    shapes.append((H, 0, F, False, 0.2))
            shapes += [(OFFSET_SHAPE[0], 0, OFFSET_SHAPE[2], True, 0.2), (3, 0, 7, False, 0.0)]
        for H, K, F, offset, slope in shapes:
            for dtype in DTYPES:
                for bias in ("none", "entry", "head"):
                    for p in (0.0, DROPOUT_P):
                        name = f"{family}-{dtype}-H{H}" + (f"-K{K}" if family == "attention" else "") + f"-F{F}"
                        name += ("-offset" if offset else "") + (f"-slope{slope}" if family == "gat" else "")
                        name += f"-bias_{bias}-p{p}"
                        out.append(dict(name=name, family=family, dtype=dtype, H=H, K=K, F=F, offset=offset,
                                        slope=slope, bias=bias, p=p, index=len(out)))
    return out


def small(g, shape, dtype):
    """Integers in [-128, 128] over 64: the same on every machine, then rounded once for bf16."""
    return (torch.randint(-128, 129, shape, generator=g).to(torch.float32) / 64).to(dtype)


def inputs(case, nnz, rowptr):
    """The CPU inputs of a case by name: the dense operands, grad_out and the bias (or None)."""
    g = torch.Generator().manual_seed(1000 + case["index"])
    dtype, H, K, F = DTYPES[case["dtype"]], case["H"], case["K"], case["F"]
    if case["family"] == "attention":
        dense = dict(q=small(g, (M, H, K), dtype), k=small(g, (N, H, K), dtype))
    else:
        dense = dict(a_row=small(g, (M, H), dtype), a_col=small(g, (N, H), dtype))
    dense["v"] = small(g, (N, H, F), dtype)
    dense["grad_out"] = small(g, (M, H, F), dtype)
    bias = None
    if case["bias"] != "none":
        bias = small(g, (nnz,) if case["bias"] == "entry" else (nnz, H), torch.float32)
        first = torch.zeros(nnz, dtype=torch.bool)
        first[rowptr[:-1][rowptr[:-1] < nnz]] = True  # never the first entry of a row: no row of nothing but -inf
        masked = (torch.arange(nnz) % 29 == 7) & ~first
        bias[masked] = float("-inf")
    return dense, bias


def one_off(t):
    """The same numbers in a view that starts one element into its allocation."""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = base[1:].view(t.shape)
    view.copy_(t)
    return view


def results(case, rowptr, col, dense, bias):
    """out, stat and the gradients of a case as device tensors, by name."""
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import ops

    put = (lambda t: one_off(t.to(DEV))) if case["offset"] else (lambda t: t.to(DEV))
    rp, cl = rowptr.to(DEV), col.to(DEV)
    names = ("q", "k", "v") if case["family"] == "attention" else ("a_row", "a_col", "v")
    ops_in = [put(dense[n]) for n in names]
    bd = None if bias is None else bias.to(DEV)
    drop = dict(dropout_p=case["p"], seed=SEED)
    if case["family"] == "attention":
        how = dict(scale=float(case["K"]) ** -0.5)
        out, stat = ops.attention_raw(rp, cl, *ops_in, bias=bd, **how, **drop)
    else:
        how = dict(negative_slope=case["slope"])
        out, stat = ops.gat_attention_raw(rp, cl, *ops_in, bias=bd, **how, **drop)
    leaves = [t.detach().requires_grad_() for t in ops_in]
    if bd is not None:
        bd = bd.detach().requires_grad_()
    A = psa.SparseTensor(rowptr=rp, col=cl, value=bd, sparse_sizes=(M, N), is_sorted=True)
    fused = A.attention if case["family"] == "attention" else A.gat_attention
    again = fused(*leaves, bias=bd is not None, **how, **drop)
    again.backward(put(dense["grad_out"]))
    assert torch.equal(again.view(torch.uint8), out.view(torch.uint8)), "autograd's forward differs from the raw one"
    res = {"out": out, "stat": stat}
    res.update({"grad_" + n: t.grad for n, t in zip(names, leaves)})
    if bd is not None:
        res["grad_bias"] = bd.grad
    return res


def run_case(case, rowptr, col):
    """(input hashes, result hashes) of one case."""
    dense, bias = inputs(case, col.numel(), rowptr)
    ins = {n: sha(t) for n, t in dense.items()}
    if bias is not None:
        ins["bias"] = sha(bias)
    return ins, {n: sha(t) for n, t in results(case, rowptr, col, dense, bias).items()}


def main():
    rowptr, col = pattern()
    record = {"pattern": {"rowptr": sha(rowptr), "col": sha(col)}, "cases": {}}
    for case in cases():
        ins, first = run_case(case, rowptr, col)
        _, second = run_case(case, rowptr, col)
        if first != second:
            diff = [n for n in first if first[n] != second[n]]
            raise SystemExit(f"{case['name']}: two runs differ in {diff}; nothing recorded")
        record["cases"][case["name"]] = {"inputs": ins, "results": first}
    lines = [f'{json.dumps(n)}: {json.dumps(c, sort_keys=True)}' for n, c in record["cases"].items()]  # a case per line
    FIXTURE.write_text('{"pattern": ' + json.dumps(record["pattern"], sort_keys=True) + ',\n"cases": {\n' +
                       ",\n".join(lines) + "\n}}\n")
    json.loads(FIXTURE.read_text())
    print(f"{len(record['cases'])} cases -> {FIXTURE}")


if __name__ == "__main__":
    main()
