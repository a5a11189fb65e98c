"""What tests/test_workspace_layout.py checks and tests/golden/make_workspace_golden.py records: the argument grid of
every psa_*_workspace_bytes, and one refused call per entry point that cuts regions out of a caller's workspace.

Nothing here runs a kernel.  A refusal case is a small VALID problem whose operands and workspace are real, full-size
buffers (on the GPU when there is one, else on the host); only the size it declares is short.  A library that
wrongly accepted it would run a legitimate call on a GPU, or fail with a HIP status without one."""
import functools
import itertools
import re
from pathlib import Path

import torch

HEADER = Path(__file__).resolve().parent.parent / "include" / "paddle_sparse_hip.h"

# ---- sizes: values on both sides of every threshold of the formulas -----------------------------------------------
NNZ = [0, 1, 128, 129, 1000, 2**19 - 1, 2**19, 2**20 - 1, 2**20, 2**25, 2**31 - 1]  # kLongRow, the sort's tile rules
WIDTH = [0, 1, 4, 8, 64, 128, 256, 512]  # K / D
HEADS = [1, 2, 8]  # H, F
ROWS = [0, 1, 1000, 2**24]  # M, N
REDUCE = [0, 3]  # sum, max
MAX_VALUE = [1, 2**20, 2**48]  # 0, 3 and 6 radix passes

SIZE_GRIDS = {
    "psa_spmm_workspace_bytes": (REDUCE, WIDTH, NNZ),
    "psa_spmm_half_workspace_bytes": (REDUCE, WIDTH, NNZ),
    "psa_spmm_half_bw_csc_workspace_bytes": (WIDTH, NNZ),
    "psa_spmm_value_bw_workspace_bytes": (NNZ,),
    "psa_spmm_minmax_bw_csc_workspace_bytes": (ROWS, WIDTH, NNZ),
    "psa_spmm_minmax_bw_eb_workspace_bytes": (WIDTH, NNZ),
    "psa_spmm_sum_bw_csc_workspace_bytes": (WIDTH, NNZ),
    "psa_index_sort_workspace_bytes": (NNZ, MAX_VALUE),
    "psa_coalesce_small_workspace_bytes": (NNZ,),
    "psa_coalesce_workspace_bytes": (NNZ, ROWS, ROWS),
    "psa_count2ptr_workspace_bytes": (NNZ,),
    "psa_unique_workspace_bytes": (NNZ,),
    "psa_scatter_workspace_bytes": (NNZ,),
    "psa_diag_workspace_bytes": (ROWS + NNZ,),
    "psa_saint_workspace_bytes": (NNZ, NNZ),
    "psa_rcm_workspace_bytes": (NNZ, NNZ),
    "psa_neighbor_workspace_bytes": (NNZ,),
    "psa_neighbor_hop_workspace_bytes": (NNZ,),
    "psa_segment_softmax_workspace_bytes": (NNZ, WIDTH),
    "psa_spmm_heads_workspace_bytes": (NNZ, HEADS, HEADS),
    "psa_sddmm_heads_workspace_bytes": (NNZ,),
    "psa_attention_workspace_bytes": (NNZ, HEADS, HEADS),
}


def size_calls(name):
    return [list(args) for args in itertools.product(*SIZE_GRIDS[name])]


@functools.lru_cache(maxsize=None)
def header_params():
    """{entry point: [parameter names]} from the header."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(psa_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text):
        params = [p.strip() for p in m.group(2).split(",")]
        out[m.group(1)] = [] if params == ["void"] else [re.search(r"(\w+)$", p).group(1) for p in params]
    return out


# ---- refusals -----------------------------------------------------------------------------------------------------
SUM, MAX, BF16 = 0, 3, 5
M, N, NNZ_LONG, K, H, F = 4, 320, 300, 8, 2, 8  # one row of 300 entries: nnz > 128 engages the long-row scratch
SORT_N, SORT_MAX = 1000, 2**20

# Pointer parameters that get a zero-filled 64 KiB buffer of their own (the largest operand, [320, 2, 8] floats, is
# 20 KiB).
BUFFERS = {"value", "mat", "out", "grad", "x", "y", "q", "k", "v", "stat", "grad_out", "p", "ds", "dz", "a_row", "a_col",
           "src", "grad_src", "sorted_out", "perm_out", "payload", "payload_out", "out_row", "out_col", "ptr", "perm",
           "count_out", "rowcount_out", "rowptr_out", "tag", "arg_bytes", "weight_csc", "grad_value_csc", "grad_mat"}
SCALARS = dict(reduce=SUM, dtype=BF16, K=K, H=H, F=F, D=K, nnz=NNZ_LONG, n=NNZ_LONG, num_hot=0, ldo=0, arg_width=1,
               algo=0, bias_heads=1, scale=1.0, alpha=1.0, dropout_p=0.25, seed=1, negative_slope=0.2, insert=1,
               first_bit=0, max_value=SORT_MAX)
NULLS = {"hot_rows", "arg_out", "bias", "stream", "colcount", "colcount_out", "row_scale", "hot_grad", "hot_bytes"}

# (entry point, overrides, (size function, its arguments by name), bytes declared: None = one short of the need)
_ATTN = ("psa_attention_workspace_bytes", ("nnz", "H", "F"))
CASES = [
    # psa_spmm's public size is the larger of the edge-range and the long-row need; 256 is short of both
    ("psa_spmm", {}, ("psa_spmm_workspace_bytes", ("reduce", "K", "nnz")), 256),
    ("psa_spmm", {"reduce": MAX}, ("psa_spmm_workspace_bytes", ("reduce", "K", "nnz")), 256),
    ("psa_spmm_coo", {}, ("psa_spmm_workspace_bytes", ("reduce", "K", "nnz")), 256),
    ("psa_spmm_coo", {"algo": 2}, ("psa_spmm_workspace_bytes", ("reduce", "K", "nnz")), None),  # the edge ranges
    ("psa_spmm_half_coo", {"algo": 2}, ("psa_spmm_half_workspace_bytes", ("reduce", "K", "nnz")), None),
    ("psa_spmm_value_bw", {}, ("psa_spmm_value_bw_workspace_bytes", ("nnz",)), None),
    ("psa_spmm_sum_bw_csc", {}, ("psa_spmm_sum_bw_csc_workspace_bytes", ("K", "nnz")), None),
    ("psa_spmm_minmax_bw_csc", {}, ("psa_spmm_minmax_bw_csc_workspace_bytes", ("M", "K", "nnz")), None),
    ("psa_spmm_minmax_bw_eb", {}, ("psa_spmm_minmax_bw_eb_workspace_bytes", ("K", "nnz")), None),
    ("psa_spmm_half_sum_bw_csc", {}, ("psa_spmm_half_bw_csc_workspace_bytes", ("K", "nnz")), None),
    ("psa_spmm_half_minmax_bw_csc", {}, ("psa_spmm_half_bw_csc_workspace_bytes", ("K", "nnz")), None),
    ("psa_index_sort", {"n": SORT_N}, ("psa_index_sort_workspace_bytes", ("n", "max_value")), None),
    ("psa_sort_pairs_u32", {"n": SORT_N}, ("psa_index_sort_workspace_bytes", ("n", "max_value")), None),
    ("psa_sort_pairs_u32_field", {"n": SORT_N}, ("psa_index_sort_workspace_bytes", ("n", "max_value")), None),
    ("psa_coalesce_small", {}, ("psa_coalesce_small_workspace_bytes", ("n",)), None),
    ("psa_coalesce_count", {"value": None, "dtype": 0, "D": 1}, ("psa_coalesce_workspace_bytes", ("n", "M", "N")), None),
    ("psa_diag_count", {"k": 0}, ("psa_diag_workspace_bytes", ("M",)), None),
    ("psa_segment_softmax", {"perm": None}, ("psa_segment_softmax_workspace_bytes", ("n", "D")), None),
    ("psa_segment_softmax_bw", {"perm": None}, ("psa_segment_softmax_workspace_bytes", ("n", "D")), None),
    ("psa_spmm_heads", {}, ("psa_spmm_heads_workspace_bytes", ("nnz", "H", "F")), None),
    ("psa_spmm_heads_half", {}, ("psa_spmm_heads_workspace_bytes", ("nnz", "H", "F")), None),
    ("psa_sddmm_heads", {}, ("psa_sddmm_heads_workspace_bytes", ("nnz",)), None),
    ("psa_attention_fw", {}, _ATTN, None),
    ("psa_attention_dropout_fw", {}, _ATTN, None),
    ("psa_attention_half_fw", {}, _ATTN, None),
    ("psa_attention_half_dropout_fw", {}, _ATTN, None),
    ("psa_gat_attention_fw", {}, _ATTN, None),
    ("psa_gat_attention_half_fw", {}, _ATTN, None),
    # the backward passes use the list alone
    ("psa_attention_bw_entries", {}, ("psa_sddmm_heads_workspace_bytes", ("nnz",)), None),
    ("psa_attention_dropout_bw_entries", {}, ("psa_sddmm_heads_workspace_bytes", ("nnz",)), None),
    ("psa_attention_half_bw_entries", {}, ("psa_sddmm_heads_workspace_bytes", ("nnz",)), None),
    ("psa_attention_half_dropout_bw_entries", {}, ("psa_sddmm_heads_workspace_bytes", ("nnz",)), None),
    ("psa_gat_attention_bw_entries", {}, ("psa_sddmm_heads_workspace_bytes", ("nnz",)), None),
    ("psa_gat_attention_half_bw_entries", {}, ("psa_sddmm_heads_workspace_bytes", ("nnz",)), None),
]
# These read the CSC view: the same pattern transposed, 320 x 4 with one COLUMN of 300 entries.
CSC_VIEW = {"psa_spmm_sum_bw_csc", "psa_spmm_minmax_bw_csc", "psa_spmm_minmax_bw_eb", "psa_spmm_half_sum_bw_csc",
            "psa_spmm_half_minmax_bw_csc"}


def case_id(case):
    name, over = case[0], case[1]
    return name + "".join(f"[{k}={v}]" for k, v in over.items() if k in ("reduce", "algo"))


def device():
    return "cuda" if torch.cuda.is_available() else "cpu"


# psa_diag_count asks for no alignment beyond its int64 words
MISALIGNED_CASES = [c for c in CASES if c[0] != "psa_diag_count"]


def build_call(lib, case, misaligned=False):
    """(arguments, tensors to keep alive) of a refusal case: a workspace declared too small, or (misaligned) one of
    the full size that starts 8 bytes past a 16-byte boundary."""
    name, over, (size_fn, size_args), declared = case
    dev = device()
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    long_ptr = [0] + [NNZ_LONG] * M  # row (or column) 0 holds every entry
    env = dict(SCALARS)
    if name in CSC_VIEW:  # entry e = (row e, column 0)
        env.update(M=N, N=M, colptr=i64(long_ptr), row_csc=torch.arange(NNZ_LONG, device=dev), col_csc=i64([0] * NNZ_LONG),
                   csr2csc=torch.arange(NNZ_LONG, device=dev), rowptr=i64([min(r, NNZ_LONG) for r in range(N + 1)]))
    else:  # entry e = (row 0, column e)
        env.update(M=M, N=N, rowptr=i64(long_ptr), indptr=i64(long_ptr), nseg=M, row=i64([0] * NNZ_LONG),
                   col=torch.arange(NNZ_LONG, device=dev), arg_bytes=None, keys=torch.arange(SORT_N, device=dev) * 1000)
    env.update(over)
    need = getattr(lib, size_fn)(*[env[a] for a in size_args])
    assert need > (declared or 1), (name, need)  # the scratch is engaged
    workspace = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
    assert workspace.data_ptr() % 16 == 0
    if misaligned:
        env.update(workspace=workspace.data_ptr() + 8, workspace_bytes=need)
    else:
        env.update(workspace=workspace, workspace_bytes=need - 1 if declared is None else declared)
    args, keep = [], [workspace]
    for p in header_params()[name]:
        if p in env:
            v = env[p]
        elif p in NULLS:
            v = None
        else:
            assert p in BUFFERS, (name, p)
            v = torch.zeros(65536, dtype=torch.uint8, device=dev)
        if isinstance(v, torch.Tensor):
            keep.append(v)
            v = v.data_ptr()
        args.append(v)
    return args, keep
