"""Operator surface of the HIP core — the counterpart of the reference's
`paddle_sparse_ops` extension module (csrc/convert.cpp:37-43,70-76,
csrc/version.cpp:35-40), same names and argument meaning, on torch tensors
that live in MI355X HBM.

torch is plumbing here (device memory + the current HIP stream); every op is
one or more calls through the C-ABI in include/paddle_sparse_hip.h.  Outputs
are allocated by the caller side (here: torch's allocator), as the reference
does with paddle::empty.  Calls are asynchronous on the current stream.

CPU tensors are rejected: this build has no CPU kernels and never falls back.
"""
from __future__ import annotations

import os
from typing import List, Optional, Tuple

import torch

from . import _lib
from ._lib import REDUCE_ID, HipCoreError, check

_check = check  # for functions with a parameter named `check`


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """The current HIP stream of the current device as an integer handle (2.9 us through
    torch.cuda.current_stream(), which builds a Stream object; 0.3 us through the raw getter)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


class _NoSwitch:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_SWITCH = _NoSwitch()


def _on(device):
    """Context that makes `device` current for the launches inside — the no-op
    singleton when it already is (torch.cuda.device() costs ~8 us per op even
    then, as much as two kernel launches)."""
    idx = device.index
    if idx is None or idx == torch.cuda.current_device():
        return _NO_SWITCH
    return torch.cuda.device(device)


def _gpu(x: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not x.is_cuda:
        raise RuntimeError(
            f"{name} must be a GPU tensor: paddle_sparse_amd runs on MI355X "
            "only and has no CPU path")
    return x


def _index(x: torch.Tensor, name: str) -> torch.Tensor:
    _gpu(x, name)
    if x.dtype != torch.int64:
        raise TypeError(f"{name} must be int64 (got {x.dtype})")
    if x.dim() != 1:
        raise ValueError(f"{name} must be 1-D")
    return x.contiguous()


def _ptr(x: Optional[torch.Tensor]) -> Optional[int]:
    return None if x is None else x.data_ptr()


def _aligned16(x: torch.Tensor) -> torch.Tensor:
    """x itself when its data starts on a 16-byte boundary, else a contiguous copy (a fresh allocation is):
    the vector kernels load 16 bytes at a time and their C-ABI refuses other operands.  A contiguous view
    can start anywhere (flat[1:1 + N * K].view(N, K))."""
    return x if x.data_ptr() % 16 == 0 else x.clone(memory_format=torch.contiguous_format)


def sparse_cuda_version() -> torch.Tensor:
    """csrc/version.cpp:14-22: int64[1] on the CPU; -1 on this (HIP) build."""
    return torch.full((1,), _lib.load().psa_sparse_cuda_version(), dtype=torch.int64)


def ind2ptr(ind: torch.Tensor, M: int) -> torch.Tensor:
    """csrc/convert.cpp:13-43.  ind: sorted int64[E] -> int64[M+1]."""
    ind = _index(ind, "ind")
    out = torch.empty(M + 1, dtype=torch.int64, device=ind.device)
    with _on(ind.device):
        check(_lib.load().psa_ind2ptr(_ptr(ind), ind.numel(), M, _ptr(out), _stream()))
    return out


def ptr2ind(ptr: torch.Tensor, E: int) -> torch.Tensor:
    """csrc/convert.cpp:46-76.  ptr: int64[M+1] -> int64[E]."""
    ptr = _index(ptr, "ptr")
    if ptr.numel() < 1:
        raise ValueError("ptr must have at least one element")
    out = torch.empty(E, dtype=torch.int64, device=ptr.device)
    with _on(ptr.device):
        check(_lib.load().psa_ptr2ind(_ptr(ptr), ptr.numel() - 1, E, _ptr(out), _stream()))
    return out


def _spmm(reduce: str, rowptr: torch.Tensor, col: torch.Tensor,
          value: Optional[torch.Tensor], mat: torch.Tensor, want_arg_bytes: bool = False,
          want_arg: bool = True, row: Optional[torch.Tensor] = None, algo: str = "auto",
          out: Optional[torch.Tensor] = None, hot_rows: Optional[torch.Tensor] = None,
          no_long_rows: bool = False):
    """(out, arg_out | None) — and, with want_arg_bytes (min/max, K % 4 == 0), a
    third result: arg_out as row-local byte indices for spmm_minmax_bw_csc.
    want_arg=False (min/max) skips the int64 arg_out altogether: the kernel then
    stores `out` (and the bytes, if asked for) only — two thirds of the output
    traffic gone; for callers that need no backward, or whose backward is served
    by the bytes alone (no row longer than ARG_BYTES_EXACT_ROW entries).
    `row` (the COO row ids, SparseStorage.row()) is optional: the edge-balanced
    kernels read it and derive it from rowptr when it is not given.  `algo`:
    "auto" | "row_waves" | "edge_ranges" (psa_spmm_algo; csr_row_stats /
    SparseStorage._spmm_algo() choose per matrix).  `out`: write into this
    fp32 [M, K] tensor, which may be a column slice of a wider contiguous
    matrix (row stride = the wider matrix's width).  `hot_rows` (edge_ranges
    only): float32 [h, K] compact copy of rows of mat; column ids in [N, N + h)
    name its rows (SparseStorage._hot_columns builds the redirected col).  `no_long_rows`: the
    caller knows that no row has more than 128 entries (SparseStorage._longest_row); for K <= 128 the
    call then brings no long-row workspace, which saves the three near-empty launches of the long-row
    machinery — 5 us of a 45 us problem such as BASELINE config 2."""
    rowptr = _index(rowptr, "rowptr")
    col = _index(col, "col")
    if row is not None:
        row = _index(row, "row")
        if row.numel() != col.numel():
            raise ValueError("row must have one entry per edge")
    _gpu(mat, "mat")
    if mat.dtype in (torch.float16, torch.bfloat16):
        if out is not None:
            raise ValueError("the half-width SpMM does not take `out`")
        res = _spmm_half(reduce, rowptr, col, value, mat, want_arg, row=row, algo=algo, hot_rows=hot_rows,
                         want_arg_bytes=want_arg_bytes)
        return res
    if mat.dtype != torch.float32:
        raise TypeError(f"spmm takes float32, float16 or bfloat16 dense operands (mat is {mat.dtype})")
    if mat.dim() != 2:
        raise ValueError("mat must be 2-D [N, K]")
    mat = mat.contiguous()
    if value is not None:
        _gpu(value, "value")
        if value.dtype != torch.float32 or value.dim() != 1 or value.numel() != col.numel():
            raise ValueError("value must be float32[nnz]")
        value = value.contiguous()
    if rowptr.numel() < 1:
        raise ValueError("rowptr must have at least one element")
    M, (N, K), nnz = rowptr.numel() - 1, mat.shape, col.numel()
    rid = REDUCE_ID[reduce]
    num_hot = 0
    if hot_rows is not None:
        _gpu(hot_rows, "hot_rows")
        if hot_rows.dtype != torch.float32 or hot_rows.dim() != 2 or hot_rows.shape[1] != K or not hot_rows.is_contiguous():
            raise ValueError("hot_rows must be a contiguous float32 [h, K] tensor")
        num_hot = hot_rows.shape[0]
        mat = _aligned16(mat)  # the redirected column ids are served by the edge-range kernels only (16-byte rows)
    ldo = 0
    if out is None:
        out = torch.empty((M, K), dtype=torch.float32, device=mat.device)
    else:
        _gpu(out, "out")
        if out.dtype != torch.float32 or out.shape != (M, K) or (K > 1 and out.stride(1) != 1):
            raise ValueError("out must be float32 [M, K] with unit column stride")
        ldo = out.stride(0) if M > 1 else K
        if ldo < K:
            raise ValueError("out rows overlap")
    arg = None
    minmax = rid in (_lib.MIN, _lib.MAX)
    lib = _lib.load()
    ws_bytes = lib.psa_spmm_workspace_bytes(rid, K, nnz)  # long-row scratch (0 if no row can be long)
    if no_long_rows and algo != "edge_ranges" and (K <= 64 or (K <= 128 and not want_arg_bytes and N * K * 4 < (6 << 30))):
        # every row on its own wave / lane group: same results, no list / chunk / combine launches (K <= 64: the
        # multirow kernel; 64 < K <= 128: the row kernel, as fast as the fused-roles one on rows this short —
        # 100k x 100k, F = 128: 83.5 -> 76.0 us, config 3: 1608 -> 1603 us; from K = 192 the fused kernel's
        # 128-wide tiles win, and only it gathers non-temporally for operands beyond 6 GiB)
        ws_bytes = 0
    ws = _workspace(ws_bytes, mat.device) if ws_bytes else None
    # the kernels that write the byte form themselves: K <= 64 (multirow) and, for
    # 64 < K <= 256, the fused-roles kernel — which spmm_dispatch takes only when a row
    # CAN be long (nnz > kLongRow = 128; the edge-range kernels write the bytes too, but
    # fall back to the row path on shapes they do not take).  Behind the others the
    # bytes are derived from arg_out, which must then exist.  (ws_bytes > 0 is not the
    # test: it also covers the edge-range scratch, which every nnz > 0 has.)
    # (those kernels read 16-byte rows: a misaligned `mat` or `out` sends the shape to the 1-wide kernels, which do not)
    vec4 = K % 4 == 0 and mat.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and (ldo == 0 or ldo % 4 == 0)
    bytes_in_kernel = vec4 and (K <= 64 or (K <= 256 and nnz > LONG_ROW))
    if minmax and want_arg_bytes and K % 4 == 0 and K <= 256 and not bytes_in_kernel:
        want_arg = True
    if minmax and want_arg:
        arg = torch.empty((M, K), dtype=torch.int64, device=mat.device)
    arg_bytes = None
    arg_width = 2 if want_arg_bytes == 2 else 1  # True / 1: one byte per element; 2: two (exact up to 65 536-entry rows)
    if want_arg_bytes and minmax and K % 4 == 0 and (want_arg or K <= 256):
        arg_bytes = torch.empty((M, K), dtype=torch.int16 if arg_width == 2 else torch.uint8, device=mat.device)
    with _on(mat.device):
        check(lib.psa_spmm_coo(rid, _ptr(rowptr), _ptr(row), _ptr(col), _ptr(value), _ptr(mat),
                               _ptr(hot_rows) if num_hot else None, num_hot, M, N, K, nnz, _ptr(out), ldo, _ptr(arg), _ptr(arg_bytes),
                               arg_width, _lib.SPMM_ALGO_ID[algo], _ptr(ws), ws_bytes, _stream()))
    if want_arg_bytes:
        return out, arg, arg_bytes
    return out, arg


def _spmm_half(reduce: str, rowptr, col, value, mat, want_arg: bool = True, row=None, algo: str = "auto",
               hot_rows=None, want_arg_bytes=False):
    """fp16 / bf16 `mat` -> (out in mat's dtype, arg_out | None): fp32 products and sums,
    one rounding on store (psa_spmm_half / psa_spmm_half_coo).  value: None, float32[nnz] or
    mat's dtype[nnz].  algo="edge_ranges" (with `row`, `hot_rows` as for fp32; fp32 or no values):
    the edge-balanced kernels.  K % 8 != 0 widens to fp32 and rounds the fp32 kernel's result."""
    if mat.dim() != 2:
        raise ValueError("mat must be 2-D [N, K]")
    mat = mat.contiguous()
    M, (N, K), nnz = rowptr.numel() - 1, mat.shape, col.numel()
    rid = REDUCE_ID[reduce]
    minmax = rid in (_lib.MIN, _lib.MAX)
    if value is not None:
        _gpu(value, "value")
        if value.dtype not in (torch.float32, mat.dtype) or value.dim() != 1 or value.numel() != nnz:
            raise ValueError("value must be float32[nnz] or mat's dtype[nnz]")
        value = value.contiguous()
    if want_arg_bytes and K % 8 != 0:
        raise ValueError("the half-width SpMM writes arg_bytes for K % 8 == 0 only")
    if K % 8 != 0:
        res = _spmm(reduce, rowptr, col, None if value is None else value.float(), mat.float(), want_arg=want_arg)
        return res[0].to(mat.dtype), res[1]
    mat = _aligned16(mat)  # 16-byte gathers of 8 elements
    out = torch.empty((M, K), dtype=mat.dtype, device=mat.device)
    arg = torch.empty((M, K), dtype=torch.int64, device=mat.device) if minmax and want_arg else None
    if algo == "edge_ranges" and nnz > 0 and (value is None or value.dtype == torch.float32):
        num_hot = 0
        if hot_rows is not None:
            _gpu(hot_rows, "hot_rows")
            if hot_rows.dtype != mat.dtype or hot_rows.dim() != 2 or hot_rows.shape[1] != K or not hot_rows.is_contiguous():
                raise ValueError("hot_rows must be a contiguous [h, K] tensor of mat's dtype")
            num_hot = hot_rows.shape[0]
        lib = _lib.load()
        ws = _workspace(lib.psa_spmm_half_workspace_bytes(rid, K, nnz), mat.device)
        eb_bytes, eb_width = None, 2 if want_arg_bytes == 2 else 1
        if want_arg_bytes and minmax:  # the row-local form, from the edge-range kernels (power-law matrices)
            eb_bytes = torch.empty((M, K), dtype=torch.int16 if eb_width == 2 else torch.uint8, device=mat.device)
        with _on(mat.device):
            check(lib.psa_spmm_half_coo(rid, _DTYPE_ID[mat.dtype], _ptr(rowptr), _ptr(row), _ptr(col), _ptr(value), _ptr(mat),
                                        _ptr(hot_rows) if num_hot else None, num_hot, M, N, K, nnz, _ptr(out), _ptr(arg),
                                        _ptr(eb_bytes), eb_width, _lib.SPMM_ALGO_ID[algo], _ptr(ws), ws.numel(), _stream()))
        if want_arg_bytes:
            return out, arg, eb_bytes
        return out, arg
    if hot_rows is not None:
        raise ValueError("hot_rows needs algo='edge_ranges' and fp32 (or no) values")
    arg_bytes, width = None, 2 if want_arg_bytes == 2 else 1
    if want_arg_bytes and minmax:  # the row-local form for the half-width one-pass backward (one wave per row only)
        arg_bytes = torch.empty((M, K), dtype=torch.int16 if width == 2 else torch.uint8, device=mat.device)
    with _on(mat.device):
        check(_lib.load().psa_spmm_half_arg(rid, _DTYPE_ID[mat.dtype], _ptr(rowptr), _ptr(col), _ptr(value),
                                            _DTYPE_ID[value.dtype] if value is not None else 0, _ptr(mat), M, N, K, nnz,
                                            _ptr(out), _ptr(arg), _ptr(arg_bytes), width, _stream()))
    if want_arg_bytes:
        return out, arg, arg_bytes
    return out, arg


# rows above this many entries leave their wave for the chunk role (psa::kLongRow, csrc/long_rows.h)
LONG_ROW = 128
# rows up to this many entries: the one-byte form of arg_out (arg_bytes) needs no arg_out beside it
ARG_BYTES_EXACT_ROW = 128
# ... and the two-byte form (want_arg_bytes=2)
ARG_WORDS_EXACT_ROW = 65_535  # 0xffff is "no winner" (vec_io.h)


def spmm_sum(rowptr, col, value, mat, row=None, algo="auto") -> torch.Tensor:
    """out[i] = sum_e value[e] * mat[col[e]] (value None -> weights 1)."""
    return _spmm("sum", rowptr, col, value, mat, row=row, algo=algo)[0]


def spmm_mean(rowptr, col, value, mat, row=None, algo="auto") -> torch.Tensor:
    return _spmm("mean", rowptr, col, value, mat, row=row, algo=algo)[0]


def spmm_min(rowptr, col, value, mat, row=None, algo="auto") -> Tuple[torch.Tensor, torch.Tensor]:
    """Returns (out, arg_out); arg_out == nnz marks an empty row."""
    return _spmm("min", rowptr, col, value, mat, row=row, algo=algo)


def spmm_max(rowptr, col, value, mat, row=None, algo="auto") -> Tuple[torch.Tensor, torch.Tensor]:
    return _spmm("max", rowptr, col, value, mat, row=row, algo=algo)


def csr_row_stats(rowptr: torch.Tensor) -> Tuple[int, int, int, int]:
    """(rows without entries, rows with 1-2 entries, rows above 128 entries,
    longest row) of a CSR pointer.  Synchronises (one 32-byte host read)."""
    rowptr = _index(rowptr, "rowptr")
    stats = torch.empty(4, dtype=torch.int64, device=rowptr.device)
    with _on(rowptr.device):
        check(_lib.load().psa_csr_row_stats(_ptr(rowptr), rowptr.numel() - 1, _ptr(stats), _stream()))
    e, t, b, m = stats.tolist()
    return e, t, b, m


def spmm_set_variant(variant: int) -> int:
    """Bench/test hook: pick the SpMM kernel variant (0 = auto)."""
    return _lib.load().psa_spmm_set_variant(int(variant))


# ---------------------------------------------------------------------------
# sort / gather / coalesce building blocks
# ---------------------------------------------------------------------------

_DTYPE_ID = {
    torch.float32: 0, torch.float64: 1, torch.int32: 2, torch.int64: 3,
    torch.float16: 4, torch.bfloat16: 5,
}


_POISON_WORKSPACE = os.environ.get("PSA_POISON_WORKSPACE") == "1"  # test hook: scratch starts as 0xff, not as whatever it held


def _workspace(nbytes: int, device) -> torch.Tensor:
    # torch's caching allocator hands back >= 512-byte aligned blocks
    ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
    if _POISON_WORKSPACE:
        ws.fill_(255)
    return ws


class SortScratch:
    """Workspace of a finished sort, kept alive so that the next host read can fold in the
    sort's look-back diagnostic (unique_sorted(after=...))."""

    def __init__(self, ws: torch.Tensor, n: int, max_value: int):
        self.ws, self.n, self.max_value = ws, n, max_value


def _raise_on_sort_fault(lib, ws: torch.Tensor, n: int, max_value: int, who: str) -> None:
    """One 4-byte host read behind a sort that no other host read follows: the look-back
    diagnostic of the single-sweep passes (psa_index_sort_status).  A wait that gave up has
    made the last pass store -1 instead of an order; here it becomes an exception, as the
    reference's argsort could never hand back a wrong permutation (storage.py:164-169)."""
    status = lib.psa_index_sort_status(_ptr(ws), n, max_value, _stream())
    if status != 0:
        raise HipCoreError(f"{who}: an inter-workgroup wait of a radix pass gave up "
                           f"(status {status}); the order is invalid")


def index_sort(keys: torch.Tensor, max_value: Optional[int] = None,
               with_sorted_inputs: bool = False, keep_scratch: bool = False, check: bool = False):
    """paddle_sparse/utils.py:14-23 — returns (sorted | None, perm).

    Stable LSD radix sort in HIP; `max_value` (exclusive bound on the keys, the
    reference passes M*N) selects the number of 8-bit passes.  perm is the
    stable sorting permutation, bit-identical to numpy argsort(kind="stable").
    keep_scratch: also return a SortScratch for unique_sorted(after=...).
    check: read the sort's fault word afterwards (one host read, synchronises) and
    raise HipCoreError if a look-back wait gave up — for callers whose result no other
    host read follows (SparseStorage's constructor sort, csr2csc).
    ONLY THE FAULT WORD IS AUTHORITATIVE: after a fault the outputs hold -1 where the
    faulted tiles of the last pass sat, possibly valid-looking entries and untouched memory
    elsewhere — the absence of -1 in a part of them proves nothing.  A caller that passes
    check=False must read the word itself before it trusts the order: keep_scratch=True and
    unique_sorted(after=...) (the coalesce path: the word comes back with the count, no
    extra synchronisation) or index_sort_checked / sort_fault_word.
    """
    keys = _index(keys, "keys")
    n = keys.numel()
    if max_value is None:
        max_value = (int(keys.max()) + 1) if n else 1
    max_value = max(int(max_value), 1)
    perm = torch.empty(n, dtype=torch.int64, device=keys.device)
    out = torch.empty(n, dtype=torch.int64, device=keys.device) if with_sorted_inputs else None
    lib = _lib.load()
    nbytes = lib.psa_index_sort_workspace_bytes(n, max_value)
    ws = _workspace(nbytes, keys.device)
    with _on(keys.device):
        _check(lib.psa_index_sort(_ptr(keys), n, max_value, _ptr(out), _ptr(perm),
                                  _ptr(ws), ws.numel(), _stream()))
        if check and n > 0:
            _raise_on_sort_fault(lib, ws, n, max_value, "index_sort")
    if keep_scratch:
        return out, perm, SortScratch(ws, n, max_value)
    return out, perm


def index_sort_checked(keys: torch.Tensor, max_value: int):
    """index_sort plus the look-back diagnostic word (tests): returns
    (sorted, perm, status) with status 0 when every inter-workgroup wait of the
    single-sweep passes ended normally.  Synchronises."""
    keys = _index(keys, "keys")
    n = keys.numel()
    max_value = max(int(max_value), 1)
    perm = torch.empty(n, dtype=torch.int64, device=keys.device)
    out = torch.empty(n, dtype=torch.int64, device=keys.device)
    lib = _lib.load()
    ws = _workspace(lib.psa_index_sort_workspace_bytes(n, max_value), keys.device)
    with _on(keys.device):
        check(lib.psa_index_sort(_ptr(keys), n, max_value, _ptr(out), _ptr(perm),
                                 _ptr(ws), ws.numel(), _stream()))
        status = lib.psa_index_sort_status(_ptr(ws), n, max_value, _stream())
    return out, perm, status


def sort_pairs(keys: torch.Tensor, payload: torch.Tensor, max_value: Optional[int] = None, keep_scratch: bool = False,
               check: bool = False):
    """Stable sort of (key, 4-byte payload) pairs: returns (sorted_keys,
    payload[perm]) without ever forming perm.  payload: 1-D, 4-byte dtype.
    keep_scratch: also return a SortScratch for unique_sorted(after=...).
    check: as for index_sort."""
    keys = _index(keys, "keys")
    _gpu(payload, "payload")
    if payload.dim() != 1 or payload.element_size() != 4 or payload.numel() != keys.numel():
        raise ValueError("payload must be 1-D, 4 bytes per element, same length as keys")
    payload = payload.contiguous()
    n = keys.numel()
    if max_value is None:
        max_value = (int(keys.max()) + 1) if n else 1
    max_value = max(int(max_value), 1)
    out_keys = torch.empty_like(keys)
    out_pay = torch.empty_like(payload)
    lib = _lib.load()
    ws = _workspace(lib.psa_index_sort_workspace_bytes(n, max_value), keys.device)
    with _on(keys.device):
        _check(lib.psa_sort_pairs_u32(_ptr(keys), _ptr(payload), n, max_value, _ptr(out_keys),
                                      _ptr(out_pay), _ptr(ws), ws.numel(), _stream()))
        if check and n > 0:
            _raise_on_sort_fault(lib, ws, n, max_value, "sort_pairs")
    if keep_scratch:
        return out_keys, out_pay, SortScratch(ws, n, max_value)
    return out_keys, out_pay


def sort_pairs_field(keys: torch.Tensor, payload: torch.Tensor, first_bit: int, max_value: int,
                     keep_scratch: bool = False):
    """Stable sort of (key, 4-byte payload) pairs by the bit field
    (key >> first_bit) < max_value only; the low bits ride inside the key.
    keep_scratch: also return a SortScratch for unique_sorted(after=...)."""
    keys = _index(keys, "keys")
    _gpu(payload, "payload")
    if payload.dim() != 1 or payload.element_size() != 4 or payload.numel() != keys.numel():
        raise ValueError("payload must be 1-D, 4 bytes per element, same length as keys")
    payload = payload.contiguous()
    n, max_value = keys.numel(), max(int(max_value), 1)
    out_keys, out_pay = torch.empty_like(keys), torch.empty_like(payload)
    lib = _lib.load()
    ws = _workspace(lib.psa_index_sort_workspace_bytes(n, max_value), keys.device)
    with _on(keys.device):
        check(lib.psa_sort_pairs_u32_field(_ptr(keys), _ptr(payload), n, int(first_bit), max_value,
                                           _ptr(out_keys), _ptr(out_pay), _ptr(ws), ws.numel(), _stream()))
    if keep_scratch:
        return out_keys, out_pay, SortScratch(ws, n, max_value)
    return out_keys, out_pay


def merge_sorted(a: torch.Tensor, b: torch.Tensor, payload_a: Optional[torch.Tensor] = None,
                 payload_b: Optional[torch.Tensor] = None, want_source: bool = True):
    """Stable merge of two SORTED int64 key arrays (a's entry first on ties):
    what index_sort(cat([a, b])) returns, without the sort.  Returns (merged,
    source | None, payload | None); source indexes the concatenation, payload
    (when both 4-byte 1-D payload arrays are given) is cat([pa, pb])[source]."""
    a, b = _index(a, "a"), _index(b, "b")
    na, nb = a.numel(), b.numel()
    pay_out = None
    if payload_a is not None or payload_b is not None:
        for name, p, n in (("payload_a", payload_a, na), ("payload_b", payload_b, nb)):
            if p is None:
                raise ValueError("merge_sorted: give both payloads or neither")
            _gpu(p, name)
            if p.dim() != 1 or p.element_size() != 4 or p.numel() != n or not p.is_contiguous():
                raise ValueError(f"{name} must be contiguous, 1-D, 4 bytes per element, one per key")
        if payload_a.dtype != payload_b.dtype:
            raise ValueError("merge_sorted: payload dtypes differ")
        pay_out = torch.empty(na + nb, dtype=payload_a.dtype, device=a.device)
    merged = torch.empty(na + nb, dtype=torch.int64, device=a.device)
    source = torch.empty(na + nb, dtype=torch.int64, device=a.device) if want_source else None
    with _on(a.device):
        check(_lib.load().psa_merge_sorted(_ptr(a), na, _ptr(b), nb, _ptr(payload_a), _ptr(payload_b),
                                           _ptr(merged), _ptr(source), _ptr(pay_out), _stream()))
    return merged, source, pay_out


def coalesce_small_max() -> int:
    return int(_lib.load().psa_coalesce_small_max())


def coalesce_small(row: torch.Tensor, col: torch.Tensor, m: int, n: int):
    """Sort by (row, col) + run-length structure in ONE launch of one workgroup
    (inputs of at most coalesce_small_max() entries; see the header).  Returns
    (count, ptr int64[count + 1], row' int64[count], col' int64[count], perm
    int64[nnz]) like index_sort + unique_sorted.  One host read (count)."""
    key_bound(m, n, "coalesce_small")
    row, col = _index(row, "row"), _index(col, "col")
    nnz = row.numel()
    dev = row.device
    out = torch.empty((2, nnz), dtype=torch.int64, device=dev)
    ptr = torch.empty(nnz + 1, dtype=torch.int64, device=dev)
    perm = torch.empty(nnz, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    lib = _lib.load()
    ws = _workspace(lib.psa_coalesce_small_workspace_bytes(nnz), dev)
    with _on(dev):
        check(lib.psa_coalesce_small(_ptr(row), _ptr(col), nnz, int(m), int(n), out[0].data_ptr(),
                                     out[1].data_ptr(), _ptr(ptr), _ptr(perm), _ptr(count), _ptr(ws),
                                     ws.numel(), _stream()))
    c = int(count.item())
    return c, ptr[:c + 1], out[0, :c], out[1, :c], perm


class IndexRangeError(AssertionError):
    """A row / col index lies outside the matrix (the reference asserts
    row.max() < M and col.max() < N, storage.py:78-91)."""


def key_bound(rows: int, cols: int, who: str) -> int:
    """rows * cols: the exclusive bound of the keys row * cols + col of a rows x cols matrix, as the sorts take it.
    ValueError when it does not fit a signed 64-bit integer: the keys would wrap, and ctypes would hand the C entry
    points a wrapped bound without a word.  Host arithmetic only; every op that forms such keys asks before its
    first launch."""
    rows, cols = int(rows), int(cols)
    if rows * cols >= (1 << 63):
        raise ValueError(f"{who}: the keys row * {cols} + col of a {rows} x {cols} matrix do not fit 63 bits "
                         f"({rows} * {cols} >= 2^63)")
    return rows * cols


_FUSED_SMALL = 10_240  # entries the one-launch coalesce takes (psa_coalesce_small_max_fused)


def _check_chain_flags(flags: int, m: int, n: int) -> None:
    if flags & 1:
        raise IndexRangeError(f"coalesce: an index lies outside the {m} x {n} matrix")
    if flags & 4:
        raise HipCoreError("coalesce: an inter-workgroup wait of the radix sort gave up; the result is invalid")


def coalesce_chain(row: torch.Tensor, col: torch.Tensor, value: Optional[torch.Tensor], m: int, n: int,
                   op: str = "sum", read_first: bool = False):
    """coalesce of (row, col, value) of an m x n matrix in two C-ABI calls
    (psa_coalesce_count / psa_coalesce_write) and ONE host read.  Returns
    (index int64[2, count] contiguous, value' | None, was_sorted).  With
    read_first the count is read between the calls and the outputs are sized
    exactly; otherwise both calls are enqueued on worst-case buffers first."""
    key_bound(m, n, "coalesce")
    row, col = _index(row, "row"), _index(col, "col")
    nnz, dev = row.numel(), row.device
    if col.numel() != nnz:
        raise ValueError("row and col must have the same length")
    dt, D = 0, 0
    if value is not None:
        _gpu(value, "value")
        if value.dtype not in _DTYPE_ID:
            raise TypeError(f"coalesce: unsupported value dtype {value.dtype}")
        if value.shape[0] != nnz:
            raise ValueError("value.shape[0] must equal nnz")
        value = value.contiguous()
        dt, D = _DTYPE_ID[value.dtype], 1
        for s in value.shape[1:]:
            D *= s
    if nnz == 0:
        return torch.empty((2, 0), dtype=torch.int64, device=dev), value, True
    lib = _lib.load()
    rid = REDUCE_ID[op]
    if (nnz <= _FUSED_SMALL and not read_first and 0 < m * n < (1 << 62)
            and (value is None or (D == 1 and value.dim() == 1 and value.dtype in (torch.float32, torch.int32)))):
        # one launch for everything (one workgroup, sort resident in the LDS): one buffer holds the
        # index (2 nnz words), the values (nnz 4-byte words) and the two status words
        buf = torch.empty(3 * nnz + 2, dtype=torch.int64, device=dev)
        status = buf[3 * nnz:]
        out = buf[2 * nnz:3 * nnz].view(value.dtype)[:nnz] if value is not None else None
        with _on(dev):
            check(lib.psa_coalesce_small_fused(_ptr(row), _ptr(col), _ptr(value), dt, nnz, int(m), int(n), rid,
                                               _ptr(buf), _ptr(out), _ptr(status), _stream()))
        count, flags = status.tolist()
        _check_chain_flags(flags, m, n)
        return buf[:2 * count].view(2, count), (None if out is None else out[:count]), not (flags & 2)
    ws = _workspace(lib.psa_coalesce_workspace_bytes(nnz, int(m), int(n)), dev)
    status = ws[:16].view(torch.int64)
    tail = tuple(value.shape[1:]) if value is not None else ()
    with _on(dev):
        check(lib.psa_coalesce_count(_ptr(row), _ptr(col), _ptr(value), dt, D, nnz, int(m), int(n),
                                     _ptr(ws), ws.numel(), _stream()))
        count = -1
        if read_first:
            count, flags = status.tolist()
            _check_chain_flags(flags, m, n)
        rows = nnz if count < 0 else count
        index = torch.empty(2 * rows, dtype=torch.int64, device=dev)
        out = torch.empty((rows,) + tail, dtype=value.dtype, device=dev) if value is not None else None
        check(lib.psa_coalesce_write(_ptr(value), dt, D, nnz, int(m), int(n), rid, count, _ptr(ws),
                                     _ptr(index), _ptr(out), _stream()))
        if not read_first:
            count, flags = status.tolist()
            _check_chain_flags(flags, m, n)
    index = index[:2 * count].view(2, count)
    if out is not None:
        out = out[:count]
    return index, out, not (flags & 2)


def make_keys_checked(row: torch.Tensor, col: torch.Tensor, m: int, n: int):
    """keys = row * n + col plus the device status words {0, flags}: bit 0 = an
    index outside [0, m) x [0, n), bit 1 = keys not sorted (storage.py:159-163)."""
    key_bound(m, n, "make_keys_checked")
    row, col = _index(row, "row"), _index(col, "col")
    keys = torch.empty_like(row)
    status = torch.empty(4, dtype=torch.int64, device=row.device)
    with _on(row.device):
        check(_lib.load().psa_make_keys_checked(_ptr(row), _ptr(col), row.numel(), int(m), int(n), _ptr(keys),
                                                _ptr(status), _stream()))
    return keys, status


def make_keys(a: torch.Tensor, b: torch.Tensor, mul: int, check_sorted: bool = False
              ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """keys = a * mul + b  (+ device flag "some key is smaller than its
    predecessor", storage.py:159-163)."""
    a, b = _index(a, "a"), _index(b, "b")
    if a.numel() != b.numel():
        raise ValueError("a and b must have the same length")
    keys = torch.empty_like(a)
    flag = torch.zeros(1, dtype=torch.int32, device=a.device) if check_sorted else None
    with _on(a.device):
        check(_lib.load().psa_make_keys(_ptr(a), _ptr(b), int(mul), a.numel(), _ptr(keys),
                                        _ptr(flag), _stream()))
    return keys, flag


def split_keys(keys: torch.Tensor, div: int, want_hi: bool = True, want_lo: bool = True
               ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(keys // div, keys % div): the two indices a key stream was built from,
    without a permutation gather."""
    keys = _index(keys, "keys")
    hi = torch.empty_like(keys) if want_hi else None
    lo = torch.empty_like(keys) if want_lo else None
    with _on(keys.device):
        check(_lib.load().psa_split_keys(_ptr(keys), keys.numel(), int(div), _ptr(hi), _ptr(lo),
                                         _stream()))
    return hi, lo


def needs_grad(x: Optional[torch.Tensor]) -> bool:
    """True when autograd will want a gradient for x (callers then keep the
    values on a differentiable route instead of letting them ride a sort)."""
    return x is not None and torch.is_grad_enabled() and x.requires_grad


class _GatherRows(torch.autograd.Function):
    """src[perm] with the reference's differentiability (paddle `value[perm]`,
    storage.py:166-169, transpose.py:14-22): the backward adds every output
    row's gradient back into the row it was read from — a gather through the
    inverse permutation when the caller has one, a scatter-add otherwise."""

    @staticmethod
    def forward(ctx, src, perm, inverse):
        ctx.save_for_backward(perm, inverse)
        ctx.rows = src.shape[0]
        return _gather_rows_raw(src, perm)

    @staticmethod
    def backward(ctx, grad):
        perm, inverse = ctx.saved_tensors
        grad = grad.contiguous()
        if inverse is not None:
            return _gather_rows_raw(grad, inverse), None, None
        acc = grad if grad.dtype in (torch.float32, torch.float64) else grad.float()
        return scatter(acc, perm, ctx.rows, "sum").to(grad.dtype), None, None


def gather_rows(src: torch.Tensor, perm: torch.Tensor, inverse: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src[perm] along dim 0 for any dtype / trailing shape; differentiable in
    src.  `inverse` (optional): the inverse of perm when perm is a permutation
    of all rows — the backward is then a gather instead of a scatter-add."""
    if needs_grad(src):
        return _GatherRows.apply(src, perm, inverse)
    return _gather_rows_raw(src, perm)


def _gather_rows_raw(src: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    _gpu(src, "src")
    perm = _index(perm, "perm")
    src = src.contiguous()
    n = perm.numel()
    out = torch.empty((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    row_bytes = src.element_size()
    for s in src.shape[1:]:
        row_bytes *= s
    with _on(src.device):
        check(_lib.load().psa_gather_rows(_ptr(src), _ptr(perm), n, row_bytes, _ptr(out), _stream()))
    return out


def gather_rows_window(src: torch.Tensor, perm: torch.Tensor, col0: int, width: int,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src[perm, col0:col0 + width] for a 2-D contiguous src, as a dense [n, width]
    tensor (into `out` when given): rows and feature slice packed in one pass."""
    _gpu(src, "src")
    perm = _index(perm, "perm")
    if src.dim() != 2 or not src.is_contiguous():
        raise ValueError("src must be a contiguous 2-D tensor")
    if not (0 <= col0 and col0 + width <= src.shape[1]):
        raise ValueError("column window outside src")
    n, es = perm.numel(), src.element_size()
    if out is None:
        out = torch.empty((n, width), dtype=src.dtype, device=src.device)
    elif out.shape != (n, width) or out.dtype != src.dtype or not out.is_contiguous():
        raise ValueError("out must be a contiguous [n, width] tensor of src's dtype")
    with _on(src.device):
        check(_lib.load().psa_gather_rows_window(_ptr(src), src.shape[1] * es, col0 * es, width * es, _ptr(perm), n,
                                                 _ptr(out), _stream()))
    return out


def invert_permutation(perm: torch.Tensor) -> torch.Tensor:
    perm = _index(perm, "perm")
    inv = torch.empty_like(perm)
    with _on(perm.device):
        check(_lib.load().psa_invert_permutation(_ptr(perm), perm.numel(), _ptr(inv), _stream()))
    return inv


class PermutePlan:
    """Route of every element of a 4-byte array through a fixed permutation (psa_permute_apply_u32):
    structure only, 8 bytes per element; built by permute_plan, cached by the caller."""

    def __init__(self, sl, gs, lo, n):
        self.sl, self.gs, self.lo, self.n = sl, gs, lo, n


PERMUTE_PLAN_FROM = 1 << 20  # elements from which the planned two-pass form beats n dependent 4-byte reads


def permute_plan(dest: torch.Tensor) -> PermutePlan:
    """Plan for out[i] = src[perm[i]] given dest = the INVERSE of perm (dest[s] = where source s
    goes; csr2csc / csc2csr are each other's).  Two stable sorts, one inverse, one pack pass — once
    per permutation (see include/paddle_sparse_hip.h)."""
    dest = _index(dest, "dest")
    n, dev = dest.numel(), dest.device
    if n >= (1 << 31):
        raise ValueError("permute_plan: n must be below 2^31")
    lib = _lib.load()
    T = int(lib.psa_permute_tile())
    nb = max((n + T - 1) // T, 1)
    block, _ = split_keys(dest, T, want_lo=False)
    tile, _ = split_keys(torch.arange(n, dtype=torch.int64, device=dev), T, want_lo=False)
    keys_ts, _ = make_keys(tile, block, nb)
    del tile
    _, perm_ts = index_sort(keys_ts, nb * nb, check=True)
    del keys_ts
    _, perm_mid = index_sort(block, nb, check=True)
    del block
    gslot = invert_permutation(perm_mid)
    sl = torch.empty(n, dtype=torch.int16, device=dev)
    gs = torch.empty(n, dtype=torch.int32, device=dev)
    lo = torch.empty(n, dtype=torch.int16, device=dev)
    with _on(dev):
        check(lib.psa_permute_plan_pack(_ptr(perm_ts), _ptr(gslot), _ptr(perm_mid), _ptr(dest), n, _ptr(sl), _ptr(gs),
                                        _ptr(lo), _stream()))
    return PermutePlan(sl, gs, lo, n)


def permute_apply(src: torch.Tensor, plan: PermutePlan) -> torch.Tensor:
    """src[perm] for a contiguous 1-D 4-byte array along the plan of `perm` (no autograd)."""
    _gpu(src, "src")
    if src.dim() != 1 or src.element_size() != 4 or src.numel() != plan.n or not src.is_contiguous():
        raise ValueError("permute_apply takes a contiguous 1-D array of 4-byte elements, one per planned element")
    out, mid = torch.empty_like(src), torch.empty_like(src)
    with _on(src.device):
        check(_lib.load().psa_permute_apply_u32(_ptr(src), _ptr(plan.sl), _ptr(plan.gs), _ptr(plan.lo), plan.n, _ptr(mid),
                                                _ptr(out), _stream()))
    return out


class _SegmentCsr(torch.autograd.Function):
    """segment_csr with paddle_scatter's differentiability for sum / mean (the
    coalesce and reduce(dim) call sites, storage.py:471, reduce.py:51): every
    element of a segment receives the segment's gradient (over the segment's
    length for mean); with `perm` the gradient lands on src[perm[i]]."""

    @staticmethod
    def forward(ctx, src, indptr, reduce, perm):
        if REDUCE_ID[reduce] not in (_lib.SUM, _lib.MEAN):
            raise NotImplementedError(
                f"segment_csr(reduce={reduce!r}) is not differentiable in this build (sum / mean are)")
        ctx.save_for_backward(indptr, perm)
        ctx.mean, ctx.rows = REDUCE_ID[reduce] == _lib.MEAN, src.shape[0]
        return _segment_csr_raw(src, indptr, reduce, perm)

    @staticmethod
    def backward(ctx, grad):
        indptr, perm = ctx.saved_tensors
        n = perm.numel() if perm is not None else ctx.rows
        grad = grad.contiguous()
        if ctx.mean:
            # one division in fp32 (fp64 for fp64) and one rounding: a bf16 copy of the count is no
            # longer the count from 257 on
            wide = grad.dtype if grad.dtype == torch.float64 else torch.float32
            count = (indptr[1:] - indptr[:-1]).clamp(min=1).to(wide)
            grad = (grad.to(wide) / count.view((-1,) + (1,) * (grad.dim() - 1))).to(grad.dtype)
        g = _gather_rows_raw(grad, ptr2ind(indptr, n))  # the segment's gradient for each of its elements
        if perm is not None:
            acc = g if g.dtype in (torch.float32, torch.float64) else g.float()
            g = scatter(acc, perm, ctx.rows, "sum").to(grad.dtype)
        return g, None, None, None


def segment_csr(src: torch.Tensor, indptr: torch.Tensor, reduce: str = "sum",
                perm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """paddle_scatter.segment_csr(src, indptr, reduce=...) along dim 0
    (call sites storage.py:471, reduce.py:51); with `perm`, reduces
    src[perm] without materialising it.  Differentiable in src for sum / mean."""
    if needs_grad(src):
        return _SegmentCsr.apply(src, indptr, reduce, perm)
    return _segment_csr_raw(src, indptr, reduce, perm)


def _segment_csr_raw(src: torch.Tensor, indptr: torch.Tensor, reduce: str = "sum",
                     perm: Optional[torch.Tensor] = None) -> torch.Tensor:
    _gpu(src, "src")
    indptr = _index(indptr, "indptr")
    if src.dtype not in _DTYPE_ID:
        raise TypeError(f"segment_csr: unsupported dtype {src.dtype}")
    src = src.contiguous()
    if perm is not None:
        perm = _index(perm, "perm")
    nseg = indptr.numel() - 1
    D = 1
    for s in src.shape[1:]:
        D *= s
    n_rows = perm.numel() if perm is not None else src.shape[0]
    out = torch.empty((nseg,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    with _on(src.device):
        check(_lib.load().psa_segment_reduce(REDUCE_ID[reduce], _DTYPE_ID[src.dtype], _ptr(src),
                                             _ptr(perm), _ptr(indptr), nseg, D, n_rows,
                                             _ptr(out), _stream()))
    return out


def _unique_count(sorted_keys: torch.Tensor, after: Optional["SortScratch"]):
    """Phase 1 of unique_sorted: run heads counted per block and scanned; the ONE host read of the count (with the
    preceding sort's look-back diagnostic when `after` is given).  Returns (count, scratch, device count word)."""
    n, dev = sorted_keys.numel(), sorted_keys.device
    lib = _lib.load()
    ws = _workspace(lib.psa_unique_workspace_bytes(n), dev)
    count_d = torch.empty(2, dtype=torch.int64, device=dev)
    with _on(dev):
        if after is not None and after.n == n:
            check(lib.psa_unique_count_after_sort(_ptr(sorted_keys), n, _ptr(ws), ws.numel(), _ptr(after.ws),
                                                  after.max_value, _ptr(count_d), _stream()))
            count, fault = count_d.tolist()
            if fault:
                raise HipCoreError("index_sort: an inter-workgroup wait of a radix pass gave up; the order is invalid")
        else:
            check(lib.psa_unique_count(_ptr(sorted_keys), n, _ptr(ws), ws.numel(), _ptr(count_d), _stream()))
            count = int(count_d[0].item())
    return count, ws, count_d


def unique_sorted(sorted_keys: torch.Tensor, N: int, want_ptr: bool = True,
                  want_rowcol: bool = True, after: Optional[SortScratch] = None, _counted=None):
    """Run-length structure of SORTED keys (storage.py:455-470 without the
    bool-mask selects).  Returns (count, ptr | None, row | None, col | None)
    with row = key // N, col = key % N of each distinct key.  One host sync
    (reading the count to size the outputs) — the reference has three.
    after: the SortScratch of the sort that produced the keys; its look-back
    diagnostic comes back with the count (HipCoreError if a wait gave up)."""
    sorted_keys = _index(sorted_keys, "sorted_keys")
    n = sorted_keys.numel()
    dev = sorted_keys.device
    lib = _lib.load()
    count, ws, count_d = _counted if _counted is not None else _unique_count(sorted_keys, after)
    with _on(dev):
        ptr = torch.empty(count + 1, dtype=torch.int64, device=dev) if want_ptr else None
        # row and col are the two rows of ONE [2, count] buffer, so the
        # functional API's `stack([row, col])` (coalesce.py:29) is `row._base`
        index = torch.empty((2, count), dtype=torch.int64, device=dev) if want_rowcol else None
        row = index[0] if want_rowcol else None
        col = index[1] if want_rowcol else None
        if n > 0 and (want_ptr or want_rowcol):
            check(lib.psa_unique_write(_ptr(sorted_keys), n, int(N), _ptr(ws), _ptr(count_d),
                                       _ptr(ptr), _ptr(row), _ptr(col), _stream()))
        elif want_ptr:
            ptr.zero_()
    return count, ptr, row, col


def unique_sorted_reduce(sorted_keys: torch.Tensor, N: int, payload: torch.Tensor, reduce: str = "sum",
                         after: Optional[SortScratch] = None):
    """unique_sorted + segment_csr for 4-byte scalar values that are in the keys' sorted order already (they rode the
    sort as its payload, or the input was sorted): returns (count, row, col, value') with value'[s] = the reduction of
    run s.  When the runs are short (count * 32 > n) the index and the reduced values come from ONE launch and no
    ptr array is written (psa_unique_write_reduce); otherwise the two-launch form, whose reducer takes a wave per run."""
    sorted_keys = _index(sorted_keys, "sorted_keys")
    _gpu(payload, "payload")
    n, dev = sorted_keys.numel(), sorted_keys.device
    if payload.dim() != 1 or payload.numel() != n or payload.dtype not in (torch.float32, torch.int32):
        raise ValueError("payload must be float32[n] or int32[n]")
    counted = _unique_count(sorted_keys, after)
    count, ws, count_d = counted
    if 0 < count < n and count * 32 > n:
        payload = payload.contiguous()
        index = torch.empty((2, count), dtype=torch.int64, device=dev)
        value = torch.empty(count, dtype=payload.dtype, device=dev)
        with _on(dev):
            check(_lib.load().psa_unique_write_reduce(REDUCE_ID[reduce], _DTYPE_ID[payload.dtype], _ptr(sorted_keys), n, int(N),
                                                      _ptr(ws), _ptr(count_d), _ptr(index), _ptr(payload), _ptr(value), _stream()))
        return count, index[0], index[1], value
    count, ptr, row, col = unique_sorted(sorted_keys, N, want_ptr=count < n, _counted=counted)
    return count, row, col, (payload if count == n else _segment_csr_raw(payload, ptr, reduce))


# ---------------------------------------------------------------------------
# SpMM backward
# ---------------------------------------------------------------------------

def _f32(x: torch.Tensor, name: str) -> torch.Tensor:
    _gpu(x, name)
    if x.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {x.dtype})")
    return x.contiguous()


def spmm_value_bw(row, rowptr, col, mat, grad, reduce: str = "sum") -> torch.Tensor:
    """Upstream spmm_value_bw(row, rowptr, col, mat, grad, reduce): gradient
    wrt the nnz values for sum/mean.  `row` is accepted for signature parity
    but not read (one wave per CSR row knows its row)."""
    rowptr, col = _index(rowptr, "rowptr"), _index(col, "col")
    mat, grad = _f32(mat, "mat"), _f32(grad, "grad")
    if reduce not in ("sum", "add", "mean"):
        raise ValueError("spmm_value_bw: reduce must be sum or mean")
    M, K, nnz = rowptr.numel() - 1, mat.shape[1], col.numel()
    if grad.shape != (M, K):
        raise ValueError("grad must be [M, K]")
    out = torch.empty(nnz, dtype=torch.float32, device=mat.device)
    lib = _lib.load()
    ws_bytes = lib.psa_spmm_value_bw_workspace_bytes(nnz)
    ws = _workspace(ws_bytes, mat.device) if ws_bytes else None
    with _on(mat.device):
        check(lib.psa_spmm_value_bw(REDUCE_ID[reduce], _ptr(rowptr), _ptr(col), _ptr(mat),
                                    _ptr(grad), M, K, nnz, _ptr(out), _ptr(ws), ws_bytes, _stream()))
    return out


def transpose_weights(value, csr2csc, row_csc, rowptr, mean: bool) -> torch.Tensor:
    """Edge weights in CSC order for gB = A^T gOut (value[csr2csc], scaled by
    1/deg(row) for mean)."""
    csr2csc = _index(csr2csc, "csr2csc")
    nnz = csr2csc.numel()
    if value is not None:
        value = _f32(value, "value")
    if mean:
        row_csc, rowptr = _index(row_csc, "row_csc"), _index(rowptr, "rowptr")
    out = torch.empty(nnz, dtype=torch.float32, device=csr2csc.device)
    with _on(csr2csc.device):
        check(_lib.load().psa_transpose_weights(_ptr(value), _ptr(csr2csc),
                                                _ptr(row_csc) if mean else None,
                                                _ptr(rowptr) if mean else None,
                                                nnz, int(mean), _ptr(out), _stream()))
    return out


def spmm_minmax_bw(col, value, mat, grad, arg_out, want_value: bool = True, want_mat: bool = True):
    """Backward of spmm_min / spmm_max through arg_out.  Returns
    (grad_value | None, grad_mat | None)."""
    col = _index(col, "col")
    mat, grad = _f32(mat, "mat"), _f32(grad, "grad")
    _gpu(arg_out, "arg_out")
    arg_out = arg_out.contiguous()
    if value is not None:
        value = _f32(value, "value")
    (N, K), M, nnz = mat.shape, grad.shape[0], col.numel()
    gv = torch.empty(nnz, dtype=torch.float32, device=mat.device) if want_value else None
    gm = torch.empty((N, K), dtype=torch.float32, device=mat.device) if want_mat else None
    with _on(mat.device):
        check(_lib.load().psa_spmm_minmax_bw(_ptr(col), _ptr(value), _ptr(mat), _ptr(grad),
                                             _ptr(arg_out), M, N, K, nnz, _ptr(gv), _ptr(gm),
                                             _stream()))
    return gv, gm


def csc_edge_tags(rowptr, row_csc, csr2csc, width: int = 1) -> torch.Tensor:
    """Position of every CSC-ordered edge inside its CSR row, in the form of arg_bytes:
    width 1 -> uint8[nnz] (mod 128; bit 7 marks rows of more than 128 edges), width 2 ->
    int16[nnz] (mod 65 536).  Structure only — cache it next to csr2csc."""
    if width not in (1, 2):
        raise ValueError("width must be 1 or 2")
    rowptr, row_csc, csr2csc = _index(rowptr, "rowptr"), _index(row_csc, "row_csc"), _index(csr2csc, "csr2csc")
    tag = torch.empty(csr2csc.numel(), dtype=torch.int16 if width == 2 else torch.uint8, device=csr2csc.device)
    with _on(csr2csc.device):
        check(_lib.load().psa_csc_edge_tags(_ptr(rowptr), _ptr(row_csc), _ptr(csr2csc),
                                            csr2csc.numel(), _ptr(tag), width, _stream()))
    return tag


def minmax_bw_csc_supported(K: int) -> bool:
    return K % 4 == 0 and 0 < K <= 256


def spmm_minmax_bw_csc(rowptr, colptr, row_csc, csr2csc, tag, value, mat, grad, arg_out,
                       want_value: bool = True, csc2csr: Optional[torch.Tensor] = None,
                       arg_bytes: Optional[torch.Tensor] = None, hot_ids: Optional[torch.Tensor] = None,
                       to_csr_plan: Optional["PermutePlan"] = None, value_csc: Optional[torch.Tensor] = None,
                       hot_bytes_tail: Optional[torch.Tensor] = None):
    """Backward of spmm_min / spmm_max in one pass over the CSC view, no atomics
    (see include/paddle_sparse_hip.h).  Returns (grad_value f32[nnz] | None,
    grad_mat f32[N, K]); grad_value is in CSR order (the pass writes it in CSC
    order, `csc2csr` — computed here when not given — brings it back).
    tag / arg_bytes: uint8 (one byte per entry) or int16 (two).  hot_ids: int64[h]
    rows of grad / arg_bytes that row_csc refers to as M + position (compact copies
    of them are gathered here; needs arg_bytes exact, arg_out None).  hot_bytes_tail: int16[t, K], the
    row-local winners of the LAST t rows hot_ids names, given instead of gathered (the pieces of rows above
    65 535 entries, SparseStorage._huge_backward_plan)."""
    rowptr, colptr = _index(rowptr, "rowptr"), _index(colptr, "colptr")
    row_csc, csr2csc = _index(row_csc, "row_csc"), _index(csr2csc, "csr2csc")
    grad = _aligned16(_f32(grad, "grad"))
    if arg_out is None and arg_bytes is None:
        raise ValueError("spmm_minmax_bw_csc needs arg_out or arg_bytes")
    if arg_out is not None:
        _gpu(arg_out, "arg_out")
        arg_out = arg_out.contiguous()
    if value is not None:
        value = _f32(value, "value")
    edge_ids = csr2csc
    if value_csc is not None:
        if arg_out is not None:
            raise ValueError("value_csc goes with the exact arg_bytes forms (arg_out is compared with CSR edge ids)")
        value, edge_ids = _f32(value_csc, "value_csc"), None
    _gpu(tag, "tag")
    if tag.dtype not in (torch.uint8, torch.int16) or tag.numel() != csr2csc.numel():
        raise ValueError("tag must be uint8[nnz] or int16[nnz] (ops.csc_edge_tags)")
    width = tag.element_size()
    (M, K), N, nnz = grad.shape, colptr.numel() - 1, csr2csc.numel()
    if arg_out is not None and (arg_out.shape != grad.shape or arg_out.dtype != torch.int64):
        raise ValueError("arg_out must be int64[M, K] like grad")
    if arg_bytes is not None:
        _gpu(arg_bytes, "arg_bytes")
        if arg_bytes.dtype != tag.dtype or arg_bytes.shape != grad.shape or not arg_bytes.is_contiguous():
            raise ValueError("arg_bytes must be a contiguous [M, K] tensor of the tags' dtype (the third result of ops._spmm)")
    hot_grad = hot_bytes = None
    num_hot = 0
    if hot_ids is not None and hot_ids.numel():
        if arg_bytes is None or arg_out is not None or width != 2:
            raise ValueError("hot_ids need an exact arg_bytes in the two-byte form and no arg_out")
        hot_ids = _index(hot_ids, "hot_ids")
        num_hot = hot_ids.numel()
        hot_grad, hot_bytes = _gather_rows_raw(grad, hot_ids), _hot_bytes(arg_bytes, hot_ids, hot_bytes_tail)
    gv = None
    if want_value:
        mat = _aligned16(_f32(mat, "mat"))
        if mat.shape != (N, K):
            raise ValueError("mat must be [N, K]")
        gv = torch.empty(nnz, dtype=torch.float32, device=grad.device)
    gm = torch.empty((N, K), dtype=torch.float32, device=grad.device)
    lib = _lib.load()
    ws = _workspace(lib.psa_spmm_minmax_bw_csc_workspace_bytes(M, K, nnz), grad.device)
    with _on(grad.device):
        check(lib.psa_spmm_minmax_bw_csc(_ptr(rowptr), _ptr(colptr), _ptr(row_csc), _ptr(edge_ids),
                                         _ptr(tag.contiguous()), _ptr(value),
                                         _ptr(mat) if want_value else None, _ptr(grad), _ptr(arg_out),
                                         _ptr(arg_bytes), width, _ptr(hot_grad), _ptr(hot_bytes), num_hot,
                                         M, N, K, nnz, _ptr(gv), _ptr(gm), _ptr(ws), ws.numel(), _stream()))
    if gv is not None:
        if to_csr_plan is not None:
            gv = permute_apply(gv, to_csr_plan)
        else:
            gv = gather_rows(gv, csc2csr if csc2csr is not None else invert_permutation(csr2csc))
    return gv, gm


def _hot_bytes(arg_bytes: torch.Tensor, hot_ids: torch.Tensor, tail: Optional[torch.Tensor]) -> torch.Tensor:
    """Compact copy of the rows `hot_ids` of arg_bytes; the last len(tail) rows are `tail` itself."""
    if tail is None or tail.shape[0] == 0:
        return _gather_rows_raw(arg_bytes, hot_ids)
    _gpu(tail, "hot_bytes_tail")
    t = tail.shape[0]
    if tail.dtype != arg_bytes.dtype or tail.dim() != 2 or tail.shape[1] != arg_bytes.shape[1] or t > hot_ids.numel():
        raise ValueError("hot_bytes_tail must be [t <= len(hot_ids), K] of arg_bytes' dtype")
    out = torch.empty((hot_ids.numel(), arg_bytes.shape[1]), dtype=arg_bytes.dtype, device=arg_bytes.device)
    head = hot_ids.numel() - t
    if head:
        out[:head] = _gather_rows_raw(arg_bytes, hot_ids[:head])
    out[head:] = tail
    return out


def spmm_minmax_bw_eb(colptr, col_csc, row_csc, tag, weight_csc, grad, arg_bytes, hot_ids=None,
                      hot_bytes_tail: Optional[torch.Tensor] = None) -> torch.Tensor:
    """grad_mat f32[N, K] of spmm_min / spmm_max for a fixed adjacency, by the edge-range kernels over
    the CSC view (psa_spmm_minmax_bw_eb): power-law matrices.  col_csc: column of every CSC-ordered
    entry or None; tag / arg_bytes: uint8 or int16 (exact form); weight_csc: value[csr2csc] or None;
    hot_ids: rows of grad / arg_bytes that row_csc names as M + position (copies gathered here)."""
    colptr, row_csc = _index(colptr, "colptr"), _index(row_csc, "row_csc")
    if col_csc is not None:
        col_csc = _index(col_csc, "col_csc")
    grad = _aligned16(_f32(grad, "grad"))
    _gpu(tag, "tag")
    _gpu(arg_bytes, "arg_bytes")
    if tag.dtype not in (torch.uint8, torch.int16) or arg_bytes.dtype != tag.dtype or arg_bytes.shape != grad.shape:
        raise ValueError("tag / arg_bytes must be uint8 or int16, arg_bytes [M, K] like grad")
    arg_bytes, tag = arg_bytes.contiguous(), tag.contiguous()
    if weight_csc is not None:
        weight_csc = _f32(weight_csc, "weight_csc")
    (M, K), N, nnz = grad.shape, colptr.numel() - 1, row_csc.numel()
    hot_grad = hot_bytes = None
    num_hot = 0
    if hot_ids is not None and hot_ids.numel():
        hot_ids = _index(hot_ids, "hot_ids")
        num_hot = hot_ids.numel()
        hot_grad, hot_bytes = _gather_rows_raw(grad, hot_ids), _hot_bytes(arg_bytes, hot_ids, hot_bytes_tail)
    gm = torch.empty((N, K), dtype=torch.float32, device=grad.device)
    lib = _lib.load()
    ws = _workspace(lib.psa_spmm_minmax_bw_eb_workspace_bytes(K, nnz), grad.device)
    with _on(grad.device):
        check(lib.psa_spmm_minmax_bw_eb(_ptr(colptr), _ptr(col_csc), _ptr(row_csc), _ptr(tag), _ptr(weight_csc), _ptr(grad),
                                        _ptr(arg_bytes), tag.element_size(), _ptr(hot_grad), _ptr(hot_bytes), num_hot,
                                        M, N, K, nnz, _ptr(gm), _ptr(ws), ws.numel(), _stream()))
    return gm


def spmm_sum_bw_csc(colptr, row_csc, csr2csc, value, mat, grad, want_value: bool = True,
                    csc2csr: Optional[torch.Tensor] = None, row_scale: Optional[torch.Tensor] = None,
                    hot_ids: Optional[torch.Tensor] = None, to_csr_plan: Optional["PermutePlan"] = None,
                    value_csc: Optional[torch.Tensor] = None):
    """sum backward, both gradients in one pass over the CSC view (see
    include/paddle_sparse_hip.h).  Returns (grad_value f32[nnz] | None, in CSR
    order, grad_mat f32[N, K]).  For mean, pass row_scale = 1 / max(deg, 1)
    (f32[M]): it multiplies both gradients per edge.  hot_ids: int64[h] rows of grad
    that row_csc refers to as M + position (a compact copy is gathered here)."""
    colptr, row_csc, csr2csc = _index(colptr, "colptr"), _index(row_csc, "row_csc"), _index(csr2csc, "csr2csc")
    grad = _aligned16(_f32(grad, "grad"))
    if value is not None:
        value = _f32(value, "value")
    (M, K), N, nnz = grad.shape, colptr.numel() - 1, csr2csc.numel()
    if value_csc is not None:  # value[csr2csc] at hand (SparseStorage._permute_plan("to_csc")): the pass reads it as a stream
        value, edge_ids = _f32(value_csc, "value_csc"), None
    else:
        edge_ids = csr2csc
    hot_grad, num_hot = None, 0
    if hot_ids is not None and hot_ids.numel():
        hot_ids = _index(hot_ids, "hot_ids")
        num_hot = hot_ids.numel()
        hot_grad = _gather_rows_raw(grad, hot_ids)
    if row_scale is not None:
        row_scale = _f32(row_scale, "row_scale")
        if row_scale.shape != (M,):
            raise ValueError("row_scale must be f32[M]")
        if num_hot:
            row_scale = torch.cat([row_scale, row_scale[hot_ids]])
    gv = None
    if want_value:
        mat = _aligned16(_f32(mat, "mat"))
        if mat.shape != (N, K):
            raise ValueError("mat must be [N, K]")
        gv = torch.empty(nnz, dtype=torch.float32, device=grad.device)
    gm = torch.empty((N, K), dtype=torch.float32, device=grad.device)
    lib = _lib.load()
    ws = _workspace(lib.psa_spmm_sum_bw_csc_workspace_bytes(K, nnz), grad.device)
    with _on(grad.device):
        check(lib.psa_spmm_sum_bw_csc(_ptr(colptr), _ptr(row_csc), _ptr(edge_ids), _ptr(value),
                                      _ptr(row_scale), _ptr(mat) if want_value else None, _ptr(grad),
                                      _ptr(hot_grad), num_hot, M, N, K, nnz,
                                      _ptr(gv), _ptr(gm), _ptr(ws), ws.numel(), _stream()))
    if gv is not None:
        if to_csr_plan is not None:
            gv = permute_apply(gv, to_csr_plan)
        else:
            gv = gather_rows(gv, csc2csr if csc2csr is not None else invert_permutation(csr2csc))
    return gv, gm


def half_sum_bw_csc_supported(K: int) -> bool:
    return K % 8 == 0 and 0 < K <= 512


def _half_long_workspace(K: int, nnz: int, device, long_columns: bool):
    """Scratch of the long-column path of the half-width passes over the CSC view (chunk list + fp32 partials)."""
    if not long_columns:
        return None
    nbytes = _lib.load().psa_spmm_half_bw_csc_workspace_bytes(K, nnz)
    return _workspace(nbytes, device) if nbytes else None


def spmm_half_sum_bw_csc(colptr, row_csc, weight_csc, mat, grad, want_value: bool = True,
                         row_scale: Optional[torch.Tensor] = None, long_columns: bool = True):
    """sum / mean backward over the CSC view with fp16 / bf16 dense operands (psa_spmm_half_sum_bw_csc):
    returns (grad_value f32[nnz] IN CSC ORDER | None, grad_mat [N, K] in grad's dtype).  weight_csc:
    f32[nnz] = value[csr2csc] or None; row_scale f32[M] (mean) or None.  The caller brings
    grad_value to CSR order (SparseStorage._permute_plan("to_csr") / csc2csr).  long_columns=False: the caller
    knows that no column has more than 128 entries (the view's _longest_row()) and saves the two near-empty launches."""
    colptr, row_csc = _index(colptr, "colptr"), _index(row_csc, "row_csc")
    _gpu(grad, "grad")
    if grad.dtype not in (torch.float16, torch.bfloat16) or grad.dim() != 2:
        raise TypeError("grad must be a 2-D float16 / bfloat16 tensor")
    grad = _aligned16(grad.contiguous())
    (M, K), N, nnz = grad.shape, colptr.numel() - 1, row_csc.numel()
    if weight_csc is not None:
        weight_csc = _f32(weight_csc, "weight_csc")
    if row_scale is not None:
        row_scale = _f32(row_scale, "row_scale")
        if row_scale.shape != (M,):
            raise ValueError("row_scale must be f32[M]")
    gv = None
    if want_value:
        _gpu(mat, "mat")
        if mat.dtype != grad.dtype or mat.shape != (N, K):
            raise ValueError("mat must be [N, K] in grad's dtype")
        mat = _aligned16(mat.contiguous())
        gv = torch.empty(nnz, dtype=torch.float32, device=grad.device)
    gm = torch.empty((N, K), dtype=grad.dtype, device=grad.device)
    ws = _half_long_workspace(K, nnz, grad.device, long_columns)
    with _on(grad.device):
        check(_lib.load().psa_spmm_half_sum_bw_csc(_DTYPE_ID[grad.dtype], _ptr(colptr), _ptr(row_csc), _ptr(weight_csc),
                                                   _ptr(row_scale), _ptr(mat) if want_value else None, _ptr(grad), M, N, K,
                                                   nnz, _ptr(gv), _ptr(gm), _ptr(ws), ws.numel() if ws is not None else 0,
                                                   _stream()))
    return gv, gm


def spmm_half_minmax_bw_csc(colptr, row_csc, tag, weight_csc, mat, grad, arg_bytes, want_value: bool = True,
                            long_columns: bool = True):
    """min / max backward over the CSC view with fp16 / bf16 dense operands (psa_spmm_half_minmax_bw_csc):
    returns (grad_value f32[nnz] IN CSC ORDER | None, grad_mat [N, K] in grad's dtype).  tag / arg_bytes:
    uint8 or int16, the exact row-local forms (ops.csc_edge_tags / the third result of ops._spmm)."""
    colptr, row_csc = _index(colptr, "colptr"), _index(row_csc, "row_csc")
    _gpu(grad, "grad")
    if grad.dtype not in (torch.float16, torch.bfloat16) or grad.dim() != 2:
        raise TypeError("grad must be a 2-D float16 / bfloat16 tensor")
    grad = _aligned16(grad.contiguous())
    (M, K), N, nnz = grad.shape, colptr.numel() - 1, row_csc.numel()
    _gpu(tag, "tag")
    _gpu(arg_bytes, "arg_bytes")
    if tag.dtype not in (torch.uint8, torch.int16) or arg_bytes.dtype != tag.dtype or arg_bytes.shape != grad.shape or tag.numel() != nnz:
        raise ValueError("tag / arg_bytes must be uint8 or int16, tag [nnz], arg_bytes [M, K] like grad")
    arg_bytes, tag = arg_bytes.contiguous(), tag.contiguous()
    if weight_csc is not None:
        weight_csc = _f32(weight_csc, "weight_csc")
    gv = None
    if want_value:
        _gpu(mat, "mat")
        if mat.dtype != grad.dtype or mat.shape != (N, K):
            raise ValueError("mat must be [N, K] in grad's dtype")
        mat = _aligned16(mat.contiguous())
        gv = torch.empty(nnz, dtype=torch.float32, device=grad.device)
    gm = torch.empty((N, K), dtype=grad.dtype, device=grad.device)
    ws = _half_long_workspace(K, nnz, grad.device, long_columns)
    with _on(grad.device):
        check(_lib.load().psa_spmm_half_minmax_bw_csc(_DTYPE_ID[grad.dtype], _ptr(colptr), _ptr(row_csc), _ptr(tag),
                                                      _ptr(weight_csc), _ptr(mat) if want_value else None, _ptr(grad),
                                                      _ptr(arg_bytes), tag.element_size(), M, N, K, nnz, _ptr(gv), _ptr(gm),
                                                      _ptr(ws), ws.numel() if ws is not None else 0, _stream()))
    return gv, gm


def bincount(index: torch.Tensor, size: int) -> torch.Tensor:
    """int64[size] occurrence counts (colcount, storage.py:414-418)."""
    index = _index(index, "index")
    out = torch.empty(size, dtype=torch.int64, device=index.device)
    with _on(index.device):
        check(_lib.load().psa_bincount(_ptr(index), index.numel(), size, _ptr(out), _stream()))
    return out


def count2ptr(counts: torch.Tensor) -> torch.Tensor:
    """[0, cumsum(counts)] as int64[n+1] (colptr, storage.py:397-398)."""
    counts = _index(counts, "counts")
    n = counts.numel()
    out = torch.empty(n + 1, dtype=torch.int64, device=counts.device)
    lib = _lib.load()
    ws = _workspace(lib.psa_count2ptr_workspace_bytes(n), counts.device)
    with _on(counts.device):
        check(lib.psa_count2ptr(_ptr(counts), n, _ptr(out), _ptr(ws), ws.numel(), _stream()))
    return out


def scatter(src: torch.Tensor, index: torch.Tensor, dim_size: int, reduce: str = "sum") -> torch.Tensor:
    """paddle_scatter.scatter(src, index, 0, None, dim_size, reduce) as called
    by reduce.py:42 (reduction over sparse dim 0, index = col)."""
    _gpu(src, "src")
    index = _index(index, "index")
    if src.dtype not in (torch.float32, torch.float64, torch.int32, torch.int64):
        raise TypeError(f"scatter: unsupported dtype {src.dtype}")
    src = src.contiguous()
    if src.shape[0] != index.numel():
        raise ValueError("src.shape[0] must equal index.numel()")
    D = 1
    for s in src.shape[1:]:
        D *= s
    out = torch.empty((dim_size,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    lib = _lib.load()
    ws = _workspace(lib.psa_scatter_workspace_bytes(dim_size), src.device)
    with _on(src.device):
        check(lib.psa_scatter_reduce(REDUCE_ID[reduce], _DTYPE_ID[src.dtype], _ptr(src), _ptr(index),
                                     index.numel(), D, dim_size, _ptr(out), _ptr(ws), ws.numel(),
                                     _stream()))
    return out


def spspmm_count(colA: torch.Tensor, rowptrB: torch.Tensor) -> torch.Tensor:
    """counts[e] = stored entries of B's row colA[e] (products A entry e takes part in)."""
    colA, rowptrB = _index(colA, "colA"), _index(rowptrB, "rowptrB")
    out = torch.empty_like(colA)
    with _on(colA.device):
        check(_lib.load().psa_spspmm_count(_ptr(colA), colA.numel(), _ptr(rowptrB), _ptr(out),
                                           _stream()))
    return out


def spspmm_expand(rowA, colA, valA, rowptrB, colB, valB, offsets, owner, total: int, n: int,
                  dtype: torch.dtype):
    """All `total` partial products of A @ B as (key = i * n + j, value) pairs,
    in A-storage order (see csrc/spspmm.hip)."""
    rowA, colA = _index(rowA, "rowA"), _index(colA, "colA")
    rowptrB, colB = _index(rowptrB, "rowptrB"), _index(colB, "colB")
    offsets, owner = _index(offsets, "offsets"), _index(owner, "owner")
    if dtype not in (torch.float32, torch.float64, torch.int32, torch.int64):
        raise TypeError(f"spspmm: unsupported dtype {dtype}")
    for name, v, cnt in (("valueA", valA, colA.numel()), ("valueB", valB, colB.numel())):
        if v is not None:
            _gpu(v, name)
            if v.dtype != dtype or v.dim() != 1 or v.numel() != cnt or not v.is_contiguous():
                raise ValueError(f"{name} must be a contiguous 1-D {dtype} tensor with one entry per index")
    has_value = valA is not None or valB is not None
    keys = torch.empty(total, dtype=torch.int64, device=colA.device)
    vals = torch.empty(total, dtype=dtype, device=colA.device) if has_value else None
    with _on(colA.device):
        check(_lib.load().psa_spspmm_expand(_DTYPE_ID[dtype], _ptr(rowA), _ptr(colA), _ptr(valA),
                                            _ptr(rowptrB), _ptr(colB), _ptr(valB), _ptr(offsets),
                                            _ptr(owner), int(total), int(n), _ptr(keys), _ptr(vals),
                                            _stream()))
    return keys, vals


def sample_adj(rowptr: torch.Tensor, col: torch.Tensor, idx: torch.Tensor, num_neighbors: int,
               replace: bool = False, seed: int = 0, num_cols: Optional[int] = None,
               cum: Optional[torch.Tensor] = None
               ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """paddle_sparse_ops.sample_adj(rowptr, col, idx, num_neighbors, replace)
    (csrc/sample.cpp:8-24, CPU text csrc/cpu/sample_cpu.cpp:9-148) on GPU
    tensors: returns (out_rowptr, out_col, n_id, e_id).  `seed` selects the
    counter-based random stream (see include/paddle_sparse_hip.h); `num_cols`
    (exclusive bound on col, known to the SparseTensor caller) saves the
    col.max() pass that sizes the relabel scratch.

    cum (row_cdf of the entries' weights) makes the picks weighted: slot t of subset row i
    takes the entry the weighted pick of (stream i, draw t) finds in the row's cum, and a row
    whose total is zero makes no picks.  Only the count and the select step differ; weighted
    picks without replacement (num_neighbors >= 0, replace False) are not implemented."""
    rowptr, col, idx = _index(rowptr, "rowptr"), _index(col, "col"), _index(idx, "idx")
    if cum is not None:
        cum = _cdf(cum, col.numel())
        if int(num_neighbors) >= 0 and not replace:
            raise NotImplementedError("sample_adj: weighted picks without replacement are not implemented")
    dev = rowptr.device
    lib = _lib.load()
    S, k, rep, seed = idx.numel(), int(num_neighbors), int(bool(replace)), int(seed) & (2**64 - 1)
    num_nodes = rowptr.numel() - 1
    with _on(dev):
        counts = torch.empty(S, dtype=torch.int64, device=dev)
        if cum is None:
            check(lib.psa_sample_count(_ptr(rowptr), _ptr(idx), S, k, rep, _ptr(counts), _stream()))
        else:
            check(lib.psa_sample_count_weighted(_ptr(rowptr), _ptr(cum), _ptr(idx), S, k, rep, _ptr(counts), _stream()))
        out_rowptr = count2ptr(counts)
        E = int(out_rowptr[-1].item())
        owner = ptr2ind(out_rowptr, E)
        e_raw = torch.empty(E, dtype=torch.int64, device=dev)
        if cum is None:
            check(lib.psa_sample_select(_ptr(rowptr), _ptr(idx), S, _ptr(out_rowptr), _ptr(owner), E,
                                        k, rep, seed, _ptr(e_raw), _stream()))
        else:
            check(lib.psa_sample_select_weighted(_ptr(rowptr), _ptr(cum), _ptr(idx), S, _ptr(out_rowptr), _ptr(owner),
                                                 E, k, rep, seed, _ptr(e_raw), _stream()))
        # node ids live in [0, max(num_rows, num_cols)): col values index newid too
        if num_cols is not None:
            n_scratch = max(num_nodes, int(num_cols))
        else:
            n_scratch = max(num_nodes, int(col.max().item()) + 1 if col.numel() else 0) if E else num_nodes
        newid = torch.empty(n_scratch, dtype=torch.int64, device=dev)
        flags = torch.empty(E, dtype=torch.int64, device=dev)
        check(lib.psa_relabel_mark(_ptr(idx), S, _ptr(col), _ptr(e_raw), E, n_scratch,
                                   _ptr(newid), _ptr(flags), _stream()))
        rank = count2ptr(flags)
        n_out = S + int(rank[-1].item())
        n_id = torch.empty(n_out, dtype=torch.int64, device=dev)
        keys = torch.empty(E, dtype=torch.int64, device=dev)
        check(lib.psa_relabel_finish(_ptr(idx), S, _ptr(col), _ptr(e_raw), E, _ptr(newid),
                                     _ptr(rank), _ptr(owner), n_out, _ptr(n_id), _ptr(keys),
                                     _stream()))
    if E == 0:
        return out_rowptr, keys, n_id, e_raw
    keys, perm = index_sort(keys, max(S * n_out, 1), with_sorted_inputs=True, check=True)
    _, out_col = split_keys(keys, n_out, want_hi=False)
    return out_rowptr, out_col, n_id, gather_rows(e_raw, perm)


# ---- diagonal ops (csrc/diag.hip) ------------------------------------------------

def _row_bytes(x: torch.Tensor) -> int:
    b = x.element_size()
    for s in x.shape[1:]:
        b *= s
    return b


def diag_extent(M: int, N: int, k: int) -> Tuple[int, int]:
    """(start, num_diag) of the k-th diagonal of an M x N matrix: its cells are (r, r + k)
    for r in [start, start + num_diag)."""
    n = min(M, N - k) if k >= 0 else min(M + k, N)
    return max(-k, 0), max(n, 0)


class DiagPlan:
    """What psa_diag_count left behind for psa_diag_write: the result's row pointer and
    row lengths (its caches), the adjusted column counts, and the workspace."""

    def __init__(self, M, N, k, insert, nnz, rowcount, rowptr, colcount, nnz_out, ws):
        self.M, self.N, self.k, self.insert, self.nnz = M, N, k, insert, nnz
        self.rowcount, self.rowptr, self.colcount, self.nnz_out, self.ws = rowcount, rowptr, colcount, nnz_out, ws


def diag_count(rowptr: torch.Tensor, col: torch.Tensor, M: int, N: int, k: int, insert: bool,
               colcount: Optional[torch.Tensor] = None) -> DiagPlan:
    """Count pass of remove_diag (insert=False) / set_diag (insert=True) and the one host
    read: the output size rowptr'[M]."""
    rowptr, col = _index(rowptr, "rowptr"), _index(col, "col")
    if rowptr.numel() != M + 1:
        raise ValueError("rowptr must have M + 1 entries")
    if colcount is not None:
        colcount = _index(colcount, "colcount")
    dev = rowptr.device
    lib = _lib.load()
    rowcount = torch.empty(M, dtype=torch.int64, device=dev)
    rowptr_out = torch.empty(M + 1, dtype=torch.int64, device=dev)
    colcount_out = torch.empty(N, dtype=torch.int64, device=dev) if colcount is not None else None
    ws = _workspace(lib.psa_diag_workspace_bytes(M), dev)
    with _on(dev):
        check(lib.psa_diag_count(_ptr(rowptr), _ptr(col), M, N, int(k), int(bool(insert)), _ptr(colcount),
                                 _ptr(rowcount), _ptr(rowptr_out), _ptr(colcount_out), _ptr(ws), ws.numel(),
                                 _stream()))
        nnz_out = int(rowptr_out[M].item())
    return DiagPlan(M, N, int(k), bool(insert), col.numel(), rowcount, rowptr_out, colcount_out, nnz_out, ws)


def diag_write(plan: DiagPlan, rowptr: torch.Tensor, col: torch.Tensor, value: Optional[torch.Tensor],
               diag_values: Optional[torch.Tensor] = None, want_maps: bool = False):
    """Write pass: (col', value' or None, out_pos or None, diag_pos or None).  diag_values:
    [num_diag, *value.shape[1:]] of value's dtype (insert plans with values)."""
    rowptr, col = _index(rowptr, "rowptr"), _index(col, "col")
    dev = rowptr.device
    col_out = torch.empty(plan.nnz_out, dtype=torch.int64, device=dev)
    value_out = rb = None
    if value is not None:
        _gpu(value, "value")
        value = value.contiguous()
        rb = _row_bytes(value)
        value_out = torch.empty((plan.nnz_out,) + tuple(value.shape[1:]), dtype=value.dtype, device=dev)
        if plan.insert:
            if diag_values is None:
                raise ValueError("diag_values required to insert into a matrix with values")
            _gpu(diag_values, "diag_values")
            if (diag_values.dtype != value.dtype or diag_values.shape[1:] != value.shape[1:]
                    or diag_values.shape[0] != diag_extent(plan.M, plan.N, plan.k)[1]):
                raise ValueError("diag_values must be [num_diag, *value.shape[1:]] of value's dtype")
            diag_values = diag_values.contiguous()
    if value is None or not plan.insert:
        diag_values = None
    out_pos = diag_pos = None
    if want_maps:
        out_pos = torch.empty(plan.nnz, dtype=torch.int64, device=dev)
        if diag_values is not None:
            diag_pos = torch.empty(diag_values.shape[0], dtype=torch.int64, device=dev)
    with _on(dev):
        check(_lib.load().psa_diag_write(_ptr(rowptr), _ptr(col), _ptr(value), rb or 0, _ptr(diag_values),
                                         plan.M, plan.N, plan.k, int(plan.insert), plan.nnz, _ptr(plan.rowptr),
                                         plan.nnz_out, _ptr(plan.ws), _ptr(col_out), _ptr(value_out),
                                         _ptr(out_pos), _ptr(diag_pos), _stream()))
    return col_out, value_out, out_pos, diag_pos


def get_diag(rowptr: torch.Tensor, col: torch.Tensor, value: Optional[torch.Tensor], M: int, N: int,
             want_pos: bool = False):
    """(main diagonal [min(M, N), *value.shape[1:]], positions of the entries read or None).
    Value-less: float32 ones where an entry is stored."""
    rowptr, col = _index(rowptr, "rowptr"), _index(col, "col")
    dev = rowptr.device
    D = min(M, N)
    if value is not None:
        _gpu(value, "value")
        value = value.contiguous()
        if value.numel() == 0:  # no entries (or zero-width rows): nothing is stored on the diagonal
            pos = torch.full((D,), -1, dtype=torch.int64, device=dev) if want_pos else None
            return torch.zeros((D,) + tuple(value.shape[1:]), dtype=value.dtype, device=dev), pos
        out = torch.empty((D,) + tuple(value.shape[1:]), dtype=value.dtype, device=dev)
    else:
        out = torch.empty(D, dtype=torch.float32, device=dev)
    pos = torch.empty(D, dtype=torch.int64, device=dev) if want_pos else None
    with _on(dev):
        check(_lib.load().psa_get_diag(_ptr(rowptr), _ptr(col), _ptr(value), _row_bytes(value) if value is not None
                                       else 0, M, N, _ptr(out), _ptr(pos), _stream()))
    return out, pos


def diag_gather(src: torch.Tensor, index_map: torch.Tensor) -> torch.Tensor:
    """src[index_map] with zero rows where index_map is -1."""
    _gpu(src, "src")
    index_map = _index(index_map, "map")
    src = src.contiguous()
    out = torch.empty((index_map.numel(),) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    with _on(src.device):
        check(_lib.load().psa_diag_gather(_ptr(src), _ptr(index_map), index_map.numel(), _row_bytes(src),
                                          _ptr(out), _stream()))
    return out


def diag_scatter(src: torch.Tensor, pos: torch.Tensor, n: int) -> torch.Tensor:
    """zeros([n, *src.shape[1:]]) with row pos[i] = src[i] for pos[i] >= 0."""
    _gpu(src, "src")
    pos = _index(pos, "pos")
    src = src.contiguous()
    out = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    with _on(src.device):
        check(_lib.load().psa_diag_scatter(_ptr(src), _ptr(pos), pos.numel(), _row_bytes(src), _ptr(out),
                                           _stream()))
    return out


# ---- GraphSAINT random-walk sampler (csrc/walk.hip) --------------------------------

def random_walk(rowptr: torch.Tensor, col: torch.Tensor, start: torch.Tensor, walk_length: int,
                seed: int) -> torch.Tensor:
    """int64[S, walk_length + 1] walks of a square CSR matrix from start (int64[S]): the
    next node is a uniform draw among the current node's entries (the counter-based
    stream of sample_adj: walk n, step l), or the node itself when it has none.  Raises
    IndexError when a start lies outside the matrix (one host read)."""
    rowptr, col, start = _index(rowptr, "rowptr"), _index(col, "col"), _index(start, "start")
    L = int(walk_length)
    if L < 0:
        raise ValueError("walk_length must be >= 0")
    N, S, dev = rowptr.numel() - 1, start.numel(), rowptr.device
    out = torch.empty((S, L + 1), dtype=torch.int64, device=dev)
    if S == 0:
        return out
    flags = torch.zeros(1, dtype=torch.int64, device=dev)
    with _on(dev):
        check(_lib.load().psa_random_walk(_ptr(rowptr), _ptr(col), N, _ptr(start), S, L, int(seed) & (2**64 - 1),
                                          _ptr(out), _ptr(flags), _stream()))
        if int(flags.item()) & 1:
            raise IndexError(f"random_walk: a start node lies outside [0, {N})")
    return out


def random_walk_set_variant(variant: int) -> int:
    """Bench hook: the store scheme of psa_random_walk (0 = default); returns the previous one."""
    return _lib.load().psa_random_walk_set_variant(int(variant))


# ---- edge-weighted sampling (csrc/weighted.hip) -------------------------------------

CDF_NEGATIVE, CDF_NONFINITE, CDF_OVERFLOW = 1, 2, 4


def _cdf(cum: torch.Tensor, nnz: int) -> torch.Tensor:
    _gpu(cum, "cum")
    if cum.dtype != torch.float64 or cum.dim() != 1 or cum.numel() != nnz:
        raise ValueError(f"cum must be float64[{nnz}], the row CDF of this matrix")
    return cum.contiguous()


def row_cdf(rowptr: torch.Tensor, weight: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(cum float64[nnz], flags int64[1]): cum is the inclusive prefix sum of weight
    (float64[nnz]) inside every row, summed strictly left to right in float64, so that it is
    numpy's cumsum of the row bit for bit.  flags stays on the device (no host read here):
    CDF_NEGATIVE = a weight < 0, CDF_NONFINITE = a NaN or infinite weight, CDF_OVERFLOW = a
    row total that overflowed to infinity."""
    rowptr = _index(rowptr, "rowptr")
    _gpu(weight, "weight")
    if weight.dtype != torch.float64 or weight.dim() != 1:
        raise TypeError("weight must be a 1-D float64 tensor")
    weight = weight.contiguous()
    dev = rowptr.device
    cum = torch.empty_like(weight)
    flags = torch.zeros(1, dtype=torch.int64, device=dev)
    with _on(dev):
        check(_lib.load().psa_row_cdf(_ptr(rowptr), _ptr(weight), rowptr.numel() - 1, _ptr(cum), _ptr(flags),
                                      _stream()))
    return cum, flags


def weighted_pick_host(cum, r: int) -> int:
    """The weighted pick of the kernels, run on the host: the index picked in one row's cum
    (a sequence of floats) by the random word r, or -1 for no pick."""
    import ctypes

    row = [float(x) for x in cum]
    arr = (ctypes.c_double * max(len(row), 1))(*row)
    return int(_lib.load().psa_weighted_pick_host(ctypes.cast(arr, ctypes.c_void_p), len(row), int(r) & (2**64 - 1)))


def weighted_pick_without_host(cum, k: int, words_entry, words_gap) -> List[int]:
    """The weighted picks without replacement of neighbor_sample's kernels, run on the host
    (DESIGN 3.22): the indices picked in one row's cum (a sequence of floats) by up to k
    draws, in draw order; draw t uses the random words words_entry[t] and, from draw 1 on,
    words_gap[t] (sequences of k integers).  min(k, entries of positive weight) picks."""
    import ctypes

    row = [float(x) for x in cum]
    k = int(k)
    if k < 0 or len(words_entry) != k or len(words_gap) != k:
        raise ValueError("words_entry and words_gap must hold k words each, k >= 0")
    n = max(k, 1)
    arr = (ctypes.c_double * max(len(row), 1))(*row)
    we = (ctypes.c_uint64 * n)(*[int(r) & (2**64 - 1) for r in words_entry])
    wg = (ctypes.c_uint64 * n)(*[int(r) & (2**64 - 1) for r in words_gap])
    out = (ctypes.c_int64 * n)(*([-1] * n))
    as_ptr = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    count = int(_lib.load().psa_weighted_pick_without_host(as_ptr(arr), len(row), k, as_ptr(we), as_ptr(wg), as_ptr(out)))
    return [int(out[t]) for t in range(count)]


def random_walk_weighted(rowptr: torch.Tensor, col: torch.Tensor, cum: Optional[torch.Tensor], start: torch.Tensor,
                         walk_length: int, seed: int, return_edge_ids: bool = False):
    """random_walk with each step's entry drawn in proportion to its weight: cum is row_cdf
    of the weights (None: the uniform draw, the bits of random_walk).  A walk stays where it
    is at a node without entries or with a zero total.  With return_edge_ids the result is
    (walks int64[S, L + 1], e_id int64[S, L]): the storage position of every entry taken, -1
    where the walk stayed.  Raises IndexError when a start lies outside the matrix (one host
    read)."""
    rowptr, col, start = _index(rowptr, "rowptr"), _index(col, "col"), _index(start, "start")
    if cum is not None:
        cum = _cdf(cum, col.numel())
    L = int(walk_length)
    if L < 0:
        raise ValueError("walk_length must be >= 0")
    N, S, dev = rowptr.numel() - 1, start.numel(), rowptr.device
    out = torch.empty((S, L + 1), dtype=torch.int64, device=dev)
    e_id = torch.empty((S, L), dtype=torch.int64, device=dev) if return_edge_ids else None
    if S > 0:
        flags = torch.zeros(1, dtype=torch.int64, device=dev)
        with _on(dev):
            check(_lib.load().psa_random_walk_weighted(_ptr(rowptr), _ptr(col), _ptr(cum), N, _ptr(start), S, L,
                                                       int(seed) & (2**64 - 1), _ptr(out), _ptr(e_id), _ptr(flags),
                                                       _stream()))
            if int(flags.item()) & 1:
                raise IndexError(f"random_walk: a start node lies outside [0, {N})")
    return (out, e_id) if return_edge_ids else out


# ---- node2vec (p, q) walks (csrc/node2vec.hip) ---------------------------------------

NODE2VEC_ONE, NODE2VEC_MAX_TRIES = 2**53, 32768


def _node2vec_args(thr, max_tries):
    thr = tuple(int(t) for t in thr)
    if len(thr) != 3 or any(t < 0 or t > NODE2VEC_ONE for t in thr):
        raise ValueError("thr must be three integers in [0, 2^53]")
    max_tries = int(max_tries)
    if not 1 <= max_tries <= NODE2VEC_MAX_TRIES:
        raise ValueError(f"max_tries must lie in [1, {NODE2VEC_MAX_TRIES}]")
    return thr, max_tries


def node2vec_walk(rowptr: torch.Tensor, col: torch.Tensor, cum: Optional[torch.Tensor], start: torch.Tensor,
                  walk_length: int, seed: int, thr, max_tries: int, return_edge_ids: bool = False):
    """random_walk_weighted with node2vec's second-order bias: at every step after the first
    a proposed entry (the plain step's draw) is accepted when a 53-bit random word lies below
    thr[class], class 0 = back to the previous node t, 1 = a column row t stores, 2 = neither;
    after max_tries refusals the last proposal is taken (include/paddle_sparse_hip.h states
    the step in full).  thr: three integers in [0, 2^53]; rw.random_walk makes them from p
    and q.  cum None: uniform proposals.  Results and IndexError as random_walk_weighted."""
    rowptr, col, start = _index(rowptr, "rowptr"), _index(col, "col"), _index(start, "start")
    if cum is not None:
        cum = _cdf(cum, col.numel())
    thr, max_tries = _node2vec_args(thr, max_tries)
    L = int(walk_length)
    if L < 0:
        raise ValueError("walk_length must be >= 0")
    N, S, dev = rowptr.numel() - 1, start.numel(), rowptr.device
    out = torch.empty((S, L + 1), dtype=torch.int64, device=dev)
    e_id = torch.empty((S, L), dtype=torch.int64, device=dev) if return_edge_ids else None
    if S > 0:
        flags = torch.zeros(1, dtype=torch.int64, device=dev)
        with _on(dev):
            check(_lib.load().psa_node2vec_walk(_ptr(rowptr), _ptr(col), _ptr(cum), N, _ptr(start), S, L,
                                                int(seed) & (2**64 - 1), *thr, max_tries, _ptr(out), _ptr(e_id),
                                                _ptr(flags), _stream()))
            if int(flags.item()) & 1:
                raise IndexError(f"random_walk: a start node lies outside [0, {N})")
    return (out, e_id) if return_edge_ids else out


def node2vec_walk_host(rowptr, col, cum, start, walk_length: int, seed: int, thr, max_tries: int):
    """node2vec_walk run serially on the host by the kernel's own step (numpy arrays in,
    (nodes, e_id, flags) numpy out): what the CPU suite holds the restatement to.  flags has
    bit 0 when a start lies outside the matrix; that walk's rows are left at -7."""
    import numpy as np

    rowptr = np.ascontiguousarray(rowptr, np.int64)
    col = np.ascontiguousarray(col, np.int64)
    start = np.ascontiguousarray(start, np.int64)
    cum = None if cum is None else np.ascontiguousarray(cum, np.float64)
    S, L = start.size, int(walk_length)
    nodes = np.full((S, max(L, 0) + 1), -7, np.int64)
    e_id = np.full((S, max(L, 0)), -7, np.int64)
    flags = np.zeros(1, np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    check(_lib.load().psa_node2vec_walk_host(ptr(rowptr), ptr(col), ptr(cum), rowptr.size - 1, ptr(start), S, L,
                                             int(seed) & (2**64 - 1), *(int(t) for t in thr), int(max_tries),
                                             ptr(nodes), ptr(e_id), ptr(flags)))
    return nodes, e_id, int(flags[0])


# ---- edge lookup and negative sampling (csrc/negative.hip) ------------------------------

LOOKUP_RANGE, NEGATIVE_FAILED = 1, 2  # bits of the flags word
NEGATIVE_MAX_TRIES = 32768
NEGATIVE_POISON = -(2**62)


def _negative_out(out: Optional[torch.Tensor], n: int, dev, name: str) -> torch.Tensor:
    """The caller's output buffer (int64[n], contiguous, on dev) or a new one, which under the
    test hook _POISON_WORKSPACE starts as NEGATIVE_POISON (0xff bytes would read as -1, an
    answer): the kernels write every element."""
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=dev)
        return out.fill_(NEGATIVE_POISON) if _POISON_WORKSPACE else out
    _gpu(out, name)
    if out.dtype != torch.int64 or out.dim() != 1 or out.numel() != n or not out.is_contiguous() \
            or out.device != dev:
        raise ValueError(f"{name} must be a contiguous int64[{n}] tensor on {dev}")
    return out


def edge_lookup(rowptr: torch.Tensor, col: torch.Tensor, N: int, row_q: torch.Tensor, col_q: torch.Tensor,
                out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(pos int64[Q], flags int64[1]) for a CSR matrix of rowptr.numel() - 1 rows and N columns
    sorted by (row, col): pos[q] is the storage position of the first entry (row_q[q],
    col_q[q]), or -1 when it is not stored; a pair outside the matrix gives -1 and sets
    LOOKUP_RANGE in flags, which stays on the device (no host read here).  One launch; out,
    when given, receives pos."""
    rowptr, col = _index(rowptr, "rowptr"), _index(col, "col")
    row_q, col_q = _index(row_q, "row"), _index(col_q, "col")
    if row_q.numel() != col_q.numel():
        raise ValueError(f"row and col differ in length ({row_q.numel()}, {col_q.numel()})")
    M, N, Q, dev = rowptr.numel() - 1, int(N), row_q.numel(), rowptr.device
    if M < 0 or N < 0:
        raise ValueError("rowptr must not be empty and N must be >= 0")
    pos = _negative_out(out, Q, dev, "out")
    flags = torch.zeros(1, dtype=torch.int64, device=dev)
    if Q > 0:
        with _on(dev):
            check(_lib.load().psa_edge_lookup(_ptr(rowptr), _ptr(col), M, N, _ptr(row_q), _ptr(col_q), Q, _ptr(pos),
                                              _ptr(flags), _stream()))
    return pos, flags


def _negative_args(M: int, N: int, k: int, no_self_loops: bool, max_tries: int):
    k, max_tries = int(k), int(max_tries)
    if k < 1:
        raise ValueError("the number of samples per source must be >= 1")
    if not 1 <= max_tries <= NEGATIVE_MAX_TRIES:
        raise ValueError(f"max_tries must lie in [1, {NEGATIVE_MAX_TRIES}]")
    if no_self_loops and M != N:
        raise ValueError(f"no_self_loops needs a square matrix (got {(M, N)})")
    return k, max_tries


def negative_sample(rowptr: torch.Tensor, col: torch.Tensor, N: int, src: Optional[torch.Tensor], count: int,
                    no_self_loops: bool, max_tries: int, seed: int, out_row: Optional[torch.Tensor] = None,
                    out_col: Optional[torch.Tensor] = None):
    """Pairs that the sorted CSR matrix (rowptr.numel() - 1 rows, N columns) does not store,
    by at most max_tries proposals per sample from the counter-based stream of `seed`
    (include/paddle_sparse_hip.h states the step in full).  src None: `count` pairs with the
    row drawn too; returns (row int64[count], col int64[count], flags).  src int64[S]: `count`
    columns for every given row; returns (col int64[S * count], flags), sample i belonging to
    src[i // count].  A sample whose proposals were all refused is -1 and sets
    NEGATIVE_FAILED; a given row outside the matrix is -1 and sets LOOKUP_RANGE.  flags stays
    on the device (no host read here).  One launch; out_row / out_col, when given, receive the
    results."""
    rowptr, col = _index(rowptr, "rowptr"), _index(col, "col")
    M, N, dev = rowptr.numel() - 1, int(N), rowptr.device
    if M < 0 or N < 0:
        raise ValueError("rowptr must not be empty and N must be >= 0")
    count = int(count)
    if src is None:
        if count < 0:
            raise ValueError("the number of samples must be >= 0")
        S, k = count, 1
        _, max_tries = _negative_args(M, N, 1, no_self_loops, max_tries)
    else:
        src = _index(src, "src")
        S = src.numel()
        k, max_tries = _negative_args(M, N, count, no_self_loops, max_tries)
    row = _negative_out(out_row, S * k, dev, "out_row") if src is None else None
    cols = _negative_out(out_col, S * k, dev, "out_col")
    flags = torch.zeros(1, dtype=torch.int64, device=dev)
    if S > 0:
        with _on(dev):
            check(_lib.load().psa_negative_sample(_ptr(rowptr), _ptr(col), M, N, _ptr(src), S, k, int(bool(no_self_loops)),
                                                  max_tries, int(seed) & (2**64 - 1), _ptr(row), _ptr(cols),
                                                  _ptr(flags), _stream()))
    return (cols, flags) if src is not None else (row, cols, flags)


def edge_lookup_host(rowptr, col, N: int, row_q, col_q):
    """edge_lookup run serially on the host by the kernel's own step (numpy arrays in, (pos,
    flags) numpy out): what the CPU suite holds the restatement to.  pos starts at -7: every
    element is written."""
    import numpy as np

    rowptr, col = np.ascontiguousarray(rowptr, np.int64), np.ascontiguousarray(col, np.int64)
    row_q, col_q = np.ascontiguousarray(row_q, np.int64), np.ascontiguousarray(col_q, np.int64)
    if row_q.shape != col_q.shape or row_q.ndim != 1:
        raise ValueError("row and col must be 1-D and of one length")
    pos, flags = np.full(row_q.size, -7, np.int64), np.zeros(1, np.int64)
    check(_lib.load().psa_edge_lookup_host(rowptr.ctypes.data, col.ctypes.data, rowptr.size - 1, int(N),
                                           row_q.ctypes.data, col_q.ctypes.data, row_q.size, pos.ctypes.data,
                                           flags.ctypes.data))
    return pos, int(flags[0])


def negative_sample_host(rowptr, col, N: int, src, count: int, no_self_loops: bool, max_tries: int, seed: int):
    """negative_sample run serially on the host by the kernel's own step (numpy arrays in,
    numpy out, flags as an int): (row, col, flags) without src, (col, flags) with it.  The
    outputs start at -7: every element is written."""
    import numpy as np

    rowptr, col = np.ascontiguousarray(rowptr, np.int64), np.ascontiguousarray(col, np.int64)
    src = None if src is None else np.ascontiguousarray(src, np.int64)
    S, k = (int(count), 1) if src is None else (src.size, int(count))
    n = max(S, 0) * max(k, 0)
    row = np.full(n, -7, np.int64) if src is None else None
    cols, flags = np.full(n, -7, np.int64), np.zeros(1, np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    check(_lib.load().psa_negative_sample_host(ptr(rowptr), ptr(col), rowptr.size - 1, int(N), ptr(src), S, k,
                                               int(bool(no_self_loops)), int(max_tries), int(seed) & (2**64 - 1),
                                               ptr(row), ptr(cols), ptr(flags)))
    return (cols, int(flags[0])) if src is not None else (row, cols, int(flags[0]))


# ---- connected components (csrc/components.hip) -----------------------------------------

COMPONENTS_RANGE = 1  # bit of the flags word


def components_init(rowptr: torch.Tensor, col: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """parent int64[N], N = rowptr.numel() - 1: the first stored column of row v where it is a
    smaller node, else v.  One launch; out, when given, receives parent."""
    rowptr, col = _index(rowptr, "rowptr"), _index(col, "col")
    N, dev = rowptr.numel() - 1, rowptr.device
    if N < 0:
        raise ValueError("rowptr must not be empty")
    parent = _negative_out(out, N, dev, "out")
    with _on(dev):
        check(_lib.load().psa_components_init(_ptr(rowptr), _ptr(col), N, col.numel(), _ptr(parent), _stream()))
    return parent


def components_hook(row: torch.Tensor, col: torch.Tensor, parent: torch.Tensor) -> torch.Tensor:
    """Joins row[e] and col[e] in parent (int64[N] as components_init left it, updated in place)
    for every entry e; returns flags int64[1], which stays on the device: COMPONENTS_RANGE when
    an entry had an end outside [0, N) (it joins nothing).  One launch."""
    row, col = _index(row, "row"), _index(col, "col")
    if row.numel() != col.numel():
        raise ValueError(f"row and col differ in length ({row.numel()}, {col.numel()})")
    N, dev = parent.numel(), row.device
    _negative_out(parent, N, dev, "parent")
    flags = torch.zeros(1, dtype=torch.int64, device=dev)
    with _on(dev):
        check(_lib.load().psa_components_hook(_ptr(row), _ptr(col), row.numel(), N, _ptr(parent), _ptr(flags),
                                              _stream()))
    return flags


def components_flatten(parent: torch.Tensor, out_root: Optional[torch.Tensor] = None,
                       out_is_root: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(root int64[N], is_root int64[N] of 0 / 1) from the parent array that components_hook left
    (compressed in place along the way).  One launch; out_root / out_is_root, when given, receive
    the results."""
    N, dev = parent.numel(), parent.device
    _negative_out(parent, N, dev, "parent")
    root = _negative_out(out_root, N, dev, "out_root")
    is_root = _negative_out(out_is_root, N, dev, "out_is_root")
    with _on(dev):
        check(_lib.load().psa_components_flatten(_ptr(parent), N, _ptr(root), _ptr(is_root), _stream()))
    return root, is_root


def components_host(rowptr, row, col):
    """init, hook and flatten run serially on the host by the kernels' own steps (numpy arrays
    in, (parent, root, is_root, flags) numpy out, flags as an int): what the CPU suite holds the
    restatement to.  The outputs start at -7: every element is written."""
    import numpy as np

    rowptr, row, col = (np.ascontiguousarray(a, np.int64) for a in (rowptr, row, col))
    if row.shape != col.shape or row.ndim != 1 or rowptr.ndim != 1 or rowptr.size < 1:
        raise ValueError("row and col must be 1-D and of one length, rowptr 1-D and not empty")
    N = rowptr.size - 1
    parent, root, is_root = (np.full(N, -7, np.int64) for _ in range(3))
    flags = np.zeros(1, np.int64)
    check(_lib.load().psa_components_host(rowptr.ctypes.data, row.ctypes.data, col.ctypes.data, N, col.size,
                                          parent.ctypes.data, root.ctypes.data, is_root.ctypes.data, flags.ctypes.data))
    return parent, root, is_root, int(flags[0])


SAINT_DUPLICATES, SAINT_UNSORTED = 2, 4


def saint_subgraph(rowptr: torch.Tensor, col: torch.Tensor, node_idx: torch.Tensor):
    """The subgraph of a square CSR matrix induced by node_idx (int64[S]): returns
    (rowptr' int64[S+1], row', col', edge_index int64[nnz'], flags) in candidate order
    (selection order of the rows, storage order inside a row); col' = position of the
    column's node in node_idx, the last one for a duplicated node.  flags has
    SAINT_DUPLICATES when node_idx repeats a node and SAINT_UNSORTED when it decreases
    somewhere (only then is candidate order not sorted by (row', col')).  Two C-ABI calls
    and ONE host read; IndexError for a node outside the matrix."""
    rowptr, col, node_idx = _index(rowptr, "rowptr"), _index(col, "col"), _index(node_idx, "node_idx")
    N, S, dev = rowptr.numel() - 1, node_idx.numel(), rowptr.device
    lib = _lib.load()
    ws = _workspace(lib.psa_saint_workspace_bytes(S, N), dev)
    info = torch.empty(2, dtype=torch.int64, device=dev)
    with _on(dev):
        check(lib.psa_saint_count(_ptr(rowptr), _ptr(col), N, _ptr(node_idx), S, _ptr(ws), ws.numel(), _ptr(info),
                                  _stream()))
        nnz_out, flags = info.tolist()  # the one host read
        if flags & 1:
            raise IndexError(f"saint_subgraph: a node lies outside [0, {N})")
        rowptr_out = torch.empty(S + 1, dtype=torch.int64, device=dev)
        out = torch.empty((3, nnz_out), dtype=torch.int64, device=dev)
        check(lib.psa_saint_write(_ptr(rowptr), _ptr(col), N, _ptr(node_idx), S, _ptr(ws), nnz_out,
                                  _ptr(rowptr_out), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream()))
    return rowptr_out, out[0], out[1], out[2], flags


# ---- neighbor_sample (csrc/neighbor.hip) ------------------------------------------------------------

NEIGHBOR_DUP_SEED, NEIGHBOR_SEED_OUTSIDE, NEIGHBOR_COL_OUTSIDE = 1, 2, 4


class NeighborWorkspace:
    """The relabel map of neighbor_sample (int32[N] on the device) and whether it is clean.
    A clean map is reused as it is: a call then costs stores per touched node, not per node."""

    def __init__(self, num_nodes: int, device):
        nbytes = _lib.load().psa_neighbor_workspace_bytes(int(num_nodes))
        if nbytes == 0:
            raise ValueError(f"neighbor_sample needs N < 2^31 (got {num_nodes})")
        self.num_nodes, self.buf, self.clean = int(num_nodes), _workspace(nbytes, device), False


def neighbor_sample(rowptr: torch.Tensor, col: torch.Tensor, seeds: torch.Tensor, num_neighbors, replace: bool = False,
                    seed: int = 0, workspace: Optional[NeighborWorkspace] = None, stats: Optional[dict] = None,
                    want_edges: bool = True, cum: Optional[torch.Tensor] = None):
    """Multi-hop neighbour sampling of a square sorted CSR matrix: returns
    (n_id int64[n], rowptr' int64[n+1], col' int64[E], e_id int64[E], nodes_per_hop,
    edges_per_hop), the entries sorted (stable) by (row', col').  seeds int64[S], distinct
    (ValueError) and inside the matrix (IndexError); num_neighbors: one fan-out >= -1 per
    hop; -1 takes every entry.  A hop with fan-out k >= 0 is sized by its bound, (frontier
    nodes) * k slots of 28 bytes, before anything is counted, and that bound stays below
    2^31: to take all entries pass -1, which counts first, not a large k.
    Draw t of the node at local id i comes from stream i of `seed`, whatever the hop.
    One host read per hop (two when the fan-out is -1) and one behind the sort; stats (a
    dict, optional) receives host_reads and hops_run.  workspace: a NeighborWorkspace kept
    between calls.  want_edges=False stops after the node set (the caller induces the
    subgraph): no hop writes its entries and the edge outputs are None.  Not capturable in a graph: the sizes depend on
    the data.  N, n < 2^31.
    cum (float64[nnz] on the matrix's device, row_cdf of the entries' weights) makes the picks
    of every hop with a fan-out >= 0 weighted: with replacement slot t is the
    weighted pick of weighted sample_adj, without replacement the node draws its entries one
    after the other in proportion to the weights that are left and makes min(k, entries of
    positive weight) picks.  A fan-out of -1 takes every entry whatever its weight."""
    if cum is not None:  # checked before anything else looks at a tensor, and before any launch
        if not isinstance(cum, torch.Tensor):
            raise TypeError("cum must be a torch.Tensor")
        if cum.dtype != torch.float64:
            raise TypeError(f"cum must be float64 (got {cum.dtype})")
        if not isinstance(col, torch.Tensor) or cum.dim() != 1 or cum.numel() != col.numel():
            raise ValueError(f"cum must be float64[nnz], the row CDF of this matrix (got shape {tuple(cum.shape)})")
        if isinstance(rowptr, torch.Tensor) and cum.device != rowptr.device:
            raise ValueError(f"cum lies on {cum.device}, the matrix on {rowptr.device}")
    rowptr, col, seeds = _index(rowptr, "rowptr"), _index(col, "col"), _index(seeds, "seeds")
    if cum is not None:
        cum = cum.contiguous()
    if rowptr.numel() < 1:
        raise ValueError("rowptr must have at least one element")
    fanouts = [int(k) for k in num_neighbors]
    if any(k < -1 for k in fanouts):
        raise ValueError(f"num_neighbors must be >= -1 (got {fanouts})")
    N, S, dev = rowptr.numel() - 1, seeds.numel(), rowptr.device
    if N >= 2**31 or S >= 2**31:
        raise ValueError(f"neighbor_sample needs N < 2^31 and fewer than 2^31 seeds (got {N}, {S})")
    ws = workspace if workspace is not None else NeighborWorkspace(N, dev)
    if ws.num_nodes != N or ws.buf.device != dev:
        raise ValueError("the workspace belongs to another matrix or device")
    lib = _lib.load()
    rep, seed = int(bool(replace)), int(seed) & (2**64 - 1)
    count = {"host_reads": 0, "hops_run": 0}
    state = torch.empty(8, dtype=torch.int64, device=dev)
    empty = torch.empty(0, dtype=torch.int64, device=dev)
    nodes, rows, cols, edges = [seeds], [], [], []
    nodes_per_hop, edges_per_hop = [S], []

    def reset(hop_ws=None, slots=0):
        ids = torch.cat(nodes) if len(nodes) > 1 else nodes[0]
        check(lib.psa_neighbor_reset(_ptr(ids), ids.numel(), N, _ptr(col), _ptr(hop_ws), slots, _ptr(ws.buf),
                                     _stream()))
        ws.clean = True
        return ids

    def raise_on(flags, hop_ws=None, slots=0):
        if not flags:
            return
        reset(hop_ws, slots)
        if stats is not None:
            stats.update(count)
        if flags & NEIGHBOR_SEED_OUTSIDE:
            raise IndexError(f"neighbor_sample: a seed lies outside [0, {N})")
        if flags & NEIGHBOR_DUP_SEED:
            raise ValueError("neighbor_sample: the seeds must be distinct")
        raise ValueError(f"neighbor_sample: a stored column lies outside [0, {N})")

    with _on(dev):
        fresh, ws.clean = not ws.clean, False  # stays False if anything below raises: the next call refills
        check(lib.psa_neighbor_init(_ptr(seeds), S, N, int(fresh), _ptr(ws.buf), ws.buf.numel(), _ptr(state), _stream()))
        begin, end, frontier, checked = 0, S, seeds, False
        for k in fanouts:
            F, slots, fptr = (end - begin if col.numel() else 0), 0, None  # a matrix without entries: nothing to pick
            if F > 0 and k < 0:
                counts = torch.empty(F, dtype=torch.int64, device=dev)
                check(lib.psa_neighbor_hop_count(_ptr(rowptr), N, _ptr(frontier), F, _ptr(counts), _stream()))
                fptr = count2ptr(counts)
                slots = int(fptr[-1].item())
                count["host_reads"] += 1
            elif F > 0:
                slots = F * k
            n_edges = n_new = 0
            new = empty
            if slots > 0:
                nbytes = lib.psa_neighbor_hop_workspace_bytes(slots)
                if nbytes == 0:
                    reset()
                    raise ValueError(f"neighbor_sample: a hop of {slots} picks does not fit 2^31")
                hop_ws = _workspace(nbytes, dev)
                if cum is not None and k >= 0:
                    check(lib.psa_neighbor_hop_pick_weighted(_ptr(rowptr), _ptr(col), _ptr(cum), N, _ptr(frontier), F,
                                                             None, begin, k, rep, seed, slots, _ptr(ws.buf),
                                                             _ptr(hop_ws), hop_ws.numel(), _ptr(state), _stream()))
                else:
                    check(lib.psa_neighbor_hop_pick(_ptr(rowptr), _ptr(col), N, _ptr(frontier), F, _ptr(fptr), begin, k,
                                                    rep, seed, slots, _ptr(ws.buf), _ptr(hop_ws), hop_ws.numel(),
                                                    _ptr(state), _stream()))
                n_edges, n_new, flags = state[:3].tolist()  # the hop's host read
                count["host_reads"] += 1
                count["hops_run"] += 1
                checked = True
                raise_on(flags, hop_ws, slots)
                if end + n_new >= 2**31:
                    reset(hop_ws, slots)
                    raise ValueError("neighbor_sample: the sample has 2^31 nodes or more")
                new = torch.empty(n_new, dtype=torch.int64, device=dev)
                out = torch.empty((3, n_edges), dtype=torch.int64, device=dev) if want_edges else (None,) * 3
                check(lib.psa_neighbor_hop_write(_ptr(col), begin, end, k, slots, n_edges, n_new, _ptr(ws.buf),
                                                 _ptr(hop_ws), _ptr(new), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                                 _stream()))
                if n_edges > 0 and want_edges:
                    rows.append(out[0]), cols.append(out[1]), edges.append(out[2])
                if n_new > 0:
                    nodes.append(new)
            nodes_per_hop.append(n_new)
            edges_per_hop.append(n_edges)
            begin, end, frontier = end, end + n_new, new
        if not checked and S > 0:
            flags = int(state[2].item())
            count["host_reads"] += 1
            raise_on(flags)
        n_id = reset()
        n, E = end, sum(edges_per_hop)
        if not want_edges:
            if stats is not None:
                stats.update(count)
            return n_id, None, None, None, nodes_per_hop, None
        if E == 0:
            if stats is not None:
                stats.update(count)
            return n_id, torch.zeros(n + 1, dtype=torch.int64, device=dev), empty, empty.clone(), nodes_per_hop, edges_per_hop
        row = torch.cat(rows) if len(rows) > 1 else rows[0]
        col_new = torch.cat(cols) if len(cols) > 1 else cols[0]
        e_raw = torch.cat(edges) if len(edges) > 1 else edges[0]
        keys, _ = make_keys(row, col_new, n)
        keys, perm = index_sort(keys, n * n, with_sorted_inputs=True, check=True)  # stable: ties keep slot order
        count["host_reads"] += 1
        if stats is not None:
            stats.update(count)
        row, col_new = split_keys(keys, n)
        # the nodes of the last hop that appended any were never expanded: rows from `begin` on are empty.  They are
        # filled here; as the tail of psa_ind2ptr they would be one run, which a single wave writes
        rowptr_out = torch.empty(n + 1, dtype=torch.int64, device=dev)
        check(lib.psa_ind2ptr(_ptr(row), E, begin, _ptr(rowptr_out), _stream()))
        rowptr_out[begin + 1:] = E
        return n_id, rowptr_out, col_new, _gather_rows_raw(e_raw, perm), nodes_per_hop, edges_per_hop


# ---- ego_k_hop_sample (csrc/ego.hip) ----------------------------------------------------------------

EGO_SEED_OUTSIDE, EGO_COL_OUTSIDE = 1, 2
EGO_MAX_SLOTS = 2**31 - 16


def ego_set_threshold(threshold: int) -> int:
    """Bench/test hook: T, the longest probe side of an induce row that a group of 8 lanes runs (default 32);
    returns the previous value.  Every T produces the same bits."""
    return _lib.load().psa_ego_set_threshold(int(threshold))


def ego_k_hop_sample(rowptr: torch.Tensor, col: torch.Tensor, seeds: torch.Tensor, num_neighbors, replace: bool = False,
                     seed: int = 0, stats: Optional[dict] = None):
    """Per-seed k-hop ego subgraphs of a square sorted CSR matrix: returns (n_id int64[n],
    ptr int64[S+1], root int64[S], rowptr' int64[n+1], col' int64[nnz'], e_id int64[nnz']).  seeds int64[S], inside
    the matrix (IndexError), duplicates allowed: every position is an ego of its own.  num_neighbors: one fan-out
    >= -1 per hop; -1 takes every entry, 0 ends the sampling.  Hop l expands every walk entry of hop l - 1
    (duplicates kept); the parent at walk index i draws from stream i of `seed`.  A hop with k >= 0 has (entries of
    the previous hop) * k slots, known without a read; every hop stays below 2^31 - 16 slots and the walk list as a
    whole below 2^31 entries (ValueError, before anything is allocated where the fan-outs alone decide it), S * N
    below 2^62.  Ego g's nodes are n_id[ptr[g]:ptr[g+1]], ascending; root[g] is the position of its seed; the
    entries are sorted by (row', col') as they are written.
    Host reads (stats["host_reads"]): one per hop with k < 0 that runs, one for the node count (it carries the
    sort's fault word) and one for nnz' (it carries the flags): 2 + #{hops run with k < 0}, whatever S; none for
    S = 0.  stats also receives hops_run and walk_entries.  Not capturable in a graph: the sizes depend on the data."""
    rowptr, col, seeds = _index(rowptr, "rowptr"), _index(col, "col"), _index(seeds, "seeds")
    if rowptr.numel() < 1:
        raise ValueError("rowptr must have at least one element")
    fanouts = [int(k) for k in num_neighbors]
    if any(k < -1 for k in fanouts):
        raise ValueError(f"num_neighbors must be >= -1 (got {fanouts})")
    N, S, dev = rowptr.numel() - 1, seeds.numel(), rowptr.device
    if S >= 2**31:
        raise ValueError(f"ego_k_hop_sample needs fewer than 2^31 seeds (got {S})")
    if S * N >= 2**62:
        raise ValueError(f"ego_k_hop_sample: the keys ego * {N} + node of {S} egos do not fit 62 bits")
    bound = key_bound(S, N, "ego_k_hop_sample")

    def check_slots(hop, slots, total):
        if slots >= EGO_MAX_SLOTS:
            raise ValueError(f"ego_k_hop_sample: hop {hop} has {slots} slots, the limit is 2^31 - 16: "
                             f"to take all entries pass -1, not a large fan-out")
        if total >= 2**31:
            raise ValueError(f"ego_k_hop_sample: the walk list reaches {total} entries at hop {hop}, the limit is 2^31")

    # the numbering of the hops with k >= 0 is host arithmetic: refuse before anything is allocated
    F, total = S, S
    for hop, k in enumerate(fanouts, 1):
        if k <= 0 or F == 0:
            break
        F *= k
        total += F
        check_slots(hop, F, total)
    count = {"host_reads": 0, "hops_run": 0, "walk_entries": S}
    i64 = dict(dtype=torch.int64, device=dev)
    if S == 0:
        if stats is not None:
            stats.update(count)
        return (torch.empty(0, **i64), torch.zeros(1, **i64), torch.empty(0, **i64), torch.zeros(1, **i64),
                torch.empty(0, **i64), torch.empty(0, **i64))
    if N == 0:
        raise IndexError("ego_k_hop_sample: a seed lies outside [0, 0)")
    lib = _lib.load()
    rep, seed = int(bool(replace)), int(seed) & (2**64 - 1)
    with _on(dev):
        flags = torch.empty(1, **i64)
        node, ego, key = torch.empty(S, **i64), torch.empty(S, dtype=torch.int32, device=dev), torch.empty(S, **i64)
        check(lib.psa_ego_init(_ptr(seeds), S, N, _ptr(node), _ptr(ego), _ptr(key), S, _ptr(flags), _stream()))
        keys, begin, F, total = [key], 0, S, S
        for hop, k in enumerate(fanouts, 1):
            if k == 0 or col.numel() == 0:
                break
            pptr = None
            if k < 0:
                counts = torch.empty(F, **i64)
                check(lib.psa_ego_hop_count(_ptr(rowptr), N, _ptr(node), F, _ptr(counts), F, _stream()))
                pptr = count2ptr(counts)
                slots = int(pptr[-1].item())
                count["host_reads"] += 1
                if slots == 0:
                    break
            else:
                slots = F * k
            total += slots
            check_slots(hop, slots, total)
            node2, ego2 = torch.empty(slots, **i64), torch.empty(slots, dtype=torch.int32, device=dev)
            key2 = torch.empty(slots, **i64)
            check(lib.psa_ego_hop_pick(_ptr(rowptr), _ptr(col), N, _ptr(seeds), S, _ptr(node), _ptr(ego), F, _ptr(pptr),
                                       begin, k, rep, seed, slots, _ptr(node2), _ptr(ego2), _ptr(key2), slots,
                                       _ptr(flags), _stream()))
            keys.append(key2)
            begin, F, node, ego = begin + F, slots, node2, ego2
            count["hops_run"] += 1
        count["walk_entries"] = total
        keys = torch.cat(keys) if len(keys) > 1 else keys[0]
        keys, _, scratch = index_sort(keys, bound, with_sorted_inputs=True, keep_scratch=True)
        n, _, ego_of, n_id = unique_sorted(keys, N, want_ptr=False, after=scratch)  # the count carries the fault word
        count["host_reads"] += 1
        ptr = ind2ptr(ego_of, S)
        root, counts = torch.empty(S, **i64), torch.empty(n, **i64)
        check(lib.psa_ego_induce_count(_ptr(rowptr), _ptr(col), N, _ptr(seeds), S, _ptr(n_id), _ptr(ego_of), _ptr(ptr),
                                       n, _ptr(root), S, _ptr(counts), n, _stream()))
        rowptr_out = count2ptr(counts)
        state = torch.empty(2, **i64)
        check(lib.psa_ego_total(_ptr(rowptr_out), n, _ptr(flags), _ptr(state), _stream()))
        nnz_out, raised = state.tolist()  # the one read behind the count pass: nnz' and the flags
        count["host_reads"] += 1
        if stats is not None:
            stats.update(count)
        if raised & EGO_SEED_OUTSIDE:
            raise IndexError(f"ego_k_hop_sample: a seed lies outside [0, {N})")
        if raised & EGO_COL_OUTSIDE:
            raise ValueError(f"ego_k_hop_sample: a stored column lies outside [0, {N})")
        out = torch.empty((2, nnz_out), **i64)
        check(lib.psa_ego_induce_write(_ptr(rowptr), _ptr(col), N, S, _ptr(n_id), _ptr(ego_of), _ptr(ptr), n,
                                       _ptr(rowptr_out), nnz_out, _ptr(out[0]), _ptr(out[1]), nnz_out, _stream()))
    return n_id, ptr, root, rowptr_out, out[0], out[1]


# ---- temporal_neighbor_sample (csrc/temporal.hip) ---------------------------------------------------

TEMPORAL_BAD_INDEX = 4
TEMPORAL_STRATEGY = {"uniform": 0, "last": 1}


def edge_time_order(rowptr: torch.Tensor, time: torch.Tensor, lo: int, hi: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(order int64[nnz], sorted_time int64[nnz]) of EdgeTimeOrder: inside every row the storage positions
    ascending by (time, position), and their times.  time int64[nnz] in storage order with lo <= time <= hi
    (hi - lo < 2^62).  Two stable sorts, by time - lo and then by row, and two gathers; both fault words are
    read (check=True)."""
    rowptr, time = _index(rowptr, "rowptr"), _index(time, "time")
    N, nnz = rowptr.numel() - 1, time.numel()
    if nnz == 0:
        return time.clone(), time.clone()
    _, by_time = index_sort(time - lo, hi - lo + 1, check=True)
    rows = _gather_rows_raw(ptr2ind(rowptr, nnz), by_time)
    _, by_row = index_sort(rows, N, check=True)
    order = _gather_rows_raw(by_time, by_row)
    return order, _gather_rows_raw(time, order)


def temporal_pick_host(sorted_time, start: int, deg: int, bound: int, k: int, replace: bool, strategy: str, seed: int,
                       stream: int) -> List[int]:
    """The ranks that the kernels of temporal_neighbor_sample pick for one parent, run on the host:
    sorted_time is a sequence of integers that holds the row at [start, start + deg), bound the parent's time
    bound, stream its walk index.  Ranks into the eligible prefix, in slot order."""
    import ctypes

    times = [int(x) for x in sorted_time]
    if start < 0 or deg < 0 or start + deg > len(times):
        raise ValueError("the row leaves sorted_time")
    arr = (ctypes.c_int64 * max(len(times), 1))(*times)
    cap = max(deg, int(k), 1)
    out = (ctypes.c_int64 * cap)()
    count = int(_lib.load().psa_temporal_pick_host(ctypes.cast(arr, ctypes.c_void_p), int(start), int(deg), int(bound),
                                                   int(k), int(bool(replace)), TEMPORAL_STRATEGY[strategy],
                                                   int(seed) & (2**64 - 1), int(stream),
                                                   ctypes.cast(out, ctypes.c_void_p), cap))
    if count < 0:
        raise ValueError("psa_temporal_pick_host refused its arguments")
    return list(out[:count])


def temporal_neighbor_sample(rowptr: torch.Tensor, col: torch.Tensor, order: torch.Tensor, sorted_time: torch.Tensor,
                             seeds: torch.Tensor, seed_time: torch.Tensor, num_neighbors, strategy: str = "uniform",
                             replace: bool = False, seed: int = 0, stats: Optional[dict] = None):
    """Time-bounded per-seed sampling on a square sorted CSR matrix with an EdgeTimeOrder: returns
    (n_id int64[n], ptr int64[S+1], root int64[S], rowptr' int64[n+1], col' int64[nnz'], e_id int64[nnz']).  Walk
    list, streams, slot numbering, n_id / ptr / root and the limits are ego_k_hop_sample's, and S * nnz < 2^62 in
    addition; a parent of ego g picks among the entries of its row with time <= seed_time[g].  The matrix holds
    the SAMPLED entries, one per distinct (ego, entry), in (ego, entry) order, which is (row', col') order.
    Host reads (stats["host_reads"]): one per hop with k < 0 that runs, one for n (with the node sort's fault
    word), one for nnz' (with the edge sort's fault word and the flags; the flags alone when no hop ran); none
    for S = 0.  Not capturable in a graph: the sizes depend on the data."""
    rowptr, col, seeds = _index(rowptr, "rowptr"), _index(col, "col"), _index(seeds, "seeds")
    order, sorted_time = _index(order, "order"), _index(sorted_time, "sorted_time")
    seed_time = _index(seed_time, "seed_time")
    if rowptr.numel() < 1:
        raise ValueError("rowptr must have at least one element")
    if strategy not in TEMPORAL_STRATEGY:
        raise ValueError(f"strategy must be 'uniform' or 'last' (got {strategy!r})")
    if strategy == "last" and replace:
        raise ValueError("strategy='last' takes the most recent entries: it has no draws to replace")
    fanouts = [int(k) for k in num_neighbors]
    if any(k < -1 for k in fanouts):
        raise ValueError(f"num_neighbors must be >= -1 (got {fanouts})")
    N, S, nnz, dev = rowptr.numel() - 1, seeds.numel(), col.numel(), rowptr.device
    if seed_time.numel() != S:
        raise ValueError(f"seed_time must hold one bound per seed ({S}), got {seed_time.numel()}")
    if order.numel() != nnz or sorted_time.numel() != nnz:
        raise ValueError(f"order and sorted_time must hold one element per entry ({nnz})")
    who = "temporal_neighbor_sample"
    if S >= 2**31:
        raise ValueError(f"{who} needs fewer than 2^31 seeds (got {S})")
    if S * N >= 2**62:
        raise ValueError(f"{who}: the keys ego * {N} + node of {S} egos do not fit 62 bits")
    if S * nnz >= 2**62:
        raise ValueError(f"{who}: the keys ego * {nnz} + entry of {S} egos do not fit 62 bits")
    bound = key_bound(S, N, who)

    def check_slots(hop, slots, total):
        if slots >= EGO_MAX_SLOTS:
            raise ValueError(f"{who}: hop {hop} has {slots} slots, the limit is 2^31 - 16: "
                             f"to take all eligible entries pass -1, not a large fan-out")
        if total >= 2**31:
            raise ValueError(f"{who}: the walk list reaches {total} entries at hop {hop}, the limit is 2^31")

    F, total = S, S
    for hop, k in enumerate(fanouts, 1):
        if k <= 0 or F == 0:
            break
        F *= k
        total += F
        check_slots(hop, F, total)
    count = {"host_reads": 0, "hops_run": 0, "walk_entries": S}
    i64 = dict(dtype=torch.int64, device=dev)
    if S == 0:
        if stats is not None:
            stats.update(count)
        return (torch.empty(0, **i64), torch.zeros(1, **i64), torch.empty(0, **i64), torch.zeros(1, **i64),
                torch.empty(0, **i64), torch.empty(0, **i64))
    if N == 0:
        raise IndexError(f"{who}: a seed lies outside [0, 0)")
    lib = _lib.load()
    rep, strat, seed = int(bool(replace)), TEMPORAL_STRATEGY[strategy], int(seed) & (2**64 - 1)

    def raise_on(raised):
        if raised & EGO_SEED_OUTSIDE:
            raise IndexError(f"{who}: a seed lies outside [0, {N})")
        if raised & EGO_COL_OUTSIDE:
            raise ValueError(f"{who}: a stored column lies outside [0, {N})")
        if raised & TEMPORAL_BAD_INDEX:
            raise ValueError(f"{who}: rowptr or the time order do not describe the matrix")

    with _on(dev):
        flags = torch.empty(1, **i64)
        node, ego, key = torch.empty(S, **i64), torch.empty(S, dtype=torch.int32, device=dev), torch.empty(S, **i64)
        check(lib.psa_ego_init(_ptr(seeds), S, N, _ptr(node), _ptr(ego), _ptr(key), S, _ptr(flags), _stream()))
        keys, ekeys, begin, F, total = [key], [], 0, S, S
        for hop, k in enumerate(fanouts, 1):
            if k == 0 or nnz == 0:
                break
            pptr = None
            if k < 0:
                counts = torch.empty(F, **i64)
                check(lib.psa_temporal_hop_count(_ptr(rowptr), _ptr(sorted_time), N, nnz, _ptr(seed_time), S,
                                                 _ptr(node), _ptr(ego), F, _ptr(counts), F, _ptr(flags), _stream()))
                pptr = count2ptr(counts)
                slots = int(pptr[-1].item())
                count["host_reads"] += 1
                if slots == 0:
                    break
            else:
                slots = F * k
            total += slots
            check_slots(hop, slots, total)
            node2, ego2 = torch.empty(slots, **i64), torch.empty(slots, dtype=torch.int32, device=dev)
            key2, ekey2 = torch.empty(slots, **i64), torch.empty(slots, **i64)
            check(lib.psa_temporal_hop_pick(_ptr(rowptr), _ptr(col), _ptr(order), _ptr(sorted_time), N, nnz,
                                            _ptr(seeds), _ptr(seed_time), S, _ptr(node), _ptr(ego), F, _ptr(pptr),
                                            begin, k, rep, strat, seed, slots, _ptr(node2), _ptr(ego2), _ptr(key2),
                                            _ptr(ekey2), slots, _ptr(flags), _stream()))
            keys.append(key2)
            ekeys.append(ekey2)
            begin, F, node, ego = begin + F, slots, node2, ego2
            count["hops_run"] += 1
        count["walk_entries"] = total
        keys = torch.cat(keys) if len(keys) > 1 else keys[0]
        keys, _, scratch = index_sort(keys, bound, with_sorted_inputs=True, keep_scratch=True)
        n, _, ego_of, n_id = unique_sorted(keys, N, want_ptr=False, after=scratch)  # the count carries the fault word
        count["host_reads"] += 1
        ptr = ind2ptr(ego_of, S)
        root = torch.empty(S, **i64)
        if ekeys:
            # one sentinel of its own, so that the largest distinct key is the sentinel whatever the slots hold
            ekeys.append(torch.full((1,), S * nnz, **i64))
            ekeys = torch.cat(ekeys)
            E = ekeys.numel()
            ekeys, _, scratch = index_sort(ekeys, S * nnz + 1, with_sorted_inputs=True, keep_scratch=True)
            ws = _workspace(lib.psa_unique_workspace_bytes(E), dev)
            count_d, state = torch.empty(2, **i64), torch.empty(3, **i64)
            check(lib.psa_unique_count_after_sort(_ptr(ekeys), E, _ptr(ws), ws.numel(), _ptr(scratch.ws),
                                                  scratch.max_value, _ptr(count_d), _stream()))
            check(lib.psa_temporal_total(_ptr(count_d), _ptr(flags), _ptr(state), _stream()))
            distinct, fault, raised = state.tolist()  # the one read: nnz' + 1, the sort's fault word, the flags
        else:
            distinct, fault, raised = 1, 0, int(flags.item())
        count["host_reads"] += 1
        if stats is not None:
            stats.update(count)
        if fault:
            raise HipCoreError("index_sort: an inter-workgroup wait of a radix pass gave up; the order is invalid")
        raise_on(raised)
        m = distinct - 1
        out = torch.empty((3, m), **i64)
        key_ego = key_edge = None
        if m > 0:
            _, _, key_ego, key_edge = unique_sorted(ekeys, nnz, want_ptr=False, _counted=(distinct, ws, count_d))
        check(lib.psa_temporal_finish(_ptr(rowptr), _ptr(col), N, nnz, _ptr(seeds), S, _ptr(key_ego), _ptr(key_edge), m,
                                      _ptr(n_id), _ptr(ptr), n, _ptr(root), S, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                      m, _ptr(flags), _stream()))
        rowptr_out = ind2ptr(out[0], n) if m > 0 else torch.zeros(n + 1, **i64)
    return n_id, ptr, root, rowptr_out, out[1], out[2]


# ---- reverse_cuthill_mckee (csrc/rcm.hip) ---------------------------------------------------------

RCM_DONE, RCM_HANDOVER, RCM_BAD_INPUT = 0, 1, 2


def rcm_set_variant(variant: int) -> int:
    """Test/bench hook: 0 = default, 1 = every level through the large path, 2 = the small path
    with a capacity of 8 candidate edges; returns the previous one.  All give the same bits."""
    return _lib.load().psa_rcm_set_variant(int(variant))


def rcm_small_capacity() -> int:
    """Candidate edges of a level that the one-workgroup path takes under the current variant."""
    return int(_lib.load().psa_rcm_small_capacity())


def rcm_tile() -> int:
    """Candidates per workgroup of the large path."""
    return int(_lib.load().psa_rcm_tile())


def reverse_cuthill_mckee(rowptr: torch.Tensor, col: torch.Tensor, stats: Optional[dict] = None) -> torch.Tensor:
    """perm int64[N]: the reverse Cuthill-McKee ordering of the square sorted CSR pattern
    (rowptr int64[N+1], col int64[nnz]) — scipy's algorithm with its ties fixed: seeds and
    neighbours in (degree, id) order, degree = stored entries of the row.  Built
    on the device: levels of up to rcm_small_capacity() candidate edges run inside one
    workgroup, level after level, with one host read per launch; a larger level is a fixed
    launch sequence with one host read.  Which path served a level does not change the
    result.  stats (a dict, optional) receives the level and host-read counts.
    Not capturable in a graph: the launch sequence depends on the data.  N < 2^31."""
    rowptr, col = _index(rowptr, "rowptr"), _index(col, "col")
    if rowptr.numel() < 1:
        raise ValueError("rowptr must have at least one element")
    N, nnz, dev = rowptr.numel() - 1, col.numel(), rowptr.device
    if N >= 2**31:
        raise ValueError(f"reverse_cuthill_mckee needs N < 2^31 (got {N})")
    count = {"host_reads": 0, "small_launches": 0, "small_levels": 0, "large_levels": 0}
    if stats is not None:
        stats.update(count)
    if N == 0 or nnz == 0:  # every node is its own component, in id order
        return torch.arange(N - 1, -1, -1, dtype=torch.int64, device=dev)
    lib = _lib.load()
    n_empty, _, _, max_deg = csr_row_stats(rowptr)
    count["host_reads"] += 1
    ws = _workspace(lib.psa_rcm_workspace_bytes(N, nnz), dev)
    state = torch.empty(16, dtype=torch.int64, device=dev)
    perm = torch.empty(N, dtype=torch.int64, device=dev)
    cap = lib.psa_rcm_small_capacity()
    a = (_ptr(rowptr), _ptr(col), N, nnz)
    w = (_ptr(ws), ws.numel(), _ptr(state))
    with _on(dev):
        check(lib.psa_rcm_init(_ptr(rowptr), N, nnz, n_empty, max_deg, *w, _stream()))
        for _ in range(N + 1):  # every small launch ends the order or hands over a level that places a node
            check(lib.psa_rcm_small(*a, max_deg, *w, _stream()))
            placed, lo, hi, _, status, cand, _, _, fault, small_levels = state.tolist()[:10]
            count["host_reads"] += 1
            count["small_launches"] += 1
            count["small_levels"] = small_levels
            if fault or status != RCM_HANDOVER:
                break
            while True:
                check(lib.psa_rcm_level_count(*a, lo, hi, cand, *w, _stream()))
                n_new, next_cand = state[6:8].tolist()
                count["host_reads"] += 1
                count["large_levels"] += 1
                check(lib.psa_rcm_level_write(*a, lo, hi, cand, n_new, max_deg, *w, _stream()))
                lo, hi, cand = hi, hi + n_new, next_cand
                if n_new == 0 or cand <= cap:
                    break
        if stats is not None:
            stats.update(count)
        if fault:
            raise HipCoreError("reverse_cuthill_mckee: an inter-workgroup wait of a radix pass gave up; "
                               "the order is invalid")
        if status != RCM_DONE or placed != N:
            raise ValueError("reverse_cuthill_mckee: the level search placed "
                             f"{placed} of {N} nodes (status {status}); are the rows of the matrix sorted?")
        check(lib.psa_rcm_finish(N, nnz, _ptr(ws), ws.numel(), _ptr(perm), _stream()))
    return perm


# ---- the attention path: segmented softmax (csrc/softmax.hip) and sddmm ----------------------------

def _softmax_operands(a: torch.Tensor, name: str, indptr: torch.Tensor, perm: Optional[torch.Tensor]):
    _gpu(a, name)
    indptr = _index(indptr, "indptr")
    if a.dtype != torch.float32:
        raise TypeError(f"segment_softmax: {name} must be float32 (got {a.dtype})")
    if a.dim() < 1:
        raise ValueError(f"{name} must have at least one dim")
    if indptr.numel() < 1:
        raise ValueError("indptr must have at least one element")
    a = a.contiguous()
    if perm is not None:
        perm = _index(perm, "perm")
        if perm.numel() != a.shape[0]:
            raise ValueError("perm must have one entry per row of the values")
    D = 1
    for s in a.shape[1:]:
        D *= s
    return a, indptr, perm, indptr.numel() - 1, D


def _segment_softmax_raw(src: torch.Tensor, indptr: torch.Tensor, perm: Optional[torch.Tensor] = None) -> torch.Tensor:
    src, indptr, perm, nseg, D = _softmax_operands(src, "src", indptr, perm)
    n = src.shape[0]
    out = torch.empty_like(src)
    lib = _lib.load()
    ws_bytes = lib.psa_segment_softmax_workspace_bytes(n, D)
    ws = _workspace(ws_bytes, src.device) if ws_bytes else None
    with _on(src.device):
        check(lib.psa_segment_softmax(_ptr(src), _ptr(perm), _ptr(indptr), nseg, D, n, _ptr(out), _ptr(ws), ws_bytes,
                                      _stream()))
    return out


def segment_softmax_bw(y: torch.Tensor, grad: torch.Tensor, indptr: torch.Tensor,
                       perm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Backward of segment_softmax from its saved output: y * (grad - sum over the segment of y * grad),
    per column.  Same layout and `perm` rule as the forward; fp32 only."""
    y, indptr, perm, nseg, D = _softmax_operands(y, "y", indptr, perm)
    _gpu(grad, "grad")
    if grad.dtype != torch.float32:
        raise TypeError(f"segment_softmax_bw: grad must be float32 (got {grad.dtype})")
    if grad.shape != y.shape:
        raise ValueError("grad must have y's shape")
    grad = grad.contiguous()
    n = y.shape[0]
    out = torch.empty_like(y)
    lib = _lib.load()
    ws_bytes = lib.psa_segment_softmax_workspace_bytes(n, D)
    ws = _workspace(ws_bytes, y.device) if ws_bytes else None
    with _on(y.device):
        check(lib.psa_segment_softmax_bw(_ptr(y), _ptr(grad), _ptr(perm), _ptr(indptr), nseg, D, n, _ptr(out), _ptr(ws),
                                         ws_bytes, _stream()))
    return out


class _SegmentSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, indptr, perm):
        y = _segment_softmax_raw(src, indptr, perm)
        ctx.save_for_backward(y, indptr, perm)
        return y

    @staticmethod
    def backward(ctx, grad):
        y, indptr, perm = ctx.saved_tensors
        return segment_softmax_bw(y, grad, indptr, perm), None, None


def segment_softmax(src: torch.Tensor, indptr: torch.Tensor, perm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Softmax of src (fp32 [n] or [n, H]; further value dims count as columns) over every segment of
    indptr (int64[nseg + 1]), one softmax per column.  With `perm` the entry at position j of the segment
    order is src[perm[j]] and its result lands at out[perm[j]]: the result keeps src's order.  Entries that
    no segment covers are left unwritten.  Differentiable in src (the backward reads the saved output)."""
    if needs_grad(src):
        return _SegmentSoftmax.apply(src, indptr, perm)
    return _segment_softmax_raw(src, indptr, perm)


def _sddmm_raw(rowptr: torch.Tensor, col: torch.Tensor, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    rowptr, col = _index(rowptr, "rowptr"), _index(col, "col")
    x, y = _f32(x, "x"), _f32(y, "y")
    if rowptr.numel() < 1:
        raise ValueError("rowptr must have at least one element")
    M, nnz = rowptr.numel() - 1, col.numel()
    if x.dim() != 2 or y.dim() != 2 or x.shape[0] != M or x.shape[1] != y.shape[1]:
        raise ValueError(f"sddmm: x must be [{M}, K] and y [N, K] (got {tuple(x.shape)}, {tuple(y.shape)})")
    K = x.shape[1]
    if K % 4 == 0:  # the 16-byte gathers of psa_spmm_value_bw; other K (and views) take its 4-byte form
        x, y = _aligned16(x), _aligned16(y)
    out = torch.empty(nnz, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    ws_bytes = lib.psa_spmm_value_bw_workspace_bytes(nnz)
    ws = _workspace(ws_bytes, x.device) if ws_bytes else None
    with _on(x.device):
        check(lib.psa_spmm_value_bw(_lib.SUM, _ptr(rowptr), _ptr(col), _ptr(y), _ptr(x), M, K, nnz, _ptr(out), _ptr(ws),
                                    ws_bytes, _stream()))
    return out


class _Sddmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, rowptr, col, csc):
        ctx.save_for_backward(x, y, rowptr, col)
        ctx.csc = csc
        if _is_heads(x, y):
            return _sddmm_heads_raw(rowptr, col, x, y)
        return _sddmm_raw(rowptr, col, x, y)

    @staticmethod
    def backward(ctx, grad):
        x, y, rowptr, col = ctx.saved_tensors
        grad = grad.contiguous()
        grad_x = grad_y = None
        if x.dim() == 3:  # per head: both gradients are psa_spmm_heads with the [nnz, H] gradient as the values
            if ctx.needs_input_grad[0]:
                grad_x = _spmm_heads_raw(rowptr, col, grad, y)
            if ctx.needs_input_grad[1]:
                grad_y = _spmm_heads_transposed(_csc_view(ctx.csc, rowptr, col, y.shape[0]), grad, x)
            return grad_x, grad_y, None, None, None
        if ctx.needs_input_grad[0]:  # grad_x[r] = sum over the row's entries of g[e] * y[col[e]]
            grad_x = _spmm("sum", rowptr, col, grad, y, want_arg=False)[0]
        if ctx.needs_input_grad[1]:  # grad_y[c] = sum over the column's entries of g[e] * x[row(e)]: SpMM over the CSC view
            colptr, row_csc, csr2csc = _csc_view(ctx.csc, rowptr, col, y.shape[0])
            grad_y = _spmm("sum", colptr, row_csc, _gather_rows_raw(grad, csr2csc), x, want_arg=False)[0]
        return grad_x, grad_y, None, None, None


def _is_heads(x, y) -> bool:
    """Both operands 3-D: the per-head form.  Everything else goes to the 2-D call and its errors."""
    return isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.dim() == 3 and y.dim() == 3


def sddmm(rowptr: torch.Tensor, col: torch.Tensor, x: torch.Tensor, y: torch.Tensor, csc=None) -> torch.Tensor:
    """f32[nnz]: out[e] = <x[row(e)], y[col[e]]> for every entry of the CSR pattern (rowptr, col), with x fp32
    [M, K] and y fp32 [N, K] — psa_spmm_value_bw with mat = y, grad = x.  Differentiable in x and y:
    grad_x = spmm_sum(rowptr, col, g, y), grad_y = the SpMM over the CSC view with g[csr2csc].  `csc`:
    (colptr, row[csr2csc], csr2csc), or a callable returning it, when the caller has that view (a
    SparseStorage does); without it the backward sorts `col` once.
    Per head: x fp32 [M, H, K] and y fp32 [N, H, K] give f32[nnz, H], out[e, h] = <x[row(e), h], y[col[e], h]>
    (psa_sddmm_heads), with both gradients from psa_spmm_heads."""
    if needs_grad(x) or needs_grad(y):
        return _Sddmm.apply(x, y, rowptr, col, csc)
    if _is_heads(x, y):
        return _sddmm_heads_raw(rowptr, col, x, y)
    return _sddmm_raw(rowptr, col, x, y)


# ---- multi-head ends of the attention path (csrc/spmm_heads.hip) ----------------------------------

def _heads_pattern(rowptr: torch.Tensor, col: torch.Tensor):
    rowptr, col = _index(rowptr, "rowptr"), _index(col, "col")
    if rowptr.numel() < 1:
        raise ValueError("rowptr must have at least one element")
    return rowptr, col, rowptr.numel() - 1, col.numel()


def _spmm_heads_raw(rowptr: torch.Tensor, col: torch.Tensor, value: torch.Tensor, mat: torch.Tensor) -> torch.Tensor:
    rowptr, col, M, nnz = _heads_pattern(rowptr, col)
    value, mat = _f32(value, "value"), _f32(mat, "mat")
    if mat.dim() != 3:
        raise ValueError(f"spmm over per-head values: the dense operand must be [N, H, F] (got {tuple(mat.shape)})")
    N, H, F = mat.shape
    if value.dim() != 2 or value.shape[0] != nnz or value.shape[1] != H:
        raise ValueError(f"spmm over per-head values: value must be [{nnz}, {H}] (got {tuple(value.shape)})")
    if F % 4 == 0:  # the 16-byte gathers; other F (and views) take the 4-byte form
        mat = _aligned16(mat)
    out = torch.empty((M, H, F), dtype=torch.float32, device=mat.device)
    lib = _lib.load()
    ws_bytes = lib.psa_spmm_heads_workspace_bytes(nnz, H, F)
    ws = _workspace(ws_bytes, mat.device) if ws_bytes else None
    with _on(mat.device):
        check(lib.psa_spmm_heads(_ptr(rowptr), _ptr(col), _ptr(value), _ptr(mat), M, N, H, F, nnz, _ptr(out), _ptr(ws),
                                 ws_bytes, _stream()))
    return out


def spmm_heads_half_raw(rowptr: torch.Tensor, col: torch.Tensor, value: torch.Tensor, mat: torch.Tensor,
                        alpha: float = 1.0) -> torch.Tensor:
    """bf16[M, H, F] = round(alpha * sum over the entries of row r of value[e, h] * mat[col[e], h, :]) with value
    fp32 [nnz, H] and mat bf16 [N, H, F]: fp32 products and sums, one rounding (psa_spmm_heads_half).  A raw call
    without autograd: the backward of the bf16 attention takes its three gradients from it."""
    rowptr, col, M, nnz = _heads_pattern(rowptr, col)
    value = _f32(value, "value")
    _gpu(mat, "mat")
    if mat.dtype != torch.bfloat16:
        raise TypeError(f"mat must be bfloat16 (got {mat.dtype})")
    if mat.dim() != 3:
        raise ValueError(f"spmm over per-head values: the dense operand must be [N, H, F] (got {tuple(mat.shape)})")
    mat = mat.contiguous()
    N, H, F = mat.shape
    if value.dim() != 2 or value.shape[0] != nnz or value.shape[1] != H:
        raise ValueError(f"spmm over per-head values: value must be [{nnz}, {H}] (got {tuple(value.shape)})")
    if F % 8 == 0:  # the 16-byte gathers; other F (and views) take the 2-byte form
        mat = _aligned16(mat)
    out = torch.empty((M, H, F), dtype=mat.dtype, device=mat.device)
    lib = _lib.load()
    ws_bytes = lib.psa_spmm_heads_workspace_bytes(nnz, H, F)  # the partials are fp32
    ws = _workspace(ws_bytes, mat.device) if ws_bytes else None
    with _on(mat.device):
        check(lib.psa_spmm_heads_half(_DTYPE_ID[mat.dtype], _ptr(rowptr), _ptr(col), _ptr(value), _ptr(mat),
                                      float(alpha), M, N, H, F, nnz, _ptr(out), _ptr(ws), ws_bytes, _stream()))
    return out


def _sddmm_heads_raw(rowptr: torch.Tensor, col: torch.Tensor, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    rowptr, col, M, nnz = _heads_pattern(rowptr, col)
    x, y = _f32(x, "x"), _f32(y, "y")
    if x.dim() != 3 or y.dim() != 3 or x.shape[0] != M or x.shape[1:] != y.shape[1:]:
        raise ValueError(f"sddmm: x must be [{M}, H, K] and y [N, H, K] (got {tuple(x.shape)}, {tuple(y.shape)})")
    H, K = x.shape[1], x.shape[2]
    if K % 4 == 0:
        x, y = _aligned16(x), _aligned16(y)
    out = torch.empty((nnz, H), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    ws_bytes = lib.psa_sddmm_heads_workspace_bytes(nnz)
    ws = _workspace(ws_bytes, x.device) if ws_bytes else None
    with _on(x.device):
        check(lib.psa_sddmm_heads(_ptr(rowptr), _ptr(col), _ptr(x), _ptr(y), M, H, K, nnz, _ptr(out), _ptr(ws), ws_bytes,
                                  _stream()))
    return out


def _csc_view(csc, rowptr: torch.Tensor, col: torch.Tensor, N: int):
    """(colptr, row[csr2csc], csr2csc): the caller's (a tuple or a callable returning one), else built by one sort of col."""
    csc = csc() if callable(csc) else csc
    if csc is None:
        col_csc, csr2csc = index_sort(col, N, with_sorted_inputs=True, check=True)
        csc = (ind2ptr(col_csc, N), _gather_rows_raw(ptr2ind(rowptr, col.numel()), csr2csc), csr2csc)
    return csc


def _spmm_heads_transposed(csc, weight: torch.Tensor, dense: torch.Tensor) -> torch.Tensor:
    """out[c, h, :] = sum over the column's entries of weight[e, h] * dense[row(e), h, :]: psa_spmm_heads over
    the CSC view, the [nnz, H] weights brought to CSC order by a row gather."""
    colptr, row_csc, csr2csc = csc
    return _spmm_heads_raw(colptr, row_csc, _gather_rows_raw(weight, csr2csc), dense)


class _SpmmHeads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, value, mat, rowptr, col, csc):
        ctx.save_for_backward(value, mat, rowptr, col)
        ctx.csc = csc
        return _spmm_heads_raw(rowptr, col, value, mat)

    @staticmethod
    def backward(ctx, grad):
        value, mat, rowptr, col = ctx.saved_tensors
        grad = grad.contiguous()
        grad_value = grad_mat = None
        if ctx.needs_input_grad[0]:  # grad_value[e, h] = <grad[row(e), h, :], mat[col[e], h, :]>
            grad_value = _sddmm_heads_raw(rowptr, col, grad, mat)
        if ctx.needs_input_grad[1]:  # grad_mat[c] = sum over the column's entries of value[e] * grad[row(e)]
            grad_mat = _spmm_heads_transposed(_csc_view(ctx.csc, rowptr, col, mat.shape[0]), value, grad)
        return grad_value, grad_mat, None, None, None


def spmm_heads(rowptr: torch.Tensor, col: torch.Tensor, value: torch.Tensor, mat: torch.Tensor, csc=None) -> torch.Tensor:
    """f32[M, H, F]: out[r, h, :] = sum over the entries of row r of value[e, h] * mat[col[e], h, :], with value
    fp32 [nnz, H] and mat fp32 [N, H, F] — the aggregation of a multi-head attention layer in one launch.
    Differentiable in value (psa_sddmm_heads of the upstream gradient and mat) and in mat (the same
    product over the CSC view).  `csc` as for sddmm."""
    if needs_grad(value) or needs_grad(mat):
        return _SpmmHeads.apply(value, mat, rowptr, col, csc)
    return _spmm_heads_raw(rowptr, col, value, mat)


# ---- fused attention: sddmm + row softmax + SpMM in one pass (csrc/attention.hip) -------------------

def _attention_operands(rowptr, col, q, k, v, bias):
    """The checked, contiguous operands in heads form, plus (M, N, H, K, F, nnz) and whether the caller gave the
    2-D form."""
    rowptr, col, M, nnz = _heads_pattern(rowptr, col)
    q, k, v = _attention_dense(q, "q"), _attention_dense(k, "k"), _attention_dense(v, "v")
    if not (q.dtype == k.dtype == v.dtype):
        raise TypeError(f"attention: q, k, v must share one dtype (got {q.dtype}, {k.dtype}, {v.dtype})")
    dims = {q.dim(), k.dim(), v.dim()}
    if dims not in ({2}, {3}):
        raise ValueError(f"attention: q, k, v must all be 2-D, or all 3-D [rows, H, width] "
                         f"(got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)})")
    flat = q.dim() == 2
    if flat:
        q, k, v = q.unsqueeze(1), k.unsqueeze(1), v.unsqueeze(1)
    H, K = q.shape[1], q.shape[2]
    N, F = k.shape[0], v.shape[2]
    if q.shape[0] != M or k.shape[1:] != q.shape[1:] or v.shape[0] != N or v.shape[1] != H:
        raise ValueError(f"attention: q must be [{M}, H, K], k [N, H, K] and v [N, H, F] "
                         f"(got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)})")
    if H < 1 or K < 1 or F < 1:
        raise ValueError("attention: H, K and F must be at least 1")
    if bias is not None:
        bias = _f32(bias, "bias")
        if bias.shape not in ((nnz,), (nnz, H)):
            raise ValueError(f"attention: bias must be [{nnz}] or [{nnz}, {H}] (got {tuple(bias.shape)})")
    if K % _vec16(q) == 0 and F % _vec16(q) == 0:  # the 16-byte form; other widths (and views) take the element form
        q, k, v = _aligned16(q), _aligned16(k), _aligned16(v)
    return rowptr, col, q, k, v, bias, (M, N, H, K, F, nnz), flat


def _attention_dense(x: torch.Tensor, name: str) -> torch.Tensor:
    _gpu(x, name)
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{name} must be float32 or bfloat16 (got {x.dtype})")
    return x.contiguous()


def _vec16(x: torch.Tensor) -> int:
    """Elements of x's dtype in one 16-byte load: 4 fp32, 8 bf16."""
    return 16 // x.element_size()


def _bias_heads(bias: Optional[torch.Tensor]) -> int:
    return 1 if bias is None or bias.dim() == 1 else bias.shape[1]


def _dropout_args(dropout_p, seed, who: str = "attention", draw: bool = True):
    """(dropout_p, seed) checked: a float in [0, 1) and an int in [0, 2^64).  seed=None with dropout_p > 0 draws one
    from torch's CPU default generator where `draw` allows it (torch.manual_seed reproduces it; no device read, no
    sync).  With dropout_p == 0 the seed is not looked at and comes back as 0."""
    if isinstance(dropout_p, bool) or not isinstance(dropout_p, (int, float)):
        raise ValueError(f"{who}: dropout_p must be a float in [0, 1) (got {dropout_p!r})")
    dropout_p = float(dropout_p)
    if not 0.0 <= dropout_p < 1.0:  # a NaN fails both comparisons
        raise ValueError(f"{who}: dropout_p must be in [0, 1) (got {dropout_p})")
    if dropout_p == 0.0:
        return 0.0, 0
    if seed is None and draw:
        lo, hi = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
        return dropout_p, (hi << 32) | lo
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise TypeError(f"{who}: seed must be an int in [0, 2^64) (got {type(seed).__name__})")
    if not 0 <= seed < (1 << 64):
        raise ValueError(f"{who}: seed must be in [0, 2^64) (got {seed})")
    return dropout_p, seed


def attention_dropout_mask(nnz: int, H: int, dropout_p: float, seed: int, device="cuda") -> torch.Tensor:
    """bool [nnz, H] on the device: keep(e, h) of the fused op's dropout for this (dropout_p, seed), e the position
    of the entry in CSR order and h the head (psa_attention_dropout_mask).  The unfused chain with the same mask is
    spmm_heads(softmax(sddmm) * mask * float32(1 / (1 - dropout_p)), v)."""
    if isinstance(nnz, bool) or isinstance(H, bool) or not isinstance(nnz, int) or not isinstance(H, int):
        raise TypeError("attention_dropout_mask: nnz and H must be ints")
    if nnz < 0 or H < 1:
        raise ValueError("attention_dropout_mask: nnz must be at least 0 and H at least 1")
    p, seed = _dropout_args(dropout_p, seed, "attention_dropout_mask", draw=False)
    mask = torch.empty((nnz, H), dtype=torch.uint8, device=device)
    with _on(mask.device):
        check(_lib.load().psa_attention_dropout_mask(nnz, H, p, seed, _ptr(mask), _stream()))
    return mask.view(torch.bool)


def _attention_fw_raw(rowptr, col, q, k, v, bias, scale: float, dropout_p: float = 0.0, seed: int = 0):
    """(out [M, H, F], stat [M, H, 2] = {row maximum, sum of exp(s - maximum)}) from checked heads-form operands;
    dropout_p == 0.0 takes the plain entry points, anything else the dropout forms (with a checked seed)."""
    M, H, K = q.shape
    N, F, nnz = k.shape[0], v.shape[2], col.numel()
    out = torch.empty((M, H, F), dtype=q.dtype, device=q.device)
    stat = torch.empty((M, H, 2), dtype=torch.float32, device=q.device)
    lib = _lib.load()
    ws_bytes = lib.psa_attention_workspace_bytes(nnz, H, F)  # the partials are fp32 for either dtype
    ws = _workspace(ws_bytes, q.device) if ws_bytes else None
    with _on(q.device):
        if dropout_p != 0.0 and q.dtype == torch.float32:
            check(lib.psa_attention_dropout_fw(_ptr(rowptr), _ptr(col), _ptr(q), _ptr(k), _ptr(v), _ptr(bias),
                                               _bias_heads(bias), scale, dropout_p, seed, M, N, H, K, F, nnz, _ptr(out),
                                               _ptr(stat), _ptr(ws), ws_bytes, _stream()))
        elif dropout_p != 0.0:
            check(lib.psa_attention_half_dropout_fw(_DTYPE_ID[q.dtype], _ptr(rowptr), _ptr(col), _ptr(q), _ptr(k),
                                                    _ptr(v), _ptr(bias), _bias_heads(bias), scale, dropout_p, seed, M, N,
                                                    H, K, F, nnz, _ptr(out), _ptr(stat), _ptr(ws), ws_bytes, _stream()))
        elif q.dtype == torch.float32:
            check(lib.psa_attention_fw(_ptr(rowptr), _ptr(col), _ptr(q), _ptr(k), _ptr(v), _ptr(bias),
                                       _bias_heads(bias), scale, M, N, H, K, F, nnz, _ptr(out), _ptr(stat), _ptr(ws),
                                       ws_bytes, _stream()))
        else:
            check(lib.psa_attention_half_fw(_DTYPE_ID[q.dtype], _ptr(rowptr), _ptr(col), _ptr(q), _ptr(k), _ptr(v),
                                            _ptr(bias), _bias_heads(bias), scale, M, N, H, K, F, nnz, _ptr(out),
                                            _ptr(stat), _ptr(ws), ws_bytes, _stream()))
    return out, stat


def _attention_bw_entries_raw(rowptr, col, q, k, v, bias, scale: float, grad_out, out, stat, dropout_p: float = 0.0,
                              seed: int = 0):
    """(p [nnz, H], dS = p * (dP - delta) [nnz, H]): the per-entry half of the backward, from the saved {m, l}.
    With dropout (D = keep * inv_keep, recomputed from the seed): (p * D, p * (D * dP - delta))."""
    M, H, K = q.shape
    N, F, nnz = k.shape[0], v.shape[2], col.numel()
    if grad_out.dtype != q.dtype:
        raise TypeError(f"attention: grad_out must be {q.dtype} as q, k, v (got {grad_out.dtype})")
    if K % _vec16(q) == 0 and F % _vec16(q) == 0:
        grad_out = _aligned16(grad_out)
    p = torch.empty((nnz, H), dtype=torch.float32, device=q.device)
    ds = torch.empty((nnz, H), dtype=torch.float32, device=q.device)
    lib = _lib.load()
    ws_bytes = lib.psa_attention_workspace_bytes(nnz, H, F)
    ws = _workspace(ws_bytes, q.device) if ws_bytes else None
    with _on(q.device):
        if dropout_p != 0.0 and q.dtype == torch.float32:
            check(lib.psa_attention_dropout_bw_entries(_ptr(rowptr), _ptr(col), _ptr(q), _ptr(k), _ptr(v), _ptr(bias),
                                                       _bias_heads(bias), scale, dropout_p, seed, _ptr(grad_out),
                                                       _ptr(out), _ptr(stat), M, N, H, K, F, nnz, _ptr(p), _ptr(ds),
                                                       _ptr(ws), ws_bytes, _stream()))
        elif dropout_p != 0.0:
            check(lib.psa_attention_half_dropout_bw_entries(_DTYPE_ID[q.dtype], _ptr(rowptr), _ptr(col), _ptr(q),
                                                            _ptr(k), _ptr(v), _ptr(bias), _bias_heads(bias), scale,
                                                            dropout_p, seed, _ptr(grad_out), _ptr(out), _ptr(stat), M, N,
                                                            H, K, F, nnz, _ptr(p), _ptr(ds), _ptr(ws), ws_bytes,
                                                            _stream()))
        elif q.dtype == torch.float32:
            check(lib.psa_attention_bw_entries(_ptr(rowptr), _ptr(col), _ptr(q), _ptr(k), _ptr(v), _ptr(bias),
                                               _bias_heads(bias), scale, _ptr(grad_out), _ptr(out), _ptr(stat), M, N, H,
                                               K, F, nnz, _ptr(p), _ptr(ds), _ptr(ws), ws_bytes, _stream()))
        else:
            check(lib.psa_attention_half_bw_entries(_DTYPE_ID[q.dtype], _ptr(rowptr), _ptr(col), _ptr(q), _ptr(k),
                                                    _ptr(v), _ptr(bias), _bias_heads(bias), scale, _ptr(grad_out),
                                                    _ptr(out), _ptr(stat), M, N, H, K, F, nnz, _ptr(p), _ptr(ds),
                                                    _ptr(ws), ws_bytes, _stream()))
    return p, ds


def attention_raw(rowptr, col, q, k, v, bias=None, scale: float = 1.0, dropout_p: float = 0.0, seed: int = 0):
    """The forward alone, without autograd: (out, stat) with stat [M, H, 2] = {m, l} (2-D operands: [M, 2]).
    dropout_p > 0 takes the dropout entry points with this seed (an int: attention_bw needs the same one)."""
    rowptr, col, q, k, v, bias, _, flat = _attention_operands(rowptr, col, q, k, v, bias)
    dropout_p, seed = _dropout_args(dropout_p, seed, draw=False)
    out, stat = _attention_fw_raw(rowptr, col, q.detach(), k.detach(), v.detach(),
                                  None if bias is None else bias.detach(), float(scale), dropout_p, seed)
    return (out[:, 0], stat[:, 0]) if flat else (out, stat)


def attention_bw(rowptr, col, q, k, v, bias, scale: float, grad_out, out, stat, csc=None,
                 want=(True, True, True, True), dropout_p: float = 0.0, seed: int = 0):
    """(grad_q, grad_k, grad_v, grad_bias) of attention from what its forward left (heads-form operands, out and
    stat of attention_raw); None where `want` says so.  p and dS [nnz, H] live only inside this call.  dropout_p and
    seed are the forward's: the mask is recomputed from them, and p below is then p * keep * inv_keep."""
    want_q, want_k, want_v, want_b = want
    grad_out = grad_out.contiguous()
    dropout_p, seed = _dropout_args(dropout_p, seed, draw=False)
    p, ds = _attention_bw_entries_raw(rowptr, col, q, k, v, bias, scale, grad_out, out, stat, dropout_p, seed)
    grad_q = grad_k = grad_v = grad_b = None
    if q.dtype != torch.float32:  # psa_spmm_heads_half: fp32 sums, scale before the one rounding, no fp32 copies
        if want_q:
            grad_q = spmm_heads_half_raw(rowptr, col, ds, k, scale)
        if want_k or want_v:
            colptr, row_csc, csr2csc = _csc_view(csc, rowptr, col, k.shape[0])
            if want_k:
                grad_k = spmm_heads_half_raw(colptr, row_csc, _gather_rows_raw(ds, csr2csc), q, scale)
            if want_v:
                grad_v = spmm_heads_half_raw(colptr, row_csc, _gather_rows_raw(p, csr2csc), grad_out, 1.0)
        if want_b and bias is not None:
            grad_b = ds.sum(dim=1) if bias.dim() == 1 else ds
        return grad_q, grad_k, grad_v, grad_b
    if want_q:  # grad_q[r, h] = scale * sum over the row's entries of dS[e, h] * k[col[e], h]
        grad_q = _spmm_heads_raw(rowptr, col, ds, k)
        if scale != 1.0:
            grad_q *= scale
    if want_k or want_v:
        csc = _csc_view(csc, rowptr, col, k.shape[0])
        if want_k:  # grad_k[c, h] = scale * sum over the column's entries of dS[e, h] * q[row(e), h]
            grad_k = _spmm_heads_transposed(csc, ds, q)
            if scale != 1.0:
                grad_k *= scale
        if want_v:  # grad_v[c, h] = sum over the column's entries of p[e, h] * grad_out[row(e), h]
            grad_v = _spmm_heads_transposed(csc, p, grad_out)
    if want_b and bias is not None:
        grad_b = ds.sum(dim=1) if bias.dim() == 1 else ds
    return grad_q, grad_k, grad_v, grad_b


class _Attention(torch.autograd.Function):
    """Heads-form operands, already checked.  Saves q, k, v, out, stat and the caller's bias: no tensor with nnz
    rows of its own (the pattern is the caller's and rides on ctx)."""

    @staticmethod
    def forward(ctx, q, k, v, bias, rowptr, col, scale, csc, dropout_p, seed):
        out, stat = _attention_fw_raw(rowptr, col, q, k, v, bias, scale, dropout_p, seed)
        ctx.save_for_backward(q, k, v, bias, out, stat)
        ctx.pattern, ctx.scale, ctx.csc = (rowptr, col), scale, csc
        ctx.dropout_p, ctx.seed = dropout_p, seed  # two Python scalars: the backward recomputes the mask
        return out

    @staticmethod
    def backward(ctx, grad):
        q, k, v, bias, out, stat = ctx.saved_tensors
        rowptr, col = ctx.pattern
        grads = attention_bw(rowptr, col, q, k, v, bias, ctx.scale, grad, out, stat, ctx.csc,
                             ctx.needs_input_grad[:4], ctx.dropout_p, ctx.seed)
        return grads + (None, None, None, None, None, None)


def attention(rowptr: torch.Tensor, col: torch.Tensor, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
              bias: Optional[torch.Tensor] = None, scale: float = 1.0, csc=None, dropout_p: float = 0.0,
              seed: Optional[int] = None) -> torch.Tensor:
    """[M, H, F]: out[r, h, :] = sum over the entries of row r of p[e, h] * v[col[e], h, :], p[., h] the softmax
    over the row of s[e, h] = scale * <q[row(e), h, :], k[col[e], h, :]> (+ bias[e, h] or bias[e]), with q
    [M, H, K], k [N, H, K], v [N, H, F] all float32 or all bfloat16 and bias fp32 [nnz] or [nnz, H]; 2-D q, k, v
    are one head and give [M, F].  One pass per row (psa_attention_fw); only {max, sum} per row and head is kept
    for the backward, which recomputes the scores (psa_attention_bw_entries) and takes the gradients of q, k, v
    from psa_spmm_heads over the CSR and the CSC view.  bfloat16 operands (psa_attention_half_fw /
    _bw_entries / psa_spmm_heads_half) give a bfloat16 out and bfloat16 gradients: gathers are half-width,
    all arithmetic, stat and grad_bias are fp32, each bfloat16 result is rounded once.  Differentiable in
    q, k, v and bias; `scale` is a float.  `csc` as for sddmm.

    dropout_p in [0, 1) drops attention weights after the softmax, inside the kernels (the psa_attention_*dropout*
    entry points): out = inv_keep * sum keep(e, h) * p[e, h] * v[col[e], h, :] with inv_keep = float32(1 / (1 -
    dropout_p)) and keep(e, h) a counter-based draw that depends on (seed, position of the entry in CSR order, head)
    only, so fp32 and bf16 operands drop the same entries and attention_dropout_mask(nnz, H, dropout_p, seed) gives
    the same mask to the unfused chain.  The backward recomputes the mask; nothing more is saved.  `seed` is an int
    in [0, 2^64); seed=None draws one from torch's CPU default generator (torch.manual_seed reproduces a run; no
    device read, no sync).  The seed is a launch argument: a captured graph replays the same mask at every replay.
    dropout_p == 0.0 is the op without dropout, bit for bit, and ignores the seed."""
    rowptr, col, q, k, v, bias, _, flat = _attention_operands(rowptr, col, q, k, v, bias)
    scale = float(scale)
    dropout_p, seed = _dropout_args(dropout_p, seed)  # resolved here: forward and backward see one value
    if needs_grad(q) or needs_grad(k) or needs_grad(v) or needs_grad(bias):
        out = _Attention.apply(q, k, v, bias, rowptr, col, scale, csc, dropout_p, seed)
    else:
        out = _attention_fw_raw(rowptr, col, q, k, v, bias, scale, dropout_p, seed)[0]
    return out[:, 0] if flat else out


# ---- fused GAT attention: additive LeakyReLU scores in the one-pass kernels (csrc/attention.hip, A::kGat) ----

def _slope_arg(negative_slope, who: str = "gat_attention") -> float:
    """negative_slope checked: a finite Python number (0 and negative slopes are served)."""
    if isinstance(negative_slope, bool) or not isinstance(negative_slope, (int, float)):
        raise TypeError(f"{who}: negative_slope must be a float (got {type(negative_slope).__name__})")
    negative_slope = float(negative_slope)
    if negative_slope != negative_slope or negative_slope in (float("inf"), float("-inf")):
        raise ValueError(f"{who}: negative_slope must be finite (got {negative_slope})")
    return negative_slope


def _gat_operands(rowptr, col, a_row, a_col, v, bias):
    """The checked, contiguous operands in heads form (a_row [M, H], a_col [N, H], v [N, H, F]) and whether the
    caller gave the one-head form.  Nothing is copied for alignment: the kernels take the element form for a v that
    does not start on 16 bytes."""
    rowptr, col, M, nnz = _heads_pattern(rowptr, col)
    a_row, a_col, v = _attention_dense(a_row, "a_row"), _attention_dense(a_col, "a_col"), _attention_dense(v, "v")
    if not (a_row.dtype == a_col.dtype == v.dtype):
        raise TypeError(f"gat_attention: a_row, a_col, v must share one dtype (got {a_row.dtype}, {a_col.dtype}, "
                        f"{v.dtype})")
    dims = (a_row.dim(), a_col.dim(), v.dim())
    if dims not in ((1, 1, 2), (2, 2, 3)):
        raise ValueError(f"gat_attention: a_row, a_col, v must be [M], [N], [N, F] or [M, H], [N, H], [N, H, F] "
                         f"(got {tuple(a_row.shape)}, {tuple(a_col.shape)}, {tuple(v.shape)})")
    flat = v.dim() == 2
    if flat:
        a_row, a_col, v = a_row.unsqueeze(1), a_col.unsqueeze(1), v.unsqueeze(1)
    N, H, F = v.shape
    if a_row.shape != (M, H) or a_col.shape != (N, H):
        raise ValueError(f"gat_attention: a_row must be [{M}, H], a_col [N, H] and v [N, H, F] "
                         f"(got {tuple(a_row.shape)}, {tuple(a_col.shape)}, {tuple(v.shape)})")
    if H < 1 or F < 1:
        raise ValueError("gat_attention: H and F must be at least 1")
    if bias is not None:
        bias = _f32(bias, "bias")
        if bias.shape not in ((nnz,), (nnz, H)):
            raise ValueError(f"gat_attention: bias must be [{nnz}] or [{nnz}, {H}] (got {tuple(bias.shape)})")
    return rowptr, col, a_row, a_col, v, bias, flat


def _gat_fw_raw(rowptr, col, a_row, a_col, v, bias, slope: float, dropout_p: float = 0.0, seed: int = 0):
    """(out [M, H, F], stat [M, H, 2]) from checked heads-form operands."""
    M, H = a_row.shape
    N, F, nnz = v.shape[0], v.shape[2], col.numel()
    out = torch.empty((M, H, F), dtype=v.dtype, device=v.device)
    stat = torch.empty((M, H, 2), dtype=torch.float32, device=v.device)
    lib = _lib.load()
    ws_bytes = lib.psa_attention_workspace_bytes(nnz, H, F)
    ws = _workspace(ws_bytes, v.device) if ws_bytes else None
    with _on(v.device):
        if v.dtype == torch.float32:
            check(lib.psa_gat_attention_fw(_ptr(rowptr), _ptr(col), _ptr(a_row), _ptr(a_col), _ptr(v), _ptr(bias),
                                           _bias_heads(bias), slope, dropout_p, seed, M, N, H, F, nnz, _ptr(out),
                                           _ptr(stat), _ptr(ws), ws_bytes, _stream()))
        else:
            check(lib.psa_gat_attention_half_fw(_DTYPE_ID[v.dtype], _ptr(rowptr), _ptr(col), _ptr(a_row), _ptr(a_col),
                                                _ptr(v), _ptr(bias), _bias_heads(bias), slope, dropout_p, seed, M, N, H,
                                                F, nnz, _ptr(out), _ptr(stat), _ptr(ws), ws_bytes, _stream()))
    return out, stat


def _gat_bw_entries_raw(rowptr, col, a_row, a_col, v, bias, slope: float, grad_out, out, stat, dropout_p: float = 0.0,
                        seed: int = 0):
    """(p * D [nnz, H], dZ [nnz, H]) with D = keep * inv_keep (1 without dropout): the per-entry half of the
    backward, from the saved {m, l}."""
    M, H = a_row.shape
    N, F, nnz = v.shape[0], v.shape[2], col.numel()
    if grad_out.dtype != v.dtype:
        raise TypeError(f"gat_attention: grad_out must be {v.dtype} as a_row, a_col, v (got {grad_out.dtype})")
    p = torch.empty((nnz, H), dtype=torch.float32, device=v.device)
    dz = torch.empty((nnz, H), dtype=torch.float32, device=v.device)
    lib = _lib.load()
    ws_bytes = lib.psa_attention_workspace_bytes(nnz, H, F)
    ws = _workspace(ws_bytes, v.device) if ws_bytes else None
    with _on(v.device):
        if v.dtype == torch.float32:
            check(lib.psa_gat_attention_bw_entries(_ptr(rowptr), _ptr(col), _ptr(a_row), _ptr(a_col), _ptr(v),
                                                   _ptr(bias), _bias_heads(bias), slope, dropout_p, seed, _ptr(grad_out),
                                                   _ptr(out), _ptr(stat), M, N, H, F, nnz, _ptr(p), _ptr(dz), _ptr(ws),
                                                   ws_bytes, _stream()))
        else:
            check(lib.psa_gat_attention_half_bw_entries(_DTYPE_ID[v.dtype], _ptr(rowptr), _ptr(col), _ptr(a_row),
                                                        _ptr(a_col), _ptr(v), _ptr(bias), _bias_heads(bias), slope,
                                                        dropout_p, seed, _ptr(grad_out), _ptr(out), _ptr(stat), M, N, H,
                                                        F, nnz, _ptr(p), _ptr(dz), _ptr(ws), ws_bytes, _stream()))
    return p, dz


def gat_attention_raw(rowptr, col, a_row, a_col, v, bias=None, negative_slope: float = 0.2, dropout_p: float = 0.0,
                      seed: int = 0):
    """The forward alone, without autograd: (out, stat) with stat [M, H, 2] = {m, l} of the scores after the
    activation (one-head operands: [M, 2]).  dropout_p > 0 needs the seed as an int (gat_attention_bw takes the same)."""
    rowptr, col, a_row, a_col, v, bias, flat = _gat_operands(rowptr, col, a_row, a_col, v, bias)
    slope = _slope_arg(negative_slope)
    dropout_p, seed = _dropout_args(dropout_p, seed, "gat_attention", draw=False)
    out, stat = _gat_fw_raw(rowptr, col, a_row.detach(), a_col.detach(), v.detach(),
                            None if bias is None else bias.detach(), slope, dropout_p, seed)
    return (out[:, 0], stat[:, 0]) if flat else (out, stat)


def gat_attention_bw(rowptr, col, a_row, a_col, v, bias, negative_slope: float, grad_out, out, stat, csc=None,
                     want=(True, True, True, True), dropout_p: float = 0.0, seed: int = 0):
    """(grad_a_row, grad_a_col, grad_v, grad_bias) of gat_attention from what its forward left (heads-form operands,
    out and stat of gat_attention_raw); None where `want` says so.  p and dZ [nnz, H] live only inside this call.
    The sums of dZ are fp32 (psa_segment_reduce, in entry order) and rounded once for bfloat16 operands; the CSC view
    is asked for only by the gradients of a_col and v."""
    want_r, want_c, want_v, want_b = want
    grad_out = grad_out.contiguous()
    slope = _slope_arg(negative_slope)
    dropout_p, seed = _dropout_args(dropout_p, seed, "gat_attention", draw=False)
    p, dz = _gat_bw_entries_raw(rowptr, col, a_row, a_col, v, bias, slope, grad_out, out, stat, dropout_p, seed)
    grad_r = grad_c = grad_v = grad_b = None
    if want_r:  # grad_a_row[r, h] = sum over the row's entries of dZ[e, h]
        grad_r = _segment_csr_raw(dz, rowptr, "sum").to(a_row.dtype)
    if want_c or want_v:
        colptr, row_csc, csr2csc = csc = _csc_view(csc, rowptr, col, v.shape[0])
        if want_c:  # grad_a_col[c, h] = sum over the column's entries of dZ[e, h]
            grad_c = _segment_csr_raw(dz, colptr, "sum", perm=csr2csc).to(a_col.dtype)
        if want_v:  # grad_v[c, h] = sum over the column's entries of (p * D)[e, h] * grad_out[row(e), h]
            if v.dtype != torch.float32:
                grad_v = spmm_heads_half_raw(colptr, row_csc, _gather_rows_raw(p, csr2csc), grad_out, 1.0)
            else:
                grad_v = _spmm_heads_transposed(csc, p, grad_out)
    if want_b and bias is not None:
        grad_b = dz.sum(dim=1) if bias.dim() == 1 else dz
    return grad_r, grad_c, grad_v, grad_b


class _GatAttention(torch.autograd.Function):
    """Heads-form operands, already checked.  Saves a_row, a_col, v, out, stat and the caller's bias: no tensor with
    nnz rows of its own (the pattern is the caller's and rides on ctx)."""

    @staticmethod
    def forward(ctx, a_row, a_col, v, bias, rowptr, col, slope, csc, dropout_p, seed):
        out, stat = _gat_fw_raw(rowptr, col, a_row, a_col, v, bias, slope, dropout_p, seed)
        ctx.save_for_backward(a_row, a_col, v, bias, out, stat)
        ctx.pattern, ctx.slope, ctx.csc = (rowptr, col), slope, csc
        ctx.dropout_p, ctx.seed = dropout_p, seed  # two Python scalars: the backward recomputes the mask
        return out

    @staticmethod
    def backward(ctx, grad):
        a_row, a_col, v, bias, out, stat = ctx.saved_tensors
        rowptr, col = ctx.pattern
        grads = gat_attention_bw(rowptr, col, a_row, a_col, v, bias, ctx.slope, grad, out, stat, ctx.csc,
                                 ctx.needs_input_grad[:4], ctx.dropout_p, ctx.seed)
        return grads + (None, None, None, None, None, None)


def gat_attention(rowptr: torch.Tensor, col: torch.Tensor, a_row: torch.Tensor, a_col: torch.Tensor, v: torch.Tensor,
                  bias: Optional[torch.Tensor] = None, negative_slope: float = 0.2, csc=None, dropout_p: float = 0.0,
                  seed: Optional[int] = None) -> torch.Tensor:
    """[M, H, F]: the aggregation of a GAT layer in one pass per row.  With a_row [M, H], a_col [N, H] (one scalar
    per node and head) and v [N, H, F], all float32 or all bfloat16, and bias fp32 [nnz] or [nnz, H]:

        z[e, h]      = (a_row[row(e), h] + a_col[col[e], h]) (+ bias)
        s[e, h]      = z if z > 0 else negative_slope * z        (z == 0 takes the slope, as leaky_relu's backward)
        out[r, h, :] = sum over the entries of row r of softmax_row(s)[e, h] * v[col[e], h, :]

    1-D a_row [M], a_col [N] with v [N, F] are one head and give [M, F].  The kernels are those of `attention` with
    the dot replaced by the sum (psa_gat_attention_fw / _bw_entries and their _half forms): nothing per entry is
    kept, the backward recomputes the scores from {max, sum} per row and head, grad_a_row and grad_a_col are
    segment sums of dZ = dS * (1 or negative_slope) over the rows and the columns, grad_v is psa_spmm_heads over
    the CSC view, grad_bias is dZ.  bfloat16 operands: half-width loads, fp32 arithmetic, each bfloat16 result
    rounded once; bias and its gradient stay fp32.  Differentiable in a_row, a_col, v and bias; negative_slope is a
    finite Python float.  A -inf bias masks an entry for negative_slope > 0; with negative_slope == 0 it is
    0 * -inf = NaN and poisons its row and head.  `csc`, dropout_p and seed as for `attention`: the same mask for
    the same seed."""
    rowptr, col, a_row, a_col, v, bias, flat = _gat_operands(rowptr, col, a_row, a_col, v, bias)
    slope = _slope_arg(negative_slope)
    dropout_p, seed = _dropout_args(dropout_p, seed, "gat_attention")  # resolved here: forward and backward see one value
    if needs_grad(a_row) or needs_grad(a_col) or needs_grad(v) or needs_grad(bias):
        out = _GatAttention.apply(a_row, a_col, v, bias, rowptr, col, slope, csc, dropout_p, seed)
    else:
        out = _gat_fw_raw(rowptr, col, a_row, a_col, v, bias, slope, dropout_p, seed)[0]
    return out[:, 0] if flat else out


# ---- pair intersection (csrc/intersect.hip) ------------------------------------------

_INTERSECT_DTYPES = (torch.float32, torch.float64, torch.int64)


def _list_family(lists, name: str):
    if not isinstance(lists, (tuple, list)) or len(lists) != 3:
        raise TypeError(f"{name} must be a (ptr, idx, val or None) triple")
    ptr, idx, val = lists
    ptr, idx = _index(ptr, f"{name} ptr"), _index(idx, f"{name} idx")
    if ptr.numel() < 1:
        raise ValueError(f"{name} ptr must have at least one element")
    if val is not None:
        _gpu(val, f"{name} val")
    return ptr, idx, val


def pair_intersect(x, y, pair_x: torch.Tensor, pair_y: torch.Tensor, weight: Optional[torch.Tensor] = None,
                   dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """out[p] = sum over k in X[pair_x[p]] n Y[pair_y[p]] of x_val * y_val * weight[k] (psa_pair_intersect).
    x and y are (ptr, idx, val | None) triples, list families in CSR form: every list ascending and free of
    duplicates.  A missing val or weight counts as ones; weight is read at the common index, so it must cover
    every index value.  dtype (default: that of the values and the weight, int64 without any) is float32,
    float64 or int64, the counting form, which takes neither values nor weight.  A pair index outside its
    family writes 0.  No scratch, no host read.  The raw op: not differentiable."""
    x_ptr, x_idx, x_val = _list_family(x, "x")
    y_ptr, y_idx, y_val = _list_family(y, "y")
    pair_x, pair_y = _index(pair_x, "pair_x"), _index(pair_y, "pair_y")
    if pair_x.numel() != pair_y.numel():
        raise ValueError(f"pair_x and pair_y differ in length ({pair_x.numel()}, {pair_y.numel()})")
    if weight is not None:
        _gpu(weight, "weight")
    given = [(n, t) for n, t in (("x val", x_val), ("y val", y_val), ("weight", weight)) if t is not None]
    if dtype is None:
        dtype = given[0][1].dtype if given else torch.int64
    if dtype not in _INTERSECT_DTYPES:
        raise TypeError(f"pair_intersect: dtype must be float32, float64 or int64 (got {dtype})")
    if dtype == torch.int64 and given:
        raise TypeError("pair_intersect: the counting form (int64) takes no values and no weight")
    for name, t in given:
        if t.dtype != dtype:
            raise TypeError(f"pair_intersect: {name} must be {dtype} (got {t.dtype})")
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"pair_intersect: {name} must be a contiguous 1-D tensor")
    for name, val, idx in (("x val", x_val, x_idx), ("y val", y_val, y_idx)):
        if val is not None and val.numel() != idx.numel():
            raise ValueError(f"pair_intersect: {name} must have one entry per index ({val.numel()}, {idx.numel()})")
    dev = pair_x.device
    for name, t in (("x ptr", x_ptr), ("x idx", x_idx), ("y ptr", y_ptr), ("y idx", y_idx), ("pair_y", pair_y)) \
            + tuple(given):
        if t.device != dev:
            raise ValueError(f"pair_intersect: {name} is on {t.device}, pair_x on {dev}")
    P = pair_x.numel()
    out = torch.empty(P, dtype=dtype, device=dev)
    if P and (x_idx.numel() == 0 or y_idx.numel() == 0):
        return out.zero_()  # a family without entries has no storage to point at, and no intersection
    with _on(dev):
        check(_lib.load().psa_pair_intersect(_DTYPE_ID[dtype], _ptr(x_ptr), _ptr(x_idx), _ptr(x_val), x_ptr.numel() - 1,
                                             _ptr(y_ptr), _ptr(y_idx), _ptr(y_val), y_ptr.numel() - 1, _ptr(weight),
                                             _ptr(pair_x), _ptr(pair_y), P, _ptr(out), _stream()))
    return out


# ---- segmented top-k selection (csrc/topk.hip) -------------------------------------------

TOPK_SHORT, TOPK_LDS = 64, 4096  # segment lengths up to which the keys sit in registers / in LDS
TOPK_GRID, TOPK_CHUNK = 2048, 256  # workgroups of the long-segment kernel; segments each takes per trip


def _topk_k(k, nseg: int):
    """(scalar k, k_seg or None) from an int or an int64[nseg] array / tensor."""
    if isinstance(k, bool):
        raise TypeError("k must be an int or an int64 tensor with one entry per segment")
    if isinstance(k, int):
        return k, None
    if not hasattr(k, "dtype") or "int64" not in str(k.dtype):
        raise TypeError("k must be an int or an int64 tensor with one entry per segment")
    if k.ndim != 1 or k.shape[0] != nseg:
        raise ValueError(f"k must have one entry per segment ({nseg}), got shape {tuple(k.shape)}")
    return 0, k


def segment_topk(value: torch.Tensor, indptr: torch.Tensor, k, perm: Optional[torch.Tensor] = None,
                 largest: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """keep uint8[n]: 1 for the k greatest (largest=False: smallest) of value[perm[j]] over the positions j
    of every segment of indptr (int64[nseg + 1]), 0 for the others, in value's order.  value is 1-D
    float32, float64, int32, int64, float16 or bfloat16; k an int or an int64[nseg] tensor (k <= 0 keeps
    nothing, k >= the length everything).  NaN counts as the greatest value in both directions, -0.0
    equals +0.0, ties go to the earlier position of the segment (include/paddle_sparse_hip.h states the
    rule in full).  keep starts zero-filled unless out (uint8[n]) is given: only positions inside a valid
    segment are written.  One or two launches, no scratch, no host read: capturable.  Not differentiable."""
    _gpu(value, "value")
    if value.dtype not in _DTYPE_ID:
        raise TypeError(f"segment_topk: unsupported value dtype {value.dtype}")
    if value.dim() != 1:
        raise ValueError(f"segment_topk: value must be 1-D (got {tuple(value.shape)})")
    value, indptr = value.detach().contiguous(), _index(indptr, "indptr")
    n, nseg, dev = value.numel(), indptr.numel() - 1, value.device
    if nseg < 0:
        raise ValueError("indptr must not be empty")
    k, k_seg = _topk_k(k, nseg)
    if k_seg is not None:
        k_seg = _index(k_seg, "k")
    if perm is not None:
        perm = _index(perm, "perm")
        if perm.numel() != n:
            raise ValueError(f"perm must have one entry per value ({n}), got {perm.numel()}")
    for name, t in (("indptr", indptr), ("k", k_seg), ("perm", perm)):
        if t is not None and t.device != dev:
            raise ValueError(f"segment_topk: {name} is on {t.device}, value on {dev}")
    if out is None:
        out = torch.zeros(n, dtype=torch.uint8, device=dev)
    else:
        _gpu(out, "out")
        if out.dtype != torch.uint8 or out.dim() != 1 or out.numel() != n or not out.is_contiguous() \
                or out.device != dev:
            raise ValueError(f"out must be a contiguous uint8[{n}] tensor on {dev}")
    if n > 0 and nseg > 0:
        with _on(dev):
            check(_lib.load().psa_segment_topk(_ptr(value), _DTYPE_ID[value.dtype], _ptr(perm), _ptr(indptr), nseg, n,
                                               int(k), _ptr(k_seg), int(bool(largest)), _ptr(out), _stream()))
    return out


_TOPK_HOST_DTYPES = {"float32": 0, "float64": 1, "int32": 2, "int64": 3, "float16": 4}


def segment_topk_host(value, indptr, k, perm=None, largest: bool = True, out=None, dtype: Optional[str] = None):
    """segment_topk run serially on the host by the kernels' own steps (numpy arrays in, keep uint8[n]
    numpy out): what the CPU suite holds the restatement to.  dtype="bfloat16" reads a uint16 array as
    bfloat16 bits (numpy has no such type)."""
    import numpy as np

    value = np.ascontiguousarray(value)
    if dtype == "bfloat16":
        if value.dtype != np.uint16:
            raise TypeError("dtype='bfloat16' takes the bits as a uint16 array")
        dtype_id = 5
    elif dtype is None and value.dtype.name in _TOPK_HOST_DTYPES:
        dtype_id = _TOPK_HOST_DTYPES[value.dtype.name]
    else:
        raise TypeError(f"segment_topk_host: unsupported value dtype {value.dtype} (dtype={dtype!r})")
    indptr = np.ascontiguousarray(indptr, np.int64)
    if value.ndim != 1 or indptr.ndim != 1 or indptr.size < 1:
        raise ValueError("value must be 1-D, indptr 1-D and not empty")
    n, nseg = value.size, indptr.size - 1
    k, k_seg = _topk_k(k, nseg)
    k_seg = None if k_seg is None else np.ascontiguousarray(k_seg, np.int64)
    perm = None if perm is None else np.ascontiguousarray(perm, np.int64)
    if perm is not None and perm.shape != (n,):
        raise ValueError(f"perm must have one entry per value ({n})")
    if out is None:
        out = np.zeros(n, np.uint8)
    elif out.dtype != np.uint8 or out.shape != (n,) or not out.flags.c_contiguous:
        raise ValueError(f"out must be a contiguous uint8[{n}] array")
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    check(_lib.load().psa_segment_topk_host(ptr(value), dtype_id, ptr(perm), ptr(indptr), nseg, n, int(k), ptr(k_seg),
                                            int(bool(largest)), ptr(out)))
    return out
