"""GPU: the index kernels every sparse op is stitched from (csrc/util.hip, csrc/merge.hip, csrc/spspmm.hip)
against tests/index_ref.py on inputs built AT their edges: scan sizes and carries at the wave (512), tile (2048)
and second-level (1024 blocks) boundaries of count2ptr, every element width of the row gather through the row
size and through the alignment of either operand, the window gather of the halo pack, one inversion at a lane,
wave or workgroup edge of make_keys, merges whose totals, runs and splits sit at the 2048-key tile, and the
expand step of spspmm with every value type, one-sided values and both key forms.

Every comparison is exact (np.array_equal / torch.equal; float payloads as integer bit patterns).  Direct C-ABI
calls write into a slice of a larger buffer filled with a sentinel, and the elements either side must keep it.
No kernel here is given an index outside its operand: `perm` and `colA` are in range by construction, and the
only out-of-range inputs are the bincount indices its kernel documents and guards.
"""
import functools

import numpy as np
import pytest
import torch

import index_ref as ir
from sort_cases import payload_bits

pytestmark = pytest.mark.gpu

SENT = -0x0123456789abcdef      # int64 sentinel
SENT8 = 0xa5                    # byte sentinel
TORCH = {"float32": torch.float32, "bfloat16": torch.bfloat16, "uint8": torch.uint8, "float64": torch.float64,
         "int32": torch.int32, "int64": torch.int64}
VALUE_TYPES = ("float32", "float64", "int32", "int64")


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()


def host(t):
    return t.cpu().numpy()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    """A float tensor as the integers of its bit patterns (NaN payloads and signed zeros compare as stored)."""
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    return t


def same_bits(got, want_np, what=""):
    """got (GPU tensor) equals want (numpy) in dtype, shape and every bit."""
    want = torch.from_numpy(np.array(want_np))
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{tuple(got.shape)} for {want.dtype}{tuple(want.shape)}"
    if not torch.equal(bits(got), bits(want)):
        bad = torch.nonzero((bits(got) != bits(want)).reshape(-1)).reshape(-1)
        raise AssertionError(f"{what}: {bad.numel()} of {want.numel()} differ, first at {int(bad[0])}: "
                             f"{got.reshape(-1)[bad[0]].item()} for {want.reshape(-1)[bad[0]].item()}")


# ---------------------------------------------------------------------------------------------
# count2ptr
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", ir.SCAN_SIZES)
def test_count2ptr_edges(n):
    """Sizes at the wave, tile and second-level edges (the last two sizes give per = 2 and per = 3 block sums a
    thread), with carries that must cross each of them and sums far past 2^32."""
    from paddle_sparse_amd import ops

    for label, kw in ir.scan_cases(n):
        counts = ir.scan_counts(n, **kw)
        got = host(ops.count2ptr(dev(counts)))
        want = ir.count2ptr(counts)
        assert got.shape == (n + 1,) and int(got[0]) == 0, label
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"n = {n}, {label}: {bad.size} pointers differ, first ptr[{bad[0]}] = {got[bad[0]]} "
                                 f"for {want[bad[0]]} (block {(bad[0] - 1) // ir.SCAN_TILE})")
        if label == "ones":
            assert np.array_equal(got, np.arange(n + 1))


def test_count2ptr_abi_keeps_its_neighbours():
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    for n in (1, 2049, 3 * ir.SCAN_TILE):
        counts = ir.scan_counts(n, "random", seed=n)
        buf = torch.full((n + 1 + 32,), SENT, dtype=torch.int64, device="cuda")
        ws = torch.empty(lib.psa_count2ptr_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        c = dev(counts)
        _lib.check(lib.psa_count2ptr(c.data_ptr(), n, buf[16:].data_ptr(), ws.data_ptr(), ws.numel(), stream()))
        got = host(buf)
        assert np.all(got[:16] == SENT) and np.all(got[16 + n + 1:] == SENT)
        assert np.array_equal(got[16:16 + n + 1], ir.count2ptr(counts))


def test_count2ptr_refuses_a_short_workspace():
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    n = 2 * ir.SCAN_TILE + 1
    need = lib.psa_count2ptr_workspace_bytes(n)
    c = dev(ir.scan_counts(n, "ones"))
    out = torch.full((n + 1,), SENT, dtype=torch.int64, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.HipCoreError, match="workspace"):
        _lib.check(lib.psa_count2ptr(c.data_ptr(), n, out.data_ptr(), ws.data_ptr(), need - 1, stream()))
    assert bool((out == SENT).all())
    _lib.check(lib.psa_count2ptr(c.data_ptr(), n, out.data_ptr(), ws.data_ptr(), need, stream()))
    assert np.array_equal(host(out), np.arange(n + 1))


# ---------------------------------------------------------------------------------------------
# gather_rows
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", ir.GATHER_N)
def test_gather_rows_width_dispatch(n):
    """15 row sizes x 5 starts of src x 5 starts of out, through the C-ABI on byte buffers: every element width
    (16, 8, 4, 2, 1 bytes) is reached through the row size and through the alignment of either operand, with
    power-of-two chunk counts (shift) and 3, 5 and 65 chunks (division).  Bytes and guard bytes are compared."""
    from paddle_sparse_amd import _lib

    lib, s = _lib.load(), stream()
    R = ir.gather_rows_of(n)
    perm_h = ir.gather_perm(n, R, n)
    perm = dev(perm_h)
    assert int(perm_h.min()) >= 0 and int(perm_h.max()) < R
    rng = np.random.default_rng(n)
    guard = 64
    seen = set()
    for rb in ir.GATHER_ROW_BYTES:
        src_h = rng.integers(0, 256, 16 + R * rb, dtype=np.uint8)
        src_buf = dev(src_h)
        out_buf = torch.empty(2 * guard + 16 + n * rb, dtype=torch.uint8, device="cuda")
        assert src_buf.data_ptr() % 16 == 0 and out_buf.data_ptr() % 16 == 0
        for so in ir.GATHER_OFFSETS:
            want = ir.gather_bytes(src_h[so:so + R * rb], perm_h, rb)
            for oo in ir.GATHER_OFFSETS:
                out_buf.fill_(SENT8)
                at = guard + oo
                _lib.check(lib.psa_gather_rows(src_buf.data_ptr() + so, perm.data_ptr(), n, rb,
                                               out_buf.data_ptr() + at, s))
                got = host(out_buf)
                what = f"row_bytes {rb}, src + {so}, out + {oo} (width {ir.gather_width(rb, so, oo)})"
                assert np.array_equal(got[at:at + n * rb].reshape(n, rb), want), what
                assert np.all(got[:at] == SENT8) and np.all(got[at + n * rb:] == SENT8), what
                seen.add(ir.gather_width(rb, so, oo))
    assert seen == set(ir.GATHER_WIDTHS)


def test_gather_rows_views_and_shapes():
    from paddle_sparse_amd import ops

    rng = np.random.default_rng(0)
    R = 1000
    perm_h = ir.gather_perm(3333, R, 1)
    perm = dev(perm_h)
    # a transposed view: rows 160 bytes apart in memory order, not contiguous
    base_h = rng.integers(-2**31, 2**31 - 1, (40, R)).astype(np.int32)
    src = dev(base_h).view(torch.float32).t()
    assert not src.is_contiguous() and src.shape == (R, 40)
    same_bits(ops.gather_rows(src, perm), base_h.T[perm_h].view(np.float32), "transposed view")
    # 64-byte rows that start 4 bytes into their buffer: the 4-byte kernel, not the 16-byte one
    flat_h = rng.integers(-2**31, 2**31 - 1, 1 + R * 16).astype(np.int32)
    src = dev(flat_h).view(torch.float32)[1:].view(R, 16)
    assert src.is_contiguous() and src.data_ptr() % 16 == 4
    same_bits(ops.gather_rows(src, perm), flat_h[1:].reshape(R, 16)[perm_h].view(np.float32), "view at + 4 bytes")
    # no rows
    empty = ops.gather_rows(src, torch.empty(0, dtype=torch.int64, device="cuda"))
    assert empty.shape == (0, 16) and empty.dtype == torch.float32
    # trailing shape (4, 5): 80-byte rows, 5 chunks of 16 bytes
    tail_h = rng.integers(-2**31, 2**31 - 1, (R, 4, 5)).astype(np.int32)
    same_bits(ops.gather_rows(dev(tail_h).view(torch.float32), perm), tail_h[perm_h].view(np.float32), "trailing (4, 5)")
    same_bits(ops.gather_rows(dev(tail_h), perm), tail_h[perm_h], "trailing (4, 5), int32")


# ---------------------------------------------------------------------------------------------
# gather_rows_window
# ---------------------------------------------------------------------------------------------

def _window_src(name, W, lead, rng):
    """(src [R, W] of the named dtype whose data starts `lead` bytes into a fresh buffer, its bytes on the host)."""
    size = ir.WINDOW_ITEMSIZE[name]
    bytes_h = rng.integers(0, 256, lead + ir.WINDOW_R * W * size, dtype=np.uint8)
    flat = dev(bytes_h)[lead:]
    src = (flat if name == "uint8" else flat.view(TORCH[name])).view(ir.WINDOW_R, W)
    assert src.is_contiguous() and src.data_ptr() % 16 == lead
    return src, bytes_h[lead:]


@pytest.mark.parametrize("n", ir.WINDOW_N)
@pytest.mark.parametrize("name", sorted(ir.WINDOW_CASES))
def test_gather_rows_window(name, n):
    """src[perm, col0:col0 + width] bit for bit, for every class of (row size | offset | width) the dtype allows
    (16-byte, 4-byte and 1-byte kernels), windows at the start, at the end and over the whole row, chunk counts
    that are no power of two, and a src that starts 4 bytes (uint8: 1 byte) into its buffer."""
    from paddle_sparse_amd import ops

    size = ir.WINDOW_ITEMSIZE[name]
    rng = np.random.default_rng(n + size)
    perm_h = ir.gather_perm(n, ir.WINDOW_R, n)
    perm = dev(perm_h)
    leads = {"float32": (0, 4), "bfloat16": (0, 4), "uint8": (0, 1), "float64": (0,)}[name]
    for cls, W, col0, width in ir.WINDOW_CASES[name]:
        for lead in leads:
            src, bytes_h = _window_src(name, W, lead, rng)
            want = ir.gather_bytes(bytes_h, perm_h, width * size, stride=W * size, first=col0 * size)
            what = f"{name} W = {W}, window [{col0}, {col0 + width}), src + {lead} bytes ({cls})"
            got = ops.gather_rows_window(src, perm, col0, width)
            assert got.dtype == src.dtype and got.shape == (n, width) and got.is_contiguous(), what
            assert np.array_equal(host(got.view(torch.uint8)), want), what
            out = torch.empty((n, width), dtype=src.dtype, device="cuda")
            out.view(torch.uint8).fill_(SENT8)
            assert ops.gather_rows_window(src, perm, col0, width, out=out) is out
            assert np.array_equal(host(out.view(torch.uint8)), want), what + ", out="


def test_gather_rows_window_empty_results():
    from paddle_sparse_amd import ops

    src = torch.arange(300 * 16, dtype=torch.float32, device="cuda").view(300, 16)
    perm = dev(ir.gather_perm(257, 300, 0))
    got = ops.gather_rows_window(src, perm, 4, 0)
    assert got.shape == (257, 0) and got.dtype == torch.float32
    got = ops.gather_rows_window(src, perm, 16, 0)
    assert got.shape == (257, 0)
    got = ops.gather_rows_window(src, perm[:0], 4, 8)
    assert got.shape == (0, 8) and got.dtype == torch.float32


def test_gather_rows_window_errors():
    from paddle_sparse_amd import ops

    src = torch.arange(300 * 16, dtype=torch.float32, device="cuda").view(300, 16)
    perm = dev(ir.gather_perm(10, 300, 0))
    for col0, width in ((8, 9), (16, 1), (-1, 4), (0, 17)):
        with pytest.raises(ValueError):
            ops.gather_rows_window(src, perm, col0, width)
    with pytest.raises(ValueError):
        ops.gather_rows_window(src.t(), perm[:1] * 0, 0, 4)
    with pytest.raises(ValueError):
        ops.gather_rows_window(src[:, :8], perm, 0, 4)
    for out in (torch.empty((10, 5), device="cuda"), torch.empty((9, 4), device="cuda"),
                torch.empty((10, 4), dtype=torch.float64, device="cuda"), torch.empty((4, 10), device="cuda").t()):
        with pytest.raises(ValueError):
            ops.gather_rows_window(src, perm, 0, 4, out=out)


# ---------------------------------------------------------------------------------------------
# make_keys / split_keys
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", ir.KEY_N)
def test_make_keys_single_inversion_at_every_edge(n):
    """One inversion, at the element whose predecessor lives in the neighbouring lane (1, 63, 65, ...), wave
    (64, 512) or workgroup (256, 512), or at the last element: the flag must be 1 and the keys exact.  The sorted
    stream, also with equal keys across i = 64 and i = 256, gives 0."""
    from paddle_sparse_amd import ops

    for i in ir.inversion_positions(n):
        a, b = ir.inversion_stream(n, i, n)
        want, flag = ir.make_keys(a, b, ir.KEY_MUL)
        assert flag == 1
        keys, got = ops.make_keys(dev(a), dev(b), ir.KEY_MUL, check_sorted=True)
        assert got.dtype == torch.int32 and got.shape == (1,)
        assert int(got) == 1, f"inversion at {i} of {n} not seen"
        assert np.array_equal(host(keys), want), f"inversion at {i}"
    for equal_runs in (False, True):
        a, b = ir.sorted_stream(n, n, equal_runs=equal_runs)
        want, flag = ir.make_keys(a, b, ir.KEY_MUL)
        assert flag == 0
        keys, got = ops.make_keys(dev(a), dev(b), ir.KEY_MUL, check_sorted=True)
        assert int(got) == 0 and np.array_equal(host(keys), want)
    keys, got = ops.make_keys(dev(a), dev(b), ir.KEY_MUL, check_sorted=False)
    assert got is None and np.array_equal(host(keys), want)


def test_make_keys_single_element():
    from paddle_sparse_amd import ops

    a, b = ir.sorted_stream(1)
    keys, flag = ops.make_keys(dev(a), dev(b), ir.KEY_MUL, check_sorted=True)
    assert int(flag) == 0 and np.array_equal(host(keys), ir.make_keys(a, b, ir.KEY_MUL)[0])


@pytest.mark.parametrize("n", ir.SPLIT_N)
def test_split_keys_both_division_paths_in_one_wave(n):
    from paddle_sparse_amd import ops

    keys_h = ir.split_stream(n)
    keys = dev(keys_h)
    for div in ir.SPLIT_DIVS:
        want_hi, want_lo = ir.split_keys(keys_h, div)
        hi, lo = ops.split_keys(keys, div)
        assert np.array_equal(host(hi), want_hi) and np.array_equal(host(lo), want_lo), div
        hi, lo = ops.split_keys(keys, div, want_hi=False)
        assert hi is None and np.array_equal(host(lo), want_lo), div
        hi, lo = ops.split_keys(keys, div, want_lo=False)
        assert lo is None and np.array_equal(host(hi), want_hi), div


# ---------------------------------------------------------------------------------------------
# bincount / invert_permutation
# ---------------------------------------------------------------------------------------------

def test_bincount_one_hot_bin():
    from paddle_sparse_amd import ops

    n = 1 << 20
    assert host(ops.bincount(torch.zeros(n, dtype=torch.int64, device="cuda"), 1)).tolist() == [n]
    assert host(ops.bincount(torch.full((n,), 4, dtype=torch.int64, device="cuda"), 5)).tolist() == [0, 0, 0, 0, n]


@pytest.mark.parametrize("n", [255, 256, 257, 5000])
def test_bincount_ignores_indices_outside(n):
    from paddle_sparse_amd import ops

    size = 37
    rng = np.random.default_rng(n)
    index = rng.integers(0, size, n, dtype=np.int64)
    bad = rng.choice(n, n // 5, replace=False)
    index[bad] = rng.choice(np.array([-1, size, 1 << 40, ir.INT64_MIN], np.int64), bad.size)
    index[[0, n - 1]] = size, -1
    want = ir.bincount(index, size)
    assert int(want.sum()) < n and int(want.sum()) == int(((index >= 0) & (index < size)).sum())
    got = ops.bincount(dev(index), size)
    assert got.dtype == torch.int64 and np.array_equal(host(got), want)
    clean = np.where((index >= 0) & (index < size), index, 0)
    assert np.array_equal(host(ops.bincount(dev(clean), size)), ir.bincount(clean, size))
    assert ops.bincount(dev(index), 0).shape == (0,)


@pytest.mark.parametrize("kind", ir.PERM_KINDS)
def test_invert_permutation(kind):
    from paddle_sparse_amd import ops

    for n in ir.PERM_N:
        perm_h = ir.permutation(n, kind)
        perm = dev(perm_h)
        inv = ops.invert_permutation(perm)
        assert np.array_equal(host(inv), ir.invert_permutation(perm_h)), n
        ident = torch.arange(n, device="cuda")
        assert torch.equal(inv[perm], ident) and torch.equal(perm[inv], ident), n


# ---------------------------------------------------------------------------------------------
# merge_sorted
# ---------------------------------------------------------------------------------------------

def _merge_family(name):
    """total2049-na1 -> total2049, runs64 -> runs, long-short-below -> long-short: the cases of one family share a
    pytest case (the whole list would be 71)."""
    if name.startswith("total"):
        return name.split("-")[0]
    for family in ("alternating", "runs", "identical", "long-short", "short-long"):
        if name.startswith(family):
            return family
    return {"sparse-in-dense": "one-per-2047", "dense-in-sparse": "one-per-2047"}.get(name, name)


MERGE_FAMILIES = {}
for _name in ir.MERGE_CASES:
    MERGE_FAMILIES.setdefault(_merge_family(_name), []).append(_name)


@pytest.mark.parametrize("family", list(MERGE_FAMILIES))
def test_merge_sorted(family):
    """Merged keys, source and payload against the stable argsort of the concatenation.  The int32 payload is the
    concatenation index (so it must equal source); the float32 payload holds NaNs, denormals and signed zeros and
    is compared as bits."""
    for name in MERGE_FAMILIES[family]:
        _check_merge(name)


def _check_merge(name):
    from paddle_sparse_amd import ops

    a_h, b_h = ir.MERGE_CASES[name]()
    na, nb = a_h.size, b_h.size
    want_keys, want_src = ir.merge_sorted(a_h, b_h)
    a, b = dev(a_h), dev(b_h)
    idx = torch.arange(na + nb, dtype=torch.int32, device="cuda")
    merged, source, pay = ops.merge_sorted(a, b, idx[:na].clone(), idx[na:].clone())
    same_bits(merged, want_keys, f"{name}: merged")
    same_bits(source, want_src, f"{name}: source")
    assert pay.dtype == torch.int32 and torch.equal(pay.to(torch.int64), source), name
    bits_h = payload_bits(na + nb, na)
    fbits = dev(bits_h).view(torch.float32)
    merged, source, pay = ops.merge_sorted(a, b, fbits[:na].clone(), fbits[na:].clone())
    same_bits(merged, want_keys, f"{name}: merged (float payload)")
    same_bits(source, want_src, f"{name}: source (float payload)")
    assert pay.dtype == torch.float32, name
    same_bits(pay.view(torch.int32), bits_h[want_src], f"{name}: float payload bits")


@pytest.mark.parametrize("name", ["total4097-na2048", "runs2049", "long-short-middle"])
def test_merge_sorted_without_source_or_payload(name):
    from paddle_sparse_amd import ops

    a_h, b_h = ir.MERGE_CASES[name]()
    want_keys, want_src = ir.merge_sorted(a_h, b_h)
    a, b = dev(a_h), dev(b_h)
    merged, source, pay = ops.merge_sorted(a, b)
    assert pay is None
    same_bits(merged, want_keys, "merged")
    same_bits(source, want_src, "source")
    idx = torch.arange(a_h.size + b_h.size, dtype=torch.int32, device="cuda")
    merged, source, pay = ops.merge_sorted(a, b, idx[:a_h.size].clone(), idx[a_h.size:].clone(), want_source=False)
    assert source is None
    same_bits(merged, want_keys, "merged")
    same_bits(pay.to(torch.int64), want_src, "payload without source")
    merged, source, pay = ops.merge_sorted(a, b, want_source=False)
    assert source is None and pay is None
    same_bits(merged, want_keys, "merged alone")


def test_merge_sorted_abi_keeps_its_neighbours():
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    a_h, b_h = ir.MERGE_CASES["total4097-na2048"]()
    total = a_h.size + b_h.size
    want_keys, want_src = ir.merge_sorted(a_h, b_h)
    a, b = dev(a_h), dev(b_h)
    pay_in = torch.arange(total, dtype=torch.int32, device="cuda")
    keys = torch.full((total + 32,), SENT, dtype=torch.int64, device="cuda")
    src = torch.full((total + 32,), SENT, dtype=torch.int64, device="cuda")
    pay = torch.full((total + 32,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    _lib.check(lib.psa_merge_sorted(a.data_ptr(), a_h.size, b.data_ptr(), b_h.size, pay_in.data_ptr(),
                                    pay_in[a_h.size:].data_ptr(), keys[16:].data_ptr(), src[16:].data_ptr(),
                                    pay[16:].data_ptr(), stream()))
    for buf, want, sent in ((keys, want_keys, SENT), (src, want_src, SENT), (pay, want_src.astype(np.int32), 0x5a5a5a5a)):
        got = host(buf)
        assert np.all(got[:16] == sent) and np.all(got[16 + total:] == sent)
        assert np.array_equal(got[16:16 + total], want)


# ---------------------------------------------------------------------------------------------
# spspmm_count / spspmm_expand
# ---------------------------------------------------------------------------------------------

def _expand_inputs(name):
    from paddle_sparse_amd import ops

    c = ir.expand_case(name)
    assert int(c.colA.min()) >= 0 and int(c.colA.max()) < c.k   # colA is taken on trust by the kernels
    d = {f: dev(getattr(c, f)) for f in ("rowA", "colA", "rowptrB", "colB")}
    counts = ops.spspmm_count(d["colA"], d["rowptrB"])
    offsets = ops.count2ptr(counts)
    total = int(offsets[-1])
    owner = ops.ptr2ind(offsets, total)
    return c, d, counts, offsets, owner, total


@pytest.mark.parametrize("name", ir.EXPAND_CASES)
def test_spspmm_count_offsets_owner(name):
    c, d, counts, offsets, owner, total = _expand_inputs(name)
    want = ir.spspmm_products(c.rowA, c.colA, None, c.rowptrB, c.colB, None, c.n)
    same_bits(counts, want.counts, "counts")
    same_bits(offsets, want.offsets, "offsets")
    assert total == want.keys.size
    same_bits(owner, want.owner, "owner")


@pytest.mark.parametrize("dtype", VALUE_TYPES)
def test_spspmm_expand(dtype):
    """Keys and values of every product, in the documented order, for both key forms (i * n + j, and the packed
    (j << 32) | i of n = -1) and values on both sides, on A only, on B only, on neither."""
    for name in ir.EXPAND_CASES:
        _check_expand(name, dtype)


def _check_expand(name, dtype):
    from paddle_sparse_amd import ops

    c, d, counts, offsets, owner, total = _expand_inputs(name)
    vA_h = ir.small_int_values(c.colA.size, np.dtype(dtype), 1)
    vB_h = ir.small_int_values(c.colB.size, np.dtype(dtype), 2)
    vA, vB = dev(vA_h), dev(vB_h)
    for n in (c.n, -1):
        for mode in ("both", "A", "B", "none"):
            a_h, a = (vA_h, vA) if mode in ("both", "A") else (None, None)
            b_h, b = (vB_h, vB) if mode in ("both", "B") else (None, None)
            want = ir.spspmm_products(c.rowA, c.colA, a_h, c.rowptrB, c.colB, b_h, n)
            keys, vals = ops.spspmm_expand(d["rowA"], d["colA"], a, d["rowptrB"], d["colB"], b, offsets, owner, total,
                                           n, TORCH[dtype])
            what = f"{name} {dtype} n = {n} values: {mode}"
            same_bits(keys, want.keys, what + ", keys")
            if mode == "none":
                assert vals is None and want.vals is None
            else:
                same_bits(vals, want.vals, what + ", values")


def test_spspmm_expand_abi_keeps_its_neighbours():
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    c, d, counts, offsets, owner, total = _expand_inputs("total257")
    vA_h, vB_h = ir.small_int_values(c.colA.size, np.float32, 1), ir.small_int_values(c.colB.size, np.float32, 2)
    vA, vB = dev(vA_h), dev(vB_h)
    want = ir.spspmm_products(c.rowA, c.colA, vA_h, c.rowptrB, c.colB, vB_h, c.n)
    keys = torch.full((total + 32,), SENT, dtype=torch.int64, device="cuda")
    vals = torch.full((total + 32,), -777.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((c.colA.size + 32,), SENT, dtype=torch.int64, device="cuda")
    _lib.check(lib.psa_spspmm_count(d["colA"].data_ptr(), c.colA.size, d["rowptrB"].data_ptr(), cnt[16:].data_ptr(), stream()))
    _lib.check(lib.psa_spspmm_expand(0, d["rowA"].data_ptr(), d["colA"].data_ptr(), vA.data_ptr(), d["rowptrB"].data_ptr(),
                                     d["colB"].data_ptr(), vB.data_ptr(), offsets.data_ptr(), owner.data_ptr(), total, c.n,
                                     keys[16:].data_ptr(), vals[16:].data_ptr(), stream()))
    got = host(cnt)
    assert np.all(got[:16] == SENT) and np.all(got[16 + c.colA.size:] == SENT) and np.array_equal(got[16:16 + c.colA.size], want.counts)
    got = host(keys)
    assert np.all(got[:16] == SENT) and np.all(got[16 + total:] == SENT) and np.array_equal(got[16:16 + total], want.keys)
    got = host(vals)
    assert np.all(got[:16] == -777.0) and np.all(got[16 + total:] == -777.0)
    assert np.array_equal(got[16:16 + total].view(np.int32), want.vals.view(np.int32))


# ---------------------------------------------------------------------------------------------
# spspmm end to end: every value type, one-sided values, both routes
# ---------------------------------------------------------------------------------------------

M_, K_, N_ = 300, 200, 250
MODES = ("both", "A", "B")


class Spy:
    """Records the names of the `ops.<name>` called while active."""

    def __init__(self, *names):
        from paddle_sparse_amd import ops

        self.ops, self.names, self.calls = ops, names, []
        self.real = {n: getattr(ops, n) for n in names}

    def __enter__(self):
        for n in self.names:
            setattr(self.ops, n, (lambda n_: lambda *a, **k: self.calls.append(n_) or self.real[n_](*a, **k))(n))
        return self

    def __exit__(self, *exc):
        for n, f in self.real.items():
            setattr(self.ops, n, f)


@functools.lru_cache(maxsize=None)
def _operands():
    iA, iB = ir.random_coo(M_, K_, 4000, 11), ir.random_coo(K_, N_, 3000, 12)
    return iA, iB


@functools.lru_cache(maxsize=None)
def _reference(dtype, mode):
    """(indexA, valueA | None, indexB, valueB | None, index, value | None): computed once per (dtype, mode)."""
    iA, iB = _operands()
    vA = ir.small_nonzero_values(iA.shape[1], np.dtype(dtype), 13) if mode in ("both", "A") else None
    vB = ir.small_nonzero_values(iB.shape[1], np.dtype(dtype), 14) if mode in ("both", "B") else None
    index, value = ir.spspmm(iA, vA, iB, vB, M_, K_, N_)
    for x in (vA, vB, index, value):
        if x is not None:
            x.setflags(write=False)
    return iA, vA, iB, vB, index, value


def _dev_or_none(x):
    return None if x is None else dev(x)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", VALUE_TYPES)
def test_spspmm_every_type_and_one_sided_values(dtype, mode):
    """spspmm(...) and A @ B against the Gustavson product of tests/index_ref.py, index and value exactly
    (integer-valued data: every sum is exact in every type), with the route each value width must take: 4-byte
    values the column walk (sort_pairs_field on the packed keys), 8-byte values the row walk (index_sort)."""
    from paddle_sparse_amd import SparseTensor, spspmm

    iA, vA, iB, vB, want_index, want_value = _reference(dtype, mode)
    assert want_value.dtype == np.dtype(dtype)
    four = np.dtype(dtype).itemsize == 4
    with Spy("sort_pairs_field", "index_sort", "sort_pairs") as spy:
        index, value = spspmm(dev(iA), _dev_or_none(vA), dev(iB), _dev_or_none(vB), M_, K_, N_)
    if four:
        assert "sort_pairs_field" in spy.calls and "sort_pairs" not in spy.calls, spy.calls
    else:
        assert "index_sort" in spy.calls and "sort_pairs_field" not in spy.calls and "sort_pairs" not in spy.calls, spy.calls
    same_bits(index, want_index, "index")
    assert value.dtype == TORCH[dtype] and np.array_equal(host(value), want_value)
    A = SparseTensor(row=dev(iA[0]), col=dev(iA[1]), value=_dev_or_none(vA), sparse_sizes=(M_, K_))
    B = SparseTensor(row=dev(iB[0]), col=dev(iB[1]), value=_dev_or_none(vB), sparse_sizes=(K_, N_))
    with Spy("sort_pairs_field", "sort_pairs") as spy:
        C = A @ B
    assert ("sort_pairs_field" in spy.calls) == four and "sort_pairs" not in spy.calls, spy.calls
    row, col, value = C.coo()
    assert C.sparse_sizes() == (M_, N_)
    same_bits(torch.stack([row, col]), want_index, "A @ B index")
    assert value.dtype == TORCH[dtype] and np.array_equal(host(value), want_value)


def test_spspmm_without_values():
    from paddle_sparse_amd import SparseTensor, spspmm

    iA, _, iB, _, want_index, _ = _reference("float32", "both")
    index, value = spspmm(dev(iA), None, dev(iB), None, M_, K_, N_)
    assert value is None
    same_bits(index, want_index, "index")
    A = SparseTensor(row=dev(iA[0]), col=dev(iA[1]), sparse_sizes=(M_, K_))
    B = SparseTensor(row=dev(iB[0]), col=dev(iB[1]), sparse_sizes=(K_, N_))
    row, col, value = (A @ B).coo()
    assert value is None
    same_bits(torch.stack([row, col]), want_index, "A @ B index")


def test_spspmm_refuses_operands_of_two_types():
    from paddle_sparse_amd import SparseTensor, spspmm

    iA, vA, iB, vB, _, _ = _reference("float32", "both")
    with pytest.raises(ValueError):
        spspmm(dev(iA), dev(vA), dev(iB), dev(vB.astype(np.float64)), M_, K_, N_)
    A = SparseTensor(row=dev(iA[0]), col=dev(iA[1]), value=dev(vA), sparse_sizes=(M_, K_))
    B = SparseTensor(row=dev(iB[0]), col=dev(iB[1]), value=dev(vB.astype(np.float64)), sparse_sizes=(K_, N_))
    with pytest.raises(ValueError):
        A @ B


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_spspmm_coalesces_shuffled_operands_without_values_on_a(dtype):
    from paddle_sparse_amd import spspmm

    iA, _, iB, vB, want_index, want_value = _reference(dtype, "B")
    rng = np.random.default_rng(5)
    pA, pB = rng.permutation(iA.shape[1]), rng.permutation(iB.shape[1])
    index, value = spspmm(dev(iA[:, pA]), None, dev(iB[:, pB]), dev(vB[pB]), M_, K_, N_, coalesced=True)
    same_bits(index, want_index, "index")
    assert value.dtype == TORCH[dtype] and np.array_equal(host(value), want_value)
