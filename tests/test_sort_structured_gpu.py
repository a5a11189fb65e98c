"""The radix sort on the structured key streams of tests/sort_cases.py: single-bucket tiles, runs of
equal keys across waves and tiles, pass-count edges, every tile shape and the sizes where the
production rule changes shape — through index_sort, sort_pairs, sort_pairs_field and the routes
built on them (coalesce, the SparseStorage constructor, csr2csc).

Every comparison is exact, against np.argsort(kind="stable") (torch.sort(stable=True) for the one
33 M-key case); payloads are opaque 32-bit patterns (NaNs, -0.0, denormals) compared as int32 bits;
wherever a checked entry point exists the sort's fault word must read 0."""
import functools

import numpy as np
import pytest
import torch

import sort_cases as sc

pytestmark = pytest.mark.gpu

MID, STATUS_EDGE, HUGE = 1 << 19, 1 << 20, 1 << 25  # 1024x4 below MID, 512x16 from there, 1024x16 from HUGE


def production_tile(n):
    return 4096 if n < MID else 8192 if n < HUGE else 16384


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()  # a copy: the shared streams are read-only


def bits_of(t):
    """A 4-byte tensor as int32 patterns on the host."""
    return t.contiguous().view(torch.int32).cpu().numpy()


def run_heads(a):
    return int(1 + np.count_nonzero(a[1:] != a[:-1])) if a.size else 0


@functools.lru_cache(maxsize=6)
def stream(name, n, tile, seed=0):
    """(keys, max_value, stable argsort) of one case: computed once, shared, never written to."""
    keys, max_value = sc.case(name).make(n, tile, seed)
    ref = sc.stable_argsort(keys)
    keys.setflags(write=False)
    ref.setflags(write=False)
    return keys, max_value, ref


class sort_variant:
    """`with sort_variant(v):` runs the sorts inside with the tile shape / kernel family v and puts
    the previous one back."""

    def __init__(self, variant):
        self.variant = variant

    def __enter__(self):
        from paddle_sparse_amd import _lib

        self.prev = _lib.load().psa_sort_set_variant(self.variant) if self.variant is not None else None

    def __exit__(self, *exc):
        from paddle_sparse_amd import _lib

        if self.variant is not None:
            _lib.load().psa_sort_set_variant(self.prev)
        return False


def check_every_entry_point(keys, max_value, ref, seed=0):
    """index_sort (checked; permutation only; with the sorted keys and the scratch) and sort_pairs (fp32
    and int32 payload) against the stable argsort `ref`; fault words 0."""
    from paddle_sparse_amd import ops

    n = keys.size
    k = dev(keys)
    want_keys = keys[ref]
    distinct = run_heads(want_keys)
    srt, perm, status = ops.index_sort_checked(k, max_value)
    assert status == 0
    assert np.array_equal(perm.cpu().numpy(), ref)
    assert np.array_equal(srt.cpu().numpy(), want_keys)
    none, perm_only = ops.index_sort(k, max_value)
    assert none is None and np.array_equal(perm_only.cpu().numpy(), ref)
    srt, perm, scratch = ops.index_sort(k, max_value, with_sorted_inputs=True, keep_scratch=True)
    assert np.array_equal(perm.cpu().numpy(), ref) and np.array_equal(srt.cpu().numpy(), want_keys)
    # the count read raises if the fault word of that sort is set
    assert ops.unique_sorted(srt, 1, want_ptr=False, want_rowcol=False, after=scratch)[0] == distinct
    pay = sc.payload_bits(n, seed)
    for dtype in (torch.float32, torch.int32):
        skeys, spay, scratch = ops.sort_pairs(k, dev(pay).view(dtype), max_value, keep_scratch=True)
        assert spay.dtype == dtype
        assert np.array_equal(skeys.cpu().numpy(), want_keys)
        assert np.array_equal(bits_of(spay), pay[ref])
        assert ops.unique_sorted(skeys, 1, want_ptr=False, want_rowcol=False, after=scratch)[0] == distinct
    assert np.array_equal(k.cpu().numpy(), keys)  # the input is read only


# name, variant of psa_sort_set_variant (None: production rule), keys per tile, n
SHAPES = [
    ("production-1024x4", None, 4096, 3 * 4096 + 1),
    ("production-512x16", None, 8192, MID + 8193),
    ("forced-1024x8", 5, 8192, 3 * 8192 + 1),
    ("forced-1024x16", 6, 16384, 3 * 16384 + 1),
]
FAMILY_CASES = [c.name for c in sc.CASES] + ["digit_boundary-k2+1", "digit_boundary-2^63-1"]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s[0])
@pytest.mark.parametrize("name", FAMILY_CASES)
def test_every_family_in_every_tile_shape(name, shape):
    _, variant, tile, n = shape
    assert production_tile(n) == tile or variant is not None
    keys, max_value, ref = stream(name, n, tile)
    with sort_variant(variant):
        check_every_entry_point(keys, max_value, ref)


@pytest.mark.parametrize("variant,name,tile", [
    (1, "one_bucket_per_tile-p1-reverse", 4096), (2, "wave_runs-64", 4096), (3, "descending", 4096),
    (4, "sawtooth-257", 4096), (7, "runs_across_tiles", 8192)])
def test_three_launch_variants_on_one_family_each(variant, name, tile):
    keys, max_value, ref = stream(name, 3 * tile + 1, tile)
    with sort_variant(variant):
        check_every_entry_point(keys, max_value, ref)


# the smallest sizes that cross each edge: one wave, the 4096-key tile, the switch to 512 x 16 tiles at
# 2^19, the status-word area at 2^20, and k * 8192 -+ 1 behind it
SIZE_EDGES = [1, 63, 64, 65, 4095, 4096, 4097, MID - 1, MID, MID + 1, STATUS_EDGE - 1, STATUS_EDGE, STATUS_EDGE + 1,
              STATUS_EDGE + 8191, STATUS_EDGE + 8193]


@pytest.mark.parametrize("n", SIZE_EDGES)
@pytest.mark.parametrize("name", ["zipf_matrix", "runs_across_tiles"])
def test_size_edges_of_the_production_rule(name, n):
    keys, max_value, ref = stream(name, n, production_tile(n))
    check_every_entry_point(keys, max_value, ref, seed=n)


def _runs_across_tiles_on_device(n, tile, seed):
    """sort_cases.runs_across_tiles built with torch on the GPU (another permutation, the same runs)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    keys = 2 * torch.randperm(n, generator=g, device="cuda") + 1
    i = torch.arange(n, device="cuda") - sc.RUN_START(tile)
    in_run = (i >= 0) & (i % sc.RUN_PERIOD(tile) < sc.RUN_LENGTH(tile))
    return torch.where(in_run, 2 * (n // 2 + torch.div(i, sc.RUN_PERIOD(tile), rounding_mode="floor")), keys), 2 * n + 2


def test_device_built_runs_match_the_host_family():
    n, tile = 8 * 4096 + 1, 4096
    got, max_value = _runs_across_tiles_on_device(n, tile, 0)
    want, want_max = sc.runs_across_tiles(n, tile, 0)
    got = got.cpu().numpy()
    even = want % 2 == 0
    assert max_value == want_max and np.array_equal(got % 2 == 0, even) and np.array_equal(got[even], want[even])
    assert np.unique(got[~even]).size == np.count_nonzero(~even)


def test_runs_across_the_16384_key_tiles_of_the_huge_rule():
    """From 2^25 keys the production rule takes 1024 x 16 tiles: runs of 40 960 equal keys that start at
    8193 + 57 344 j, against torch's stable sort (a host argsort of 33 M keys is too slow for a test)."""
    from paddle_sparse_amd import ops

    n, tile = HUGE + 16385, 16384
    assert production_tile(n) == tile
    keys, max_value = _runs_across_tiles_on_device(n, tile, 1)
    s = sc.RUN_START(tile)
    assert int(keys[s]) == int(keys[s + sc.RUN_LENGTH(tile) - 1]) != int(keys[s - 1])
    out, perm, scratch = ops.index_sort(keys, max_value, with_sorted_inputs=True, keep_scratch=True)
    ref = torch.sort(keys, stable=True)
    assert torch.equal(out, ref.values) and torch.equal(perm, ref.indices)
    distinct = int(1 + (ref.values[1:] != ref.values[:-1]).sum())
    del ref
    assert ops.unique_sorted(out, 1, want_ptr=False, want_rowcol=False, after=scratch)[0] == distinct
    pay = torch.arange(n, dtype=torch.int32, device="cuda") ^ 0x7fc00000  # quiet-NaN patterns when read as fp32
    out2, pay2 = ops.sort_pairs(keys, pay.view(torch.float32), max_value)
    assert torch.equal(out2, out) and torch.equal((pay2.view(torch.int32) ^ 0x7fc00000).long(), perm)


@pytest.mark.parametrize("n", [20_000, MID + 5])
@pytest.mark.parametrize("name", [c.name for c in sc.DIGIT_BOUNDARY_CASES])
def test_digit_boundaries_of_max_value(name, n):
    """max_value = 2^(8k) - 1, 2^(8k), 2^(8k) + 1 (k = 1 .. 7) and 2^63 - 1: where the pass count steps.
    The largest key present is max_value - 1 and it lands last."""
    from paddle_sparse_amd import ops

    keys, max_value, ref = stream(name, n, production_tile(n), 7)
    assert int(keys.max()) == max_value - 1 and int(keys.min()) == 0
    check_every_entry_point(keys, max_value, ref, seed=n)
    srt, perm = ops.index_sort(dev(keys), max_value, with_sorted_inputs=True)
    assert int(srt[-1]) == max_value - 1 and int(srt[0]) == 0
    assert int(perm[-1]) == int(np.flatnonzero(keys == max_value - 1)[-1])  # the last of the largest: stable
    skeys, spay = ops.sort_pairs(dev(keys), torch.arange(n, dtype=torch.int32, device="cuda"), max_value)
    assert int(skeys[-1]) == max_value - 1 and int(spay[-1]) == int(perm[-1])


FIELD_BITS = 24  # every field source below has max_value = 2^24


def _field_keys(field, first_bit, low, seed):
    n = field.size
    if low == "ones":
        lo = np.full(n, (1 << first_bit) - 1, np.uint64)
    elif low == "zeros":
        lo = np.zeros(n, np.uint64)
    else:
        lo = np.random.default_rng(seed).integers(0, 1 << first_bit, n, dtype=np.uint64)
    return ((field.astype(np.uint64) << np.uint64(first_bit)) | lo).view(np.int64), lo


@pytest.mark.parametrize("n", [3 * 4096 + 1, MID + 8193])
@pytest.mark.parametrize("first_bit", [1, 8, 20, 32, 40])
@pytest.mark.parametrize("name", ["one_bucket_per_tile-p1-reverse", "wave_runs-64", "digit_boundary-k3+0"])
def test_sort_pairs_on_a_structured_bit_field(name, first_bit, n):
    """Order by (key >> first_bit) only.  The low bits — all ones next to fields of zeros, all zeros,
    random — come out unchanged and in input order within a field value; first_bit = 40 puts the 24-bit
    field at bits 40 .. 63 exactly; a field that would need bit 64 is refused."""
    from paddle_sparse_amd import ops

    field, max_value, ref = stream(name, n, production_tile(n))
    assert max_value == 1 << FIELD_BITS
    pay = sc.payload_bits(n, first_bit)
    for low in ("ones", "zeros", "random"):
        keys, lo = _field_keys(field, first_bit, low, n + first_bit)
        for dtype in (torch.float32, torch.int32):
            skeys, spay, scratch = ops.sort_pairs_field(dev(keys), dev(pay).view(dtype), first_bit, max_value,
                                                        keep_scratch=True)
            got = skeys.cpu().numpy()
            assert np.array_equal(got, keys[ref]), low
            assert np.array_equal(got.view(np.uint64) & np.uint64((1 << first_bit) - 1), lo[ref]), low
            assert np.array_equal(bits_of(spay), pay[ref]), low
            assert ops.unique_sorted(skeys, 1, want_ptr=False, want_rowcol=False, after=scratch)[0] == run_heads(keys[ref])
    # the widest field that still ends at bit 63 (max_value is an int64: 2^63 - 1 stands in for 2^63)
    widest = min(1 << (64 - first_bit), (1 << 63) - 1)
    assert first_bit + sc.bits_for(widest) == 64
    skeys, spay = ops.sort_pairs_field(dev(keys), dev(pay), first_bit, widest)
    assert np.array_equal(skeys.cpu().numpy(), keys[ref]) and np.array_equal(bits_of(spay), pay[ref])
    with pytest.raises(Exception):
        ops.sort_pairs_field(dev(keys), dev(pay), first_bit + 1, widest)
    with pytest.raises(Exception):
        ops.sort_pairs_field(dev(keys), dev(pay), 64, 1)


@pytest.mark.parametrize("n", [3 * 4096 + 1, MID + 8193])
def test_misaligned_and_strided_operands(n):
    """Keys that start 8 bytes into their buffer (not 16-byte aligned), a payload 4 bytes into its
    buffer, and strided views of both: sorted correctly or refused, never read as if contiguous."""
    from paddle_sparse_amd import ops

    keys, max_value, ref = stream("zipf_matrix", n, production_tile(n))
    pay = sc.payload_bits(n, 3)
    kbuf = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    kbuf[1:] = dev(keys)
    pbuf = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    pbuf[1:] = dev(pay)
    k, p = kbuf[1:], pbuf[1:]
    assert k.data_ptr() % 16 == 8 and p.data_ptr() % 8 == 4
    skeys, spay = ops.sort_pairs(k, p.view(torch.float32), max_value)
    assert np.array_equal(skeys.cpu().numpy(), keys[ref]) and np.array_equal(bits_of(spay), pay[ref])
    first_bit = 12
    fkeys = (keys << first_bit) | (np.arange(n) & 0xfff)
    kbuf[1:] = dev(fkeys)
    skeys, spay = ops.sort_pairs_field(k, p, first_bit, max_value)
    assert np.array_equal(skeys.cpu().numpy(), fkeys[ref]) and np.array_equal(bits_of(spay), pay[ref])

    wide = torch.full((2 * n,), -1, dtype=torch.int64, device="cuda")
    wide[::2] = dev(keys)
    pwide = torch.full((2 * n,), -1, dtype=torch.int32, device="cuda")
    pwide[::2] = dev(pay)
    ks, ps = wide[::2], pwide[::2]
    assert not ks.is_contiguous() and not ps.is_contiguous()
    calls = {
        "index_sort": lambda: ops.index_sort(ks, max_value, with_sorted_inputs=True),
        "sort_pairs": lambda: ops.sort_pairs(ks, ps, max_value),
        "sort_pairs_field": lambda: ops.sort_pairs_field(ks, ps, 0, max_value),
    }
    for who, call in calls.items():
        try:
            a, b = call()
        except (ValueError, TypeError, RuntimeError):
            continue  # refused: fine
        assert np.array_equal(a.cpu().numpy(), keys[ref]), who
        assert np.array_equal(b.cpu().numpy() if who == "index_sort" else bits_of(b), ref if who == "index_sort" else pay[ref]), who


# ---------------------------------------------------------------------------------------------
# the user-facing routes over the same streams
# ---------------------------------------------------------------------------------------------

ROUTE_N = sc.ZIPF_N  # columns of the matrix a key stream is read as: key = row * ROUTE_N + col
ONE_WORKGROUP = 10_240  # entries the one-workgroup LDS sort of the chain takes
CHAIN = 1 << 20  # entries the two-call chain takes; the sort_pairs route above


def _reduce_ref(inverse, count, value, op):
    """value reduced per distinct key (inverse: np.unique's) in float64, by ufunc.at."""
    ufunc, init = {"add": (np.add, 0.0), "min": (np.minimum, np.inf), "max": (np.maximum, -np.inf)}[op]
    out = np.full(count, init, np.float64)
    ufunc.at(out, inverse, value.astype(np.float64))
    return out


@pytest.mark.parametrize("n", [ONE_WORKGROUP - 1, ONE_WORKGROUP, ONE_WORKGROUP + 1, CHAIN - 1, CHAIN, CHAIN + 1])
@pytest.mark.parametrize("name", ["zipf_matrix", "runs_across_tiles", "one_bucket_per_tile-p1-reverse"])
def test_coalesce_storage_and_csr2csc_over_the_structured_streams(name, n):
    """coalesce(add / min / max), the SparseStorage constructor and csr2csc() on a stream read as
    (key // N, key % N): the one-workgroup sort and its limit (10 239 / 10 240 / 10 241 entries), the
    two-call chain with prepared histograms and the route above it (2^20 - 1 / 2^20 / 2^20 + 1).
    Values are integers in [-3, 3] with every |sum| below 2^24: exact in fp32 in any order."""
    from paddle_sparse_amd import SparseStorage, coalesce

    tile = 2048 if n <= ONE_WORKGROUP + 1 else production_tile(n)  # runs of 5120 inside the 10 240-entry tile
    keys, max_value, ref = stream(name, n, tile)
    N = ROUTE_N
    M = -(-max_value // N)
    row, col = keys // N, keys % N
    assert (np.diff(keys) < 0).any()  # unsorted: every route has to sort
    value = np.random.default_rng(n).integers(-3, 4, n).astype(np.float32)
    uniq, inverse = np.unique(keys, return_inverse=True)
    assert _reduce_ref(inverse, uniq.size, np.abs(value), "add").max() < float(1 << 24)  # as exact_ref.assert_exact_preconditions: sums exact in any order
    index = torch.stack([dev(row), dev(col)])
    for op in ("add", "min", "max"):
        want = _reduce_ref(inverse, uniq.size, value, op)
        out_index, out_value = coalesce(index, dev(value), M, N, op)
        assert np.array_equal(out_index.cpu().numpy(), np.stack([uniq // N, uniq % N])), op
        assert out_value.dtype == torch.float32
        assert np.array_equal(out_value.cpu().numpy(), want.astype(np.float32)), op
    out_index, none = coalesce(index, None, M, N)
    assert none is None and np.array_equal(out_index.cpu().numpy(), np.stack([uniq // N, uniq % N]))

    # the constructor sorts by (row, col) and keeps duplicates: np.lexsort, opaque value bits ride along
    pay = sc.payload_bits(n, n)
    order = np.lexsort((col, row))
    assert np.array_equal(order, ref)
    st = SparseStorage(row=dev(row), col=dev(col), value=dev(pay).view(torch.float32), sparse_sizes=(M, N))
    assert np.array_equal(st.row().cpu().numpy(), row[order]) and np.array_equal(st.col().cpu().numpy(), col[order])
    assert np.array_equal(bits_of(st.value()), pay[order])
    to_csc = st.csr2csc().cpu().numpy()
    assert np.array_equal(to_csc, np.lexsort((row[order], col[order])))
