"""segment_topk restated in numpy (csrc/topk_select.h, include/paddle_sparse_hip.h), and the case
list that tests/test_zz_topk_ref.py runs through the host export and tests/test_zz_topk_gpu.py
through the kernels.

key_of maps every element to the unsigned key of the header: order-preserving, every NaN the one
greatest key, -0.0 == +0.0, complemented for largest=False.  topk_ref_loop is the rule as the
header words it, one segment at a time: keep = the first k of argsort(~key, kind="stable").
topk_ref is the same by two stable sorts over all entries at once (by ~key, then by segment), so
that a case of several hundred thousand segments costs no Python loop; test_zz_topk_ref.py holds
the two to each other.  bfloat16 travels as its bits in a uint16 array (numpy has no such type)
with bf16=True.

Nothing here imports the package: the numbers 64 / 4096 / 2048 / 256 are passed in by the tests
from ops.TOPK_SHORT / TOPK_LDS / TOPK_GRID / TOPK_CHUNK.
"""
import numpy as np

DTYPES = ("float32", "float64", "int32", "int64", "float16", "bfloat16")


def key_of(value, largest=True, bf16=False):
    value = np.ascontiguousarray(value)
    if bf16:
        assert value.dtype == np.uint16
        return key_of((value.astype(np.uint32) << 16).view(np.float32), largest)
    name = value.dtype.name
    if name in ("int32", "int64"):
        u = np.uint32 if name == "int32" else np.uint64
        key = value.view(u) ^ u(1 << (31 if name == "int32" else 63))
    elif name == "float16":
        b = value.view(np.uint16).astype(np.uint32)
        nan = (b & 0x7FFF) > 0x7C00
        b = np.where(b == 0x8000, np.uint32(0), b)
        key = np.where(b & 0x8000 != 0, ~b & np.uint32(0xFFFF), b | np.uint32(0x8000))
        key = np.where(nan, np.uint32(0xFFFFFFFF), key).astype(np.uint32)
    elif name in ("float32", "float64"):
        u, bits = (np.uint32, 32) if name == "float32" else (np.uint64, 64)
        sign, inf = u(1 << (bits - 1)), u(0x7F800000 if bits == 32 else 0x7FF0000000000000)
        b = value.view(u)
        nan = (b & ~sign) > inf
        b = np.where(b == sign, u(0), b)
        key = np.where(b & sign != 0, ~b, b | sign)
        key = np.where(nan, ~u(0), key).astype(u)
    else:
        raise TypeError(name)
    return key if largest else ~key


def _valid(indptr, n):
    b, e = indptr[:-1], indptr[1:]
    return (0 <= b) & (b <= e) & (e <= n)


def _k_of(k, nseg):
    return np.full(nseg, k, np.int64) if isinstance(k, int) else np.asarray(k, np.int64)


def topk_ref_loop(value, indptr, k, perm=None, largest=True, out=None, bf16=False):
    key = key_of(value, largest, bf16)
    indptr = np.asarray(indptr, np.int64)
    n, nseg = key.size, indptr.size - 1
    keep = np.zeros(n, np.uint8) if out is None else out
    ks, ok = _k_of(k, nseg), _valid(indptr, n)
    for s in range(nseg):
        if not ok[s]:
            continue
        j = np.arange(indptr[s], indptr[s + 1])
        at = j if perm is None else np.asarray(perm)[j]
        order = np.argsort(~key[at], kind="stable")
        keep[at] = 0
        keep[at[order[:max(int(ks[s]), 0)]]] = 1
    return keep


def topk_ref(value, indptr, k, perm=None, largest=True, out=None, bf16=False):
    key = key_of(value, largest, bf16)
    indptr = np.asarray(indptr, np.int64)
    n, nseg = key.size, indptr.size - 1
    keep = np.zeros(n, np.uint8) if out is None else out
    ok = _valid(indptr, n)
    begin, length, ks = indptr[:-1][ok], (indptr[1:] - indptr[:-1])[ok], _k_of(k, nseg)[ok]
    total = int(length.sum())
    if total == 0:
        return keep
    first = np.cumsum(length) - length  # of every valid segment among the covered positions
    seg = np.repeat(np.arange(length.size), length)
    j = np.arange(total) - np.repeat(first, length) + np.repeat(begin, length)
    at = j if perm is None else np.asarray(perm)[j]
    order = np.argsort(~key[at], kind="stable")
    order = order[np.argsort(seg[order], kind="stable")]  # by (segment, ~key, position)
    rank = np.arange(total) - np.repeat(first, length)
    keep[at[order]] = (rank < np.repeat(ks, length)).astype(np.uint8)
    return keep


# ---- the case list ---------------------------------------------------------------------------

def as_dtype(x, dtype):
    """float64 / int64 numbers -> (array, bf16 flag) of the named dtype."""
    if dtype == "bfloat16":
        return (np.asarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16), True
    return np.asarray(x).astype(dtype), False


def ptr_of(lengths):
    return np.concatenate(([0], np.cumsum(np.asarray(lengths, np.int64)))).astype(np.int64)


def tied(rng, n, dtype):
    """n numbers with heavy ties, both signs and, for the floats, NaN, +-inf, +-0 and a denormal."""
    x = rng.integers(-6, 7, n).astype(np.float64)
    if dtype in ("int32", "int64"):
        return as_dtype(x.astype(np.int64), dtype)
    if n >= 8:
        spots = rng.integers(0, n, max(n // 8, 6))
        x[spots] = rng.choice([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 6e-8, -6e-8], spots.size)
    return as_dtype(x, dtype)


K_SHORT = ("0", "1", "2", "len-1", "len", "len+1", "short", "short+1")
K_LONG = ("1", "2", "255", "256", "257", "len-1", "len", "len+1")


def k_named(name, lengths, short):
    lengths = np.asarray(lengths, np.int64)
    if name.startswith("len"):
        return lengths + int(name[3:] or 0)
    return {"short": short, "short+1": short + 1}.get(name) if name.startswith("short") else int(name)


def short_lengths(width, short):
    """Every length 0 .. short + 1, then empty segments until the mean length selects the group
    width `width` (8: mean <= 8, 16: <= 16, 32: <= 32, 64: above)."""
    lengths = list(range(short + 2))
    total = sum(lengths)
    if width < 64:
        lengths += [0] * (-(-total // width) - len(lengths))
    mean = -(-total // len(lengths))
    assert (width == 64 and mean > 32) or (width // 2 < mean <= width) or (width == 8 and mean <= 8)
    return lengths


def long_lengths(short, lds):
    return [short + 1, 255, 256, 257, 511, 513, lds - 1, lds, lds + 1, 3 * lds + 17]


def case(value, bf16, lengths, k, largest=True, perm=None, indptr=None):
    return dict(value=value, bf16=bf16, indptr=ptr_of(lengths) if indptr is None else indptr, k=k, largest=largest,
                perm=perm)


def regime_cases(short, lds):
    """name -> case: the short regime at every group width and the LDS / stream lengths, every k of
    the lists above, both directions."""
    rng = np.random.default_rng(7)
    out = {}
    for width in (8, 16, 32, 64):
        lengths = short_lengths(width, short)
        value, bf16 = tied(rng, sum(lengths), "float32")
        for kn in K_SHORT:
            for largest in (True, False):
                out[f"short-w{width}-k{kn}-{'max' if largest else 'min'}"] = case(
                    value, bf16, lengths, k_named(kn, lengths, short), largest)
    lengths = long_lengths(short, lds)
    for dtype in ("float32", "float64"):
        value, bf16 = tied(rng, sum(lengths), dtype)
        for kn in K_LONG:
            for largest in (True, False):
                out[f"long-{dtype}-k{kn}-{'max' if largest else 'min'}"] = case(
                    value, bf16, lengths, k_named(kn, lengths, short), largest)
    return out


def mixed_lengths(short, lds):
    return [0, 1, 5, short, short + 1, 0, 300, 9, lds + 1, 2, lds, 33]


def dtype_cases(short, lds):
    """Every dtype over short, LDS and stream segments at once: scalar k, per-segment k with zeros,
    negatives and values above the length, a random perm, both directions."""
    rng = np.random.default_rng(11)
    lengths = mixed_lengths(short, lds)
    n = sum(lengths)
    out = {}
    for dtype in DTYPES:
        value, bf16 = tied(rng, n, dtype)
        k_seg = np.array([rng.integers(-2, ln + 4) for ln in lengths], np.int64)
        k_seg[[4, 6]] = [0, -3]
        perm = rng.permutation(n).astype(np.int64)
        for largest in (True, False):
            d = "max" if largest else "min"
            out[f"{dtype}-k3-{d}"] = case(value, bf16, lengths, 3, largest)
            out[f"{dtype}-k257-{d}"] = case(value, bf16, lengths, 257, largest)
            out[f"{dtype}-kseg-{d}"] = case(value, bf16, lengths, k_seg, largest)
            out[f"{dtype}-kseg-perm-{d}"] = case(value, bf16, lengths, k_seg, largest, perm)
    return out


def _three(pattern, short, lds):
    """The generator pattern(n) -> float64 / int64 numbers at a short, an LDS and a stream length."""
    lengths = [short - 24, 300, lds + 4]
    return np.concatenate([pattern(n) for n in lengths]), lengths


def _one_byte(rng, n, nbytes, byte):
    """Integers of nbytes bytes that differ in byte `byte` alone (every other byte is 0x01); the top
    byte runs through the sign."""
    base = sum(1 << (8 * b) for b in range(nbytes) if b != byte)
    u = (rng.integers(0, 256, n).astype(np.uint64) << np.uint64(8 * byte)) | np.uint64(base)
    return u.astype(np.uint32).view(np.int32).astype(np.int64) if nbytes == 4 else u.view(np.int64)


def structured_cases(short, lds):
    rng = np.random.default_rng(13)
    out = {}

    def add(name, numbers, lengths, k, dtypes, largest=(True, False)):
        for dtype in dtypes:
            value, bf16 = as_dtype(numbers, dtype)
            for lg in largest:
                out[f"{name}-{dtype}-{'max' if lg else 'min'}"] = case(value, bf16, lengths, k, lg)

    x, lengths = _three(lambda n: np.full(n, 2.5), short, lds)
    add("all-equal", x, lengths, 7, ("float32", "float64", "float16"))
    add("all-equal-i", x.astype(np.int64), lengths, 7, ("int32", "int64"))
    for dtype, nbytes in (("int32", 4), ("int64", 8)):
        for byte in range(nbytes):
            x, lengths = _three(lambda n: _one_byte(rng, n, nbytes, byte), short, lds)
            add(f"byte{byte}", x, lengths, 9, (dtype,))
            add(f"byte{byte}-k200", x, lengths, np.array([9, 200, 200], np.int64), (dtype,))
    # two distinct values: c entries of the greater one, k on either side of c
    lengths = [40, 300, lds + 4]
    counts = [11, 120, 1700]
    x = np.concatenate([rng.permutation(np.r_[np.full(c, 3.0), np.full(n - c, -1.0)]) for n, c in zip(lengths, counts)])
    for off in (-1, 0, 1):
        add(f"two-values-c{off:+d}", x, lengths, np.array(counts, np.int64) + off, ("float32", "int64", "bfloat16"))
    # g entries above the threshold, m equal to it: quota 1 (k = g + 1) and quota m - 1 (k = g + m - 1)
    g, m = [5, 40, 900], [9, 77, 1300]
    x = np.concatenate([rng.permutation(np.r_[rng.integers(10, 99, gi), np.full(mi, 4), rng.integers(-50, 4, n - gi - mi)])
                        for n, gi, mi in zip(lengths, g, m)]).astype(np.float64)
    add("quota-1", x, lengths, np.array(g, np.int64) + 1, ("float32", "float64", "int32"), (True,))
    add("quota-m-1", x, lengths, np.array(g, np.int64) + np.array(m, np.int64) - 1, ("float32", "float64", "int32"),
        (True,))
    floats = ("float32", "float64", "float16", "bfloat16")
    x, lengths = _three(lambda n: np.full(n, np.nan), short, lds)
    add("all-nan", x, lengths, 6, floats)
    x, lengths = _three(lambda n: rng.choice([np.nan, -np.nan, np.inf, -np.inf, 1.0, -1.0], n), short, lds)
    for k in (2, 150):
        add(f"nan-inf-k{k}", x, lengths, k, floats)
    x, lengths = _three(lambda n: rng.choice([0.0, -0.0], n), short, lds)
    add("zeros", x, lengths, 5, floats)
    x, lengths = _three(lambda n: rng.choice([0.0, -0.0, 1.0, -1.0], n), short, lds)
    add("zeros-ones", x, lengths, np.array([13, 100, 1500], np.int64), floats)
    for dtype, tiny in (("float32", 1.4e-45), ("float64", 4.9e-324), ("float16", 6e-8), ("bfloat16", 9.2e-41)):
        x, lengths = _three(lambda n: rng.integers(-3, 4, n) * tiny, short, lds)
        add("denormals", x, lengths, np.array([7, 100, 1500], np.int64), (dtype,))
    for dtype in ("int32", "int64"):
        info = np.iinfo(dtype)
        x, lengths = _three(lambda n: rng.choice(np.array([info.min, -1, 0, info.max], np.int64), n), short, lds)
        add("int-limits", x, lengths, np.array([11, 100, 2000], np.int64), (dtype,))
    for dtype, big in (("float16", 65504.0), ("bfloat16", 3.3895313892515355e38)):
        x, lengths = _three(lambda n: rng.choice([big, -big, np.inf, -np.inf, 1.0, 0.0], n), short, lds)
        add("half-extremes", x, lengths, np.array([9, 100, 1400], np.int64), (dtype,))
    return out


def pointer_cases(short, lds):
    """Pointers that leave a head and a tail uncovered, and segments with bounds outside the arrays."""
    rng = np.random.default_rng(17)
    out = {}
    n = 6 + 30 + (short + 6) + (lds + 9) + 11
    value, bf16 = tied(rng, n, "float32")
    indptr = np.array([6, 36, 36 + short + 6, 36 + short + 6 + lds + 9], np.int64)
    assert indptr[0] > 0 and indptr[-1] < n
    perm = rng.permutation(n).astype(np.int64)
    for largest in (True, False):
        d = "max" if largest else "min"
        out[f"head-tail-{d}"] = case(value, bf16, None, 4, largest, indptr=indptr)
        out[f"head-tail-perm-{d}"] = case(value, bf16, None, 4, largest, perm, indptr=indptr)
    # segment 0 begins below 0, 2 ends beyond n, 3 begins there, 5 runs backwards: 1 (short) and 4 (long) are valid
    s = 9 + short + 2
    indptr = np.array([-1, 9, s, n + 2, s + 20, s + 400, s + 350], np.int64)
    out["invalid-segments"] = case(value, bf16, None, 5, True, indptr=indptr)
    return out


def all_cases(short, lds):
    out = {}
    for group in (regime_cases, dtype_cases, structured_cases, pointer_cases):
        out.update(group(short, lds))
    return out
