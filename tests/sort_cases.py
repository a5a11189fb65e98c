"""Structured key streams for the radix sort tests, and the reference they are compared with.

Plain numpy: no GPU, no package import.  The reference of every sort test is
`np.argsort(keys, kind="stable")` (`stable_argsort`).

Uniform random keys give flat digit histograms: a tile of 4096 .. 16384 keys puts 16 .. 64 keys in each
of its 256 buckets, and the paths a real key stream takes (a tile with ONE digit, a look-back over
long chains of zero counts, a run of equal keys that spans tiles, a pass count that steps) are never
reached.  Each family below aims at one of them.  A family is a function

    family(n, tile, seed, ...) -> (keys int64[n], max_value)

with keys in [0, max_value); `tile` is the number of keys one workgroup of the sort under test takes
per pass (4096, 8192 or 16384 for the single-sweep passes, 10240 for the one-workgroup sort of the
small coalesce).  The sort runs `ceil(bits(max_value - 1) / 8)` passes of 8 bits (`passes_for`); every
docstring states the count its max_value gives, and `Case.passes` carries the same number for
tests/test_sort_cases.py, which also checks that each family has the property it claims, so that a
later edit cannot turn one into uniform noise.

`CASES` lists the fixed-parameter instances the GPU tests run (`Case.make(n, tile, seed)`),
`DIGIT_BOUNDARY_CASES` the 22 pass-count edges.
"""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Tuple

import numpy as np

WAVE = 64
RADIX_BITS = 8
RADIX = 1 << RADIX_BITS


# ---------------------------------------------------------------------------------------------
# reference and model
# ---------------------------------------------------------------------------------------------

def stable_argsort(keys: np.ndarray) -> np.ndarray:
    """THE reference: the stable sorting permutation of `keys`."""
    return np.argsort(keys, kind="stable")


def bits_for(max_value: int) -> int:
    """Bits needed for keys in [0, max_value): the bit length of max_value - 1 (0 for max_value <= 1)."""
    return int(max_value - 1).bit_length() if max_value > 1 else 0


def passes_for(max_value: int) -> int:
    """8-bit passes a sort bounded by max_value runs."""
    return (bits_for(max_value) + RADIX_BITS - 1) // RADIX_BITS


def digit(keys: np.ndarray, p: int, first_bit: int = 0) -> np.ndarray:
    """Digit of pass p: bits [first_bit + 8 p, first_bit + 8 p + 8) of the keys read as uint64."""
    return ((keys.astype(np.uint64) >> np.uint64(first_bit + RADIX_BITS * p)) & np.uint64(RADIX - 1)).astype(np.int64)


def lsd_model(keys: np.ndarray, bits: int, first_bit: int = 0) -> np.ndarray:
    """The permutation an 8-bit LSD radix sort of bits [first_bit, first_bit + bits) gives: one numpy
    stable argsort of one digit at a time, least significant first.  Equals `stable_argsort` of
    (keys >> first_bit) whenever that field fits in `bits` bits."""
    perm = np.arange(keys.size, dtype=np.int64)
    for p in range((bits + RADIX_BITS - 1) // RADIX_BITS):
        perm = perm[np.argsort(digit(keys[perm], p, first_bit), kind="stable")]
    return perm


# ---------------------------------------------------------------------------------------------
# payloads
# ---------------------------------------------------------------------------------------------

# quiet NaN with a payload, signalling NaN, negative quiet NaN, -0.0, all ones (a NaN), +0.0,
# the smallest and the largest positive denormal, a negative denormal
PAYLOAD_SPECIALS = (0x7fc00001, 0x7f800001, 0xffc00000, 0x80000000, 0xffffffff, 0x00000000,
                    0x00000001, 0x007fffff, 0x80000001)


def payload_bits(n: int, seed: int) -> np.ndarray:
    """int32[n] of opaque 32-bit patterns: random words with every pattern of PAYLOAD_SPECIALS at a
    random place (for n below their number, the first n of them).  A sort that moved its payload
    through a float register and canonicalised a NaN, flushed a denormal or dropped the sign of -0.0
    changes one of them; compare as int32 bits, never as floats."""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    special = np.array(PAYLOAD_SPECIALS, np.uint32)
    if n <= special.size:
        out[:] = special[:n]
    else:
        reps = min(n // special.size, 8)  # several copies: first, last and inner tiles all meet some
        where = rng.choice(n, reps * special.size, replace=False)
        out[where] = np.tile(special, reps)
    return out.view(np.int32)


# ---------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------

_FIXED_BYTES = (0x5a, 0xa5, 0x3c)  # the constant, non-zero digit of passes 0, 1, 2 where a family fixes one


def _fixed_except(p: int) -> int:
    return sum(b << (RADIX_BITS * q) for q, b in enumerate(_FIXED_BYTES) if q != p)


def one_bucket_per_tile(n: int, tile: int, seed: int, p: int = 0, reverse: bool = False) -> Tuple[np.ndarray, int]:
    """Tile t (keys [t * tile, (t + 1) * tile)) holds ONE key: digit t % 256 in pass p (255 - t % 256
    with `reverse`, so the input is not sorted already), the constants 0x5a / 0xa5 / 0x3c in the
    other two passes.  max_value = 2^24: 3 passes.

    Aims at: a tile whose keys share one digit (every wave a 64-lane peer set, in all three passes);
    in pass p a tile adds 0 to 255 of the 256 digits, so the look-back of a digit walks back over
    zero-count words to the tile 256 before; the order of the equal keys of a tile rests on the ranks
    alone."""
    t = (np.arange(n, dtype=np.int64) // tile) % RADIX
    d = (RADIX - 1 - t) if reverse else t
    return _fixed_except(p) + (d << (RADIX_BITS * p)), 1 << 24


def all_but_one_pass_constant(n: int, tile: int, seed: int, p: int = 0) -> Tuple[np.ndarray, int]:
    """A uniform random digit in pass p, the constants 0x5a / 0xa5 / 0x3c in the other two passes.
    max_value = 2^24: 3 passes.

    Aims at: the two passes that must be the identity — one bucket per tile, and any slip in their
    ranks or offsets destroys the order pass p made (p < 2) or shuffles its input (p > 0)."""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, RADIX, n, dtype=np.int64)
    return _fixed_except(p) + (d << (RADIX_BITS * p)), 1 << 24


def descending(n: int, tile: int, seed: int) -> Tuple[np.ndarray, int]:
    """n - 1, n - 2, ..., 0 with max_value = n: ceil(bits(n - 1) / 8) passes.

    Aims at: every wave of pass 0 sees 64 distinct digits (peer sets of one), every element moves,
    and the output of each tile is spread over every digit in reverse."""
    return np.arange(n - 1, -1, -1, dtype=np.int64), max(n, 1)


def sawtooth(n: int, tile: int, seed: int, period: int = 256) -> Tuple[np.ndarray, int]:
    """i % period with max_value = period: 1 pass for period 255 and 256, 2 passes for 257.

    Aims at: 64 distinct digits per wave while the rank bases of a digit grow item by item; with
    period 255 / 257 the teeth drift against the 64-lane waves and the tile, so a digit's run of
    ranks rolls over in the middle of a tile; 257 adds a second pass with two buckets (0 and 1)."""
    return np.arange(n, dtype=np.int64) % period, period


def _run_key(r: np.ndarray) -> np.ndarray:
    # r -> r * odd mod 2^24 is a bijection of [0, 2^24): distinct runs get distinct, scattered keys
    return (r * 0x9e3779) & 0xffffff


def wave_runs(n: int, tile: int, seed: int, length: int = 64) -> Tuple[np.ndarray, int]:
    """Runs of `length` equal keys; run r holds the key r * 0x9e3779 mod 2^24, so neighbouring runs
    differ and the runs are scattered over every digit of all 3 passes.  max_value = 2^24: 3 passes.

    Aims at: full 64-lane peer sets (length 64: every wave of the first pass is one run), almost full
    ones and a run that straddles two waves (63 and 65: peer sets of 63 + 1, 62 + 2, ...)."""
    return _run_key(np.arange(n, dtype=np.int64) // length), 1 << 24


def RUN_START(tile: int) -> int:  # the first run starts here ...
    return tile // 2 + 1


def RUN_LENGTH(tile: int) -> int:  # ... is this long ...
    return 5 * tile // 2


def RUN_PERIOD(tile: int) -> int:  # ... and the next one starts this much later
    return 7 * tile // 2


def runs_across_tiles(n: int, tile: int, seed: int) -> Tuple[np.ndarray, int]:
    """Distinct odd keys 2 * perm(i) + 1 (perm a random permutation of [0, n)) around runs of
    2.5 * tile equal keys: run j covers [tile / 2 + 1 + 3.5 j tile, + 2.5 tile) and holds the even key
    2 * (n / 2 + j), in the middle of the distinct ones.  max_value = 2 n + 2:
    ceil(bits(2 n + 1) / 8) passes.

    Aims at: stability across tile boundaries — a run starts in the middle of a tile, covers two
    whole tiles and ends inside a fourth, so the order of its elements rests on the look-back."""
    rng = np.random.default_rng(seed)
    keys = 2 * rng.permutation(n).astype(np.int64) + 1
    i = np.arange(n, dtype=np.int64) - RUN_START(tile)
    in_run = (i >= 0) & (i % RUN_PERIOD(tile) < RUN_LENGTH(tile))
    keys[in_run] = 2 * (n // 2 + i[in_run] // RUN_PERIOD(tile))
    return keys, 2 * n + 2


def digit_boundary_max(k: int, delta: int) -> int:
    return (1 << (RADIX_BITS * k)) + delta


def digit_boundary(n: int, tile: int, seed: int, k: int = 1, delta: int = 0, max_value: int = 0) -> Tuple[np.ndarray, int]:
    """max_value = 2^(8k) + delta (or the given max_value, for 2^63 - 1).  Half of the keys are drawn
    from {0, 1, 2^(8k) - 1, 2^(8k), max_value - 1} — those of them below max_value — the other half
    uniformly from [0, max_value); 0 and max_value - 1 are always present (n >= 2).
    Passes: k for delta = -1 and 0, k + 1 for delta = +1, 8 for max_value = 2^63 - 1.

    Aims at: the values where the pass count steps.  One pass too few leaves max_value - 1 (delta = +1:
    the only key with a non-zero top digit) out of place; the top digit of the largest key, 0xff or
    0x01, is where an off-by-one in the bit count shows; 2^63 - 1 runs all 8 passes."""
    if not max_value:
        max_value = digit_boundary_max(k, delta)
    else:
        k = (bits_for(max_value) + RADIX_BITS - 1) // RADIX_BITS - 1  # specials around the top digit's boundary
    rng = np.random.default_rng(seed)
    edge = 1 << (RADIX_BITS * k)
    special = np.array(sorted({v for v in (0, 1, edge - 1, edge, max_value - 1) if 0 <= v < max_value}), np.int64)
    keys = rng.integers(0, max_value, n, dtype=np.int64)
    pick = rng.random(n) < 0.5
    keys[pick] = special[rng.integers(0, special.size, int(pick.sum()))]
    if n >= 2:  # the two ends, at places that are neither first nor last when n allows
        a, b = rng.choice(n, 2, replace=False)
        keys[a], keys[b] = max_value - 1, 0
    return keys, max_value


ZIPF_M, ZIPF_N = 3000, 3001


def zipf_matrix(n: int, tile: int, seed: int, M: int = ZIPF_M, N: int = ZIPF_N) -> Tuple[np.ndarray, int]:
    """row * N + col of n entries of an M x N matrix whose rows and columns follow a Zipf law
    (exponent 1.3, folded into range), in arrival order, duplicates kept.  max_value = M * N
    (3000 x 3001: 24 bits, 3 passes).

    Aims at: the shape of a real COO stream — a few hub rows hold most entries, so the top digits are
    crowded into a few buckets while the low ones are near uniform, and equal keys are common."""
    rng = np.random.default_rng(seed)
    row = (rng.zipf(1.3, n) - 1) % M
    col = (rng.zipf(1.3, n) - 1) % N
    return row.astype(np.int64) * N + col.astype(np.int64), M * N


TWO_VALUES = (0x01ff, 0x0200)


def two_values(n: int, tile: int, seed: int, by: str = "lane") -> Tuple[np.ndarray, int]:
    """Only the keys 0x01ff and 0x0200, which differ in both digits: 0x0200 at odd positions
    (by="lane": lanes alternate, two peer sets of 32 in every wave) or in odd groups of 64
    (by="wave": every wave one 64-lane peer set, neighbouring waves in different buckets).
    max_value = 0x0201: 2 passes.

    Aims at: two buckets only — 254 zero counts per tile, half of the tile in each of the others."""
    i = np.arange(n, dtype=np.int64)
    odd = (i & 1) if by == "lane" else ((i // WAVE) & 1)
    lo, hi = TWO_VALUES
    return np.where(odd == 1, hi, lo).astype(np.int64), hi + 1


# ---------------------------------------------------------------------------------------------
# the instances the tests run
# ---------------------------------------------------------------------------------------------

class Case(NamedTuple):
    name: str
    family: Callable
    params: dict
    passes: Callable[[int], int]  # n -> the pass count the family's docstring states

    def make(self, n: int, tile: int, seed: int = 0) -> Tuple[np.ndarray, int]:
        return self.family(n, tile, seed, **self.params)


def _const(k: int) -> Callable[[int], int]:
    return lambda n: k


def _bytes_of(top: Callable[[int], int]) -> Callable[[int], int]:
    # passes for keys whose largest is top(n)
    return lambda n: (int(top(n)).bit_length() + RADIX_BITS - 1) // RADIX_BITS


CASES: List[Case] = (
    [Case(f"one_bucket_per_tile-p{p}", one_bucket_per_tile, {"p": p}, _const(3)) for p in range(3)]
    + [Case("one_bucket_per_tile-p1-reverse", one_bucket_per_tile, {"p": 1, "reverse": True}, _const(3))]
    + [Case(f"all_but_one_pass_constant-p{p}", all_but_one_pass_constant, {"p": p}, _const(3)) for p in range(3)]
    + [Case("descending", descending, {}, _bytes_of(lambda n: n - 1))]
    + [Case(f"sawtooth-{period}", sawtooth, {"period": period}, _const(2 if period > 256 else 1))
       for period in (255, 256, 257)]
    + [Case(f"wave_runs-{length}", wave_runs, {"length": length}, _const(3)) for length in (63, 64, 65)]
    + [Case("runs_across_tiles", runs_across_tiles, {}, _bytes_of(lambda n: 2 * n + 1))]
    + [Case("zipf_matrix", zipf_matrix, {}, _const(3))]
    + [Case(f"two_values-{by}", two_values, {"by": by}, _const(2)) for by in ("lane", "wave")]
)

DIGIT_BOUNDARY_CASES: List[Case] = (
    [Case(f"digit_boundary-k{k}{delta:+d}", digit_boundary, {"k": k, "delta": delta}, _const(k + (delta > 0)))
     for k in range(1, 8) for delta in (-1, 0, 1)]
    + [Case("digit_boundary-2^63-1", digit_boundary, {"max_value": (1 << 63) - 1}, _const(8))]
)


def case(name: str) -> Case:
    for c in CASES + DIGIT_BOUNDARY_CASES:
        if c.name == name:
            return c
    raise KeyError(name)
