"""The key families of tests/sort_cases.py have the properties their docstrings claim, the LSD model
equals the stable argsort on every one of them, and each gives the pass count it states.  CPU only:
this is what keeps a later edit from turning a family into uniform noise."""
import numpy as np
import pytest

import sort_cases as sc

TILES = (4096, 8192)
ALL = sc.CASES + sc.DIGIT_BOUNDARY_CASES


def _n(tile):
    return 3 * tile + 1


def _waves(keys):
    """The whole 64-key groups of the stream, one per row."""
    return keys[: keys.size // sc.WAVE * sc.WAVE].reshape(-1, sc.WAVE)


def _distinct_per_row(a):
    s = np.sort(a, axis=1)
    return 1 + (s[:, 1:] != s[:, :-1]).sum(1)


def _runs(keys):
    """(start, length, key) of every maximal run of equal neighbours."""
    cut = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    return cut, np.diff(np.concatenate([cut, [keys.size]])), keys[cut]


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_range_pass_count_and_model(case, tile):
    n = _n(tile)
    keys, max_value = case.make(n, tile, seed=1)
    assert keys.dtype == np.int64 and keys.shape == (n,)
    assert keys.min() >= 0 and int(keys.max()) < max_value
    assert sc.passes_for(max_value) == case.passes(n)
    again, _ = case.make(n, tile, seed=1)
    assert np.array_equal(keys, again)  # a seed names one stream
    ref = sc.stable_argsort(keys)
    assert np.array_equal(sc.lsd_model(keys, sc.bits_for(max_value)), ref)


def test_pass_count_steps_where_the_docstrings_say():
    assert [sc.passes_for(v) for v in (0, 1, 2, 255, 256, 257, 65535, 65536, 65537)] == [0, 0, 1, 1, 1, 2, 2, 2, 3]
    assert sc.passes_for((1 << 56) + 1) == 8 and sc.passes_for((1 << 63) - 1) == 8 and sc.passes_for(1 << 56) == 7
    names = [c.name for c in sc.DIGIT_BOUNDARY_CASES]
    assert len(names) == len(set(names)) == 22


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("p", [0, 1, 2])
@pytest.mark.parametrize("reverse", [False, True])
def test_one_bucket_per_tile(p, reverse, tile):
    n = _n(tile)
    keys, _ = sc.one_bucket_per_tile(n, tile, 0, p=p, reverse=reverse)
    t = np.arange(n) // tile
    for q in range(3):
        d = sc.digit(keys, q)
        for i in range(4):
            assert np.unique(d[t == i]).size == 1  # one bucket per tile, in every pass
        if q == p:
            assert np.array_equal(d, 255 - t % 256 if reverse else t % 256)
        else:
            assert np.unique(d).size == 1 and d[0] != 0
    # more than 256 tiles: the digit wraps, so a digit's look-back reaches 256 tiles back
    many, _ = sc.one_bucket_per_tile(300 * 64, 64, 0, p=p, reverse=reverse)
    assert np.unique(sc.digit(many, p)).size == 256 and sc.digit(many, p)[0] == sc.digit(many, p)[256 * 64]
    assert (np.diff(keys) < 0).any() == reverse  # only the reversed form needs a sort at this size


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("p", [0, 1, 2])
def test_all_but_one_pass_constant(p, tile):
    n = _n(tile)
    keys, _ = sc.all_but_one_pass_constant(n, tile, 3, p=p)
    for q in range(3):
        d = sc.digit(keys, q)
        if q == p:
            for i in range(3):  # 4096 draws from 256 digits miss one with probability 256 e^-16 < 1e-4
                assert np.unique(d[i * tile:(i + 1) * tile]).size == 256
        else:
            assert np.unique(d).size == 1 and d[0] != 0
    assert not np.array_equal(sc.stable_argsort(keys), np.arange(n))


@pytest.mark.parametrize("tile", TILES)
def test_descending_and_sawtooth(tile):
    n = _n(tile)
    keys, max_value = sc.descending(n, tile, 0)
    assert np.array_equal(keys, np.arange(n)[::-1]) and max_value == n
    assert (_distinct_per_row(sc.digit(_waves(keys), 0)) == 64).all()
    assert np.array_equal(sc.stable_argsort(keys), np.arange(n)[::-1])
    for period in (255, 256, 257):
        keys, max_value = sc.sawtooth(n, tile, 0, period=period)
        assert np.array_equal(keys, np.arange(n) % period) and max_value == period
        distinct = _distinct_per_row(sc.digit(_waves(keys), 0))
        # 256 and 0 share the digit 0 of pass 0: a wave that holds both has 63 distinct digits
        assert (distinct >= (64 if period <= 256 else 63)).all()
        assert (tile % period != 0) == (period != 256)  # 255 / 257: teeth drift against the tile
        assert int(keys.max()) == max_value - 1


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("length", [63, 64, 65])
def test_wave_runs(length, tile):
    n = _n(tile)
    keys, _ = sc.wave_runs(n, tile, 0, length=length)
    start, size, _ = _runs(keys)
    assert np.array_equal(start, np.arange(0, n, length))  # neighbouring runs never merge
    assert (size[:-1] == length).all() and size[-1] == n - start[-1]
    assert np.unique(keys).size == start.size  # runs hold distinct keys
    per_wave = _distinct_per_row(_waves(keys))
    if length == 64:
        assert (per_wave == 1).all()  # every wave one 64-lane peer set
    else:
        # runs straddle the waves: a boundary falls inside all but about one wave in 64
        assert per_wave.max() == 2 and (per_wave == 2).mean() > 0.95
        w = _waves(keys)
        assert ((w == w[:, :1]).sum(1) == 63).any()  # an almost-full peer set: 63 + 1
    for q in range(3):
        assert np.unique(sc.digit(keys, q)).size > 100  # scattered over the digits of every pass


@pytest.mark.parametrize("tile", TILES)
def test_runs_across_tiles(tile):
    n = 8 * tile + 1  # two complete runs and the beginning of a third
    keys, max_value = sc.runs_across_tiles(n, tile, 0)
    start, size, key = _runs(keys)
    long = size > 1
    want = np.arange(sc.RUN_START(tile), n, sc.RUN_PERIOD(tile))
    assert np.array_equal(start[long], want) and want.size == 3
    assert np.array_equal(size[long], np.minimum(sc.RUN_LENGTH(tile), n - want))
    assert (start[long] % tile != 0).all()  # a run starts inside a tile ...
    first, last = want[0], want[0] + sc.RUN_LENGTH(tile) - 1
    assert last // tile - first // tile == 3 and (last + 1) % tile != 0  # ... covers two whole ones, ends inside a fourth
    assert (key[long] % 2 == 0).all() and np.unique(key[long]).size == 3
    single = key[~long]
    assert (single % 2 == 1).all() and np.unique(single).size == single.size
    assert single.min() < key[long].min() and key[long].max() < single.max()  # the runs sort into the middle
    assert max_value == 2 * n + 2
    # the size the GPU tests use: one run from tile / 2 + 1 to the end
    keys, _ = sc.runs_across_tiles(_n(tile), tile, 0)
    start, size, _ = _runs(keys)
    assert start[size > 1].tolist() == [tile // 2 + 1] and size[size > 1].tolist() == [sc.RUN_LENGTH(tile)]


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", sc.DIGIT_BOUNDARY_CASES, ids=lambda c: c.name)
def test_digit_boundary(case, tile):
    n = _n(tile)
    keys, max_value = case.make(n, tile, seed=5)
    if "max_value" in case.params:
        assert max_value == (1 << 63) - 1
        edge = 1 << 56
    else:
        k, delta = case.params["k"], case.params["delta"]
        assert max_value == (1 << (8 * k)) + delta
        edge = 1 << (8 * k)
    present = set(np.unique(keys).tolist())
    for v in (0, 1, edge - 1, edge, max_value - 1):
        assert (v in present) == (v < max_value), v
    assert int(keys.max()) == max_value - 1 and int(keys.min()) == 0
    # the top digit of the largest key is what an off-by-one in the bit count loses
    top = sc.digit(np.array([max_value - 1]), case.passes(n) - 1)[0]
    assert top != 0
    assert np.unique(keys).size > min(max_value, 100) // 2  # the uniform half is there too
    last = sc.stable_argsort(keys)[-1]
    assert keys[last] == max_value - 1


@pytest.mark.parametrize("tile", TILES)
def test_zipf_matrix(tile):
    n = _n(tile)
    keys, max_value = sc.zipf_matrix(n, tile, 2)
    assert max_value == sc.ZIPF_M * sc.ZIPF_N
    row, col = keys // sc.ZIPF_N, keys % sc.ZIPF_N
    assert row.max() < sc.ZIPF_M
    # Zipf with exponent 1.3: P(first) = 1 / zeta(1.3) = 0.25
    assert (row == 0).mean() > 0.15 and (col == 0).mean() > 0.15
    assert np.unique(keys).size < 0.9 * n  # duplicates are common ...
    assert np.unique(keys).size > 0.2 * n  # ... and so are entries of their own
    top = np.bincount(sc.digit(keys, 2), minlength=256)
    assert top.max() > 0.15 * n and (top == 0).sum() < 128  # crowded top digit, long tail
    assert (np.diff(keys) < 0).any()


@pytest.mark.parametrize("tile", TILES)
def test_two_values(tile):
    n = _n(tile)
    lo, hi = sc.TWO_VALUES
    assert all(((lo >> s) & 255) != ((hi >> s) & 255) for s in (0, 8))
    keys, max_value = sc.two_values(n, tile, 0, by="lane")
    assert max_value == hi + 1 and set(np.unique(keys).tolist()) == {lo, hi}
    assert ((_waves(keys) == hi).sum(1) == 32).all()
    assert np.array_equal(keys[:4], [lo, hi, lo, hi])
    keys, _ = sc.two_values(n, tile, 0, by="wave")
    w = _waves(keys)
    assert (_distinct_per_row(w) == 1).all()
    assert np.array_equal(w[:, 0], np.where(np.arange(w.shape[0]) % 2 == 1, hi, lo))


def test_payload_bits():
    want = np.array(sc.PAYLOAD_SPECIALS, np.uint32).view(np.int32)
    for pattern in (0x7fc00001, 0x7f800001, 0xffc00000, 0x80000000, 0xffffffff, 0):
        assert pattern in sc.PAYLOAD_SPECIALS
    as_float = want.view(np.float32)
    assert np.isnan(as_float).sum() == 4 and (np.abs(as_float[~np.isnan(as_float)]) < np.finfo(np.float32).tiny).all()
    assert ((want.view(np.uint32) & 0x7f800000) == 0).sum() == 5  # +-0 and three denormals
    for n in (9, 10, 12289, 100000):
        pay = sc.payload_bits(n, seed=n)
        assert pay.dtype == np.int32 and pay.shape == (n,)
        assert np.isin(want, pay).all()
        assert np.array_equal(pay, sc.payload_bits(n, seed=n))
    for n in (0, 1, 5):
        assert np.array_equal(sc.payload_bits(n, 0), want[:n])
    assert np.unique(sc.payload_bits(100000, 1)).size > 99000


@pytest.mark.parametrize("first_bit", [1, 8, 20, 32, 40])
def test_lsd_model_on_a_bit_field(first_bit):
    rng = np.random.default_rng(first_bit)
    n, bits = 20000, 24
    hi = rng.integers(0, 1 << bits, n, dtype=np.int64)
    hi[::5] = hi[0]
    lo = rng.integers(0, 1 << first_bit, n, dtype=np.int64)
    keys = ((hi.astype(np.uint64) << np.uint64(first_bit)) | lo.astype(np.uint64)).view(np.int64)
    assert (first_bit + bits == 64) == bool((keys < 0).any())  # the field may reach bit 63
    assert np.array_equal(sc.lsd_model(keys, bits, first_bit), sc.stable_argsort(hi))
    # one pass too few is NOT the stable order: the model can tell a pass count from another
    assert not np.array_equal(sc.lsd_model(keys, bits - 8, first_bit), sc.stable_argsort(hi))
