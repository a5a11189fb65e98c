"""CPU suite: tests/bf16_ref.py against torch.Tensor.bfloat16() on the CPU."""
import numpy as np
import torch

import bf16_ref


def torch_round(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).bfloat16().float().numpy().astype(np.float64)


def same(a, b):
    ok = ~np.isnan(a)  # a NaN is a NaN, whatever its sign and payload
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a[ok]), np.signbit(b[ok]))


def from_bits(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def test_ties_go_to_even():
    # 1 + 2^-8 lies midway between 1 and 1 + 2^-7: down to the even 1; 1 + 3 * 2^-8 midway: up to 1 + 2^-6
    x = from_bits([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000])
    want = from_bits([0x3F800000, 0x3F820000, 0x3F810000, 0x3F800000, 0xBF800000, 0xBF820000]).astype(np.float64)
    assert same(bf16_ref.round_bf16(x), want) and same(torch_round(x), want)
    assert bf16_ref.round_bf16(np.float32(257.0)) == 256.0 and bf16_ref.round_bf16(np.float32(259.0)) == 260.0


def test_subnormals_infinities_nan_and_the_edge_of_overflow():
    x = from_bits([0x00000000, 0x80000000, 0x00000001, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x00800000,
                   0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF,
                   0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000, 0x7F7E8000])
    got, want = bf16_ref.round_bf16(x), torch_round(x)
    assert same(got, want)
    assert got[2] == 0 and got[3] == 0 and got[4] > 0          # half of the smallest bf16 subnormal: a tie to 0
    assert np.isinf(got[13]) and np.isinf(got[14]) and got[14] < 0 and np.isfinite(got[15]) and np.isinf(got[16])
    assert np.isnan(got[10:13]).all()


def test_every_rounding_position_of_random_bits():
    rng = np.random.default_rng(5)
    x = from_bits(rng.integers(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32))
    assert same(bf16_ref.round_bf16(x), torch_round(x))
    # all 2^16 lower halves under one upper half, and around a binade edge
    x = from_bits((np.uint32(0x3FFF0000) + np.arange(1 << 17, dtype=np.uint32)))
    assert same(bf16_ref.round_bf16(x), torch_round(x))


def test_is_bf16():
    assert bf16_ref.is_bf16(np.array([0.0, 1.75, -256.0, 255.0, 0.25])).all()
    assert not bf16_ref.is_bf16(np.array([257.0, 1.0 + 2.0 ** -9, 1e-50])).any()
