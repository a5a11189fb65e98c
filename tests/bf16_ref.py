"""bfloat16 rounding in numpy: fp32 -> bf16 (round to nearest, ties to even) -> float64.  The bf16 GPU tests
round their float64 references with it; tests/test_bf16_ref.py holds it to torch.Tensor.bfloat16() on the CPU.

A bf16 is the upper 16 bits of an fp32, so the rounding is integer arithmetic on the bits: add 0x7fff plus the
lowest kept bit and drop the lower half.  A carry out of the fraction moves into the exponent, which is the
right answer (the next binade, or inf next to overflow); subnormals round like everything else; NaN stays NaN."""
import numpy as np


def round_bf16(x):
    """float64 array of the bf16 values nearest (ties to even) to the fp32 values of x."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    bits = x.view(np.uint32).astype(np.uint64)
    rounded = ((bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    with np.errstate(invalid="ignore"):  # a signalling NaN among the bits
        out = rounded.view(np.float32).astype(np.float64)
    out[np.isnan(x)] = np.nan
    return out


def is_bf16(x):
    """True where the float64 values of x are bf16 numbers already."""
    x = np.asarray(x, dtype=np.float64)
    x32 = x.astype(np.float32)
    return (x32.astype(np.float64) == x) & (round_bf16(x32) == x)
