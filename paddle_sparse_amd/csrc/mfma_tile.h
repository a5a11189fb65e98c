// The device text that typed_spmm.hip and basis_spmm.hip share: the tile constants their LDS strides are made of, 16-byte
// words of fp32 or bf16 elements, the fp32 <-> operand type conversions, one MFMA step group per operand type and the
// accumulator map of a 32 x 32 sub-tile.  Everything sits in the including file's anonymous namespace.  KS and Geo::LDH
// belong to typed_spmm.hip alone (Geo needs them here); basis_spmm.hip has a slab of its own, KB, and uses LD and LDW.
#pragma once

#include "common.h"

namespace {

constexpr int BM = 64;    // rows of a tile
constexpr int BK = 32;    // reduction step of the transform
constexpr int KS = 128;   // columns of x in one slab of H

typedef float v16f __attribute__((ext_vector_type(16)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));

template <typename T>
struct Geo {
  static constexpr int VPL = 16 / static_cast<int>(sizeof(T));  // elements of a 16-byte word
  static constexpr int LD = BK + VPL;                           // row stride of a weight tile
  static constexpr int LDH = KS + VPL;                          // row stride of H (forward)
  static constexpr int LDW = BM + VPL;                          // row stride of H^T and G^T (weight gradient)
};

template <typename T>
union Word {
  uint4 q;
  T e[16 / sizeof(T)];
};

// VPL elements from p, of which the first `valid` exist (<= 0: none; p is not read then)
template <typename T, bool VEC>
__device__ __forceinline__ uint4 load_word(const T* p, int64_t valid) {
  constexpr int VPL = Geo<T>::VPL;
  if constexpr (VEC) {
    return valid > 0 ? *reinterpret_cast<const uint4*>(p) : make_uint4(0, 0, 0, 0);
  } else {
    Word<T> w;
#pragma unroll
    for (int i = 0; i < VPL; ++i) w.e[i] = i < valid ? p[i] : T(0);
    return w.q;
  }
}

template <typename T>
__device__ __forceinline__ float widen(T v) {
  if constexpr (sizeof(T) == 4) return v;
  else return __uint_as_float(static_cast<uint32_t>(v) << 16);
}

// fp32 -> the operand / output type, one round to nearest even for bf16 (a NaN stays a quiet NaN)
template <typename T>
__device__ __forceinline__ T narrow(float f) {
  if constexpr (sizeof(T) == 4) {
    return f;
  } else {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return static_cast<uint16_t>((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return static_cast<uint16_t>(u >> 16);
  }
}

__device__ __forceinline__ v16f mfma(uint4 a, uint4 b, v16f acc, float) {
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
}

__device__ __forceinline__ v16f mfma(uint4 a, uint4 b, v16f acc, uint16_t) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), acc, 0, 0, 0);
}

// row of the 32 x 32 sub-tile that accumulator v of this lane holds (its column is lane % 32)
__device__ __forceinline__ int acc_row(int v) { return 8 * (v / 4) + 4 * ((threadIdx.x % 64) / 32) + v % 4; }

}  // namespace
