// Helpers shared by the row kernels (attention_kernels.h, spmm_heads_half.hip): a lane's VEC elements of a
// two-byte operand widened to fp32 on load and rounded once on store, fp32 loads and stores of the same shape (the
// fp32 operands of attention and the fp32 partials of the long-row chunks), and the two small host / device
// utilities the plans use.
#pragma once

#include "half_util.h"

namespace psa_half {

typedef uint16_t elem_t;  // the two bytes of an operand element; T (the format tag) says which format

// VEC = 8: one 16-byte load (p 16-byte aligned); VEC = 1: one 2-byte load
template <typename T, int VEC>
__device__ __forceinline__ void load_vec(const elem_t* p, float (&dst)[VEC]) {
  if constexpr (VEC == 8) {
    widen8<T>(*reinterpret_cast<const uint4*>(p), dst);
  } else {
    dst[0] = widen1<T>(p, 0);
  }
}

// the one rounding of a result
template <typename T, int VEC>
__device__ __forceinline__ void store_vec(elem_t* p, const float (&src)[VEC]) {
  if constexpr (VEC == 8) {
    *reinterpret_cast<uint4*>(p) = narrow8<T>(src);
  } else {
    *p = narrow1<T>(src[0]);
  }
}

// fp32 operands, and the fp32 partials of the long-row chunks whatever the operands are (VEC = 4: one 16-byte
// access, VEC = 8: two)
template <int VEC>
__device__ __forceinline__ void load_f32(const float* p, float (&dst)[VEC]) {
  if constexpr (VEC == 8) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    dst[0] = a.x, dst[1] = a.y, dst[2] = a.z, dst[3] = a.w;
    dst[4] = b.x, dst[5] = b.y, dst[6] = b.z, dst[7] = b.w;
  } else if constexpr (VEC == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    dst[0] = v.x, dst[1] = v.y, dst[2] = v.z, dst[3] = v.w;
  } else {
    dst[0] = *p;
  }
}

template <int VEC>
__device__ __forceinline__ void store_f32(float* p, const float (&src)[VEC]) {
  if constexpr (VEC == 8) {
    *reinterpret_cast<float4*>(p) = make_float4(src[0], src[1], src[2], src[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(src[4], src[5], src[6], src[7]);
  } else if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(src[0], src[1], src[2], src[3]);
  } else {
    *p = src[0];
  }
}

__device__ __forceinline__ void clamp_range(int64_t& s, int64_t& e, int64_t nnz) {
  s = s < 0 ? 0 : s;
  e = e > nnz ? nnz : e;  // never past the arrays, whatever rowptr holds
}

// the power of two >= min(n, cap) and its log2
inline int pow2_at_least(int64_t n, int cap, int* shift) {
  int p = 1;
  *shift = 0;
  while (p < cap && p < n) {
    p <<= 1;
    ++*shift;
  }
  return p;
}

}  // namespace psa_half
