// Counter-based random stream shared by every sampler and walk: draw t of stream i under
// `seed` depends on (seed, i, t) only, so results do not depend on scheduling and a CPU
// restatement reproduces them bit for bit (oracle/sample_oracle.c restates it for sample_adj).
// Host and device: the `_host` exports run the very text the kernels run.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// Marks the plain-C++ text that kernels and `_host` exports share (weighted_pick.h,
// uniform_pick.h, search.h, temporal_pick.h, edge_lookup.h, node2vec_step.h, ppr_step.h).
// Everything under csrc/ is compiled by hipcc, so both halves always exist.
#define PSA_HD __host__ __device__ inline

namespace psa {

PSA_HD uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// High half of a 64 x 64 product: __umul64hi on the device, a 128-bit product on the host,
// the same integer.
PSA_HD uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return static_cast<uint64_t>((static_cast<unsigned __int128>(a) * b) >> 64);
#endif
}

// The per-stream part of randint, hoisted out of a loop over t.
PSA_HD uint64_t rand_stream(uint64_t seed, int64_t i) {
  return mix64(seed ^ mix64(static_cast<uint64_t>(i)));
}

// uniform integer in [0, n) of draw t of a stream: high half of a 64 x 64 product (n > 0)
PSA_HD int64_t rand_draw(uint64_t stream, int64_t t, int64_t n) {
  return static_cast<int64_t>(mulhi64(mix64(stream + static_cast<uint64_t>(t)), static_cast<uint64_t>(n)));
}

PSA_HD int64_t randint(uint64_t seed, int64_t i, int64_t t, int64_t n) {
  return rand_draw(rand_stream(seed, i), t, n);
}

}  // namespace psa
