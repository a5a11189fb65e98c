// Counter-based random stream shared by sample_adj (sample.hip) and random_walk
// (walk.hip): draw t of stream i under `seed` depends on (seed, i, t) only, so
// results do not depend on scheduling and a CPU restatement reproduces them bit
// for bit (oracle/sample_oracle.c restates it for sample_adj).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace psa {

__host__ __device__ inline uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// The per-stream part of randint, hoisted out of a loop over t.
__host__ __device__ inline uint64_t rand_stream(uint64_t seed, int64_t i) {
  return mix64(seed ^ mix64(static_cast<uint64_t>(i)));
}

// uniform integer in [0, n) of draw t of a stream: high half of a 64 x 64 product (n > 0)
__device__ inline int64_t rand_draw(uint64_t stream, int64_t t, int64_t n) {
  const uint64_t r = mix64(stream + static_cast<uint64_t>(t));
  return static_cast<int64_t>(__umul64hi(r, static_cast<uint64_t>(n)));
}

__device__ inline int64_t randint(uint64_t seed, int64_t i, int64_t t, int64_t n) {
  return rand_draw(rand_stream(seed, i), t, n);
}

}  // namespace psa
