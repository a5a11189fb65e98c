// Dropout of the attention weights, shared by both formats of attention_kernels.h.
//
//   T          = floor(dropout_p * 2^24)                        (in double; 0 <= T < 2^24)
//   r(e, h)    = mix64(rand_stream(seed, e) + h)                (rng.h; e = position of the entry in CSR order,
//                                                                h = absolute head index, uint64 wrap-around)
//   keep(e, h) = (r(e, h) >> 40) >= T
//   inv_keep   = float32(1 / (1 - dropout_p))
//
// The mask depends on (seed, e, h) only: not on head blocks, chunks, the load width, the dtype, or forward
// versus backward, and a host restatement reproduces it bit for bit (tests/dropout_ref.py).
#pragma once

#include "common.h"
#include "rng.h"

namespace psa {

struct Drop {
  uint64_t seed;
  uint32_t T;      // an entry is kept when the top 24 bits of its draw are at least T
  float inv_keep;
};

// keep(e, h) from the entry's stream = rand_stream(seed, e)
__host__ __device__ inline bool keep_of(uint64_t stream, int64_t h, uint32_t T) {
  return static_cast<uint32_t>(mix64(stream + static_cast<uint64_t>(h)) >> 40) >= T;
}

// false (and the error message set) unless 0 <= dropout_p < 1; a NaN fails both comparisons.
inline bool make_drop(const char* who, double dropout_p, uint64_t seed, Drop* d) {
  if (!(dropout_p >= 0.0 && dropout_p < 1.0)) {
    set_error(std::string(who) + ": dropout_p must be in [0, 1)");
    return false;
  }
  d->seed = seed;
  d->T = static_cast<uint32_t>(dropout_p * 16777216.0);  // < 2^24: the conversion truncates, as floor
  d->inv_keep = static_cast<float>(1.0 / (1.0 - dropout_p));
  return true;
}

}  // namespace psa
