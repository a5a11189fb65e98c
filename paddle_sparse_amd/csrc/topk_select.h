// The steps of topk.hip, in plain C++ so that the host export psa_segment_topk_host runs the
// text the kernels run: the key mapping, the digit passes that give the threshold key T and
// the quota q of entries equal to T, and the ordered write.
//
// Every element maps to an unsigned key that preserves the value order (32 bits for fp32,
// fp16, bf16 and int32, 64 bits for fp64 and int64).  Every NaN, whatever its sign or
// payload, maps to the one greatest key; -0.0 and +0.0 map to one key; largest = false
// complements the key, so a selection only ever keeps the k GREATEST keys.  Entry j of a
// segment is kept iff
//   #{j' : key(j') > key(j)} + #{j' : key(j') == key(j), j' < j} < k
// (positions in segment order): exactly min(max(k, 0), len) entries, ties to the earlier
// position.
//
// A segment of up to kTopkShort entries counts that rank directly (topk_beats over all
// pairs).  A longer one finds (T, q) by an MSB-first radix select with 8-bit digits: every
// pass counts, in 256 counters, the digit of the entries whose higher digits equal those of
// the prefix found so far, walks the counters from the top to the digit that holds the
// k-th greatest entry (topk_pick_digit) and narrows (topk_narrow).  After the last pass the
// prefix is T and the remaining k is q >= 1; the write keeps key > T and the first q entries
// with key == T in position order (topk_keep).  Every loop is bounded by the segment length
// or the digit count.
#pragma once

#include <stdint.h>

#include "paddle_sparse_hip.h"
#include "weighted_pick.h"  // PSA_PICK_FN

namespace psa {

constexpr int kTopkShort = 64;    // entries: all-pairs rank in registers up to here
constexpr int kTopkLds = 4096;    // entries: keys staged in LDS up to here, streamed above
constexpr int kTopkGrid = 2048;   // workgroups of the long-segment kernel
constexpr int kTopkChunk = 256;   // segments one workgroup looks at per trip

template <int DT> struct TopkKey { using type = uint32_t; };
template <> struct TopkKey<PSA_F64> { using type = uint64_t; };
template <> struct TopkKey<PSA_I64> { using type = uint64_t; };

PSA_PICK_FN uint32_t topk_key_f32(uint32_t b) {
  if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;  // NaN: the greatest key
  if (b == 0x80000000u) b = 0u;                             // -0.0 is +0.0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

PSA_PICK_FN uint64_t topk_key_f64(uint64_t b) {
  if ((b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) return ~0ull;
  if (b == 0x8000000000000000ull) b = 0ull;
  return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}

// fp16 keeps its 16 bits in the low half of the key; only NaN has the high half set.
PSA_PICK_FN uint32_t topk_key_f16(uint32_t b) {
  if ((b & 0x7fffu) > 0x7c00u) return 0xffffffffu;
  if (b == 0x8000u) b = 0u;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}

// The key of value[i].  bf16 is the high half of an fp32 and maps as one.
template <int DT>
PSA_PICK_FN typename TopkKey<DT>::type topk_key(const void* value, int64_t i, bool smallest) {
  typename TopkKey<DT>::type key;
  if constexpr (DT == PSA_F32) key = topk_key_f32(static_cast<const uint32_t*>(value)[i]);
  else if constexpr (DT == PSA_F64) key = topk_key_f64(static_cast<const uint64_t*>(value)[i]);
  else if constexpr (DT == PSA_I32) key = static_cast<const uint32_t*>(value)[i] ^ 0x80000000u;
  else if constexpr (DT == PSA_I64) key = static_cast<const uint64_t*>(value)[i] ^ 0x8000000000000000ull;
  else if constexpr (DT == PSA_F16) key = topk_key_f16(static_cast<const uint16_t*>(value)[i]);
  else key = topk_key_f32(static_cast<uint32_t>(static_cast<const uint16_t*>(value)[i]) << 16);
  return smallest ? static_cast<typename TopkKey<DT>::type>(~key) : key;
}

// Does the entry (other, p2) come before the entry (key, p) in the kept order?
template <typename K>
PSA_PICK_FN bool topk_beats(K other, int p2, K key, int p) {
  return other > key || (other == key && p2 < p);
}

// Does `key` still match the prefix above the digit at `shift`?  (The first pass matches all.)
template <typename K>
PSA_PICK_FN bool topk_matches(K key, K prefix, int shift) {
  constexpr int kBits = static_cast<int>(sizeof(K)) * 8;
  return shift + 8 >= kBits || (key >> (shift + 8)) == (prefix >> (shift + 8));
}

template <typename K>
PSA_PICK_FN unsigned topk_digit(K key, int shift) {
  return static_cast<unsigned>(key >> shift) & 255u;
}

// The digit that holds the k-th greatest of the counted entries (1 <= k <= their total), and
// *above = the number of entries in greater digits.  The kernels run the same walk on 64
// lanes (topk.hip, pick_digit_wave): four counters per lane, a prefix sum over the lanes.
PSA_PICK_FN unsigned topk_pick_digit(const unsigned long long* hist, int64_t k, int64_t* above) {
  int64_t seen = 0;
  for (int d = 255; d > 0; --d) {
    const int64_t c = static_cast<int64_t>(hist[d]);
    if (seen + c >= k) {
      *above = seen;
      return static_cast<unsigned>(d);
    }
    seen += c;
  }
  *above = seen;
  return 0u;
}

// One pass done: the digit joins the prefix, the entries above it leave the count.
template <typename K>
PSA_PICK_FN void topk_narrow(K* prefix, int64_t* k, unsigned digit, int64_t above, int shift) {
  *prefix |= static_cast<K>(digit) << shift;
  *k -= above;
}

// The write: eq_before = the entries equal to T at earlier positions of the segment.
template <typename K>
PSA_PICK_FN uint8_t topk_keep(K key, K T, int64_t eq_before, int64_t q) {
  return (key > T || (key == T && eq_before < q)) ? 1 : 0;
}

PSA_PICK_FN bool topk_valid_segment(int64_t b, int64_t e, int64_t n) { return 0 <= b && b <= e && e <= n; }

}  // namespace psa
