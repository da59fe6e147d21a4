// What the robust-aggregation kernels share (robust.hip, and the q8 robust reduce of compress.hip): the sorting
// network, the element extraction and the bf16 rounding of the rule of ops/robust.py, and the launchers' dispatch
// on the padded peer count and their refusals. Device code is __forceinline__ helpers only: every kernel keeps its
// own body and its own algorithm.
//
// Not here, after a measurement: the selection itself (keys, thresholds), the loads of the live rows and the
// counters' way out of a workgroup. As shared helpers they changed the machine code of the trimmed, cclip and q8
// kernels, and rows of the A/B against the bodies written out came out slower than its spread allows
// (profiles/robust_refactor_ab.txt), so those kernels keep their own text.
#pragma once
#include "vcx_common.h"

#include <stdexcept>
#include <string>
#include <type_traits>

namespace vcx {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int TR_MAX_P = 16;
constexpr unsigned int TR_DEAD_KEY = 0xFFFFFFFFu;  // live keys stay below 2^24

// Batcher's odd-even merge sort over N = 2^k keys, ascending; fully unrolled.
template <int N>
__host__ __device__ __forceinline__ void tr_sort(unsigned int (&a)[N]) {
#pragma unroll
  for (int p = 1; p < N; p *= 2) {
#pragma unroll
    for (int k = p; k >= 1; k /= 2) {
#pragma unroll
      for (int j = k % p; j + k < N; j += 2 * k) {
#pragma unroll
        for (int i = 0; i < k; ++i) {
          const int x = i + j, y = i + j + k;
          if (y < N && x / (2 * p) == y / (2 * p)) {
            const unsigned int lo = a[x] < a[y] ? a[x] : a[y];
            const unsigned int hi = a[x] < a[y] ? a[y] : a[x];
            a[x] = lo;
            a[y] = hi;
          }
        }
      }
    }
  }
}

// fp32 pattern of element j (0..7) of a vector of 8 bf16
__device__ __forceinline__ unsigned int tr_elem(const u32x4& raw, int j) {
  return (j & 1) ? (raw[j >> 1] & 0xFFFF0000u) : (raw[j >> 1] << 16);
}

// bf16_rne(r) as a 16-bit pattern; a NaN is written as the canonical 0x7FC0
__device__ __forceinline__ unsigned int tr_bf16_bits(float r) {
  const bf16 h = (bf16)r;
  unsigned int hb = (unsigned int)__builtin_bit_cast(unsigned short, h);
  if (r != r) hb = 0x7FC0u;
  return hb;
}

// Host side. run(std::integral_constant<int, PP>) with PP = P padded to a power of two: the instantiation that
// takes a call of P rows (1 <= P <= 16).
template <class Run>
inline void for_padded_peers(int P, Run&& run) {
  if (P <= 2)
    run(std::integral_constant<int, 2>{});
  else if (P <= 4)
    run(std::integral_constant<int, 4>{});
  else if (P <= 8)
    run(std::integral_constant<int, 8>{});
  else
    run(std::integral_constant<int, 16>{});
}

inline void check_rows(const std::string& who, int P, uint32_t live_mask) {
  if (P < 1 || P > TR_MAX_P) throw std::invalid_argument(who + ": P must be in 1..16, got " + std::to_string(P));
  if (live_mask == 0 || (live_mask >> P) != 0)
    throw std::invalid_argument(who + ": live_mask must name at least one of the P rows and no other");
}

// f = min(trim, (K - 1) / 2) among K voters
inline int trim_of(int trim, int K) { return trim < (K - 1) / 2 ? trim : (K - 1) / 2; }

// the fp32 value of 1 / (K - 2f) as ops/robust.py trim_plan forms it: the double quotient, rounded once more
inline float trim_inv(int K, int f) { return (float)(1.0 / (double)(K - 2 * f)); }

}  // namespace vcx
