// Coordinate-wise trimmed mean over the peers' copies of one shard (gfx950): the robust middle step
// of the direct all-reduce, next to reduce_bcast_bf16_kernel (optim.hip). Same bytes, same contract:
// P*n bf16 read, (P+1)*n written, 16 B per lane per access, `out` may alias `in`.
//
// The rule, per element position (ops/robust.py holds the torch definition; the two agree bit for bit):
//   * a bf16 pattern u has order key s = (u & 0x8000) ? (~u & 0xFFFF) : (u | 0x8000), ties go to the
//     row: key = (s << 8) | row. The order is total, -NaN < -Inf < ... < -0 < +0 < ... < +Inf < +NaN,
//     so a non-finite value is always an extreme. Rows outside `live` take a key above every live key.
//   * K = popcount(live), f = min(trim, (K - 1) / 2). Row k is kept iff its key lies between the
//     (f+1)-th smallest and the (f+1)-th largest live key, inclusive: K - 2f rows.
//   * result = bf16_rne((sum of the kept values) * inv): fp32 sum in ascending row order from +0, inv
//     the fp32 1 / (K - 2f) from the host, no fused multiply-add; a NaN result is written as 0x7FC0.
//   * counts[k] += 1 for every live row k that was not kept.
//
// Only the two threshold keys are needed, not the sorted values, because the sum runs in row order:
// a Batcher odd-even merge network sorts a copy of the keys (63 compare-exchanges at 16 rows), the
// thresholds are picked from it by a chain of wave-uniform selects, and each row compares its own key
// against them. Every array is indexed statically and stays in registers.
//
// No reference analog: the reference averages nothing.
#include "vcx_common.h"

#include <stdexcept>
#include <string>

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

// PP: P padded to a power of two; rows P..PP-1 are never read and never written.
template <int PP>
__global__ void __launch_bounds__(256) trimmed_reduce_bcast_bf16_kernel(const bf16* in, bf16* out, bf16* mine, int P,
                                                                        int64_t n8, int f, int K, unsigned int live,
                                                                        float inv,
                                                                        unsigned long long* __restrict__ counts) {
#pragma clang fp contract(off)
  __shared__ unsigned int wave_cnt[4][PP];
  const int64_t n = n8 * 8;
  unsigned int cnt[PP];  // rows of this thread's elements that were not kept (dead rows: dropped at the end)
#pragma unroll
  for (int k = 0; k < PP; ++k) cnt[k] = 0;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i * 8;
    u32x4 raw[PP];  // all live rows of these 8 elements are read before anything is written (out may alias in)
#pragma unroll
    for (int k = 0; k < PP; ++k) {
      raw[k] = u32x4{0u, 0u, 0u, 0u};
      if ((live >> k) & 1u) raw[k] = *(const u32x4*)(in + k * n + b);
    }
    u32x4 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // keys in the form (s << 16) | row: the order of (s << 8) | row, built from the fp32 pattern of the value
      // with wave-uniform masks (scalar registers) in place of per-row selects
      unsigned int val[PP], key[PP], srt[PP];
#pragma unroll
      for (int k = 0; k < PP; ++k) {
        val[k] = (j & 1) ? (raw[k][j >> 1] & 0xFFFF0000u) : (raw[k][j >> 1] << 16);
        const unsigned int neg = (unsigned int)((int)val[k] >> 31);         // all ones below zero
        const unsigned int s = val[k] ^ ((neg & 0xFFFF0000u) | 0x80000000u);  // order key in the high half
        const unsigned int dead = ((live >> k) & 1u) - 1u;                    // all ones for a dead row
        key[k] = s | (unsigned int)k | dead;
        srt[k] = key[k];
      }
      tr_sort<PP>(srt);
      unsigned int lo = 0u, hi = 0u;  // srt[f] and srt[K - 1 - f]: the dead keys sort behind the K live ones
#pragma unroll
      for (int k = 0; k < PP; ++k) {
        if (k < PP / 2) lo |= srt[k] & (0u - (unsigned int)(k == f));  // f <= (K - 1) / 2 < PP / 2
        hi |= srt[k] & (0u - (unsigned int)(k == K - 1 - f));
      }
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < PP; ++k) {
        const bool kept = key[k] >= lo && key[k] <= hi;
        t += kept ? __uint_as_float(val[k]) : 0.f;  // + (+0) leaves a sum that started at +0 unchanged
        cnt[k] += kept ? 0u : 1u;
      }
      const float r = t * inv;
      const bf16 h = (bf16)r;
      unsigned int hb = (unsigned int)__builtin_bit_cast(unsigned short, h);
      if (r != r) hb = 0x7FC0u;
      if (j & 1)
        o[j >> 1] |= hb << 16;
      else
        o[j >> 1] = hb;
    }
    if (out)
      for (int k = 0; k < P; ++k) *(u32x4*)(out + k * n + b) = o;
    if (mine) *(u32x4*)(mine + b) = o;
  }
  if (counts) {  // registers -> wave -> block (LDS) -> one global atomic per live row per block
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < PP; ++k) {
      unsigned int c = cnt[k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
      if (lane == 0) wave_cnt[wid][k] = c;
    }
    __syncthreads();
    if (threadIdx.x < PP && ((live >> threadIdx.x) & 1u)) {
      const unsigned int c = wave_cnt[0][threadIdx.x] + wave_cnt[1][threadIdx.x] + wave_cnt[2][threadIdx.x] +
                             wave_cnt[3][threadIdx.x];
      if (c) atomicAdd(counts + threadIdx.x, (unsigned long long)c);
    }
  }
}

}  // namespace vcx

using namespace vcx;

// A call the kernel cannot take raises before anything is launched.
void vcx_trimmed_reduce_bcast_bf16(const void* in, void* out, void* mine, int P, int64_t n, int trim,
                                   uint32_t live_mask, float inv, int64_t* counts, hipStream_t s) {
  const char* who = "trimmed_reduce_bcast_bf16";
  if (P < 1 || P > TR_MAX_P)
    throw std::invalid_argument(std::string(who) + ": P must be in 1..16, got " + std::to_string(P));
  if (live_mask == 0 || (P < 32 && (live_mask >> P) != 0))
    throw std::invalid_argument(std::string(who) + ": live_mask must name at least one of the P rows and no other");
  if (n < 0 || n % 8 != 0)
    throw std::invalid_argument(std::string(who) + ": n must be a multiple of 8, got " + std::to_string(n));
  if (trim < 0) throw std::invalid_argument(std::string(who) + ": trim must be >= 0");
  if (!in || ((uintptr_t)in & 15) || ((uintptr_t)out & 15) || ((uintptr_t)mine & 15))
    throw std::invalid_argument(std::string(who) + ": in, out and mine must be 16-byte aligned");
  if ((uintptr_t)counts & 7) throw std::invalid_argument(std::string(who) + ": counts must be 8-byte aligned");
  if (n == 0) return;
  const int K = __builtin_popcount(live_mask);
  const int f = trim < (K - 1) / 2 ? trim : (K - 1) / 2;
  const int64_t n8 = n / 8;
  const dim3 grid(stream_grid(n8, 256)), block(256);
  unsigned long long* c = (unsigned long long*)counts;
#define VCX_TR_LAUNCH(PP)                                                                                     \
  hipLaunchKernelGGL(trimmed_reduce_bcast_bf16_kernel<PP>, grid, block, 0, s, (const bf16*)in, (bf16*)out, \
                     (bf16*)mine, P, n8, f, K, live_mask, inv, c)
  if (P <= 2)
    VCX_TR_LAUNCH(2);
  else if (P <= 4)
    VCX_TR_LAUNCH(4);
  else if (P <= 8)
    VCX_TR_LAUNCH(8);
  else
    VCX_TR_LAUNCH(16);
#undef VCX_TR_LAUNCH
}
