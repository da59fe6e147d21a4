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
// against them. Every array is indexed statically and stays in registers. The sorting network and what else the
// cclip kernels below and the q8 robust reduce (compress.hip) use as well are in robust_common.h.
//
// No reference analog: the reference averages nothing.
#include "robust_common.h"

namespace vcx {

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
      // (the value is extracted inline, not by tr_elem: through the helper PP = 16 compiles to other machine code)
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
      const unsigned int hb = tr_bf16_bits(t * inv);
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


// ---------------------------------------------------------------------------------------------------------------
// Centered clipping (cclip): the per-peer rule next to the coordinate-wise one. ops/robust.py holds the definition
// and the torch reference; these kernels agree with it bit for bit. In short, over the live rows x_i of one shard:
//   v = float(median rule's result); L times: D_i = sum_j (x_i[j] - v[j])^2 in the fixed order below,
//   d_i = sqrt(D_i), w_i = d_i <= tau ? 1 : tau / d_i (0 for a non-finite D_i; tau = 0: the (K-1)/2-th smallest
//   d_i), v += (sum_i w_i (x_i - v)) * inv_K; result = bf16_rne(v).
// The order of a distance depends on n only. A chunk is 4096 elements = 512 vectors of 8; thread t of the 256 adds
// the squares of vector t, then of vector 256 + t, in ascending element order from +0 (a vector past the end adds
// nothing: the sums are never -0). The 256 thread sums are combined pairwise over adjacent indices: the xor
// butterfly inside a wave (an IEEE add commutes, so both lanes of a pair hold lower + higher), then (w0 + w1) +
// (w2 + w3). Workgroups stride over whole chunks and write one partial per row and chunk, so nothing depends on the
// grid; the weights kernel adds the partials in ascending chunk order. 2L + 1 launches on one stream: init,
// L x (weights, step). No atomics, no fused multiply-add.
constexpr int CC_CHUNK_VEC = 512;      // vectors of 8 elements per chunk
constexpr int CC_MAX_BLOCKS = 256 * 8;  // workgroup cap of the init and step passes: more chunks are strided over
constexpr int CC_MAX_ITERS = 8;
constexpr int CC_TILE = 512;  // chunk partials per row staged in LDS by the weights kernel

__device__ __forceinline__ bool cc_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// The trimmed kernel's rule on one element position (val: the rows' fp32 patterns): (sum of the kept) * inv.
template <int PP>
__device__ __forceinline__ float cc_trimmed(const unsigned int (&val)[PP], int f, int K, unsigned int live, float inv) {
#pragma clang fp contract(off)
  unsigned int key[PP], srt[PP];
#pragma unroll
  for (int k = 0; k < PP; ++k) {
    const unsigned int neg = (unsigned int)((int)val[k] >> 31);
    const unsigned int s = val[k] ^ ((neg & 0xFFFF0000u) | 0x80000000u);
    const unsigned int dead = ((live >> k) & 1u) - 1u;
    key[k] = s | (unsigned int)k | dead;
    srt[k] = key[k];
  }
  tr_sort<PP>(srt);
  unsigned int lo = 0u, hi = 0u;
#pragma unroll
  for (int k = 0; k < PP; ++k) {
    if (k < PP / 2) lo |= srt[k] & (0u - (unsigned int)(k == f));
    hi |= srt[k] & (0u - (unsigned int)(k == K - 1 - f));
  }
  float t = 0.f;
#pragma unroll
  for (int k = 0; k < PP; ++k) t += (key[k] >= lo && key[k] <= hi) ? __uint_as_float(val[k]) : 0.f;
  return t * inv;
}

// The 256 thread sums s[k] of one chunk -> part[k * nchunks + c], for every live row k.
template <int PP>
__device__ __forceinline__ void cc_chunk_sum(float (&s)[PP], float (*wave_part)[PP], float* __restrict__ part,
                                             int64_t nchunks, int64_t c, unsigned int live) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < PP; ++k) {
    float a = s[k];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) a = a + __shfl_xor(a, o, 64);
    if (lane == 0) wave_part[wid][k] = a;
  }
  __syncthreads();
  if (threadIdx.x < PP && ((live >> threadIdx.x) & 1u)) {
    const int k = threadIdx.x;
    part[k * nchunks + c] = (wave_part[0][k] + wave_part[1][k]) + (wave_part[2][k] + wave_part[3][k]);
  }
  __syncthreads();  // wave_part is written again in the next chunk
}

// Init pass: v = float(median rule's result) and the chunk partials of the first distances.
template <int PP>
__global__ void __launch_bounds__(256) cclip_init_kernel(const bf16* __restrict__ in, float* __restrict__ v,
                                                         float* __restrict__ part, int64_t n8, int64_t nchunks, int f,
                                                         int K, unsigned int live, float inv) {
#pragma clang fp contract(off)
  __shared__ float wave_part[4][PP];
  const int64_t n = n8 * 8;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    float s[PP];
#pragma unroll
    for (int k = 0; k < PP; ++k) s[k] = 0.f;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      const int64_t i = c * CC_CHUNK_VEC + h * 256 + threadIdx.x;
      if (i >= n8) continue;
      const int64_t b = i * 8;
      u32x4 raw[PP];
#pragma unroll
      for (int k = 0; k < PP; ++k) {
        raw[k] = u32x4{0u, 0u, 0u, 0u};
        if ((live >> k) & 1u) raw[k] = *(const u32x4*)(in + k * n + b);
      }
      float vv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        unsigned int val[PP];
#pragma unroll
        for (int k = 0; k < PP; ++k) val[k] = tr_elem(raw[k], j);
        const float r = cc_trimmed<PP>(val, f, K, live, inv);
        const float c0 = __uint_as_float(tr_bf16_bits(r) << 16);  // the median rule's bf16 result, as fp32
        vv[j] = c0;
        const bool fin = cc_finite(c0);
#pragma unroll
        for (int k = 0; k < PP; ++k) {
          const float e = fin ? __uint_as_float(val[k]) - c0 : 0.f;
          if ((live >> k) & 1u) s[k] = s[k] + e * e;
        }
      }
      *(f32x4*)(v + b) = f32x4{vv[0], vv[1], vv[2], vv[3]};
      *(f32x4*)(v + b + 4) = f32x4{vv[4], vv[5], vv[6], vv[7]};
    }
    cc_chunk_sum<PP>(s, wave_part, part, nchunks, c, live);
  }
}

// Weights: D_k = the row's chunk partials added in ascending order from +0, d = sqrt(D), tau, w. One workgroup: all
// threads stage the partials through LDS (the next tile's loads are in flight while thread k adds row k's tile).
template <int PP>
__global__ void __launch_bounds__(256) cclip_weights_kernel(const float* __restrict__ part, int64_t nchunks, int P,
                                                            int K, unsigned int live, float tau,
                                                            float* __restrict__ w, float* __restrict__ w_user) {
#pragma clang fp contract(off)
  __shared__ float tile[PP][CC_TILE + 1];
  __shared__ unsigned int dkey[PP];
  const int tid = threadIdx.x;
  float nxt[PP][CC_TILE / 256];
  auto fetch = [&](int64_t base) {
#pragma unroll
    for (int k = 0; k < PP; ++k)
#pragma unroll
      for (int u = 0; u < CC_TILE / 256; ++u) {
        const int64_t c = base + tid + 256 * u;
        nxt[k][u] = (((live >> k) & 1u) && c < nchunks) ? part[k * nchunks + c] : 0.f;
      }
  };
  fetch(0);
  float D = 0.f;
  for (int64_t base = 0; base < nchunks; base += CC_TILE) {
#pragma unroll
    for (int k = 0; k < PP; ++k)
#pragma unroll
      for (int u = 0; u < CC_TILE / 256; ++u) tile[k][tid + 256 * u] = nxt[k][u];
    __syncthreads();
    if (base + CC_TILE < nchunks) fetch(base + CC_TILE);
    if (tid < PP) {
      const int cnt = nchunks - base < CC_TILE ? (int)(nchunks - base) : CC_TILE;
      for (int i = 0; i < cnt; ++i) D = D + tile[tid][i];
    }
    __syncthreads();
  }
  const bool alive = tid < PP && ((live >> tid) & 1u);
  const bool fin = alive && cc_finite(D);
  const float d = fin ? sqrtf(D) : 0.f;
  // d >= +0: the fp32 patterns order like the values; a non-finite distance counts as +Inf, a dead row sorts behind
  if (tid < PP) dkey[tid] = alive ? (fin ? __float_as_uint(d) : 0x7F800000u) : TR_DEAD_KEY;
  __syncthreads();
  if (tid < P) {
    float t = tau;
    if (!(tau > 0.f)) {
      unsigned int srt[PP];
#pragma unroll
      for (int k = 0; k < PP; ++k) srt[k] = dkey[k];
      tr_sort<PP>(srt);
      unsigned int pick = 0u;
#pragma unroll
      for (int k = 0; k < PP / 2; ++k) pick |= srt[k] & (0u - (unsigned int)(k == (K - 1) / 2));  // (K-1)/2 < PP/2
      t = __uint_as_float(pick);
    }
    const float wk = fin ? (d <= t ? 1.f : t / d) : 0.f;
    w[tid] = wk;
    if (w_user) w_user[tid] = wk;
  }
}

// Step pass: v += (sum over the live rows with w > 0, ascending, of w (x - v)) * inv_K where v is finite. Not LAST:
// v is written back and the next distances' chunk partials come from the rows still in registers. LAST: the bf16
// result goes to every row of out and to mine.
template <int PP, bool LAST>
__global__ void __launch_bounds__(256) cclip_step_kernel(const bf16* in, bf16* out, bf16* mine, float* __restrict__ v,
                                                         const float* __restrict__ w, float* __restrict__ part, int P,
                                                         int64_t n8, int64_t nchunks, unsigned int live, float inv_k) {
#pragma clang fp contract(off)
  __shared__ float wave_part[4][PP];
  const int64_t n = n8 * 8;
  float wk[PP];
  unsigned int use = 0u;  // live rows with a weight above zero: the others are skipped, never multiplied
#pragma unroll
  for (int k = 0; k < PP; ++k) {
    wk[k] = (k < P && ((live >> k) & 1u)) ? w[k] : 0.f;
    if (wk[k] > 0.f) use |= 1u << k;
  }
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    float s[PP];
#pragma unroll
    for (int k = 0; k < PP; ++k) s[k] = 0.f;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      const int64_t i = c * CC_CHUNK_VEC + h * 256 + threadIdx.x;
      if (i >= n8) continue;
      const int64_t b = i * 8;
      u32x4 raw[PP];  // all live rows of these 8 elements are read before anything is written (out may alias in)
#pragma unroll
      for (int k = 0; k < PP; ++k) {
        raw[k] = u32x4{0u, 0u, 0u, 0u};
        if ((live >> k) & 1u) raw[k] = *(const u32x4*)(in + k * n + b);
      }
      const f32x4 v0 = *(const f32x4*)(v + b), v1 = *(const f32x4*)(v + b + 4);
      float vv[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      u32x4 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float c0 = vv[j];
        float x[PP];
#pragma unroll
        for (int k = 0; k < PP; ++k) x[k] = __uint_as_float(tr_elem(raw[k], j));
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < PP; ++k) {
          const float term = wk[k] * (x[k] - c0);
          t = ((use >> k) & 1u) ? t + term : t;
        }
        const float c1 = cc_finite(c0) ? c0 + t * inv_k : c0;
        vv[j] = c1;
        if (LAST) {
          const unsigned int hb = tr_bf16_bits(c1);
          if (j & 1)
            o[j >> 1] |= hb << 16;
          else
            o[j >> 1] = hb;
        } else {
          const bool fin = cc_finite(c1);
#pragma unroll
          for (int k = 0; k < PP; ++k) {
            const float e = fin ? x[k] - c1 : 0.f;
            if ((live >> k) & 1u) s[k] = s[k] + e * e;
          }
        }
      }
      if (LAST) {
        if (out)
          for (int k = 0; k < P; ++k) *(u32x4*)(out + k * n + b) = o;
        if (mine) *(u32x4*)(mine + b) = o;
      } else {
        *(f32x4*)(v + b) = f32x4{vv[0], vv[1], vv[2], vv[3]};
        *(f32x4*)(v + b + 4) = f32x4{vv[4], vv[5], vv[6], vv[7]};
      }
    }
    if (!LAST) cc_chunk_sum<PP>(s, wave_part, part, nchunks, c, live);
  }
}

// One voter: its row, unchanged, to every row of out and to mine; its weight is 1.
__global__ void __launch_bounds__(256) cclip_one_voter_kernel(const bf16* in, bf16* out, bf16* mine, int P, int64_t n8,
                                                              int row, float* __restrict__ w_user) {
  const int64_t n = n8 * 8;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    const u32x4 o = *(const u32x4*)(in + row * n + i * 8);
    if (out)
      for (int k = 0; k < P; ++k) *(u32x4*)(out + k * n + i * 8) = o;
    if (mine) *(u32x4*)(mine + i * 8) = o;
  }
  if (w_user && blockIdx.x == 0 && threadIdx.x < P) w_user[threadIdx.x] = (int)threadIdx.x == row ? 1.f : 0.f;
}

}  // namespace vcx

using namespace vcx;

// A call the kernel cannot take raises before anything is launched.
void vcx_trimmed_reduce_bcast_bf16(const void* in, void* out, void* mine, int P, int64_t n, int trim,
                                   uint32_t live_mask, float inv, int64_t* counts, hipStream_t s) {
  const std::string who = "trimmed_reduce_bcast_bf16";
  check_rows(who, P, live_mask);
  if (n < 0 || n % 8 != 0) throw std::invalid_argument(who + ": n must be a multiple of 8, got " + std::to_string(n));
  if (trim < 0) throw std::invalid_argument(who + ": trim must be >= 0");
  if (!in || ((uintptr_t)in & 15) || ((uintptr_t)out & 15) || ((uintptr_t)mine & 15))
    throw std::invalid_argument(who + ": in, out and mine must be 16-byte aligned");
  if ((uintptr_t)counts & 7) throw std::invalid_argument(who + ": counts must be 8-byte aligned");
  if (n == 0) return;
  const int K = __builtin_popcount(live_mask), f = trim_of(trim, K);
  const int64_t n8 = n / 8;
  const dim3 grid(stream_grid(n8, 256)), block(256);
  for_padded_peers(P, [&](auto pp) {
    hipLaunchKernelGGL(trimmed_reduce_bcast_bf16_kernel<decltype(pp)::value>, grid, block, 0, s, (const bf16*)in,
                       (bf16*)out, (bf16*)mine, P, n8, f, K, live_mask, inv, (unsigned long long*)counts);
  });
}


int vcx_cclip_max_workgroups() { return CC_MAX_BLOCKS; }

// The weights launch alone: the q8 centered clipping of compress.hip writes partials of the same layout.
void vcx_cclip_weights(const float* part, int64_t nchunks, int P, uint32_t live_mask, float tau, float* w,
                       float* w_user, hipStream_t s) {
  const int K = __builtin_popcount(live_mask);
  for_padded_peers(P, [&](auto pp) {
    hipLaunchKernelGGL(cclip_weights_kernel<decltype(pp)::value>, dim3(1), dim3(256), 0, s, part, nchunks, P, K,
                       live_mask, tau, w, w_user);
  });
}

int64_t vcx_cclip_workspace_floats(int P, int64_t n) {
  const int64_t nchunks = (n / 8 + CC_CHUNK_VEC - 1) / CC_CHUNK_VEC;
  return n + (int64_t)P * nchunks + TR_MAX_P;
}

// A call the kernels cannot take raises before anything is launched.
void vcx_cclip_reduce_bcast_bf16(const void* in, void* out, void* mine, int P, int64_t n, uint32_t live_mask, float tau,
                                 int iters, float* weights, float* workspace, hipStream_t s) {
  const std::string who = "cclip_reduce_bcast_bf16";
  check_rows(who, P, live_mask);
  if (n < 0 || n % 8 != 0) throw std::invalid_argument(who + ": n must be a multiple of 8, got " + std::to_string(n));
  if (!(tau >= 0.f) || tau > 3.402823466e38f)
    throw std::invalid_argument(who + ": tau must be finite and >= 0 (0: adaptive)");
  if (iters < 1 || iters > CC_MAX_ITERS)
    throw std::invalid_argument(who + ": iters must be in 1..8, got " + std::to_string(iters));
  if (!in || ((uintptr_t)in & 15) || ((uintptr_t)out & 15) || ((uintptr_t)mine & 15))
    throw std::invalid_argument(who + ": in, out and mine must be 16-byte aligned");
  if (!workspace || ((uintptr_t)workspace & 15))
    throw std::invalid_argument(who + ": workspace must be 16-byte aligned");
  if ((uintptr_t)weights & 3) throw std::invalid_argument(who + ": weights must be 4-byte aligned");
  if (n == 0) return;
  const int K = __builtin_popcount(live_mask);
  const int64_t n8 = n / 8;
  if (K == 1) {
    hipLaunchKernelGGL(cclip_one_voter_kernel, dim3(stream_grid(n8, 256)), dim3(256), 0, s, (const bf16*)in,
                       (bf16*)out, (bf16*)mine, P, n8, __builtin_ctz(live_mask), weights);
    return;
  }
  const int f = trim_of(TR_MAX_P, K);  // the median rule is the start: all the trim that K voters allow
  const float inv = trim_inv(K, f), inv_k = trim_inv(K, 0);
  const int64_t nchunks = (n8 + CC_CHUNK_VEC - 1) / CC_CHUNK_VEC;
  float* v = workspace;
  float* part = v + n;
  float* w = part + (int64_t)P * nchunks;
  const dim3 grid((unsigned int)(nchunks < CC_MAX_BLOCKS ? nchunks : CC_MAX_BLOCKS)), block(256);
  for_padded_peers(P, [&](auto pp) {
    constexpr int PP = decltype(pp)::value;
    hipLaunchKernelGGL(cclip_init_kernel<PP>, grid, block, 0, s, (const bf16*)in, v, part, n8, nchunks, f, K,
                       live_mask, inv);
    for (int l = 0; l < iters; ++l) {
      const bool last = l == iters - 1;
      hipLaunchKernelGGL(cclip_weights_kernel<PP>, dim3(1), block, 0, s, part, nchunks, P, K, live_mask, tau, w,
                         last ? weights : (float*)nullptr);
      if (last)
        hipLaunchKernelGGL((cclip_step_kernel<PP, true>), grid, block, 0, s, (const bf16*)in, (bf16*)out,
                           (bf16*)mine, v, w, part, P, n8, nchunks, live_mask, inv_k);
      else
        hipLaunchKernelGGL((cclip_step_kernel<PP, false>), grid, block, 0, s, (const bf16*)in, (bf16*)out,
                           (bf16*)mine, v, w, part, P, n8, nchunks, live_mask, inv_k);
    }
  });
}
