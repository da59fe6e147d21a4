// Gradient / pseudo-gradient compression kernels (gfx950): exact top-k with error feedback
// and PowerSGD rank-r with error feedback. No reference analog (BASELINE.json
// configs 3 and 5).
//
// Top-k: the k-th largest |g + e| is found EXACTLY by a 3-pass radix select on the IEEE bit
// pattern of |x| (monotonic for non-negative floats): 12 + 12 + 7 bits. Pass 1 (fused with the
// error-feedback accumulation) is a per-block LDS histogram of the top 12 bits; passes 2 and 3
// read x again and histogram ONLY the elements inside the chosen bin (a few per mille); a
// 1-block scan after each pass narrows the prefix. All state stays on the device (no host sync; graph-capturable). Selection then
// compacts the winners: elements above the threshold fill the output from the front, ties with
// it from the back, both claimed with ONE 64-bit atomic per 16k elements.
//
// HBM traffic per element: 10 B (accumulate: g 2 + e 4 read, e 4 written) + 2 x 4 B (passes 2,
// 3) + 4 B (select) = 22 B.
//
// PowerSGD (Vogels et al. 2019): M <- g + e; P = M Q; allreduce(P); P = orth(P);
// Q = M^T P; allreduce(Q); out = P Q^T; e = M - out. For rank r <= 8 the two products are
// HBM-bound (2r FLOP per 4-B element), so they are single-pass streaming kernels with the
// small Q/P operands served from L2; all matrices of a model are processed by ONE launch per
// stage through a device-side descriptor table (grouped kernels).
//
// q8: 8-bit quantisation in blocks of 128 with one fp32 scale each and error feedback: three
// streaming kernels (encode, reduce on the shard owner, decode), described at their section below,
// and the robust reduce (the trimmed mean of ops/robust.py over the decoded records) that takes the
// place of the rank-order sum under --aggregate trimmed | median, and under --aggregate cclip (on request) the
// centered clipping of the decoded records: an init pass, then a weights launch and a step pass per update.
#include "robust_common.h"
#include "vcx_api.h"

namespace vcx {

// =====================================================================================
// top-k
// =====================================================================================
// state layout (int32): [0] prefix bits, [1] remaining k (after the last pass: the tie budget),
//                       [3] threshold bits, [6..7] 64-bit output claim counter (above | ties << 32)
constexpr int TK_BINS = 4096;

__device__ __forceinline__ uint32_t absbits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// acc = g + e (written to e, fp32), histogram pass 1 of |acc| (bits 30..19 -> 12 bits).
// 8 elements per lane per step (one 16-B g load for bf16, two 16-B e loads/stores).
template <typename GT>
__device__ __forceinline__ void load8(const GT* __restrict__ g, int64_t i, float (&a)[8]) {
  if constexpr (sizeof(GT) == 2) {
    const bf16x8 v = *(const bf16x8*)(g + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = (float)v[j];
  } else {
    const f32x4 u = *(const f32x4*)(g + i), w = *(const f32x4*)(g + i + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] = u[j];
      a[j + 4] = w[j];
    }
  }
}

template <typename GT>
__global__ void __launch_bounds__(256) topk_accum_hist_kernel(const GT* __restrict__ g, float* __restrict__ e,
                                                               int64_t n, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[TK_BINS];
  for (int i = threadIdx.x; i < TK_BINS; i += 256) h[i] = 0;
  __syncthreads();
  const bool vec = ((((uintptr_t)g) | ((uintptr_t)e)) & 15) == 0;
  const int64_t n8 = vec ? n / 8 : 0;
  for (int64_t v = blockIdx.x * 256ll + threadIdx.x; v < n8; v += (int64_t)gridDim.x * 256) {
    float a[8];
    load8(g, v * 8, a);
    f32x4 e0 = *(const f32x4*)(e + v * 8), e1 = *(const f32x4*)(e + v * 8 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      e0[j] += a[j];
      e1[j] += a[j + 4];
    }
    *(f32x4*)(e + v * 8) = e0;
    *(f32x4*)(e + v * 8 + 4) = e1;
    // per-lane LDS atomics: same-bin lanes serialise inside the LDS, which costs far less than a
    // ballot-leader loop over the ~30 distinct bins of a wave's gradient values
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      atomicAdd(&h[absbits(e0[j]) >> 19], 1u);
      atomicAdd(&h[absbits(e1[j]) >> 19], 1u);
    }
  }
  for (int64_t i = n8 * 8 + blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float a = (float)g[i] + e[i];
    e[i] = a;
    atomicAdd(&h[absbits(a) >> 19], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TK_BINS; i += 256)
    if (h[i]) atomicAdd(&hist[i], h[i]);
}

// passes 2 and 3: histogram of the next bit field (`nbits` bits at `shift`) over the elements
// whose higher bits equal the current prefix. Only those few per mille take part: a per-lane
// LDS atomic each, one global atomic per nonzero bin per block at the end.
__global__ void __launch_bounds__(256) topk_hist_kernel(const float* __restrict__ x, int64_t n,
                                                         const int* __restrict__ st, int shift_hi, int shift,
                                                         int nbits, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[TK_BINS];
  const int nb = 1 << nbits;
  for (int i = threadIdx.x; i < nb; i += 256) h[i] = 0;
  __syncthreads();
  const uint32_t prefix = (uint32_t)st[0];
  const bool vec = (((uintptr_t)x) & 15) == 0;
  const int64_t n8 = vec ? n / 8 : 0;
  for (int64_t v = blockIdx.x * 256ll + threadIdx.x; v < n8; v += (int64_t)gridDim.x * 256) {
    const f32x4 a = *(const f32x4*)(x + v * 8), b = *(const f32x4*)(x + v * 8 + 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t u = absbits(j < 4 ? a[j] : b[j - 4]);
      if ((u >> shift_hi) == prefix) atomicAdd(&h[(u >> shift) & (nb - 1)], 1u);
    }
  }
  for (int64_t i = n8 * 8 + blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint32_t u = absbits(x[i]);
    if ((u >> shift_hi) == prefix) atomicAdd(&h[(u >> shift) & (nb - 1)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += 256)
    if (h[i]) atomicAdd(&hist[i], h[i]);
}

// one block of T threads: find the bin (from the top) where the cumulative count reaches the
// remaining k; extend the prefix by it; update remaining k. Thread t owns the t-th chunk of
// nb / T bins counted from the top; a block scan of the chunk sums finds the one chunk where the
// count crosses, and only that thread walks its bins. `hist` is re-zeroed by the launcher.
// (A 19-bit second pass into a global histogram was tried: bf16 gradients put every hit of the
// 12-bit bin on 8 of its 2^19 bins and the global atomics serialised — 3.7 ms.)
template <int T>
__global__ void __launch_bounds__(T) topk_scan_kernel(const uint32_t* __restrict__ hist, int nbits,
                                                       int* __restrict__ st, int last) {
  __shared__ uint32_t ws[T / 64];
  const int nb = 1 << nbits;
  const int rem = st[1];
  const uint32_t pre = (uint32_t)st[0];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int C = (nb + T - 1) / T;
  const int hi = max(0, nb - t * C), lo = max(0, hi - C);
  uint32_t sum = 0;
  for (int b = lo; b < hi; ++b) sum += hist[b];
  uint32_t incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) ws[wid] = incl;
  __syncthreads();
  uint32_t before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < T / 64; ++w) {
    before += w < wid ? ws[w] : 0u;
    total += ws[w];
  }
  const uint32_t excl = before + incl - sum;
  const uint32_t need = (uint32_t)rem;
  int bin = -1;
  uint32_t cum = excl;
  if (hi > lo && excl < need && excl + sum >= need) {
    for (int b = hi - 1; b >= lo; --b) {
      if (cum + hist[b] >= need) {
        bin = b;
        break;
      }
      cum += hist[b];
    }
  } else if (t == T - 1 && total < need) {  // fewer candidates than rem: keep them all (bin 0)
    bin = 0;
    cum = total;
  }
  if (bin >= 0) {
    st[0] = (int)((pre << nbits) | (uint32_t)bin);
    st[1] = rem - (int)cum;  // how many elements equal to the final prefix we still need
    if (last) st[3] = st[0];  // full 31-bit pattern of the k-th largest magnitude
  }
}

// compact: |x| > thr always selected (filling the output from the front); |x| == thr selected
// while the tie budget st[1] lasts (filling it from the back). Selected entries are removed from
// the error buffer (error feedback keeps the rest).
// A block step covers TOPK_SUB sub-steps of 256 x TOPK_EPT elements (TOPK_EPT / 4 coalesced
// f32x4 loads per lane each); per sub-step a lane keeps only two 32-bit masks (above / tie, parked
// in LDS), the values die as soon as the masks are built and the few winners are re-read when
// written out (holding the values across the claim needed 226 VGPRs: 2 waves/SIMD). The step claims its
// output slots with ONE 64-bit atomic on st[6..7] (low word: above count, high word: ties) —
// one per 32k elements: the claims on that single address serialise in L2 (16k claims: 0.37 ms,
// 32k: 0.51 ms for 268M elements). Bf16 gradients put tens of thousands of elements exactly on the
// threshold value; the old per-wave tie atomic on one address took 2.9 ms.
constexpr int TOPK_EPT = 32;  // values per lane per sub-step (fits the 32-bit masks)
constexpr int TOPK_SUB = 4;   // sub-steps per claim: packed 16-bit block counts stay <= 32768

template <typename VT>
__global__ void __launch_bounds__(256) topk_select_kernel(float* __restrict__ x, int64_t n, int* __restrict__ st,
                                                           int k, int32_t* __restrict__ idx_out,
                                                           VT* __restrict__ val_out) {
  __shared__ uint32_t wsum[4];
  __shared__ unsigned long long bbase;
  __shared__ uint32_t sgm[TOPK_SUB][256], stm[TOPK_SUB][256];  // per-lane masks of the sub-steps
  const uint32_t thr = (uint32_t)st[3];
  const int tie_budget = st[1];
  unsigned long long* claim = (unsigned long long*)(st + 6);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const bool vec = (((uintptr_t)x) & 15) == 0;
  constexpr int64_t SUBSTEP = 256ll * TOPK_EPT, STEP = SUBSTEP * TOPK_SUB;
  for (int64_t base = blockIdx.x * STEP; base < n; base += (int64_t)gridDim.x * STEP) {
    // element j of sub-step u for this lane: base + u * SUBSTEP + (j / 4) * 1024 + 4 * threadIdx.x + (j % 4)
    uint32_t mine = 0;
#pragma unroll 1
    for (int u = 0; u < TOPK_SUB; ++u) {  // not unrolled: one sub-step of values live at a time
      const int64_t sb = base + u * SUBSTEP;
      float v[TOPK_EPT];
#pragma unroll
      for (int c = 0; c < TOPK_EPT / 4; ++c) {
        const int64_t i0 = sb + (int64_t)c * 1024 + 4 * threadIdx.x;
        if (vec && i0 + 3 < n) {
          const f32x4 t = *(const f32x4*)(x + i0);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[c * 4 + j] = t[j];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[c * 4 + j] = (i0 + j < n) ? x[i0 + j] : 0.f;
        }
      }
      uint32_t g = 0, t = 0;
#pragma unroll
      for (int j = 0; j < TOPK_EPT; ++j) {
        const uint32_t b = absbits(v[j]);
        g |= (uint32_t)(b > thr) << j;
        t |= (uint32_t)(b == thr && b != 0u) << j;  // zero padding never ties
      }
      sgm[u][threadIdx.x] = g;
      stm[u][threadIdx.x] = t;
      mine += (uint32_t)__popc(g) | ((uint32_t)__popc(t) << 16);  // packed (above | ties << 16)
    }
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wid] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
      bbase = tot ? atomicAdd(claim, (unsigned long long)(tot & 0xffffu) | ((unsigned long long)(tot >> 16) << 32))
                  : 0ull;
    }
    __syncthreads();
    uint32_t excl = incl - mine;
    for (int w = 0; w < wid; ++w) excl += wsum[w];
    const unsigned long long bb = bbase;
    int pos = (int)(uint32_t)bb + (int)(excl & 0xffffu);
    int tie = (int)(uint32_t)(bb >> 32) + (int)(excl >> 16);
#pragma unroll 1
    for (int u = 0; u < TOPK_SUB; ++u) {
      const uint32_t gmu = sgm[u][threadIdx.x], tmu = stm[u][threadIdx.x];
      for (uint32_t m = gmu | tmu; m; m &= m - 1) {  // ascending (u, j): the order of the counts
        const int j = __builtin_ctz(m);
        const bool isg = (gmu >> j) & 1u;
        const int slot = isg ? pos : k - 1 - tie;
        const bool take = isg ? pos < k : tie < tie_budget;
        pos += isg;
        tie += !isg;
        if (take) {
          const int64_t i = base + u * SUBSTEP + (int64_t)(j >> 2) * 1024 + 4 * threadIdx.x + (j & 3);
          const float val = x[i];
          const VT sent = (VT)val;
          idx_out[slot] = (int32_t)i;
          val_out[slot] = sent;
          x[i] = val - (float)sent;  // the wire-dtype rounding residual stays in error feedback
        }
      }
    }
    __syncthreads();  // wsum / bbase are rewritten by the next step
  }
}

// dense[idx[j]] += scale * val[j]  (fp32 accumulation of gathered sparse contributions).
// Indices outside [0, n) are dropped in the kernel (no host-side max/min sync per round).
// zero values are skipped: slots the selection left unfilled (fewer than k nonzero candidates)
// hold idx 0 / val 0, and thousands of no-op atomics on dense[0] serialised the kernel (3.2 ms)
template <typename VT>
__global__ void __launch_bounds__(256) scatter_add_kernel(const int32_t* __restrict__ idx, const VT* __restrict__ val,
                                                           int64_t m, float scale, float* __restrict__ dense,
                                                           int64_t n) {
  for (int64_t j = blockIdx.x * 256ll + threadIdx.x; j < m; j += (int64_t)gridDim.x * 256) {
    const float v = (float)val[j];
    const uint32_t i = (uint32_t)idx[j];
    if (v != 0.f && i < (uint32_t)n) atomicAdd(&dense[i], scale * v);
  }
}

// the all-gathered wire format of P peers: per peer L int32 words = k indices, then k values
// (VT) packed into the following words
template <typename VT>
__global__ void __launch_bounds__(256) scatter_add_packed_kernel(const int32_t* __restrict__ wire, int P, int k,
                                                                  int64_t L, float scale, float* __restrict__ dense,
                                                                  int64_t n) {
  const int64_t m = (int64_t)P * k;
  for (int64_t j = blockIdx.x * 256ll + threadIdx.x; j < m; j += (int64_t)gridDim.x * 256) {
    const int64_t p = j / k, r = j - p * k;
    const int32_t* w = wire + p * L;
    const float v = (float)((const VT*)(w + k))[r];
    const uint32_t i = (uint32_t)w[r];
    if (v != 0.f && i < (uint32_t)n) atomicAdd(&dense[i], scale * v);
  }
}

// =====================================================================================
// PowerSGD (grouped over matrices)
// =====================================================================================
struct MatDesc {
  int64_t off;   // element offset of M in the flat fp32 buffer
  int64_t poff;  // element offset of P [rows, R]
  int64_t qoff;  // element offset of Q [cols, R]
  int rows, cols;
  int blk0;      // first block of this matrix in the current launch's block numbering
  int pad;
};

__device__ __forceinline__ int find_mat(const MatDesc* __restrict__ d, int nmat, int b, int stage) {
  // blk0 for stage s is stored in descriptor table s (caller passes the table for the stage)
  int lo = 0, hi = nmat - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].blk0 <= b) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// R consecutive fp32 values (a row of P or Q) — 16-B loads when R is a multiple of 4 (P / Q
// offsets are multiples of R, so those rows are 16-B aligned)
template <int R>
__device__ __forceinline__ void load_rv(const float* __restrict__ p, float (&v)[R]) {
  if constexpr (R % 4 == 0) {
#pragma unroll
    for (int i = 0; i < R; i += 4) {
      const f32x4 t = *(const f32x4*)(p + i);
      v[i] = t[0];
      v[i + 1] = t[1];
      v[i + 2] = t[2];
      v[i + 3] = t[3];
    }
  } else {
#pragma unroll
    for (int i = 0; i < R; ++i) v[i] = p[i];
  }
}

// matrices whose flat offset and row length are multiples of 4 take the 16-B paths below
__device__ __forceinline__ bool psgd_vec(const MatDesc& md) { return ((md.off | (int64_t)md.cols) & 3) == 0; }

// psgd_mq / psgd_reconstruct: each wave owns PSGD_ROWS consecutive rows of a matrix (16 per block)
// and sweeps their columns, so every Q fragment it loads serves PSGD_ROWS rows (one row per wave
// read R floats of Q per element of M: 4x the M traffic at R = 4, through L2).
constexpr int PSGD_ROWS = 4;

// P[row, :] = M[row, :] . Q with the error-feedback accumulation M += G fused into this first pass
// over M (G == nullptr: no accumulation). On the 16-B path each lane takes 4 consecutive columns
// per step (f32x4 M load/store, 8-B G load per row).
// LAZY: the previous round's reconstruct left M = e + P Q^T (it only wrote the output), so this
// pass first subtracts P_prev Q^T from each element (P_prev = this wave's P rows as they stand, Q =
// the warm-start Q, i.e. exactly the pair the previous reconstruct used): e = M - P_prev Q^T + G.
// That moves the error-feedback update out of reconstruct, whose pass then never touches M
// (2 x 4 B per element less HBM traffic per round), at R extra FMAs per element here.
template <int R, bool LAZY>
__global__ void __launch_bounds__(256) psgd_mq_kernel(const MatDesc* __restrict__ d, int nmat, float* __restrict__ M,
                                                       const bf16* __restrict__ G, const float* __restrict__ Q,
                                                       float* __restrict__ P) {
  const int mi = find_mat(d, nmat, blockIdx.x, 0);
  const MatDesc md = d[mi];
  const int rw = ((blockIdx.x - md.blk0) * 4 + (threadIdx.x >> 6)) * PSGD_ROWS;
  const int lane = threadIdx.x & 63;
  if (rw >= md.rows) return;
  const int nr = min(PSGD_ROWS, md.rows - rw);  // wave-uniform
  const int64_t rb = md.off + (int64_t)rw * md.cols;
  const float* q = Q + md.qoff;
  float acc[PSGD_ROWS][R];
  float pold[PSGD_ROWS][R];
#pragma unroll
  for (int i = 0; i < PSGD_ROWS; ++i) {
#pragma unroll
    for (int r = 0; r < R; ++r) acc[i][r] = pold[i][r] = 0.f;
    if (LAZY && i < nr) load_rv<R>(P + md.poff + (int64_t)(rw + i) * R, pold[i]);
  }
  if (psgd_vec(md)) {
    for (int c = 4 * lane; c < md.cols; c += 256) {
      float qv[4][R];
#pragma unroll
      for (int j = 0; j < 4; ++j) load_rv<R>(q + (int64_t)(c + j) * R, qv[j]);
#pragma unroll
      for (int i = 0; i < PSGD_ROWS; ++i) {
        if (i < nr) {
          const int64_t e = rb + (int64_t)i * md.cols + c;
          f32x4 mv = *(const f32x4*)(M + e);
          if (LAZY) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float s = 0.f;
#pragma unroll
              for (int r = 0; r < R; ++r) s = fmaf(pold[i][r], qv[j][r], s);
              mv[j] -= s;
            }
          }
          if (G) {
            const bf16x4 gv = *(const bf16x4*)(G + e);
#pragma unroll
            for (int j = 0; j < 4; ++j) mv[j] += (float)gv[j];
          }
          if (LAZY || G) *(f32x4*)(M + e) = mv;
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < R; ++r) acc[i][r] = fmaf(mv[j], qv[j][r], acc[i][r]);
        }
      }
    }
  } else {
    for (int c = lane; c < md.cols; c += 64) {
      float qv[R];
#pragma unroll
      for (int r = 0; r < R; ++r) qv[r] = q[(int64_t)c * R + r];
#pragma unroll
      for (int i = 0; i < PSGD_ROWS; ++i) {
        if (i < nr) {
          const int64_t e = rb + (int64_t)i * md.cols + c;
          float mv = M[e];
          if (LAZY) {
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r) s = fmaf(pold[i][r], qv[r], s);
            mv -= s;
          }
          if (G) mv += (float)G[e];
          if (LAZY || G) M[e] = mv;
#pragma unroll
          for (int r = 0; r < R; ++r) acc[i][r] = fmaf(mv, qv[r], acc[i][r]);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < PSGD_ROWS; ++i) {
    if (i < nr) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float s = wave_sum(acc[i][r]);
        if (lane == 0) P[md.poff + (int64_t)(rw + i) * R + r] = s;
      }
    }
  }
}

// Q[c, :] += sum over a 256-row slab of M[row, c] * P[row, :]   (Q zeroed beforehand)
// block = (matrix, row slab of 256, column chunk of 256): each wave sweeps 64 rows of the slab for
// 4 consecutive columns per lane (one f32x4 M load per row on the 16-B path, P's slab broadcast
// from LDS); the 4 waves' partials are summed in LDS and added to Q with coalesced atomics
// (consecutive lanes -> consecutive Q words, R / 256 atomics per element of M).
constexpr int PSGD_MTP_ROWS = 256, PSGD_MTP_COLS = 256;

template <int R>
__global__ void __launch_bounds__(256) psgd_mtp_kernel(const MatDesc* __restrict__ d, int nmat,
                                                        const float* __restrict__ M, const float* __restrict__ P,
                                                        float* __restrict__ Q) {
  const int mi = find_mat(d, nmat, blockIdx.x, 1);
  const MatDesc md = d[mi];
  const int local = blockIdx.x - md.blk0;
  const int nck = (md.cols + PSGD_MTP_COLS - 1) / PSGD_MTP_COLS;
  const int slab = local / nck, ck = local % nck;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r0 = slab * PSGD_MTP_ROWS;
  __shared__ float sp[PSGD_MTP_ROWS][R];
  __shared__ float red[4][PSGD_MTP_COLS * R];
  for (int i = threadIdx.x; i < PSGD_MTP_ROWS * R; i += 256) {
    const int rr = r0 + i / R;
    sp[i / R][i % R] = rr < md.rows ? P[md.poff + (int64_t)rr * R + (i % R)] : 0.f;
  }
  __syncthreads();
  const int c = ck * PSGD_MTP_COLS + 4 * lane;
  const int wr0 = r0 + 64 * w, wr1 = min(wr0 + 64, md.rows);
  float acc[4][R];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < R; ++r) acc[j][r] = 0.f;
  if (c < md.cols) {
    const float* mb = M + md.off + c;
    if (psgd_vec(md)) {  // cols % 4 == 0: all 4 columns are in range
#pragma unroll 8
      for (int row = wr0; row < wr1; ++row) {
        const f32x4 mv = *(const f32x4*)(mb + (int64_t)row * md.cols);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < R; ++r) acc[j][r] = fmaf(mv[j], sp[row - r0][r], acc[j][r]);
      }
    } else {
      for (int row = wr0; row < wr1; ++row) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float mv = c + j < md.cols ? mb[(int64_t)row * md.cols + j] : 0.f;
#pragma unroll
          for (int r = 0; r < R; ++r) acc[j][r] = fmaf(mv, sp[row - r0][r], acc[j][r]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < R; ++r) red[w][(4 * lane + j) * R + r] = acc[j][r];
  __syncthreads();
  float* qc = Q + md.qoff + (int64_t)ck * PSGD_MTP_COLS * R;
  for (int i = threadIdx.x; i < PSGD_MTP_COLS * R; i += 256)
    if (ck * PSGD_MTP_COLS + i / R < md.cols) atomicAdd(qc + i, red[0][i] + red[1][i] + red[2][i] + red[3][i]);
}

// modified Gram-Schmidt on the R columns of each P (one block per matrix)
// orth(P) for every matrix at once, as CholeskyQR2 in coefficient space: the R x R Gram
// G = P^T P of each matrix is reduced over row slabs by many blocks (one pass over P); every
// block then derives the upper-triangular T with (P T)^T (P T) = I by modified Gram-Schmidt on
// G (R^3 flops, redundantly per thread) and rewrites its rows P <- P T, accumulating the Gram of
// the result for the second, re-orthogonalising round. Three launches, three streaming passes
// over P with every CU busy, instead of the old one-block-per-matrix serial Gram-Schmidt
// (R(R+1) dependent block reductions per matrix: 1.73 ms for Llama-3-8B's 224 matrices).
// For R <= 8 the Gram is R(R+1)/2 dot products per row — a VALU reduction; MFMA tiles would
// be >90% padding.
constexpr int ORTH_RPT = 8;  // rows per thread -> 2048-row slabs per block

template <int R>
__device__ __forceinline__ void orth_coeffs(const float* __restrict__ Gs, float (&t)[R][R]) {
  // Gs: upper triangle of the symmetric Gram, Gs[a*R+b] for a <= b
  auto G = [&](int a, int b) { return a <= b ? Gs[a * R + b] : Gs[b * R + a]; };
#pragma unroll
  for (int i = 0; i < R; ++i) {
#pragma unroll
    for (int k = 0; k < R; ++k) t[i][k] = (k == i) ? 1.f : 0.f;
#pragma unroll
    for (int j = 0; j < i; ++j) {  // c = q_j^T v_i = t_j^T G t_i
      float c = 0.f;
#pragma unroll
      for (int a = 0; a <= j; ++a)
#pragma unroll
        for (int b = 0; b <= i; ++b) c = fmaf(t[j][a] * G(a, b), t[i][b], c);
#pragma unroll
      for (int k = 0; k <= j; ++k) t[i][k] -= c * t[j][k];
    }
    float nrm = 0.f;
#pragma unroll
    for (int a = 0; a <= i; ++a)
#pragma unroll
      for (int b = 0; b <= i; ++b) nrm = fmaf(t[i][a] * G(a, b), t[i][b], nrm);
    const float inv = nrm > 1e-30f ? rsqrtf(nrm) : 0.f;  // a null column stays zero
#pragma unroll
    for (int k = 0; k <= i; ++k) t[i][k] *= inv;
  }
}

// mode 0: Gram of P into Gout. mode 1: P <- P T(Gin), Gram of the result into Gout. mode 2:
// P <- P T(Gin) only.
template <int R, int MODE>
__global__ void __launch_bounds__(256) psgd_orth_pass_kernel(const MatDesc* __restrict__ d, int nmat,
                                                              float* __restrict__ P, const float* __restrict__ Gin,
                                                              float* __restrict__ Gout) {
  constexpr int NG = R * (R + 1) / 2;
  __shared__ float part[4][NG];
  const int mi = find_mat(d, nmat, blockIdx.x, 0);
  const MatDesc md = d[mi];
  float t[R][R];
  if constexpr (MODE != 0) orth_coeffs<R>(Gin + (int64_t)mi * R * R, t);
  float acc[NG];
#pragma unroll
  for (int q = 0; q < NG; ++q) acc[q] = 0.f;
  const int row0 = (blockIdx.x - md.blk0) * 256 * ORTH_RPT;
  float* p = P + md.poff;
#pragma unroll 2
  for (int rr = 0; rr < ORTH_RPT; ++rr) {
    const int row = row0 + rr * 256 + threadIdx.x;
    if (row < md.rows) {
      float v[R];
      load_rv<R>(p + (int64_t)row * R, v);
      if constexpr (MODE != 0) {
        float w[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
          float a = 0.f;
#pragma unroll
          for (int k = 0; k <= i; ++k) a = fmaf(v[k], t[i][k], a);
          w[i] = a;
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
          v[i] = w[i];
          p[(int64_t)row * R + i] = w[i];
        }
      }
      if constexpr (MODE != 2) {
        int q = 0;
#pragma unroll
        for (int a = 0; a < R; ++a)
#pragma unroll
          for (int b = a; b < R; ++b) {
            acc[q] = fmaf(v[a], v[b], acc[q]);
            ++q;
          }
      }
    }
  }
  if constexpr (MODE != 2) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NG; ++q) {
      const float r = wave_sum(acc[q]);
      if (lane == 0) part[wid][q] = r;
    }
    __syncthreads();
    if (threadIdx.x < NG) {
      const int q = threadIdx.x;
      int a = 0, rem = q;
      while (rem >= R - a) {  // q -> (a, b) of the upper triangle, row-major
        rem -= R - a;
        ++a;
      }
      const int b = a + rem;
      atomicAdd(&Gout[(int64_t)mi * R * R + a * R + b], part[0][q] + part[1][q] + part[2][q] + part[3][q]);
    }
  }
}

// out = P Q^T (bf16, into the flat output buffer at md.off), e = M - P Q^T (in place on M; with
// UPDATE_M false M is left alone and the next psgd_mq<LAZY> applies the subtraction).
// Same row ownership as psgd_mq (PSGD_ROWS rows per wave, P rows held in registers, each Q
// fragment used for all of them); 16-B M load/store and 8-B out store per row on the vector path.
template <int R, bool UPDATE_M>
__global__ void __launch_bounds__(256) psgd_reconstruct_kernel(const MatDesc* __restrict__ d, int nmat,
                                                                float* __restrict__ M, const float* __restrict__ P,
                                                                const float* __restrict__ Q, bf16* __restrict__ out) {
  const int mi = find_mat(d, nmat, blockIdx.x, 2);
  const MatDesc md = d[mi];
  const int rw = ((blockIdx.x - md.blk0) * 4 + (threadIdx.x >> 6)) * PSGD_ROWS;
  const int lane = threadIdx.x & 63;
  if (rw >= md.rows) return;
  const int nr = min(PSGD_ROWS, md.rows - rw);
  const int64_t rb = md.off + (int64_t)rw * md.cols;
  const float* q = Q + md.qoff;
  float pv[PSGD_ROWS][R];
#pragma unroll
  for (int i = 0; i < PSGD_ROWS; ++i) {
    if (i < nr) {
      load_rv<R>(P + md.poff + (int64_t)(rw + i) * R, pv[i]);
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) pv[i][r] = 0.f;
    }
  }
  if (psgd_vec(md)) {
    for (int c = 4 * lane; c < md.cols; c += 256) {
      float qv[4][R];
#pragma unroll
      for (int j = 0; j < 4; ++j) load_rv<R>(q + (int64_t)(c + j) * R, qv[j]);
#pragma unroll
      for (int i = 0; i < PSGD_ROWS; ++i) {
        if (i < nr) {
          f32x4 v;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r) s = fmaf(pv[i][r], qv[j][r], s);
            v[j] = s;
          }
          const int64_t e = rb + (int64_t)i * md.cols + c;
          if (UPDATE_M) {
            f32x4 mv = *(const f32x4*)(M + e);
            mv -= v;
            *(f32x4*)(M + e) = mv;
          }
          const bf16x4 ov = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
          *(bf16x4*)(out + e) = ov;
        }
      }
    }
  } else {
    for (int c = lane; c < md.cols; c += 64) {
      float qv[R];
#pragma unroll
      for (int r = 0; r < R; ++r) qv[r] = q[(int64_t)c * R + r];
#pragma unroll
      for (int i = 0; i < PSGD_ROWS; ++i) {
        if (i < nr) {
          float v = 0.f;
#pragma unroll
          for (int r = 0; r < R; ++r) v = fmaf(pv[i][r], qv[r], v);
          const int64_t e = rb + (int64_t)i * md.cols + c;
          if (UPDATE_M) M[e] -= v;
          out[e] = (bf16)v;
        }
      }
    }
  }
}

// e = e + g  (fp32 += bf16) over a flat range; used before PowerSGD
__global__ void __launch_bounds__(256) ef_accum_kernel(const bf16* __restrict__ g, float* __restrict__ e, int64_t n8) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    bf16x8 gv = *(const bf16x8*)(g + i * 8);
    f32x4 a = *(const f32x4*)(e + i * 8), b = *(const f32x4*)(e + i * 8 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] += (float)gv[j];
      b[j] += (float)gv[j + 4];
    }
    *(f32x4*)(e + i * 8) = a;
    *(f32x4*)(e + i * 8 + 4) = b;
  }
}

// =====================================================================================
// q8: 8-bit block quantisation with error feedback
// =====================================================================================
// Codec of one block of Q8_BLOCK consecutive fp32 values v: amax = max |v|; blocks with
// amax < 2^-100 send nothing (scale 0, codes 0); otherwise scale = amax * (1/127),
// inv = 127 / amax, q = clamp(rint(v * inv), -127, 127), dec = float(q) * scale. Every product and
// difference is its own fp32 operation (contraction is switched off in these functions), so the
// kernels agree bit for bit with the torch reference in parallel/compression.py.
//
// Wire record of a shard of m elements (m a multiple of Q8_BLOCK): m int8 codes, then m / 128 fp32
// scales: m + m / 32 bytes, so a record starts on a 4-byte boundary only. A buffer of n elements
// over P peers is padded to L = P m elements; shard j holds the elements [j m, (j + 1) m).
//
// Work split of all three kernels: 8 consecutive elements per lane, 16 lanes per block (4 blocks
// per wave), the block maximum by 4 cross-lane exchanges inside those 16 lanes.
// HBM traffic per element: encode 2 (bf16 g) + 4 + 4 (e) + 1.03; reduce (P + 1) * 1.03 of the
// shard; decode 1.03 + 2.
constexpr int Q8_BLOCK = 128;
constexpr int64_t Q8_REC = Q8_BLOCK + 4;  // bytes of one block in a record: codes + its scale
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef u32x2 u32x2_a4 __attribute__((aligned(4)));

__device__ __forceinline__ float q8_group_max(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 16));
  return v;
}

__device__ __forceinline__ float q8_code(uint32_t w, int j) { return (float)(int8_t)(w >> (8 * j)); }

// this lane's 8 values of a block whose maximum magnitude is amax -> 8 packed codes, the block's
// scale and the decoded values. Finite input only: with an Inf in the block inv is 0, Inf * 0 is NaN
// and the clamp turns it into -127 (fmaxf drops a NaN where torch's amax keeps it), so kernel and
// reference part there and e stays non-finite; non-finite gradients are unsupported
__device__ __forceinline__ u32x2 q8_quantise8(const float (&v)[8], float amax, float& scale, float (&dec)[8]) {
#pragma clang fp contract(off)
  const bool ok = amax >= 0x1p-100f;
  scale = ok ? amax * (1.0f / 127.0f) : 0.f;
  const float inv = ok ? 127.0f / amax : 0.f;
  u32x2 w = {0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float q = fminf(fmaxf(rintf(v[j] * inv), -127.f), 127.f);
    dec[j] = q * scale;
    w[j >> 2] |= ((uint32_t)(int)q & 0xffu) << (8 * (j & 3));
  }
  return w;
}

// v = e + g, encode v into the P records of `wire`, e = v - dec. units = L / 8 (a multiple of 16, so
// the 16 lanes of a block run the same trips and every lane of a wave reaches the exchanges);
// bps = blocks per shard. Elements in [n, L) encode as zeros and are neither read nor written.
template <typename GT>
__global__ void __launch_bounds__(256) q8_encode_kernel(const GT* __restrict__ g, float* __restrict__ e, int64_t n,
                                                         uint32_t units, uint32_t bps, uint8_t* __restrict__ wire) {
#pragma clang fp contract(off)
  const bool vec = ((((uintptr_t)g) | ((uintptr_t)e)) & 15) == 0;
  for (uint32_t base = blockIdx.x * 256u; base < units; base += gridDim.x * 256u) {
    const uint32_t u = base + threadIdx.x;
    const bool live = u < units;
    const int64_t i = (int64_t)u * 8;
    const bool full = live && vec && i + 8 <= n;
    float v[8];
    if (full) {
      load8(g, i, v);
      const f32x4 e0 = *(const f32x4*)(e + i), e1 = *(const f32x4*)(e + i + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = e0[j] + v[j];
        v[j + 4] = e1[j] + v[j + 4];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (live && i + j < n) ? e[i + j] + (float)g[i + j] : 0.f;
    }
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
    amax = q8_group_max(amax);
    float scale, dec[8];
    const u32x2 w = q8_quantise8(v, amax, scale, dec);
    if (!live) continue;
    const uint32_t blk = u >> 4, sh = blk / bps, rb = blk - sh * bps;
    uint8_t* r = wire + (int64_t)sh * bps * Q8_REC;
    *(u32x2_a4*)(r + (int64_t)rb * Q8_BLOCK + (u & 15u) * 8) = w;
    if ((u & 15u) == 0) *(float*)(r + (int64_t)bps * Q8_BLOCK + (int64_t)rb * 4) = scale;
    if (full) {
      f32x4 e0, e1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        e0[j] = v[j] - dec[j];
        e1[j] = v[j + 4] - dec[j + 4];
      }
      *(f32x4*)(e + i) = e0;
      *(f32x4*)(e + i + 4) = e1;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (i + j < n) e[i + j] = v[j] - dec[j];
    }
  }
}

// recv: the P peers' records of this peer's shard (bps blocks each). acc = sum of the decoded
// values over p = 0 .. P-1 IN THAT ORDER (fp32), acc *= avg_scale, encode acc into one record.
__global__ void __launch_bounds__(256) q8_reduce_kernel(const uint8_t* __restrict__ recv, int P, uint32_t bps,
                                                         float avg_scale, uint8_t* __restrict__ out) {
#pragma clang fp contract(off)
  const uint32_t units = bps * 16u;
  const int64_t rec = (int64_t)bps * Q8_REC, soff = (int64_t)bps * Q8_BLOCK;
  for (uint32_t base = blockIdx.x * 256u; base < units; base += gridDim.x * 256u) {
    const uint32_t u = base + threadIdx.x;
    const bool live = u < units;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    if (live) {
      const uint8_t* c = recv + (int64_t)u * 8;
      const uint8_t* s = recv + soff + (int64_t)(u >> 4) * 4;
#pragma unroll 4
      for (int p = 0; p < P; ++p) {
        const u32x2 w = *(const u32x2_a4*)(c + p * rec);
        const float sc = *(const float*)(s + p * rec);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = acc[j] + q8_code(w[j >> 2], j & 3) * sc;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = acc[j] * avg_scale;
    }
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(acc[j]));
    amax = q8_group_max(amax);
    float scale, dec[8];
    const u32x2 w = q8_quantise8(acc, amax, scale, dec);
    if (!live) continue;
    *(u32x2_a4*)(out + (int64_t)u * 8) = w;
    if ((u & 15u) == 0) *(float*)(out + soff + (int64_t)(u >> 4) * 4) = scale;
  }
}

// records: the P gathered records (bps blocks each); out[i] = bf16(float(q[i]) * scale) for i < n
__global__ void __launch_bounds__(256) q8_decode_kernel(const uint8_t* __restrict__ records, int64_t n, uint32_t bps,
                                                         bf16* __restrict__ out) {
#pragma clang fp contract(off)
  const bool vec = (((uintptr_t)out) & 15) == 0;
  const uint32_t units = (uint32_t)((n + 7) / 8);
  for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u) {
    const uint32_t blk = u >> 4, sh = blk / bps, rb = blk - sh * bps;
    const uint8_t* r = records + (int64_t)sh * bps * Q8_REC;
    const u32x2 w = *(const u32x2_a4*)(r + (int64_t)rb * Q8_BLOCK + (u & 15u) * 8);
    const float sc = *(const float*)(r + (int64_t)bps * Q8_BLOCK + (int64_t)rb * 4);
    const int64_t i = (int64_t)u * 8;
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (bf16)(q8_code(w[j >> 2], j & 3) * sc);
    if (vec && i + 8 <= n) {
      *(bf16x8*)(out + i) = o;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (i + j < n) out[i + j] = o[j];
    }
  }
}

// The robust sibling of q8_reduce_kernel: the rank-order sum becomes the coordinate-wise trimmed mean
// of ops/robust.py over the decoded records (parallel/compression.py, reduce_robust, holds the torch
// definition; the two agree bit for bit). Per element of the shard, over the rows named by `live`:
//   * dec = float(code) * scale, one fp32 multiply on whatever bytes the record holds; a NaN product
//     counts as the canonical +NaN 0x7FC00000 (the sign and payload of a NaN that an operation makes
//     differ between processors: 0 * Inf is 0xFFC00000 on x86 and 0x7FC00000 here).
//   * order key s = pattern ^ (negative ? 0xFFFFFFFF : 0x80000000), ties go to the row. An fp32 key
//     and a row do not fit one dword, so nothing is sorted: for every pair j < k, row j precedes row k
//     iff s_j <= s_k, and a row's rank is the number of rows that precede it. A dead row takes the key
//     0xFFFFFFFF, above every live key, so the K live rows hold the ranks 0 .. K-1.
//   * kept iff f <= rank <= K-1-f; result = (sum of the kept values, ascending row order, from +0) *
//     inv, no fused multiply-add; a non-finite result becomes +0 and adds 1 to `nonfinite`.
//   * elements at or beyond `valid` (the padding of the last shards) do not vote: result +0, no count.
//   * counts[k] += 1 for every live row k that voted and was not kept.
// The results are quantised by the codec of the other q8 kernels into one record. Same work split as
// q8_reduce_kernel; every lane of a wave, lanes past the end included, reaches the cross-lane maximum.
// PP: P padded to a power of two; rows outside `live` (P..PP-1 among them) are never read.
constexpr int Q8_TRIMMED_MAX_BLOCKS = 2048;  // the grid cap: a shard above 2048 * 256 * 8 elements takes a second trip

template <int PP>
__global__ void __launch_bounds__(256) q8_trimmed_reduce_kernel(const uint8_t* __restrict__ recv, uint32_t bps,
                                                                 uint32_t valid, int f, int K, uint32_t live,
                                                                 float inv, uint8_t* __restrict__ out,
                                                                 unsigned long long* __restrict__ counts,
                                                                 unsigned long long* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  __shared__ uint32_t wave_cnt[4][PP + 1];
  const uint32_t units = bps * 16u;
  const int64_t rec = (int64_t)bps * Q8_REC, soff = (int64_t)bps * Q8_BLOCK;
  const uint32_t span = (uint32_t)(K - 1 - 2 * f);
  uint32_t cnt[PP];  // elements of this thread at which the row voted and was not kept (dead rows: dropped below)
#pragma unroll
  for (int k = 0; k < PP; ++k) cnt[k] = 0;
  uint32_t bad = 0;
  for (uint32_t base = blockIdx.x * 256u; base < units; base += gridDim.x * 256u) {
    const uint32_t u = base + threadIdx.x;
    const bool in_range = u < units;
    u32x2 w[PP];
    float sc[PP];
#pragma unroll
    for (int k = 0; k < PP; ++k) {
      w[k] = u32x2{0u, 0u};
      sc[k] = 0.f;
      if (in_range && ((live >> k) & 1u)) {
        w[k] = *(const u32x2_a4*)(recv + k * rec + (int64_t)u * 8);
        sc[k] = *(const float*)(recv + k * rec + soff + (int64_t)(u >> 4) * 4);
      }
    }
    float res[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool votes = in_range && u * 8u + j < valid;  // below 2^31, as m is
      uint32_t val[PP], s[PP], rank[PP];
#pragma unroll
      for (int k = 0; k < PP; ++k) {
        const float d = q8_code(w[k][j >> 2], j & 3) * sc[k];
        val[k] = d != d ? 0x7FC00000u : __float_as_uint(d);
        // a dead row (w = 0, sc = 0: val = +0) takes the key 0xFFFFFFFF, above every live key: live keys end at
        // +NaN, 0xFFC00000, now that NaN has one pattern. The mask is wave-uniform and folds into the sign flip
        const uint32_t flip = 0x80000000u | (((live >> k) & 1u) - 1u);
        s[k] = val[k] ^ ((uint32_t)((int32_t)val[k] >> 31) | flip);
        rank[k] = (uint32_t)(PP - 1 - k - f);  // rank - f, modulo 2^32, once the rows after k have had their say
      }
#pragma unroll
      for (int k = 1; k < PP; ++k) {
#pragma unroll
        for (int i = 0; i < k; ++i) {
          const uint32_t first = s[i] <= s[k] ? 1u : 0u;  // row i precedes row k
          rank[k] += first;
          rank[i] -= first;
        }
      }
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < PP; ++k) {
        const bool kept = rank[k] <= span;  // f <= rank <= K - 1 - f; a dead row's rank is K or more
        t += kept ? __uint_as_float(val[k]) : 0.f;  // + (+0) leaves a sum that started at +0 unchanged
        cnt[k] += (votes && !kept) ? 1u : 0u;
      }
      const float r = t * inv;
      const bool finite = (__float_as_uint(r) & 0x7F800000u) != 0x7F800000u;
      bad += (votes && !finite) ? 1u : 0u;
      res[j] = (votes && finite) ? r : 0.f;
      // one element at a time: left to itself the scheduler interleaves the eight elements' comparisons, whose lane
      // masks (120 pairs of scalar registers per element at 16 rows) then spill by the thousand
      __builtin_amdgcn_sched_barrier(0);
    }
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(res[j]));
    amax = q8_group_max(amax);
    float scale, dec[8];
    const u32x2 o = q8_quantise8(res, amax, scale, dec);
    if (!in_range) continue;
    *(u32x2_a4*)(out + (int64_t)u * 8) = o;
    if ((u & 15u) == 0) *(float*)(out + soff + (int64_t)(u >> 4) * 4) = scale;
  }
  if (counts || nonfinite) {  // registers -> wave -> block (LDS) -> one global atomic per live row per block
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k <= PP; ++k) {
      uint32_t c = k < PP ? cnt[k < PP ? k : 0] : bad;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
      if (lane == 0) wave_cnt[wid][k] = c;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k <= PP) {
      const uint32_t c = wave_cnt[0][k] + wave_cnt[1][k] + wave_cnt[2][k] + wave_cnt[3][k];
      if (k < PP) {
        if (counts && ((live >> k) & 1u) && c) atomicAdd(counts + k, (unsigned long long)c);
      } else if (nonfinite && c) {
        atomicAdd(nonfinite, (unsigned long long)c);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Centered clipping over the q8 records: the cross of q8_trimmed_reduce_kernel above and the cclip kernels of
// robust.hip. parallel/compression.py, reduce_cclip_reference, holds the definition (decode as above, then
// ops/robust.py centered_clip_reference on the fp32 rows dec[:, :valid], then the finish of the trimmed kernel and the
// codec); these kernels agree with it bit for bit. Over the rows named by `live` of one shard of m elements:
//   init   v = the median rule on the decoded fp32 rows (the pairwise rank count of the trimmed kernel), kept in
//          fp32 in the workspace, and the chunk partials of the first distances;
//   L x    weights from the partials (cclip_weights_kernel of robust.hip, through vcx_cclip_weights), then a step:
//          decode again, v += (sum over the rows with w > 0, ascending, of w (x - v)) * inv_K where v is finite.
//          Not LAST: v is written back and the next partials come from the values still in registers. LAST: a
//          non-finite v becomes +0 and is counted, elements at or beyond `valid` become +0 uncounted, and the m
//          values are quantised into one record.
// The work split is the q8 one and cclip's at once: a unit is 8 consecutive elements of one lane, a chunk is 512
// units (4096 elements, 32 q8 blocks); thread t takes unit c * 512 + t, then c * 512 + 256 + t, so the 16 lanes of a
// q8 block are the 16 aligned lanes q8_group_max exchanges among, and the thread sums of a distance are cclip's 256
// slots. Elements at or beyond `valid` add +0 to every distance (the definition sums over `valid` elements only; a
// distance is never -0, so the bits agree). No lane leaves a trip early: lanes past the end carry zeros to every
// cross-lane exchange and barrier. Rows outside `live` are never read. No float atomics, no fused multiply-add.
constexpr uint32_t Q8_CC_CHUNK_UNITS = 512;  // units of 8 elements per chunk
constexpr int Q8_CC_MAX_BLOCKS = 2048;       // workgroup cap of the init and step passes: more chunks are strided over

__device__ __forceinline__ bool q8_cc_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// The 256 thread sums s[k] of one chunk -> part[k * nchunks + c] for every live row k: the xor butterfly inside a
// wave (both lanes of a pair hold lower + higher), then (w0 + w1) + (w2 + w3).
template <int PP>
__device__ __forceinline__ void q8_cc_chunk_sum(float (&s)[PP], float (*wave_part)[PP], float* __restrict__ part,
                                                uint32_t nchunks, uint32_t c, uint32_t live) {
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
    part[(int64_t)k * nchunks + c] = (wave_part[0][k] + wave_part[1][k]) + (wave_part[2][k] + wave_part[3][k]);
  }
  __syncthreads();  // wave_part is written again in the next chunk
}

template <int PP>
__global__ void __launch_bounds__(256) q8_cclip_init_kernel(const uint8_t* __restrict__ recv, uint32_t bps,
                                                             uint32_t valid, int f, int K, uint32_t live, float inv,
                                                             float* __restrict__ v, float* __restrict__ part,
                                                             uint32_t nchunks) {
#pragma clang fp contract(off)
  __shared__ float wave_part[4][PP];
  const uint32_t units = bps * 16u;
  const int64_t rec = (int64_t)bps * Q8_REC, soff = (int64_t)bps * Q8_BLOCK;
  const uint32_t span = (uint32_t)(K - 1 - 2 * f);
  for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    float s[PP];
#pragma unroll
    for (int k = 0; k < PP; ++k) s[k] = 0.f;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      const uint32_t u = c * Q8_CC_CHUNK_UNITS + h * 256u + threadIdx.x;
      const bool in_range = u < units;
      u32x2 w[PP];
      float sc[PP];
#pragma unroll
      for (int k = 0; k < PP; ++k) {
        w[k] = u32x2{0u, 0u};
        sc[k] = 0.f;
        if (in_range && ((live >> k) & 1u)) {
          w[k] = *(const u32x2_a4*)(recv + k * rec + (int64_t)u * 8);
          sc[k] = *(const float*)(recv + k * rec + soff + (int64_t)(u >> 4) * 4);
        }
      }
      float vv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool votes = in_range && u * 8u + j < valid;  // below 2^31, as m is
        uint32_t val[PP], sk[PP], rank[PP];
#pragma unroll
        for (int k = 0; k < PP; ++k) {
          const float d = q8_code(w[k][j >> 2], j & 3) * sc[k];
          val[k] = d != d ? 0x7FC00000u : __float_as_uint(d);
          const uint32_t flip = 0x80000000u | (((live >> k) & 1u) - 1u);  // a dead row takes the key 0xFFFFFFFF
          sk[k] = val[k] ^ ((uint32_t)((int32_t)val[k] >> 31) | flip);
          rank[k] = (uint32_t)(PP - 1 - k - f);  // rank - f, modulo 2^32, once the rows after k have had their say
        }
#pragma unroll
        for (int k = 1; k < PP; ++k) {
#pragma unroll
          for (int i = 0; i < k; ++i) {
            const uint32_t first = sk[i] <= sk[k] ? 1u : 0u;  // row i precedes row k
            rank[k] += first;
            rank[i] -= first;
          }
        }
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < PP; ++k) t += rank[k] <= span ? __uint_as_float(val[k]) : 0.f;
        const float c0 = t * inv;  // the median rule's fp32 result: the start
        vv[j] = c0;
        const bool fin = votes && q8_cc_finite(c0);
#pragma unroll
        for (int k = 0; k < PP; ++k) {
          const float e = fin ? __uint_as_float(val[k]) - c0 : 0.f;
          if ((live >> k) & 1u) s[k] = s[k] + e * e;
        }
        // one element at a time, as in q8_trimmed_reduce_kernel: interleaved, the comparisons' lane masks spill
        __builtin_amdgcn_sched_barrier(0);
      }
      if (in_range) {
        *(f32x4*)(v + (int64_t)u * 8) = f32x4{vv[0], vv[1], vv[2], vv[3]};
        *(f32x4*)(v + (int64_t)u * 8 + 4) = f32x4{vv[4], vv[5], vv[6], vv[7]};
      }
    }
    q8_cc_chunk_sum<PP>(s, wave_part, part, nchunks, c, live);
  }
}

template <int PP, bool LAST>
__global__ void __launch_bounds__(256) q8_cclip_step_kernel(const uint8_t* __restrict__ recv, uint32_t bps,
                                                             uint32_t valid, int P, uint32_t live, float inv_k,
                                                             float* __restrict__ v, const float* __restrict__ wgt,
                                                             float* __restrict__ part, uint32_t nchunks,
                                                             uint8_t* __restrict__ out,
                                                             unsigned long long* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  __shared__ float wave_part[4][PP];
  __shared__ uint32_t wave_bad[4];
  const uint32_t units = bps * 16u;
  const int64_t rec = (int64_t)bps * Q8_REC, soff = (int64_t)bps * Q8_BLOCK;
  float wk[PP];
  uint32_t use = 0u;  // live rows with a weight above zero: the others are skipped, never multiplied
#pragma unroll
  for (int k = 0; k < PP; ++k) {
    wk[k] = (k < P && ((live >> k) & 1u)) ? wgt[k] : 0.f;
    if (wk[k] > 0.f) use |= 1u << k;
  }
  uint32_t bad = 0;
  for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    float s[PP];
#pragma unroll
    for (int k = 0; k < PP; ++k) s[k] = 0.f;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      const uint32_t u = c * Q8_CC_CHUNK_UNITS + h * 256u + threadIdx.x;
      const bool in_range = u < units;
      u32x2 w[PP];
      float sc[PP];
#pragma unroll
      for (int k = 0; k < PP; ++k) {
        w[k] = u32x2{0u, 0u};
        sc[k] = 0.f;
        if (in_range && ((live >> k) & 1u)) {
          w[k] = *(const u32x2_a4*)(recv + k * rec + (int64_t)u * 8);
          sc[k] = *(const float*)(recv + k * rec + soff + (int64_t)(u >> 4) * 4);
        }
      }
      float vv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) vv[j] = 0.f;
      if (in_range) {
        const f32x4 v0 = *(const f32x4*)(v + (int64_t)u * 8), v1 = *(const f32x4*)(v + (int64_t)u * 8 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          vv[j] = v0[j];
          vv[j + 4] = v1[j];
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool votes = in_range && u * 8u + j < valid;
        const float c0 = vv[j];
        float x[PP];
#pragma unroll
        for (int k = 0; k < PP; ++k) x[k] = q8_code(w[k][j >> 2], j & 3) * sc[k];
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < PP; ++k) {
          const float term = wk[k] * (x[k] - c0);
          t = ((use >> k) & 1u) ? t + term : t;
        }
        const float c1 = q8_cc_finite(c0) ? c0 + t * inv_k : c0;
        if (LAST) {
          const bool finite = q8_cc_finite(c1);
          bad += (votes && !finite) ? 1u : 0u;
          vv[j] = (votes && finite) ? c1 : 0.f;
        } else {
          vv[j] = c1;
          const bool fin = votes && q8_cc_finite(c1);
#pragma unroll
          for (int k = 0; k < PP; ++k) {
            const float e = fin ? x[k] - c1 : 0.f;
            if ((live >> k) & 1u) s[k] = s[k] + e * e;
          }
        }
      }
      if (LAST) {
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(vv[j]));
        amax = q8_group_max(amax);
        float scale, dec[8];
        const u32x2 o = q8_quantise8(vv, amax, scale, dec);
        if (in_range) {
          *(u32x2_a4*)(out + (int64_t)u * 8) = o;
          if ((u & 15u) == 0) *(float*)(out + soff + (int64_t)(u >> 4) * 4) = scale;
        }
      } else if (in_range) {
        *(f32x4*)(v + (int64_t)u * 8) = f32x4{vv[0], vv[1], vv[2], vv[3]};
        *(f32x4*)(v + (int64_t)u * 8 + 4) = f32x4{vv[4], vv[5], vv[6], vv[7]};
      }
    }
    if (!LAST) q8_cc_chunk_sum<PP>(s, wave_part, part, nchunks, c, live);
  }
  if (LAST && nonfinite) {  // registers -> wave -> block (LDS) -> one global atomic per workgroup
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t b = bad;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b += __shfl_xor(b, o, 64);
    if (lane == 0) wave_bad[wid] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t tot = wave_bad[0] + wave_bad[1] + wave_bad[2] + wave_bad[3];
      if (tot) atomicAdd(nonfinite, (unsigned long long)tot);
    }
  }
}

// One voter: its decoded row through the finish (non-finite -> +0, counted; at or beyond `valid` -> +0), quantised
// again; its weight is 1, the others' 0.
__global__ void __launch_bounds__(256) q8_cclip_one_voter_kernel(const uint8_t* __restrict__ recv, uint32_t bps,
                                                                  uint32_t valid, int P, int row,
                                                                  uint8_t* __restrict__ out,
                                                                  float* __restrict__ w_user,
                                                                  unsigned long long* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  __shared__ uint32_t wave_bad[4];
  const uint32_t units = bps * 16u;
  const int64_t rec = (int64_t)bps * Q8_REC, soff = (int64_t)bps * Q8_BLOCK;
  const uint8_t* r = recv + row * rec;
  uint32_t bad = 0;
  for (uint32_t base = blockIdx.x * 256u; base < units; base += gridDim.x * 256u) {
    const uint32_t u = base + threadIdx.x;
    const bool in_range = u < units;
    u32x2 w = {0u, 0u};
    float sc = 0.f;
    if (in_range) {
      w = *(const u32x2_a4*)(r + (int64_t)u * 8);
      sc = *(const float*)(r + soff + (int64_t)(u >> 4) * 4);
    }
    float res[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool votes = in_range && u * 8u + j < valid;
      const float d = q8_code(w[j >> 2], j & 3) * sc;
      const bool finite = q8_cc_finite(d);
      bad += (votes && !finite) ? 1u : 0u;
      res[j] = (votes && finite) ? d : 0.f;
    }
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(res[j]));
    amax = q8_group_max(amax);
    float scale, dec[8];
    const u32x2 o = q8_quantise8(res, amax, scale, dec);
    if (!in_range) continue;
    *(u32x2_a4*)(out + (int64_t)u * 8) = o;
    if ((u & 15u) == 0) *(float*)(out + soff + (int64_t)(u >> 4) * 4) = scale;
  }
  if (w_user && blockIdx.x == 0 && (int)threadIdx.x < P) w_user[threadIdx.x] = (int)threadIdx.x == row ? 1.f : 0.f;
  if (nonfinite) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
    if (lane == 0) wave_bad[wid] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t tot = wave_bad[0] + wave_bad[1] + wave_bad[2] + wave_bad[3];
      if (tot) atomicAdd(nonfinite, (unsigned long long)tot);
    }
  }
}

}  // namespace vcx

// ====================================================================================== launchers
using namespace vcx;

void vcx_topk_ef(const void* g, int g_is_bf16, float* e, int64_t n, int k, int* st, uint32_t* hist,
                 int32_t* idx_out, void* val_out, int val_is_bf16, hipStream_t s) {
  // st = {0, k, 0, 0, 0, 0, 0, 0} (set by the caller); hist: TK_BINS zeroed words, left zeroed
  const int grid = stream_grid(n / 8 + 1, 256, 2048);
  const size_t hb = TK_BINS * sizeof(uint32_t);
  if (g_is_bf16)
    hipLaunchKernelGGL(topk_accum_hist_kernel<bf16>, dim3(grid), dim3(256), 0, s, (const bf16*)g, e, n, hist);
  else
    hipLaunchKernelGGL(topk_accum_hist_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)g, e, n, hist);
  hipLaunchKernelGGL(topk_scan_kernel<256>, dim3(1), dim3(256), 0, s, hist, 12, st, 0);
  hipMemsetAsync(hist, 0, hb, s);
  hipLaunchKernelGGL(topk_hist_kernel, dim3(grid), dim3(256), 0, s, e, n, st, 19, 7, 12, hist);
  hipLaunchKernelGGL(topk_scan_kernel<256>, dim3(1), dim3(256), 0, s, hist, 12, st, 0);
  hipMemsetAsync(hist, 0, hb, s);
  hipLaunchKernelGGL(topk_hist_kernel, dim3(grid), dim3(256), 0, s, e, n, st, 7, 0, 7, hist);
  hipLaunchKernelGGL(topk_scan_kernel<256>, dim3(1), dim3(256), 0, s, hist, 7, st, 1);
  hipMemsetAsync(hist, 0, hb, s);
  const int sgrid = stream_grid((n + TOPK_EPT * TOPK_SUB - 1) / (TOPK_EPT * TOPK_SUB), 256, 2048);
  if (val_is_bf16)
    hipLaunchKernelGGL(topk_select_kernel<bf16>, dim3(sgrid), dim3(256), 0, s, e, n, st, k, idx_out, (bf16*)val_out);
  else
    hipLaunchKernelGGL(topk_select_kernel<float>, dim3(sgrid), dim3(256), 0, s, e, n, st, k, idx_out,
                       (float*)val_out);
}

int vcx_topk_hist_words() { return TK_BINS; }

void vcx_scatter_add(const int32_t* idx, const void* val, int val_is_bf16, int64_t m, float scale, float* dense,
                     int64_t n, hipStream_t s) {
  const int grid = stream_grid(m, 256, 1024);
  if (val_is_bf16)
    hipLaunchKernelGGL(scatter_add_kernel<bf16>, dim3(grid), dim3(256), 0, s, idx, (const bf16*)val, m, scale, dense,
                       n);
  else
    hipLaunchKernelGGL(scatter_add_kernel<float>, dim3(grid), dim3(256), 0, s, idx, (const float*)val, m, scale,
                       dense, n);
}

void vcx_scatter_add_packed(const int32_t* wire, int P, int k, int64_t L, int val_is_bf16, float scale, float* dense,
                            int64_t n, hipStream_t s) {
  const int grid = stream_grid((int64_t)P * k, 256, 1024);
  if (val_is_bf16)
    hipLaunchKernelGGL(scatter_add_packed_kernel<bf16>, dim3(grid), dim3(256), 0, s, wire, P, k, L, scale, dense, n);
  else
    hipLaunchKernelGGL(scatter_add_packed_kernel<float>, dim3(grid), dim3(256), 0, s, wire, P, k, L, scale, dense, n);
}

#define PSGD_R_DISPATCH(RV, ...)                              \
  switch (RV) {                                               \
    case 1: { constexpr int R = 1; __VA_ARGS__; } break;      \
    case 2: { constexpr int R = 2; __VA_ARGS__; } break;      \
    case 4: { constexpr int R = 4; __VA_ARGS__; } break;      \
    default: { constexpr int R = 8; __VA_ARGS__; } break;     \
  }

void vcx_psgd_mq(const void* desc, int nmat, int nblocks, float* M, const void* G, const float* Q, float* P, int rank,
                 int lazy, hipStream_t s) {
  if (lazy) {
    PSGD_R_DISPATCH(rank, hipLaunchKernelGGL((psgd_mq_kernel<R, true>), dim3(nblocks), dim3(256), 0, s,
                                             (const MatDesc*)desc, nmat, M, (const bf16*)G, Q, P));
  } else {
    PSGD_R_DISPATCH(rank, hipLaunchKernelGGL((psgd_mq_kernel<R, false>), dim3(nblocks), dim3(256), 0, s,
                                             (const MatDesc*)desc, nmat, M, (const bf16*)G, Q, P));
  }
}

void vcx_psgd_mtp(const void* desc, int nmat, int nblocks, const float* M, const float* P, float* Q, int rank,
                  hipStream_t s) {
  PSGD_R_DISPATCH(rank, hipLaunchKernelGGL(psgd_mtp_kernel<R>, dim3(nblocks), dim3(256), 0, s, (const MatDesc*)desc,
                                           nmat, M, P, Q));
}

void vcx_psgd_orth(const void* desc, int nmat, int nblocks, float* P, float* G, int rank, hipStream_t s) {
  // G: 2 * nmat * rank^2 floats of scratch (zeroed here)
  const int64_t gm = (int64_t)nmat * rank * rank;
  hipMemsetAsync(G, 0, 2 * gm * sizeof(float), s);
  PSGD_R_DISPATCH(rank, {
    const MatDesc* d = (const MatDesc*)desc;
    hipLaunchKernelGGL((psgd_orth_pass_kernel<R, 0>), dim3(nblocks), dim3(256), 0, s, d, nmat, P, G, G);
    hipLaunchKernelGGL((psgd_orth_pass_kernel<R, 1>), dim3(nblocks), dim3(256), 0, s, d, nmat, P, G, G + gm);
    hipLaunchKernelGGL((psgd_orth_pass_kernel<R, 2>), dim3(nblocks), dim3(256), 0, s, d, nmat, P, G + gm, G);
  });
}

int vcx_psgd_orth_rows() { return 256 * ORTH_RPT; }

void vcx_psgd_reconstruct(const void* desc, int nmat, int nblocks, float* M, const float* P, const float* Q,
                          void* out, int rank, int update_m, hipStream_t s) {
  if (update_m) {
    PSGD_R_DISPATCH(rank, hipLaunchKernelGGL((psgd_reconstruct_kernel<R, true>), dim3(nblocks), dim3(256), 0, s,
                                             (const MatDesc*)desc, nmat, M, P, Q, (bf16*)out));
  } else {
    PSGD_R_DISPATCH(rank, hipLaunchKernelGGL((psgd_reconstruct_kernel<R, false>), dim3(nblocks), dim3(256), 0, s,
                                             (const MatDesc*)desc, nmat, M, P, Q, (bf16*)out));
  }
}

void vcx_ef_accum(const void* g, float* e, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(ef_accum_kernel, dim3(stream_grid(n / 8, 256)), dim3(256), 0, s, (const bf16*)g, e, n / 8);
}

void vcx_q8_encode(const void* g, int g_is_bf16, float* e, int64_t n, int64_t L, int P, uint8_t* wire, hipStream_t s) {
  const uint32_t units = (uint32_t)(L / 8), bps = (uint32_t)(L / P / Q8_BLOCK);
  const int grid = stream_grid(units, 256, 2048);
  if (g_is_bf16)
    hipLaunchKernelGGL(q8_encode_kernel<bf16>, dim3(grid), dim3(256), 0, s, (const bf16*)g, e, n, units, bps, wire);
  else
    hipLaunchKernelGGL(q8_encode_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)g, e, n, units, bps, wire);
}

void vcx_q8_reduce(const uint8_t* recv, int P, int64_t m, float avg_scale, uint8_t* out_record, hipStream_t s) {
  const uint32_t bps = (uint32_t)(m / Q8_BLOCK);
  hipLaunchKernelGGL(q8_reduce_kernel, dim3(stream_grid(m / 8, 256, 2048)), dim3(256), 0, s, recv, P, bps, avg_scale,
                     out_record);
}

// A call the kernel cannot take raises before anything is launched.
void vcx_q8_trimmed_reduce(const uint8_t* recv, int P, int64_t m, int trim, uint32_t live_mask, int64_t valid,
                           uint8_t* out_record, int64_t* counts, int64_t* nonfinite, hipStream_t s) {
  const std::string who = "q8_trimmed_reduce";
  check_rows(who, P, live_mask);
  if (m <= 0 || m % Q8_BLOCK != 0 || m >= INT32_MAX)
    throw std::invalid_argument(who + ": m must be a positive multiple of 128 below 2^31, got " + std::to_string(m));
  if (valid < 0 || valid > m)
    throw std::invalid_argument(who + ": valid must be in 0..m, got " + std::to_string(valid));
  if (trim < 0) throw std::invalid_argument(who + ": trim must be >= 0");
  if (!recv || ((uintptr_t)recv & 15)) throw std::invalid_argument(who + ": recv must be 16-byte aligned");
  if (!out_record || ((uintptr_t)out_record & 3))
    throw std::invalid_argument(who + ": out_record must be 4-byte aligned");
  if (((uintptr_t)counts | (uintptr_t)nonfinite) & 7)
    throw std::invalid_argument(who + ": counts and nonfinite must be 8-byte aligned");
  const int K = __builtin_popcount(live_mask), f = trim_of(trim, K);
  const float inv = trim_inv(K, f);
  const uint32_t bps = (uint32_t)(m / Q8_BLOCK);
  const dim3 grid(stream_grid(m / 8, 256, Q8_TRIMMED_MAX_BLOCKS)), block(256);
  for_padded_peers(P, [&](auto pp) {
    hipLaunchKernelGGL(q8_trimmed_reduce_kernel<decltype(pp)::value>, grid, block, 0, s, recv, bps, (uint32_t)valid, f,
                       K, live_mask, inv, out_record, (unsigned long long*)counts, (unsigned long long*)nonfinite);
  });
}

int vcx_q8_trimmed_reduce_max_blocks() { return Q8_TRIMMED_MAX_BLOCKS; }

int vcx_q8_cclip_max_workgroups() { return Q8_CC_MAX_BLOCKS; }

int64_t vcx_q8_cclip_workspace_floats(int P, int64_t m) {
  const int64_t nchunks = (m / 8 + Q8_CC_CHUNK_UNITS - 1) / Q8_CC_CHUNK_UNITS;
  return m + (int64_t)P * nchunks + TR_MAX_P;
}

// A call the kernels cannot take raises before anything is launched.
void vcx_q8_cclip_reduce(const uint8_t* recv, int P, int64_t m, uint32_t live_mask, int64_t valid, float tau, int iters,
                         uint8_t* out_record, float* weights, int64_t* nonfinite, float* workspace, hipStream_t s) {
  const std::string who = "q8_cclip_reduce";
  check_rows(who, P, live_mask);
  if (m <= 0 || m % Q8_BLOCK != 0 || m >= INT32_MAX)
    throw std::invalid_argument(who + ": m must be a positive multiple of 128 below 2^31, got " + std::to_string(m));
  if (valid < 0 || valid > m)
    throw std::invalid_argument(who + ": valid must be in 0..m, got " + std::to_string(valid));
  if (!(tau >= 0.f) || tau > 3.402823466e38f)
    throw std::invalid_argument(who + ": tau must be finite and >= 0 (0: adaptive)");
  if (iters < 1 || iters > 8)
    throw std::invalid_argument(who + ": iters must be in 1..8, got " + std::to_string(iters));
  if (!recv || ((uintptr_t)recv & 15)) throw std::invalid_argument(who + ": recv must be 16-byte aligned");
  if (!out_record || ((uintptr_t)out_record & 3))
    throw std::invalid_argument(who + ": out_record must be 4-byte aligned");
  if ((uintptr_t)weights & 3) throw std::invalid_argument(who + ": weights must be 4-byte aligned");
  if ((uintptr_t)nonfinite & 7) throw std::invalid_argument(who + ": nonfinite must be 8-byte aligned");
  if (!workspace || ((uintptr_t)workspace & 15))
    throw std::invalid_argument(who + ": workspace must be 16-byte aligned");
  const int K = __builtin_popcount(live_mask);
  const uint32_t bps = (uint32_t)(m / Q8_BLOCK);
  const dim3 block(256);
  if (K == 1) {
    hipLaunchKernelGGL(q8_cclip_one_voter_kernel, dim3(stream_grid(m / 8, 256, Q8_CC_MAX_BLOCKS)), block, 0, s, recv,
                       bps, (uint32_t)valid, P, __builtin_ctz(live_mask), out_record, weights,
                       (unsigned long long*)nonfinite);
    return;
  }
  const int f = trim_of(TR_MAX_P, K);  // the median rule is the start: all the trim that K voters allow
  const float inv = trim_inv(K, f), inv_k = trim_inv(K, 0);
  const uint32_t nchunks = (uint32_t)((m / 8 + Q8_CC_CHUNK_UNITS - 1) / Q8_CC_CHUNK_UNITS);
  float* v = workspace;
  float* part = v + m;
  float* w = part + (int64_t)P * nchunks;
  const dim3 grid(nchunks < (uint32_t)Q8_CC_MAX_BLOCKS ? nchunks : (uint32_t)Q8_CC_MAX_BLOCKS);
  for_padded_peers(P, [&](auto pp) {
    constexpr int PP = decltype(pp)::value;
    hipLaunchKernelGGL(q8_cclip_init_kernel<PP>, grid, block, 0, s, recv, bps, (uint32_t)valid, f, K, live_mask, inv, v,
                       part, nchunks);
    for (int l = 0; l < iters; ++l) {
      const bool last = l == iters - 1;
      vcx_cclip_weights(part, nchunks, P, live_mask, tau, w, last ? weights : (float*)nullptr, s);
      if (last)
        hipLaunchKernelGGL((q8_cclip_step_kernel<PP, true>), grid, block, 0, s, recv, bps, (uint32_t)valid, P, live_mask,
                           inv_k, v, (const float*)w, part, nchunks, out_record, (unsigned long long*)nonfinite);
      else
        hipLaunchKernelGGL((q8_cclip_step_kernel<PP, false>), grid, block, 0, s, recv, bps, (uint32_t)valid, P,
                           live_mask, inv_k, v, (const float*)w, part, nchunks, out_record,
                           (unsigned long long*)nonfinite);
    }
  });
}

void vcx_q8_decode(const uint8_t* records, int64_t n, int64_t L, int P, void* out_bf16, hipStream_t s) {
  const uint32_t bps = (uint32_t)(L / P / Q8_BLOCK);
  hipLaunchKernelGGL(q8_decode_kernel, dim3(stream_grid((n + 7) / 8, 256, 2048)), dim3(256), 0, s, records, n, bps,
                     (bf16*)out_bf16);
}

int vcx_q8_block() { return Q8_BLOCK; }

int vcx_psgd_desc_size() { return (int)sizeof(MatDesc); }
int vcx_psgd_rows_per_block() { return 4 * PSGD_ROWS; }
int vcx_psgd_mtp_rows() { return PSGD_MTP_ROWS; }
int vcx_psgd_mtp_cols() { return PSGD_MTP_COLS; }
