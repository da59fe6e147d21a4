// The LDS-DMA ring toolkit shared by the GEMM kernels (gemm.hip, gemm_f.hip, gemm_ps.hip, gemm_wg.hip) and the
// ring variants of the attention kernels (attention.hip): the pieces where a mistake is silent, once.
//
// The ring. An operand slice is staged HBM -> LDS by LDS-DMA (a buffer load with the `lds` bit: no staging VGPRs,
// no ds_write) into one slot of a 3- or 4-slot ring while older slots are consumed. Each wave issues a fixed
// number of 1-KB pieces per slice, so "slice s + 1 has landed" is a COUNTED wait, s_waitcnt vmcnt(N) with N = the
// pieces of the younger slices, which stay in flight across the raw s_barrier that follows (a __syncthreads()
// would drain them). That only holds if nothing else moves vmcnt behind the kernel's back, hence:
//
//   * dma16 is inline asm, not __builtin_amdgcn_raw_ptr_buffer_load_lds / global_load_lds. hipcc (ROCm 7.2)
//     cannot tell a pending LDS-DMA from the slot a later LDS read touches, and its waitcnt pass drains vmcnt(0)
//     in front of such reads: 8 full drains per step in front of the ds_read_b64_tr_b16 fragment reads of the
//     earlier transposed-operand GEMM, the whole pipeline serialised (the "waves parked on vmcnt 73 % of the
//     time" of profiles/r2_gemm_tn.txt were those drains, not memory latency). Issued as asm the DMA is invisible
//     to that pass and is ordered only by the kernel's own wait_vm: 1165-1229 TF/s against the library's 808-978
//     (profiles/r5_gemm_wg.txt). The price: hipcc cannot count these loads either, so a kernel retires every
//     compiler-issued load (vmcnt(0)) before its first dma16 and does its own counting from there.
//   * the M0 hazard. The DMA takes its LDS byte address from M0, written by an s_mov right in front of it; the
//     hardware wants one wait state between an SALU write of M0 and an LDS-DMA, and hipcc's hazard recognizer
//     pads only instructions it generates itself, never the inside of an asm statement. The `s_nop 0` that opens
//     dma16's string is that wait state (the M0 write is the compiler's, through the "{m0}" constraint).
//   * the s_waitcnt immediate (gfx9 encoding): vmcnt[3:0] in bits 3:0 and vmcnt[5:4] in bits 15:14, expcnt in
//     6:4, lgkmcnt in 11:8. wait_vm<N> is vmcnt(N) lgkmcnt(0) with expcnt at its maximum (0x0070 | ...): it also
//     retires the wave's own ds_reads of the slot about to be overwritten. An N >= 16 put into the low field
//     alone would overflow into expcnt and wait for the wrong count, silently; the static_assert and the split
//     are the guard. wait_lgkm0 is the same with vmcnt at its maximum, 63 (0xC07F): no VM wait.
//   * barrier() is the bare s_barrier as a volatile asm with a memory clobber: the builtin is IntrNoMem, so the
//     compiler may move LDS reads across it, and __syncthreads() adds the vmcnt(0) this design avoids.
//
// The 64-byte-row image. A slot of the K-contiguous GEMMs holds rows of 32 bf16 (64 B, four 16-B chunks). A
// ds_read_b128 lane group (16 lanes: 16 rows, two chunks) must hit 16 distinct 16-B bank slots, so chunk c of
// row r is stored at chunk c ^ F[(r >> 2) & 3], F = {0, 2, 3, 1} (swz64). The DMA writes a wave's piece
// lane-linearly (lane l -> LDS bytes [16 l, 16 l + 16) of the piece: row l >> 2, physical chunk l & 3) and cannot
// scatter, so the swizzle is applied to each lane's SOURCE address instead: the lane that fills physical chunk
// l & 3 fetches logical chunk (l & 3) ^ F(row). The fragment read applies the same XOR to the LDS address
// (chunk64 for both).
//
// Tile order. Hardware block b runs on XCD b % 8, each XCD with its own L2. xcd_order gives every XCD a contiguous
// range of logical ids (bijective for any grid size), and grouped_tile walks the logical ids as blocks of GROUP_M
// row panels x all column panels in column-major order, so the ~32 tiles an XCD runs at once are a 4 x 8 block
// (4 A + 8 B panels in flight) instead of one A panel x 32 B panels (the whole B operand re-streamed by every
// XCD every round at large N).
#pragma once
#include "vcx_common.h"

namespace vcx {

typedef short sx8 __attribute__((ext_vector_type(8)));
typedef short sx4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// buffer resource words over [base, base + bytes) for an inline-asm "s" operand: wave-uniform base and size
// (SGPRs), 32-bit per-lane offsets; 48-bit base, stride 0, num_records in bytes, the flags word
// __builtin_amdgcn_make_buffer_rsrc callers in the tree use (a load past num_records returns 0)
__device__ __forceinline__ u32x4 desc(const void* base, unsigned bytes) {
  const uint64_t a = (uint64_t)base;
  return u32x4{(unsigned)a, (unsigned)(a >> 32) & 0xffffu, bytes, 0x00020000u};
}

// one 1-KB LDS-DMA piece: 16 B per lane from d + voff (per lane) + soff (wave-uniform) to lds + 16 lane
__device__ __forceinline__ void dma16(u32x4 d, int voff, int soff, const void* lds) {
  const unsigned m0 = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)lds;
  asm volatile("s_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(voff), "s"(d), "s"(soff), "{m0}"(m0)
               : "memory");
}
// ... with the literal soffset 0 (no SGPR: a different instruction encoding from dma16(d, voff, 0, lds))
__device__ __forceinline__ void dma16(u32x4 d, int voff, const void* lds) {
  const unsigned m0 = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)lds;
  asm volatile("s_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(voff), "s"(d), "{m0}"(m0) : "memory");
}

// s_waitcnt vmcnt(N) lgkmcnt(0), 0 <= N < 64
template <int N>
__device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt field");
  __builtin_amdgcn_s_waitcnt(0x0070 | (N & 15) | ((N >> 4) << 14));
}
__device__ __forceinline__ void wait_lgkm0() { __builtin_amdgcn_s_waitcnt(0xC07F); }
__device__ __forceinline__ void barrier() { asm volatile("s_barrier" ::: "memory"); }

// ---- the 64-byte-row image: F[(row >> 2) & 3] = {0, 2, 3, 1}, packed 2 bits per entry
__device__ __forceinline__ int swz64(int row) { return (0x78 >> (((row >> 2) & 3) * 2)) & 3; }
// chunk ^ F(row): the logical chunk a DMA lane fetches for physical chunk `chunk` of its row (lane l of a 16-row
// piece: row l >> 2, chunk l & 3), and equally the physical chunk a fragment read finds logical chunk `chunk` in
// (lane l: row l & 15 of a 16-row block, k chunk l >> 4; byte offset row * 64 + (chunk64(row, l >> 4) << 4)).
// It takes the row and chunk already split, and the offset sum stays in the kernels: helpers that split the lane
// id themselves, or that formed the whole fragment offset, were simplified on their own before inlining and came
// out as different instruction sequences in gemm_nt_kernel<EPI_DGELU> and in every gemm_f_kernel.
__device__ __forceinline__ int chunk64(int row, int chunk) { return chunk ^ swz64(row); }

// ---- tile order: logical id of hardware block bid of nwg (blocks bid, bid + 8, ... -> consecutive ids)
__device__ __forceinline__ int xcd_order(int bid, int nwg) {
  const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}
// logical id wg -> (row panel tm, column panel tn) of a tilesM x tilesN grid, GROUP_M = 4 row panels per block
__device__ __forceinline__ void grouped_tile(int wg, int tilesM, int tilesN, int& tm, int& tn) {
  constexpr int GROUP_M = 4;
  const int per_group = GROUP_M * tilesN;
  const int gfirst = (wg / per_group) * GROUP_M;
  const int gsize = min(tilesM - gfirst, GROUP_M);
  tm = gfirst + (wg % per_group) % gsize;
  tn = (wg % per_group) / gsize;
}

}  // namespace vcx
