// Launchers of kernels/compress.hip (top-k + error feedback, PowerSGD, q8 block quantisation).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

void vcx_topk_ef(const void* g, int g_is_bf16, float* e, int64_t n, int k, int* st, uint32_t* hist,
                 int32_t* idx_out, void* val_out, int val_is_bf16, hipStream_t s);
int vcx_topk_hist_words();  // size of the histogram scratch topk_ef needs (uint32 words)
// dense[idx] += scale * val over m pairs; indices outside [0, n) are dropped
void vcx_scatter_add(const int32_t* idx, const void* val, int val_is_bf16, int64_t m, float scale, float* dense,
                     int64_t n, hipStream_t s);
// same over P all-gathered wire blocks of L int32 words each: k indices then k packed values
void vcx_scatter_add_packed(const int32_t* wire, int P, int k, int64_t L, int val_is_bf16, float scale, float* dense,
                            int64_t n, hipStream_t s);
// M += G (bf16, G may be null) fused with P = M Q; lazy: first M -= P_prev Q^T (P_prev = P on entry)
void vcx_psgd_mq(const void* desc, int nmat, int nblocks, float* M, const void* G, const float* Q, float* P, int rank,
                 int lazy, hipStream_t s);
void vcx_psgd_mtp(const void* desc, int nmat, int nblocks, const float* M, const float* P, float* Q, int rank,
                  hipStream_t s);
// CholeskyQR2 of every matrix's P (blocks of psgd_orth_rows() rows); G: 2 * nmat * rank^2 floats scratch
void vcx_psgd_orth(const void* desc, int nmat, int nblocks, float* P, float* G, int rank, hipStream_t s);
int vcx_psgd_orth_rows();
void vcx_psgd_reconstruct(const void* desc, int nmat, int nblocks, float* M, const float* P, const float* Q,
                          void* out, int rank, int update_m, hipStream_t s);
void vcx_ef_accum(const void* g, float* e, int64_t n, hipStream_t s);
// q8 (8-bit codes in blocks of vcx_q8_block() elements, one fp32 scale per block). A record of a
// shard of m elements is m int8 codes then m / 128 fp32 scales. L = P m >= n, m a multiple of 128.
// encode: v = e + g, codes and scales of the P shards into `wire` (P records), e = v - decoded
void vcx_q8_encode(const void* g, int g_is_bf16, float* e, int64_t n, int64_t L, int P, uint8_t* wire, hipStream_t s);
// recv: P records of one shard; out_record = encode(avg_scale * sum over p = 0..P-1 of decoded record p)
void vcx_q8_reduce(const uint8_t* recv, int P, int64_t m, float avg_scale, uint8_t* out_record, hipStream_t s);
// recv: P records of one shard; out_record = encode(trimmed mean over the rows of live_mask of the decoded
// records), the rule of ops/robust.py with f = min(trim, (K - 1) / 2); elements at or beyond `valid` do not
// vote and encode as +0; a non-finite result becomes +0 and adds 1 to *nonfinite. counts (P int64, += the
// elements at which a live row was trimmed) and nonfinite (1 int64) may be null. Throws
// std::invalid_argument, before anything is launched, for a call the kernel cannot take.
void vcx_q8_trimmed_reduce(const uint8_t* recv, int P, int64_t m, int trim, uint32_t live_mask, int64_t valid,
                           uint8_t* out_record, int64_t* counts, int64_t* nonfinite, hipStream_t s);
int vcx_q8_trimmed_reduce_max_blocks();  // the launcher's grid cap (blocks of 256 lanes, 8 elements per lane)
// recv: P records of one shard; out_record = encode(centered clipping over the rows of live_mask of the decoded
// records): the rule of ops/robust.py on the fp32 rows, `iters` (1..8) updates with radius tau (finite, >= 0; 0:
// adaptive), started at their median; elements at or beyond `valid` do not vote and encode as +0; a non-finite
// result becomes +0 and adds 1 to *nonfinite. weights (P floats: the last update's) and nonfinite (1 int64) may be
// null. workspace: vcx_q8_cclip_workspace_floats(P, m) floats, 16-byte aligned, holds no state between calls.
// 2 iters + 1 launches on s (one with a single voter). Throws std::invalid_argument, before anything is launched,
// for a call the kernels cannot take.
void vcx_q8_cclip_reduce(const uint8_t* recv, int P, int64_t m, uint32_t live_mask, int64_t valid, float tau, int iters,
                         uint8_t* out_record, float* weights, int64_t* nonfinite, float* workspace, hipStream_t s);
int64_t vcx_q8_cclip_workspace_floats(int P, int64_t m);
int vcx_q8_cclip_max_workgroups();  // workgroup cap of the passes: more chunks of 4096 elements are strided over
// records: P records (L elements); writes the first n decoded values as bf16
void vcx_q8_decode(const uint8_t* records, int64_t n, int64_t L, int P, void* out_bf16, hipStream_t s);
int vcx_q8_block();
int vcx_psgd_desc_size();
// block tables: psgd_mq / psgd_reconstruct take rows_per_block rows per block; psgd_mtp blocks are
// (row slab of mtp_rows) x (column chunk of mtp_cols)
int vcx_psgd_rows_per_block();
int vcx_psgd_mtp_rows();
int vcx_psgd_mtp_cols();
