// One launch for many small jobs: a table of jobs passed BY VALUE as a kernel argument (no H2D copy; a hipGraph
// kernel node keeps its own copy), with one workgroup index space over the tiles of every job. first[j] is the
// first workgroup of job j and first[njobs] the grid size; a workgroup finds its job by binary search.
// Plain C++ (no HIP types): the packing below is host pointer arithmetic that a stand-alone program can include
// and run under a sanitizer (tests/csrc/job_table_check.cpp).
#pragma once
#include <stdint.h>

namespace vcx {

constexpr int JOBS_MAX = 64;  // per launch: 64 x 32-B jobs + 65 ints = 2.3 KB of the 4 KB kernel-argument limit

// dst[Cc, R] = src[R, Cc]^T (bf16) in 64 x 64 tiles
struct TransposeJob {
  const void* src;
  void* dst;
  int R, Cc;
  int tiles_x;  // column tiles: workgroup t of the job is tile (t / tiles_x, t % tiles_x)
  int v8;       // 1: the 16-B body (R, Cc multiples of 8, both pointers 16-B aligned), 0: the scalar body
};

struct TransposeTable {
  int njobs;
  int first[JOBS_MAX + 1];
  TransposeJob job[JOBS_MAX];
};

// Packs jobs[start ...] into `t` until the table is full (JOBS_MAX) or the grid would pass INT32_MAX; empty
// matrices take no slot. Returns the index of the first job NOT consumed (== n when the list is done): the
// caller launches `t` when t->njobs > 0 and calls again from there. A single job over INT32_MAX tiles is not
// representable and returns -1 (nothing packed).
inline int pack_transpose_jobs(const TransposeJob* jobs, int n, int start, TransposeTable* t) {
  t->njobs = 0;
  t->first[0] = 0;
  int i = start < 0 ? 0 : start;
  for (; i < n && t->njobs < JOBS_MAX; ++i) {
    const TransposeJob& in = jobs[i];
    if (in.R <= 0 || in.Cc <= 0) continue;
    const int64_t tx = ((int64_t)in.Cc + 63) / 64, ty = ((int64_t)in.R + 63) / 64;
    if (tx * ty > INT32_MAX) return -1;
    const int64_t end = (int64_t)t->first[t->njobs] + tx * ty;
    if (end > INT32_MAX) break;  // this job opens the next launch
    TransposeJob& o = t->job[t->njobs];
    o = in;
    o.tiles_x = (int)tx;
    o.v8 = (in.R % 8 == 0 && in.Cc % 8 == 0 && ((uintptr_t)in.src | (uintptr_t)in.dst) % 16 == 0) ? 1 : 0;
    t->first[++t->njobs] = (int)end;
  }
  return i;
}

// The job of workgroup b (0 <= b < t.first[t.njobs]): the j with first[j] <= b < first[j + 1].
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int job_of_workgroup(const int* first, int njobs, int b) {
  int lo = 0, hi = njobs;  // invariant: first[lo] <= b < first[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace vcx
