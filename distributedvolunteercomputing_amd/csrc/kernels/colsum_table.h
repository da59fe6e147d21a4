// The deferred finish of many two-stage column sums in one pair of launches (norm_act.hip: colsum_stage1_many /
// colsum_stage2_many): a table of jobs passed BY VALUE as the kernel argument, like job_table.h. Job j sums the
// fp32 partial rows part[P, C] into the bf16 out[C]; stage 1 runs grid (ceil(Cmax / 64), NB, njobs) and writes
// stage[j][by][c] (layout [njobs][NB][Cmax]), stage 2 runs grid (ceil(Cmax / 64), njobs). A workgroup whose 64
// columns lie past its job's C returns.
// Plain C++ (no HIP types): the packing and the index arithmetic the kernels share are host-checkable
// (tests/csrc/colsum_table_check.cpp runs them under a sanitizer).
#pragma once
#include <stdint.h>

#include "job_table.h"

#if defined(__HIPCC__)
#define VCX_HD __host__ __device__
#else
#define VCX_HD
#endif

namespace vcx {

constexpr int COLSUM_NB = 32;  // stage-1 row chunks (== VCX_COLSUM_NB)

struct ColsumJob {
  const float* part;  // [P, C] fp32 partial rows
  int P, C;
  void* out;       // bf16 [C]
  int accumulate;  // out += sums instead of out = sums
  int zero_src;    // stage 1 leaves every element of part it read zeroed (a zero-at-rest accumulation row)
};

struct ColsumTable {
  int njobs;
  int Cmax;
  ColsumJob job[JOBS_MAX];  // 64 x 32 B + 8 B of the 4 KB kernel-argument limit
};

// Packs jobs[start ...] into `t` until the table is full; jobs without columns take no slot. Returns the index
// of the first job NOT consumed (== n when the list is done): the caller launches `t` when t->njobs > 0 and
// calls again from there. A job with P < 0, or a null pointer with something to read or write, returns -1.
inline int pack_colsum_jobs(const ColsumJob* jobs, int n, int start, ColsumTable* t) {
  t->njobs = 0;
  t->Cmax = 0;
  int i = start < 0 ? 0 : start;
  for (; i < n && t->njobs < JOBS_MAX; ++i) {
    const ColsumJob& in = jobs[i];
    if (in.C <= 0) continue;
    if (in.P < 0 || !in.out || (in.P > 0 && !in.part)) return -1;
    ColsumJob& o = t->job[t->njobs++];
    o = in;
    o.accumulate = in.accumulate ? 1 : 0;
    o.zero_src = in.zero_src ? 1 : 0;
    if (in.C > t->Cmax) t->Cmax = in.C;
  }
  return i;
}

inline int colsum_grid_x(const ColsumTable& t) { return (t.Cmax + 63) / 64; }

// fp32 elements of the stage buffer one launch pair of `t` writes and reads
inline int64_t colsum_stage_floats(const ColsumTable& t) { return (int64_t)t.njobs * COLSUM_NB * t.Cmax; }

// the most any table of a list needs: a full table of the list's widest job
inline int64_t colsum_stage_floats_max(const ColsumJob* jobs, int n) {
  int cmax = 0, live = 0;
  for (int i = 0; i < n; ++i)
    if (jobs[i].C > 0) {
      ++live;
      if (jobs[i].C > cmax) cmax = jobs[i].C;
    }
  return (int64_t)(live < JOBS_MAX ? live : JOBS_MAX) * COLSUM_NB * cmax;
}

// rows [r0, r1) of stage-1 chunk `by` of NB over P partial rows
VCX_HD inline void colsum_rows(int P, int by, int NB, int* r0, int* r1) {
  *r0 = (int)((int64_t)P * by / NB);
  *r1 = (int)((int64_t)P * (by + 1) / NB);
}

// offset of stage[slot][by][0] for rows of `width` columns (slot: the output, or the job of a table)
VCX_HD inline int64_t colsum_stage_row(int slot, int by, int NB, int width) {
  return ((int64_t)slot * NB + by) * width;
}

}  // namespace vcx
