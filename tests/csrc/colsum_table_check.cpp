// Host check of the column-sum job table (csrc/kernels/colsum_table.h), built by tests/test_colsum_table_cpu.py
// under -fsanitize=address,undefined. Every launch pair the packer forms is replayed on the host the way
// colsum_stage1_many_kernel / colsum_stage2_many_kernel walk it -- grid (ceil(Cmax / 64), NB, njobs), the early
// return past a job's C, four waves striding the chunk's rows, the [njobs][NB][Cmax] stage -- on heap buffers of
// exactly the sizes the host code allocates, so a wrong offset, grid or stage size is an out-of-bounds access the
// sanitizer reports, and a wrong mapping is a wrong sum. The data are small integers: every sum is exact in fp32,
// so the result does not depend on the order of the additions.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "colsum_table.h"

using vcx::COLSUM_NB;
using vcx::ColsumJob;
using vcx::ColsumTable;
using vcx::JOBS_MAX;

#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);  \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

struct Job {
  int P, C, accumulate, zero_src;
  std::vector<float> part, out, out0, want;  // out stands for the bf16 row (integers: no rounding to model)
};

// one stage-1 workgroup (bx, by, j) and one stage-2 workgroup (bx, j), as the kernels run them
static void stage1_workgroup(const ColsumTable& t, float* stage, int bx, int by, int j) {
  const ColsumJob& job = t.job[j];
  if (bx * 64 >= job.C) return;
  float* row = stage + vcx::colsum_stage_row(j, by, COLSUM_NB, t.Cmax);
  int r0, r1;
  vcx::colsum_rows(job.P, by, COLSUM_NB, &r0, &r1);
  CHECK(0 <= r0 && r0 <= r1 && r1 <= job.P);
  for (int lane = 0; lane < 64; ++lane) {
    const int c = bx * 64 + lane;
    if (c >= job.C) continue;
    float red = 0.f;
    for (int w = 0; w < 4; ++w)
      for (int r = r0 + w; r < r1; r += 4) {
        red += job.part[(int64_t)r * job.C + c];
        if (job.zero_src) const_cast<float*>(job.part)[(int64_t)r * job.C + c] = 0.f;
      }
    row[c] = red;
  }
}

static void stage2_workgroup(const ColsumTable& t, const float* stage, int bx, int j) {
  const ColsumJob& job = t.job[j];
  for (int lane = 0; lane < 64; ++lane) {
    const int c = bx * 64 + lane;
    if (c >= job.C) continue;
    const float* st = stage + vcx::colsum_stage_row(j, 0, COLSUM_NB, t.Cmax) + c;
    float acc = 0.f;
    for (int i = 0; i < COLSUM_NB; ++i) acc += st[(int64_t)i * t.Cmax];
    float* o = (float*)job.out;
    if (job.accumulate) acc += o[c];
    o[c] = acc;
  }
}

// returns the launch pairs made
static int run_list(std::vector<Job>& js) {
  std::vector<ColsumJob> jobs;
  uint32_t seed = 1;
  for (Job& j : js) {
    j.part.resize((size_t)j.P * j.C);
    for (float& v : j.part) v = (float)(int)((seed = seed * 1664525u + 1013904223u) >> 28) - 8.f;
    j.out0.resize(j.C);
    for (float& v : j.out0) v = (float)(int)((seed = seed * 1664525u + 1013904223u) >> 29);
    j.out = j.out0;
    j.want.assign(j.C, 0.f);
    for (int c = 0; c < j.C; ++c) {
      float s = 0.f;
      for (int r = 0; r < j.P; ++r) s += j.part[(size_t)r * j.C + c];
      j.want[c] = s + (j.accumulate ? j.out0[c] : 0.f);
    }
    ColsumJob o{};
    o.part = j.part.data();
    o.P = j.P;
    o.C = j.C;
    o.out = j.out.data();
    o.accumulate = j.accumulate;
    o.zero_src = j.zero_src;
    jobs.push_back(o);
  }
  const int n = (int)jobs.size();
  const int64_t stage_max = vcx::colsum_stage_floats_max(jobs.data(), n);
  int pairs = 0, packed = 0;
  for (int i = 0; i < n;) {
    ColsumTable t{};
    const int next = vcx::pack_colsum_jobs(jobs.data(), n, i, &t);
    CHECK(next > i && next <= n);
    CHECK(t.njobs >= 0 && t.njobs <= JOBS_MAX);
    i = next;
    if (t.njobs == 0) break;
    ++pairs;
    packed += t.njobs;
    int cmax = 0;
    for (int j = 0; j < t.njobs; ++j) cmax = t.job[j].C > cmax ? t.job[j].C : cmax;
    CHECK(t.Cmax == cmax && vcx::colsum_grid_x(t) == (cmax + 63) / 64);
    CHECK(vcx::colsum_stage_floats(t) <= stage_max);
    std::vector<float> stage((size_t)vcx::colsum_stage_floats(t), -1e30f);  // exactly what one pair may touch
    const int gx = vcx::colsum_grid_x(t);
    for (int j = 0; j < t.njobs; ++j)
      for (int by = 0; by < COLSUM_NB; ++by)
        for (int bx = 0; bx < gx; ++bx) stage1_workgroup(t, stage.data(), bx, by, j);
    for (int j = 0; j < t.njobs; ++j)
      for (int bx = 0; bx < gx; ++bx) stage2_workgroup(t, stage.data(), bx, j);
  }
  int live = 0;
  for (const Job& j : js) {
    live += j.C > 0;
    for (int c = 0; c < j.C; ++c) CHECK(j.out[c] == j.want[c]);
    if (j.zero_src)
      for (float v : j.part) CHECK(v == 0.f);
  }
  CHECK(packed == live);
  return pairs;
}

int main() {
  const int shapes[][2] = {{1, 3072}, {5, 8}, {37, 72}, {256, 768}, {513, 72}, {0, 64}, {3, 0}, {31, 65}, {33, 1}, {64, 128}};
  const int nshape = sizeof(shapes) / sizeof(shapes[0]);
  auto list = [&](int n, bool with_empty) {
    std::vector<Job> js;
    for (int k = 0; (int)js.size() < n; ++k) {
      const int* s = shapes[k % nshape];
      if (!with_empty && s[1] == 0) continue;
      Job j{};
      j.P = s[0];
      j.C = s[1];
      j.accumulate = k & 1;
      j.zero_src = (k >> 1) & 1;
      js.push_back(j);
    }
    return js;
  };
  std::vector<Job> js = list(0, false);
  CHECK(run_list(js) == 0);  // empty list: nothing launched
  js = list(1, false);
  CHECK(run_list(js) == 1);
  js = list(JOBS_MAX, false);
  CHECK(run_list(js) == 1);  // exactly the cap
  js = list(JOBS_MAX + 1, false);
  CHECK(run_list(js) == 2);  // cap + 1
  js = list(2 * JOBS_MAX + 2, true);  // mixed widths, jobs without columns among them (they take no slot)
  CHECK(run_list(js) >= 2);
  // refused: negative P, a missing output, missing partial rows with rows to read
  ColsumTable t{};
  float x[8] = {};
  ColsumJob bad{};
  bad.part = x;
  bad.out = x;
  bad.C = 8;
  bad.P = -1;
  CHECK(vcx::pack_colsum_jobs(&bad, 1, 0, &t) == -1);
  bad.P = 1;
  bad.out = nullptr;
  CHECK(vcx::pack_colsum_jobs(&bad, 1, 0, &t) == -1);
  bad.out = x;
  bad.part = nullptr;
  CHECK(vcx::pack_colsum_jobs(&bad, 1, 0, &t) == -1);
  bad.P = 0;  // no rows: nothing is read, the sum is zero
  CHECK(vcx::pack_colsum_jobs(&bad, 1, 0, &t) == 1 && t.njobs == 1);
  std::printf("OK\n");
  return 0;
}
