// Host check of the job-table packing (csrc/kernels/job_table.h), built by tests/test_job_table_cpu.py under
// -fsanitize=address,undefined. Every launch the packer forms is replayed on the host the way
// transpose_bf16_many_kernel walks it -- workgroup -> job by binary search -> tile -> elements -- on heap
// buffers of exactly the matrices' sizes, so a wrong offset or tile count is an out-of-bounds access the
// sanitizer reports, and a wrong mapping is a wrong transpose.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "job_table.h"

using vcx::JOBS_MAX;
using vcx::TransposeJob;
using vcx::TransposeTable;

#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);  \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

struct Mat {
  int R, Cc;
  std::vector<uint16_t> src, dst;
};

static void run_tile(const TransposeJob& j, int tile) {
  const int r0 = (tile / j.tiles_x) * 64, c0 = (tile % j.tiles_x) * 64;
  const uint16_t* s = (const uint16_t*)j.src;
  uint16_t* d = (uint16_t*)j.dst;
  for (int rr = 0; rr < 64; ++rr)
    for (int cc = 0; cc < 64; ++cc)
      if (r0 + rr < j.R && c0 + cc < j.Cc) d[(int64_t)(c0 + cc) * j.R + r0 + rr] = s[(int64_t)(r0 + rr) * j.Cc + c0 + cc];
}

// returns the launches made
static int run_list(std::vector<Mat>& ms) {
  std::vector<TransposeJob> jobs;
  uint16_t seed = 1;
  for (Mat& m : ms) {
    m.src.resize((size_t)m.R * m.Cc);
    m.dst.assign((size_t)m.R * m.Cc, 0xffff);
    for (uint16_t& v : m.src) v = seed = (uint16_t)(seed * 75u + 74u) & 0x7fff;
    TransposeJob j{};
    j.src = m.src.data();
    j.dst = m.dst.data();
    j.R = m.R;
    j.Cc = m.Cc;
    jobs.push_back(j);
  }
  const int n = (int)jobs.size();
  int launches = 0, packed = 0;
  for (int i = 0; i < n;) {
    TransposeTable t{};
    const int next = vcx::pack_transpose_jobs(jobs.data(), n, i, &t);
    CHECK(next > i && next <= n);
    CHECK(t.njobs >= 0 && t.njobs <= JOBS_MAX && t.first[0] == 0);
    i = next;
    if (t.njobs == 0) break;
    ++launches;
    packed += t.njobs;
    for (int j = 0; j < t.njobs; ++j) {
      const TransposeJob& o = t.job[j];
      CHECK(t.first[j + 1] - t.first[j] == ((o.R + 63) / 64) * ((o.Cc + 63) / 64));
      CHECK(o.tiles_x == (o.Cc + 63) / 64);
      CHECK(o.v8 == (o.R % 8 == 0 && o.Cc % 8 == 0 && ((uintptr_t)o.src | (uintptr_t)o.dst) % 16 == 0));
    }
    for (int b = 0; b < t.first[t.njobs]; ++b) {
      const int j = vcx::job_of_workgroup(t.first, t.njobs, b);
      CHECK(j >= 0 && j < t.njobs && t.first[j] <= b && b < t.first[j + 1]);
      run_tile(t.job[j], b - t.first[j]);
    }
  }
  int nonempty = 0;
  for (const Mat& m : ms) {
    nonempty += m.R > 0 && m.Cc > 0;
    for (int r = 0; r < m.R; ++r)
      for (int c = 0; c < m.Cc; ++c) CHECK(m.dst[(size_t)c * m.R + r] == m.src[(size_t)r * m.Cc + c]);
  }
  CHECK(packed == nonempty);
  return launches;
}

int main() {
  const int shapes[][2] = {{768, 768}, {64, 8}, {1, 136}, {200, 136}, {77, 50}, {0, 16}, {136, 1}, {65, 129}, {16, 0}};
  const int nshape = sizeof(shapes) / sizeof(shapes[0]);
  auto list = [&](int n, bool with_empty) {
    std::vector<Mat> ms;
    for (int k = 0; (int)ms.size() < n; ++k) {
      const int* s = shapes[k % nshape];
      if (!with_empty && (s[0] == 0 || s[1] == 0)) continue;
      ms.push_back(Mat{s[0], s[1], {}, {}});
    }
    return ms;
  };
  std::vector<Mat> ms = list(0, false);
  CHECK(run_list(ms) == 0);  // empty list: nothing launched
  ms = list(1, false);
  CHECK(run_list(ms) == 1);
  ms = list(JOBS_MAX, false);
  CHECK(run_list(ms) == 1);  // exactly the cap
  ms = list(JOBS_MAX + 1, false);
  CHECK(run_list(ms) == 2);  // cap + 1
  ms = list(3 * JOBS_MAX + 5, true);  // mixed shapes, empty matrices among them (they take no slot)
  CHECK(run_list(ms) >= 3);
  ms = {Mat{0, 8, {}, {}}, Mat{8, 0, {}, {}}};
  CHECK(run_list(ms) == 0);  // only empty matrices
  // a grid that would pass INT32_MAX is cut at the job that crosses it; one matrix alone over it is refused
  std::vector<TransposeJob> big(3);
  for (TransposeJob& j : big) {
    j = TransposeJob{};
    j.R = 64 * 40000;
    j.Cc = 64 * 40000;  // 1.6e9 tiles each
  }
  TransposeTable t{};
  CHECK(vcx::pack_transpose_jobs(big.data(), 3, 0, &t) == 1 && t.njobs == 1);
  CHECK(vcx::pack_transpose_jobs(big.data(), 3, 1, &t) == 2 && t.njobs == 1);
  big[0].R = big[0].Cc = 64 * 50000;  // 2.5e9 tiles
  CHECK(vcx::pack_transpose_jobs(big.data(), 3, 0, &t) == -1);
  std::printf("OK\n");
  return 0;
}
