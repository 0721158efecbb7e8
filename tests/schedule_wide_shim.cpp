// extern "C" face of rsparse_amd/csrc/wrmf_schedule.cpp for tests/test_schedule_wide.py (compiled with g++ into pytest's tmp_path,
// like tests/schedule_shim.cpp): the two positions at which bucket 1 of the quad-layout CG kernels is cut at rank 97..128.
#include <cstdint>

#include "../rsparse_amd/csrc/wrmf_schedule.h"

using namespace rsparse_hip;

namespace {
// the row-length classes of wrmf_cgq.hip's bucket table (kBuckets[.][b].max_len)
int bucket_of(int len) { return len > 512 ? 0 : len > 256 ? 1 : len > 128 ? 2 : len > 64 ? 3 : len > 32 ? 4 : 5; }
}  // namespace

extern "C" {

// out = {kTeam4Max, kTeam4WideMax, team4_wide_first, team4_first, off[0..6]}; order_out: n_cols entries.  0: col_ptrs decreases
int sched_wide(const int32_t* col_ptrs, int n_cols, int cus, int64_t out[11], int64_t* order_out) {
  SchedulePlan p;
  if (!plan_schedule(col_ptrs, n_cols, cus, bucket_of, p)) return 0;
  int k = 0;
  out[k++] = kTeam4Max; out[k++] = kTeam4WideMax; out[k++] = p.team4_wide_first; out[k++] = p.team4_first;
  for (int b = 0; b < 7; b++) out[k++] = p.off[b];
  for (int i = 0; i < n_cols; i++) order_out[i] = p.order[(std::size_t)i];
  return 1;
}

}  // extern "C"
