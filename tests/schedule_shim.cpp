// extern "C" face of rsparse_amd/csrc/wrmf_schedule.cpp for tests/test_schedule.py, which compiles the two with g++ into
// pytest's tmp_path.  Not part of the library: it exports no rsparse_hip_* symbol.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../rsparse_amd/csrc/wrmf_schedule.h"

using namespace rsparse_hip;

namespace {
// the row-length classes of wrmf_cgq.hip's bucket table (kBuckets[.][b].max_len)
int bucket_of(int len) { return len > 512 ? 0 : len > 256 ? 1 : len > 128 ? 2 : len > 64 ? 3 : len > 32 ? 4 : 5; }

template <class V>
int64_t copy_out(const V& v, int64_t* out, int64_t cap) {
  for (std::size_t i = 0; i < v.size() && (int64_t)i < cap; i++) out[i] = (int64_t)v[i];
  return (int64_t)v.size();
}
int64_t copy_items(const NeCut& c, bool cost, int64_t* out, int64_t cap) {
  for (std::size_t i = 0; i < c.items.size() && (int64_t)i < cap; i++) out[i] = cost ? c.items[i].cost : (int64_t)c.items[i].entry;
  return (int64_t)c.items.size();
}
}  // namespace

extern "C" {

// nullptr: col_ptrs decreases somewhere
void* sched_plan(const int32_t* col_ptrs, int n_cols, int cus) {
  SchedulePlan* p = new SchedulePlan();
  if (plan_schedule(col_ptrs, n_cols, cus, bucket_of, *p)) return p;
  delete p;
  return nullptr;
}
void sched_free(void* h) { delete static_cast<SchedulePlan*>(h); }

void sched_counters(const void* h, int64_t out[32]) {
  const SchedulePlan& p = *static_cast<const SchedulePlan*>(h);
  int k = 0;
  out[k++] = p.max_len; out[k++] = p.n_long; out[k++] = p.nnz_long; out[k++] = p.n_empty;
  for (int b = 0; b < 7; b++) out[k++] = p.off[b];
  for (int b = 0; b < 6; b++) out[k++] = p.nnz[b];
  out[k++] = p.pair_first; out[k++] = p.team4_first; out[k++] = p.gt32; out[k++] = p.gt48;
  out[k++] = p.lr_first; out[k++] = p.n_lr; out[k++] = p.n_chol_long; out[k++] = p.n_nec; out[k++] = p.nec_is_ne ? 1 : 0;
}

// copies at most cap entries of vector `which`, returns its length
int64_t sched_vector(const void* h, int which, int64_t* out, int64_t cap) {
  const SchedulePlan& p = *static_cast<const SchedulePlan*>(h);
  const NeCut& c = which >= 20 ? p.cut_nec : p.cut;
  switch (which) {
    case 0: return copy_out(p.order, out, cap);
    case 1: return copy_out(p.stream_off, out, cap);
    case 10: case 20: return copy_items(c, true, out, cap);
    case 11: case 21: return copy_items(c, false, out, cap);
    case 12: case 22: return copy_out(c.segs, out, cap);
    case 13: case 23: return copy_out(c.split_rows, out, cap);
    case 14: case 24: return copy_out(c.split_ptr, out, cap);
    case 15: return copy_out(p.fine.rows, out, cap);
    case 16: return copy_out(p.fine.ptr, out, cap);
    case 17: return copy_out(p.coarse.rows, out, cap);
    case 18: return copy_out(p.coarse.ptr, out, cap);
    case 25: return copy_out(p.nec.rows, out, cap);
    case 26: return copy_out(p.nec.ptr, out, cap);
  }
  return -1;
}

}  // extern "C"
