// Planning of the per-matrix launch schedule (wrmf_schedule.h).  No HIP header: integers and vectors only.
#include "wrmf_schedule.h"

#include <algorithm>
#include <functional>
#include <queue>
#include <utility>

namespace rsparse_hip {

namespace {
// the workgroup slots of the whole machine (two workgroups of the rank-128 fp16 kernel are resident per CU): what the share
// of the split rule refers to
int ne_slots(int cus) { return 2 * std::max(cus, 1); }
}  // namespace

// grid (workgroups of 4 waves x rows_per_wave rows) for n_rows rows: about 32 visits per wave, small sets spread over the CUs first
int cgp_grid(int n_rows, int rows_per_wave) {
  if (n_rows <= 0) return 0;
  const long sets = ((long)n_rows + rows_per_wave - 1) / rows_per_wave;
  long per_wave = 32;
  const long spread = 4L * 512;
  if (sets < spread * per_wave) per_wave = (sets + spread - 1) / spread;
  if (per_wave < 1) per_wave = 1;
  return (int)((sets + 4 * per_wave - 1) / (4 * per_wave));
}
int cgp_visits(int n_rows, int rows_per_wave) {
  const long grid = cgp_grid(n_rows, rows_per_wave);
  if (grid <= 0) return 0;
  const long sets = ((long)n_rows + rows_per_wave - 1) / rows_per_wave;
  return (int)((sets + grid * 4 - 1) / (grid * 4));
}
int64_t cgp_loss_slots(int n_rows, int rows_per_wave) { return (int64_t)cgp_grid(n_rows, rows_per_wave) * 4; }

// Items of the deal: whole rows, and SEGMENTS of the rows that are too long to balance (the 5e5-non-zero item of the
// bench matrix is by itself an average workgroup's share; on a rank of an 8-GPU run it is eight shares).  A row
// whose cost exceeds half a share is cut into up to kNeMaxSeg runs of whole steps of about a quarter share; the
// workgroups that get the leading segments write their partial accumulators to an HBM scratch, the one with the
// last segment adds them in segment order and solves (wrmf_ne.hip).  List entry >= 0: a row; -(s + 1): segment s
// of the table {row, first non-zero, non-zeros, index within the row, segments of the row, scratch slot}.
// (round 6: the share is that of the slots of the whole machine even when there are fewer rows than slots -- the giant rows that
//  wrmf_cg_mf.hip leaves to this kernel are a few hundred: one workgroup per row left 40 % of the slots empty and every row as
//  long as its wave could stream it, 4.4 GB in 4.7 ms; cut to the machine's share they are segments of >= 64 steps)
// The CUT must not depend on the deal: the two list sets of a matrix (fine / one list per slot) share ONE segment table and
// one list of split rows -- cut by the fine rule only, a row was whole in the coarse lists and "split" in
// the table, and the collecting launch overwrote its solution with the sum of two stale partials (ranks up to 96, fewer
// than 512 long rows, a row of >= 2048 non-zeros: tests/test_bias.py caught it at the end of round 6).  Hence a cut is
// computed once per prefix and ne_deal takes it as it is.
NeCut ne_cut(const int32_t* order, const int32_t* col_ptrs, int n_prefix, int64_t fixed, int cus) {
  NeCut c;
  if (n_prefix <= 0) return c;
  auto len_of = [&](int r) { return (int64_t)(col_ptrs[order[r] + 1] - col_ptrs[order[r]]); };
  auto steps_of = [](int64_t len) { return (len + 15) / 16; };
  const int n_slots = ne_slots(cus);
  int64_t total = 0;
  for (int r = 0; r < n_prefix; r++) total += steps_of(len_of(r)) + fixed;
  const int64_t share = std::max<int64_t>(1, total / n_slots);
  c.items.reserve((size_t)n_prefix + 64);
  int n_seg = 0;
  for (int r = 0; r < n_prefix; r++) {
    const int64_t len = len_of(r);
    const int64_t st = steps_of(len);
    int parts = 1;
    if (n_slots >= 8 && 2 * (st + fixed) > share)
      parts = (int)std::min<int64_t>(std::min<int64_t>(kNeMaxSeg, st / 64), (4 * st + share - 1) / share);   // (a segment: >= 64 steps)
    if (parts < 2 || n_seg + parts > kNeMaxSegTotal) {
      c.items.push_back({st + fixed, order[r]});
      continue;
    }
    const int64_t per = (st + parts - 1) / parts;   // steps per segment
    const int slot = n_seg;
    const int made = (int)((st + per - 1) / per);
    int idx = 0;
    for (int64_t s0 = 0; s0 < st; s0 += per, idx++) {
      const int64_t n0 = s0 * 16, n1 = std::min(len, (s0 + per) * 16);
      c.segs.insert(c.segs.end(), {order[r], (int32_t)n0, (int32_t)(n1 - n0), idx, made, slot});
      c.items.push_back({steps_of(n1 - n0) + fixed, -(int32_t)(n_seg + 1)});
      n_seg++;
    }
    c.split_rows.push_back(-(int32_t)(slot + 1));   // its first segment
  }
  if (n_seg > 0)
    for (size_t i = 0; i <= c.split_rows.size(); i++) c.split_ptr.push_back((int32_t)i);
  // the order of the deal: longest processing time first
  std::stable_sort(c.items.begin(), c.items.end(), [](const NeCut::Item& x, const NeCut::Item& y) { return x.cost > y.cost; });
  return c;
}

// Row lists of the normal-equation kernel: one workgroup per CU, rows dealt longest-processing-time first (the rows
// arrive sorted by length, each goes to the least loaded workgroup; cost = the row's 16-non-zero steps + a fixed
// per-row solve).  Static lists make the per-row loss slots and the summation order deterministic.
NeDeal ne_deal(const NeCut& cut, int n_prefix, int cus, bool fine) {
  NeDeal d;
  const size_t n_items = cut.items.size();
  if (!n_items) return d;
  // `fine`: many more lists than workgroup slots (eight rows or more per list, up to 256 lists per CU; two workgroups of the
  // rank-128 fp16 kernel are resident per CU): the
  // hardware hands the next list to whichever slot frees up.  With exactly one list per slot the launch ended 13 % after
  // its mean workgroup (round 3, in-kernel counters): of the two workgroups that share a CU's SIMDs the one dispatched
  // first wins the issue arbitration and runs 27 % faster -- every workgroup of index < 256 took 63.9 M ticks for its
  // list, every one of index >= 256 81.4 M for an equal list, the last 17 M of them alone on its CU.
  // (`fine` = false: one list per slot, for the kernels that are resident once per CU -- no such asymmetry there, and a
  //  workgroup start costs more: XtX tiles into LDS; many short lists cost them 1..7 %)
  const int n_slots = ne_slots(cus);
  int n_wg = fine ? std::max(n_slots, std::min(n_prefix / 8, 256 * std::max(cus, 1))) : n_slots;
  n_wg = (int)std::min<size_t>((size_t)n_wg, n_items);   // (no empty lists)
  std::vector<int> owner(n_items);
  d.ptr.assign((size_t)n_wg + 1, 0);
  std::priority_queue<std::pair<int64_t, int>, std::vector<std::pair<int64_t, int>>, std::greater<>> heap;
  for (int w = 0; w < n_wg; w++) heap.push({0, w});
  for (size_t e = 0; e < n_items; e++) {
    auto top = heap.top();
    heap.pop();
    owner[e] = top.second;
    d.ptr[(size_t)top.second + 1]++;
    heap.push({top.first + cut.items[e].cost, top.second});
  }
  for (int w = 0; w < n_wg; w++) d.ptr[(size_t)w + 1] += d.ptr[(size_t)w];
  d.rows.resize(n_items);
  std::vector<int32_t> fill(d.ptr.begin(), d.ptr.end() - 1);
  for (size_t e = 0; e < n_items; e++) d.rows[(size_t)fill[(size_t)owner[e]]++] = cut.items[e].entry;
  return d;
}

bool plan_schedule(const int32_t* col_ptrs, int n_cols, int cus, int (*bucket_of)(int len), SchedulePlan& out) {
  out = SchedulePlan();
  const int n = n_cols;
  int max_len = 0;
  for (int i = 0; i < n; i++) {
    const int len = col_ptrs[i + 1] - col_ptrs[i];
    if (len < 0) return false;
    max_len = std::max(max_len, len);
  }
  out.max_len = max_len;
  if (n <= 0) {
    out.nec_is_ne = true;   // (both prefixes are empty)
    return true;
  }
  // counting sort by length, descending; ties keep ascending row order (deterministic).  Every counter of the plan is a
  // sum over the histogram: the column pointers are walked three times in all (maximum, histogram, placement)
  std::vector<int64_t> start((size_t)max_len + 2, 0);   // start[max_len - len + 1] = rows of length len, then its prefix sums
  for (int i = 0; i < n; i++) start[(size_t)(max_len - (col_ptrs[i + 1] - col_ptrs[i])) + 1]++;
  int cnt_b[6] = {0, 0, 0, 0, 0, 0};
  for (int len = max_len; len >= 0; len--) {
    const int cnt = (int)start[(size_t)(max_len - len) + 1];
    if (!cnt) continue;
    if (len > kTileNnz) { out.n_long += cnt; out.nnz_long += (int64_t)len * cnt; }
    if (len == 0) out.n_empty += cnt;
    if (len > kCholLongLen) out.n_chol_long += cnt;
    if (len > kCgMfMax) out.n_nec += cnt;
    if (len > 16) out.pair_first += cnt;
    if (len > kTeam4Max) out.team4_first += cnt;
    if (len > kTeam4WideMax) out.team4_wide_first += cnt;
    if (len > 32) out.gt32 += cnt;
    if (len > 48) out.gt48 += cnt;
    if (len > kCholLrMax) out.lr_first += cnt;
    else if (len >= 1) out.n_lr += cnt;
    const int b = bucket_of(len);
    cnt_b[b] += cnt;
    out.nnz[b] += (int64_t)len * cnt;
  }
  for (int b = 0; b < 6; b++) out.off[b + 1] = out.off[b] + cnt_b[b];
  for (size_t b = 1; b < start.size(); b++) start[b] += start[b - 1];
  out.order.resize((size_t)n);
  for (int i = 0; i < n; i++) out.order[(size_t)start[(size_t)(max_len - (col_ptrs[i + 1] - col_ptrs[i]))]++] = i;
  // streamed bucket (bucket 0): slot of each row's first non-zero in the per-sweep scratch, and the normal-equation lists --
  // many lists (`fine`), and the same rows and segments as one list per workgroup slot for the ranks whose kernel is resident
  // once per CU
  const int n_stream = out.off[1];
  if (n_stream > 0) {
    out.stream_off.assign((size_t)n_stream + 1, 0);
    for (int r = 0; r < n_stream; r++) {
      const int row = out.order[(size_t)r];
      out.stream_off[(size_t)r + 1] = out.stream_off[(size_t)r] + (col_ptrs[row + 1] - col_ptrs[row]);
    }
    out.cut = ne_cut(out.order.data(), col_ptrs, n_stream, 12, cus);
    out.fine = ne_deal(out.cut, n_stream, cus, true);
    out.coarse = ne_deal(out.cut, n_stream, cus, false);
  }
  // a second set of lists for a shorter prefix of the order.  Round 6: the rows beyond kCgMfMax non-zeros -- what is left to the
  // normal-equation kernel when wrmf_cg_mf.hip takes the rows of 513..kCgMfMax (rank 128, implicit conjugate gradient).
  // (Rounds 2-5: the rows beyond 64, for solver == CHOLESKY at rank 65..128 -- wrmf_chol_mf.hip has those now.)
  out.nec_is_ne = out.n_nec == n_stream;
  if (!out.nec_is_ne) {
    out.cut_nec = ne_cut(out.order.data(), col_ptrs, out.n_nec, 12, cus);
    out.nec = ne_deal(out.cut_nec, out.n_nec, cus, true);
  }
  return true;
}

}  // namespace rsparse_hip
