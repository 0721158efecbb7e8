// The per-matrix launch schedule, planned on the host: the length-sorted row order, the positions at which the launchers cut
// it, and the row lists of the normal-equation launch (wrmf_ne.hip).  Pure integer work on the column pointers -- this unit
// includes no HIP header, so that tests/test_schedule.py can build and check it without a device; wrmf_capi.cpp asks the
// device for its CU count, calls plan_schedule and uploads the vectors.
#pragma once
#include <cstdint>
#include <vector>

namespace rsparse_hip {

// Row lengths (non-zeros) at which the launchers cut the order; what each launcher does with its rows: wrmf_internal.h
constexpr int kTileNnz = 32;         // tile capacity (non-zeros per wave tile) the CG kernels are instantiated for
constexpr int kTeam4Max = 320;       // bucket 1 at rank 97..128: the rows of up to kTeam4Max non-zeros on 4-wave teams of 20 quads per wave (wrmf_cgq.hip)
constexpr int kTeam4WideMax = 384;   // ... and the rows of kTeam4Max + 1..kTeam4WideMax on 4-wave teams of 24 quads per wave
constexpr int kCholLrMax = 64;       // rows of 1..kCholLrMax non-zeros, implicit feedback, rank 98..128: the low-rank form of the exact solve (wrmf_chol_lr.hip)
constexpr int kCholLongLen = 4096;   // Cholesky: rows beyond it go to a second launch that sums the rank-one updates in two levels (wrmf_chol.hip)
constexpr int kCgMfMax = 16384;      // rank 128, implicit CG: the rows of kNeMinLen + 1 .. kCgMfMax non-zeros one wave per row (wrmf_cg_mf.hip), the rows beyond on wrmf_ne.hip
constexpr int kNeMaxSeg = 16;        // segments per split row
constexpr int kNeMaxSegTotal = 1024;   // ... per list set (186 MB of partial accumulators at most)

// The short-row launches of wrmf_cgp.hip: workgroups of 4 waves, a wave VISITS `rows_per_wave` rows of the list at a time (2, or 4
// in the four-rows form), visit v of wave w taking rows [(w + v * waves) * rows_per_wave, + rows_per_wave).  One loss slot per
// wave.  The launcher and the loss-slot count of wrmf_cgq.hip both call these, for the same range of rows.
int cgp_grid(int n_rows, int rows_per_wave = 2);     // workgroups: about 32 visits per wave, small sets spread over the CUs first
int cgp_visits(int n_rows, int rows_per_wave = 2);   // visits per wave: cgp_grid * 4 * cgp_visits * rows_per_wave >= n_rows
int64_t cgp_loss_slots(int n_rows, int rows_per_wave = 2);

// The CUT of the normal-equation launch over a prefix of the order: the items that are dealt to workgroups -- whole rows,
// and SEGMENTS of the rows that are too long to balance -- in the order of the deal (dearest first, stable).
struct NeCut {
  struct Item { int64_t cost; int32_t entry; };   // entry >= 0: a row; -(s + 1): segment s of the table
  std::vector<Item> items;
  std::vector<int32_t> segs;         // [nseg][6]: {row, first non-zero, non-zeros, index within the row, segments of the row, scratch slot}
  std::vector<int32_t> split_rows;   // lists of the COLLECT launch (one workgroup per split row): -(index of its first segment + 1)
  std::vector<int32_t> split_ptr;    // 0, 1, 2, ... (empty when no row is split)
  int nseg() const { return (int)(segs.size() / 6); }
};
// A DEAL of a cut: workgroup b owns rows[ptr[b], ptr[b + 1]); no list is empty
struct NeDeal {
  std::vector<int32_t> rows, ptr;
  int wg() const { return ptr.empty() ? 0 : (int)ptr.size() - 1; }
};

// order = every row, longest first; `fixed` = the per-row cost of the solve in 16-non-zero steps (CG: 12; the exact solve of
// solver == CHOLESKY: 72); cus = compute units of the device.  n_prefix <= 0: an empty cut.
NeCut ne_cut(const int32_t* order, const int32_t* col_ptrs, int n_prefix, int64_t fixed, int cus);
// `fine`: many more lists than workgroup slots; else one list per slot (see wrmf_schedule.cpp).  The same cut may be dealt both ways.
NeDeal ne_deal(const NeCut& cut, int n_prefix, int cus, bool fine);

struct SchedulePlan {
  int max_len = 0;
  int n_long = 0;         // rows of more than kTileNnz non-zeros: the first n_long entries of `order`
  int64_t nnz_long = 0;
  int n_empty = 0;
  std::vector<int32_t> order;   // every row, longest first; ties keep ascending row order (deterministic)
  int off[7] = {0, 0, 0, 0, 0, 0, 0};   // bucket b of the quad-layout CG kernels occupies order[off[b], off[b + 1])
  int64_t nnz[6] = {0, 0, 0, 0, 0, 0};
  // positions in `order` (it is longest first: the rows of at most L non-zeros are a suffix)
  int pair_first = 0;     // first row of at most 16 non-zeros
  int team4_first = 0;    // ... of at most kTeam4Max
  int team4_wide_first = 0;   // ... of at most kTeam4WideMax (<= team4_first)
  int gt32 = 0, gt48 = 0;   // rows of more than 32 / 48 non-zeros
  int lr_first = 0, n_lr = 0;   // rows of 1..kCholLrMax non-zeros: order[lr_first, lr_first + n_lr)
  int n_chol_long = 0;    // rows of more than kCholLongLen non-zeros
  int n_nec = 0;          // rows of more than kCgMfMax non-zeros
  std::vector<int64_t> stream_off;   // prefix sums of the streamed bucket's (bucket 0's) row lengths; empty without such rows
  // the streamed bucket's rows cut once and dealt twice; the rows beyond kCgMfMax (a shorter prefix) cut and dealt on their
  // own unless the two prefixes coincide (nec_is_ne: the lists are then the fine ones)
  NeCut cut, cut_nec;
  NeDeal fine, coarse, nec;
  bool nec_is_ne = false;
};

// bucket_of(len): the bucket of the quad-layout CG kernels a row of `len` non-zeros belongs to (wrmf_cgq.hip kBuckets), 0..5,
// non-decreasing as len falls.  False: col_ptrs decreases somewhere (nothing else about `out` is then meaningful).
bool plan_schedule(const int32_t* col_ptrs, int n_cols, int cus, int (*bucket_of)(int len), SchedulePlan& out);

}  // namespace rsparse_hip
