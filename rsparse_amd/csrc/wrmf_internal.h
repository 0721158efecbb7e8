// Internal interface between the C-ABI layer (wrmf_capi.cpp) and the kernel launchers
// (wrmf_kernels.hip).  Not installed; the public boundary is include/rsparse_wrmf_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>

#include "wrmf_schedule.h"

namespace rsparse_hip {

// Constants of the reference (inst/include/wrmf.hpp:20-22, inst/include/nnls.hpp:8), once per type
constexpr float kCgTol = 1e-10f;      // CG_TOL: the conjugate-gradient exit on the squared residual
constexpr double kCgTolD = 1e-10;
constexpr int kScdMaxIter = 10000;    // SCD_MAX_ITER: sweeps of the coordinate descent (NNLS)
constexpr float kScdTol = 1e-4f;      // SCD_TOL: its exit on the largest relative coordinate change of a sweep
constexpr double kScdTolD = 1e-4;
constexpr float kNnlsEps = 1e-16f;    // EPS: added to the diagonal of XtX and to the denominators
constexpr double kNnlsEpsD = 1e-16;

// One list set of the normal-equation launch (wrmf_ne.hip), on the device: the rows of a prefix of the order dealt to `wg`
// workgroups, longest processing time first -- workgroup b owns rows[ptr[b], ptr[b + 1]); an entry >= 0 is a row, -(s + 1)
// segment s of the rows that are split across workgroups (planned by wrmf_schedule.cpp: NeCut / NeDeal).  A view: the
// arrays belong to the handle (rsparse_hip_csc::owned), and list sets of one handle may share them.
struct NeListSet {
  const int32_t* rows = nullptr;
  const int32_t* ptr = nullptr;
  int wg = 0;
  int entries = 0;                       // list entries = rows that are not split + segments
  const int32_t* segs = nullptr;         // [nseg][6]: segments of the rows split across workgroups
  int nseg = 0;
  const int32_t* split_rows = nullptr;   // lists of the COLLECT launch (one workgroup per split row): -(index of its first segment + 1)
  const int32_t* split_ptr = nullptr;    // 0, 1, 2, ...
  int nsplit = 0;
};

// Device-resident CSC + launch schedule.
struct DevCSC {
  int n_rows = 0;  // = number of entities on the fixed side (columns of X)
  int n_cols = 0;  // = rows solved
  int64_t nnz = 0;
  const int32_t* col_ptrs = nullptr;
  const int32_t* row_idx = nullptr;
  const float* vals = nullptr;
  // rows with more than `short_max` non-zeros, longest first (solved one workgroup per row): the first n_long entries of q_order
  int n_long = 0;
  int short_max = 0;  // tile capacity T the schedule was built for
  int max_len = 0;
  // quad-layout CG schedule: every row, longest first; bucket b occupies order[q_off[b], q_off[b+1])
  // (bucket table: wrmf_cgq.hip kBuckets)
  const int32_t* q_order = nullptr;
  int q_off[7] = {0, 0, 0, 0, 0, 0, 0};
  int q_cfg = 0;
  int q_pair_first = 0;   // position in q_order of the first row with at most 16 non-zeros (wrmf_cgp.hip: two rows per wave)
  int q_team4_first = 0;  // ... of the first row with at most kTeam4Max non-zeros (bucket 1's 4-wave launch at rank 97..128)
  int q_team4_wide_first = 0;  // ... with at most kTeam4WideMax non-zeros (bucket 1's wide 4-wave launch in front of it)
  int64_t q_nnz[6] = {0, 0, 0, 0, 0, 0};
  const int64_t* q_stream_off = nullptr;  // prefix sums of the streamed bucket's row lengths (device)
  int q_n_chol_long = 0;   // rows of more than kCholLongLen non-zeros (a prefix of q_order)
  int q_gt32 = 0;                   // rows of more than 32 non-zeros
  int q_gt48 = 0;                   // ... of more than 48
  int q_lr_first = 0, q_n_lr = 0;   // rows of 1..kCholLrMax non-zeros: q_order[q_lr_first, q_lr_first + q_n_lr)
  // normal-equation kernel (wrmf_ne.hip): the long rows (bucket 0) as many lists (two workgroups per CU pick them up) ...
  NeListSet q_ne;
  // ... and the same rows and segments dealt to one list per workgroup slot (kernels resident once per CU)
  NeListSet q_ne1;
  // the same lists for the rows beyond kCgMfMax non-zeros (a shorter prefix of q_order): the normal-equation launch beside
  // wrmf_cg_mf.hip, and solver == CHOLESKY's when wrmf_chol_mf.hip does not run; = q_ne when the two prefixes coincide
  int q_n_nec = 0;      // rows of more than kCgMfMax non-zeros (a prefix of q_order)
  NeListSet q_nec;
  int64_t nnz_long = 0;
  int n_empty = 0;
  // rsparse_hip_csc_freeze_values: the caller promises that the values do not change while the flag is set; the statistics of
  // the values that the fp16 kernels scale their operands by (max c, "some c < 1": launch_ne_stats) are then scanned once per
  // handle instead of once per half-iteration.  vstats: 2 words on the device, valid once vstats_valid
  mutable bool vals_frozen = false;
  mutable bool vstats_valid = false;
  mutable unsigned* vstats = nullptr;
  mutable hipStream_t vstats_stream = nullptr;   // the stream whose scan wrote vstats: only work queued on it is ordered behind that scan
};

struct AlsArgs {
  const int32_t* col_ptrs;
  const int32_t* row_idx;
  const float* vals;
  const float* X;    // k x n_rows, ld = k
  float* Y;          // k x n_cols, ld = k
  const float* XtX;  // k x k (implicit) or nullptr
  const int32_t* long_rows;
  int n_long;
  int n_cols;
  int k;
  int cg_steps;
  float lambda;        // lambda as the kernels use it in fp32 (regulariser inside the explicit system)
  double lambda_loss;  // lambda of the loss term (double, wrmf_implicit.hpp:259-261)
  int dynamic_lambda;
  double* loss_partials;  // one double per wave (short kernel) / per workgroup (long kernel)
  // Cholesky: fail_counter[0] = rows whose factorisation met a non-positive pivot (they are appended to fail_rows, at most
  // fail_cap of them, and re-solved by the general solver, wrmf_lu.hip), fail_counter[1] = rows that one could not solve either
  int* fail_counter;
  int* fail_rows;
  int fail_cap;
  // streamed CG rows: scratch [cg_steps+1][stream_nnz] for the per-non-zero dot products of every sweep,
  // stream_off[r] = first slot of the r-th streamed row (rows in schedule order); nullptr = re-gather for the loss
  const float* zero_row;  // >= 128 zero floats: what the padding slots of a gather read
  // user/item biases with implicit feedback (Cholesky / NNLS kernels only; all nullptr otherwise):
  const float* rhs_vals;   // per non-zero: coefficient of x_j in the right-hand side, c - x_b (c - 1)  (default: vals)
  const float* loss_tgt;   // per non-zero: target of the loss term, 1 - global_bias - x_b               (default: loss_tgt_const)
  float loss_tgt_const;    // target of the loss term when loss_tgt is nullptr: 1, or 1 - global_bias (wrmf_implicit.hpp:262-264)
  const float* rhs_init;   // k floats added to every right-hand side; non-null also means "solve empty rows too"
  // implicit feedback, conjugate gradient with a global bias (cg_solver_implicit_global_bias, wrmf_implicit.hpp:35-57):
  // gbias != 0 selects it; rhs_init = global_bias_base, loss_tgt_const = 1 - gbias.  The normal-equation kernel's rows
  // (wrmf_ne.hip) take the extra term of their first residual, global_bias_base - gbias X_nnz (c - 1), from ne_r0
  // [ne_r0_slot[row]][k] (launch_gb_row_terms)
  float gbias;
  const float* ne_r0;
  const int32_t* ne_r0_slot;
  float* tscr;
  const int64_t* stream_off;
  int64_t stream_nnz;
  // Cholesky: rows of more than kCholLongLen non-zeros = the first n_chol_long entries of the length-sorted row order
  const int32_t* chol_long_rows;
  int n_chol_long;
  // ... and the main launch's rows as ranges of the same order (nullptr: it walks every column and skips what it does
  // not own): [chol_first, chol_first + chol_n_main) = the rows of more than kCholLrMax non-zeros that no other launch
  // takes, then, when the low-rank kernel stands down, the short rows behind them; the empty rows
  // [chol_empty_first, n_cols) always
  const int32_t* chol_list;
  int chol_first, chol_n_main, chol_empty_first;
  // Cholesky, short rows: lr_rows = the n_lr rows of 1..kCholLrMax non-zeros; lr_flags (device word, nullable): 0 = the
  // low-rank kernel solves them and wrmf_chol.hip's skips them, else the other way round; lr_M = 3 x 128 x 128 floats
  const int32_t* lr_rows;
  int n_lr;
  int lr_n_gt32, lr_n_gt16;   // how many of them (a prefix: the list is longest first) have more than 32 / 16 non-zeros; -1 = unknown
  int lr_n_gt48;              // ... more than 48
  float* nnls_lhs;            // NNLS, rank 65..128: chol_loss_slots(n_cols) x 128 x 128 floats -- lhs of the workgroup's row (nullable: lhs in LDS)
  const int32_t* nnls_order;  // NNLS, one wave per row: the rows longest first (nullable: natural order) -- a row's cost is its sweep count,
                              // which grows with its length, and what runs last decides when the launch ends
  int lrx;                    // explicit feedback: lr_rows are solved by the push-through wave kernel (wrmf_chol_lr.hip) and the k x k kernels skip them
  unsigned* lr_flags;
  float* lr_M;
  // rows split across workgroups: segment table, per-segment partial accumulators (kNeSegFloats floats each) and flags
  const int32_t* ne_segs;
  float* ne_seg_scratch;
  int* ne_seg_flags;
  int ne_chol;                   // long rows through wrmf_ne.hip with the exact solve instead of CG (solver == CHOLESKY)
  int ne_chol_min;               // ... the rows of more than this many non-zeros (wrmf_chol.hip skips them)
  const unsigned* ne_stats;      // implicit NE launches: {bits of max |x|, bits of max c, any c < 1} (launch_ne_stats), or nullptr
  const float* mf_XtX;           // wrmf_chol_mf.hip, implicit feedback: XtX padded to 128 x 128 (identity beyond the rank); = XtX at rank 128
  const unsigned* wave_stats;    // the same block for the wave-per-row kernels at rank 33..64 (operand scales of their matrix-core assembly), or nullptr
};

struct QSchedule {
  const int32_t* order;
  int off[7];
  int pair_first;   // see DevCSC::q_pair_first
  int team4_first;  // see DevCSC::q_team4_first; = off[2] when bucket 1 runs on the 8-wave kernel alone (global bias)
  int team4_wide_first;  // see DevCSC::q_team4_wide_first; = off[2] in the same case
  bool pair_wide;   // the last bucket's rows of 17..32 non-zeros two per wave as well (cgp_wide_supported), else one per wave
  bool pair_quad = false;   // the last bucket's rows of at most 16 non-zeros four per wave (cgp_quad_supported), else two per wave
  int cfg;  // geometry the schedule was built for (see wrmf_cgq.hip kBuckets)
  NeListSet ne;   // the list set of this call's normal-equation launch (one of DevCSC::q_ne / q_ne1 / q_nec)
  const int32_t* mf_rows = nullptr;   // wrmf_cg_mf.hip's rows of the first bucket (the normal-equation lists above then hold the giant rows only)
  int mf_n = 0;
};
int cgq_default_cfg();
void cgq_set_launch_mode(int mode);   // rsparse_hip_set_launch_mode
int cgq_num_buckets();               // 6
int cgq_bucket_wpr(int cfg, int b);  // waves per row of bucket b (0 = unused)
int cgq_bucket_capq(int cfg, int b);
int cgq_bucket_waves(int cfg, int b);  // waves per workgroup of bucket b's kernel
int cgq_bucket_stream(int cfg, int b);
int cgq_bucket_grid(int n_rows, int bucket, int cfg);
// bucket 1 at rank 97..128: the rows of up to kTeam4Max (wrmf_schedule.h) non-zeros on 4-wave teams of 20 quads per wave (wrmf_cgq.hip)
int cgq_team4_grid(int n_rows);
// ... and the rows of kTeam4Max + 1..kTeam4WideMax on 4-wave teams of 24 quads per wave
int cgq_team4_wide_grid(int n_rows);
int cgq_bucket_of(int len, int cfg);
size_t cgq_loss_slots(const QSchedule& q, int k, bool implicit);
// the rows of at most 16 non-zeros of the last bucket, two per wave (wrmf_cgp.hip): rank 65..128, implicit feedback;
// its rows of 17..32 non-zeros too ("wide") at rank 128 without a global bias; under the same conditions its rows of at
// most 16 non-zeros four per wave ("quad")
bool cgp_supported(int k, bool implicit);
bool cgp_wide_supported(int k, bool implicit, bool gbias);
bool cgp_quad_supported(int k, bool implicit, bool gbias);
enum CgpForm { kCgpPair = 0, kCgpWide = 1, kCgpQuad = 2 };
inline int cgp_rows_per_wave(CgpForm form) { return form == kCgpQuad ? 4 : 2; }
// (grid, visits per wave and loss slots of a launch: cgp_grid / cgp_visits / cgp_loss_slots of wrmf_schedule.h)
hipError_t launch_als_cgp(const AlsArgs& a, const int32_t* rows, int n_rows, CgpForm form, size_t loss_slot0, hipStream_t s,
                          hipEvent_t* ev_slot);
// long rows (bucket 0) by one-pass normal equations on the matrix cores (wrmf_ne.hip) instead of the streamed CG kernel
bool ne_supported(int k);
constexpr int kNeMinLen = 512;       // its rows: more non-zeros than the largest resident bucket of wrmf_cgq.hip holds
// (kNeMaxSeg segments per split row, kNeMaxSegTotal per list set -- 186 MB of partial accumulators at most: wrmf_schedule.h)
constexpr int kNeSegFloats = 4 * (11 * 16 * 64 + 128 + 2);   // per segment: 4 waves x (<= 11 accumulator tiles + b + sum c)
// absmax_hint (nullable, device float): max |X| supplied by the caller -- X is then not scanned
// cached_vstats (nullable, 2 device words = stats[1..2] of an earlier scan of the same values): the values are not read;
// save_vstats (nullable): receives stats[1..2] of this scan
hipError_t launch_ne_stats(const float* X, int64_t nx, const float* vals, int64_t nnz, unsigned* stats, hipStream_t s,
                           const float* absmax_hint = nullptr, const unsigned* cached_vstats = nullptr,
                           unsigned* save_vstats = nullptr);
hipError_t launch_als_ne(const AlsArgs& a, const QSchedule& q, bool implicit, double* row_loss, hipStream_t s,
                         hipEvent_t* ev_slot = nullptr);
// global bias + conjugate gradient: out[r][:] = base - gbias * sum_j (c_j - 1) x_j for the n rows `rows` (one workgroup
// per row), slot_of_row[rows[r]] = r
hipError_t launch_gb_row_terms(const AlsArgs& a, const int32_t* rows, int n, float* out, int32_t* slot_of_row, hipStream_t s);
// ev (optional): 7 events, ev[b] before bucket b's kernel, ev[6] after the last one
hipError_t launch_als_cgq(const AlsArgs& a, const QSchedule& q, bool implicit, hipStream_t s, hipEvent_t* ev = nullptr);

// (kTileNnz, the tile capacity the CG kernels are instantiated for: wrmf_schedule.h)
constexpr int kWavesPerWG = 4;
constexpr int kRowsPerWGShort = 64;  // rows handed to one short-row workgroup
constexpr int kRowsPerWGLong = 8;    // rows handed to one long-row workgroup

constexpr int kCholMaxGrid = 256 * 96;  // Cholesky / NNLS workgroups (grid-stride over rows); many more than slots (3 per CU): the hardware deals them as slots free up

// number of loss partial slots each launcher writes
size_t cg_loss_slots(int n_cols, int n_long);
size_t chol_loss_slots(int n_cols);

// Optional per-kernel timing: when `ev` is non-null the launchers record ev[0] before the first
// kernel, ev[1] between kernels and ev[2] after the last one (all on stream s).
hipError_t launch_als_cg(const AlsArgs& a, bool implicit, hipStream_t s, hipEvent_t* ev = nullptr);
// register-blocked Cholesky (wrmf_chol.hip); rows beyond kCholLongLen non-zeros go to a second launch that sums the
// rank-one updates in two levels (see there); its workgroups' loss slots follow the main launch's
constexpr int kCholLongGrid = 512;
// rows of 1..kCholLrMax non-zeros, implicit feedback, rank 98..128: the low-rank form of the exact solve (wrmf_chol_lr.hip)
constexpr int kCholLrGrid = 65536;   // (many more than workgroup slots: the hardware deals them as slots free up, see ne_deal, wrmf_schedule.cpp)
size_t chol2_loss_slots(int n_cols);
bool chol_lr_supported(const AlsArgs& a, bool implicit);
bool chol_lrx_supported(const AlsArgs& a, bool implicit);
hipError_t launch_als_chol_lrx(const AlsArgs& a, const int32_t* rows, int n_rows, const unsigned* stats, int loss_slot0,
                               hipStream_t s, hipEvent_t* ev_slot);
hipError_t launch_als_chol_lr(const AlsArgs& a, const int32_t* rows, int n_rows, float* M, float* Mt, unsigned* flags,
                              int loss_slot0, hipStream_t s, hipEvent_t* ev_slot = nullptr);
hipError_t launch_als_chol2(const AlsArgs& a, bool implicit, hipStream_t s, hipEvent_t* ev = nullptr);
// rank <= 64: the main launch of the exact solve as one wave per row (wrmf_chol_wave.hip); same rows, same loss slots
bool chol_wave_supported(int k);
hipError_t launch_als_chol_wave(const AlsArgs& a, bool implicit, int grid, int loss_slot0, hipStream_t s, hipEvent_t* ev_slot);
// rank 65..128 (round 6, wrmf_chol_mf.hip): the rows of kCholLrMax + 1 .. kCholMfMax non-zeros as one wave per row -- assembly on
// the matrix cores into the accumulator registers, blocked Cholesky with the trailing updates on v_mfma_f32_32x32x2_f32.
// Needs a.wave_stats (operand scales).  Loss partials [loss_slot0, loss_slot0 + chol_mf_loss_slots(n_rows, implicit))
constexpr int kCholMfMax = 512;       // = kNeMinLen: beyond it the normal-equation launch (rows split across workgroups) keeps the row
constexpr int kCholMfGrid = 256 * 32; // workgroups of one wave, grid-stride over the rows (longest first)
bool chol_mf_supported(int k);
int chol_mf_grid(int n_rows);
int chol_mf_loss_slots(int n_rows, bool implicit);
hipError_t launch_als_chol_mf(const AlsArgs& a, bool implicit, const int32_t* rows, int n_rows, int loss_slot0, hipStream_t s,
                              hipEvent_t* ev_slot);
// rank 128, implicit feedback, conjugate gradient (round 6, wrmf_cg_mf.hip): the rows of kNeMinLen + 1 .. kCgMfMax non-zeros as one
// wave per row -- both normal-equation matrices in the accumulator registers, CG from the tiles.  The rows beyond kCgMfMax stay
// on wrmf_ne.hip (it splits them across workgroups).  Needs a.ne_stats.  Loss partials [loss_slot0, + cg_mf_loss_slots(n_rows))
constexpr int kCgMfGrid = 256 * 16;   // workgroups of four waves (a row each at a time), grid-stride over the rows (longest first)
bool cg_mf_supported(int k, bool implicit);
int cg_mf_grid(int n_rows);
int cg_mf_loss_slots(int n_rows);
hipError_t launch_als_cg_mf(const AlsArgs& a, const int32_t* rows, int n_rows, int loss_slot0, hipStream_t s, hipEvent_t* ev_slot);
hipError_t launch_als_nnls(const AlsArgs& a, bool implicit, hipStream_t s, hipEvent_t* ev = nullptr);
constexpr int kLuGrid = 64;          // workgroups (and loss slots) of the general-solver fallback
constexpr int kFailCap = 1 << 16;    // rows it can take per half-iteration call
hipError_t launch_als_lu_fallback(const AlsArgs& a, bool implicit, size_t loss_slot0, hipStream_t s);
// the failure block: [0] rows sent to the general solver by the current call, [1] of them unresolved, [2], [3] the same
// summed over the earlier calls since rsparse_hip_take_numeric_failures, [4 ..] the current call's row ids
hipError_t launch_fail_roll(int* fails, hipStream_t s);
constexpr int kSumStageBlocks = 256;
hipError_t launch_sum_partials(const double* partials, size_t n, double* out, hipStream_t s, double* tail = nullptr);
hipError_t launch_bias_shift_values(const float* vals, const int32_t* row_idx, const float* X, int k, int bias_row,
                                    int64_t nnz, float* out, hipStream_t s);
hipError_t launch_bias_sweep(const int32_t* p, const int32_t* i, const float* x, const float* other, int n_cols,
                             float lambda, int dynamic_lambda, int non_negative, float* out, hipStream_t s);
hipError_t launch_values_sum(const float* x, int64_t n, double* partials, double* out, hipStream_t s);
hipError_t launch_bias_implicit_terms(const float* vals, const int32_t* row_idx, const float* X, int k, int bias_row,
                                      int64_t nnz, float global_bias, float* rhs_vals, float* loss_tgt, hipStream_t s);
// out[t] = - sum_e X[off + t, e] * ((bias_row >= 0 ? X[bias_row, e] : 0) + global_bias),  t < k1
hipError_t launch_bias_rhs_init(const float* X, int k, int off, int k1, int bias_row, float global_bias, int n,
                                float* scratch, float* out, hipStream_t s);
size_t bias_rhs_init_scratch_floats();
// dst (n x k1p, k1p = k1 rounded up to a multiple of 4) = columns [src_off, src_off + k1) of src (n rows of src_stride floats),
// zeros beyond; Gp (k1p x k1p) = G (k1 x k1) with an identity on the padded diagonal (wrmf_bias.hip: why)
hipError_t launch_pad_rows(const float* src, int src_stride, int src_off, int k1, int k1p, int64_t n, float* dst, hipStream_t s);
hipError_t launch_pad_gramian(const float* G, int k1, int k1p, float* Gp, hipStream_t s);
hipError_t launch_bias_implicit_prep(const int32_t* p, const float* x, int n_cols, int n_other, double lambda,
                                     double* means, double* adj, hipStream_t s);
hipError_t launch_bias_implicit_sweep(const int32_t* p, const int32_t* i, const float* x, const float* other, int n_cols,
                                      int n_other, const double* other_sum, const double* means, const double* adj,
                                      int non_negative, double global_bias, float* out, hipStream_t s);
hipError_t launch_values_subtract_mean(float* x, int64_t n, const double* sum, double inv_count, hipStream_t s);

// Gramian: scratch must hold gramian_scratch_floats(k, n) floats.
size_t gramian_scratch_floats(int k, int64_t n);
hipError_t launch_gramian(const float* X, int k, int64_t n, float ridge, float* XtX, double* sumsq, float* scratch,
                          hipStream_t s, hipEvent_t* ev = nullptr, unsigned* absmax_bits = nullptr);
hipError_t launch_weighted_sumsq(const float* X, int k, int64_t n, const float* w, double* out,
                                 double* scratch /* >= 1024 doubles */, hipStream_t s);
hipError_t launch_f64_to_f32(const double* in, float* out, size_t n, hipStream_t s);
hipError_t check_row_indices_device(const int32_t* i, int64_t nnz, int n_rows, hipStream_t s, int* bad_index);
hipError_t transpose_csc_device(int n_rows, int n_cols, int64_t nnz, const int32_t* p, const int32_t* i, const float* x,
                                int32_t* pt, int32_t* it, float* xt, hipStream_t s, int* bad_index);
hipError_t launch_f32_to_f64(const float* in, double* out, size_t n, hipStream_t s);

// scores = U V^T per user fused with top-k and exclusions (wrmf_topk.hip); U: n_users x k, V: n_items x k,
// both row-major; res / scores: n_users x topk row-major, indices 1-based, INT32_MIN / NaN when fewer than topk
hipError_t launch_top_product(const float* U, const float* V, int n_users, int n_items, int k_rank, int topk,
                              const int32_t* nr_ptr, const int32_t* nr_idx, const int32_t* excl, int n_excl,
                              float glob_mean, int32_t* res, float* scores, hipStream_t s, float* scratch = nullptr);
// `$predict` ordered like the reference's double product (wrmf_topk.hip): kc >= topk candidates per user from the fp32 kernel,
// re-scored in double (U64 / V64, or the fp32 factors widened when they are null), the reference's heap replayed over them;
// scratch: top_product_f64_scratch_words(n_users, kc, topk) 4-byte words; split_scratch as launch_top_product's (for kc)
size_t top_product_f64_scratch_words(int n_users, int kc, int topk);
hipError_t launch_top_product_f64(const float* U32, const float* V32, const double* U64, const double* V64, int n_users,
                                  int n_items, int rank, int topk, int kc, const int32_t* nr_ptr, const int32_t* nr_idx,
                                  const int32_t* excl, int n_excl, double glob_mean, int32_t* res, double* scores, hipStream_t s,
                                  float* scratch, float* split_scratch);
// (the scratch both want -- the slices' lists of a call for few users over many items, or the global candidate buffers of a call
// for many users -- is top_product_plan(...).scratch_floats, wrmf_topk_plan.h)
// 256 < topk <= 8192 (wrmf_topk_large.hip): scores to a global key matrix per chunk of users, the kc-th key of every user by a radix
// select, the candidates at or above it ordered in LDS (fp32 scores, or re-scored in double), the reference heap's result in closed
// form; users whose candidate list overflows replay the heap.  ws: top_product_large_ws_floats(...) floats (chunk_users: users
// per chunk).  kc: top_product_large_kc (the fp32 form selects kc = topk).
constexpr int kTopLargeMin = 256;    // RSPARSE_HIP_MAX_TOPK: larger k only
constexpr int kTopLargeMax = 8192;   // RSPARSE_HIP_MAX_TOPK_LARGE
size_t top_product_large_ws_floats(int n_users, int n_items, int topk, int kc, int* chunk_users = nullptr);
int top_product_large_kc(int topk, int extra, int n_items);
hipError_t launch_top_product_large(const float* U, const float* V, int n_users, int n_items, int rank, int topk,
                                    const int32_t* nr_ptr, const int32_t* nr_idx, const int32_t* excl, int n_excl, float glob_mean,
                                    int32_t* res, float* scores, hipStream_t s, float* ws);
hipError_t launch_top_product_large_f64(const float* U32, const float* V32, const double* U64, const double* V64, int n_users,
                                        int n_items, int rank, int topk, int kc, const int32_t* nr_ptr, const int32_t* nr_idx,
                                        const int32_t* excl, int n_excl, double glob_mean, int32_t* res, double* scores,
                                        hipStream_t s, float* ws);
// its first two stages: the keys of U V^T for nu users (rows of `ld` words, ld % 4 == 0, rank <= 256 as above), and key 0 on every
// user's not_recommend row (nr_ptr: the nu + 1 slots of these users, absolute positions into nr_idx; nullable) and on `excl`
hipError_t launch_topl_score(const float* U, const float* V, int nu, int n_items, int rank, unsigned* keys, size_t ld, hipStream_t s);
hipError_t launch_topl_mask(unsigned* keys, size_t ld, int n_items, int nu, const int32_t* nr_ptr, const int32_t* nr_idx,
                            const int32_t* excl, int n_excl, hipStream_t s);

// full-ranking counts over that key matrix (wrmf_ranks.hip): per stored entry of `actual` (act_ptr / act_idx: CSR slots) the
// admissible items scored above it and tied with it (-1, -1 for an inadmissible entry), per user the admissible items.
// ws: held_out_ranks_ws_floats(...) floats (chunk_users: users per chunk; max_chunk_users > 0 caps it).  Then the per-user
// numbers from the counts: mpr, auc, mrr (n_users doubles) and sums (n_users x 3: sum w, sum w pct, P), each nullable; act_x is
// read for mpr and sums only.
size_t held_out_ranks_ws_floats(int n_users, int n_items, int max_chunk_users, int* chunk_users = nullptr);
hipError_t launch_held_out_ranks(const float* U, const float* V, int n_users, int n_items, int rank, const int32_t* nr_ptr,
                                 const int32_t* nr_idx, const int32_t* excl, int n_excl, const int32_t* act_ptr,
                                 const int32_t* act_idx, int max_chunk_users, int32_t* above, int32_t* tied, int32_t* n_adm,
                                 hipStream_t s, float* ws);
hipError_t launch_rank_summary(int n_users, const int32_t* act_ptr, const double* act_x, const int32_t* above, const int32_t* tied,
                               const int32_t* n_adm, double* mpr, double* auc, double* mrr, double* sums, hipStream_t s);

// ranking metrics ap@k / ndcg@k of row-major 1-based lists (wrmf_metrics.hip).  X may be null when ndcg_out is; either output may
// be null, not both.  long_buf: n_users + 1 ints of scratch (a count and the users whose idcg takes the long-row launch).
hipError_t launch_ranking_metrics(const int32_t* pred, int n_users, int k, const int32_t* P, const int32_t* J, const double* X,
                                  double* ap_out, double* ndcg_out, int* long_buf, hipStream_t s);

// hit-based metrics of the same lists at n_cutoffs <= kHitMaxCutoffs strictly ascending cutoffs in 1 .. k (wrmf_hits.hip), one
// launch and no scratch: hits / precision / recall / hit / mrr (n_users x n_cutoffs row-major), first (n_users), each nullable;
// first_seen (n_items, nullable) is min-updated with the first position at which any list names the item.  cutoffs: HOST (they
// travel as a kernel argument); k is the row stride of the lists.
constexpr int kHitMaxCutoffs = 16;   // RSPARSE_HIP_MAX_CUTOFFS
hipError_t launch_hit_metrics(const int32_t* pred, int n_users, int k, const int32_t* P, const int32_t* J, const int32_t* cutoffs,
                              int n_cutoffs, int32_t* hits, int32_t* first, double* precision, double* recall, double* hit,
                              double* mrr, int32_t* first_seen, int n_items, hipStream_t s);

// beyond-accuracy metrics of the same lists at the same cutoffs (wrmf_lists.hip), one launch and no scratch: valid (int32),
// count_sum / info_sum (int64), popularity / novelty (double), each n_users x n_cutoffs row-major and nullable.  item_count
// (int32 of n_items, >= 0) / item_info (int64 of n_items, 0 <= v < 2^40) are gathered only when not null.  exposure (n_cutoffs x
// n_items int32, nullable, caller-zeroed): += 1 at [b][item] for every valid position of the cutoff INTERVAL b -- the caller
// cumulates along b.  Items are 1 .. n_items; anything else (NA_integer_ too) is skipped.
hipError_t launch_list_metrics(const int32_t* pred, int n_users, int k, const int32_t* cutoffs, int n_cutoffs,
                               const int32_t* item_count, const int64_t* item_info, int n_items, int32_t* valid, int64_t* count_sum,
                               int64_t* info_sum, double* popularity, double* novelty, int32_t* exposure, hipStream_t s);

// intra-list cosine distance (wrmf_diversity.hip).  launch_item_inv_norms: inv[item] = 1 / |V[item, c0 : c0 + r)| in double, 0.0
// for a degenerate item (sum of squares zero or not finite); V fp32, or fp64 when f64, n_items x ld row-major, 1 <= r <= 256.
// launch_list_diversity: counted (int32) / diversity (double), n_users x n_cutoffs row-major, either nullable, from the
// factors as stored and that inv.
hipError_t launch_item_inv_norms(const void* V, bool f64, int n_items, int64_t ld, int c0, int r, double* inv, hipStream_t s);
hipError_t launch_list_diversity(const int32_t* pred, int n_users, int k, const int32_t* cutoffs, int n_cutoffs, const void* V,
                                 bool f64, int n_items, int64_t ld, int c0, int r, const double* inv, int32_t* counted,
                                 double* diversity, hipStream_t s);

// greedy MMR re-ranking of a pool of n_pool positions per user down to k (wrmf_mmr.hip; 1 <= k <= n_pool <= 8192, 1 <= r <= 256,
// 0 <= theta <= 1).  lists (1-based, INT32_MIN = NA) / scores: n_users x n_pool row-major; V and inv as for launch_list_diversity.
// items (1-based, NA-padded), picked (the picks' own scores), positions (1-based into the pool), objective: n_users x k
// row-major, NaN / NA where fewer than k positions are valid; each nullable except items.
hipError_t launch_mmr_rerank(const int32_t* lists, const double* scores, int n_users, int n_pool, int k, double theta, const void* V,
                             bool f64, int n_items, int64_t ld, int c0, int r, const double* inv, int32_t* items, double* picked,
                             int32_t* positions, double* objective, hipStream_t s);

// pointwise predictions at a CSR pattern (wrmf_score.hip), T = float or double, 1 <= r <= 256: scores[t] = add + U[row(t)] .
// V[J[t]] in double for every stored position t < P[n_rows] (the count stays on the device: a capped grid strides over it); then
// the squared / absolute error sums per row of given scores against `actual` (sse / sae: either may be null)
template <class T>
hipError_t launch_score_pairs(const T* U, const T* V, int n_rows, int n_cols, int r, const int32_t* P, const int32_t* J, double add,
                              double* scores, hipStream_t s);
hipError_t launch_score_error_sums(const double* scores, const double* actual, const int32_t* P, int n_rows, double* sse,
                                   double* sae, hipStream_t s);

// one soft-ALS half-iteration over a CSR matrix (wrmf_softals.hip), T = float or double, 1 <= r <= 256: out[row] = s o sum_t res_t
// M[J[t]] + t o W[row], res_t = X[t] - (w o W[row]) . M[J[t]], *sumsq = sum res^2 (nullable).  ws: softals_ws_doubles(r) doubles
// whose first 768 hold w, s, t at strides of 256 (zeros where absent and beyond r); res: W and w are used, has_t: W and t are.
size_t softals_ws_doubles(int r);
template <class T>
hipError_t launch_softals_half(const int32_t* P, const int32_t* J, const T* X, const T* M, const T* W, int n_rows, int n_cols, int r,
                               bool res, bool has_t, T* out, double* sumsq, double* ws, hipStream_t s);

// ItemKNN (wrmf_itemknn.hip; defined in rsparse_wrmf_hip.h).  `rows` dense rows of n_items cells per batch in ws (uint32 cells
// for the binary neighbours, uint64 for the weighted ones and for the lists), which is all zeros on entry and again when the
// enqueued work is done.  h_ip: the host copy of ip[item0 .. item1]; h_xp: of xp[0 .. n_rows].  1 <= K <= 256, 1 <= k <= 1024.
// il / ur: the weighted operands by stored position of either orientation; xv: the rows' weights, or null (all ones).
hipError_t launch_cooc_neighbors(const int32_t* ip, const int32_t* iu, const int32_t* up, const int32_t* uj, int n_users,
                                 int n_items, int item0, int item1, const int32_t* h_ip, int sim, int K, int64_t rows,
                                 unsigned* ws, int32_t* neighbors, int32_t* counts, hipStream_t s);
hipError_t launch_cooc_neighbors_weighted(const int32_t* ip, const int32_t* iu, const uint32_t* il, const int32_t* up, const int32_t* uj,
                                          const uint32_t* ur, int n_users, int n_items, int item0, int item1, const int32_t* h_ip,
                                          const double* a, const double* b, double h, int K, int64_t rows, unsigned long long* ws,
                                          int32_t* neighbors, unsigned long long* sums, hipStream_t s);
hipError_t launch_knn_recommend(const int32_t* xp, const int32_t* xj, const uint32_t* xv, int n_rows, int n_items, const int32_t* h_xp,
                                const int32_t* neighbors, const uint32_t* q, int K, const int32_t* nr_p, const int32_t* nr_j,
                                const int32_t* excl, int n_excl, int k, int64_t rows, unsigned long long* ws, int32_t* items,
                                long long* scores, hipStream_t s);
// Three more consumers of the same dense rows of scores (operands and workspace as launch_knn_recommend): the cells at the stored
// positions of a pattern (pp, pj) over the rows, unmasked; the lists within the rows' candidates (cp, cj); the counts above / tied
// with every entry of (ap, aj) among the row's admissible cells, and those cells' number.  pp / cp / ap: n_rows + 1 absolute
// slots; h_pp / h_cp: their host copies; scores / above / tied parallel pj / aj.
hipError_t launch_knn_score_pairs(const int32_t* xp, const int32_t* xj, const uint32_t* xv, int n_rows, int n_items, const int32_t* h_xp,
                                  const int32_t* neighbors, const uint32_t* q, int K, const int32_t* pp, const int32_t* pj,
                                  const int32_t* h_pp, int64_t rows, unsigned long long* ws, long long* scores, hipStream_t s);
hipError_t launch_knn_top_candidates(const int32_t* xp, const int32_t* xj, const uint32_t* xv, int n_rows, int n_items, const int32_t* h_xp,
                                     const int32_t* neighbors, const uint32_t* q, int K, const int32_t* cp, const int32_t* cj,
                                     const int32_t* h_cp, const int32_t* nr_p, const int32_t* nr_j, const int32_t* excl, int n_excl, int k,
                                     int64_t rows, unsigned long long* ws, int32_t* items, long long* scores, hipStream_t s);
hipError_t launch_knn_held_out_ranks(const int32_t* xp, const int32_t* xj, const uint32_t* xv, int n_rows, int n_items, const int32_t* h_xp,
                                     const int32_t* neighbors, const uint32_t* q, int K, const int32_t* ap, const int32_t* aj,
                                     const int32_t* nr_p, const int32_t* nr_j, const int32_t* excl, int n_excl, int64_t rows,
                                     unsigned long long* ws, int32_t* above, int32_t* tied, int32_t* n_adm, hipStream_t s);

// The steps of the above that another scorer of dense rows shares (wrmf_ease.hip); they enqueue the kernels of wrmf_itemknn.hip as
// they are.  fit_scatter: the co-occurrence counts of the items [r0, r1), whose stored entries are the slots [t0, t1) of iu, into
// r1 - r0 uint32 rows of n_items cells (the diagonal left out).  mask_rows: the all-ones sentinel into the not_recommend cells
// (nr_p: the slots of THESE rows, nullable) and the excl cells of n_batch uint64 rows.  select_lists: the k cells of largest
// value per row, ties to the smaller item, cells of 0 behind them in ascending order, all-ones cells never (items 1-based with
// INT32_MIN where a list ends, scores the cells' values).  zero_rows: the memset behind a batch.
void launch_knn_fit_scatter(const int32_t* ip, const int32_t* iu, const int32_t* up, const int32_t* uj, int n_users, int n_items, int r0,
                            int r1, unsigned t0, unsigned t1, unsigned* ws, hipStream_t s);
void launch_knn_mask_rows(unsigned long long* ws, size_t ld, int n_items, int n_batch, const int32_t* nr_p, const int32_t* nr_j,
                          const int32_t* excl, int n_excl, hipStream_t s);
void launch_knn_select_lists(const unsigned long long* ws, size_t ld, int n_items, int n_batch, int k, int32_t* items, long long* scores,
                             hipStream_t s);
hipError_t launch_knn_zero_rows(void* ws, size_t bytes, hipStream_t s);
// gather_rows: out[t] = the cell (row(t) - row0, pj[t]) of n_batch uint64 rows for the slots [t0, t1) of the pattern (pp: n_rows + 1
// absolute slots), 0 for a column outside the items.  ranks_rows: above / tied / n_adm of launch_knn_held_out_ranks for n_batch
// scored and masked rows (ap: the slots of THESE rows, absolute positions into aj / above / tied; n_adm: of these rows).
void launch_knn_gather_rows(const int32_t* pp, const int32_t* pj, int n_rows, int row0, int n_batch, unsigned t0, unsigned t1,
                            const unsigned long long* ws, size_t ld, int n_items, long long* out, hipStream_t s);
void launch_knn_ranks_rows(const unsigned long long* ws, size_t ld, int n_items, int n_batch, const int32_t* ap, const int32_t* aj,
                           int32_t* above, int32_t* tied, int32_t* n_adm, hipStream_t s);

// EASE (wrmf_ease.hip; defined in rsparse_wrmf_hip.h), on the ItemKNN workspace (all zeros on entry and again when the enqueued
// work is done).  item_gram: rows [item0, item1) of G + lambda I in double, `rows` uint32 rows per batch; h_ip: the host copy of
// ip[item0 .. item1].  recommend: T = float or double, B: n_items rows of ld_B elements, ld_B >= n_items and ld_B sizeof(T) a
// multiple of 16, B 16-byte aligned; `rows` uint64 rows per batch; scores: the order keys of the doubles.
hipError_t launch_ease_item_gram(const int32_t* ip, const int32_t* iu, const int32_t* up, const int32_t* uj, int n_users, int n_items,
                                 int item0, int item1, const int32_t* h_ip, double lambda, int64_t rows, unsigned* ws, double* out,
                                 size_t ld_out, hipStream_t s);
template <class T>
hipError_t launch_ease_recommend(const int32_t* xp, const int32_t* xj, int n_rows, int n_items, const T* B, size_t ld_B,
                                 const int32_t* nr_p, const int32_t* nr_j, const int32_t* excl, int n_excl, int k, int64_t rows,
                                 unsigned long long* ws, int32_t* items, long long* scores, hipStream_t s);
// EASE under the evaluation protocols (operands as launch_ease_recommend; pp / cp / ap: n_rows + 1 absolute slots, h_pp / h_cp their
// host copies).  A row of m pairs / candidates with m <= RSPARSE_HIP_KNN_LDS_CAND and m RSPARSE_HIP_EASE_CELLS_RATIO <= n_items is
// scored at its cells (no workspace); the others, in runs of at most `rows` consecutive ones, through the dense rows of ws.
// scores (score_pairs): one key per slot of pj, the key of +0.0 for a column outside the items.  keys (top_candidates): scratch,
// one per slot of cj; the candidate columns of a row strictly ascending.  held_out_ranks: every row through ws.
template <class T>
hipError_t launch_ease_score_pairs(const int32_t* xp, const int32_t* xj, int n_rows, int n_items, const T* B, size_t ld_B,
                                   const int32_t* pp, const int32_t* pj, const int32_t* h_pp, int64_t rows, unsigned long long* ws,
                                   unsigned long long* scores, hipStream_t s);
template <class T>
hipError_t launch_ease_top_candidates(const int32_t* xp, const int32_t* xj, int n_rows, int n_items, const T* B, size_t ld_B,
                                      const int32_t* cp, const int32_t* cj, const int32_t* h_cp, const int32_t* nr_p, const int32_t* nr_j,
                                      const int32_t* excl, int n_excl, int k, int64_t rows, unsigned long long* ws,
                                      unsigned long long* keys, int32_t* items, long long* scores, hipStream_t s);
template <class T>
hipError_t launch_ease_held_out_ranks(const int32_t* xp, const int32_t* xj, int n_rows, int n_items, const T* B, size_t ld_B,
                                      const int32_t* ap, const int32_t* aj, const int32_t* nr_p, const int32_t* nr_j, const int32_t* excl,
                                      int n_excl, int64_t rows, unsigned long long* ws, int32_t* above, int32_t* tied, int32_t* n_adm,
                                      hipStream_t s);

// SLIM (wrmf_slim.hip; defined in rsparse_wrmf_hip.h).  support: msize[c] = the support size of column cols[c] of G, -1 for a
// column outside the items.  state_bytes: the workspace of n_global columns beyond RSPARSE_HIP_SLIM_LDS_SUPPORT whose largest
// support is max_support -> bytes, with the slices (at most kSlimSlices workgroups, each striding over the columns) and the
// entries of one.  columns: the fits; n_lds: how many columns are within the LDS bound (0 = that launch is left out), slices = 0
// leaves the other out; ws: state_bytes bytes, 8-byte aligned.
constexpr int kSlimSlices = 512;
void launch_slim_support(const double* G, size_t ld_G, int n_items, const int32_t* cols, int n_cols, int32_t* msize, hipStream_t s);
size_t slim_state_bytes(int n_global, int max_support, int& slices, int& stride);
hipError_t launch_slim_columns(const double* G, size_t ld_G, int n_items, const int32_t* cols, const int32_t* msize, int n_cols,
                               int n_lds, int slices, int stride, double l1, double l2, int max_iter, double tol, void* W,
                               size_t ld_W, bool w_is_double, int32_t* sweeps, char* ws, hipStream_t s);

// BPR (wrmf_bpr.hip; defined in rsparse_wrmf_hip.h).  A run: the canonical CSR rows (p from 0, nnz = p[n_rows] handed in, so that
// nothing is read back), the stream's parameters and the step size; n_steps: the steps of an epoch.  triples: (u, i, j) of one
// step, cnt = ceil((nnz - step) / n_steps) each.  run: the steps [0, n_steps) (only_step < 0) or the one step only_step of the
// epochs [epoch0, epoch0 + n_epochs), in place on U, V (ld = rank), aU, aV; counts[2 e], counts[2 e + 1]: n_valid and n_correct of
// epoch epoch0 + e, ADDED to.  !update_items: V and aV are read only.  Allocates its scratch and waits for `s` before it returns.
struct BprRun {
  const int32_t* p;
  const int32_t* j;
  int n_rows, n_items;
  int64_t nnz, row0;
  uint64_t seed;
  int mode, n_steps, rank;
  double lr, lambda;
  bool update_items;
};
hipError_t launch_bpr_triples(const BprRun& r, int epoch, int step, int32_t* tu, int32_t* ti, int32_t* tj, hipStream_t s);
template <class T>
hipError_t launch_bpr_run(const BprRun& r, int epoch0, int n_epochs, int only_step, T* U, T* V, double* aU, double* aV,
                          unsigned long long* counts, hipStream_t s);

// top-k within per-user candidate lists (wrmf_candidates.hip), T = float or double, 1 <= topk <= kTopLargeMax: for every row of
// the CSR pattern (cand_p: n_users + 1 slots, absolute positions into cand_j; p0 = cand_p[0], nnz = cand_p[n_users] - p0, read by
// the caller; columns ascending and unique within a row) the topk best admissible candidates by launch_score_pairs' scores
// (glob_mean included), with the reference heap's tie rule; not_recommend (nr_ptr: the slots of these users, absolute positions
// into nr_idx, columns ascending; nullable) and excl (ascending; nullable) make a candidate inadmissible.  res: 1-based items,
// INT32_MIN where fewer than topk are admissible (scores NaN there).  ws: top_candidates_ws_bytes(n_users, nnz) bytes.
size_t top_candidates_ws_bytes(int n_users, int64_t nnz);
template <class T>
hipError_t launch_top_candidates(const T* U, const T* V, int n_users, int n_items, int rank, int topk, const int32_t* cand_p,
                                 const int32_t* cand_j, int32_t p0, int64_t nnz, const int32_t* nr_ptr, const int32_t* nr_idx,
                                 const int32_t* excl, int n_excl, double glob_mean, int32_t* res, double* scores, hipStream_t s,
                                 void* ws);

// per-item contributions to a score (wrmf_explain.hip), T = float or double, 1 <= r <= 128: for every target q (t_p / t_j: CSR
// over the users) of a user with the row (x_p / x_j) and the per-non-zero weights wa (assembly) and wb (contribution),
// contrib[out_p[q] + t] = wb_t (z . V[x_j[t]]) with (base + (diag + diag_per_nnz len) I + sum_t wa_t V[x_j[t]] V[x_j[t]]^T) z =
// V[t_j[q]], and total[q] their sum; flags[u] = 1 (outputs NaN) where the system is not positive definite, 0 for every other
// user that has a target.  One workgroup per user.
template <class T>
hipError_t launch_explain(const T* V, int n_items, int r, const T* base, double diag, double diag_per_nnz, int n_users,
                          const int32_t* x_p, const int32_t* x_j, const T* wa, const T* wb, const int32_t* t_p, const int32_t* t_j,
                          const int64_t* out_p, T* contrib, double* total, int32_t* flags, hipStream_t s);

// initial factors drawn on the device (wrmf_init.hip), T = float or double: the rows [row0, row0 + n_rows) of the (., rank) matrix
// of `stream` (0 users, 1 items) under `seed`, written to `out` (row row0's first element, leading dimension ld >= rank) as
// scale * N(0, 1), |.| with abs_values, the column ones_col (-1: none) exactly 1.  The generator: rsparse_wrmf_hip.h.
template <class T>
hipError_t launch_init_factors(uint64_t seed, int stream, int64_t row0, int n_rows, int rank, int64_t ld, double scale,
                               int abs_values, int ones_col, T* out, hipStream_t s);

// negative sampling (wrmf_sample.hip): the stream is defined in rsparse_wrmf_hip.h.  launch_sample_row_pointers writes out_p
// (n_rows + 1) from the lengths of the seen / keep rows on the device; ws: sample_negatives_ws_bytes(n_rows) bytes, *d_status
// points into it, for the caller to read back before it samples: total = the 64-bit out_p[n_rows], flag non-zero = row pointers
// that are negative or decrease, a seen row longer than n_item, a keep row longer than its seen row.  launch_sample_negatives
// writes the rows: 1 <= n <= kSampleMaxNegatives, row0 + n_rows <= 2^32, keep_p / keep_j both null or both set.
constexpr int kSampleMaxNegatives = 8192;
struct SampleStatus {
  long long total;
  int flag, pad;
};
size_t sample_negatives_ws_bytes(int n_rows);
hipError_t launch_sample_row_pointers(int n_rows, int n_item, int n, const int32_t* seen_p, const int32_t* keep_p, int32_t* out_p,
                                      void* ws, SampleStatus** d_status, hipStream_t s);
hipError_t launch_sample_negatives(uint64_t seed, int64_t row0, int n_rows, int n_item, int n, const int32_t* seen_p,
                                   const int32_t* seen_j, const int32_t* keep_p, const int32_t* keep_j, const int32_t* out_p,
                                   int32_t* out_j, hipStream_t s);
// the scan behind out_p, for other row-pointer arrays too (wrmf_split.hip): out_p[row + 1] holds the row's length and bsum[b] the
// sum of the lengths of rows [256 b, 256 b + 256); boff: (n_rows + 255) / 256 words of scratch; *total = the 64-bit out_p[n_rows]
hipError_t launch_row_pointer_scan(int n_rows, const long long* bsum, long long* boff, long long* total, int32_t* out_p, hipStream_t s);

// popularity-weighted negative sampling (wrmf_sample_weighted.hip): the stream is defined in rsparse_wrmf_hip.h.
// launch_weights_prefix writes cum[i] = w[0] + ... + w[i] (n_item >= 1 of them); ws: weights_prefix_ws_bytes(n_item) bytes, *d_flag
// points into it, for the caller to read back: non-zero = a zero weight.  launch_sample_negatives_weighted writes the rows at the
// out_p of launch_sample_row_pointers (the lengths are the uniform sampler's) and adds the rows it had to fill to *filled_rows
// (null: not counted); the limits are launch_sample_negatives'.
size_t weights_prefix_ws_bytes(int n_item);
hipError_t launch_weights_prefix(const uint32_t* w, int n_item, uint64_t* cum, void* ws, int** d_flag, hipStream_t s);
hipError_t launch_sample_negatives_weighted(uint64_t seed, int64_t row0, int n_rows, int n_item, int n, const int32_t* seen_p,
                                            const int32_t* seen_j, const int32_t* keep_p, const int32_t* keep_j, const uint64_t* cum,
                                            const int32_t* out_p, int32_t* out_j, int* filled_rows, hipStream_t s);

// train / test split (wrmf_split.hip): the stream is defined in rsparse_wrmf_hip.h.  mode 0 = proportion (threshold <= 2^32, no
// `by`), 1 = leave-out (leave_out >= 1, min_train >= 0; by: one double per stored entry, or null = random keys).
// launch_split_count writes both row-pointer arrays (n_rows + 1 each) and keeps the rows' thresholds in ws (split_ws_bytes(n_rows)
// bytes, which launch_split_write must be given unchanged); *d_status points into it, for the caller to read back before it
// writes: the two 64-bit totals, flag non-zero = row pointers that are negative or decrease.  launch_split_write copies every
// entry's index and value (value_bytes 0, 4 or 8: opaque words) to its place.  n_rows >= 1, row0 + n_rows <= 2^32.
struct SplitStatus {
  long long total_train, total_test;
  int flag, pad;
};
size_t split_ws_bytes(int n_rows);
hipError_t launch_split_count(uint64_t seed, int64_t row0, int n_rows, int mode, uint64_t threshold, int leave_out, int min_train,
                              const int32_t* p, const double* by, int32_t* train_p, int32_t* test_p, void* ws, SplitStatus** d_status,
                              hipStream_t s);
hipError_t launch_split_write(uint64_t seed, int64_t row0, int n_rows, int mode, uint64_t threshold, int leave_out, int min_train,
                              const int32_t* p, const int32_t* j, const void* v, int value_bytes, const double* by,
                              const int32_t* train_p, int32_t* train_j, void* train_v, const int32_t* test_p, int32_t* test_j,
                              void* test_v, void* ws, hipStream_t s);

// confidence weighting (wrmf_confidence.hip; the kinds and tables are defined in rsparse_wrmf_hip.h).  A matrix is (p, i, x) with
// n_seg segments, p[0] = 0, p[n_seg] = nnz.  launch_confidence_moments needs confidence_ws_doubles(nnz) doubles of scratch.
size_t confidence_ws_doubles(int64_t nnz);
hipError_t launch_confidence_moments(const int32_t* p, const double* x, int n_seg, int64_t nnz, int power, double* out, double* total,
                                     double* ws, hipStream_t s);
hipError_t launch_confidence_table(int table, int n, const int32_t* p, const double* moment, const double* total, double a, double b,
                                   double c, double* out, hipStream_t s);
hipError_t launch_confidence_apply(int kind, const int32_t* p, const int32_t* i, const double* x, int n_seg, int64_t nnz,
                                   const double* seg_table, const double* idx_table, int n_idx, int seg_is_item, double a, double b,
                                   void* out, int out_float, hipStream_t s);

// the interaction matrix from an event log (wrmf_events.hip; the aggregates and their summation order are defined in
// rsparse_wrmf_hip.h).  n >= 1 events, n_users, n_items >= 1; every pointer is device memory, values / ts / count / latest may be
// null.  Allocates its scratch (16 or 24 bytes per event, plus about one byte per event for the long cells) and
// waits for the stream: after the pack launch to read the id flag, after the scan to read the number of cells, and at the end.
// *status: 0 = done; 1 = an id outside the shape (nothing was written); 2 = *n_cells > capacity (nothing was written).
hipError_t events_to_csr_device(int64_t n, int n_users, int n_items, const int32_t* users, const int32_t* items, const double* values,
                                const double* ts, int aggregate, double half_life, int has_now, double now, int32_t* p, int32_t* j,
                                double* x, int32_t* count, double* latest, int64_t capacity, int64_t* n_cells, hipStream_t s,
                                int* status);

// item-to-item cosine similarity (wrmf_similar.hip): the operands of the top-k path above.
// launch_normalize_items: V (fp32, or fp64 when f64) n_items x ld row-major, columns [c0, c0 + r), 1 <= r <= 256 ->
// Vn64 / Vn32 (n_items x r, compact) with unit rows, flags[item] = 1 and a row of zeros where the sum of squares is zero or
// not finite.
hipError_t launch_normalize_items(const void* V, bool f64, int n_items, int64_t ld, int c0, int r, float* Vn32, double* Vn64,
                                  int32_t* flags, hipStream_t s);
// what a batch of n_q queries needs next to the top-k call, carved from one allocation of similar_query_ws_bytes(n_q, r):
// the gathered operands, the self-exclusion slots (nr_p = 0..n_q, nr_j = the query's id) and bad[q] = 1 for a query that is
// degenerate or out of range (launch_mask_queries then overwrites its row with NA_integer_ / NaN)
struct SimilarQueryWs {
  double* Q64;
  float* Q32;
  int32_t* nr_p;
  int32_t* nr_j;
  int32_t* bad;
};
size_t similar_query_ws_bytes(int n_q, int r);
SimilarQueryWs similar_query_ws(void* ws, int n_q, int r);
hipError_t launch_gather_queries(const float* Vn32, const double* Vn64, int n_items, int r, const int32_t* query, int n_q,
                                 const SimilarQueryWs& w, hipStream_t s);
hipError_t launch_mask_queries(const int32_t* bad, int n_q, int k, int32_t* res, double* scores, hipStream_t s);

// device helpers of the multi-GPU context (wrmf_ctx_kernels.hip / wrmf_ctx.cpp)
hipError_t launch_ctx_accumulate(const float* Gpart, const double* sumsq, double* red, int k, hipStream_t s);
hipError_t launch_ctx_put_absmax(const float* absmax, double* red, int k, hipStream_t s);
hipError_t launch_ctx_reduce(const double* all, int ws, int k, float ridge, float* G, double* scal0, float* absmax, hipStream_t s);
hipError_t launch_ctx_sum(const double* v, int n, double* out, hipStream_t s);
hipError_t launch_ctx_add(const double* src, double* dst, hipStream_t s);   // *dst += *src

int padded_rank(int k);  // 32 / 64 / 128, or 0 if unsupported

// ranks 129..256 (wrmf_wide.hip): every variant of the half-iteration on one kernel family, the row's system a packed lower
// triangle in LDS; the Gramian likewise.  launch_als_wide reads the operands of `a` that the rank <= 128 kernels read
// (col_ptrs, row_idx, vals, X, Y, XtX, k, cg_steps, lambda_loss, dynamic_lambda, rhs_vals, loss_tgt, loss_tgt_const, rhs_init,
// gbias, loss_partials [wide_als_grid(n_cols) slots], fail_counter).
bool wide_supported(int k);
int wide_als_grid(int n_cols);
size_t wide_m2_floats_per_wg(int k);            // NNLS scratch per workgroup
size_t wide_gramian_scratch_floats(int k);
hipError_t launch_als_wide(const AlsArgs& a, bool implicit, unsigned solver, float* m2_scratch, float* lu_scratch, hipStream_t s,
                           int n_lo = -1);   // n_lo: rows of at most that many non-zeros belong to another launch
// plain conjugate gradient at these ranks, rows of at most kWideCgMaxLen non-zeros: one wave per row, no k x k system (wrmf_wide_cg.hip)
constexpr int kWideCgMaxLen = 2048;
bool wide_cg_wave_supported(const AlsArgs& a, unsigned solver);
int wide_cg_wave_grid(int n_cols);
int wide_cg_team_grid(int n_cols);
hipError_t launch_wide_cg_wave(const AlsArgs& a, bool implicit, int n_hi, const int32_t* order, int slot0, hipStream_t s);
hipError_t launch_gramian_wide(const float* X, int k, int64_t n, float ridge, float* XtX, double* sumsq, float* scratch,
                               hipStream_t s);

// Measurement harness (rsparse_hip_profile_*): the launcher that records the event `ev_slot` in front of a kernel also
// says which kernel it is about to launch (host function pointer); rsparse_hip_profile_last_names resolves the pointers
// to the names a profiler prints.  No-op when ev_slot is null.
void prof_note(hipEvent_t* ev_slot, const void* kernel_fn);

// Shared by the translation units of the C ABI (wrmf_capi.cpp, wrmf_f64_capi.cpp, wrmf_capi_host.cpp): the thread-local error text behind
// rsparse_hip_last_error(), and the device block of the exact solvers' failure counters (see launch_fail_roll; nullptr if
// the workspace could not be set up -- the error text then says why).
int capi_fail(int code, const std::string& msg);
int capi_hip_fail(hipError_t e, const char* what);
int* capi_fail_counters();
// RAII for the stateless entry points: takes the failure counts an earlier device-resident call left on the device when the
// stateless call starts (they are not its own) and hands them back to the next reader when it ends
void capi_fail_carry_add(int64_t unresolved, int64_t fallback);
// Grow-only device scratch of the two workspaces.  Every buffer is a member constructed on its workspace's chain, so that
// the workspace's release (a device change) reaches each of them without naming it.
struct GrowBufBase {
  void* p = nullptr;
  size_t cap = 0;   // elements
  GrowBufBase* const next;
  explicit GrowBufBase(GrowBufBase*& chain) : next(chain) { chain = this; }
  GrowBufBase(const GrowBufBase&) = delete;
  GrowBufBase& operator=(const GrowBufBase&) = delete;
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  static void release_all(GrowBufBase* chain) {
    for (; chain; chain = chain->next) chain->release();
  }
};
template <class T>
struct GrowBuf : GrowBufBase {
  using GrowBufBase::GrowBufBase;
  // at least n elements; growing frees first, with plain hipFree: it waits for work still using the old buffer
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    hipError_t e = hipMalloc(&p, n * sizeof(T));
    if (e == hipSuccess) cap = n;
    return e;
  }
  operator T*() const { return static_cast<T*>(p); }
};
struct DevBuf {  // RAII for the stateless entry points
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
  template <class T> T* as() { return static_cast<T*>(p); }
};

struct StaleFailures {
  int64_t unresolved = 0, fallback = 0;
  StaleFailures();
  ~StaleFailures() { capi_fail_carry_add(unresolved, fallback); }
  StaleFailures(const StaleFailures&) = delete;
  StaleFailures& operator=(const StaleFailures&) = delete;
};

}  // namespace rsparse_hip
