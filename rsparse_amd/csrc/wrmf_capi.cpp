// C ABI of librsparse_wrmf_hip.so (declared in include/rsparse_wrmf_hip.h).
//
// Host-side responsibilities only: argument validation with the reference's error behaviour turned
// into status codes (the reference raises R errors through END_RCPP, src/RcppExports.cpp:374,392),
// device buffers, the row-length schedule, and the bookkeeping around the kernels in
// wrmf_kernels.hip.  No torch, no R, no Armadillo types anywhere.
#include "../../include/rsparse_wrmf_hip.h"

#include <cxxabi.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "wrmf_capi_common.h"
#include "wrmf_topk_plan.h"

using namespace rsparse_hip;

struct rsparse_hip_csc {
  DevCSC d;
  int device = 0;
  std::vector<void*> owned;   // every device array the handle allocated: rsparse_hip_csc_destroy frees each, once
};

namespace {
thread_local std::string g_err;   // behind rsparse_hip_last_error()
}

int rsparse_hip::capi_fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int rsparse_hip::capi_hip_fail(hipError_t e, const char* what) {
  return fail(RSPARSE_HIP_ERR_RUNTIME, std::string(what) + ": " + hipGetErrorString(e));
}

namespace {

using CscGuard = HandleGuard<rsparse_hip_csc, rsparse_hip_csc_destroy>;

// Grow-only per-process scratch (single host thread drives the library, like the reference's
// single R thread; not re-entrant across streams).
struct Workspace {
  GrowBufBase* all = nullptr;
  GrowBuf<float> gram{all};
  GrowBuf<double> partials{all};   // partial_slots() slots + the tail of the two-stage sum
  GrowBuf<double> scalars{all};    // [0] loss rows, [1] sumsq, [2..] spare
  GrowBuf<int> fails{all};         // see launch_fail_roll
  GrowBuf<unsigned> ne_stats{all};   // normal-equation kernel: max |x|, max c, any c < 1 (launch_ne_stats)
  GrowBuf<float> lr_M{all};          // M = L^-T and its transpose of the low-rank Cholesky path
  GrowBuf<float> ne_seg_scratch{all};   // split rows of the normal-equation kernel: partial accumulators + ready flags
  GrowBuf<int> ne_seg_flags{all};
  GrowBuf<float> zero_row{all};   // 256 zero floats (padding slots of the CG gathers)
  GrowBuf<float> tscr{all};       // streamed CG rows: per-non-zero dot products of every sweep
  GrowBuf<float> bias_buf{all};   // explicit + biases: X', Y', shifted ratings
  GrowBuf<float> gb_r0{all};      // global bias + CG: per long row, base - g X_nnz (c - 1)  (launch_gb_row_terms)
  GrowBuf<int32_t> gb_slot{all};  // ... and the slot of every row in it
  GrowBuf<float> wide_m2{all};    // ranks 129..256 (wrmf_wide.hip): NNLS squared systems / the general solver's matrices
  GrowBuf<float> wide_lu{all};
  GrowBuf<int> met_buf{all};      // ranking metrics (wrmf_metrics.hip): count + list of the users whose idcg takes the long-row launch
  GrowBuf<char> sim_buf{all};     // item-to-item similarity (wrmf_similar.hip): a batch's gathered queries and self-exclusion slots
  GrowBuf<double> score_buf{all};   // pointwise predictions (wrmf_score.hip): the scores of a call that asks for the error sums only;
                                    // top-k within candidate lists (wrmf_candidates.hip): its scores / keys, bits and row lists
  GrowBuf<double> softals_buf{all};   // soft-ALS half-iteration (wrmf_softals.hip): w, s, t and the partial sums of split rows
  GrowBuf<char> knn_buf{all};     // ItemKNN (wrmf_itemknn.hip): a batch of dense rows, all zeros between calls
  bool knn_dirty = false;         // ... unless a call failed between its scatter and its zeroing
  GrowBuf<float> mf_G{all};       // wrmf_chol_mf.hip at rank 65..127: XtX padded to 128 x 128
  GrowBuf<float> pad_buf{all};    // ranks that are not a multiple of 4: the padded copies of X, Y, XtX, rhs_init (run_half_iteration)
  int device = -1;

  int ensure_device() {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != device) {  // buffers belong to the device they were allocated on
      GrowBufBase::release_all(all);
      device = dev;
    }
    // The fixed blocks that start zeroed.  hipMemset of device memory may return before it has run, and it runs on the null
    // stream, which does not order the work of a caller's hipStreamNonBlocking stream (the rank threads of wrmf_ctx.cpp): the
    // zeroing of ne_stats then landed between a first call's scan and the kernels that read max |X| from it, and their fp16
    // operand scale became that of 1e-30 -- NaN rows (tests/test_ctx_rows.py).  So the thread waits for it.
    bool zeroed = false;
    if (!scalars) {
      HIP_TRY(scalars.ensure(16));
      HIP_TRY(hipMemset(scalars, 0, 16 * sizeof(double)));
      zeroed = true;
    }
    if (!fails) {
      HIP_TRY(fails.ensure((size_t)(4 + kFailCap)));
      HIP_TRY(hipMemset(fails, 0, 4 * sizeof(int)));
      zeroed = true;
    }
    if (!ne_stats) {
      HIP_TRY(ne_stats.ensure(4));
      HIP_TRY(hipMemset(ne_stats, 0, 4 * sizeof(unsigned)));
      zeroed = true;
    }
    if (!zero_row) {
      HIP_TRY(zero_row.ensure(256));
      HIP_TRY(hipMemset(zero_row, 0, 256 * sizeof(float)));
      zeroed = true;
    }
    if (zeroed) HIP_TRY(hipStreamSynchronize(nullptr));
    return RSPARSE_HIP_OK;
  }
  int ensure_partials(size_t slots) {
    HIP_TRY(partials.ensure(std::max<size_t>(slots, 1024) + kSumStageBlocks));   // + the tail of the two-stage sum
    return RSPARSE_HIP_OK;
  }
  size_t partial_slots() const { return partials.cap - kSumStageBlocks; }
};
thread_local Workspace g_ws;   // per host thread: the multi-GPU context (wrmf_ctx.cpp) drives one device from one thread each

// the sum scratch of this thread's workspace for the bodies of wrmf_capi_common.h
int sum_scratch(SumScratch& w) {
  int rc = g_ws.ensure_device();
  if (rc) return rc;
  if ((rc = g_ws.ensure_partials(1024))) return rc;
  w = {g_ws.partials, g_ws.scalars};
  return RSPARSE_HIP_OK;
}

struct Profiler {
  bool on = false;
  bool have = false;
  int nseg = 0;
  hipEvent_t ev[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const void* kern[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipEvent_t* begin() {
    have = false;
    if (!on) return nullptr;
    for (auto& e : ev)
      if (!e && hipEventCreate(&e) != hipSuccess) return nullptr;
    for (auto& k : kern) k = nullptr;
    return ev;
  }
};
thread_local Profiler g_prof;

// a planned vector as a device array of handle m (nullptr for an empty one)
template <class T>
int upload(rsparse_hip_csc& m, const std::vector<T>& v, const T** out) {
  *out = nullptr;
  if (v.empty()) return RSPARSE_HIP_OK;
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, v.size() * sizeof(T)));
  m.owned.push_back(p);
  HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *out = static_cast<const T*>(p);
  return RSPARSE_HIP_OK;
}

int upload_cut(rsparse_hip_csc& m, const NeCut& cut, NeListSet& L) {
  L = NeListSet();
  L.entries = (int)cut.items.size();
  L.nseg = cut.nseg();
  L.nsplit = (int)cut.split_rows.size();
  if (int rc = upload(m, cut.segs, &L.segs)) return rc;
  if (int rc = upload(m, cut.split_rows, &L.split_rows)) return rc;
  return upload(m, cut.split_ptr, &L.split_ptr);
}
int upload_deal(rsparse_hip_csc& m, const NeDeal& deal, NeListSet& L) {
  L.wg = deal.wg();
  if (int rc = upload(m, deal.rows, &L.rows)) return rc;
  return upload(m, deal.ptr, &L.ptr);
}

// The launch schedule of handle m (one-off per matrix): planned on the host from the column pointers (wrmf_schedule.cpp),
// published here
int build_schedule(rsparse_hip_csc& m, const int32_t* host_col_ptrs) {
  DevCSC& d = m.d;
  int cus = 256;
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, m.device));
  d.q_cfg = cgq_default_cfg();
  SchedulePlan plan;
  if (!plan_schedule(host_col_ptrs, d.n_cols, cus, [](int len) { return cgq_bucket_of(len, cgq_default_cfg()); }, plan))
    return fail(RSPARSE_HIP_ERR_INVALID, "col_ptrs is not non-decreasing");
  d.max_len = plan.max_len; d.nnz_long = plan.nnz_long; d.n_empty = plan.n_empty;
  d.short_max = kTileNnz; d.n_long = plan.n_long;
  for (int b = 0; b < 7; b++) d.q_off[b] = plan.off[b];
  for (int b = 0; b < 6; b++) d.q_nnz[b] = plan.nnz[b];
  d.q_pair_first = plan.pair_first; d.q_team4_first = plan.team4_first;
  d.q_team4_wide_first = plan.team4_wide_first;
  d.q_gt32 = plan.gt32; d.q_gt48 = plan.gt48; d.q_lr_first = plan.lr_first; d.q_n_lr = plan.n_lr;
  d.q_n_chol_long = plan.n_chol_long; d.q_n_nec = plan.n_nec;
  int rc;
  if ((rc = upload(m, plan.order, &d.q_order))) return rc;
  if ((rc = upload(m, plan.stream_off, &d.q_stream_off))) return rc;
  if ((rc = upload_cut(m, plan.cut, d.q_ne))) return rc;
  d.q_ne1 = d.q_ne;   // (the same segment table and split rows: the deal does not change the cut)
  if ((rc = upload_deal(m, plan.fine, d.q_ne))) return rc;
  if ((rc = upload_deal(m, plan.coarse, d.q_ne1))) return rc;
  if (plan.nec_is_ne) {
    d.q_nec = d.q_ne;
  } else {
    if ((rc = upload_cut(m, plan.cut_nec, d.q_nec))) return rc;
    if ((rc = upload_deal(m, plan.nec, d.q_nec))) return rc;
  }
  return RSPARSE_HIP_OK;
}

// the register-resident quad-layout CG kernels need rank % 4 == 0 and 16-byte aligned factor matrices; other ranks take
// the LDS-tile kernels of wrmf_kernels.hip
bool use_cgq(int rank, const void* X, const void* Y) {
  return rank % 4 == 0 && ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y)) & 15) == 0;
}

int check_common(int n_rows, int n_cols, const void* col_ptrs, const void* X, const void* Y, int rank) {
  if (n_rows < 0 || n_cols < 0) return fail(RSPARSE_HIP_ERR_INVALID, "negative matrix dimension");
  if (!col_ptrs) return fail(RSPARSE_HIP_ERR_INVALID, "col_ptrs is NULL");
  if (!X || !Y) return fail(RSPARSE_HIP_ERR_INVALID, "X or Y is NULL");
  if (rank <= 0) return fail(RSPARSE_HIP_ERR_INVALID, "rank must be positive");
  if (rank > RSPARSE_HIP_MAX_RANK)
    return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "rank > 256 is not on the device path");
  return RSPARSE_HIP_OK;
}

// rows whose failure counts were taken off the device on behalf of a LATER reader (rsparse_hip_take_numeric_failures adds them)
thread_local int64_t g_fail_carry[2] = {0, 0};   // unresolved, re-solved by the general solver

// wrmf_implicit.hpp:108-109: a global bias below sqrt(eps) of the element type T is treated as zero (float: 3.45e-4,
// double: 1.49e-8; the device layer holds floats, the stateless *_double entry point passes dbl = true)
bool has_global_bias(double global_bias, bool dbl = false) {
  return global_bias >= std::sqrt(dbl ? DBL_EPSILON : (double)FLT_EPSILON);
}

// Ranks that are not a multiple of 4 run on zero-padded copies: a padded coordinate sees a right-hand side of 0
// against lambda_use on the diagonal (implicit: the ridge of the padded Gramian, written as 1) and stays 0.  With explicit
// feedback, lambda = 0 (the reference's default) and the exact solver that diagonal is 0: every padded system would be
// singular where the true one is not.  Those fits keep the true rank on the LDS-tile kernels.
bool zero_padding_is_neutral(bool implicit, unsigned solver, double lambda) {
  return implicit || solver != RSPARSE_SOLVER_CHOLESKY || lambda != 0.0;
}

int check_variant(unsigned solver, int with_biases, double global_bias, bool implicit = true) {
  if (solver > RSPARSE_SOLVER_NNLS) return fail(RSPARSE_HIP_ERR_INVALID, "unknown solver code");
  if (with_biases && implicit && solver == RSPARSE_SOLVER_CONJUGATE_GRADIENT)
    // the reference drops a row of the warm start twice on this path (wrmf_implicit.hpp:189,197) and cannot run it
    return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "with_user_item_bias + conjugate_gradient with implicit feedback is not on the device path");
  // (a global bias goes with every solver: Cholesky / NNLS wrmf_implicit.hpp:228-229,262-270, conjugate gradient
  // cg_solver_implicit_global_bias :35-57; with explicit feedback it is removed from the data by the R driver)
  (void)global_bias;
  return RSPARSE_HIP_OK;
}

struct BiasTerms {   // implicit feedback with user/item biases and / or a global bias, see AlsArgs
  const float* rhs_vals;
  const float* loss_tgt;
  const float* rhs_init;
  float tgt_const = 1.f;
  float gbias = 0.f;   // conjugate gradient with a global bias: the bias itself (rhs_init = global_bias_base)
};

// launch_ne_stats for the values of handle d: a handle whose values are frozen (rsparse_hip_csc_freeze_values) is scanned once
hipError_t take_value_stats(const DevCSC& d, const float* d_X, int64_t nx, hipStream_t s, const float* d_absmax) {
  if (d.vals_frozen && !d.vstats && hipMalloc(&d.vstats, 2 * sizeof(unsigned)) != hipSuccess) d.vstats = nullptr;
  // (the saved words are ordered behind their scan only on the stream that ran it: a call on another stream scans again and
  // takes the cache over -- ADVICE r05)
  if (d.vals_frozen && d.vstats && d.vstats_valid && d.vstats_stream == s)
    return launch_ne_stats(d_X, nx, d.vals, d.nnz, g_ws.ne_stats, s, d_absmax, d.vstats, nullptr);
  hipError_t e = launch_ne_stats(d_X, nx, d.vals, d.nnz, g_ws.ne_stats, s, d_absmax, nullptr,
                                 (d.vals_frozen && d.vstats) ? d.vstats : nullptr);
  if (e == hipSuccess && d.vals_frozen && d.vstats) { d.vstats_valid = true; d.vstats_stream = s; }
  return e;
}

// d_absmax (nullable, device float): max |X| supplied by the caller -- X is then not scanned for the fp16 operand scales
int run_half_iteration(const rsparse_hip_csc* conf, bool implicit, const float* d_X, float* d_Y,
                       const float* d_XtX, int rank, double lambda, unsigned solver, unsigned cg_steps,
                       int dynamic_lambda, double* d_loss_rows_out, hipStream_t s, const BiasTerms* bias = nullptr,
                       const float* d_absmax = nullptr) {
  if (!conf) return fail(RSPARSE_HIP_ERR_INVALID, "conf is NULL");
  if (!d_X || !d_Y) return fail(RSPARSE_HIP_ERR_INVALID, "X or Y is NULL");
  if (implicit && !d_XtX) return fail(RSPARSE_HIP_ERR_INVALID, "XtX is NULL");
  if (rank <= 0) return fail(RSPARSE_HIP_ERR_INVALID, "rank must be positive");
  if (rank > RSPARSE_HIP_MAX_RANK) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "rank > 256 is not on the device path");
  int rc = check_variant(solver, 0, 0.0);
  if (rc) return rc;
  if ((rc = g_ws.ensure_device())) return rc;
  const DevCSC& d = conf->d;
  // (end of round 6) the exact solver at the ranks 65..127: the rank-128 kernels (matrix-core assembly, a wave per row) on copies
  // padded to 128 beat the routes of a rank below the padded rank by 1.5-5 x (1M x 100k, ms per iteration: explicit rank 100
  // 102 -> 21, implicit 44 -> 29, explicit rank 64 with biases -- a system of order 65 -- 99 -> 28).  A padded coordinate is an exact
  // zero of an exact solve (identity / lambda on its diagonal, zero right-hand side); without per-non-zero bias operands only
  const bool pad_to_128 = solver == RSPARSE_SOLVER_CHOLESKY && !bias && rank > 64 && rank < 128 && zero_padding_is_neutral(implicit, solver, lambda);
  // ... and below rank 64 on copies padded to 64: the one-wave-per-row kernel with its matrix-core assembly exists at the padded rank
  // 64 only (1M x 100k, ms per iteration: rank 10 35 -> 20, rank 20 50 -> 20, rank 32 36 -> 20, rank 48 26 -> 20).  (First measured
  // with a failing cell of the reference's grid -- explicit feedback, lambda = 1000, the factors at 1e-28 --: that was the
  // explicit low-rank kernel's scaled solve overflowing, a bug of the native ranks 64 and 128 too, fixed in wrmf_chol_lr.hip.)
  const bool pad_to_64 = solver == RSPARSE_SOLVER_CHOLESKY && !bias && rank < 64 && zero_padding_is_neutral(implicit, solver, lambda);
  if (((rank % 4 != 0 && rank < 128) || pad_to_128 || pad_to_64) && zero_padding_is_neutral(implicit, solver, lambda)) {
    // A rank that is not a multiple of 4 (the reference's default is 10): the register-resident kernels take their vectors in
    // 16-byte pieces, and the LDS-tile fallback that took these ranks through round 3 is several times slower.  Coordinates of
    // zeros change nothing (wrmf_bias.hip, launch_pad_rows: the same argument as for the biased half-iterations), so the
    // half-iteration runs on copies padded to the next multiple of 4 and the solved rows are copied back.
    const int kp = pad_to_128 ? 128 : (pad_to_64 ? 64 : ((rank + 3) & ~3));
    const size_t nx = (size_t)d.n_rows * kp, ny = (size_t)d.n_cols * kp, ng = (size_t)kp * kp;
    HIP_TRY(g_ws.pad_buf.ensure(nx + ny + ng + 256 + 16));
    float* Xp = g_ws.pad_buf;
    float* Yp = Xp + nx;
    float* Gp = Yp + ny;
    float* rp = Gp + ng;
    hipError_t e;
    if ((e = launch_pad_rows(d_X, rank, 0, rank, kp, d.n_rows, Xp, s)) != hipSuccess) return hip_fail(e, "launch_pad_rows");
    if ((e = launch_pad_rows(d_Y, rank, 0, rank, kp, d.n_cols, Yp, s)) != hipSuccess) return hip_fail(e, "launch_pad_rows");
    if (implicit && (e = launch_pad_gramian(d_XtX, rank, kp, Gp, s)) != hipSuccess) return hip_fail(e, "launch_pad_gramian");
    BiasTerms bp;
    if (bias) {
      bp = *bias;
      if (bias->rhs_init) {   // (rank entries at the caller's: one row of kp, zeros beyond)
        if ((e = launch_pad_rows(bias->rhs_init, rank, 0, rank, kp, 1, rp, s)) != hipSuccess) return hip_fail(e, "launch_pad_rows");
        bp.rhs_init = rp;
      }
    }
    rc = run_half_iteration(conf, implicit, Xp, Yp, implicit ? Gp : nullptr, kp, lambda, solver, cg_steps, dynamic_lambda,
                            d_loss_rows_out, s, bias ? &bp : nullptr, d_absmax);
    if (rc) return rc;
    if (d.n_cols > 0)
      HIP_TRY(hipMemcpy2DAsync(d_Y, (size_t)rank * 4, Yp, (size_t)kp * 4, (size_t)rank * 4, (size_t)d.n_cols,
                               hipMemcpyDeviceToDevice, s));
    return RSPARSE_HIP_OK;
  }
  if (wide_supported(rank)) {
    // ranks 129..256: one kernel family for every solver and operand set (wrmf_wide.hip), no launch schedule
    double* outw = d_loss_rows_out ? d_loss_rows_out : g_ws.scalars;
    if (d.n_cols == 0) {
      HIP_TRY(hipMemsetAsync(outw, 0, sizeof(double), s));
      return RSPARSE_HIP_OK;
    }
    const int grid = wide_als_grid(d.n_cols);
    const int grid_w = wide_cg_wave_grid(d.n_cols) + wide_cg_team_grid(d.n_cols);   // (plain conjugate gradient: wrmf_wide_cg.hip's two launches)
    if ((rc = g_ws.ensure_partials((size_t)grid + (size_t)grid_w))) return rc;
    HIP_TRY(g_ws.wide_m2.ensure(solver == RSPARSE_SOLVER_NNLS ? (size_t)grid * wide_m2_floats_per_wg(rank) : 0));
    HIP_TRY(g_ws.wide_lu.ensure(solver == RSPARSE_SOLVER_CHOLESKY ? (size_t)grid * rank * rank : 0));
    AlsArgs a{};
    a.col_ptrs = d.col_ptrs; a.row_idx = d.row_idx; a.vals = d.vals;
    a.X = d_X; a.Y = d_Y; a.XtX = implicit ? d_XtX : nullptr;
    a.n_cols = d.n_cols; a.k = rank; a.cg_steps = (int)cg_steps;
    a.lambda = (float)lambda; a.lambda_loss = lambda; a.dynamic_lambda = dynamic_lambda ? 1 : 0;
    a.loss_partials = g_ws.partials; a.fail_counter = g_ws.fails;
    a.rhs_vals = bias ? bias->rhs_vals : nullptr;
    a.loss_tgt = bias ? bias->loss_tgt : nullptr;
    a.rhs_init = bias ? bias->rhs_init : nullptr;
    a.loss_tgt_const = bias ? bias->tgt_const : 1.f;
    a.gbias = (solver == RSPARSE_SOLVER_CONJUGATE_GRADIENT && implicit && bias) ? bias->gbias : 0.f;
    // plain conjugate gradient: the operator form, one wave per row (teams of 8 for the rows beyond kWideCgMaxLen non-zeros) -- no k x k
    // system; everything else: wrmf_wide.hip
    const bool wave_cg = wide_cg_wave_supported(a, solver) && (d.q_order || d.max_len <= kWideCgMaxLen);
    hipError_t we = wave_cg ? launch_wide_cg_wave(a, implicit, kWideCgMaxLen, d.max_len > kWideCgMaxLen ? d.q_order : nullptr, 0, s)
                            : launch_als_wide(a, implicit, solver, g_ws.wide_m2, g_ws.wide_lu, s);
    if (we != hipSuccess) return hip_fail(we, wave_cg ? "launch_wide_cg_wave" : "launch_als_wide");
    if ((we = launch_sum_partials(g_ws.partials, wave_cg ? (size_t)grid_w : (size_t)grid, outw, s, g_ws.partials + g_ws.partial_slots())) != hipSuccess)
      return hip_fail(we, "launch_sum_partials");
    return RSPARSE_HIP_OK;
  }
  const bool cg = solver == RSPARSE_SOLVER_CONJUGATE_GRADIENT;
  const bool cgq = cg && use_cgq(rank, d_X, d_Y);
  QSchedule qs;
  qs.order = d.q_order;
  qs.cfg = d.q_cfg;
  qs.pair_first = d.q_pair_first;
  for (int b = 0; b < 7; b++) qs.off[b] = d.q_off[b];
  // (the global-bias CG keeps bucket 1 on the 8-wave kernel: no 4-wave launch, no loss slots for one)
  qs.team4_first = (implicit && bias && bias->gbias != 0.f) ? d.q_off[2] : d.q_team4_first;
  qs.team4_wide_first = (implicit && bias && bias->gbias != 0.f) ? d.q_off[2] : d.q_team4_wide_first;
  qs.pair_wide = cgp_wide_supported(rank, implicit, implicit && bias && bias->gbias != 0.f);
  qs.pair_quad = cgp_quad_supported(rank, implicit, implicit && bias && bias->gbias != 0.f);
  // round 6, rank 128, implicit conjugate gradient without bias operands: the rows of 513..kCgMfMax non-zeros of the first bucket on
  // the wave-per-row kernel of wrmf_cg_mf.hip, the giant rows (a prefix of the order) on the normal-equation kernel's second lists
  const bool cg_mf = cgq && implicit && !bias && cg_mf_supported(rank, implicit) && d.q_order && d.q_off[1] > d.q_n_nec;
  if (cg_mf) {
    qs.mf_rows = d.q_order + d.q_n_nec;
    qs.mf_n = d.q_off[1] - d.q_n_nec;
  }
  // solver == CHOLESKY: the rows beyond 512 non-zeros are assembled by the normal-equation kernel (matrix cores, one pass)
  // and solved exactly there (a.ne_chol); wrmf_chol.hip's kernel then skips them
  // (the lower threshold pays at rank 65..128 only: at rank <= 64 wrmf_chol.hip's kernel is cheaper than the fixed cost of
  // the tile solve up to 512 non-zeros -- config 5 with Cholesky 4.5 against 4.1 iterations/s)
  // (round 6, rank 65..128: the rows of 65..512 non-zeros go to the wave-per-row kernel of wrmf_chol_mf.hip instead -- the
  // normal-equation launch keeps the rows beyond 512, its CG lists)
  const bool chol_mf = chol_mf_supported(rank) && !cg && solver == RSPARSE_SOLVER_CHOLESKY && !bias && d.q_order && ne_supported(rank) &&
                       use_cgq(rank, d_X, d_Y) && d.q_lr_first > d.q_off[1];
  const int mf_first = d.q_off[1];
  const int n_mf = chol_mf ? d.q_lr_first - mf_first : 0;
  const bool nec_lists = padded_rank(rank) > 64 && d.q_nec.wg > 0 && !chol_mf;
  const bool ne_chol = !cg && solver == RSPARSE_SOLVER_CHOLESKY && !bias && (nec_lists || d.q_ne.wg > 0 || chol_mf) &&
                       ne_supported(rank) && use_cgq(rank, d_X, d_Y);
  // which lists the normal-equation launch walks: the rows beyond kCgMfMax non-zeros beside wrmf_cg_mf.hip and for the exact
  // solve's own lists; else the streamed bucket's -- many lists where two workgroups per CU pick them up (only for implicit
  // feedback at rank 97..128: the fp16 QUAD kernel of wrmf_ne.hip), else one list per slot
  qs.ne = (cg_mf || (ne_chol && nec_lists)) ? d.q_nec : ((implicit && padded_rank(rank) == 128) ? d.q_ne : d.q_ne1);
  const size_t chol_base = chol2_loss_slots(d.n_cols);
  const size_t slots = cgq ? cgq_loss_slots(qs, rank, implicit) : (cg ? cg_loss_slots(d.n_cols, d.n_long)
                                   : (solver == RSPARSE_SOLVER_NNLS ? chol_loss_slots(d.n_cols)
                                      : chol_base + (ne_chol ? (size_t)(qs.ne.entries + qs.ne.nsplit) : 0) +
                                            (size_t)(chol_mf ? chol_mf_loss_slots(n_mf, implicit) : 0) + (size_t)kLuGrid));
  if ((rc = g_ws.ensure_partials(slots))) return rc;
  double* out = d_loss_rows_out ? d_loss_rows_out : g_ws.scalars;
  if (d.n_cols == 0) {
    HIP_TRY(hipMemsetAsync(out, 0, sizeof(double), s));
    return RSPARSE_HIP_OK;
  }
  AlsArgs a;
  a.col_ptrs = d.col_ptrs; a.row_idx = d.row_idx; a.vals = d.vals;
  a.X = d_X; a.Y = d_Y; a.XtX = implicit ? d_XtX : nullptr;
  a.long_rows = d.n_long ? d.q_order : nullptr; a.n_long = d.n_long; a.n_cols = d.n_cols;
  a.chol_long_rows = d.q_order; a.n_chol_long = d.q_order ? d.q_n_chol_long : 0;
  a.chol_list = nullptr; a.chol_first = 0; a.chol_n_main = 0; a.chol_empty_first = 0;
  a.lr_rows = nullptr; a.n_lr = 0; a.lr_flags = nullptr; a.lr_M = nullptr; a.lr_n_gt32 = a.lr_n_gt16 = a.lr_n_gt48 = -1; a.lrx = 0;
  a.nnls_order = solver == RSPARSE_SOLVER_NNLS ? d.q_order : nullptr;
  a.nnls_lhs = nullptr;
  if (solver == RSPARSE_SOLVER_NNLS && padded_rank(rank) == 128) {   // (the wide family's buffer: no rank uses both)
    HIP_TRY(g_ws.wide_m2.ensure(chol_loss_slots(d.n_cols) * (size_t)128 * 128));
    a.nnls_lhs = g_ws.wide_m2;
  }
  a.k = rank; a.cg_steps = (int)cg_steps;
  a.lambda = (float)lambda; a.lambda_loss = lambda; a.dynamic_lambda = dynamic_lambda ? 1 : 0;
  a.loss_partials = g_ws.partials; a.fail_counter = g_ws.fails; a.zero_row = g_ws.zero_row;
  a.fail_rows = g_ws.fails + 4; a.fail_cap = kFailCap;
  a.rhs_vals = bias ? bias->rhs_vals : nullptr;
  a.loss_tgt = bias ? bias->loss_tgt : nullptr;
  a.rhs_init = bias ? bias->rhs_init : nullptr;
  a.loss_tgt_const = bias ? bias->tgt_const : 1.f;
  const bool gb_cg = cg && implicit && bias && bias->gbias != 0.f;   // cg_solver_implicit_global_bias
  a.gbias = gb_cg ? bias->gbias : 0.f;
  a.ne_r0 = nullptr; a.ne_r0_slot = nullptr;
  a.tscr = nullptr; a.stream_off = d.q_stream_off; a.stream_nnz = d.q_nnz[0];
  a.ne_stats = nullptr; a.wave_stats = nullptr; a.mf_XtX = nullptr;
  a.ne_segs = nullptr; a.ne_seg_scratch = nullptr; a.ne_seg_flags = nullptr;
  a.ne_chol = ne_chol ? 1 : 0;
  a.ne_chol_min = nec_lists ? kCgMfMax : kNeMinLen;
  if (d.q_order && solver == RSPARSE_SOLVER_CHOLESKY) {
    // the k x k kernel's own rows as ranges of the length-sorted order: behind the prefix that the normal-equation launch
    // (or the LONG launch) takes, down to the short rows of the low-rank kernel, and the empty rows at the end
    const int first = chol_mf ? d.q_lr_first : (ne_chol ? (nec_lists ? d.q_n_nec : d.q_off[1]) : d.q_n_chol_long);
    a.chol_list = d.q_order;
    a.chol_first = first;
    a.chol_n_main = std::max(0, d.q_lr_first - first);
    a.chol_empty_first = d.q_lr_first + d.q_n_lr;
  }
  if ((cgq || ne_chol) && qs.ne.nseg > 0 && ne_supported(rank)) {
    HIP_TRY(g_ws.ne_seg_scratch.ensure((size_t)qs.ne.nseg * (size_t)kNeSegFloats));
    HIP_TRY(g_ws.ne_seg_flags.ensure((size_t)qs.ne.nseg));
    a.ne_segs = qs.ne.segs; a.ne_seg_scratch = g_ws.ne_seg_scratch; a.ne_seg_flags = g_ws.ne_seg_flags;
  }
  // the statistics of the values and of X in g_ws.ne_stats (take_value_stats): scanned by the first launch set-up below that
  // wants them, once per call
  bool stats_taken = false;
  auto want_stats = [&]() -> int {
    if (stats_taken) return RSPARSE_HIP_OK;
    hipError_t se = take_value_stats(d, d_X, (int64_t)d.n_rows * rank, s, d_absmax);
    if (se != hipSuccess) return hip_fail(se, "launch_ne_stats");
    stats_taken = true;
    return RSPARSE_HIP_OK;
  };
  if (chol_mf) {   // the operand scales of its matrix-core assembly (max |X|, max c)
    if ((rc = want_stats())) return rc;
    a.wave_stats = g_ws.ne_stats;
    if (implicit) {
      a.ne_stats = g_ws.ne_stats;
      a.mf_XtX = d_XtX;
      if (rank != 128) {
        HIP_TRY(g_ws.mf_G.ensure((size_t)128 * 128));
        hipError_t pe = launch_pad_gramian(d_XtX, rank, 128, g_ws.mf_G, s);
        if (pe != hipSuccess) return hip_fail(pe, "launch_pad_gramian");
        a.mf_XtX = g_ws.mf_G;
      }
    }
  }
  if (!a.ne_stats && (cgq || ne_chol) && implicit && (qs.ne.wg > 0 || qs.mf_n > 0) && ne_supported(rank) && (!bias || gb_cg)) {
    // operand scales of the fp16 normal-equation kernel (and whether it may run at all), decided on the device
    if ((rc = want_stats())) return rc;
    a.ne_stats = g_ws.ne_stats;
    if (gb_cg && cgq) {   // the long rows' share of the first residual: base - g X_nnz (c - 1), one more pass over them
      const int n_ne = d.q_off[1];
      HIP_TRY(g_ws.gb_r0.ensure((size_t)n_ne * rank));
      HIP_TRY(g_ws.gb_slot.ensure((size_t)d.n_cols));
      hipError_t ge = launch_gb_row_terms(a, d.q_order, n_ne, g_ws.gb_r0, g_ws.gb_slot, s);
      if (ge != hipSuccess) return hip_fail(ge, "launch_gb_row_terms");
      a.ne_r0 = g_ws.gb_r0; a.ne_r0_slot = g_ws.gb_slot;
    }
  }
  // ranks the normal-equation kernel does not take (<= 32): the streamed CG bucket keeps its per-sweep dot products in
  // an HBM scratch instead of re-gathering for the loss
  if (cgq && !ne_supported(rank) && d.q_stream_off && d.q_nnz[0] > 0 && cg_steps >= 1 && cg_steps <= 4) {
    HIP_TRY(g_ws.tscr.ensure((size_t)(cg_steps + 1) * (size_t)d.q_nnz[0]));
    a.tscr = g_ws.tscr;
  }
  if (!cg && solver == RSPARSE_SOLVER_CHOLESKY && d.q_order && d.q_n_lr > 0 && chol_lr_supported(a, implicit)) {
    // low-rank form for the short rows; "some confidence < 1" comes from the values scan of launch_ne_stats (word 2)
    HIP_TRY(g_ws.lr_M.ensure((size_t)3 * 128 * 128));
    // (with the long rows on the normal-equation kernel the full statistics were just taken)
    // max |X| too: the low-rank kernel scales its fp16 operand terms by it
    if ((rc = want_stats())) return rc;
    a.lr_rows = d.q_order + d.q_lr_first; a.n_lr = d.q_n_lr; a.lr_flags = g_ws.ne_stats + 2; a.lr_M = g_ws.lr_M;
    a.lr_n_gt32 = d.q_gt32 - d.q_lr_first; a.lr_n_gt16 = d.q_pair_first - d.q_lr_first;
    a.lr_n_gt48 = d.q_gt48 - d.q_lr_first;
  }
  const bool chol = !cg && solver == RSPARSE_SOLVER_CHOLESKY;
  if (chol && d.q_order && d.q_n_lr > 0 && chol_lrx_supported(a, implicit)) {
    // explicit feedback, ranks 64 / 128: the rows of 1..64 ratings in push-through form, one wave per pass
    if ((rc = want_stats())) return rc;
    a.wave_stats = g_ws.ne_stats;
    a.lr_rows = d.q_order + d.q_lr_first; a.n_lr = d.q_n_lr; a.lrx = 1;
    a.lr_n_gt32 = d.q_gt32 - d.q_lr_first; a.lr_n_gt16 = d.q_pair_first - d.q_lr_first;
    a.lr_n_gt48 = d.q_gt48 - d.q_lr_first;
  }
  if (chol && chol_wave_supported(rank) && padded_rank(rank) == 64) {
    // rank 33..64, one wave per row: the assembly runs on the matrix cores from fp16 operand terms scaled by max |X| (and max c)
    if ((rc = want_stats())) return rc;
    a.wave_stats = g_ws.ne_stats;
  }
  if (chol) {
    hipError_t fe = launch_fail_roll(g_ws.fails, s);
    if (fe != hipSuccess) return hip_fail(fe, "launch_fail_roll");
  }
  hipEvent_t* ev = g_prof.begin();
  if (chol && ev) HIP_TRY(hipEventRecord(ev[0], s));   // Cholesky: [0] normal-equation launch, [1] low-rank, [2] k x k, [3] wave-per-row (rank 65..128), [4] loss
  if (ne_chol && qs.ne.wg > 0 && mf_first != 0) {
    hipError_t ne = launch_als_ne(a, qs, implicit, g_ws.partials + chol_base, s, ev);
    if (ne != hipSuccess) return hip_fail(ne, "launch_als_ne");
  }
  hipError_t e = cgq ? launch_als_cgq(a, qs, implicit, s, ev)
                     : (cg ? launch_als_cg(a, implicit, s, ev)
                           : (solver == RSPARSE_SOLVER_NNLS
                                  ? launch_als_nnls(a, implicit, s, ev)
                                  : launch_als_chol2(a, implicit, s, ev ? ev + 1 : nullptr)));
  if (e != hipSuccess) return hip_fail(e, cgq ? "launch_als_cgq" : (cg ? "launch_als_cg" : "launch_als_chol"));
  if (chol_mf) {   // (launch_als_chol2 recorded ev[3] behind its kernels)
    const size_t mf_base = chol_base + (size_t)(qs.ne.entries + qs.ne.nsplit);
    hipError_t me = launch_als_chol_mf(a, implicit, d.q_order + mf_first, n_mf, (int)mf_base, s, ev ? ev + 3 : nullptr);
    if (me != hipSuccess) return hip_fail(me, "launch_als_chol_mf");
  }
  if (chol && ev) HIP_TRY(hipEventRecord(ev[4], s));
  if (chol) {
    // rows whose factorisation met a non-positive pivot: the general solver, as arma::solve falls back to (wrmf_lu.hip).
    // The counters are per call: a previous call's count was taken by rsparse_hip_take_numeric_failures or is added to.
    if ((e = launch_als_lu_fallback(a, implicit, slots - (size_t)kLuGrid, s)) != hipSuccess)
      return hip_fail(e, "launch_als_lu_fallback");
  }
  e = launch_sum_partials(g_ws.partials, slots, out, s, g_ws.partials + g_ws.partial_slots());
  if (e != hipSuccess) return hip_fail(e, "launch_sum_partials");
  if (ev) {
    const int last = cgq ? 7 : (chol ? 5 : 3);
    HIP_TRY(hipEventRecord(ev[last], s));
    g_prof.have = true;
    g_prof.nseg = last;
  }
  return RSPARSE_HIP_OK;
}

// als_explicit<T> with_biases (inst/include/wrmf_explicit.hpp:41-64,86-91,113-127) by re-packing: see wrmf_bias.hip.
int run_half_iteration_explicit_biased(const rsparse_hip_csc* conf, const float* d_X, float* d_Y, int rank, double lambda,
                                       unsigned solver, unsigned cg_steps, int dynamic_lambda, int is_x_bias_last_row,
                                       double* d_loss_rows_out, hipStream_t s) {
  if (!conf) return fail(RSPARSE_HIP_ERR_INVALID, "conf is NULL");
  if (!d_X || !d_Y) return fail(RSPARSE_HIP_ERR_INVALID, "X or Y is NULL");
  if (rank < 2) return fail(RSPARSE_HIP_ERR_INVALID, "with_biases needs rank >= 2 (a row of ones and a bias row)");
  if (rank > RSPARSE_HIP_MAX_RANK) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "rank > 256 is not on the device path");
  int rc = g_ws.ensure_device();
  if (rc) return rc;
  const DevCSC& d = conf->d;
  const int k1 = rank - 1;
  const int xoff = is_x_bias_last_row ? 0 : 1;       // first kept row of X_nnz            (:88)
  const int xb = is_x_bias_last_row ? rank - 1 : 0;  // row of X holding the x biases       (:59-64)
  const int ioff = is_x_bias_last_row ? 1 : 0;       // first kept entry of the warm start  (:90)
  const int ooff = is_x_bias_last_row ? 0 : 1;       // head / tail of Y.col(i)             (:115-127)
  // the copies are padded to a multiple of 4 (wrmf_bias.hip: why) -- unless the padding would make the systems singular
  const int k1p = zero_padding_is_neutral(false, solver, lambda) ? std::min((k1 + 3) & ~3, RSPARSE_HIP_MAX_RANK) : k1;
  const size_t nx = (size_t)d.n_rows * k1p, ny = (size_t)d.n_cols * k1p, nv = (size_t)std::max<int64_t>(d.nnz, 1);
  HIP_TRY(g_ws.bias_buf.ensure(nx + ny + nv + 16));
  float* Xp = g_ws.bias_buf;
  float* Yp = Xp + nx;
  float* vp = Yp + ny;
  hipError_t e;
  if ((e = launch_pad_rows(d_X, rank, xoff, k1, k1p, d.n_rows, Xp, s)) != hipSuccess) return hip_fail(e, "launch_pad_rows");
  if ((e = launch_pad_rows(d_Y, rank, ioff, k1, k1p, d.n_cols, Yp, s)) != hipSuccess) return hip_fail(e, "launch_pad_rows");
  e = launch_bias_shift_values(d.vals, d.row_idx, d_X, rank, xb, d.nnz, vp, s);
  if (e != hipSuccess) return hip_fail(e, "launch_bias_shift_values");
  rsparse_hip_csc shifted;   // same sparsity and schedule, shifted ratings (a view: it owns nothing and is never destroyed)
  shifted.d = conf->d; shifted.device = conf->device;
  shifted.d.vals_frozen = false; shifted.d.vstats_valid = false; shifted.d.vstats = nullptr;   // (its values are this call's)
  shifted.d.vals = vp;
  rc = run_half_iteration(&shifted, false, Xp, Yp, nullptr, k1p, lambda, solver, cg_steps, dynamic_lambda,
                          d_loss_rows_out, s);
  if (rc) return rc;
  if (d.n_cols > 0)
    HIP_TRY(hipMemcpy2DAsync(d_Y + ooff, (size_t)rank * 4, Yp, (size_t)k1p * 4, (size_t)k1 * 4, (size_t)d.n_cols,
                             hipMemcpyDeviceToDevice, s));
  return RSPARSE_HIP_OK;
}

// als_implicit<T> with_biases, Cholesky / NNLS (inst/include/wrmf_implicit.hpp:114-154,186-252,256-270) by re-packing
// plus three extra operands of the solve kernels (AlsArgs::rhs_vals / loss_tgt / rhs_init).  d_XtX is the
// (rank-1) x (rank-1) Gramian of X without its x_bias row, ridge included (R/model_WRMF.R:474-486).
int run_half_iteration_implicit_biased(const rsparse_hip_csc* conf, const float* d_X, float* d_Y, const float* d_XtX,
                                       int rank, double lambda, unsigned solver, int is_x_bias_last_row,
                                       double* d_loss_rows_out, hipStream_t s, double global_bias = 0.0,
                                       bool dbl_threshold = false) {
  if (!conf) return fail(RSPARSE_HIP_ERR_INVALID, "conf is NULL");
  if (!d_X || !d_Y || !d_XtX) return fail(RSPARSE_HIP_ERR_INVALID, "X, Y or XtX is NULL");
  if (rank < 2) return fail(RSPARSE_HIP_ERR_INVALID, "with_biases needs rank >= 2 (a row of ones and a bias row)");
  if (rank > RSPARSE_HIP_MAX_RANK) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "rank > 256 is not on the device path");
  int rc = g_ws.ensure_device();
  if (rc) return rc;
  const DevCSC& d = conf->d;
  const int k1 = rank - 1;
  const int xoff = is_x_bias_last_row ? 0 : 1, xb = is_x_bias_last_row ? rank - 1 : 0;
  const int ioff = is_x_bias_last_row ? 1 : 0, ooff = is_x_bias_last_row ? 0 : 1;
  const int k1p = std::min((k1 + 3) & ~3, RSPARSE_HIP_MAX_RANK);   // the copies are padded to a multiple of 4 (wrmf_bias.hip: why)
  const size_t nx = (size_t)d.n_rows * k1p, ny = (size_t)d.n_cols * k1p, nv = (size_t)std::max<int64_t>(d.nnz, 1);
  const size_t nscr = bias_rhs_init_scratch_floats(), ng = (size_t)k1p * k1p;
  HIP_TRY(g_ws.bias_buf.ensure(nx + ny + 2 * nv + nscr + ng + 16));
  float* Xp = g_ws.bias_buf;
  float* Yp = Xp + nx;
  float* rcoef = Yp + ny;
  float* tgt = rcoef + nv;
  float* scratch = tgt + nv;
  float* rinit = scratch + (nscr - 256);   // (256 entries, zeros beyond k1)
  float* Gp = scratch + nscr;
  hipError_t e;
  if ((e = launch_pad_rows(d_X, rank, xoff, k1, k1p, d.n_rows, Xp, s)) != hipSuccess) return hip_fail(e, "launch_pad_rows");
  if ((e = launch_pad_rows(d_Y, rank, ioff, k1, k1p, d.n_cols, Yp, s)) != hipSuccess) return hip_fail(e, "launch_pad_rows");
  const float* G_use = d_XtX;
  if (k1p != k1) {
    if ((e = launch_pad_gramian(d_XtX, k1, k1p, Gp, s)) != hipSuccess) return hip_fail(e, "launch_pad_gramian");
    G_use = Gp;
  }
  const float gb = has_global_bias(global_bias, dbl_threshold) ? (float)global_bias : 0.f;
  e = launch_bias_implicit_terms(d.vals, d.row_idx, d_X, rank, xb, d.nnz, gb, rcoef, tgt, s);
  if (e != hipSuccess) return hip_fail(e, "launch_bias_implicit_terms");
  if ((e = launch_bias_rhs_init(d_X, rank, xoff, k1, xb, gb, d.n_rows, scratch, rinit, s)) != hipSuccess)
    return hip_fail(e, "launch_bias_rhs_init");
  BiasTerms bt{rcoef, tgt, rinit};
  rc = run_half_iteration(conf, true, Xp, Yp, G_use, k1p, lambda, solver, 0, 0, d_loss_rows_out, s, &bt);
  if (rc) return rc;
  if (d.n_cols > 0)
    HIP_TRY(hipMemcpy2DAsync(d_Y + ooff, (size_t)rank * 4, Yp, (size_t)k1p * 4, (size_t)k1 * 4, (size_t)d.n_cols,
                             hipMemcpyDeviceToDevice, s));
  return RSPARSE_HIP_OK;
}

// als_implicit<T> with a global bias and no user/item biases, Cholesky / NNLS (inst/include/wrmf_implicit.hpp:108-112,
// 155-157, 228-229, 262-264): rhs = X_nnz c + global_bias_base with global_bias_base = -global_bias * rowSums(X)
// (computed here when d_base_in is NULL -- initialize_bias_base -- and returned through d_base_out if given), every row
// is solved (empty ones too, :178), and the loss compares x_j.y with 1 - global_bias.
int run_half_iteration_implicit_global(const rsparse_hip_csc* conf, const float* d_X, float* d_Y, const float* d_XtX,
                                       int rank, double lambda, unsigned solver, unsigned cg_steps, double global_bias,
                                       const float* d_base_in, float* d_base_out, double* d_loss_rows_out,
                                       hipStream_t s, const float* d_absmax = nullptr) {
  if (!conf) return fail(RSPARSE_HIP_ERR_INVALID, "conf is NULL");
  if (!d_X || !d_Y || !d_XtX) return fail(RSPARSE_HIP_ERR_INVALID, "X, Y or XtX is NULL");
  if (rank <= 0) return fail(RSPARSE_HIP_ERR_INVALID, "rank must be positive");
  if (rank > RSPARSE_HIP_MAX_RANK) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "rank > 256 is not on the device path");
  int rc = g_ws.ensure_device();
  if (rc) return rc;
  const DevCSC& d = conf->d;
  const size_t nscr = bias_rhs_init_scratch_floats();
  HIP_TRY(g_ws.bias_buf.ensure(nscr + 16));
  float* scratch = g_ws.bias_buf;
  float* rinit = scratch + (nscr - 256);
  if (d_base_in) {
    HIP_TRY(hipMemcpyAsync(rinit, d_base_in, (size_t)rank * 4, hipMemcpyDeviceToDevice, s));
  } else {
    hipError_t e = launch_bias_rhs_init(d_X, rank, 0, rank, -1, (float)global_bias, d.n_rows, scratch, rinit, s);
    if (e != hipSuccess) return hip_fail(e, "launch_bias_rhs_init");
  }
  if (d_base_out) HIP_TRY(hipMemcpyAsync(d_base_out, rinit, (size_t)rank * 4, hipMemcpyDeviceToDevice, s));
  // conjugate gradient: cg_solver_implicit_global_bias (wrmf_implicit.hpp:35-57,203) from the warm start in d_Y
  const bool cg = solver == RSPARSE_SOLVER_CONJUGATE_GRADIENT;
  BiasTerms bt{nullptr, nullptr, rinit, (float)(1.0 - global_bias), cg ? (float)global_bias : 0.f};
  return run_half_iteration(conf, true, d_X, d_Y, d_XtX, rank, lambda, solver, cg ? cg_steps : 0, 0, d_loss_rows_out, s,
                            &bt, d_absmax);
}

// Body of the two stateless fp32 drop-ins (the `_double` ones: wrmf_f64_capi.cpp): stateless_half_iteration on a handle
// made from the host arrays, with the four half-iterations of this side.
int stateless(bool implicit, int n_rows, int n_cols, const int32_t* col_ptrs, const int32_t* row_indices,
              const double* values, const float* X, float* Y, const float* XtX, const float* cnt_X, int rank, double lambda,
              unsigned solver, unsigned cg_steps, int dynamic_lambda, double* loss_out, int with_biases = 0,
              int is_x_bias_last_row = 0, double global_bias = 0.0, float* global_bias_base = nullptr,
              int global_bias_base_len = 0, int initialize_bias_base = 1) {
  int rc = check_common(n_rows, n_cols, col_ptrs, X, Y, rank);
  if (rc) return rc;
  if ((rc = check_variant(solver, with_biases, global_bias, implicit))) return rc;
  rsparse_hip_csc* conf = nullptr;   // (validates the arrays; the values become floats here)
  if ((rc = rsparse_hip_csc_create_host(n_rows, n_cols, col_ptrs, row_indices, values, &conf))) return rc;
  CscGuard guard{conf};
  const bool use_base = implicit && !with_biases && has_global_bias(global_bias);   // the threshold of float
  auto scratch = [](SumScratch& w) {   // (the half-iterations size the partials themselves)
    int rc = g_ws.ensure_device();
    w = {g_ws.partials, g_ws.scalars};
    return rc;
  };
  auto half = [&](const float* dX, float* dY, const float* dG, const float* base_in, float* base_out, double* d_loss) {
    if (use_base)
      return run_half_iteration_implicit_global(conf, dX, dY, dG, rank, lambda, solver, cg_steps, global_bias, base_in, base_out,
                                                d_loss, nullptr);
    if (with_biases && implicit)
      return run_half_iteration_implicit_biased(conf, dX, dY, dG, rank, lambda, solver, is_x_bias_last_row, d_loss, nullptr,
                                                global_bias);
    if (with_biases)
      return run_half_iteration_explicit_biased(conf, dX, dY, rank, lambda, solver, cg_steps, dynamic_lambda, is_x_bias_last_row,
                                                d_loss, nullptr);
    return run_half_iteration(conf, implicit, dX, dY, dG, rank, lambda, solver, cg_steps, dynamic_lambda, d_loss, nullptr);
  };
  return stateless_half_iteration(scratch, half, implicit, n_rows, n_cols, conf->d.nnz, X, Y, XtX, cnt_X, rank, lambda,
                                  dynamic_lambda, loss_out, with_biases, is_x_bias_last_row, use_base, global_bias_base,
                                  global_bias_base_len, initialize_bias_base);
}

}  // namespace

namespace rsparse_hip {
int* capi_fail_counters() { return g_ws.ensure_device() ? nullptr : g_ws.fails; }
void capi_fail_carry_add(int64_t unresolved, int64_t fallback) {
  g_fail_carry[0] += unresolved;
  g_fail_carry[1] += fallback;
}
StaleFailures::StaleFailures() { rsparse_hip_take_numeric_failures(&unresolved, &fallback); }
void prof_note(hipEvent_t* ev_slot, const void* kernel_fn) {
  if (!ev_slot || !g_prof.on) return;
  const ptrdiff_t i = ev_slot - g_prof.ev;
  if (i >= 0 && i < 10 && !g_prof.kern[i]) g_prof.kern[i] = kernel_fn;   // the first launch of a segment names it
}
}  // namespace rsparse_hip

extern "C" {

const char* rsparse_hip_last_error(void) { return g_err.c_str(); }
int rsparse_hip_abi_version(void) { return 6; }

int rsparse_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int rsparse_hip_set_device(int device) {
  HIP_TRY(hipSetDevice(device));
  return RSPARSE_HIP_OK;
}

int rsparse_hip_csc_create_host(int n_rows, int n_cols, const int32_t* col_ptrs, const int32_t* row_indices,
                                const double* values, rsparse_hip_csc** out) {
  if (!out) return fail(RSPARSE_HIP_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (n_rows < 0 || n_cols < 0) return fail(RSPARSE_HIP_ERR_INVALID, "negative matrix dimension");
  if (!col_ptrs) return fail(RSPARSE_HIP_ERR_INVALID, "col_ptrs is NULL");
  const int64_t nnz = (int64_t)col_ptrs[n_cols] - col_ptrs[0];
  if (col_ptrs[0] != 0 || nnz < 0) return fail(RSPARSE_HIP_ERR_INVALID, "col_ptrs must start at 0 and be non-decreasing");
  if (nnz > 0 && (!row_indices || !values)) return fail(RSPARSE_HIP_ERR_INVALID, "row_indices or values is NULL");
  for (int64_t e = 0; e < nnz; e++)
    if (row_indices[e] < 0 || row_indices[e] >= n_rows)
      return fail(RSPARSE_HIP_ERR_INVALID, "row index out of range");
  rsparse_hip_csc* m = new rsparse_hip_csc();
  CscGuard guard{m};
  if (hipGetDevice(&m->device) != hipSuccess) return fail(RSPARSE_HIP_ERR_RUNTIME, "no HIP device");
  DevCSC& d = m->d;
  d.n_rows = n_rows; d.n_cols = n_cols; d.nnz = nnz;
  int32_t *dp = nullptr, *di = nullptr;
  float* dv = nullptr;
  HIP_TRY(hipMalloc(&dp, ((size_t)n_cols + 1) * 4));
  m->owned.push_back(dp);
  d.col_ptrs = dp;
  HIP_TRY(hipMalloc(&di, (size_t)std::max<int64_t>(nnz, 4) * 4));
  m->owned.push_back(di);
  d.row_idx = di;
  HIP_TRY(hipMalloc(&dv, (size_t)std::max<int64_t>(nnz, 4) * 4));
  m->owned.push_back(dv);
  d.vals = dv;
  HIP_TRY(hipMemcpy(dp, col_ptrs, ((size_t)n_cols + 1) * 4, hipMemcpyHostToDevice));
  if (nnz) {
    HIP_TRY(hipMemcpy(di, row_indices, (size_t)nnz * 4, hipMemcpyHostToDevice));
    // values: f64 on the wire (dgCMatrix@x), f32 once resident -- the conversion the reference does per
    // column with arma::conv_to (wrmf_implicit.hpp:182-183)
    std::vector<float> v32(values, values + nnz);
    HIP_TRY(hipMemcpy(dv, v32.data(), (size_t)nnz * 4, hipMemcpyHostToDevice));
  }
  if (int rc = build_schedule(*m, col_ptrs)) return rc;
  guard.c = nullptr;
  *out = m;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_csc_create_device(int n_rows, int n_cols, const int32_t* d_col_ptrs, const int32_t* d_row_indices,
                                  const float* d_values, rsparse_hip_csc** out) {
  if (!out) return fail(RSPARSE_HIP_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (n_rows < 0 || n_cols < 0) return fail(RSPARSE_HIP_ERR_INVALID, "negative matrix dimension");
  if (!d_col_ptrs) return fail(RSPARSE_HIP_ERR_INVALID, "col_ptrs is NULL");
  std::vector<int32_t> hp((size_t)n_cols + 1);
  HIP_TRY(hipMemcpy(hp.data(), d_col_ptrs, hp.size() * 4, hipMemcpyDeviceToHost));
  if (hp[0] != 0) return fail(RSPARSE_HIP_ERR_INVALID, "col_ptrs must start at 0");
  const int64_t nnz = hp[n_cols];
  if (nnz > 0 && (!d_row_indices || !d_values)) return fail(RSPARSE_HIP_ERR_INVALID, "row_indices or values is NULL");
  if (nnz < 0) return fail(RSPARSE_HIP_ERR_INVALID, "col_ptrs must be non-decreasing");
  for (int c = 0; c < n_cols; c++)
    if (hp[(size_t)c + 1] < hp[(size_t)c]) return fail(RSPARSE_HIP_ERR_INVALID, "col_ptrs must be non-decreasing");
  {   // the same validation the host constructor does: the kernels gather X[row_index] unchecked
    int bad = 0;
    HIP_TRY(check_row_indices_device(d_row_indices, nnz, n_rows, nullptr, &bad));
    if (bad) return fail(RSPARSE_HIP_ERR_INVALID, "row index out of range");
  }
  rsparse_hip_csc* m = new rsparse_hip_csc();
  CscGuard guard{m};
  if (hipGetDevice(&m->device) != hipSuccess) return fail(RSPARSE_HIP_ERR_RUNTIME, "no HIP device");
  DevCSC& d = m->d;
  d.n_rows = n_rows; d.n_cols = n_cols; d.nnz = nnz;   // (the caller's arrays: not in m->owned)
  d.col_ptrs = d_col_ptrs; d.row_idx = d_row_indices; d.vals = d_values;
  if (int rc = build_schedule(*m, hp.data())) return rc;
  guard.c = nullptr;
  *out = m;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_csc_transpose_device(int n_rows, int n_cols, const int32_t* d_p, const int32_t* d_i, const float* d_x,
                                     int32_t* d_pt, int32_t* d_it, float* d_xt, void* stream) {
  if (n_rows < 0 || n_cols < 0) return fail(RSPARSE_HIP_ERR_INVALID, "negative matrix dimension");
  if (!d_p || !d_pt) return fail(RSPARSE_HIP_ERR_INVALID, "col_ptrs (input or output) is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int32_t ends[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(&ends[0], d_p, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&ends[1], d_p + n_cols, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int64_t nnz = (int64_t)ends[1] - ends[0];
  if (ends[0] != 0 || nnz < 0) return fail(RSPARSE_HIP_ERR_INVALID, "col_ptrs must start at 0 and be non-decreasing");
  if (nnz > 0 && (!d_i || !d_x || !d_it || !d_xt)) return fail(RSPARSE_HIP_ERR_INVALID, "index or value array is NULL");
  int bad = 0;
  hipError_t e = transpose_csc_device(n_rows, n_cols, nnz, d_p, d_i, d_x, d_pt, d_it, d_xt, s, &bad);
  if (bad) return fail(RSPARSE_HIP_ERR_INVALID, "row index out of range");
  if (e != hipSuccess) return hip_fail(e, "transpose_csc_device");
  return RSPARSE_HIP_OK;
}

int rsparse_hip_values_to_float_device(int64_t n, const double* d_src, float* d_dst, void* stream) {
  if (n < 0) return fail(RSPARSE_HIP_ERR_INVALID, "negative length");
  if (n > 0 && (!d_src || !d_dst)) return fail(RSPARSE_HIP_ERR_INVALID, "NULL array");
  if (n == 0) return RSPARSE_HIP_OK;
  hipError_t e = launch_f64_to_f32(d_src, d_dst, (size_t)n, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "launch_f64_to_f32");
  return RSPARSE_HIP_OK;
}

int rsparse_hip_csc_destroy(rsparse_hip_csc* m) {
  if (!m) return RSPARSE_HIP_OK;
  for (void* p : m->owned) (void)hipFree(p);
  if (m->d.vstats) (void)hipFree(m->d.vstats);
  delete m;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_csc_freeze_values(rsparse_hip_csc* m, int frozen) {
  if (!m) return fail(RSPARSE_HIP_ERR_INVALID, "NULL handle");
  m->d.vals_frozen = frozen != 0;
  m->d.vstats_valid = false;   // (a fresh promise starts from a fresh scan)
  return RSPARSE_HIP_OK;
}

int rsparse_hip_csc_info(const rsparse_hip_csc* m, int64_t info_out[40]) {
  if (!m || !info_out) return fail(RSPARSE_HIP_ERR_INVALID, "NULL argument");
  for (int b = 0; b < 40; b++) info_out[b] = 0;
  for (int b = 0; b < 6; b++) {
    info_out[8 + b] = m->d.q_off[b + 1] - m->d.q_off[b];
    info_out[14 + b] = m->d.q_nnz[b];
  }
  info_out[20] = m->d.q_cfg;
  info_out[21] = m->d.q_ne.nseg;
  for (int b = 0; b < 6; b++) {
    info_out[22 + b] = cgq_bucket_wpr(m->d.q_cfg, b);
    info_out[28 + b] = cgq_bucket_capq(m->d.q_cfg, b);
    info_out[34 + b] = cgq_bucket_waves(m->d.q_cfg, b) * (cgq_bucket_stream(m->d.q_cfg, b) ? -1 : 1);
  }
  info_out[0] = m->d.n_rows; info_out[1] = m->d.n_cols; info_out[2] = m->d.nnz;
  info_out[3] = m->d.n_long; info_out[4] = m->d.max_len; info_out[5] = m->d.nnz_long;
  info_out[6] = m->d.n_empty; info_out[7] = m->d.short_max;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_set_launch_mode(int mode) {
  if (mode < 0 || mode > 2) return fail(RSPARSE_HIP_ERR_INVALID, "launch mode must be 0, 1 or 2");
  cgq_set_launch_mode(mode);
  return RSPARSE_HIP_OK;
}

int rsparse_hip_profile_enable(int on) {
  g_prof.on = on != 0;
  g_prof.have = false;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_profile_last_names(char* buf, int cap) {
  if (!buf || cap <= 0) return fail(RSPARSE_HIP_ERR_INVALID, "buf is NULL or empty");
  buf[0] = 0;
  if (!g_prof.on || !g_prof.have) return fail(RSPARSE_HIP_ERR_INVALID, "no profiled call to report");
  std::string out;
  for (int i = 0; i < g_prof.nseg; i++) {
    if (i) out += '\n';
    if (!g_prof.kern[i]) continue;
    const char* mangled = hipKernelNameRefByPtr(g_prof.kern[i], nullptr);
    if (!mangled) continue;
    int st = 0;
    char* dem = abi::__cxa_demangle(mangled, nullptr, nullptr, &st);
    if (st != 0 || !dem) {   // this libstdc++ does not know _Float16 ("DF16_"): demangle it as half ("Dh")
      std::string alt(mangled);
      for (size_t p2; (p2 = alt.find("DF16_")) != std::string::npos;) alt.replace(p2, 5, "Dh");
      std::free(dem);
      dem = abi::__cxa_demangle(alt.c_str(), nullptr, nullptr, &st);
    }
    out += (st == 0 && dem) ? dem : mangled;
    std::free(dem);
  }
  if ((int)out.size() + 1 > cap) return fail(RSPARSE_HIP_ERR_INVALID, "buffer too small for the kernel names");
  std::memcpy(buf, out.c_str(), out.size() + 1);
  return RSPARSE_HIP_OK;
}

int rsparse_hip_profile_last(double ms_out[8]) {
  if (!ms_out) return fail(RSPARSE_HIP_ERR_INVALID, "ms_out is NULL");
  for (int i = 0; i < 8; i++) ms_out[i] = 0.0;
  if (!g_prof.on || !g_prof.have) return fail(RSPARSE_HIP_ERR_INVALID, "no profiled call to report");
  HIP_TRY(hipEventSynchronize(g_prof.ev[g_prof.nseg]));
  for (int i = 0; i < g_prof.nseg; i++) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, g_prof.ev[i], g_prof.ev[i + 1]));
    ms_out[i] = ms;
  }
  return RSPARSE_HIP_OK;
}

int rsparse_hip_gramian_device(const float* d_X, int rank, int64_t n, double lambda, float* d_XtX_out,
                               double* d_sumsq_out, void* stream) {
  return rsparse_hip_gramian_absmax_device(d_X, rank, n, lambda, d_XtX_out, d_sumsq_out, nullptr, stream);
}

int rsparse_hip_gramian_absmax_device(const float* d_X, int rank, int64_t n, double lambda, float* d_XtX_out,
                                      double* d_sumsq_out, float* d_absmax_inout, void* stream) {
  if ((!d_X && n != 0) || !d_XtX_out) return fail(RSPARSE_HIP_ERR_INVALID, "X or XtX_out is NULL");   // (n = 0: X is never read)
  if (rank <= 0 || n < 0) return fail(RSPARSE_HIP_ERR_INVALID, "rank must be positive and n non-negative");
  if (rank > RSPARSE_HIP_MAX_RANK) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "rank > 256 is not on the device path");
  int rc = g_ws.ensure_device();
  if (rc) return rc;
  if (wide_supported(rank)) {   // ranks 129..256 (d_absmax_inout is left as it is: only the rank <= 128 long-row kernel reads it)
    HIP_TRY(g_ws.gram.ensure(wide_gramian_scratch_floats(rank)));
    hipError_t we = launch_gramian_wide(d_X, rank, n, (float)lambda, d_XtX_out, d_sumsq_out, g_ws.gram, (hipStream_t)stream);
    if (we != hipSuccess) return hip_fail(we, "launch_gramian_wide");
    return RSPARSE_HIP_OK;
  }
  HIP_TRY(g_ws.gram.ensure(gramian_scratch_floats(rank, n)));
  const float ridge = (float)lambda;  // float::fl(diag(lambda)), R/model_WRMF.R:476
  hipEvent_t* ev = g_prof.begin();
  hipError_t e = launch_gramian(d_X, rank, n, ridge, d_XtX_out, d_sumsq_out, g_ws.gram, (hipStream_t)stream, ev,
                                reinterpret_cast<unsigned*>(d_absmax_inout));
  if (e != hipSuccess) return hip_fail(e, "launch_gramian");
  if (ev) {
    g_prof.have = true;
    g_prof.nseg = 2;
  }
  return RSPARSE_HIP_OK;
}

int rsparse_hip_gramian_float(const float* X, int rank, int64_t n, double lambda, float* XtX_out) {
  return gramian_host(X, rank, n, XtX_out, [&](const float* dX, float* dG) {
    return rsparse_hip_gramian_device(dX, rank, n, lambda, dG, nullptr, nullptr);
  });
}

int rsparse_hip_als_implicit_device(const rsparse_hip_csc* conf, const float* d_X, float* d_Y, const float* d_XtX,
                                    int rank, double lambda, unsigned solver, unsigned cg_steps,
                                    const float* d_absmax, double* d_loss_rows_out, void* stream) {
  return run_half_iteration(conf, true, d_X, d_Y, d_XtX, rank, lambda, solver, cg_steps, 0, d_loss_rows_out,
                            (hipStream_t)stream, nullptr, d_absmax);
}

int rsparse_hip_als_explicit_device(const rsparse_hip_csc* conf, const float* d_X, float* d_Y, int rank,
                                    double lambda, unsigned solver, unsigned cg_steps, int dynamic_lambda,
                                    double* d_loss_rows_out, void* stream) {
  return run_half_iteration(conf, false, d_X, d_Y, nullptr, rank, lambda, solver, cg_steps, dynamic_lambda,
                            d_loss_rows_out, (hipStream_t)stream);
}

int rsparse_hip_als_implicit_bias_device(const rsparse_hip_csc* conf, const float* d_X, float* d_Y, const float* d_XtX,
                                         int rank, double lambda, unsigned solver, int is_x_bias_last_row,
                                         double* d_loss_rows_out, void* stream) {
  int rc = check_variant(solver, 1, 0.0, true);
  if (rc) return rc;
  return run_half_iteration_implicit_biased(conf, d_X, d_Y, d_XtX, rank, lambda, solver, is_x_bias_last_row,
                                            d_loss_rows_out, (hipStream_t)stream);
}

int rsparse_hip_als_implicit_global_bias_device(const rsparse_hip_csc* conf, const float* d_X, float* d_Y,
                                                const float* d_XtX, int rank, double lambda, unsigned solver,
                                                unsigned cg_steps, int with_biases, int is_x_bias_last_row,
                                                double global_bias, int double_threshold, const float* d_absmax,
                                                double* d_loss_rows_out, void* stream) {
  int rc = check_variant(solver, with_biases, global_bias, true);
  if (rc) return rc;
  if (with_biases)
    return run_half_iteration_implicit_biased(conf, d_X, d_Y, d_XtX, rank, lambda, solver, is_x_bias_last_row,
                                              d_loss_rows_out, (hipStream_t)stream, global_bias, double_threshold != 0);
  if (!has_global_bias(global_bias, double_threshold != 0))
    return run_half_iteration(conf, true, d_X, d_Y, d_XtX, rank, lambda, solver, cg_steps, 0, d_loss_rows_out,
                              (hipStream_t)stream, nullptr, d_absmax);
  return run_half_iteration_implicit_global(conf, d_X, d_Y, d_XtX, rank, lambda, solver, cg_steps, global_bias, nullptr,
                                            nullptr, d_loss_rows_out, (hipStream_t)stream, d_absmax);
}

int rsparse_hip_initialize_biases_implicit_device(const rsparse_hip_csc* c_ui, const rsparse_hip_csc* c_iu,
                                                  float* d_user_bias, float* d_item_bias, double lambda,
                                                  int non_negative, int calculate_global_bias,
                                                  double* global_bias_out, void* stream) {
  if (!c_ui || !c_iu || !d_user_bias || !d_item_bias) return fail(RSPARSE_HIP_ERR_INVALID, "NULL matrix or bias vector");
  const CscView<float> a(c_ui->d), b(c_iu->d);   // users x items (columns = items), items x users (columns = users)
  if (a.n_rows != b.n_cols || a.n_cols != b.n_rows || a.nnz != b.nnz)
    return fail(RSPARSE_HIP_ERR_INVALID, "the two matrices are not transposes of each other");
  SumScratch w;
  if (int rc = sum_scratch(w)) return rc;
  return initialize_biases_implicit(a, b, d_user_bias, d_item_bias, lambda, non_negative, calculate_global_bias, w,
                                    (hipStream_t)stream, global_bias_out);
}

// ---- single sweeps of the bias initialisation over ONE column block (sharded drivers; see the header) ----
int rsparse_hip_bias_sweep_explicit_device(const rsparse_hip_csc* conf, const float* d_other_bias, double lambda,
                                           int dynamic_lambda, int non_negative, float* d_out, void* stream) {
  if (!conf || !d_other_bias || !d_out) return fail(RSPARSE_HIP_ERR_INVALID, "NULL matrix or bias vector");
  // (float)lambda: the reference's T lambda of the float instantiation
  return bias_sweep_explicit(CscView<float>(conf->d), d_other_bias, (float)lambda, dynamic_lambda, non_negative, d_out,
                             (hipStream_t)stream);
}

int rsparse_hip_bias_prep_implicit_device(const rsparse_hip_csc* conf, int n_other, double lambda, double* d_means,
                                          double* d_adj, void* stream) {
  if (!conf || !d_means || !d_adj) return fail(RSPARSE_HIP_ERR_INVALID, "NULL matrix or output");
  return bias_prep_implicit(CscView<float>(conf->d), n_other, lambda, d_means, d_adj, (hipStream_t)stream);
}

int rsparse_hip_bias_sweep_implicit_device(const rsparse_hip_csc* conf, const float* d_other_bias, int n_other,
                                           const double* d_other_sum, const double* d_means, const double* d_adj,
                                           int non_negative, double global_bias, float* d_out, void* stream) {
  if (!conf || !d_other_bias || !d_means || !d_adj || !d_out) return fail(RSPARSE_HIP_ERR_INVALID, "NULL matrix or vector");
  return bias_sweep_implicit(CscView<float>(conf->d), d_other_bias, n_other, d_other_sum, d_means, d_adj, non_negative,
                             global_bias, d_out, (hipStream_t)stream);
}

int rsparse_hip_als_explicit_bias_device(const rsparse_hip_csc* conf, const float* d_X, float* d_Y, int rank,
                                         double lambda, unsigned solver, unsigned cg_steps, int dynamic_lambda,
                                         int is_x_bias_last_row, double* d_loss_rows_out, void* stream) {
  int rc = check_variant(solver, 1, 0.0, false);
  if (rc) return rc;
  return run_half_iteration_explicit_biased(conf, d_X, d_Y, rank, lambda, solver, cg_steps, dynamic_lambda,
                                            is_x_bias_last_row, d_loss_rows_out, (hipStream_t)stream);
}

int rsparse_hip_initialize_biases_explicit_device(rsparse_hip_csc* c_ui, rsparse_hip_csc* c_iu, float* d_user_bias,
                                                  float* d_item_bias, double lambda, int dynamic_lambda,
                                                  int non_negative, int calculate_global_bias,
                                                  double* global_bias_out, void* stream) {
  if (!c_ui || !c_iu || !d_user_bias || !d_item_bias) return fail(RSPARSE_HIP_ERR_INVALID, "NULL matrix or bias vector");
  const CscView<float> a(c_ui->d), b(c_iu->d);   // users x items (columns = items), items x users (columns = users)
  if (a.n_rows != b.n_cols || a.n_cols != b.n_rows || a.nnz != b.nnz)
    return fail(RSPARSE_HIP_ERR_INVALID, "the two matrices are not transposes of each other");
  SumScratch w;
  if (int rc = sum_scratch(w)) return rc;
  // a frozen handle promises unchanged values (the fp64 handle has no such flag)
  if (calculate_global_bias && a.nnz > 0 && (c_ui->d.vals_frozen || c_iu->d.vals_frozen))
    return fail(RSPARSE_HIP_ERR_INVALID, "the values of a frozen handle cannot lose their mean (rsparse_hip_csc_freeze_values)");
  // (float)lambda: the reference's T lambda of the float instantiation
  return initialize_biases_explicit(a, b, d_user_bias, d_item_bias, (float)lambda, dynamic_lambda, non_negative,
                                    calculate_global_bias, w, (hipStream_t)stream, global_bias_out);
}

int rsparse_hip_values_subtract_mean_device(int64_t n, float* d_x, float* d_x_other, double* mean_out, void* stream) {
  if (n < 0) return fail(RSPARSE_HIP_ERR_INVALID, "negative length");
  if (mean_out) *mean_out = 0.0;
  if (n == 0) return RSPARSE_HIP_OK;
  if (!d_x) return fail(RSPARSE_HIP_ERR_INVALID, "values is NULL");
  SumScratch w;
  if (int rc = sum_scratch(w)) return rc;
  double mean = 0.0;
  if (int rc = subtract_mean(d_x, d_x_other, n, w, (hipStream_t)stream, &mean)) return rc;
  if (mean_out) *mean_out = mean;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_weighted_sumsq_device(const float* d_X, int rank, int64_t n, const float* d_w, double* d_out,
                                      void* stream) {
  if (!d_X || !d_out) return fail(RSPARSE_HIP_ERR_INVALID, "X or out is NULL");
  if (rank <= 0 || n < 0) return fail(RSPARSE_HIP_ERR_INVALID, "rank must be positive and n non-negative");
  SumScratch w;
  if (int rc = sum_scratch(w)) return rc;
  return weighted_sumsq(d_X, rank, n, d_w, d_out, w, (hipStream_t)stream);
}

int rsparse_hip_top_product_device(const float* d_U, const float* d_V, int n_users, int n_items, int rank, int k,
                                   const int32_t* d_nr_p, const int32_t* d_nr_j, const int32_t* d_excl0,
                                   int n_exclude, double glob_mean, int32_t* d_res, float* d_scores, void* stream) {
  if (!d_U || !d_V || !d_res || !d_scores) return fail(RSPARSE_HIP_ERR_INVALID, "NULL matrix or output");
  if (n_users < 0 || n_items < 0 || rank <= 0 || k < 1) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions");
  if (rank > RSPARSE_HIP_MAX_RANK) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "rank > 256 is not on the device path");
  if (int rc = refuse_large_k(k)) return rc;
  if (n_exclude > 0 && !d_excl0) return fail(RSPARSE_HIP_ERR_INVALID, "exclude is NULL");
  if (k > RSPARSE_HIP_MAX_TOPK) {   // the large-k path (wrmf_topk_large.hip): its key matrix and lists in the grow-only workspace
    if (n_users == 0) return RSPARSE_HIP_OK;
    HIP_TRY(g_ws.pad_buf.ensure(top_product_large_ws_floats(n_users, n_items, k, k)));
    hipError_t e = launch_top_product_large(d_U, d_V, n_users, n_items, rank, k, d_nr_p, d_nr_p ? d_nr_j : nullptr, d_excl0, n_exclude,
                                            (float)glob_mean, d_res, d_scores, (hipStream_t)stream, g_ws.pad_buf);
    if (e != hipSuccess) return hip_fail(e, "launch_top_product_large");
    return RSPARSE_HIP_OK;
  }
  // (few users over many items: the items are split over the workgroups, the slices' lists land in this scratch)
  float* scratch = nullptr;
  const size_t sfl = top_product_plan(n_users, n_items, rank, k, k, false).scratch_floats;
  if (sfl > 0) {
    HIP_TRY(g_ws.pad_buf.ensure(sfl));
    scratch = g_ws.pad_buf;
  }
  hipError_t e = launch_top_product(d_U, d_V, n_users, n_items, rank, k, d_nr_p, d_nr_p ? d_nr_j : nullptr, d_excl0,
                                    n_exclude, (float)glob_mean, d_res, d_scores, (hipStream_t)stream, scratch);
  if (e != hipSuccess) return hip_fail(e, "launch_top_product");
  return RSPARSE_HIP_OK;
}

namespace {
// candidates per user: k + extra (default: a quarter of k, at least 8), never more than the kernel's 256 or the items
int top_product_kc(int k, int extra, int n_items) {
  if (extra < 0) extra = std::max(8, k / 4);
  return std::max(k, std::min(std::min(k + extra, RSPARSE_HIP_MAX_TOPK), std::max(n_items, 1)));
}
}  // namespace

int rsparse_hip_top_product_plan(int n_users, int n_items, int rank, int k, int extra, int rescore, char* text, int text_len) {
  if (!text || text_len < 1) return fail(RSPARSE_HIP_ERR_INVALID, "no text buffer");
  if (n_users < 0 || n_items < 0 || rank <= 0 || k < 1) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions");
  if (rank > RSPARSE_HIP_MAX_RANK || k > RSPARSE_HIP_MAX_TOPK)
    return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "the plan describes the kernels for rank <= 256 and k <= 256");
  const TopPlan plan = top_product_plan(n_users, n_items, rank, rescore ? top_product_kc(k, extra, n_items) : k, k, rescore != 0);
  static const char* const family[] = {"per_wave", "shared", "pipe"};
  std::string out;
  char line[256];
  for (const TopLaunch& l : plan.launches) {
    snprintf(line, sizeof line, "family=%s KP=%d UB=%d W=%d buffers=%s users=%d threads=%d lds=%zu k=%d user0=%d n_users=%d grid=%dx%d "
             "slice_items=%d flagged=%d scratch_floats=%zu\n", family[l.geo.family], l.geo.KP, l.geo.UB, l.geo.W,
             l.geo.gbuf ? "global" : "lds", l.geo.users, l.geo.threads, l.geo.lds, l.topk, l.user0, l.n_users, l.grid_x, l.n_slices,
             l.slice_items, (int)l.flagged, plan.scratch_floats);
    out += line;
  }
  if (out.size() + 1 > (size_t)text_len) return fail(RSPARSE_HIP_ERR_INVALID, "the text buffer is too small for the plan");
  memcpy(text, out.c_str(), out.size() + 1);
  return RSPARSE_HIP_OK;
}

int rsparse_hip_top_product_f64_device(const float* d_U, const float* d_V, const double* d_U64, const double* d_V64,
                                       int n_users, int n_items, int rank, int k, int extra, const int32_t* d_nr_p,
                                       const int32_t* d_nr_j, const int32_t* d_excl0, int n_exclude, double glob_mean,
                                       int32_t* d_res, double* d_scores, void* stream) {
  if (!d_U || !d_V || !d_res || !d_scores) return fail(RSPARSE_HIP_ERR_INVALID, "NULL matrix or output");
  if ((d_U64 == nullptr) != (d_V64 == nullptr)) return fail(RSPARSE_HIP_ERR_INVALID, "the double factors come as a pair");
  if (n_users < 0 || n_items < 0 || rank <= 0 || k < 1) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions");
  if (rank > RSPARSE_HIP_MAX_RANK) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "rank > 256 is not on the device path");
  if (int rc = refuse_large_k(k)) return rc;
  if (n_users == 0) return RSPARSE_HIP_OK;
  if (k > RSPARSE_HIP_MAX_TOPK) {   // the large-k path: kc = k + extra candidates (at most 10240), re-scored in double
    if (n_exclude > 0 && !d_excl0) return fail(RSPARSE_HIP_ERR_INVALID, "exclude is NULL");
    const int kcl = top_product_large_kc(k, extra, n_items);
    HIP_TRY(g_ws.pad_buf.ensure(top_product_large_ws_floats(n_users, n_items, k, kcl)));
    hipError_t e = launch_top_product_large_f64(d_U, d_V, d_U64, d_V64, n_users, n_items, rank, k, kcl, d_nr_p, d_nr_p ? d_nr_j : nullptr,
                                                d_excl0, n_exclude, glob_mean, d_res, d_scores, (hipStream_t)stream, g_ws.pad_buf);
    if (e != hipSuccess) return hip_fail(e, "launch_top_product_large_f64");
    return RSPARSE_HIP_OK;
  }
  const int kc = top_product_kc(k, extra, n_items);
  HIP_TRY(g_ws.bias_buf.ensure(top_product_f64_scratch_words(n_users, kc, k)));   // (nothing else uses this buffer meanwhile)
  float* split = nullptr;   // few users over many items: the nominating pass splits the items over the workgroups
  const size_t sfl = top_product_plan(n_users, n_items, rank, kc, k, true).scratch_floats;   // (or the candidate buffers of a large k)
  if (sfl > 0) {
    HIP_TRY(g_ws.pad_buf.ensure(sfl));
    split = g_ws.pad_buf;
  }
  hipError_t e = launch_top_product_f64(d_U, d_V, d_U64, d_V64, n_users, n_items, rank, k, kc, d_nr_p, d_nr_p ? d_nr_j : nullptr,
                                        d_excl0, n_exclude, glob_mean, d_res, d_scores, (hipStream_t)stream, g_ws.bias_buf, split);
  if (e != hipSuccess) return hip_fail(e, "launch_top_product_f64");
  return RSPARSE_HIP_OK;
}

namespace {
// rows of queries per call of the top-k path: what HipBackend.top_product uses (the same re-scoring budget above k = 256)
int similar_items_batch(int k) {
  int64_t B = 1 << 18;
  if (k > RSPARSE_HIP_MAX_TOPK) {
    const int64_t kc = k + std::max(8, k / 4);
    B = std::max<int64_t>(1, std::min<int64_t>(B, B * (2 * 320 + 2 * 256 + 1) / (2 * kc + 2 * (int64_t)k + 1)));
  }
  return (int)B;
}
}  // namespace

int rsparse_hip_normalize_items_device(const float* d_V, int n_items, int ld, int c0, int c1, float* d_Vn32, double* d_Vn64,
                                       int32_t* d_flags, void* stream) {
  int rc = normalize_items_args(d_V, n_items, ld, c0, c1, d_Vn32, d_Vn64, d_flags);
  if (rc || n_items == 0) return rc;
  hipError_t e = launch_normalize_items(d_V, false, n_items, ld, c0, c1 - c0, d_Vn32, d_Vn64, d_flags, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "launch_normalize_items");
  return RSPARSE_HIP_OK;
}

int rsparse_hip_similar_items_device(const float* d_Vn32, const double* d_Vn64, int n_items, int r, const int32_t* d_query,
                                     int n_q, int k, int exclude_self, const int32_t* d_exclude0, int n_exclude,
                                     int32_t* d_res, double* d_scores, void* stream) {
  int rc = similar_items_args(n_items, r, n_q, k, n_exclude, d_exclude0);
  if (rc) return rc;
  if (n_q > 0 && (!d_query || !d_res || !d_scores)) return fail(RSPARSE_HIP_ERR_INVALID, "NULL query or output");
  if (n_items > 0 && (!d_Vn32 || !d_Vn64)) return fail(RSPARSE_HIP_ERR_INVALID, "NULL normalised factors");
  if (n_q == 0) return RSPARSE_HIP_OK;
  if ((rc = g_ws.ensure_device())) return rc;
  const int B = similar_items_batch(k);
  HIP_TRY(g_ws.sim_buf.ensure(similar_query_ws_bytes(std::min(n_q, B), r)));
  hipStream_t s = (hipStream_t)stream;
  for (int a0 = 0; a0 < n_q; a0 += B) {   // (batches reuse the workspace: they are ordered on the stream)
    const int nb = std::min(B, n_q - a0);
    const SimilarQueryWs w = similar_query_ws(g_ws.sim_buf, nb, r);
    hipError_t e = launch_gather_queries(d_Vn32, d_Vn64, n_items, r, d_query + a0, nb, w, s);
    if (e != hipSuccess) return hip_fail(e, "launch_gather_queries");
    int32_t* res = d_res + (size_t)a0 * k;
    double* sc = d_scores + (size_t)a0 * k;
    rc = rsparse_hip_top_product_f64_device(w.Q32, d_Vn32, w.Q64, d_Vn64, nb, n_items, r, k, -1, exclude_self ? w.nr_p : nullptr,
                                            exclude_self ? w.nr_j : nullptr, d_exclude0, n_exclude, 0.0, res, sc, stream);
    if (rc) return rc;
    if ((e = launch_mask_queries(w.bad, nb, k, res, sc, s)) != hipSuccess) return hip_fail(e, "launch_mask_queries");
  }
  return RSPARSE_HIP_OK;
}

int rsparse_hip_ranking_metrics_device(const int32_t* d_pred, int n_users, int k, const int32_t* d_p, const int32_t* d_j,
                                       const double* d_x, double* d_ap_out, double* d_ndcg_out, void* stream) {
  int rc = ranking_metrics_args(d_pred, n_users, k, d_p, d_j, d_x, d_ap_out, d_ndcg_out);
  if (rc || n_users == 0) return rc;
  if ((rc = g_ws.ensure_device())) return rc;
  HIP_TRY(g_ws.met_buf.ensure((size_t)n_users + 1));
  hipError_t e = launch_ranking_metrics(d_pred, n_users, k, d_p, d_j, d_ndcg_out ? d_x : nullptr, d_ap_out, d_ndcg_out,
                                        g_ws.met_buf, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "launch_ranking_metrics");
  return RSPARSE_HIP_OK;
}

int rsparse_hip_hit_metrics_device(const int32_t* d_pred, int n_users, int k, const int32_t* d_p, const int32_t* d_j,
                                   const int32_t* cutoffs, int n_cutoffs, int32_t* d_hits, int32_t* d_first, double* d_precision,
                                   double* d_recall, double* d_hit, double* d_mrr, int32_t* d_first_seen, int n_items,
                                   void* stream) {
  const bool any = d_hits || d_first || d_precision || d_recall || d_hit || d_mrr || d_first_seen;
  int rc = hit_metrics_args(d_pred, n_users, k, d_p, d_j, cutoffs, n_cutoffs, any, d_first_seen, n_items);
  if (rc || n_users == 0) return rc;
  if ((rc = g_ws.ensure_device())) return rc;
  hipError_t e = launch_hit_metrics(d_pred, n_users, k, d_p, d_j, cutoffs, n_cutoffs, d_hits, d_first, d_precision, d_recall, d_hit,
                                    d_mrr, d_first_seen, n_items, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "launch_hit_metrics");
  return RSPARSE_HIP_OK;
}

namespace {
int item_inv_norms_device(const void* d_V, bool f64, int n_items, int ld, int c0, int c1, double* d_inv, void* stream) {
  int rc = window_args(n_items, ld, c0, c1);
  if (rc) return rc;
  if (n_items > 0 && (!d_V || !d_inv)) return fail(RSPARSE_HIP_ERR_INVALID, "NULL matrix or output");
  if (n_items == 0) return RSPARSE_HIP_OK;
  if ((rc = g_ws.ensure_device())) return rc;
  hipError_t e = launch_item_inv_norms(d_V, f64, n_items, ld, c0, c1 - c0, d_inv, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "launch_item_inv_norms");
  return RSPARSE_HIP_OK;
}

int list_diversity_device(const int32_t* d_pred, int n_users, int k, const int32_t* cutoffs, int n_cutoffs, const void* d_V, bool f64,
                          int n_items, int ld, int c0, int c1, const double* d_inv, int32_t* d_counted, double* d_diversity,
                          void* stream) {
  int rc = list_diversity_args(d_pred, n_users, k, cutoffs, n_cutoffs, d_V, n_items, ld, c0, c1, d_counted, d_diversity);
  if (rc) return rc;
  if (!d_inv) return fail(RSPARSE_HIP_ERR_INVALID, "the inverse norms are NULL");
  if (n_users == 0) return RSPARSE_HIP_OK;
  if ((rc = g_ws.ensure_device())) return rc;
  hipError_t e = launch_list_diversity(d_pred, n_users, k, cutoffs, n_cutoffs, d_V, f64, n_items, ld, c0, c1 - c0, d_inv, d_counted,
                                       d_diversity, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "launch_list_diversity");
  return RSPARSE_HIP_OK;
}
}  // namespace

int rsparse_hip_list_metrics_device(const int32_t* d_pred, int n_users, int k, const int32_t* cutoffs, int n_cutoffs,
                                    const int32_t* d_item_count, const int64_t* d_item_info, int n_items, int32_t* d_valid,
                                    int64_t* d_count_sum, int64_t* d_info_sum, double* d_popularity, double* d_novelty,
                                    int32_t* d_exposure, void* stream) {
  int rc = list_metrics_args(d_pred, n_users, k, cutoffs, n_cutoffs, d_item_count, d_item_info, n_items, d_valid, d_count_sum,
                             d_info_sum, d_popularity, d_novelty, d_exposure);
  if (rc || n_users == 0) return rc;
  if ((rc = g_ws.ensure_device())) return rc;
  // (a table that no output needs is not gathered)
  hipError_t e = launch_list_metrics(d_pred, n_users, k, cutoffs, n_cutoffs, (d_count_sum || d_popularity) ? d_item_count : nullptr,
                                     (d_info_sum || d_novelty) ? d_item_info : nullptr, n_items, d_valid, d_count_sum, d_info_sum,
                                     d_popularity, d_novelty, d_exposure, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "launch_list_metrics");
  return RSPARSE_HIP_OK;
}

int rsparse_hip_item_inv_norms_device(const float* d_V, int n_items, int ld, int c0, int c1, double* d_inv, void* stream) {
  return item_inv_norms_device(d_V, false, n_items, ld, c0, c1, d_inv, stream);
}
int rsparse_hip_item_inv_norms_f64_device(const double* d_V, int n_items, int ld, int c0, int c1, double* d_inv, void* stream) {
  return item_inv_norms_device(d_V, true, n_items, ld, c0, c1, d_inv, stream);
}

int rsparse_hip_list_diversity_device(const int32_t* d_pred, int n_users, int k, const int32_t* cutoffs, int n_cutoffs,
                                      const float* d_V, int n_items, int ld, int c0, int c1, const double* d_inv,
                                      int32_t* d_counted, double* d_diversity, void* stream) {
  return list_diversity_device(d_pred, n_users, k, cutoffs, n_cutoffs, d_V, false, n_items, ld, c0, c1, d_inv, d_counted, d_diversity,
                               stream);
}
int rsparse_hip_list_diversity_f64_device(const int32_t* d_pred, int n_users, int k, const int32_t* cutoffs, int n_cutoffs,
                                          const double* d_V, int n_items, int ld, int c0, int c1, const double* d_inv,
                                          int32_t* d_counted, double* d_diversity, void* stream) {
  return list_diversity_device(d_pred, n_users, k, cutoffs, n_cutoffs, d_V, true, n_items, ld, c0, c1, d_inv, d_counted, d_diversity,
                               stream);
}

namespace {
int mmr_rerank_device(const int32_t* d_lists, const double* d_scores, int n_users, int n_pool, int k, double trade_off, const void* d_V,
                      bool f64, int n_items, int ld, int c0, int c1, const double* d_inv, int32_t* d_items, double* d_picked,
                      int32_t* d_positions, double* d_objective, void* stream) {
  int rc = mmr_rerank_args(d_lists, d_scores, n_users, n_pool, k, trade_off, d_V, n_items, ld, c0, c1, d_items);
  if (rc) return rc;
  if (!d_inv) return fail(RSPARSE_HIP_ERR_INVALID, "the inverse norms are NULL");
  if (n_users == 0) return RSPARSE_HIP_OK;
  if ((rc = g_ws.ensure_device())) return rc;
  hipError_t e = launch_mmr_rerank(d_lists, d_scores, n_users, n_pool, k, trade_off, d_V, f64, n_items, ld, c0, c1 - c0, d_inv, d_items,
                                   d_picked, d_positions, d_objective, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "launch_mmr_rerank");
  return RSPARSE_HIP_OK;
}
}  // namespace

int rsparse_hip_mmr_rerank_device(const int32_t* d_lists, const double* d_scores, int n_users, int n_pool, int k, double trade_off,
                                  const float* d_V, int n_items, int ld, int c0, int c1, const double* d_inv, int32_t* d_items,
                                  double* d_scores_out, int32_t* d_positions, double* d_objective, void* stream) {
  return mmr_rerank_device(d_lists, d_scores, n_users, n_pool, k, trade_off, d_V, false, n_items, ld, c0, c1, d_inv, d_items,
                           d_scores_out, d_positions, d_objective, stream);
}
int rsparse_hip_mmr_rerank_f64_device(const int32_t* d_lists, const double* d_scores, int n_users, int n_pool, int k,
                                      double trade_off, const double* d_V, int n_items, int ld, int c0, int c1, const double* d_inv,
                                      int32_t* d_items, double* d_scores_out, int32_t* d_positions, double* d_objective,
                                      void* stream) {
  return mmr_rerank_device(d_lists, d_scores, n_users, n_pool, k, trade_off, d_V, true, n_items, ld, c0, c1, d_inv, d_items,
                           d_scores_out, d_positions, d_objective, stream);
}

namespace {
int rank_summary_args(int n_users, const void* act_p, const void* act_x, const void* above, const void* tied, const void* n_adm,
                      const void* mpr, const void* auc, const void* mrr, const void* sums) {
  if (!mpr && !auc && !mrr && !sums) return fail(RSPARSE_HIP_ERR_INVALID, "mpr, auc, mrr and sums are all NULL");
  if (n_users < 0) return fail(RSPARSE_HIP_ERR_INVALID, "n_users < 0");
  if (!act_p || !above || !tied || !n_adm) return fail(RSPARSE_HIP_ERR_INVALID, "actual_p, above, tied or n_adm is NULL");
  if ((mpr || sums) && !act_x) return fail(RSPARSE_HIP_ERR_INVALID, "mpr and sums need the weights: actual_x is NULL");
  return RSPARSE_HIP_OK;
}
}  // namespace

int rsparse_hip_held_out_ranks_device(const float* d_U, const float* d_V, int n_users, int n_items, int rank, const int32_t* d_nr_p,
                                      const int32_t* d_nr_j, const int32_t* d_excl0, int n_exclude, const int32_t* d_act_p,
                                      const int32_t* d_act_j, int max_chunk_users, int32_t* d_above, int32_t* d_tied,
                                      int32_t* d_n_adm, void* stream) {
  int rc = held_out_ranks_args(d_U, d_V, n_users, n_items, rank, n_exclude, d_excl0, d_act_p, d_act_j, max_chunk_users);
  if (rc) return rc;
  if (!d_above || !d_tied || !d_n_adm) return fail(RSPARSE_HIP_ERR_INVALID, "above, tied or n_adm is NULL");
  if (n_users == 0) return RSPARSE_HIP_OK;
  if ((rc = g_ws.ensure_device())) return rc;
  // the key matrix of a chunk of users lives where the large-k path keeps its own (wrmf_topk_large.hip)
  HIP_TRY(g_ws.pad_buf.ensure(held_out_ranks_ws_floats(n_users, n_items, max_chunk_users)));
  hipError_t e = launch_held_out_ranks(d_U, d_V, n_users, n_items, rank, (d_nr_p && d_nr_j) ? d_nr_p : nullptr, d_nr_j, d_excl0,
                                       n_exclude, d_act_p, d_act_j, max_chunk_users, d_above, d_tied, d_n_adm, (hipStream_t)stream,
                                       g_ws.pad_buf);
  if (e != hipSuccess) return hip_fail(e, "launch_held_out_ranks");
  return RSPARSE_HIP_OK;
}

int rsparse_hip_rank_summary_device(int n_users, const int32_t* d_act_p, const double* d_act_x, const int32_t* d_above,
                                    const int32_t* d_tied, const int32_t* d_n_adm, double* d_mpr, double* d_auc, double* d_mrr,
                                    double* d_sums, void* stream) {
  int rc = rank_summary_args(n_users, d_act_p, d_act_x, d_above, d_tied, d_n_adm, d_mpr, d_auc, d_mrr, d_sums);
  if (rc || n_users == 0) return rc;
  hipError_t e = launch_rank_summary(n_users, d_act_p, (d_mpr || d_sums) ? d_act_x : nullptr, d_above, d_tied, d_n_adm, d_mpr, d_auc,
                                     d_mrr, d_sums, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "launch_rank_summary");
  return RSPARSE_HIP_OK;
}

// `_f64_device`: wrmf_f64_capi.cpp; the host form rsparse_hip_sparse_approximation: wrmf_capi_host.cpp
int rsparse_hip_score_pairs_device(const float* d_U, const float* d_V, int n_rows, int n_cols, int r, const int32_t* d_p,
                                   const int32_t* d_j, double add, const double* d_actual, double* d_scores, double* d_sse,
                                   double* d_sae, void* stream) {
  return score_pairs_device(d_U, d_V, n_rows, n_cols, r, d_p, d_j, add, d_actual, d_scores, d_sse, d_sae, (hipStream_t)stream,
                            [](size_t n, double*& buf) {
                              if (int rc = g_ws.ensure_device()) return rc;
                              HIP_TRY(g_ws.score_buf.ensure(n));
                              buf = g_ws.score_buf;
                              return (int)RSPARSE_HIP_OK;
                            });
}

// `_f64_device`: wrmf_f64_capi.cpp
int rsparse_hip_softals_half_device(const int32_t* d_p, const int32_t* d_j, const float* d_x, const float* d_M, const float* d_W,
                                    int n_rows, int n_cols, int r, const double* w, const double* s, const double* t,
                                    float* d_out, double* d_sumsq, void* stream) {
  return softals_half_device(d_p, d_j, d_x, d_M, d_W, n_rows, n_cols, r, w, s, t, d_out, d_sumsq, (hipStream_t)stream,
                             [](size_t n, double*& buf) {
                               if (int rc = g_ws.ensure_device()) return rc;
                               HIP_TRY(g_ws.softals_buf.ensure(n));
                               buf = g_ws.softals_buf;
                               return (int)RSPARSE_HIP_OK;
                             });
}

namespace {
// The dense rows of the ItemKNN entries: `rows` rows of row_bytes each, all zeros when the work enqueued so far is done.  A
// buffer that grew, or that a failed call left behind, is zeroed here; a call that ends well leaves zeros itself.
static int knn_workspace(int64_t total_rows, size_t row_bytes, int64_t ws_rows, int64_t& rows, void*& ws, hipStream_t s) {
  rows = ws_rows > 0 ? ws_rows : (int64_t)(RSPARSE_HIP_KNN_WS_BYTES / std::max<size_t>(row_bytes, 1));
  rows = std::max<int64_t>(1, std::min(rows, total_rows));
  const size_t bytes = std::max<size_t>((size_t)rows * row_bytes, 16);
  if (int rc = g_ws.ensure_device()) return rc;
  const bool grows = bytes > g_ws.knn_buf.cap;
  HIP_TRY(g_ws.knn_buf.ensure(bytes));
  if (grows || g_ws.knn_dirty) HIP_TRY(hipMemsetAsync(g_ws.knn_buf, 0, g_ws.knn_buf.cap, s));
  g_ws.knn_dirty = true;   // until the caller has enqueued its last zeroing
  ws = g_ws.knn_buf;
  return RSPARSE_HIP_OK;
}

// n + 1 row pointers of a device pattern on the host (waits for the stream): non-negative and non-decreasing, or a refusal
static int fetch_row_pointers(const int32_t* d_p, size_t n, std::vector<int32_t>& h, hipStream_t s, const char* name) {
  h.resize(n + 1);
  HIP_TRY(hipMemcpyAsync(h.data(), d_p, (n + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (size_t r = 0; r <= n; r++)
    if (h[r] < 0 || (r > 0 && h[r] < h[r - 1])) return fail(RSPARSE_HIP_ERR_INVALID, std::string(name) + " is negative or decreases");
  return RSPARSE_HIP_OK;
}
}  // namespace

// the host forms rsparse_hip_cooc_neighbors / rsparse_hip_knn_recommend and their `_weighted` forms: wrmf_capi_host.cpp
int rsparse_hip_cooc_neighbors_device(const int32_t* d_ip, const int32_t* d_iu, const int32_t* d_up, const int32_t* d_uj, int n_users,
                                      int n_items, int item0, int item1, int similarity, int K, int64_t ws_rows,
                                      int32_t* d_neighbors, int32_t* d_counts, void* stream) {
  int rc = cooc_neighbors_args(!d_ip || !d_iu || !d_up || !d_uj || !d_neighbors || !d_counts, n_users, n_items, item0, item1,
                               similarity, K, ws_rows);
  if (rc || item1 == item0) return rc;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> h_ip;
  if ((rc = fetch_row_pointers(d_ip + item0, (size_t)(item1 - item0), h_ip, s, "ip"))) return rc;
  int64_t rows = 0;
  void* ws = nullptr;
  if ((rc = knn_workspace(item1 - item0, (size_t)n_items * sizeof(uint32_t), ws_rows, rows, ws, s))) return rc;
  hipError_t e = launch_cooc_neighbors(d_ip, d_iu, d_up, d_uj, n_users, n_items, item0, item1, h_ip.data(), similarity, K, rows,
                                       static_cast<unsigned*>(ws), d_neighbors, d_counts, s);
  if (e != hipSuccess) return hip_fail(e, "launch_cooc_neighbors");
  g_ws.knn_dirty = false;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_cooc_neighbors_weighted_device(const int32_t* d_ip, const int32_t* d_iu, const uint32_t* d_il, const int32_t* d_up,
                                               const int32_t* d_uj, const uint32_t* d_ur, int n_users, int n_items, int item0,
                                               int item1, const double* d_a, const double* d_b, double h, int K, int64_t ws_rows,
                                               int32_t* d_neighbors, uint64_t* d_sums, void* stream) {
  int rc = cooc_neighbors_weighted_args(!d_ip || !d_iu || !d_il || !d_up || !d_uj || !d_ur || !d_a || !d_b || !d_neighbors || !d_sums,
                                        n_users, n_items, item0, item1, h, K, ws_rows);
  if (rc || item1 == item0) return rc;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> h_ip;
  if ((rc = fetch_row_pointers(d_ip + item0, (size_t)(item1 - item0), h_ip, s, "ip"))) return rc;
  int64_t rows = 0;
  void* ws = nullptr;
  if ((rc = knn_workspace(item1 - item0, (size_t)n_items * sizeof(uint64_t), ws_rows, rows, ws, s))) return rc;
  hipError_t e = launch_cooc_neighbors_weighted(d_ip, d_iu, d_il, d_up, d_uj, d_ur, n_users, n_items, item0, item1, h_ip.data(), d_a,
                                                d_b, h, K, rows, static_cast<unsigned long long*>(ws), d_neighbors,
                                                reinterpret_cast<unsigned long long*>(d_sums), s);
  if (e != hipSuccess) return hip_fail(e, "launch_cooc_neighbors_weighted");
  g_ws.knn_dirty = false;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_knn_recommend_weighted_device(const int32_t* d_xp, const int32_t* d_xj, const uint32_t* d_xv, int n_rows, int n_items,
                                              const int32_t* d_neighbors, const uint32_t* d_q, int K, const int32_t* d_nr_p,
                                              const int32_t* d_nr_j, const int32_t* d_excl0, int n_exclude, int k, int64_t ws_rows,
                                              int32_t* d_items, int64_t* d_scores, void* stream) {
  int rc = knn_recommend_args(!d_xp || !d_xj || !d_neighbors || !d_q || !d_items || !d_scores, n_rows, n_items, K, d_nr_p, d_nr_j,
                              d_excl0, n_exclude, k, ws_rows);
  if (rc || n_rows == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> h_xp;
  if ((rc = fetch_row_pointers(d_xp, (size_t)n_rows, h_xp, s, "x_p"))) return rc;
  int64_t rows = 0;
  void* ws = nullptr;
  if ((rc = knn_workspace(n_rows, (size_t)n_items * sizeof(uint64_t), ws_rows, rows, ws, s))) return rc;
  hipError_t e = launch_knn_recommend(d_xp, d_xj, d_xv, n_rows, n_items, h_xp.data(), d_neighbors, d_q, K, d_nr_p, d_nr_j,
                                      n_exclude > 0 ? d_excl0 : nullptr, n_exclude, k, rows, static_cast<unsigned long long*>(ws),
                                      d_items, reinterpret_cast<long long*>(d_scores), s);
  if (e != hipSuccess) return hip_fail(e, "launch_knn_recommend");
  g_ws.knn_dirty = false;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_knn_recommend_device(const int32_t* d_xp, const int32_t* d_xj, int n_rows, int n_items, const int32_t* d_neighbors,
                                     const uint32_t* d_q, int K, const int32_t* d_nr_p, const int32_t* d_nr_j,
                                     const int32_t* d_excl0, int n_exclude, int k, int64_t ws_rows, int32_t* d_items,
                                     int64_t* d_scores, void* stream) {
  return rsparse_hip_knn_recommend_weighted_device(d_xp, d_xj, nullptr, n_rows, n_items, d_neighbors, d_q, K, d_nr_p, d_nr_j, d_excl0,
                                                   n_exclude, k, ws_rows, d_items, d_scores, stream);
}

// EASE (wrmf_ease.hip) on the same workspace; the host forms rsparse_hip_item_gram / rsparse_hip_ease_recommend: wrmf_capi_host.cpp
int rsparse_hip_item_gram_device(const int32_t* d_ip, const int32_t* d_iu, const int32_t* d_up, const int32_t* d_uj, int n_users,
                                 int n_items, int item0, int item1, double lambda, double* d_out, size_t ld_out, int64_t ws_rows,
                                 void* stream) {
  int rc = item_gram_args(!d_ip || !d_iu || !d_up || !d_uj || !d_out, n_users, n_items, item0, item1, lambda, ld_out, ws_rows);
  if (rc || item1 == item0) return rc;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> h_ip;
  if ((rc = fetch_row_pointers(d_ip + item0, (size_t)(item1 - item0), h_ip, s, "ip"))) return rc;
  int64_t rows = 0;
  void* ws = nullptr;
  if ((rc = knn_workspace(item1 - item0, (size_t)n_items * sizeof(uint32_t), ws_rows, rows, ws, s))) return rc;
  hipError_t e = launch_ease_item_gram(d_ip, d_iu, d_up, d_uj, n_users, n_items, item0, item1, h_ip.data(), lambda, rows,
                                       static_cast<unsigned*>(ws), d_out, ld_out, s);
  if (e != hipSuccess) return hip_fail(e, "launch_ease_item_gram");
  g_ws.knn_dirty = false;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_ease_recommend_device(const int32_t* d_xp, const int32_t* d_xj, int n_rows, int n_items, const void* d_B, size_t ld_B,
                                      int b_is_double, const int32_t* d_nr_p, const int32_t* d_nr_j, const int32_t* d_excl0,
                                      int n_exclude, int k, int64_t ws_rows, int32_t* d_items, uint64_t* d_scores, void* stream) {
  int rc = ease_recommend_args(!d_xp || !d_xj || !d_B || !d_items || !d_scores, n_rows, n_items, d_B, ld_B, b_is_double ? 2 : 4, d_nr_p,
                               d_nr_j, d_excl0, n_exclude, k, ws_rows);
  if (rc || n_rows == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> h_xp;
  if ((rc = fetch_row_pointers(d_xp, (size_t)n_rows, h_xp, s, "x_p"))) return rc;
  int64_t rows = 0;
  void* ws = nullptr;
  if ((rc = knn_workspace(n_rows, (size_t)n_items * sizeof(uint64_t), ws_rows, rows, ws, s))) return rc;
  const int32_t* excl = n_exclude > 0 ? d_excl0 : nullptr;
  auto* w64 = static_cast<unsigned long long*>(ws);
  auto* sc = reinterpret_cast<long long*>(d_scores);
  hipError_t e = b_is_double ? launch_ease_recommend(d_xp, d_xj, n_rows, n_items, static_cast<const double*>(d_B), ld_B, d_nr_p, d_nr_j,
                                                     excl, n_exclude, k, rows, w64, d_items, sc, s)
                             : launch_ease_recommend(d_xp, d_xj, n_rows, n_items, static_cast<const float*>(d_B), ld_B, d_nr_p, d_nr_j,
                                                     excl, n_exclude, k, rows, w64, d_items, sc, s);
  if (e != hipSuccess) return hip_fail(e, "launch_ease_recommend");
  g_ws.knn_dirty = false;
  return RSPARSE_HIP_OK;
}

namespace {
// SLIM's own grow-only scratch, per host thread and per device like the workspace above, and apart from it: no other entry sees it
struct SlimScratch {
  GrowBufBase* all = nullptr;
  GrowBuf<int32_t> m{all};    // the support size of every column of a call
  GrowBuf<char> state{all};   // the state slices of the columns beyond RSPARSE_HIP_SLIM_LDS_SUPPORT
  int device = -1;
  int ensure_device() {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != device) {
      GrowBufBase::release_all(all);
      device = dev;
    }
    return RSPARSE_HIP_OK;
  }
};
thread_local SlimScratch g_slim;
}  // namespace

// SLIM (wrmf_slim.hip); the host form rsparse_hip_slim_fit: wrmf_capi_host.cpp
int rsparse_hip_slim_columns_device(const double* d_G, size_t ld_G, int n_items, const int32_t* d_cols, int n_cols, double l1,
                                    double l2, int max_iter, double tol, void* d_W, size_t ld_W, int w_is_double, int32_t* d_sweeps,
                                    void* stream) {
  int rc = slim_args(!d_G || !d_cols || !d_W || !d_sweeps, n_items, n_cols, l1, l2, max_iter, tol, ld_G, d_W, ld_W, w_is_double ? 2 : 4);
  if (rc || n_cols == 0) return rc;
  if (n_items == 0) return fail(RSPARSE_HIP_ERR_INVALID, "a column outside [0, n_items)");
  hipStream_t s = (hipStream_t)stream;
  if ((rc = g_slim.ensure_device())) return rc;
  HIP_TRY(g_slim.m.ensure((size_t)n_cols));
  launch_slim_support(d_G, ld_G, n_items, d_cols, n_cols, g_slim.m, s);
  std::vector<int32_t> m((size_t)n_cols);
  HIP_TRY(hipMemcpyAsync(m.data(), g_slim.m, m.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  int n_lds = 0, n_global = 0, max_support = 0;
  for (int32_t v : m) {
    if (v < 0) return fail(RSPARSE_HIP_ERR_INVALID, "a column outside [0, n_items)");
    (v <= RSPARSE_HIP_SLIM_LDS_SUPPORT ? n_lds : n_global)++;
    max_support = std::max(max_support, (int)v);
  }
  int slices = 0, stride = 0;
  if (n_global) HIP_TRY(g_slim.state.ensure(slim_state_bytes(n_global, max_support, slices, stride)));
  hipError_t e = launch_slim_columns(d_G, ld_G, n_items, d_cols, g_slim.m, n_cols, n_lds, slices, stride, l1, l2, max_iter, tol, d_W,
                                     ld_W, w_is_double != 0, d_sweeps, g_slim.state, s);
  if (e != hipSuccess) return hip_fail(e, "launch_slim_columns");
  return RSPARSE_HIP_OK;
}

namespace {
// what the evaluation entries do between their argument checks and their launches: x's row pointers on the host, the workspace
static int knn_rows_begin(const int32_t* d_xp, int n_rows, int n_items, int64_t ws_rows, std::vector<int32_t>& h_xp, int64_t& rows,
                          unsigned long long*& ws, hipStream_t s) {
  if (int rc = fetch_row_pointers(d_xp, (size_t)n_rows, h_xp, s, "x_p")) return rc;
  void* buf = nullptr;
  if (int rc = knn_workspace(n_rows, (size_t)n_items * sizeof(uint64_t), ws_rows, rows, buf, s)) return rc;
  ws = static_cast<unsigned long long*>(buf);
  return RSPARSE_HIP_OK;
}
}  // namespace

int rsparse_hip_knn_score_pairs_device(const int32_t* d_xp, const int32_t* d_xj, const uint32_t* d_xv, int n_rows, int n_items,
                                       const int32_t* d_neighbors, const uint32_t* d_q, int K, const int32_t* d_pairs_p,
                                       const int32_t* d_pairs_j, int64_t ws_rows, int64_t* d_scores, void* stream) {
  int rc = knn_recommend_args(!d_xp || !d_xj || !d_neighbors || !d_q || !d_pairs_p || !d_pairs_j || !d_scores, n_rows, n_items, K, nullptr,
                              nullptr, nullptr, 0, 1, ws_rows);
  if (rc || n_rows == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> h_xp, h_pp;
  if ((rc = fetch_row_pointers(d_pairs_p, (size_t)n_rows, h_pp, s, "pairs_p"))) return rc;
  int64_t rows = 0;
  unsigned long long* ws = nullptr;
  if ((rc = knn_rows_begin(d_xp, n_rows, n_items, ws_rows, h_xp, rows, ws, s))) return rc;
  hipError_t e = launch_knn_score_pairs(d_xp, d_xj, d_xv, n_rows, n_items, h_xp.data(), d_neighbors, d_q, K, d_pairs_p, d_pairs_j,
                                        h_pp.data(), rows, ws, reinterpret_cast<long long*>(d_scores), s);
  if (e != hipSuccess) return hip_fail(e, "launch_knn_score_pairs");
  g_ws.knn_dirty = false;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_knn_top_candidates_device(const int32_t* d_xp, const int32_t* d_xj, const uint32_t* d_xv, int n_rows, int n_items,
                                          const int32_t* d_neighbors, const uint32_t* d_q, int K, const int32_t* d_cand_p,
                                          const int32_t* d_cand_j, const int32_t* d_nr_p, const int32_t* d_nr_j, const int32_t* d_excl0,
                                          int n_exclude, int k, int64_t ws_rows, int32_t* d_items, int64_t* d_scores, void* stream) {
  int rc = knn_recommend_args(!d_xp || !d_xj || !d_neighbors || !d_q || !d_cand_p || !d_cand_j || !d_items || !d_scores, n_rows, n_items, K,
                              d_nr_p, d_nr_j, d_excl0, n_exclude, k, ws_rows);
  if (rc || n_rows == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> h_xp, h_cp;
  if ((rc = fetch_row_pointers(d_cand_p, (size_t)n_rows, h_cp, s, "cand_p"))) return rc;
  int64_t rows = 0;
  unsigned long long* ws = nullptr;
  if ((rc = knn_rows_begin(d_xp, n_rows, n_items, ws_rows, h_xp, rows, ws, s))) return rc;
  hipError_t e = launch_knn_top_candidates(d_xp, d_xj, d_xv, n_rows, n_items, h_xp.data(), d_neighbors, d_q, K, d_cand_p, d_cand_j,
                                           h_cp.data(), d_nr_p, d_nr_j, n_exclude > 0 ? d_excl0 : nullptr, n_exclude, k, rows, ws, d_items,
                                           reinterpret_cast<long long*>(d_scores), s);
  if (e != hipSuccess) return hip_fail(e, "launch_knn_top_candidates");
  g_ws.knn_dirty = false;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_knn_held_out_ranks_device(const int32_t* d_xp, const int32_t* d_xj, const uint32_t* d_xv, int n_rows, int n_items,
                                          const int32_t* d_neighbors, const uint32_t* d_q, int K, const int32_t* d_actual_p,
                                          const int32_t* d_actual_j, const int32_t* d_nr_p, const int32_t* d_nr_j, const int32_t* d_excl0,
                                          int n_exclude, int64_t ws_rows, int32_t* d_above, int32_t* d_tied, int32_t* d_n_adm,
                                          void* stream) {
  int rc = knn_recommend_args(!d_xp || !d_xj || !d_neighbors || !d_q || !d_actual_p || !d_actual_j || !d_above || !d_tied || !d_n_adm,
                              n_rows, n_items, K, d_nr_p, d_nr_j, d_excl0, n_exclude, 1, ws_rows);
  if (rc || n_rows == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> h_xp;
  int64_t rows = 0;
  unsigned long long* ws = nullptr;
  if ((rc = knn_rows_begin(d_xp, n_rows, n_items, ws_rows, h_xp, rows, ws, s))) return rc;
  hipError_t e = launch_knn_held_out_ranks(d_xp, d_xj, d_xv, n_rows, n_items, h_xp.data(), d_neighbors, d_q, K, d_actual_p, d_actual_j,
                                           d_nr_p, d_nr_j, n_exclude > 0 ? d_excl0 : nullptr, n_exclude, rows, ws, d_above, d_tied, d_n_adm,
                                           s);
  if (e != hipSuccess) return hip_fail(e, "launch_knn_held_out_ranks");
  g_ws.knn_dirty = false;
  return RSPARSE_HIP_OK;
}

// EASE under the same protocols (wrmf_ease.hip); the host forms rsparse_hip_ease_top_candidates / _held_out_ranks: wrmf_capi_host.cpp
int rsparse_hip_ease_score_pairs_device(const int32_t* d_xp, const int32_t* d_xj, int n_rows, int n_items, const void* d_B, size_t ld_B,
                                        int b_is_double, const int32_t* d_pairs_p, const int32_t* d_pairs_j, int64_t ws_rows,
                                        uint64_t* d_scores, void* stream) {
  int rc = ease_recommend_args(!d_xp || !d_xj || !d_B || !d_pairs_p || !d_pairs_j || !d_scores, n_rows, n_items, d_B, ld_B,
                               b_is_double ? 2 : 4, nullptr, nullptr, nullptr, 0, 1, ws_rows);
  if (rc || n_rows == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> h_xp, h_pp;
  if ((rc = fetch_row_pointers(d_pairs_p, (size_t)n_rows, h_pp, s, "pairs_p"))) return rc;
  int64_t rows = 0;
  unsigned long long* ws = nullptr;
  if ((rc = knn_rows_begin(d_xp, n_rows, n_items, ws_rows, h_xp, rows, ws, s))) return rc;
  auto* sc = reinterpret_cast<unsigned long long*>(d_scores);
  hipError_t e = b_is_double ? launch_ease_score_pairs(d_xp, d_xj, n_rows, n_items, static_cast<const double*>(d_B), ld_B, d_pairs_p,
                                                       d_pairs_j, h_pp.data(), rows, ws, sc, s)
                             : launch_ease_score_pairs(d_xp, d_xj, n_rows, n_items, static_cast<const float*>(d_B), ld_B, d_pairs_p,
                                                       d_pairs_j, h_pp.data(), rows, ws, sc, s);
  if (e != hipSuccess) return hip_fail(e, "launch_ease_score_pairs");
  g_ws.knn_dirty = false;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_ease_top_candidates_device(const int32_t* d_xp, const int32_t* d_xj, int n_rows, int n_items, const void* d_B, size_t ld_B,
                                           int b_is_double, const int32_t* d_cand_p, const int32_t* d_cand_j, const int32_t* d_nr_p,
                                           const int32_t* d_nr_j, const int32_t* d_excl0, int n_exclude, int k, int64_t ws_rows,
                                           int32_t* d_items, uint64_t* d_scores, void* stream) {
  int rc = ease_recommend_args(!d_xp || !d_xj || !d_B || !d_cand_p || !d_cand_j || !d_items || !d_scores, n_rows, n_items, d_B, ld_B,
                               b_is_double ? 2 : 4, d_nr_p, d_nr_j, d_excl0, n_exclude, k, ws_rows);
  if (rc || n_rows == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> h_xp, h_cp;
  if ((rc = fetch_row_pointers(d_cand_p, (size_t)n_rows, h_cp, s, "cand_p"))) return rc;
  int64_t rows = 0;
  unsigned long long* ws = nullptr;
  if ((rc = knn_rows_begin(d_xp, n_rows, n_items, ws_rows, h_xp, rows, ws, s))) return rc;
  HIP_TRY(g_ws.score_buf.ensure((size_t)h_cp[n_rows] + 1));   // the cell route's keys, one per candidate slot (absolute)
  auto* keys = reinterpret_cast<unsigned long long*>(static_cast<double*>(g_ws.score_buf));
  const int32_t* excl = n_exclude > 0 ? d_excl0 : nullptr;
  auto* sc = reinterpret_cast<long long*>(d_scores);
  hipError_t e = b_is_double ? launch_ease_top_candidates(d_xp, d_xj, n_rows, n_items, static_cast<const double*>(d_B), ld_B, d_cand_p,
                                                          d_cand_j, h_cp.data(), d_nr_p, d_nr_j, excl, n_exclude, k, rows, ws, keys,
                                                          d_items, sc, s)
                             : launch_ease_top_candidates(d_xp, d_xj, n_rows, n_items, static_cast<const float*>(d_B), ld_B, d_cand_p,
                                                          d_cand_j, h_cp.data(), d_nr_p, d_nr_j, excl, n_exclude, k, rows, ws, keys,
                                                          d_items, sc, s);
  if (e != hipSuccess) return hip_fail(e, "launch_ease_top_candidates");
  g_ws.knn_dirty = false;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_ease_held_out_ranks_device(const int32_t* d_xp, const int32_t* d_xj, int n_rows, int n_items, const void* d_B, size_t ld_B,
                                           int b_is_double, const int32_t* d_actual_p, const int32_t* d_actual_j, const int32_t* d_nr_p,
                                           const int32_t* d_nr_j, const int32_t* d_excl0, int n_exclude, int64_t ws_rows, int32_t* d_above,
                                           int32_t* d_tied, int32_t* d_n_adm, void* stream) {
  int rc = ease_recommend_args(!d_xp || !d_xj || !d_B || !d_actual_p || !d_actual_j || !d_above || !d_tied || !d_n_adm, n_rows, n_items,
                               d_B, ld_B, b_is_double ? 2 : 4, d_nr_p, d_nr_j, d_excl0, n_exclude, 1, ws_rows);
  if (rc || n_rows == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> h_xp;
  int64_t rows = 0;
  unsigned long long* ws = nullptr;
  if ((rc = knn_rows_begin(d_xp, n_rows, n_items, ws_rows, h_xp, rows, ws, s))) return rc;
  const int32_t* excl = n_exclude > 0 ? d_excl0 : nullptr;
  hipError_t e = b_is_double ? launch_ease_held_out_ranks(d_xp, d_xj, n_rows, n_items, static_cast<const double*>(d_B), ld_B, d_actual_p,
                                                          d_actual_j, d_nr_p, d_nr_j, excl, n_exclude, rows, ws, d_above, d_tied, d_n_adm, s)
                             : launch_ease_held_out_ranks(d_xp, d_xj, n_rows, n_items, static_cast<const float*>(d_B), ld_B, d_actual_p,
                                                          d_actual_j, d_nr_p, d_nr_j, excl, n_exclude, rows, ws, d_above, d_tied, d_n_adm, s);
  if (e != hipSuccess) return hip_fail(e, "launch_ease_held_out_ranks");
  g_ws.knn_dirty = false;
  return RSPARSE_HIP_OK;
}

// `_f64_device`: wrmf_f64_capi.cpp; the host form rsparse_hip_top_candidates: wrmf_capi_host.cpp
int rsparse_hip_top_candidates_device(const float* d_U, const float* d_V, int n_users, int n_items, int rank, int k,
                                      const int32_t* d_cand_p, const int32_t* d_cand_j, const int32_t* d_nr_p, const int32_t* d_nr_j,
                                      const int32_t* d_excl0, int n_exclude, double glob_mean, int32_t* d_res, double* d_scores,
                                      void* stream) {
  return top_candidates_device(d_U, d_V, n_users, n_items, rank, k, d_cand_p, d_cand_j, d_nr_p, d_nr_j, d_excl0, n_exclude, glob_mean,
                               d_res, d_scores, (hipStream_t)stream, RSPARSE_HIP_MAX_RANK, [](size_t n, double*& buf) {
                                 if (int rc = g_ws.ensure_device()) return rc;
                                 HIP_TRY(g_ws.score_buf.ensure(n));
                                 buf = g_ws.score_buf;
                                 return (int)RSPARSE_HIP_OK;
                               });
}

// `_f64_device`: wrmf_f64_capi.cpp
int rsparse_hip_explain_device(const float* d_V, int n_items, int r, const float* d_base, double diag, double diag_per_nnz,
                               int n_users, const int32_t* d_x_p, const int32_t* d_x_j, const float* d_wa, const float* d_wb,
                               const int32_t* d_t_p, const int32_t* d_t_j, const int64_t* d_out_p, float* d_contrib,
                               double* d_total, int32_t* d_flags, void* stream) {
  return explain_device(d_V, n_items, r, d_base, diag, diag_per_nnz, n_users, d_x_p, d_x_j, d_wa, d_wb, d_t_p, d_t_j, d_out_p,
                        d_contrib, d_total, d_flags, (hipStream_t)stream);
}

// `_f64_device`: wrmf_f64_capi.cpp
int rsparse_hip_init_factors_device(uint64_t seed, int stream, int64_t row0, int n_rows, int rank, int64_t ld, double scale,
                                    int abs_values, int ones_col, void* d_out, void* hip_stream) {
  return init_factors_device(seed, stream, row0, n_rows, rank, ld, scale, abs_values, ones_col, static_cast<float*>(d_out),
                             (hipStream_t)hip_stream);
}

extern "C++" {
namespace {
// BPR (wrmf_bpr.hip), both precisions; the host form rsparse_hip_bpr_fit: wrmf_capi_host.cpp
BprRun bpr_run_of(const int32_t* d_p, const int32_t* d_j, int n_rows, int n_items, int64_t nnz, int64_t row0, uint64_t seed, int mode,
                  int n_steps, int rank, double lr, double lambda, int update_items) {
  BprRun r;
  r.p = d_p; r.j = d_j; r.n_rows = n_rows; r.n_items = n_items; r.nnz = nnz; r.row0 = row0; r.seed = seed; r.mode = mode;
  r.n_steps = n_steps; r.rank = rank; r.lr = lr; r.lambda = lambda; r.update_items = update_items != 0;
  return r;
}

template <class T>
int bpr_step_device(const int32_t* d_p, const int32_t* d_j, int n_rows, int n_items, int64_t nnz, int64_t row0, uint64_t seed, int mode,
                    int epoch, int step, int n_steps, int rank, double lr, double lambda, int update_items, T* d_U, T* d_V,
                    double* d_aU, double* d_aV, int64_t* d_counts, void* stream, int max_rank) {
  int rc = bpr_args(!d_p || !d_j || !d_U || !d_V || !d_aU || !d_aV || !d_counts, n_rows, n_items, nnz, row0, mode, epoch, 1, n_steps,
                    "n_steps", rank, max_rank, lr, lambda);
  if (rc) return rc;
  if (step < 0 || step >= n_steps) return fail(RSPARSE_HIP_ERR_INVALID, "step outside [0, n_steps)");
  if ((rc = bpr_step_size(nnz, n_steps, update_items))) return rc;
  if (n_rows == 0 || nnz == 0) return RSPARSE_HIP_OK;
  hipError_t e = launch_bpr_run<T>(bpr_run_of(d_p, d_j, n_rows, n_items, nnz, row0, seed, mode, n_steps, rank, lr, lambda, update_items),
                                   epoch, 1, step, d_U, d_V, d_aU, d_aV, reinterpret_cast<unsigned long long*>(d_counts),
                                   (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "launch_bpr_run");
  return RSPARSE_HIP_OK;
}

template <class T>
int bpr_epochs_device(const int32_t* d_p, const int32_t* d_j, int n_rows, int n_items, int64_t nnz, int64_t row0, uint64_t seed, int mode,
                      int epoch0, int n_epochs, int batch, int rank, double lr, double lambda, int update_items, T* d_U, T* d_V,
                      double* d_aU, double* d_aV, int64_t* d_counts, void* stream, int max_rank) {
  int rc = bpr_args(!d_p || !d_j || !d_U || !d_V || !d_aU || !d_aV || !d_counts, n_rows, n_items, nnz, row0, mode, epoch0, n_epochs,
                    batch, "batch", rank, max_rank, lr, lambda);
  if (rc) return rc;
  const int n_steps = mode == 1 || nnz == 0 ? 1 : (int)((nnz + batch - 1) / batch);
  if ((rc = bpr_step_size(nnz, n_steps, update_items))) return rc;
  if (n_rows == 0 || n_epochs == 0) return RSPARSE_HIP_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(d_counts, 0, 2 * (size_t)n_epochs * sizeof(int64_t), s));
  if (nnz == 0) return RSPARSE_HIP_OK;
  hipError_t e = launch_bpr_run<T>(bpr_run_of(d_p, d_j, n_rows, n_items, nnz, row0, seed, mode, n_steps, rank, lr, lambda, update_items),
                                   epoch0, n_epochs, -1, d_U, d_V, d_aU, d_aV, reinterpret_cast<unsigned long long*>(d_counts), s);
  if (e != hipSuccess) return hip_fail(e, "launch_bpr_run");
  return RSPARSE_HIP_OK;
}
}  // namespace
}  // extern "C++"

int rsparse_hip_bpr_triples_device(const int32_t* d_p, const int32_t* d_j, int n_rows, int n_items, int64_t nnz, int64_t row0,
                                   uint64_t seed, int mode, int epoch, int step, int n_steps, int32_t* d_u, int32_t* d_i,
                                   int32_t* d_neg, void* stream) {
  int rc = bpr_args(!d_p || !d_j || !d_u || !d_i || !d_neg, n_rows, n_items, nnz, row0, mode, epoch, 1, n_steps, "n_steps", 0, 0, 0.0,
                    0.0);
  if (rc) return rc;
  if (step < 0 || step >= n_steps) return fail(RSPARSE_HIP_ERR_INVALID, "step outside [0, n_steps)");
  if (n_rows == 0 || nnz == 0) return RSPARSE_HIP_OK;
  hipError_t e = launch_bpr_triples(bpr_run_of(d_p, d_j, n_rows, n_items, nnz, row0, seed, mode, n_steps, 0, 0.0, 0.0, 0), epoch, step,
                                    d_u, d_i, d_neg, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "launch_bpr_triples");
  return RSPARSE_HIP_OK;
}

int rsparse_hip_bpr_step_device(const int32_t* d_p, const int32_t* d_j, int n_rows, int n_items, int64_t nnz, int64_t row0,
                                uint64_t seed, int mode, int epoch, int step, int n_steps, int rank, double learning_rate,
                                double lambda, int update_items, float* d_U, float* d_V, double* d_aU, double* d_aV,
                                int64_t* d_counts, void* stream) {
  return bpr_step_device<float>(d_p, d_j, n_rows, n_items, nnz, row0, seed, mode, epoch, step, n_steps, rank, learning_rate, lambda,
                                update_items, d_U, d_V, d_aU, d_aV, d_counts, stream, RSPARSE_HIP_MAX_RANK);
}

int rsparse_hip_bpr_step_f64_device(const int32_t* d_p, const int32_t* d_j, int n_rows, int n_items, int64_t nnz, int64_t row0,
                                    uint64_t seed, int mode, int epoch, int step, int n_steps, int rank, double learning_rate,
                                    double lambda, int update_items, double* d_U, double* d_V, double* d_aU, double* d_aV,
                                    int64_t* d_counts, void* stream) {
  return bpr_step_device<double>(d_p, d_j, n_rows, n_items, nnz, row0, seed, mode, epoch, step, n_steps, rank, learning_rate, lambda,
                                 update_items, d_U, d_V, d_aU, d_aV, d_counts, stream, RSPARSE_HIP_MAX_RANK_F64);
}

int rsparse_hip_bpr_epochs_device(const int32_t* d_p, const int32_t* d_j, int n_rows, int n_items, int64_t nnz, int64_t row0,
                                  uint64_t seed, int mode, int epoch0, int n_epochs, int batch, int rank, double learning_rate,
                                  double lambda, int update_items, float* d_U, float* d_V, double* d_aU, double* d_aV,
                                  int64_t* d_counts, void* stream) {
  return bpr_epochs_device<float>(d_p, d_j, n_rows, n_items, nnz, row0, seed, mode, epoch0, n_epochs, batch, rank, learning_rate, lambda,
                                  update_items, d_U, d_V, d_aU, d_aV, d_counts, stream, RSPARSE_HIP_MAX_RANK);
}

int rsparse_hip_bpr_epochs_f64_device(const int32_t* d_p, const int32_t* d_j, int n_rows, int n_items, int64_t nnz, int64_t row0,
                                      uint64_t seed, int mode, int epoch0, int n_epochs, int batch, int rank, double learning_rate,
                                      double lambda, int update_items, double* d_U, double* d_V, double* d_aU, double* d_aV,
                                      int64_t* d_counts, void* stream) {
  return bpr_epochs_device<double>(d_p, d_j, n_rows, n_items, nnz, row0, seed, mode, epoch0, n_epochs, batch, rank, learning_rate,
                                   lambda, update_items, d_U, d_V, d_aU, d_aV, d_counts, stream, RSPARSE_HIP_MAX_RANK_F64);
}

namespace {
// the device form of both samplers: d_cum == nullptr is the uniform stream, otherwise the weighted one under that prefix
int sample_negatives_device(uint64_t seed, int64_t row0, int n_rows, int n_item, int n, const int32_t* d_seen_p,
                            const int32_t* d_seen_j, const int32_t* d_keep_p, const int32_t* d_keep_j, const uint64_t* d_cum,
                            bool weighted, int32_t* d_out_p, int32_t* d_out_j, int64_t out_capacity, int32_t* d_filled_rows,
                            void* stream) {
  int rc = sample_negatives_args(row0, n_rows, n_item, n, d_seen_p, d_seen_j, d_keep_p, d_keep_j, d_out_p, out_capacity);
  if (rc) return rc;
  if (!d_out_j) return fail(RSPARSE_HIP_ERR_INVALID, "out_j is NULL");
  if (weighted && !d_cum) return fail(RSPARSE_HIP_ERR_INVALID, "d_cum is NULL");
  if (n_rows == 0) return RSPARSE_HIP_OK;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = g_ws.ensure_device())) return rc;
  HIP_TRY(g_ws.score_buf.ensure((sample_negatives_ws_bytes(n_rows) + 7) / 8));
  SampleStatus* d_status = nullptr;
  hipError_t e = launch_sample_row_pointers(n_rows, n_item, n, d_seen_p, d_keep_p, d_out_p, g_ws.score_buf, &d_status, s);
  if (e != hipSuccess) return hip_fail(e, "launch_sample_row_pointers");
  SampleStatus st = {0, 0, 0};
  HIP_TRY(hipMemcpyAsync(&st, d_status, sizeof(st), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (st.flag)
    return fail(RSPARSE_HIP_ERR_INVALID, "row pointers that are negative or decrease, a seen row longer than n_item or a keep row longer than its seen row");
  if (st.total > 0x7fffffffll) return fail(RSPARSE_HIP_ERR_INVALID, "the output has more than 2^31 - 1 entries: sample the rows in batches");
  if (st.total > out_capacity)
    return fail(RSPARSE_HIP_ERR_INVALID, "out_capacity is " + std::to_string(out_capacity) + ", the rows need " + std::to_string(st.total));
  if (!weighted) {
    e = launch_sample_negatives(seed, row0, n_rows, n_item, n, d_seen_p, d_seen_j, d_keep_p, d_keep_j, d_out_p, d_out_j, s);
    if (e != hipSuccess) return hip_fail(e, "launch_sample_negatives");
    return RSPARSE_HIP_OK;
  }
  if (d_filled_rows) HIP_TRY(hipMemsetAsync(d_filled_rows, 0, sizeof(int32_t), s));
  e = launch_sample_negatives_weighted(seed, row0, n_rows, n_item, n, d_seen_p, d_seen_j, d_keep_p, d_keep_j, d_cum, d_out_p, d_out_j,
                                       d_filled_rows, s);
  if (e != hipSuccess) return hip_fail(e, "launch_sample_negatives_weighted");
  return RSPARSE_HIP_OK;
}
}  // namespace

int rsparse_hip_sample_negatives_device(uint64_t seed, int64_t row0, int n_rows, int n_item, int n, const int32_t* d_seen_p,
                                        const int32_t* d_seen_j, const int32_t* d_keep_p, const int32_t* d_keep_j,
                                        int32_t* d_out_p, int32_t* d_out_j, int64_t out_capacity, void* stream) {
  return sample_negatives_device(seed, row0, n_rows, n_item, n, d_seen_p, d_seen_j, d_keep_p, d_keep_j, nullptr, false, d_out_p, d_out_j,
                                 out_capacity, nullptr, stream);
}

int rsparse_hip_weights_prefix_device(const uint32_t* d_w, int n_item, uint64_t* d_cum, void* stream) {
  if (n_item < 0) return fail(RSPARSE_HIP_ERR_INVALID, "n_item < 0");
  if (!d_w || !d_cum) return fail(RSPARSE_HIP_ERR_INVALID, "d_w or d_cum is NULL");
  if (n_item == 0) return RSPARSE_HIP_OK;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = g_ws.ensure_device()) return rc;
  HIP_TRY(g_ws.score_buf.ensure((weights_prefix_ws_bytes(n_item) + 7) / 8));
  int* d_flag = nullptr;
  hipError_t e = launch_weights_prefix(d_w, n_item, d_cum, g_ws.score_buf, &d_flag, s);
  if (e != hipSuccess) return hip_fail(e, "launch_weights_prefix");
  int flag = 0;
  HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(flag), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (flag) return fail(RSPARSE_HIP_ERR_INVALID, "a weight is 0: every weight is at least 1 (exclude an item through the seen rows)");
  return RSPARSE_HIP_OK;
}

int rsparse_hip_sample_negatives_weighted_device(uint64_t seed, int64_t row0, int n_rows, int n_item, int n, const int32_t* d_seen_p,
                                                 const int32_t* d_seen_j, const int32_t* d_keep_p, const int32_t* d_keep_j,
                                                 const uint64_t* d_cum, int32_t* d_out_p, int32_t* d_out_j, int64_t out_capacity,
                                                 int32_t* d_filled_rows, void* stream) {
  return sample_negatives_device(seed, row0, n_rows, n_item, n, d_seen_p, d_seen_j, d_keep_p, d_keep_j, d_cum, true, d_out_p, d_out_j,
                                 out_capacity, d_filled_rows, stream);
}

int rsparse_hip_split_rows_device(uint64_t seed, int64_t row0, int n_rows, int mode, uint64_t test_threshold, int leave_out,
                                  int min_train, const int32_t* d_p, const int32_t* d_j, const void* d_v, int value_bytes,
                                  const double* d_by, int32_t* d_train_p, int32_t* d_train_j, void* d_train_v, int32_t* d_test_p,
                                  int32_t* d_test_j, void* d_test_v, int64_t train_capacity, int64_t test_capacity, void* stream) {
  int rc = split_rows_args(row0, n_rows, mode, test_threshold, leave_out, min_train, d_p, d_j, d_v, value_bytes, d_by, d_train_p,
                           d_train_j, d_train_v, d_test_p, d_test_j, d_test_v, train_capacity, test_capacity);
  if (rc) return rc;
  if (n_rows == 0) return RSPARSE_HIP_OK;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = g_ws.ensure_device())) return rc;
  HIP_TRY(g_ws.score_buf.ensure((split_ws_bytes(n_rows) + 7) / 8));
  SplitStatus* d_status = nullptr;
  hipError_t e = launch_split_count(seed, row0, n_rows, mode, test_threshold, leave_out, min_train, d_p, d_by, d_train_p, d_test_p,
                                    g_ws.score_buf, &d_status, s);
  if (e != hipSuccess) return hip_fail(e, "launch_split_count");
  SplitStatus st = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(&st, d_status, sizeof(st), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (st.flag) return fail(RSPARSE_HIP_ERR_INVALID, "row pointers that are negative or decrease");
  if (!d_train_j) return RSPARSE_HIP_OK;   // the sizes only
  if (st.total_train > train_capacity || st.total_test > test_capacity)
    return fail(RSPARSE_HIP_ERR_INVALID, "the capacities are " + std::to_string(train_capacity) + " / " + std::to_string(test_capacity) +
                                             ", the split needs " + std::to_string(st.total_train) + " / " + std::to_string(st.total_test));
  if (st.total_train + st.total_test == 0) return RSPARSE_HIP_OK;
  e = launch_split_write(seed, row0, n_rows, mode, test_threshold, leave_out, min_train, d_p, d_j, d_v, value_bytes, d_by, d_train_p,
                         d_train_j, d_train_v, d_test_p, d_test_j, d_test_v, g_ws.score_buf, s);
  if (e != hipSuccess) return hip_fail(e, "launch_split_write");
  return RSPARSE_HIP_OK;
}

namespace {
int confidence_apply_args(int kind, int n_seg, int64_t nnz, const void* p, const void* i, const void* x, const void* seg_table,
                          const void* idx_table, int n_idx, int seg_is_item, double b, const void* out, int out_float) {
  if (n_seg < 0 || nnz < 0 || n_idx < 0) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_seg < 0, nnz < 0 or n_idx < 0)");
  if (kind < RSPARSE_HIP_CONFIDENCE_LINEAR || kind > RSPARSE_HIP_CONFIDENCE_NORMALIZE)
    return fail(RSPARSE_HIP_ERR_INVALID, "unknown confidence kind " + std::to_string(kind));
  if (nnz > 0 && (!p || !x || !out)) return fail(RSPARSE_HIP_ERR_INVALID, "p, x or out is NULL");
  if (nnz > 0 && idx_table && !i) return fail(RSPARSE_HIP_ERR_INVALID, "an index table without indices");
  const void* item_table = seg_is_item ? seg_table : idx_table;
  const void* user_table = seg_is_item ? idx_table : seg_table;
  bool ok = true;
  switch (kind) {
    case RSPARSE_HIP_CONFIDENCE_TFIDF: ok = item_table && !user_table; break;
    case RSPARSE_HIP_CONFIDENCE_BM25: ok = item_table && user_table; break;
    case RSPARSE_HIP_CONFIDENCE_NORMALIZE: ok = !seg_table != !idx_table; break;
    default: ok = !seg_table && !idx_table;
  }
  if (!ok) return fail(RSPARSE_HIP_ERR_INVALID, "a missing or surplus table for confidence kind " + std::to_string(kind));
  if (kind == RSPARSE_HIP_CONFIDENCE_LOG && !(b != 0.0)) return fail(RSPARSE_HIP_ERR_INVALID, "eps must not be 0");
  if (out_float && nnz > 0) {
    const char *xb = static_cast<const char*>(x), *ob = static_cast<const char*>(out);
    if (ob < xb + (size_t)nnz * 8 && xb < ob + (size_t)nnz * 4) return fail(RSPARSE_HIP_ERR_INVALID, "a float output overlaps the values");
  }
  return RSPARSE_HIP_OK;
}
}  // namespace

int rsparse_hip_confidence_moments_device(int n_seg, int64_t nnz, const int32_t* d_p, const double* d_x, int power, double* d_out,
                                          double* d_total, void* stream) {
  if (n_seg < 0 || nnz < 0) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_seg < 0 or nnz < 0)");
  if (power != 1 && power != 2) return fail(RSPARSE_HIP_ERR_INVALID, "power must be 1 or 2");
  if (!d_total || (n_seg > 0 && !d_out) || (nnz > 0 && (!d_p || !d_x))) return fail(RSPARSE_HIP_ERR_INVALID, "NULL array");
  if (nnz > 0 && n_seg == 0) return fail(RSPARSE_HIP_ERR_INVALID, "entries without a segment");
  int rc;
  if ((rc = g_ws.ensure_device())) return rc;
  HIP_TRY(g_ws.score_buf.ensure(confidence_ws_doubles(nnz)));
  hipError_t e = launch_confidence_moments(d_p, d_x, n_seg, nnz, power, d_out, d_total, g_ws.score_buf, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "launch_confidence_moments");
  return RSPARSE_HIP_OK;
}

int rsparse_hip_confidence_table_device(int table, int n, const int32_t* d_p, const double* d_moment, const double* d_total, double a,
                                        double b, double c, double* d_out, void* stream) {
  if (n < 0) return fail(RSPARSE_HIP_ERR_INVALID, "negative length");
  if (table < RSPARSE_HIP_CONFIDENCE_TABLE_IDF || table > RSPARSE_HIP_CONFIDENCE_TABLE_NORM)
    return fail(RSPARSE_HIP_ERR_INVALID, "unknown confidence table " + std::to_string(table));
  if (table == RSPARSE_HIP_CONFIDENCE_TABLE_NORM && b != 1.0 && b != 2.0) return fail(RSPARSE_HIP_ERR_INVALID, "norm must be 1 or 2");
  if (n > 0) {
    const bool ok = d_out && (table == RSPARSE_HIP_CONFIDENCE_TABLE_IDF ? d_p != nullptr
                              : table == RSPARSE_HIP_CONFIDENCE_TABLE_BM25 ? d_moment && d_total : d_moment != nullptr);
    if (!ok) return fail(RSPARSE_HIP_ERR_INVALID, "NULL array");
  }
  if (n == 0) return RSPARSE_HIP_OK;
  hipError_t e = launch_confidence_table(table, n, d_p, d_moment, d_total, a, b, c, d_out, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "launch_confidence_table");
  return RSPARSE_HIP_OK;
}

int rsparse_hip_confidence_apply_device(int kind, int n_seg, int64_t nnz, const int32_t* d_p, const int32_t* d_i, const double* d_x,
                                        const double* d_seg_table, const double* d_idx_table, int n_idx, int seg_is_item, double a,
                                        double b, void* d_out, int out_float, void* stream) {
  int rc = confidence_apply_args(kind, n_seg, nnz, d_p, d_i, d_x, d_seg_table, d_idx_table, n_idx, seg_is_item, b, d_out, out_float);
  if (rc) return rc;
  if (nnz == 0) return RSPARSE_HIP_OK;
  if (n_seg == 0) return fail(RSPARSE_HIP_ERR_INVALID, "entries without a segment");
  hipError_t e = launch_confidence_apply(kind, d_p, d_i, d_x, n_seg, nnz, d_seg_table, d_idx_table, n_idx, seg_is_item ? 1 : 0, a, b,
                                         d_out, out_float ? 1 : 0, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "launch_confidence_apply");
  return RSPARSE_HIP_OK;
}

int rsparse_hip_events_to_csr_device(int64_t n_events, int n_users, int n_items, const int32_t* d_users, const int32_t* d_items,
                                     const double* d_values, const double* d_timestamps, int aggregate, double half_life, double now,
                                     int has_now, int32_t* d_p, int32_t* d_j, double* d_x, int32_t* d_count, double* d_latest,
                                     int64_t capacity, int64_t* n_cells, void* stream) {
  int rc = events_args(n_events, n_users, n_items, d_users, d_items, d_timestamps, aggregate, half_life, d_p, d_j, d_x, capacity, n_cells);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = g_ws.ensure_device())) return rc;
  *n_cells = 0;
  if (n_events == 0) {
    HIP_TRY(hipMemsetAsync(d_p, 0, ((size_t)n_users + 1) * 4, s));
    return RSPARSE_HIP_OK;
  }
  int status = 0;
  hipError_t e = events_to_csr_device(n_events, n_users, n_items, d_users, d_items, d_values, d_timestamps, aggregate, half_life, has_now,
                                      now, d_p, d_j, d_x, d_count, d_latest, capacity, n_cells, s, &status);
  if (e != hipSuccess) return hip_fail(e, "events_to_csr_device");
  if (status == 1) return fail(RSPARSE_HIP_ERR_INVALID, "a user or item id outside [0, n_users) x [0, n_items)");
  if (status == 2)
    return fail(RSPARSE_HIP_ERR_INVALID, "the capacity is " + std::to_string(capacity) + ", the log has " + std::to_string(*n_cells) + " cells");
  return RSPARSE_HIP_OK;
}

int rsparse_hip_take_numeric_failures(int64_t* unresolved_out, int64_t* fallback_out) {
  if (!unresolved_out) return fail(RSPARSE_HIP_ERR_INVALID, "unresolved_out is NULL");
  // counts a stateless call found on the device when it started and set aside (see StaleFailures): still the resident layer's
  *unresolved_out = g_fail_carry[0];
  if (fallback_out) *fallback_out = g_fail_carry[1];
  g_fail_carry[0] = g_fail_carry[1] = 0;
  if (!g_ws.fails) return RSPARSE_HIP_OK;
  int v[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpy(v, g_ws.fails, sizeof(v), hipMemcpyDeviceToHost));   // (synchronises with the device)
  if (v[0] | v[1] | v[2] | v[3]) {
    HIP_TRY(hipMemset(g_ws.fails, 0, sizeof(v)));
    HIP_TRY(hipStreamSynchronize(nullptr));   // (before a next call counts on a non-blocking stream: see ensure_device)
  }
  // rows beyond the list's capacity could not be handed over: they count as unresolved, not as re-solved
  const int64_t lost = v[0] > kFailCap ? (int64_t)v[0] - kFailCap : 0;
  const int64_t sent = (int64_t)std::min(v[0], kFailCap) + v[2];
  *unresolved_out += (int64_t)v[1] + v[3] + lost;
  if (fallback_out) *fallback_out += sent;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_als_implicit_float(int n_rows, int n_cols, const int32_t* col_ptrs, const int32_t* row_indices,
                                   const double* values, const float* X, float* Y, const float* XtX, int rank,
                                   double lambda, int n_threads, unsigned solver, unsigned cg_steps,
                                   int with_biases, int is_x_bias_last_row, double global_bias,
                                   float* global_bias_base, int global_bias_base_len, int initialize_bias_base,
                                   double* loss_out) {
  (void)n_threads;
  return stateless(true, n_rows, n_cols, col_ptrs, row_indices, values, X, Y, XtX, nullptr, rank, lambda, solver, cg_steps, 0,
                   loss_out, with_biases, is_x_bias_last_row, global_bias, global_bias_base, global_bias_base_len,
                   initialize_bias_base);
}

// Stateless counterpart of the .Call target _rsparse_initialize_biases_float (src/wrmf_init.cpp:5-34,
// src/RcppExports.cpp:417-454): the two S4 matrices flattened to their slots.  (The `_double` one: wrmf_f64_capi.cpp.)
int rsparse_hip_initialize_biases_float(int n_users, int n_items, const int32_t* csc_p, const int32_t* csc_i,
                                        double* csc_x, const int32_t* csr_p, const int32_t* csr_i, double* csr_x,
                                        float* user_bias, float* item_bias, double lambda, int dynamic_lambda,
                                        int non_negative, int calculate_global_bias, int is_explicit_feedback,
                                        double* global_bias_out) {
  if (!user_bias || !item_bias) return fail(RSPARSE_HIP_ERR_INVALID, "user_bias or item_bias is NULL");
  rsparse_hip_csc *c_ui = nullptr, *c_iu = nullptr;
  int rc = rsparse_hip_csc_create_host(n_users, n_items, csc_p, csc_i, csc_x, &c_ui);   // columns = items
  if (rc) return rc;
  CscGuard g1{c_ui};
  if ((rc = rsparse_hip_csc_create_host(n_items, n_users, csr_p, csr_i, csr_x, &c_iu))) return rc;   // columns = users
  CscGuard g2{c_iu};
  double gb = 0.0;
  rc = with_device_biases(n_users, n_items, user_bias, item_bias, [&](float* dU, float* dI) {
    return is_explicit_feedback
               ? rsparse_hip_initialize_biases_explicit_device(c_ui, c_iu, dU, dI, lambda, dynamic_lambda, non_negative,
                                                               calculate_global_bias, &gb, nullptr)
               : rsparse_hip_initialize_biases_implicit_device(c_ui, c_iu, dU, dI, lambda, non_negative, calculate_global_bias,
                                                               &gb, nullptr);
  });
  if (rc) return rc;
  if (is_explicit_feedback && calculate_global_bias) {
    // the reference removes the global mean from the @x slots of BOTH matrices in place (wrmf_utils.hpp:41-52): on the host
    // here, from the caller's doubles (the resident values are their float copies)
    const int64_t nnz = csc_p[n_items];
    for (int64_t e = 0; e < nnz; e++) csc_x[e] -= gb;
    for (int64_t e = 0; e < nnz; e++) csr_x[e] -= gb;
  }
  if (global_bias_out) *global_bias_out = gb;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_als_explicit_float(int n_rows, int n_cols, const int32_t* col_ptrs, const int32_t* row_indices,
                                   const double* values, const float* X, float* Y, const float* cnt_X, int rank,
                                   double lambda, unsigned n_threads, unsigned solver, unsigned cg_steps,
                                   int dynamic_lambda, int with_biases, int is_x_bias_last_row, double* loss_out) {
  (void)n_threads;
  return stateless(false, n_rows, n_cols, col_ptrs, row_indices, values, X, Y, nullptr, cnt_X, rank, lambda, solver, cg_steps,
                   dynamic_lambda, loss_out, with_biases, is_x_bias_last_row);
}

}  // extern "C"
