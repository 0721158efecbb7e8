// C ABI of the fp64 device path (declared in include/rsparse_wrmf_hip.h, section 3) and the two stateless `*_double`
// drop-ins, which run through it: als_implicit_double / als_explicit_double (src/wrmf_implicit.cpp:5-14,
// src/wrmf_explicit.cpp:5-14) compute in double in the reference, and so do these.  Kernels: wrmf_f64.hip.
#include "../../include/rsparse_wrmf_hip.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

#include "wrmf_capi_common.h"

using namespace rsparse_hip;

struct rsparse_hip_csc_f64 {
  int n_rows = 0, n_cols = 0;
  int64_t nnz = 0;
  const int32_t* col_ptrs = nullptr;
  const int32_t* row_idx = nullptr;
  double* vals = nullptr;
  bool owns = false;
  int device = 0;
  // the rows the conjugate-gradient path cuts into chunks (wrmf_f64.hip, "long rows"): listed once, from the column pointers
  int long_min = 0x7fffffff, chunk_len = 0, n_long = 0, n_chunks = 0;
  int32_t* long_table = nullptr;   // device: long_rows [n_long] | long_chunk0 [n_long + 1] | chunk_long [n_chunks] | chunk_off [n_chunks]
  ~rsparse_hip_csc_f64() { if (long_table) (void)hipFree(long_table); }
};

namespace {

using CscGuardF64 = HandleGuard<rsparse_hip_csc_f64, rsparse_hip_csc_f64_destroy>;

constexpr size_t kRhsInitDoubles = (size_t)256 * 128 + 128;

// Rows of more than g_long_row_min non-zeros leave the wave-per-row kernel (a 2048-row is 128 batches x 5 passes ~ 1 ms of one wave; the
// longest row of the 1M x 100k timing matrix, 154 k, was 58-80 ms); rsparse_hip_set_f64_long_rows changes the two lengths for the
// handles made afterwards (tests: small matrices)
constexpr int kF64LongRowMin = 2048, kF64LongRowChunk = 1024;
int g_long_row_min = kF64LongRowMin, g_long_row_chunk = kF64LongRowChunk;

int list_long_rows(rsparse_hip_csc_f64& m, const int32_t* host_col_ptrs) {
  const int lmin = g_long_row_min, chunk = g_long_row_chunk;
  m.long_min = lmin; m.chunk_len = chunk; m.n_long = m.n_chunks = 0;
  std::vector<int32_t> rows, chunk0, cl, co;
  for (int c = 0; c < m.n_cols; c++) {
    const int n = host_col_ptrs[(size_t)c + 1] - host_col_ptrs[(size_t)c];
    if (n <= lmin) continue;
    chunk0.push_back((int32_t)cl.size());
    for (int off = 0; off < n; off += chunk) {
      cl.push_back((int32_t)rows.size());
      co.push_back(off);
    }
    rows.push_back(c);
  }
  if (rows.empty()) return RSPARSE_HIP_OK;
  chunk0.push_back((int32_t)cl.size());
  std::vector<int32_t> all;
  all.reserve(rows.size() + chunk0.size() + 2 * cl.size());
  all.insert(all.end(), rows.begin(), rows.end());
  all.insert(all.end(), chunk0.begin(), chunk0.end());
  all.insert(all.end(), cl.begin(), cl.end());
  all.insert(all.end(), co.begin(), co.end());
  HIP_TRY(hipMalloc(&m.long_table, all.size() * sizeof(int32_t)));
  HIP_TRY(hipMemcpy(m.long_table, all.data(), all.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  m.n_long = (int)rows.size();
  m.n_chunks = (int)cl.size();
  return RSPARSE_HIP_OK;
}

// grow-only scratch of the fp64 path (one host thread drives the library, as in wrmf_capi.cpp)
struct WorkspaceF64 {
  GrowBufBase* all = nullptr;
  GrowBuf<double> gram{all};
  GrowBuf<double> partials{all};   // per-workgroup loss terms + the tail of the two-stage sum
  GrowBuf<double> scalars{all};    // [0] loss rows, [1] sumsq, [2], [3] sums of the bias sweeps
  GrowBuf<double> rinit{all};      // 256 x 128 partials + the k1 entries of rhs_init
  GrowBuf<double> m2{all};
  GrowBuf<double> longs{all};      // the long rows' partial sums and vectors (f64_long_scratch_doubles)
  GrowBuf<double> repack{all};     // explicit feedback with biases, conjugate gradient: X', Y', shifted ratings
  GrowBuf<double> score{all};      // pointwise predictions (wrmf_score.hip): the scores of a call that asks for the error sums only;
                                   // top-k within candidate lists (wrmf_candidates.hip): its scores / keys, bits and row lists
  GrowBuf<double> softals{all};    // soft-ALS half-iteration (wrmf_softals.hip): w, s, t and the partial sums of split rows
  int device = -1;
  int ensure() {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != device) {
      GrowBufBase::release_all(all);
      device = dev;
    }
    HIP_TRY(partials.ensure((size_t)std::max(kF64MaxGrid, 1024) + kSumStageBlocks + 16));
    if (!scalars) {
      HIP_TRY(scalars.ensure(16));
      HIP_TRY(hipMemset(scalars, 0, 16 * sizeof(double)));
      HIP_TRY(hipStreamSynchronize(nullptr));   // (the null stream does not order a caller's non-blocking stream: wrmf_capi.cpp, ensure_device)
    }
    HIP_TRY(rinit.ensure(kRhsInitDoubles));
    return RSPARSE_HIP_OK;
  }
  SumScratch scratch() const { return {partials, scalars}; }   // (for the bodies of wrmf_capi_common.h, after ensure())
} g_w64;

// One half-iteration in double.  d_base_in / d_base_out: global_bias_base of the no-bias global-bias variant (`rank`
// doubles; in = use it instead of recomputing -global_bias * rowSums(X), out = receives what was used), both nullable.
int f64_half_iteration(const rsparse_hip_csc_f64* conf, bool implicit, const double* d_X, double* d_Y, const double* d_XtX,
                       int rank, double lambda, unsigned solver, unsigned cg_steps, int dynamic_lambda, int with_biases,
                       int is_x_bias_last_row, double global_bias, const double* d_base_in, double* d_base_out,
                       double* d_loss_rows_out, hipStream_t s) {
  if (!conf) return fail(RSPARSE_HIP_ERR_INVALID, "conf is NULL");
  if (!d_X || !d_Y) return fail(RSPARSE_HIP_ERR_INVALID, "X or Y is NULL");
  if (implicit && !d_XtX) return fail(RSPARSE_HIP_ERR_INVALID, "XtX is NULL");
  if (rank <= 0) return fail(RSPARSE_HIP_ERR_INVALID, "rank must be positive");
  if (rank > RSPARSE_HIP_MAX_RANK_F64) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "rank > 128 is not on the fp64 device path");
  if (solver > RSPARSE_SOLVER_NNLS) return fail(RSPARSE_HIP_ERR_INVALID, "unknown solver code");
  if (with_biases && rank < 2) return fail(RSPARSE_HIP_ERR_INVALID, "with_biases needs rank >= 2 (a row of ones and a bias row)");
  if (with_biases && implicit && solver == RSPARSE_SOLVER_CONJUGATE_GRADIENT)
    // the reference drops a row of the warm start twice on this path (wrmf_implicit.hpp:189,197) and cannot run it
    return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "with_user_item_bias + conjugate_gradient with implicit feedback is not on the device path");
  int rc = g_w64.ensure();
  if (rc) return rc;
  int* fails = capi_fail_counters();
  if (!fails) return RSPARSE_HIP_ERR_RUNTIME;
  double* out = d_loss_rows_out ? d_loss_rows_out : g_w64.scalars;
  if (conf->n_cols == 0) {
    HIP_TRY(hipMemsetAsync(out, 0, sizeof(double), s));
    return RSPARSE_HIP_OK;
  }
  // wrmf_implicit.hpp:108-109: a global bias below sqrt(eps) of the element type counts as zero (double: 1.49e-8)
  const double gb = (implicit && global_bias >= std::sqrt(DBL_EPSILON)) ? global_bias : 0.0;
  F64Args a;
  a.col_ptrs = conf->col_ptrs; a.row_idx = conf->row_idx; a.vals = conf->vals;
  a.X = d_X; a.Y = d_Y; a.XtX = implicit ? d_XtX : nullptr;
  a.n_cols = conf->n_cols; a.k = rank; a.k1 = with_biases ? rank - 1 : rank;
  a.xoff = with_biases ? (is_x_bias_last_row ? 0 : 1) : 0;            // first kept row of X_nnz         (:88 / :188)
  a.xb = with_biases ? (is_x_bias_last_row ? rank - 1 : 0) : -1;      // row of X holding the x biases   (:59-64 / :116-120)
  a.ioff = with_biases ? (is_x_bias_last_row ? 1 : 0) : 0;            // drop_row(init, !is_x_bias_last_row)
  a.ooff = with_biases ? (is_x_bias_last_row ? 0 : 1) : 0;            // head / tail of Y.col(i)
  a.implicit = implicit ? 1 : 0; a.solver = (int)solver; a.cg_steps = (int)cg_steps;
  a.lambda = lambda; a.dynamic_lambda = dynamic_lambda ? 1 : 0;
  a.gbias = gb;
  a.rhs_init = nullptr;
  a.solve_empty = (implicit && (with_biases || gb != 0.0)) ? 1 : 0;   // wrmf_implicit.hpp:178
  double* rinit = g_w64.rinit + (kRhsInitDoubles - 128);
  hipError_t e;
  if (implicit && with_biases) {        // rhs_init = -X' (x_b + global_bias)  (:142-153)
    if ((e = launch_f64_rhs_init(d_X, rank, a.xoff, a.k1, a.xb, gb, conf->n_rows, g_w64.rinit, rinit, s)) != hipSuccess)
      return hip_fail(e, "launch_f64_rhs_init");
    a.rhs_init = rinit;
  } else if (gb != 0.0) {               // global_bias_base = -global_bias * rowSums(X)  (:110-112, :155-157)
    if (d_base_in) {
      HIP_TRY(hipMemcpyAsync(rinit, d_base_in, (size_t)rank * sizeof(double), hipMemcpyDeviceToDevice, s));
    } else if ((e = launch_f64_rhs_init(d_X, rank, 0, rank, -1, gb, conf->n_rows, g_w64.rinit, rinit, s)) != hipSuccess) {
      return hip_fail(e, "launch_f64_rhs_init");
    }
    if (d_base_out) HIP_TRY(hipMemcpyAsync(d_base_out, rinit, (size_t)rank * sizeof(double), hipMemcpyDeviceToDevice, s));
    a.rhs_init = rinit;
  }
  const int grid = f64_als_grid(conf->n_cols);
  a.loss_partials = g_w64.partials;
  a.fail_counter = fails;
  a.m2_scratch = nullptr;
  if (f64_needs_m2_scratch(a.k1, a.solver)) {
    HIP_TRY(g_w64.m2.ensure((size_t)grid * f64_m2_doubles_per_wg(a.k1)));
    a.m2_scratch = g_w64.m2;
  }
  a.long_min = 0x7fffffff; a.chunk_len = 0; a.n_long = a.n_chunks = 0;
  a.long_rows = a.long_chunk0 = a.chunk_long = a.chunk_off = nullptr;
  a.long_scratch = nullptr;
  if (conf->n_long > 0 && solver == RSPARSE_SOLVER_CONJUGATE_GRADIENT) {   // (only the wave-per-row path looks at these)
    HIP_TRY(g_w64.longs.ensure(f64_long_scratch_doubles(rank, conf->n_long, conf->n_chunks)));
    a.long_min = conf->long_min; a.chunk_len = conf->chunk_len; a.n_long = conf->n_long; a.n_chunks = conf->n_chunks;
    a.long_rows = conf->long_table;
    a.long_chunk0 = a.long_rows + conf->n_long;
    a.chunk_long = a.long_chunk0 + conf->n_long + 1;
    a.chunk_off = a.chunk_long + conf->n_chunks;
    a.long_scratch = g_w64.longs;
  }
  // explicit feedback with user/item biases and conjugate gradient -- the usual configuration of an explicit fit in the reference's
  // default precision -- re-packed for the wave-per-row kernels (end of round 6: it ran the generic kernel, 143 ms per iteration
  // at 1M x 100k and rank 10 where the float fit takes 10)
  const bool repack = !implicit && with_biases && solver == RSPARSE_SOLVER_CONJUGATE_GRADIENT && a.k1 >= 1;
  if (repack) {
    const int k1 = a.k1;
    const size_t nx = (size_t)conf->n_rows * k1, ny = (size_t)conf->n_cols * k1, nv = (size_t)conf->nnz;
    HIP_TRY(g_w64.repack.ensure(nx + ny + nv + 16));
    double* Xp = g_w64.repack;
    double* Yp = Xp + nx;
    double* Vp = Yp + ny;
    if ((e = launch_f64_pack_rows(d_X, rank, a.xoff, k1, conf->n_rows, Xp, s)) != hipSuccess) return hip_fail(e, "launch_f64_pack_rows");
    if ((e = launch_f64_pack_rows(d_Y, rank, a.ioff, k1, conf->n_cols, Yp, s)) != hipSuccess) return hip_fail(e, "launch_f64_pack_rows");
    if ((e = launch_f64_shift_values(conf->vals, conf->row_idx, d_X, rank, a.xb, conf->nnz, Vp, s)) != hipSuccess)
      return hip_fail(e, "launch_f64_shift_values");
    F64Args b = a;
    b.X = Xp; b.Y = Yp; b.vals = Vp;
    b.k = k1; b.k1 = k1;
    b.xoff = 0; b.xb = -1; b.ioff = 0; b.ooff = 0;
    if (conf->n_long > 0) {   // (the long rows' scratch was sized for `rank` coordinates: enough for k1)
      b.long_scratch = g_w64.longs;
    }
    if ((e = launch_f64_als(b, s)) != hipSuccess) return hip_fail(e, "launch_f64_als");
    if ((e = launch_f64_unpack_rows(Yp, k1, conf->n_cols, rank, a.ooff, d_Y, s)) != hipSuccess) return hip_fail(e, "launch_f64_unpack_rows");
  } else {
    if ((e = launch_f64_als(a, s)) != hipSuccess) return hip_fail(e, "launch_f64_als");
  }
  if ((e = launch_sum_partials(g_w64.partials, (size_t)grid, out, s)) != hipSuccess) return hip_fail(e, "launch_sum_partials");
  return RSPARSE_HIP_OK;
}

// Body of the two stateless `*_double` drop-ins: stateless_half_iteration on the matrix uploaded as it is.
int stateless_double(bool implicit, int n_rows, int n_cols, const int32_t* col_ptrs, const int32_t* row_indices,
                     const double* values, const double* X, double* Y, const double* XtX, const double* cnt_X, int rank,
                     double lambda, unsigned solver, unsigned cg_steps, int dynamic_lambda, double* loss_out,
                     int with_biases, int is_x_bias_last_row, double global_bias, double* global_bias_base,
                     int global_bias_base_len, int initialize_bias_base) {
  if (n_rows < 0 || n_cols < 0) return fail(RSPARSE_HIP_ERR_INVALID, "negative matrix dimension");
  if (!col_ptrs) return fail(RSPARSE_HIP_ERR_INVALID, "col_ptrs is NULL");
  if (!X || !Y) return fail(RSPARSE_HIP_ERR_INVALID, "X or Y is NULL");
  if (rank <= 0) return fail(RSPARSE_HIP_ERR_INVALID, "rank must be positive");
  if (rank > RSPARSE_HIP_MAX_RANK_F64) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "rank > 128 is not on the fp64 device path");
  if (solver > RSPARSE_SOLVER_NNLS) return fail(RSPARSE_HIP_ERR_INVALID, "unknown solver code");
  if (with_biases && implicit && solver == RSPARSE_SOLVER_CONJUGATE_GRADIENT)
    return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "with_user_item_bias + conjugate_gradient with implicit feedback is not on the device path");
  if (implicit && !XtX) return fail(RSPARSE_HIP_ERR_INVALID, "XtX is NULL");
  const int64_t nnz = (int64_t)col_ptrs[n_cols] - col_ptrs[0];
  if (col_ptrs[0] != 0 || nnz < 0) return fail(RSPARSE_HIP_ERR_INVALID, "col_ptrs must start at 0 and be non-decreasing");
  for (int c = 0; c < n_cols; c++)
    if (col_ptrs[c + 1] < col_ptrs[c]) return fail(RSPARSE_HIP_ERR_INVALID, "col_ptrs is not non-decreasing");
  if (nnz > 0 && (!row_indices || !values)) return fail(RSPARSE_HIP_ERR_INVALID, "row_indices or values is NULL");
  for (int64_t e = 0; e < nnz; e++)
    if (row_indices[e] < 0 || row_indices[e] >= n_rows) return fail(RSPARSE_HIP_ERR_INVALID, "row index out of range");
  DevBuf dP, dI, dV;
  HIP_TRY(upload_host(dP, col_ptrs, (size_t)n_cols + 1));
  HIP_TRY(upload_host(dI, row_indices, (size_t)nnz));
  HIP_TRY(upload_host(dV, values, (size_t)nnz));
  rsparse_hip_csc_f64 conf;
  conf.n_rows = n_rows; conf.n_cols = n_cols; conf.nnz = nnz;
  conf.col_ptrs = dP.as<int32_t>(); conf.row_idx = dI.as<int32_t>(); conf.vals = dV.as<double>();
  if (int rc = list_long_rows(conf, col_ptrs)) return rc;
  const bool use_base = implicit && !with_biases && global_bias >= std::sqrt(DBL_EPSILON);   // the threshold of double
  auto scratch = [](SumScratch& w) {
    int rc = g_w64.ensure();
    w = g_w64.scratch();
    return rc;
  };
  auto half = [&](const double* dX, double* dY, const double* dG, const double* base_in, double* base_out, double* d_loss) {
    return f64_half_iteration(&conf, implicit, dX, dY, dG, rank, lambda, solver, cg_steps, dynamic_lambda, with_biases,
                              is_x_bias_last_row, global_bias, base_in, base_out, d_loss, nullptr);
  };
  return stateless_half_iteration(scratch, half, implicit, n_rows, n_cols, nnz, X, Y, XtX, cnt_X, rank, lambda, dynamic_lambda,
                                  loss_out, with_biases, is_x_bias_last_row, use_base, global_bias_base, global_bias_base_len,
                                  initialize_bias_base);
}

}  // namespace

extern "C" {

int rsparse_hip_csc_f64_create_device(int n_rows, int n_cols, const int32_t* d_col_ptrs, const int32_t* d_row_indices,
                                      const double* d_values, rsparse_hip_csc_f64** out) {
  if (!out) return fail(RSPARSE_HIP_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (n_rows < 0 || n_cols < 0) return fail(RSPARSE_HIP_ERR_INVALID, "negative matrix dimension");
  if (!d_col_ptrs) return fail(RSPARSE_HIP_ERR_INVALID, "col_ptrs is NULL");
  std::vector<int32_t> hp((size_t)n_cols + 1);
  HIP_TRY(hipMemcpy(hp.data(), d_col_ptrs, hp.size() * 4, hipMemcpyDeviceToHost));
  if (hp[0] != 0) return fail(RSPARSE_HIP_ERR_INVALID, "col_ptrs must start at 0");
  for (int c = 0; c < n_cols; c++)
    if (hp[(size_t)c + 1] < hp[(size_t)c]) return fail(RSPARSE_HIP_ERR_INVALID, "col_ptrs must be non-decreasing");
  const int64_t nnz = hp[(size_t)n_cols];
  if (nnz > 0 && (!d_row_indices || !d_values)) return fail(RSPARSE_HIP_ERR_INVALID, "row_indices or values is NULL");
  int bad = 0;   // the kernels gather X[row_index] unchecked
  HIP_TRY(check_row_indices_device(d_row_indices, nnz, n_rows, nullptr, &bad));
  if (bad) return fail(RSPARSE_HIP_ERR_INVALID, "row index out of range");
  rsparse_hip_csc_f64* m = new rsparse_hip_csc_f64();
  if (hipGetDevice(&m->device) != hipSuccess) {
    delete m;
    return fail(RSPARSE_HIP_ERR_RUNTIME, "no HIP device");
  }
  m->n_rows = n_rows; m->n_cols = n_cols; m->nnz = nnz;
  m->col_ptrs = d_col_ptrs; m->row_idx = d_row_indices; m->vals = const_cast<double*>(d_values);
  if (int rc = list_long_rows(*m, hp.data())) {
    delete m;
    return rc;
  }
  *out = m;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_set_f64_long_rows(int min_len, int chunk_len) {
  if (min_len < 0 || chunk_len < 0) return fail(RSPARSE_HIP_ERR_INVALID, "lengths must be positive (0 = the default)");
  g_long_row_min = min_len > 0 ? min_len : kF64LongRowMin;
  g_long_row_chunk = chunk_len > 0 ? chunk_len : kF64LongRowChunk;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_csc_f64_destroy(rsparse_hip_csc_f64* m) {
  delete m;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_gramian_f64_device(const double* d_X, int rank, int64_t n, double lambda, double* d_XtX_out,
                                   double* d_sumsq_out, void* stream) {
  if ((!d_X && n != 0) || !d_XtX_out) return fail(RSPARSE_HIP_ERR_INVALID, "X or XtX_out is NULL");   // (n = 0: X is never read)
  if (rank <= 0 || n < 0) return fail(RSPARSE_HIP_ERR_INVALID, "rank must be positive and n non-negative");
  if (rank > RSPARSE_HIP_MAX_RANK_F64) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "rank > 128 is not on the fp64 device path");
  int rc = g_w64.ensure();
  if (rc) return rc;
  HIP_TRY(g_w64.gram.ensure(f64_gramian_scratch_doubles(rank)));
  const double ridge = (double)(float)lambda;   // float::fl(diag(lambda)): rounded to fp32 in the double build too, R/model_WRMF.R:476
  hipError_t e = launch_f64_gramian(d_X, rank, n, ridge, d_XtX_out, d_sumsq_out, g_w64.gram, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "launch_f64_gramian");
  return RSPARSE_HIP_OK;
}

int rsparse_hip_gramian_double(const double* X, int rank, int64_t n, double lambda, double* XtX_out) {
  return gramian_host(X, rank, n, XtX_out, [&](const double* dX, double* dG) {
    return rsparse_hip_gramian_f64_device(dX, rank, n, lambda, dG, nullptr, nullptr);
  });
}

int rsparse_hip_als_f64_device(const rsparse_hip_csc_f64* conf, int implicit, const double* d_X, double* d_Y,
                               const double* d_XtX, int rank, double lambda, unsigned solver, unsigned cg_steps,
                               int dynamic_lambda, int with_biases, int is_x_bias_last_row, double global_bias,
                               double* d_loss_rows_out, void* stream) {
  return f64_half_iteration(conf, implicit != 0, d_X, d_Y, d_XtX, rank, lambda, solver, cg_steps, dynamic_lambda,
                            with_biases, is_x_bias_last_row, global_bias, nullptr, nullptr, d_loss_rows_out,
                            (hipStream_t)stream);
}

int rsparse_hip_weighted_sumsq_f64_device(const double* d_X, int rank, int64_t n, const double* d_w, double* d_out,
                                          void* stream) {
  if (!d_X || !d_out) return fail(RSPARSE_HIP_ERR_INVALID, "X or out is NULL");
  if (rank <= 0 || n < 0) return fail(RSPARSE_HIP_ERR_INVALID, "rank must be positive and n non-negative");
  if (int rc = g_w64.ensure()) return rc;
  return weighted_sumsq(d_X, rank, n, d_w, d_out, g_w64.scratch(), (hipStream_t)stream);
}

// the cosine operands of rsparse_hip_similar_items_device from double factors (kernel: wrmf_similar.hip; the fp32 form:
// wrmf_capi.cpp, the argument rules: wrmf_capi_common.h)
int rsparse_hip_normalize_items_f64_device(const double* d_V, int n_items, int ld, int c0, int c1, float* d_Vn32,
                                           double* d_Vn64, int32_t* d_flags, void* stream) {
  int rc = normalize_items_args(d_V, n_items, ld, c0, c1, d_Vn32, d_Vn64, d_flags);
  if (rc || n_items == 0) return rc;
  hipError_t e = launch_normalize_items(d_V, true, n_items, ld, c0, c1 - c0, d_Vn32, d_Vn64, d_flags, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "launch_normalize_items");
  return RSPARSE_HIP_OK;
}

// pointwise predictions from double factors (kernels: wrmf_score.hip; the fp32 form: wrmf_capi.cpp)
int rsparse_hip_score_pairs_f64_device(const double* d_U, const double* d_V, int n_rows, int n_cols, int r, const int32_t* d_p,
                                       const int32_t* d_j, double add, const double* d_actual, double* d_scores, double* d_sse,
                                       double* d_sae, void* stream) {
  return score_pairs_device(d_U, d_V, n_rows, n_cols, r, d_p, d_j, add, d_actual, d_scores, d_sse, d_sae, (hipStream_t)stream,
                            [](size_t n, double*& buf) {
                              if (int rc = g_w64.ensure()) return rc;
                              HIP_TRY(g_w64.score.ensure(n));
                              buf = g_w64.score;
                              return (int)RSPARSE_HIP_OK;
                            });
}

// one soft-ALS half-iteration on double operands (kernels: wrmf_softals.hip; the fp32 form: wrmf_capi.cpp)
int rsparse_hip_softals_half_f64_device(const int32_t* d_p, const int32_t* d_j, const double* d_x, const double* d_M,
                                        const double* d_W, int n_rows, int n_cols, int r, const double* w, const double* s,
                                        const double* t, double* d_out, double* d_sumsq, void* stream) {
  return softals_half_device(d_p, d_j, d_x, d_M, d_W, n_rows, n_cols, r, w, s, t, d_out, d_sumsq, (hipStream_t)stream,
                             [](size_t n, double*& buf) {
                               if (int rc = g_w64.ensure()) return rc;
                               HIP_TRY(g_w64.softals.ensure(n));
                               buf = g_w64.softals;
                               return (int)RSPARSE_HIP_OK;
                             });
}

// top-k within per-user candidate lists from double factors (kernels: wrmf_score.hip, wrmf_candidates.hip; the fp32 form:
// wrmf_capi.cpp)
int rsparse_hip_top_candidates_f64_device(const double* d_U, const double* d_V, int n_users, int n_items, int rank, int k,
                                          const int32_t* d_cand_p, const int32_t* d_cand_j, const int32_t* d_nr_p,
                                          const int32_t* d_nr_j, const int32_t* d_excl0, int n_exclude, double glob_mean,
                                          int32_t* d_res, double* d_scores, void* stream) {
  return top_candidates_device(d_U, d_V, n_users, n_items, rank, k, d_cand_p, d_cand_j, d_nr_p, d_nr_j, d_excl0, n_exclude, glob_mean,
                               d_res, d_scores, (hipStream_t)stream, RSPARSE_HIP_MAX_RANK_F64, [](size_t n, double*& buf) {
                                 if (int rc = g_w64.ensure()) return rc;
                                 HIP_TRY(g_w64.score.ensure(n));
                                 buf = g_w64.score;
                                 return (int)RSPARSE_HIP_OK;
                               });
}

// per-item contributions to a score from double factors (kernel: wrmf_explain.hip; the fp32 form: wrmf_capi.cpp)
int rsparse_hip_explain_f64_device(const double* d_V, int n_items, int r, const double* d_base, double diag, double diag_per_nnz,
                                   int n_users, const int32_t* d_x_p, const int32_t* d_x_j, const double* d_wa, const double* d_wb,
                                   const int32_t* d_t_p, const int32_t* d_t_j, const int64_t* d_out_p, double* d_contrib,
                                   double* d_total, int32_t* d_flags, void* stream) {
  return explain_device(d_V, n_items, r, d_base, diag, diag_per_nnz, n_users, d_x_p, d_x_j, d_wa, d_wb, d_t_p, d_t_j, d_out_p,
                        d_contrib, d_total, d_flags, (hipStream_t)stream);
}

// initial factors in double (kernel: wrmf_init.hip; the fp32 form: wrmf_capi.cpp)
int rsparse_hip_init_factors_f64_device(uint64_t seed, int stream, int64_t row0, int n_rows, int rank, int64_t ld, double scale,
                                        int abs_values, int ones_col, void* d_out, void* hip_stream) {
  return init_factors_device(seed, stream, row0, n_rows, rank, ld, scale, abs_values, ones_col, static_cast<double*>(d_out),
                             (hipStream_t)hip_stream);
}

int rsparse_hip_values_subtract_mean_f64_device(int64_t n, double* d_x, double* d_x_other, double* mean_out, void* stream) {
  if (n < 0) return fail(RSPARSE_HIP_ERR_INVALID, "negative length");
  if (mean_out) *mean_out = 0.0;
  if (n == 0) return RSPARSE_HIP_OK;
  if (!d_x) return fail(RSPARSE_HIP_ERR_INVALID, "values is NULL");
  if (int rc = g_w64.ensure()) return rc;
  double mean = 0.0;
  if (int rc = subtract_mean(d_x, d_x_other, n, g_w64.scratch(), (hipStream_t)stream, &mean)) return rc;
  if (mean_out) *mean_out = mean;
  return RSPARSE_HIP_OK;
}

int rsparse_hip_bias_sweep_explicit_f64_device(const rsparse_hip_csc_f64* conf, const double* d_other_bias, double lambda,
                                               int dynamic_lambda, int non_negative, double* d_out, void* stream) {
  if (!conf || !d_other_bias || !d_out) return fail(RSPARSE_HIP_ERR_INVALID, "NULL matrix or bias vector");
  return bias_sweep_explicit(CscView<double>(*conf), d_other_bias, lambda, dynamic_lambda, non_negative, d_out,
                             (hipStream_t)stream);
}

int rsparse_hip_bias_prep_implicit_f64_device(const rsparse_hip_csc_f64* conf, int n_other, double lambda, double* d_means,
                                              double* d_adj, void* stream) {
  if (!conf || !d_means || !d_adj) return fail(RSPARSE_HIP_ERR_INVALID, "NULL matrix or output");
  return bias_prep_implicit(CscView<double>(*conf), n_other, lambda, d_means, d_adj, (hipStream_t)stream);
}

int rsparse_hip_bias_sweep_implicit_f64_device(const rsparse_hip_csc_f64* conf, const double* d_other_bias, int n_other,
                                               const double* d_other_sum, const double* d_means, const double* d_adj,
                                               int non_negative, double global_bias, double* d_out, void* stream) {
  if (!conf || !d_other_bias || !d_means || !d_adj || !d_out) return fail(RSPARSE_HIP_ERR_INVALID, "NULL matrix or vector");
  return bias_sweep_implicit(CscView<double>(*conf), d_other_bias, n_other, d_other_sum, d_means, d_adj, non_negative,
                             global_bias, d_out, (hipStream_t)stream);
}

int rsparse_hip_initialize_biases_f64_device(rsparse_hip_csc_f64* c_ui, rsparse_hip_csc_f64* c_iu, double* d_user_bias,
                                             double* d_item_bias, double lambda, int dynamic_lambda, int non_negative,
                                             int calculate_global_bias, int is_explicit_feedback,
                                             double* global_bias_out, void* stream) {
  if (!c_ui || !c_iu || !d_user_bias || !d_item_bias) return fail(RSPARSE_HIP_ERR_INVALID, "NULL matrix or bias vector");
  const CscView<double> a(*c_ui), b(*c_iu);   // users x items (columns = items), items x users (columns = users)
  if (a.n_rows != b.n_cols || a.n_cols != b.n_rows || a.nnz != b.nnz)
    return fail(RSPARSE_HIP_ERR_INVALID, "the two matrices are not transposes of each other");
  if (int rc = g_w64.ensure()) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (is_explicit_feedback)
    return initialize_biases_explicit(a, b, d_user_bias, d_item_bias, lambda, dynamic_lambda, non_negative,
                                      calculate_global_bias, g_w64.scratch(), s, global_bias_out);
  return initialize_biases_implicit(a, b, d_user_bias, d_item_bias, lambda, non_negative, calculate_global_bias,
                                    g_w64.scratch(), s, global_bias_out);
}

int rsparse_hip_als_implicit_double(int n_rows, int n_cols, const int32_t* col_ptrs, const int32_t* row_indices,
                                    const double* values, const double* X, double* Y, const double* XtX, int rank,
                                    double lambda, int n_threads, unsigned solver, unsigned cg_steps,
                                    int with_biases, int is_x_bias_last_row, double global_bias,
                                    double* global_bias_base, int global_bias_base_len, int initialize_bias_base,
                                    double* loss_out) {
  (void)n_threads;
  return stateless_double(true, n_rows, n_cols, col_ptrs, row_indices, values, X, Y, XtX, nullptr, rank, lambda, solver,
                          cg_steps, 0, loss_out, with_biases, is_x_bias_last_row, global_bias, global_bias_base,
                          global_bias_base_len, initialize_bias_base);
}

int rsparse_hip_als_explicit_double(int n_rows, int n_cols, const int32_t* col_ptrs, const int32_t* row_indices,
                                    const double* values, const double* X, double* Y, const double* cnt_X, int rank,
                                    double lambda, unsigned n_threads, unsigned solver, unsigned cg_steps,
                                    int dynamic_lambda, int with_biases, int is_x_bias_last_row, double* loss_out) {
  (void)n_threads;
  return stateless_double(false, n_rows, n_cols, col_ptrs, row_indices, values, X, Y, nullptr, cnt_X, rank, lambda, solver,
                          cg_steps, dynamic_lambda, loss_out, with_biases, is_x_bias_last_row, 0.0, nullptr, 0, 1);
}

// replaces initialize_biases_double (src/wrmf_init.cpp:5-19): the bias vectors, the values and every sum in double
int rsparse_hip_initialize_biases_double(int n_users, int n_items, const int32_t* csc_p, const int32_t* csc_i,
                                         double* csc_x, const int32_t* csr_p, const int32_t* csr_i, double* csr_x,
                                         double* user_bias, double* item_bias, double lambda, int dynamic_lambda,
                                         int non_negative, int calculate_global_bias, int is_explicit_feedback,
                                         double* global_bias_out) {
  if (!user_bias || !item_bias) return fail(RSPARSE_HIP_ERR_INVALID, "user_bias or item_bias is NULL");
  if (n_users < 0 || n_items < 0 || !csc_p || !csr_p) return fail(RSPARSE_HIP_ERR_INVALID, "bad matrix");
  const int64_t nnz = csc_p[n_items];
  if (csr_p[n_users] != nnz) return fail(RSPARSE_HIP_ERR_INVALID, "the two matrices are not transposes of each other");
  if (nnz > 0 && (!csc_i || !csc_x || !csr_i || !csr_x)) return fail(RSPARSE_HIP_ERR_INVALID, "NULL index or value array");
  DevBuf p1, i1, x1, p2, i2, x2;
  HIP_TRY(upload_host(p1, csc_p, (size_t)n_items + 1)); HIP_TRY(upload_host(i1, csc_i, (size_t)nnz)); HIP_TRY(upload_host(x1, csc_x, (size_t)nnz));
  HIP_TRY(upload_host(p2, csr_p, (size_t)n_users + 1)); HIP_TRY(upload_host(i2, csr_i, (size_t)nnz)); HIP_TRY(upload_host(x2, csr_x, (size_t)nnz));
  rsparse_hip_csc_f64 *c_ui = nullptr, *c_iu = nullptr;
  int rc = rsparse_hip_csc_f64_create_device(n_users, n_items, p1.as<int32_t>(), i1.as<int32_t>(), x1.as<double>(), &c_ui);
  if (rc) return rc;
  CscGuardF64 g1{c_ui};
  if ((rc = rsparse_hip_csc_f64_create_device(n_items, n_users, p2.as<int32_t>(), i2.as<int32_t>(), x2.as<double>(), &c_iu)))
    return rc;
  CscGuardF64 g2{c_iu};
  double gb = 0.0;
  rc = with_device_biases(n_users, n_items, user_bias, item_bias, [&](double* dU, double* dI) {
    return rsparse_hip_initialize_biases_f64_device(c_ui, c_iu, dU, dI, lambda, dynamic_lambda, non_negative,
                                                    calculate_global_bias, is_explicit_feedback, &gb, nullptr);
  });
  if (rc) return rc;
  if (is_explicit_feedback && calculate_global_bias && nnz) {
    // the reference removes the global mean from the @x slots of BOTH matrices in place (wrmf_utils.hpp:41-52): the resident
    // values are those doubles, so they are downloaded as the device left them
    HIP_TRY(hipMemcpy(csc_x, x1.p, (size_t)nnz * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(csr_x, x2.p, (size_t)nnz * 8, hipMemcpyDeviceToHost));
  }
  if (global_bias_out) *global_bias_out = gb;
  return RSPARSE_HIP_OK;
}

}  // extern "C"
