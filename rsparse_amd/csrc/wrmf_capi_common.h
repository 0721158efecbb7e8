// What the translation units of the C ABI share, each thing written once:
//   * the host bodies of the entries that exist in float and in double (wrmf_capi.cpp and wrmf_f64_capi.cpp hold the thin
//     `extern "C"` forms: validate, make sure of their own workspace, build the views below, call the template); what differs
//     between the two sides on purpose is listed in DESIGN.md ("shared between the precisions");
//   * the argument rules (`*_args`) of the evaluation and data-preparation entries, which the `_device` form of an entry
//     (wrmf_capi.cpp) and its host-array form (wrmf_capi_host.cpp) both apply first;
//   * the error helpers and upload_host, all that the host-array forms use besides DevBuf and the public `_device` entries.
#pragma once

#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/rsparse_wrmf_hip.h"
#include "wrmf_f64.h"
#include "wrmf_internal.h"

namespace rsparse_hip {

inline int fail(int code, const std::string& msg) { return capi_fail(code, msg); }
inline int hip_fail(hipError_t e, const char* what) { return capi_hip_fail(e, what); }
#define HIP_TRY(expr)                                       \
  do {                                                      \
    hipError_t _e = (expr);                                 \
    if (_e != hipSuccess) return hip_fail(_e, #expr);       \
  } while (0)

// the two launchers whose names differ by an `f64_` infix, as overloads (the float forms: wrmf_internal.h)
inline hipError_t launch_weighted_sumsq(const double* X, int k, int64_t n, const double* w, double* out, double* partials,
                                        hipStream_t s) {
  return launch_f64_weighted_sumsq(X, k, n, w, out, partials, s);
}
template <class T>
constexpr const char* weighted_sumsq_name() {   // (what the error text of each side has always said)
  return std::is_same<T, double>::value ? "launch_f64_weighted_sumsq" : "launch_weighted_sumsq";
}

// a handle released at the end of a scope (H: rsparse_hip_csc / rsparse_hip_csc_f64); `c = nullptr` keeps it
template <class H, int (*Destroy)(H*)>
struct HandleGuard {
  H* c;
  ~HandleGuard() { if (c) Destroy(c); }
};

// A device CSC as the bodies below see it: from rsparse_hip_csc::d (T = float) or from rsparse_hip_csc_f64 (T = double).
// Only subtract_mean writes through `vals`.
template <class T>
struct CscView {
  int n_rows, n_cols;
  int64_t nnz;
  const int32_t* col_ptrs;
  const int32_t* row_idx;
  T* vals;
  template <class M>
  explicit CscView(const M& m)
      : n_rows(m.n_rows), n_cols(m.n_cols), nnz(m.nnz), col_ptrs(m.col_ptrs), row_idx(m.row_idx), vals(const_cast<T*>(m.vals)) {}
};

// the sum scratch of a workspace, after its own ensure...() call: `partials` >= 1024 + kSumStageBlocks doubles, `scalars` 16
// doubles ([0] loss rows, [1] sumsq, [2], [3] sums of the bias sweeps)
struct SumScratch {
  double* partials;
  double* scalars;
};

// mean(x) out of x and (if given) x_other, n entries each: sum -> subtract from both -> read the sum back
template <class T>
int subtract_mean(T* x, T* x_other, int64_t n, SumScratch w, hipStream_t s, double* mean_out) {
  hipError_t e = launch_values_sum(x, n, w.partials, w.scalars + 2, s);
  if (e != hipSuccess) return hip_fail(e, "launch_values_sum");
  const double inv = 1.0 / (double)n;
  if ((e = launch_values_subtract_mean(x, n, w.scalars + 2, inv, s)) != hipSuccess)
    return hip_fail(e, "launch_values_subtract_mean");
  if (x_other && (e = launch_values_subtract_mean(x_other, n, w.scalars + 2, inv, s)) != hipSuccess)
    return hip_fail(e, "launch_values_subtract_mean");
  double sum = 0.0;
  HIP_TRY(hipMemcpyAsync(&sum, w.scalars + 2, sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *mean_out = sum * inv;
  return RSPARSE_HIP_OK;
}

// ---- single sweeps of the bias initialisation over ONE column block (sharded drivers; see the header) ----
template <class T>
int bias_sweep_explicit(CscView<T> a, const T* d_other_bias, T lambda, int dynamic_lambda, int non_negative, T* d_out,
                        hipStream_t s) {
  hipError_t e = launch_bias_sweep(a.col_ptrs, a.row_idx, a.vals, d_other_bias, a.n_cols, lambda, dynamic_lambda, non_negative,
                                   d_out, s);
  if (e != hipSuccess) return hip_fail(e, "launch_bias_sweep");
  return RSPARSE_HIP_OK;
}

template <class T>
int bias_prep_implicit(CscView<T> a, int n_other, double lambda, double* d_means, double* d_adj, hipStream_t s) {
  hipError_t e = launch_bias_implicit_prep(a.col_ptrs, a.vals, a.n_cols, n_other, lambda, d_means, d_adj, s);
  if (e != hipSuccess) return hip_fail(e, "launch_bias_implicit_prep");
  return RSPARSE_HIP_OK;
}

template <class T>
int bias_sweep_implicit(CscView<T> a, const T* d_other_bias, int n_other, const double* d_other_sum, const double* d_means,
                        const double* d_adj, int non_negative, double global_bias, T* d_out, hipStream_t s) {
  hipError_t e = launch_bias_implicit_sweep(a.col_ptrs, a.row_idx, a.vals, d_other_bias, a.n_cols, n_other, d_other_sum, d_means,
                                            d_adj, non_negative, global_bias, d_out, s);
  if (e != hipSuccess) return hip_fail(e, "launch_bias_implicit_sweep");
  return RSPARSE_HIP_OK;
}

// initialize_biases_explicit, wrmf_utils.hpp:32-84.  a: users x items, columns = items; b: items x users, columns = users
template <class T>
int initialize_biases_explicit(CscView<T> a, CscView<T> b, T* d_user_bias, T* d_item_bias, T lambda, int dynamic_lambda,
                               int non_negative, int calculate_global_bias, SumScratch w, hipStream_t s,
                               double* global_bias_out) {
  double global_bias = 0.0;
  if (calculate_global_bias && a.nnz > 0)   // :41-52: mean of the values, removed from both orientations in place
    if (int rc = subtract_mean(a.vals, b.vals, a.nnz, w, s, &global_bias)) return rc;
  for (int iter = 0; iter < 5; iter++) {    // :54-82
    if (int rc = bias_sweep_explicit(a, d_user_bias, lambda, dynamic_lambda, non_negative, d_item_bias, s)) return rc;
    if (int rc = bias_sweep_explicit(b, d_item_bias, lambda, dynamic_lambda, non_negative, d_user_bias, s)) return rc;
  }
  if (global_bias_out) *global_bias_out = global_bias;
  return RSPARSE_HIP_OK;
}

// initialize_biases_implicit, wrmf_utils.hpp:86-165 (a, b as above)
template <class T>
int initialize_biases_implicit(CscView<T> a, CscView<T> b, T* d_user_bias, T* d_item_bias, double lambda, int non_negative,
                               int calculate_global_bias, SumScratch w, hipStream_t s, double* global_bias_out) {
  const int n_items = a.n_cols, n_users = b.n_cols;
  DevBuf stats;   // means / adjustments of both sides (:97-124), doubles
  HIP_TRY(stats.alloc(((size_t)2 * n_items + (size_t)2 * n_users + 4) * sizeof(double)));
  double* item_means = stats.as<double>();
  double* item_adj = item_means + n_items;
  double* user_means = item_adj + n_items;
  double* user_adj = user_means + n_users;
  int rc;
  if ((rc = bias_prep_implicit(a, n_users, lambda, item_means, item_adj, s))) return rc;
  if ((rc = bias_prep_implicit(b, n_items, lambda, user_means, user_adj, s))) return rc;
  double global_bias = 0.0;
  hipError_t e;
  if (calculate_global_bias) {   // :90-93: sum(x) / (sum(x) + n_users n_items - nnz)
    if ((e = launch_values_sum(a.vals, a.nnz, w.partials, w.scalars + 2, s)) != hipSuccess) return hip_fail(e, "launch_values_sum");
    double sum = 0.0;
    HIP_TRY(hipMemcpyAsync(&sum, w.scalars + 2, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    global_bias = sum / (sum + (double)n_users * (double)n_items - (double)a.nnz);
  }
  if (non_negative) global_bias = std::fmax(0.0, global_bias);
  if (global_bias_out) *global_bias_out = global_bias;
  for (int iter = 0; iter < 5; iter++) {   // :130-162
    const double* usum = nullptr;
    if (iter > 0) {                        // mean of the user biases of the previous sweep (:131-135)
      if ((e = launch_values_sum(d_user_bias, n_users, w.partials, w.scalars + 2, s)) != hipSuccess)
        return hip_fail(e, "launch_values_sum");
      usum = w.scalars + 2;
    }
    if ((rc = bias_sweep_implicit(a, d_user_bias, n_users, usum, item_means, item_adj, non_negative, global_bias, d_item_bias, s)))
      return rc;
    if ((e = launch_values_sum(d_item_bias, n_items, w.partials, w.scalars + 3, s)) != hipSuccess)
      return hip_fail(e, "launch_values_sum");
    if ((rc = bias_sweep_implicit(b, d_item_bias, n_items, w.scalars + 3, user_means, user_adj, non_negative, global_bias,
                                  d_user_bias, s)))
      return rc;
  }
  HIP_TRY(hipStreamSynchronize(s));   // `stats` is released on return
  return RSPARSE_HIP_OK;
}

// lambda-free part of the regularisation term: accu(X % X), each column times w if given
template <class T>
int weighted_sumsq(const T* d_X, int rank, int64_t n, const T* d_w, double* d_out, SumScratch w, hipStream_t s) {
  hipError_t e = launch_weighted_sumsq(d_X, rank, n, d_w, d_out, w.partials, s);
  if (e != hipSuccess) return hip_fail(e, weighted_sumsq_name<T>());
  return RSPARSE_HIP_OK;
}

// X'X + lambda I of a host matrix; device_gramian(d_X, d_G) is the side's resident entry
template <class T, class DeviceGramian>
int gramian_host(const T* X, int rank, int64_t n, T* XtX_out, DeviceGramian device_gramian) {
  if (!X || !XtX_out) return fail(RSPARSE_HIP_ERR_INVALID, "X or XtX_out is NULL");
  if (rank <= 0 || n < 0) return fail(RSPARSE_HIP_ERR_INVALID, "rank must be positive and n non-negative");
  DevBuf dX, dG;
  HIP_TRY(dX.alloc((size_t)rank * n * sizeof(T)));
  HIP_TRY(dG.alloc((size_t)rank * rank * sizeof(T)));
  if (n) HIP_TRY(hipMemcpy(dX.p, X, (size_t)rank * n * sizeof(T), hipMemcpyHostToDevice));
  int rc = device_gramian(dX.as<T>(), dG.as<T>());
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(XtX_out, dG.p, (size_t)rank * rank * sizeof(T), hipMemcpyDeviceToHost));
  return RSPARSE_HIP_OK;
}

template <class T>
hipError_t upload_host(DevBuf& b, const T* src, size_t n) {   // n host elements into a fresh buffer
  hipError_t e = b.alloc(n * sizeof(T));
  return (e != hipSuccess || !n) ? e : hipMemcpy(b.p, src, n * sizeof(T), hipMemcpyHostToDevice);
}

// ---- the argument rules of the evaluation and data-preparation entries: what the `_device` form (wrmf_capi.cpp) and the
// host-array form (wrmf_capi_host.cpp) of an entry both check before anything else, and before a pointer is read ----

// the refusal every top-k entry shares (k: a list length)
inline int refuse_large_k(int64_t k) {
  if (k > RSPARSE_HIP_MAX_TOPK_LARGE) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "k > 8192 (RSPARSE_HIP_MAX_TOPK_LARGE) is not on the device path");
  return RSPARSE_HIP_OK;
}

inline int similar_items_args(int n_items, int r, int n_q, int k, int n_exclude, const void* exclude) {
  if (n_items < 0 || n_q < 0 || k < 1 || r < 1) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_items < 0, n_q < 0, k < 1 or no latent coordinate)");
  if (n_exclude < 0 || (n_exclude > 0 && !exclude)) return fail(RSPARSE_HIP_ERR_INVALID, "bad exclude");
  if (r > RSPARSE_HIP_MAX_RANK) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "more than 256 latent coordinates are not on the device path");
  return refuse_large_k(k);
}

inline int ranking_metrics_args(const int32_t* pred, int n_users, int k, const int32_t* p, const int32_t* j, const double* x,
                                const double* ap_out, const double* ndcg_out) {
  if (!ap_out && !ndcg_out) return fail(RSPARSE_HIP_ERR_INVALID, "ap_out and ndcg_out are both NULL");
  if (!pred || !p || !j) return fail(RSPARSE_HIP_ERR_INVALID, "predictions or actual (p, j) is NULL");
  if (ndcg_out && !x) return fail(RSPARSE_HIP_ERR_INVALID, "ndcg needs the relevances: actual_x is NULL");
  if (n_users < 0 || k < 1) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_users < 0 or k < 1)");
  return refuse_large_k(k);
}

// The lists and cutoffs of the entries that take cutoffs.  What differs between the two families is handed in: whether a
// needed array is missing (and how the refusal names them), and whether n_items is bad for this call (likewise).
inline int cutoff_args(bool any_output, bool missing, const char* missing_msg, int n_users, int k, const int32_t* cutoffs,
                       int n_cutoffs, bool bad_items, const char* bad_items_msg) {
  if (!any_output) return fail(RSPARSE_HIP_ERR_INVALID, "every output is NULL");
  if (missing) return fail(RSPARSE_HIP_ERR_INVALID, missing_msg);
  if (n_users < 0 || k < 1 || n_cutoffs < 1)
    return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_users < 0, k < 1 or n_cutoffs < 1)");
  if (bad_items) return fail(RSPARSE_HIP_ERR_INVALID, bad_items_msg);
  if (n_cutoffs > RSPARSE_HIP_MAX_CUTOFFS)
    return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "more than 16 cutoffs (RSPARSE_HIP_MAX_CUTOFFS) are not on the device path");
  if (int rc = refuse_large_k(k)) return rc;
  for (int t = 0; t < n_cutoffs; t++)
    if (cutoffs[t] < 1 || cutoffs[t] > k || (t > 0 && cutoffs[t] <= cutoffs[t - 1]))
      return fail(RSPARSE_HIP_ERR_INVALID, "cutoffs must be strictly ascending within 1 .. k");
  return RSPARSE_HIP_OK;
}
inline int hit_metrics_args(const int32_t* pred, int n_users, int k, const int32_t* p, const int32_t* j, const int32_t* cutoffs,
                            int n_cutoffs, bool any_output, const int32_t* first_seen, int n_items) {
  return cutoff_args(any_output, !pred || !p || !j || !cutoffs, "predictions, actual (p, j) or cutoffs is NULL", n_users, k, cutoffs,
                     n_cutoffs, first_seen && n_items < 1, "first_seen needs n_items >= 1");
}
// (every entry of the beyond-accuracy metrics)
inline int list_args(const int32_t* pred, int n_users, int k, const int32_t* cutoffs, int n_cutoffs, bool any_output, int n_items) {
  return cutoff_args(any_output, !pred || !cutoffs, "predictions or cutoffs is NULL", n_users, k, cutoffs, n_cutoffs, n_items < 1,
                     "n_items < 1");
}
inline int list_metrics_args(const int32_t* pred, int n_users, int k, const int32_t* cutoffs, int n_cutoffs, const int32_t* item_count,
                             const int64_t* item_info, int n_items, const void* valid, const void* count_sum, const void* info_sum,
                             const void* popularity, const void* novelty, const void* exposure) {
  const bool any = valid || count_sum || info_sum || popularity || novelty || exposure;
  int rc = list_args(pred, n_users, k, cutoffs, n_cutoffs, any, n_items);
  if (rc) return rc;
  if ((count_sum || popularity) && !item_count) return fail(RSPARSE_HIP_ERR_INVALID, "count_sum / popularity need item_count");
  if ((info_sum || novelty) && !item_info) return fail(RSPARSE_HIP_ERR_INVALID, "info_sum / novelty need item_info");
  return RSPARSE_HIP_OK;
}
// the window c0 .. c1 of the factors' ld columns
inline int window_args(int n_items, int ld, int c0, int c1) {
  if (n_items < 0 || c0 < 0 || c1 - c0 < 1 || c1 > ld)
    return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_items < 0 or not 0 <= c0 < c1 <= ld)");
  if (c1 - c0 > RSPARSE_HIP_MAX_RANK)
    return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "more than 256 latent coordinates are not on the device path");
  return RSPARSE_HIP_OK;
}
// the cosine operands of the item-to-item similarity (rsparse_hip_normalize_items_device / _f64_device)
inline int normalize_items_args(const void* d_V, int n_items, int ld, int c0, int c1, const void* d_Vn32, const void* d_Vn64,
                                const void* d_flags) {
  if (int rc = window_args(n_items, ld, c0, c1)) return rc;
  if (n_items > 0 && (!d_V || !d_Vn32 || !d_Vn64 || !d_flags)) return fail(RSPARSE_HIP_ERR_INVALID, "NULL matrix or output");
  return RSPARSE_HIP_OK;
}
inline int list_diversity_args(const int32_t* pred, int n_users, int k, const int32_t* cutoffs, int n_cutoffs, const void* V, int n_items,
                               int ld, int c0, int c1, const void* counted, const void* diversity) {
  int rc = list_args(pred, n_users, k, cutoffs, n_cutoffs, counted || diversity, n_items);
  if (rc) return rc;
  if (!V) return fail(RSPARSE_HIP_ERR_INVALID, "the factor matrix is NULL");
  return window_args(n_items, ld, c0, c1);
}

inline int mmr_rerank_args(const int32_t* lists, const double* scores, int n_users, int n_pool, int k, double trade_off, const void* V,
                           int n_items, int ld, int c0, int c1, const void* items) {
  if (!lists || !scores) return fail(RSPARSE_HIP_ERR_INVALID, "lists or scores is NULL");
  if (!V) return fail(RSPARSE_HIP_ERR_INVALID, "the factor matrix is NULL");
  if (!items) return fail(RSPARSE_HIP_ERR_INVALID, "the items output is NULL");
  if (n_users < 0 || n_pool < 1 || k < 1 || k > n_pool)
    return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_users < 0 or not 1 <= k <= n_pool)");
  if (!(trade_off >= 0.0 && trade_off <= 1.0)) return fail(RSPARSE_HIP_ERR_INVALID, "trade_off must lie in [0, 1]");   // (NaN too)
  if (n_items < 1) return fail(RSPARSE_HIP_ERR_INVALID, "n_items < 1");
  if (n_pool > RSPARSE_HIP_MAX_TOPK_LARGE)
    return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "a pool of more than 8192 (RSPARSE_HIP_MAX_TOPK_LARGE) is not on the device path");
  return window_args(n_items, ld, c0, c1);
}

inline int held_out_ranks_args(const void* U, const void* V, int n_users, int n_items, int rank, int n_exclude, const void* excl,
                               const void* act_p, const void* act_j, int max_chunk_users) {
  if (n_users < 0 || n_items < 0 || rank < 1) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_users < 0, n_items < 0 or rank < 1)");
  if (max_chunk_users < 0) return fail(RSPARSE_HIP_ERR_INVALID, "max_chunk_users < 0");
  if (!U || !V || !act_p || !act_j) return fail(RSPARSE_HIP_ERR_INVALID, "NULL matrix or actual (p, j)");
  if (n_exclude < 0 || (n_exclude > 0 && !excl)) return fail(RSPARSE_HIP_ERR_INVALID, "bad exclude");
  if (rank > RSPARSE_HIP_MAX_RANK) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "rank > 256 is not on the device path");
  return RSPARSE_HIP_OK;
}

inline int sample_negatives_args(int64_t row0, int n_rows, int n_item, int n, const void* seen_p, const void* seen_j, const void* keep_p,
                                 const void* keep_j, const void* out_p, int64_t out_capacity) {
  if (n_rows < 0 || n_item < 0 || n < 1 || row0 < 0 || out_capacity < 0)
    return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_rows < 0, n_item < 0, n < 1, row0 < 0 or out_capacity < 0)");
  if (row0 + n_rows > (1ll << 32)) return fail(RSPARSE_HIP_ERR_INVALID, "the global row index row0 + n_rows does not fit 32 bits");
  if (!seen_p || !seen_j || !out_p) return fail(RSPARSE_HIP_ERR_INVALID, "seen_p, seen_j or out_p is NULL");
  if (!keep_p != !keep_j) return fail(RSPARSE_HIP_ERR_INVALID, "keep_p and keep_j must both be given or both be NULL");
  if (n > RSPARSE_HIP_MAX_NEGATIVES)
    return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "n > 8192 (RSPARSE_HIP_MAX_NEGATIVES) is not on the device path");
  return RSPARSE_HIP_OK;
}

inline int split_rows_args(int64_t row0, int n_rows, int mode, uint64_t test_threshold, int leave_out, int min_train, const void* p,
                           const void* j, const void* v, int value_bytes, const void* by, const void* train_p, const void* train_j,
                           const void* train_v, const void* test_p, const void* test_j, const void* test_v, int64_t train_capacity,
                           int64_t test_capacity) {
  if (n_rows < 0 || row0 < 0 || train_capacity < 0 || test_capacity < 0)
    return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_rows < 0, row0 < 0 or a negative capacity)");
  if (row0 + n_rows > (1ll << 32)) return fail(RSPARSE_HIP_ERR_INVALID, "the global row index row0 + n_rows does not fit 32 bits");
  if (!p || !j || !train_p || !test_p) return fail(RSPARSE_HIP_ERR_INVALID, "p, j, train_p or test_p is NULL");
  if (!train_j != !test_j) return fail(RSPARSE_HIP_ERR_INVALID, "train_j and test_j must both be given or both be NULL");
  if (mode == RSPARSE_HIP_SPLIT_PROPORTION) {
    if (test_threshold > (1ull << 32)) return fail(RSPARSE_HIP_ERR_INVALID, "test_threshold > 2^32");
    if (by) return fail(RSPARSE_HIP_ERR_INVALID, "`by` has no meaning in proportion mode");
  } else if (mode == RSPARSE_HIP_SPLIT_LEAVE_OUT) {
    if (leave_out < 1 || min_train < 0) return fail(RSPARSE_HIP_ERR_INVALID, "leave_out < 1 or min_train < 0");
  } else {
    return fail(RSPARSE_HIP_ERR_INVALID, "mode is neither RSPARSE_HIP_SPLIT_PROPORTION nor RSPARSE_HIP_SPLIT_LEAVE_OUT");
  }
  if (value_bytes != 0 && value_bytes != 4 && value_bytes != 8) return fail(RSPARSE_HIP_ERR_INVALID, "value_bytes must be 0, 4 or 8");
  if (!v != (value_bytes == 0)) return fail(RSPARSE_HIP_ERR_INVALID, "v and value_bytes must both be given or both be 0");
  if (v && train_j && (!train_v || !test_v)) return fail(RSPARSE_HIP_ERR_INVALID, "values are given: train_v and test_v must be too");
  return RSPARSE_HIP_OK;
}

inline int events_args(int64_t n_events, int n_users, int n_items, const void* users, const void* items, const void* timestamps,
                       int aggregate, double half_life, const void* p, const void* j, const void* x, int64_t capacity, const void* n_cells) {
  if (n_events < 0 || n_users < 0 || n_items < 0 || capacity < 0)
    return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_events < 0, n_users < 0, n_items < 0 or capacity < 0)");
  if (n_events >= (1ll << 31)) return fail(RSPARSE_HIP_ERR_INVALID, "n_events >= 2^31: cut the log into several calls");
  if (!p || !n_cells) return fail(RSPARSE_HIP_ERR_INVALID, "p or n_cells is NULL");
  if (n_events > 0 && (!users || !items || !j || !x)) return fail(RSPARSE_HIP_ERR_INVALID, "users, items, j or x is NULL");
  if (aggregate < RSPARSE_HIP_EVENTS_SUM || aggregate > RSPARSE_HIP_EVENTS_LAST)
    return fail(RSPARSE_HIP_ERR_INVALID, "unknown aggregate " + std::to_string(aggregate));
  if (aggregate == RSPARSE_HIP_EVENTS_LAST && !timestamps) return fail(RSPARSE_HIP_ERR_INVALID, "the aggregate `last` needs timestamps");
  if (half_life > 0.0 && !timestamps) return fail(RSPARSE_HIP_ERR_INVALID, "a half life needs timestamps");
  if (half_life > 0.0 && aggregate != RSPARSE_HIP_EVENTS_SUM) return fail(RSPARSE_HIP_ERR_INVALID, "a half life goes with the aggregate `sum` only");
  return RSPARSE_HIP_OK;
}

// ItemKNN: the neighbour table and the lists scored by it (both operand sets are named by the caller's form)
inline int cooc_neighbors_args(bool missing, int n_users, int n_items, int item0, int item1, int similarity, int K, int64_t ws_rows) {
  if (missing) return fail(RSPARSE_HIP_ERR_INVALID, "a pattern array or an output is NULL");
  if (n_users < 0 || n_items < 0) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_users < 0 or n_items < 0)");
  if (item0 < 0 || item1 < item0 || item1 > n_items) return fail(RSPARSE_HIP_ERR_INVALID, "not 0 <= item0 <= item1 <= n_items");
  if (similarity < RSPARSE_HIP_KNN_COUNT || similarity > RSPARSE_HIP_KNN_JACCARD)
    return fail(RSPARSE_HIP_ERR_INVALID, "unknown similarity " + std::to_string(similarity));
  if (K < 1) return fail(RSPARSE_HIP_ERR_INVALID, "K < 1");
  if (ws_rows < 0) return fail(RSPARSE_HIP_ERR_INVALID, "ws_rows < 0");
  if (K > RSPARSE_HIP_KNN_MAX_NEIGHBORS)
    return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "K > 256 (RSPARSE_HIP_KNN_MAX_NEIGHBORS) is not on the device path");
  if (n_users > RSPARSE_HIP_KNN_MAX_USERS)
    return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "n_users > 2^26 (RSPARSE_HIP_KNN_MAX_USERS): c^2 and n_i n_j would not be exact in double");
  return RSPARSE_HIP_OK;
}
// the weighted table: no similarity kind and no n_users limit (the caller's 2^53 bound replaces it), the key's h instead
inline int cooc_neighbors_weighted_args(bool missing, int n_users, int n_items, int item0, int item1, double h, int K, int64_t ws_rows) {
  if (missing) return fail(RSPARSE_HIP_ERR_INVALID, "a pattern array, an operand, a table or an output is NULL");
  if (n_users < 0 || n_items < 0) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_users < 0 or n_items < 0)");
  if (item0 < 0 || item1 < item0 || item1 > n_items) return fail(RSPARSE_HIP_ERR_INVALID, "not 0 <= item0 <= item1 <= n_items");
  if (K < 1) return fail(RSPARSE_HIP_ERR_INVALID, "K < 1");
  if (ws_rows < 0) return fail(RSPARSE_HIP_ERR_INVALID, "ws_rows < 0");
  if (!(h >= 0.0 && h <= 0x1p400)) return fail(RSPARSE_HIP_ERR_INVALID, "h is not finite or outside [0, 2^400]");   // (NaN fails both)
  if (K > RSPARSE_HIP_KNN_MAX_NEIGHBORS)
    return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "K > 256 (RSPARSE_HIP_KNN_MAX_NEIGHBORS) is not on the device path");
  return RSPARSE_HIP_OK;
}
inline int knn_recommend_args(bool missing, int n_rows, int n_items, int K, const void* nr_p, const void* nr_j, const void* excl,
                              int n_exclude, int k, int64_t ws_rows) {
  if (missing) return fail(RSPARSE_HIP_ERR_INVALID, "the pattern (x_p, x_j), a table or an output is NULL");
  if (n_rows < 0 || n_items < 0) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_rows < 0 or n_items < 0)");
  if (K < 1 || k < 1) return fail(RSPARSE_HIP_ERR_INVALID, "K < 1 or k < 1");
  if (ws_rows < 0) return fail(RSPARSE_HIP_ERR_INVALID, "ws_rows < 0");
  if (nr_p && !nr_j) return fail(RSPARSE_HIP_ERR_INVALID, "nr_p without nr_j");
  if (n_exclude < 0 || (n_exclude > 0 && !excl)) return fail(RSPARSE_HIP_ERR_INVALID, "bad exclude");
  if (K > RSPARSE_HIP_KNN_MAX_NEIGHBORS)
    return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "K > 256 (RSPARSE_HIP_KNN_MAX_NEIGHBORS) is not on the device path");
  if (k > RSPARSE_HIP_KNN_MAX_TOPK) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "k > 1024 (RSPARSE_HIP_KNN_MAX_TOPK) is not on the device path");
  return RSPARSE_HIP_OK;
}

// EASE: the Gram rows and the lists scored by a dense weight matrix
inline int item_gram_args(bool missing, int n_users, int n_items, int item0, int item1, double lambda, size_t ld_out, int64_t ws_rows) {
  if (missing) return fail(RSPARSE_HIP_ERR_INVALID, "a pattern array or the output is NULL");
  if (n_users < 0 || n_items < 0) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_users < 0 or n_items < 0)");
  if (item0 < 0 || item1 < item0 || item1 > n_items) return fail(RSPARSE_HIP_ERR_INVALID, "not 0 <= item0 <= item1 <= n_items");
  if (ws_rows < 0) return fail(RSPARSE_HIP_ERR_INVALID, "ws_rows < 0");
  if (ld_out < (size_t)n_items) return fail(RSPARSE_HIP_ERR_INVALID, "ld_out < n_items");
  if (!(lambda >= 0.0 && lambda <= 1.7976931348623157e308))   // (NaN fails both)
    return fail(RSPARSE_HIP_ERR_INVALID, "lambda is negative or not finite");
  if (n_items > RSPARSE_HIP_EASE_MAX_ITEMS)
    return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "n_items > 32768 (RSPARSE_HIP_EASE_MAX_ITEMS): an items x items matrix of doubles would pass 8 GiB");
  return RSPARSE_HIP_OK;
}
// B_elems: the alignment of B and ld_B in elements (16 bytes / the element size); 0 = B is a host array without a leading dimension
inline int ease_recommend_args(bool missing, int n_rows, int n_items, const void* B, size_t ld_B, size_t B_elems, const void* nr_p,
                               const void* nr_j, const void* excl, int n_exclude, int k, int64_t ws_rows) {
  if (missing) return fail(RSPARSE_HIP_ERR_INVALID, "the pattern (x_p, x_j), B or an output is NULL");
  if (n_rows < 0 || n_items < 0) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_rows < 0 or n_items < 0)");
  if (k < 1) return fail(RSPARSE_HIP_ERR_INVALID, "k < 1");
  if (ws_rows < 0) return fail(RSPARSE_HIP_ERR_INVALID, "ws_rows < 0");
  if (nr_p && !nr_j) return fail(RSPARSE_HIP_ERR_INVALID, "nr_p without nr_j");
  if (n_exclude < 0 || (n_exclude > 0 && !excl)) return fail(RSPARSE_HIP_ERR_INVALID, "bad exclude");
  if (B_elems && (ld_B < (size_t)n_items || ld_B % B_elems != 0 || (uintptr_t)B % 16 != 0))
    return fail(RSPARSE_HIP_ERR_INVALID, "ld_B < n_items, or ld_B or B is not a multiple of 16 bytes");
  if (k > RSPARSE_HIP_KNN_MAX_TOPK) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "k > 1024 (RSPARSE_HIP_KNN_MAX_TOPK) is not on the device path");
  if (n_items > RSPARSE_HIP_EASE_MAX_ITEMS)
    return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "n_items > 32768 (RSPARSE_HIP_EASE_MAX_ITEMS): an items x items matrix of doubles would pass 8 GiB");
  return RSPARSE_HIP_OK;
}

// SLIM: what both entries refuse.  W_elems: as B_elems above (0 = W is a host array without a leading dimension)
inline int slim_args(bool missing, int n_items, int n_cols, double l1, double l2, int max_iter, double tol, size_t ld_G, const void* W,
                     size_t ld_W, size_t W_elems) {
  const auto ok = [](double v) { return v >= 0.0 && v <= 1.7976931348623157e308; };   // (NaN fails both)
  if (missing) return fail(RSPARSE_HIP_ERR_INVALID, "G or the pattern, the columns, W or sweeps is NULL");
  if (n_items < 0 || n_cols < 0) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_items < 0, n_users < 0 or n_cols < 0)");
  if (!ok(l1) || !ok(l2)) return fail(RSPARSE_HIP_ERR_INVALID, "l1 or l2 is negative or not finite");
  if (!ok(tol)) return fail(RSPARSE_HIP_ERR_INVALID, "tol is negative or not finite");
  if (max_iter < 1) return fail(RSPARSE_HIP_ERR_INVALID, "max_iter < 1");
  if (ld_G < (size_t)n_items) return fail(RSPARSE_HIP_ERR_INVALID, "ld_G < n_items");
  if (W_elems && (ld_W < (size_t)n_items || ld_W % W_elems != 0 || (uintptr_t)W % 16 != 0))
    return fail(RSPARSE_HIP_ERR_INVALID, "ld_W < n_items, or ld_W or W is not a multiple of 16 bytes");
  if (n_items > RSPARSE_HIP_EASE_MAX_ITEMS)
    return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "n_items > 32768 (RSPARSE_HIP_EASE_MAX_ITEMS): an items x items matrix of doubles would pass 8 GiB");
  return RSPARSE_HIP_OK;
}

// BPR: what every entry refuses.  per_epoch: n_steps of the triples / step entries, batch of the epochs / fit entries (name: which);
// rank = 0 with max_rank = 0: the entry has no factors (the triples)
inline int bpr_args(bool missing, int n_rows, int n_items, int64_t nnz, int64_t row0, int mode, int64_t epoch0, int64_t n_epochs,
                    int per_epoch, const char* name, int rank, int max_rank, double lr, double lambda) {
  const auto ok = [](double v) { return v >= 0.0 && v <= 1.7976931348623157e308; };   // (NaN fails both)
  if (missing) return fail(RSPARSE_HIP_ERR_INVALID, "the pattern, the factors, their Adagrad states or an output is NULL");
  if (n_rows < 0 || n_items < 0 || nnz < 0 || nnz > 0x7fffffffLL)
    return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_rows < 0, n_items < 0, nnz < 0 or nnz >= 2^31)");
  if (row0 < 0 || row0 + (int64_t)n_rows > (1LL << 32)) return fail(RSPARSE_HIP_ERR_INVALID, "the global row index does not fit 32 bits");
  if (mode != 0 && mode != 1) return fail(RSPARSE_HIP_ERR_INVALID, "mode is 0 (fit) or 1 (fold-in)");
  if (epoch0 < 0 || n_epochs < 0 || epoch0 + n_epochs > (1LL << 31)) return fail(RSPARSE_HIP_ERR_INVALID, "an epoch outside [0, 2^31)");
  if (per_epoch < 1) return fail(RSPARSE_HIP_ERR_INVALID, std::string(name) + " < 1");
  if (max_rank) {
    if (rank < 1) return fail(RSPARSE_HIP_ERR_INVALID, "rank < 1");
    if (!ok(lr) || !ok(lambda)) return fail(RSPARSE_HIP_ERR_INVALID, "learning_rate or lambda is negative or not finite");
    if (rank > max_rank)
      return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "rank > " + std::to_string(max_rank) + " is not on the device path");
  }
  if (nnz > 0 && n_items == 0) return fail(RSPARSE_HIP_ERR_INVALID, "entries without items");
  return RSPARSE_HIP_OK;
}

// the item side numbers the two contributions of every slot of a step, 2k and 2k + 1, in 32 bits and counts them in an int
inline int bpr_step_size(int64_t nnz, int n_steps, int update_items) {
  if (update_items && (nnz + n_steps - 1) / n_steps >= (1LL << 30))
    return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "a step of 2^30 or more triples with update_items: take a smaller batch");
  return RSPARSE_HIP_OK;
}

// rsparse_hip_score_pairs_device / _f64_device (kernels: wrmf_score.hip).  Handed in:
//   int workspace(size_t n, double*& buf)    makes sure of n doubles of the side's grow-only workspace
// which is only asked for the sums without the scores: the scores then live there, and their count, p[n_rows], has to be
// read back first (the one case in which this call waits for the stream).
template <class T, class Workspace>
int score_pairs_device(const T* d_U, const T* d_V, int n_rows, int n_cols, int r, const int32_t* d_p, const int32_t* d_j, double add,
                       const double* d_actual, double* d_scores, double* d_sse, double* d_sae, hipStream_t s, Workspace workspace) {
  if (!d_scores && !d_sse && !d_sae) return fail(RSPARSE_HIP_ERR_INVALID, "scores, sse and sae are all NULL");
  if (!d_U || !d_V || !d_p || !d_j) return fail(RSPARSE_HIP_ERR_INVALID, "U, V or the pattern (p, j) is NULL");
  if ((d_sse || d_sae) && !d_actual) return fail(RSPARSE_HIP_ERR_INVALID, "the error sums need the values: actual is NULL");
  if (n_rows < 0 || n_cols < 0 || r < 1) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_rows < 0, n_cols < 0 or r < 1)");
  if (r > RSPARSE_HIP_MAX_RANK) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "r > 256 is not on the device path");
  if (n_rows == 0) return RSPARSE_HIP_OK;
  const bool sums = d_sse || d_sae;
  double* sc = d_scores;
  if (!sc) {
    int32_t nnz = 0;
    HIP_TRY(hipMemcpyAsync(&nnz, d_p + n_rows, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (nnz <= 0) {   // nothing stored: every row's sums are 0
      if (d_sse) HIP_TRY(hipMemsetAsync(d_sse, 0, (size_t)n_rows * sizeof(double), s));
      if (d_sae) HIP_TRY(hipMemsetAsync(d_sae, 0, (size_t)n_rows * sizeof(double), s));
      return RSPARSE_HIP_OK;
    }
    if (int rc = workspace((size_t)nnz, sc)) return rc;
  }
  hipError_t e = launch_score_pairs(d_U, d_V, n_rows, n_cols, r, d_p, d_j, add, sc, s);
  if (e != hipSuccess) return hip_fail(e, "launch_score_pairs");
  if (sums && (e = launch_score_error_sums(sc, d_actual, d_p, n_rows, d_sse, d_sae, s)) != hipSuccess)
    return hip_fail(e, "launch_score_error_sums");
  return RSPARSE_HIP_OK;
}

// rsparse_hip_softals_half_device / _f64_device (kernels: wrmf_softals.hip).  `workspace` as above: the coefficient vectors and
// the partial sums of the rows that are split live there.
template <class T, class Workspace>
int softals_half_device(const int32_t* d_p, const int32_t* d_j, const T* d_x, const T* d_M, const T* d_W, int n_rows, int n_cols,
                        int r, const double* w, const double* sc, const double* t, T* d_out, double* d_sumsq, hipStream_t s,
                        Workspace workspace) {
  if (!d_p || !d_j || !d_x || !d_M || !d_out || !sc)
    return fail(RSPARSE_HIP_ERR_INVALID, "the pattern (p, j, x), M, out or s is NULL");
  if ((w || t) && !d_W) return fail(RSPARSE_HIP_ERR_INVALID, "w or t without W");
  if (n_rows < 0 || n_cols < 0 || r < 1) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_rows < 0, n_cols < 0 or r < 1)");
  if (r > RSPARSE_HIP_MAX_RANK) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "r > 256 is not on the device path");
  if (n_rows == 0) return RSPARSE_HIP_OK;
  double* ws = nullptr;
  if (int rc = workspace(softals_ws_doubles(r), ws)) return rc;
  double coef[768];
  for (int c = 0; c < 256; c++) {
    coef[c] = w && c < r ? w[c] : 0.0;
    coef[256 + c] = c < r ? sc[c] : 0.0;
    coef[512 + c] = t && c < r ? t[c] : 0.0;
  }
  // (pageable host memory: the runtime has taken its copy when the call returns)
  HIP_TRY(hipMemcpyAsync(ws, coef, sizeof(coef), hipMemcpyHostToDevice, s));
  hipError_t e = launch_softals_half(d_p, d_j, d_x, d_M, d_W, n_rows, n_cols, r, w != nullptr, t != nullptr, d_out, d_sumsq, ws, s);
  if (e != hipSuccess) return hip_fail(e, "launch_softals_half");
  return RSPARSE_HIP_OK;
}

// rsparse_hip_top_candidates_device / _f64_device (kernels: wrmf_score.hip, wrmf_candidates.hip).  `workspace` as above: the
// scores / keys, the admissibility bits and the row lists live there.  The number of candidates is read back first (this call
// waits for the stream once): the workspace is sized by it.  max_rank: the side's ceiling.
template <class T, class Workspace>
int top_candidates_device(const T* d_U, const T* d_V, int n_users, int n_items, int rank, int k, const int32_t* d_cand_p,
                          const int32_t* d_cand_j, const int32_t* d_nr_p, const int32_t* d_nr_j, const int32_t* d_excl0, int n_exclude,
                          double glob_mean, int32_t* d_res, double* d_scores, hipStream_t s, int max_rank, Workspace workspace) {
  if (!d_U || !d_V || !d_res || !d_scores) return fail(RSPARSE_HIP_ERR_INVALID, "NULL matrix or output");
  if (!d_cand_p || !d_cand_j) return fail(RSPARSE_HIP_ERR_INVALID, "the candidate pattern (cand_p, cand_j) is NULL");
  if (d_nr_p && !d_nr_j) return fail(RSPARSE_HIP_ERR_INVALID, "nr_p without nr_j");
  if (n_users < 0 || n_items < 0 || rank < 1 || k < 1 || n_exclude < 0)
    return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_users < 0, n_items < 0, rank < 1, k < 1 or n_exclude < 0)");
  if (n_exclude > 0 && !d_excl0) return fail(RSPARSE_HIP_ERR_INVALID, "exclude is NULL");
  if (rank > max_rank)
    return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "rank > " + std::to_string(max_rank) + " is not on the device path");
  if (int rc = refuse_large_k(k)) return rc;
  if (n_users == 0) return RSPARSE_HIP_OK;
  int32_t pe[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(&pe[0], d_cand_p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&pe[1], d_cand_p + n_users, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (pe[0] < 0 || pe[1] < pe[0]) return fail(RSPARSE_HIP_ERR_INVALID, "the candidate row pointers are negative or decrease");
  const int64_t nnz = (int64_t)pe[1] - pe[0];
  const size_t bytes = top_candidates_ws_bytes(n_users, nnz);
  double* ws = nullptr;
  if (int rc = workspace((bytes + 7) / 8, ws)) return rc;
  hipError_t e = launch_top_candidates(d_U, d_V, n_users, n_items, rank, k, d_cand_p, d_cand_j, pe[0], nnz, d_nr_p,
                                       d_nr_p ? d_nr_j : nullptr, n_exclude > 0 ? d_excl0 : nullptr, n_exclude, glob_mean, d_res,
                                       d_scores, s, ws);
  if (e != hipSuccess) return hip_fail(e, "launch_top_candidates");
  return RSPARSE_HIP_OK;
}

// rsparse_hip_explain_device / _f64_device (kernel: wrmf_explain.hip).  The rank ceiling is the kernel's (one k x k system per
// user in LDS), the same for both element types.
template <class T>
int explain_device(const T* d_V, int n_items, int r, const T* d_base, double diag, double diag_per_nnz, int n_users,
                   const int32_t* d_x_p, const int32_t* d_x_j, const T* d_wa, const T* d_wb, const int32_t* d_t_p,
                   const int32_t* d_t_j, const int64_t* d_out_p, T* d_contrib, double* d_total, int32_t* d_flags, hipStream_t s) {
  if (!d_V || !d_x_p || !d_t_p || !d_flags) return fail(RSPARSE_HIP_ERR_INVALID, "V, x_p, t_p or flags is NULL");
  if (d_t_j && (!d_x_j || !d_wa || !d_wb || !d_out_p || !d_contrib || !d_total))
    return fail(RSPARSE_HIP_ERR_INVALID, "targets without x_j, wa, wb, out_p, contrib or total");
  if (n_items < 0 || n_users < 0 || r < 1) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_items < 0, n_users < 0 or r < 1)");
  if (r > 128) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "explain: r > 128 is not on the device path");
  if (n_users == 0 || !d_t_j) return RSPARSE_HIP_OK;   // (no user, or no target at all: t_j is NULL)
  hipError_t e = launch_explain(d_V, n_items, r, d_base, diag, diag_per_nnz, n_users, d_x_p, d_x_j, d_wa, d_wb, d_t_p, d_t_j,
                                d_out_p, d_contrib, d_total, d_flags, s);
  if (e != hipSuccess) return hip_fail(e, "launch_explain");
  return RSPARSE_HIP_OK;
}

// rsparse_hip_init_factors_device / _f64_device (kernel: wrmf_init.hip).  No rank ceiling: nothing here depends on a solver.
template <class T>
int init_factors_device(uint64_t seed, int stream, int64_t row0, int n_rows, int rank, int64_t ld, double scale, int abs_values,
                        int ones_col, T* d_out, hipStream_t s) {
  if (n_rows < 0 || row0 < 0 || rank < 1 || ld < rank)
    return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_rows < 0, row0 < 0, rank < 1 or ld < rank)");
  if (stream < 0 || stream > 1) return fail(RSPARSE_HIP_ERR_INVALID, "stream must be 0 (user factors) or 1 (item factors)");
  if (ones_col < -1 || ones_col >= rank) return fail(RSPARSE_HIP_ERR_INVALID, "ones_col must be -1 or a column of the matrix");
  if (row0 > INT64_MAX / rank - n_rows)   // (row0 + n_rows) * rank, the end of the element index, in 63 bits
    return fail(RSPARSE_HIP_ERR_INVALID, "the element index (row0 + n_rows) * rank does not fit 63 bits");
  if (n_rows > 0 && !d_out) return fail(RSPARSE_HIP_ERR_INVALID, "d_out is NULL");
  if (n_rows == 0) return RSPARSE_HIP_OK;
  hipError_t e = launch_init_factors(seed, stream, row0, n_rows, rank, ld, scale, abs_values, ones_col, d_out, s);
  if (e != hipSuccess) return hip_fail(e, "launch_init_factors");
  return RSPARSE_HIP_OK;
}

// Shared body of the stateless drop-ins (als_implicit / als_explicit, src/wrmf_implicit.cpp:5-26, src/wrmf_explicit.cpp:5-26)
// once the caller has validated what its side validates and made its resident matrix (nnz non-zeros).  Handed in:
//   int scratch(SumScratch& w)    makes sure of the side's workspace and gives its sum scratch as it is now
//   int half(const T* dX, T* dY, const T* dG, const T* base_in, T* base_out, double* d_loss)    the side's half-iteration
// use_base: implicit feedback, no user/item biases and a global bias above the side's threshold.
template <class T, class Scratch, class Half>
int stateless_half_iteration(Scratch scratch, Half half, bool implicit, int n_rows, int n_cols, int64_t nnz, const T* X, T* Y,
                             const T* XtX, const T* cnt_X, int rank, double lambda, int dynamic_lambda, double* loss_out,
                             int with_biases, int is_x_bias_last_row, bool use_base, T* global_bias_base,
                             int global_bias_base_len, int initialize_bias_base) {
  if (implicit && !XtX) return fail(RSPARSE_HIP_ERR_INVALID, "XtX is NULL");
  const size_t nx = (size_t)rank * n_rows, ny = (size_t)rank * n_cols;
  const size_t ng = implicit && with_biases ? (size_t)(rank - 1) * (rank - 1) : (size_t)rank * rank;
  DevBuf dX, dY, dG, dW, dBase;
  HIP_TRY(upload_host(dX, X, nx));
  HIP_TRY(upload_host(dY, Y, ny));
  if (implicit) HIP_TRY(upload_host(dG, XtX, ng));
  const bool weighted = !implicit && dynamic_lambda && lambda > 0;
  if (weighted) {
    if (!cnt_X) return fail(RSPARSE_HIP_ERR_INVALID, "cnt_X is NULL with dynamic_lambda");
    HIP_TRY(upload_host(dW, cnt_X, (size_t)n_rows));
  }
  int rc;
  SumScratch w;
  if ((rc = scratch(w))) return rc;
  // counters left behind by earlier device-resident calls are not this call's: set aside here, handed back when this call
  // ends (a stateless call between a resident fit's half-iterations and its check must not swallow the fit's failures)
  StaleFailures stale_guard;
  const int blen = global_bias_base ? std::max(global_bias_base_len, 0) : 0;
  const bool given = use_base && !initialize_bias_base && blen >= rank;
  if (use_base) {
    // global_bias_base = -global_bias * rowSums(X), `rank` entries (wrmf_implicit.hpp:111-112).  The caller's buffer holds
    // global_bias_base_len entries -- the R driver allocates rank - 1 (R/model_WRMF.R:292) although the reference's C++ reads
    // and assigns `rank`; here never more than the stated length is touched: it is READ (initialize_bias_base == 0) only
    // when it holds the whole vector, otherwise the vector is recomputed from X (its definition); it is WRITTEN up to
    // min(len, rank) entries
    HIP_TRY(dBase.alloc((size_t)rank * sizeof(T)));
    if (given) HIP_TRY(hipMemcpy(dBase.p, global_bias_base, (size_t)rank * sizeof(T), hipMemcpyHostToDevice));
  }
  rc = half(dX.as<T>(), dY.as<T>(), dG.as<T>(), given ? dBase.as<T>() : nullptr, use_base && !given ? dBase.as<T>() : nullptr,
            w.scalars);
  if (rc) return rc;
  if (use_base && !given && initialize_bias_base && blen > 0) {
    std::vector<T> hb((size_t)rank);
    HIP_TRY(hipMemcpy(hb.data(), dBase.p, (size_t)rank * sizeof(T), hipMemcpyDeviceToHost));
    for (int t = 0; t < std::min(blen, rank); t++) global_bias_base[t] = hb[(size_t)t];
  }
  if ((rc = scratch(w))) return rc;   // (the half-iteration may have grown the partials)
  const bool regularised = lambda > 0 && nx > 0;
  if (regularised) {  // + lambda * accu(X % X)  [* cnt_X]
    const T* Xreg = dX.as<T>();
    int kreg = rank;
    DevBuf dXe;
    if (with_biases) {  // every row of X but the ones: drop_row(X, !is_x_bias_last_row), wrmf_explicit.hpp:147-159, :287-297
      kreg = rank - 1;
      HIP_TRY(dXe.alloc((size_t)kreg * n_rows * sizeof(T)));
      HIP_TRY(hipMemcpy2D(dXe.p, (size_t)kreg * sizeof(T), dX.as<T>() + (is_x_bias_last_row ? 1 : 0), (size_t)rank * sizeof(T),
                          (size_t)kreg * sizeof(T), (size_t)n_rows, hipMemcpyDeviceToDevice));
      Xreg = dXe.as<T>();
    }
    if ((rc = weighted_sumsq(Xreg, kreg, n_rows, weighted ? dW.as<T>() : nullptr, w.scalars + 1, w, nullptr))) return rc;
    HIP_TRY(hipDeviceSynchronize());   // dXe is released at the end of this block
  }
  HIP_TRY(hipDeviceSynchronize());
  int64_t nfail = 0;
  rsparse_hip_take_numeric_failures(&nfail, nullptr);
  double host_scalars[2] = {0, 0};
  HIP_TRY(hipMemcpy(host_scalars, w.scalars, 2 * sizeof(double), hipMemcpyDeviceToHost));
  const double reg = regularised ? lambda * host_scalars[1] : 0.0;
  if (ny) HIP_TRY(hipMemcpy(Y, dY.p, ny * sizeof(T), hipMemcpyDeviceToHost));
  if (loss_out) *loss_out = (host_scalars[0] + reg) / (double)nnz;  // wrmf_implicit.hpp:304
  if (nfail)
    return fail(RSPARSE_HIP_ERR_NUMERIC, std::to_string(nfail) + " per-row systems were singular (not positive definite, and "
                                         "the general solver found a zero pivot column)");
  return RSPARSE_HIP_OK;
}

// The host bias vectors of the stateless bias initialisation (initialize_biases_float / _double, src/wrmf_init.cpp:5-34)
// up, `run(d_user_bias, d_item_bias)` on them, and down again.
template <class T, class Run>
int with_device_biases(int n_users, int n_items, T* user_bias, T* item_bias, Run run) {
  DevBuf dU, dI;
  HIP_TRY(upload_host(dU, user_bias, (size_t)n_users));
  HIP_TRY(upload_host(dI, item_bias, (size_t)n_items));
  if (int rc = run(dU.as<T>(), dI.as<T>())) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if (n_users) HIP_TRY(hipMemcpy(user_bias, dU.p, (size_t)n_users * sizeof(T), hipMemcpyDeviceToHost));
  if (n_items) HIP_TRY(hipMemcpy(item_bias, dI.p, (size_t)n_items * sizeof(T), hipMemcpyDeviceToHost));
  return RSPARSE_HIP_OK;
}

}  // namespace rsparse_hip
