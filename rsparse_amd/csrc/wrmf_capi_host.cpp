// The host-array ("R-facing") forms of the evaluation and data-preparation entries (declared in include/rsparse_wrmf_hip.h).
//
// A client of the device layer: every function here checks its host arrays, packs them the way the device form wants them
// (R's column-major matrices become row-major, 1-based ids 0-based), uploads, calls the PUBLIC `_device` entry on the null
// stream, waits for the device and fetches the results back into the caller's layout.  Besides those entries it uses the
// error helpers, the shared argument rules, DevBuf and upload_host (wrmf_capi_common.h): no launcher and no workspace.
#include "../../include/rsparse_wrmf_hip.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "wrmf_capi_common.h"

using namespace rsparse_hip;

namespace {

// The dgRMatrix slots: p from 0 and non-decreasing over its n rows; with j, the indices strictly ascending within a row (what
// the kernels' binary search needs).  The messages name the caller's arrays.
int check_csr(const int32_t* p, int n, const char* p_name, const int32_t* j = nullptr, const char* j_name = nullptr) {
  if (p[0] != 0) return fail(RSPARSE_HIP_ERR_INVALID, std::string(p_name) + "[0] != 0");
  for (int u = 0; u < n; u++) {
    if (p[u + 1] < p[u]) return fail(RSPARSE_HIP_ERR_INVALID, std::string(p_name) + " decreases");
    if (j)
      for (int32_t e = p[u] + 1; e < p[u + 1]; e++)
        if (j[e] <= j[e - 1]) return fail(RSPARSE_HIP_ERR_INVALID, std::string(j_name) + " is not strictly ascending within a row");
  }
  return RSPARSE_HIP_OK;
}

// the columns of a checked p: inside [0, n_cols) and strictly ascending within a row (a canonical pattern)
int check_columns(const int32_t* p, const int32_t* j, int n, int n_cols, const char* j_name) {
  for (int u = 0; u < n; u++)
    for (int32_t e = p[u]; e < p[u + 1]; e++)
      if (j[e] < 0 || j[e] >= n_cols || (e > p[u] && j[e] <= j[e - 1]))
        return fail(RSPARSE_HIP_ERR_INVALID, std::string(j_name) + " has a column outside [0, n_items), or a row is not strictly ascending");
  return RSPARSE_HIP_OK;
}

// n x k column-major (an R matrix: the predicted lists, their scores, the user factors) -> row-major T
template <class T, class S>
std::vector<T> row_major(const S* a, int n, int k) {
  std::vector<T> rows((size_t)n * k);
  for (int c = 0; c < k; c++)
    for (int u = 0; u < n; u++) rows[(size_t)u * k + c] = (T)a[(size_t)c * n + u];
  return rows;
}

// n elements of a device buffer into host memory; nothing to do for n == 0
template <class T>
hipError_t download(T* dst, const DevBuf& d, size_t n) {
  return n ? hipMemcpy(dst, d.p, n * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess;
}

// n x k row-major on the device -> a column-major host matrix
template <class T>
int fetch_col_major(const DevBuf& d, int n, int k, T* out) {
  std::vector<T> h((size_t)n * k);
  HIP_TRY(download(h.data(), d, h.size()));
  for (int u = 0; u < n; u++)
    for (int c = 0; c < k; c++) out[(size_t)c * n + u] = h[(size_t)u * k + c];
  return RSPARSE_HIP_OK;
}

// R's 1-based exclude list, 0-based and within [0, n_items), joins what `ex` holds; the whole sorted and unique
void add_excluded(const int32_t* exclude, int n_exclude, int n_items, std::vector<int32_t>& ex) {
  for (int e = 0; e < n_exclude; e++)
    if (exclude[e] >= 1 && exclude[e] <= n_items) ex.push_back(exclude[e] - 1);
  std::sort(ex.begin(), ex.end());
  ex.erase(std::unique(ex.begin(), ex.end()), ex.end());
}

// the device pointer of an optional array: NULL where the caller left it out
template <class T>
T* opt(bool given, DevBuf& d) {
  return given ? d.as<T>() : nullptr;
}

// the inverse norms of the window's item vectors, for the diversity and the MMR forms
int item_inv_norms(DevBuf& dV, bool f64, int n_items, int ld, int c0, int c1, DevBuf& dInv) {
  return f64 ? rsparse_hip_item_inv_norms_f64_device(dV.as<double>(), n_items, ld, c0, c1, dInv.as<double>(), nullptr)
             : rsparse_hip_item_inv_norms_device(dV.as<float>(), n_items, ld, c0, c1, dInv.as<double>(), nullptr);
}

int list_diversity_host(const int32_t* pred, int n_users, int k, const int32_t* cutoffs, int n_cutoffs, const void* V, bool f64,
                        int n_items, int ld, int c0, int c1, int32_t* counted, double* diversity) {
  int rc = list_diversity_args(pred, n_users, k, cutoffs, n_cutoffs, V, n_items, ld, c0, c1, counted, diversity);
  if (rc || n_users == 0) return rc;
  const int T = n_cutoffs;
  const size_t nt = (size_t)n_users * T;
  const std::vector<int32_t> rows = row_major<int32_t>(pred, n_users, k);
  DevBuf dPred, dV, dInv, dCnt, dDiv;
  HIP_TRY(upload_host(dPred, rows.data(), rows.size()));
  HIP_TRY(upload_host(dV, static_cast<const char*>(V), (size_t)n_items * ld * (f64 ? 8 : 4)));
  HIP_TRY(dInv.alloc((size_t)n_items * 8));
  if (counted) HIP_TRY(dCnt.alloc(nt * 4));
  if (diversity) HIP_TRY(dDiv.alloc(nt * 8));
  if ((rc = item_inv_norms(dV, f64, n_items, ld, c0, c1, dInv))) return rc;
  int32_t* d_cnt = opt<int32_t>(counted, dCnt);
  double* d_div = opt<double>(diversity, dDiv);
  rc = f64 ? rsparse_hip_list_diversity_f64_device(dPred.as<int32_t>(), n_users, k, cutoffs, T, dV.as<double>(), n_items, ld, c0, c1,
                                                   dInv.as<double>(), d_cnt, d_div, nullptr)
           : rsparse_hip_list_diversity_device(dPred.as<int32_t>(), n_users, k, cutoffs, T, dV.as<float>(), n_items, ld, c0, c1,
                                               dInv.as<double>(), d_cnt, d_div, nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if (counted && (rc = fetch_col_major(dCnt, n_users, T, counted))) return rc;
  if (diversity && (rc = fetch_col_major(dDiv, n_users, T, diversity))) return rc;
  return RSPARSE_HIP_OK;
}

int mmr_rerank_host(const int32_t* lists, const double* scores, int n_users, int n_pool, int k, double trade_off, const void* V,
                    bool f64, int n_items, int ld, int c0, int c1, int32_t* items, double* picked, int32_t* positions,
                    double* objective) {
  int rc = mmr_rerank_args(lists, scores, n_users, n_pool, k, trade_off, V, n_items, ld, c0, c1, items);
  if (rc || n_users == 0) return rc;
  const size_t nk = (size_t)n_users * k;
  const std::vector<int32_t> rows = row_major<int32_t>(lists, n_users, n_pool);
  const std::vector<double> srows = row_major<double>(scores, n_users, n_pool);
  DevBuf dLists, dScores, dV, dInv, dItems, dPicked, dPos, dObj;
  HIP_TRY(upload_host(dLists, rows.data(), rows.size()));
  HIP_TRY(upload_host(dScores, srows.data(), srows.size()));
  HIP_TRY(upload_host(dV, static_cast<const char*>(V), (size_t)n_items * ld * (f64 ? 8 : 4)));
  HIP_TRY(dInv.alloc((size_t)n_items * 8));
  HIP_TRY(dItems.alloc(nk * 4));
  if (picked) HIP_TRY(dPicked.alloc(nk * 8));
  if (positions) HIP_TRY(dPos.alloc(nk * 4));
  if (objective) HIP_TRY(dObj.alloc(nk * 8));
  if ((rc = item_inv_norms(dV, f64, n_items, ld, c0, c1, dInv))) return rc;
  double *d_picked = opt<double>(picked, dPicked), *d_obj = opt<double>(objective, dObj);
  int32_t* d_pos = opt<int32_t>(positions, dPos);
  rc = f64 ? rsparse_hip_mmr_rerank_f64_device(dLists.as<int32_t>(), dScores.as<double>(), n_users, n_pool, k, trade_off,
                                               dV.as<double>(), n_items, ld, c0, c1, dInv.as<double>(), dItems.as<int32_t>(), d_picked,
                                               d_pos, d_obj, nullptr)
           : rsparse_hip_mmr_rerank_device(dLists.as<int32_t>(), dScores.as<double>(), n_users, n_pool, k, trade_off, dV.as<float>(),
                                           n_items, ld, c0, c1, dInv.as<double>(), dItems.as<int32_t>(), d_picked, d_pos, d_obj,
                                           nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if ((rc = fetch_col_major(dItems, n_users, k, items))) return rc;
  if (picked && (rc = fetch_col_major(dPicked, n_users, k, picked))) return rc;
  if (positions && (rc = fetch_col_major(dPos, n_users, k, positions))) return rc;
  if (objective && (rc = fetch_col_major(dObj, n_users, k, objective))) return rc;
  return RSPARSE_HIP_OK;
}

// the host form of both samplers: w == nullptr (with weighted false) is the uniform stream
int sample_negatives_host(uint64_t seed, int64_t row0, int n_rows, int n_item, int n, const int32_t* seen_p, const int32_t* seen_j,
                          const int32_t* keep_p, const int32_t* keep_j, const uint32_t* w, bool weighted, int32_t* out_p,
                          int32_t* out_j, int64_t out_capacity, int64_t* filled_rows) {
  int rc = sample_negatives_args(row0, n_rows, n_item, n, seen_p, seen_j, keep_p, keep_j, out_p, out_capacity);
  if (rc) return rc;
  if (weighted) {
    if (!w) return fail(RSPARSE_HIP_ERR_INVALID, "w is NULL");
    for (int i = 0; i < n_item; i++)
      if (w[i] == 0) return fail(RSPARSE_HIP_ERR_INVALID, "a weight is 0: every weight is at least 1 (exclude an item through the seen rows)");
    if (filled_rows) *filled_rows = 0;
  }
  // the dgRMatrix slots: p from 0, non-decreasing; j strictly ascending within a row and inside the matrix; keep within seen
  if (seen_p[0] != 0 || (keep_p && keep_p[0] != 0)) return fail(RSPARSE_HIP_ERR_INVALID, "seen_p[0] or keep_p[0] != 0");
  int64_t total = 0;
  out_p[0] = 0;
  for (int u = 0; u < n_rows; u++) {
    if (seen_p[u + 1] < seen_p[u] || (keep_p && keep_p[u + 1] < keep_p[u])) return fail(RSPARSE_HIP_ERR_INVALID, "seen_p or keep_p decreases");
    for (int32_t e = seen_p[u]; e < seen_p[u + 1]; e++)
      if (seen_j[e] < 0 || seen_j[e] >= n_item || (e > seen_p[u] && seen_j[e] <= seen_j[e - 1]))
        return fail(RSPARSE_HIP_ERR_INVALID, "a seen index is outside the matrix, or a row's indices are not strictly ascending");
    const int32_t S = seen_p[u + 1] - seen_p[u];
    int32_t K = 0;
    if (keep_p) {
      K = keep_p[u + 1] - keep_p[u];
      int32_t e = seen_p[u];
      for (int32_t t = keep_p[u]; t < keep_p[u + 1]; t++) {   // both ascending: one pass
        if (t > keep_p[u] && keep_j[t] <= keep_j[t - 1]) return fail(RSPARSE_HIP_ERR_INVALID, "a keep row's indices are not strictly ascending");
        while (e < seen_p[u + 1] && seen_j[e] < keep_j[t]) e++;
        if (e == seen_p[u + 1] || seen_j[e] != keep_j[t]) return fail(RSPARSE_HIP_ERR_INVALID, "a keep row is not a subset of its seen row");
      }
    }
    total += (int64_t)K + std::min(n, n_item - S);
    if (total > 0x7fffffffll) return fail(RSPARSE_HIP_ERR_INVALID, "the output has more than 2^31 - 1 entries: sample the rows in batches");
    out_p[u + 1] = (int32_t)total;
  }
  if (!out_j) return RSPARSE_HIP_OK;   // the sizes only: out_p[n_rows] is the capacity the second call needs
  if (total > out_capacity)
    return fail(RSPARSE_HIP_ERR_INVALID, "out_capacity is " + std::to_string(out_capacity) + ", the rows need " + std::to_string(total));
  if (n_rows == 0 || total == 0) return RSPARSE_HIP_OK;
  const size_t np1 = (size_t)n_rows + 1;
  DevBuf dSP, dSJ, dKP, dKJ, dOP, dOJ, dW, dC, dF;
  HIP_TRY(upload_host(dSP, seen_p, np1));
  HIP_TRY(upload_host(dSJ, seen_j, (size_t)seen_p[n_rows]));   // (never NULL, even when empty: the device form wants the slot)
  if (keep_p) {
    HIP_TRY(upload_host(dKP, keep_p, np1));
    HIP_TRY(upload_host(dKJ, keep_j, (size_t)keep_p[n_rows]));
  }
  HIP_TRY(dOP.alloc(np1 * 4));
  HIP_TRY(dOJ.alloc((size_t)total * 4));
  const int32_t *d_kp = opt<int32_t>(keep_p, dKP), *d_kj = opt<int32_t>(keep_p, dKJ);
  if (weighted) {   // (n_item >= 1: total > 0)
    HIP_TRY(upload_host(dW, w, (size_t)n_item));
    HIP_TRY(dC.alloc((size_t)n_item * 8));
    HIP_TRY(dF.alloc(sizeof(int32_t)));
    if ((rc = rsparse_hip_weights_prefix_device(dW.as<uint32_t>(), n_item, dC.as<uint64_t>(), nullptr))) return rc;
    rc = rsparse_hip_sample_negatives_weighted_device(seed, row0, n_rows, n_item, n, dSP.as<int32_t>(), dSJ.as<int32_t>(), d_kp, d_kj,
                                                      dC.as<uint64_t>(), dOP.as<int32_t>(), dOJ.as<int32_t>(), total, dF.as<int32_t>(),
                                                      nullptr);
  } else {
    rc = rsparse_hip_sample_negatives_device(seed, row0, n_rows, n_item, n, dSP.as<int32_t>(), dSJ.as<int32_t>(), d_kp, d_kj,
                                             dOP.as<int32_t>(), dOJ.as<int32_t>(), total, nullptr);
  }
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if (weighted && filled_rows) {
    int32_t f = 0;
    HIP_TRY(download(&f, dF, 1));
    *filled_rows = f;
  }
  HIP_TRY(download(out_p, dOP, np1));
  HIP_TRY(download(out_j, dOJ, (size_t)total));
  return RSPARSE_HIP_OK;
}

}  // namespace

extern "C" {

int rsparse_hip_top_product(const double* x, const double* y, int nr, int nc, int rank, unsigned k, unsigned n_threads,
                            const int32_t* nr_p, const int32_t* nr_j, const int32_t* exclude, int n_exclude,
                            double glob_mean, int32_t* res, double* scores) {
  (void)n_threads;
  if (!x || !y || !res || !scores) return fail(RSPARSE_HIP_ERR_INVALID, "NULL matrix or output");
  if (nr < 0 || nc < 0 || rank <= 0 || k < 1) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions");
  if (rank > RSPARSE_HIP_MAX_RANK) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "rank > 256 is not on the device path");
  if (int rc = refuse_large_k(k)) return rc;
  if (n_exclude < 0 || (n_exclude > 0 && !exclude)) return fail(RSPARSE_HIP_ERR_INVALID, "bad exclude");
  // x is nr x rank column-major -> row-major, in both precisions; y (rank x nc column-major) already has item vectors contiguous
  const std::vector<double> U64 = row_major<double>(x, nr, rank);
  const std::vector<float> U = row_major<float>(x, nr, rank), V(y, y + (size_t)nc * rank);
  std::vector<int32_t> ex;
  add_excluded(exclude, n_exclude, nc, ex);
  const int64_t nr_nnz = (nr_p && nr > 0) ? (int64_t)nr_p[nr] : 0;
  const bool filter = nr_nnz > 0 && nr_j;   // `not_empty_filter_matrix`, matrix_top_product.cpp:33
  DevBuf dU, dV, dU64, dV64, dP, dJ, dE, dR, dS;
  HIP_TRY(upload_host(dU, U.data(), U.size()));
  HIP_TRY(upload_host(dV, V.data(), V.size()));
  HIP_TRY(upload_host(dU64, U64.data(), U64.size()));
  HIP_TRY(upload_host(dV64, y, V.size()));
  HIP_TRY(dR.alloc((size_t)nr * k * 4));
  HIP_TRY(dS.alloc((size_t)nr * k * 8));
  if (filter) {
    HIP_TRY(upload_host(dP, nr_p, (size_t)nr + 1));
    HIP_TRY(upload_host(dJ, nr_j, (size_t)nr_nnz));
  }
  if (!ex.empty()) HIP_TRY(upload_host(dE, ex.data(), ex.size()));
  // candidates from the fp32 pass, scores and order from the doubles as given (find_top_product multiplies arma::mat)
  int rc = rsparse_hip_top_product_f64_device(dU.as<float>(), dV.as<float>(), dU64.as<double>(), dV64.as<double>(), nr, nc, rank,
                                              (int)k, -1, opt<int32_t>(filter, dP), opt<int32_t>(filter, dJ),
                                              opt<int32_t>(!ex.empty(), dE), (int)ex.size(), glob_mean, dR.as<int32_t>(),
                                              dS.as<double>(), nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if ((rc = fetch_col_major(dR, nr, (int)k, res))) return rc;
  return fetch_col_major(dS, nr, (int)k, scores);
}

// find_top_product (R/utils.R:31-59) within per-row candidate lists, host pointers, shaped like rsparse_hip_top_product: x is
// nr x rank and y rank x nc, column-major doubles; cand / nr: CSR over the rows of x with 0-based columns (cand: ascending and
// unique within a row); exclude: 1-based items; res / scores: nr x k column-major, 1-based with NA_integer_ / NA_real_.
int rsparse_hip_top_candidates(const double* x, const double* y, int nr, int nc, int rank, unsigned k, unsigned n_threads,
                               const int32_t* cand_p, const int32_t* cand_j, const int32_t* nr_p, const int32_t* nr_j,
                               const int32_t* exclude, int n_exclude, double glob_mean, int32_t* res, double* scores) {
  (void)n_threads;
  if (!x || !y || !res || !scores) return fail(RSPARSE_HIP_ERR_INVALID, "NULL matrix or output");
  if (!cand_p) return fail(RSPARSE_HIP_ERR_INVALID, "cand_p is NULL");
  if (nr < 0 || nc < 0 || rank <= 0 || k < 1) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions");
  if (rank > RSPARSE_HIP_MAX_RANK_F64) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "rank > 128 is not on the fp64 device path");
  int rc = refuse_large_k(k);
  if (rc) return rc;
  if (n_exclude < 0 || (n_exclude > 0 && !exclude)) return fail(RSPARSE_HIP_ERR_INVALID, "bad exclude");
  if ((rc = check_csr(cand_p, nr, "cand_p"))) return rc;
  const size_t nnz = (size_t)cand_p[nr];
  if (nnz && !cand_j) return fail(RSPARSE_HIP_ERR_INVALID, "cand_j is NULL");
  for (int i = 0; i < nr; i++)
    for (int t = cand_p[i]; t < cand_p[i + 1]; t++)
      if (cand_j[t] < 0 || cand_j[t] >= nc || (t > cand_p[i] && cand_j[t] <= cand_j[t - 1]))
        return fail(RSPARSE_HIP_ERR_INVALID, "a candidate index is outside the matrix, or a row's indices are not strictly ascending");
  const int64_t nr_nnz = (nr_p && nr_j && nr > 0) ? (int64_t)nr_p[nr] : 0;
  const bool filter = nr_nnz > 0;
  std::vector<int32_t> hj;   // not_recommend with ascending columns (what the device form asks for)
  if (filter) {
    if ((rc = check_csr(nr_p, nr, "nr_p"))) return rc;
    hj.assign(nr_j, nr_j + nr_nnz);
    for (int i = 0; i < nr; i++) std::sort(hj.begin() + nr_p[i], hj.begin() + nr_p[i + 1]);
  }
  std::vector<int32_t> ex;
  add_excluded(exclude, n_exclude, nc, ex);
  const std::vector<double> U = row_major<double>(x, nr, rank);   // (y already has item vectors contiguous)
  DevBuf dU, dV, dCP, dCJ, dP, dJ, dE, dR, dS;
  HIP_TRY(upload_host(dU, U.data(), U.size()));
  HIP_TRY(upload_host(dV, y, (size_t)rank * nc));
  HIP_TRY(upload_host(dCP, cand_p, (size_t)nr + 1));
  HIP_TRY(upload_host(dCJ, cand_j, nnz));
  if (filter) {
    HIP_TRY(upload_host(dP, nr_p, (size_t)nr + 1));
    HIP_TRY(upload_host(dJ, hj.data(), hj.size()));
  }
  if (!ex.empty()) HIP_TRY(upload_host(dE, ex.data(), ex.size()));
  HIP_TRY(dR.alloc((size_t)nr * k * 4));
  HIP_TRY(dS.alloc((size_t)nr * k * 8));
  rc = rsparse_hip_top_candidates_f64_device(dU.as<double>(), dV.as<double>(), nr, nc, rank, (int)k, dCP.as<int32_t>(),
                                             dCJ.as<int32_t>(), opt<int32_t>(filter, dP), opt<int32_t>(filter, dJ),
                                             opt<int32_t>(!ex.empty(), dE), (int)ex.size(), glob_mean, dR.as<int32_t>(),
                                             dS.as<double>(), nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if ((rc = fetch_col_major(dR, nr, (int)k, res))) return rc;
  return fetch_col_major(dS, nr, (int)k, scores);
}

int rsparse_hip_similar_items(const double* components, int rank, int n_items, int first_row, int n_rows, const int32_t* query,
                              int n_q, int k, int exclude_self, const int32_t* exclude, int n_exclude, int32_t* res,
                              double* scores) {
  int rc = similar_items_args(n_items, n_rows, n_q, k, n_exclude, exclude);
  if (rc) return rc;
  if (first_row < 0 || rank < 1 || (int64_t)first_row + n_rows > rank)
    return fail(RSPARSE_HIP_ERR_INVALID, "first_row / n_rows do not select rows of components");
  if (!components || (n_q > 0 && (!query || !res || !scores))) return fail(RSPARSE_HIP_ERR_INVALID, "NULL matrix, query or output");
  std::vector<int32_t> q0((size_t)n_q);
  for (int q = 0; q < n_q; q++) {   // R indices are 1-based
    if (query[q] < 1 || query[q] > n_items) return fail(RSPARSE_HIP_ERR_INVALID, "query item id out of range");
    q0[q] = query[q] - 1;
  }
  if (n_q == 0) return RSPARSE_HIP_OK;
  const int r = n_rows;
  // rank x n_items column-major = item vectors contiguous: the device form's n_items x ld row-major with ld = rank
  DevBuf dV, dVn32, dVn64, dF, dQ, dE, dR, dS;
  HIP_TRY(upload_host(dV, components, (size_t)n_items * rank));
  HIP_TRY(upload_host(dQ, q0.data(), q0.size()));
  HIP_TRY(dVn32.alloc((size_t)n_items * r * 4));
  HIP_TRY(dVn64.alloc((size_t)n_items * r * 8));
  HIP_TRY(dF.alloc((size_t)n_items * 4));
  HIP_TRY(dR.alloc((size_t)n_q * k * 4));
  HIP_TRY(dS.alloc((size_t)n_q * k * 8));
  // (the window's rules hold after the checks above -- a query exists, so n_items >= 1 -- and no buffer is NULL: none of the
  // entry's own refusals can fire)
  if ((rc = rsparse_hip_normalize_items_f64_device(dV.as<double>(), n_items, rank, first_row, first_row + r, dVn32.as<float>(),
                                                   dVn64.as<double>(), dF.as<int32_t>(), nullptr)))
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  // never returned: the degenerate items and the caller's exclusions
  std::vector<int32_t> flags((size_t)n_items), ex;
  HIP_TRY(download(flags.data(), dF, flags.size()));
  for (int i = 0; i < n_items; i++)
    if (flags[i]) ex.push_back(i);
  add_excluded(exclude, n_exclude, n_items, ex);
  if (!ex.empty()) HIP_TRY(upload_host(dE, ex.data(), ex.size()));
  rc = rsparse_hip_similar_items_device(dVn32.as<float>(), dVn64.as<double>(), n_items, r, dQ.as<int32_t>(), n_q, k, exclude_self,
                                        opt<int32_t>(!ex.empty(), dE), (int)ex.size(), dR.as<int32_t>(), dS.as<double>(), nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if ((rc = fetch_col_major(dR, n_q, k, res))) return rc;
  return fetch_col_major(dS, n_q, k, scores);
}

int rsparse_hip_ranking_metrics(const int32_t* pred, int n_users, int k, const int32_t* p, const int32_t* j, const double* x,
                                double* ap_out, double* ndcg_out) {
  int rc = ranking_metrics_args(pred, n_users, k, p, j, x, ap_out, ndcg_out);
  if (rc || (rc = check_csr(p, n_users, "actual_p", j, "actual_j"))) return rc;
  if (n_users == 0) return RSPARSE_HIP_OK;
  const size_t nnz = (size_t)p[n_users];
  const std::vector<int32_t> rows = row_major<int32_t>(pred, n_users, k);
  DevBuf dPred, dP, dJ, dX, dAp, dNdcg;
  HIP_TRY(upload_host(dPred, rows.data(), rows.size()));
  HIP_TRY(upload_host(dP, p, (size_t)n_users + 1));
  HIP_TRY(upload_host(dJ, j, nnz));   // (never NULL, even when empty: the device form wants the slot)
  if (ndcg_out) HIP_TRY(upload_host(dX, x, nnz));
  if (ap_out) HIP_TRY(dAp.alloc((size_t)n_users * 8));
  if (ndcg_out) HIP_TRY(dNdcg.alloc((size_t)n_users * 8));
  rc = rsparse_hip_ranking_metrics_device(dPred.as<int32_t>(), n_users, k, dP.as<int32_t>(), dJ.as<int32_t>(), opt<double>(ndcg_out, dX),
                                          opt<double>(ap_out, dAp), opt<double>(ndcg_out, dNdcg), nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if (ap_out) HIP_TRY(download(ap_out, dAp, (size_t)n_users));
  if (ndcg_out) HIP_TRY(download(ndcg_out, dNdcg, (size_t)n_users));
  return RSPARSE_HIP_OK;
}

int rsparse_hip_hit_metrics(const int32_t* pred, int n_users, int k, const int32_t* p, const int32_t* j, const int32_t* cutoffs,
                            int n_cutoffs, int32_t* hits, int32_t* first, double* precision, double* recall, double* hit,
                            double* mrr, int32_t* first_seen, int n_items) {
  const bool any = hits || first || precision || recall || hit || mrr || first_seen;
  int rc = hit_metrics_args(pred, n_users, k, p, j, cutoffs, n_cutoffs, any, first_seen, n_items);
  if (rc || (rc = check_csr(p, n_users, "actual_p", j, "actual_j"))) return rc;
  if (first_seen) std::fill(first_seen, first_seen + n_items, INT32_MAX);
  if (n_users == 0) return RSPARSE_HIP_OK;
  const int T = n_cutoffs;
  const size_t nt = (size_t)n_users * T;
  const std::vector<int32_t> rows = row_major<int32_t>(pred, n_users, k);
  DevBuf dPred, dP, dJ, dHits, dFirst, dSeen, dD[4];
  double *outs[4] = {precision, recall, hit, mrr}, *d_outs[4];
  HIP_TRY(upload_host(dPred, rows.data(), rows.size()));
  HIP_TRY(upload_host(dP, p, (size_t)n_users + 1));
  HIP_TRY(upload_host(dJ, j, (size_t)p[n_users]));   // (never NULL, even when empty: the device form wants the slot)
  if (hits) HIP_TRY(dHits.alloc(nt * 4));
  if (first) HIP_TRY(dFirst.alloc((size_t)n_users * 4));
  for (int q = 0; q < 4; q++) {
    if (outs[q]) HIP_TRY(dD[q].alloc(nt * 8));
    d_outs[q] = opt<double>(outs[q], dD[q]);
  }
  if (first_seen) HIP_TRY(upload_host(dSeen, first_seen, (size_t)n_items));
  rc = rsparse_hip_hit_metrics_device(dPred.as<int32_t>(), n_users, k, dP.as<int32_t>(), dJ.as<int32_t>(), cutoffs, T,
                                      opt<int32_t>(hits, dHits), opt<int32_t>(first, dFirst), d_outs[0], d_outs[1], d_outs[2], d_outs[3],
                                      opt<int32_t>(first_seen, dSeen), n_items, nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if (hits && (rc = fetch_col_major(dHits, n_users, T, hits))) return rc;
  if (first) HIP_TRY(download(first, dFirst, (size_t)n_users));
  for (int q = 0; q < 4; q++)
    if (outs[q] && (rc = fetch_col_major(dD[q], n_users, T, outs[q]))) return rc;
  if (first_seen) HIP_TRY(download(first_seen, dSeen, (size_t)n_items));
  return RSPARSE_HIP_OK;
}

int rsparse_hip_list_metrics(const int32_t* pred, int n_users, int k, const int32_t* cutoffs, int n_cutoffs,
                             const int32_t* item_count, const int64_t* item_info, int n_items, int32_t* valid, int64_t* count_sum,
                             int64_t* info_sum, double* popularity, double* novelty, int32_t* exposure) {
  int rc = list_metrics_args(pred, n_users, k, cutoffs, n_cutoffs, item_count, item_info, n_items, valid, count_sum, info_sum,
                             popularity, novelty, exposure);
  if (rc) return rc;
  if (item_count)
    for (int i = 0; i < n_items; i++)
      if (item_count[i] < 0) return fail(RSPARSE_HIP_ERR_INVALID, "item_count holds a negative value");
  if (item_info)
    for (int i = 0; i < n_items; i++)
      if (item_info[i] < 0 || item_info[i] >= ((int64_t)1 << 40))
        return fail(RSPARSE_HIP_ERR_INVALID, "item_info must lie in 0 <= v < 2^40");
  const int T = n_cutoffs;
  if (exposure) std::fill(exposure, exposure + (size_t)n_items * T, 0);
  if (n_users == 0) return RSPARSE_HIP_OK;
  const size_t nt = (size_t)n_users * T, ne = (size_t)n_items * T;
  const std::vector<int32_t> rows = row_major<int32_t>(pred, n_users, k);
  const bool use_count = item_count && (count_sum || popularity), use_info = item_info && (info_sum || novelty);
  DevBuf dPred, dCount, dInfo, dValid, dCs, dIs, dPop, dNov, dExp;
  HIP_TRY(upload_host(dPred, rows.data(), rows.size()));
  if (use_count) HIP_TRY(upload_host(dCount, item_count, (size_t)n_items));
  if (use_info) HIP_TRY(upload_host(dInfo, item_info, (size_t)n_items));
  if (valid) HIP_TRY(dValid.alloc(nt * 4));
  if (count_sum) HIP_TRY(dCs.alloc(nt * 8));
  if (info_sum) HIP_TRY(dIs.alloc(nt * 8));
  if (popularity) HIP_TRY(dPop.alloc(nt * 8));
  if (novelty) HIP_TRY(dNov.alloc(nt * 8));
  if (exposure) {
    HIP_TRY(dExp.alloc(ne * 4));
    HIP_TRY(hipMemset(dExp.p, 0, ne * 4));
  }
  rc = rsparse_hip_list_metrics_device(dPred.as<int32_t>(), n_users, k, cutoffs, T, opt<int32_t>(use_count, dCount),
                                       opt<int64_t>(use_info, dInfo), n_items, opt<int32_t>(valid, dValid), opt<int64_t>(count_sum, dCs),
                                       opt<int64_t>(info_sum, dIs), opt<double>(popularity, dPop), opt<double>(novelty, dNov),
                                       opt<int32_t>(exposure, dExp), nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if (valid && (rc = fetch_col_major(dValid, n_users, T, valid))) return rc;
  if (count_sum && (rc = fetch_col_major(dCs, n_users, T, count_sum))) return rc;
  if (info_sum && (rc = fetch_col_major(dIs, n_users, T, info_sum))) return rc;
  if (popularity && (rc = fetch_col_major(dPop, n_users, T, popularity))) return rc;
  if (novelty && (rc = fetch_col_major(dNov, n_users, T, novelty))) return rc;
  if (exposure) {   // T x n_items per interval -> n_items x T column-major: the same layout, cumulated along the cutoffs
    HIP_TRY(download(exposure, dExp, ne));
    for (int t = 1; t < T; t++)
      for (int i = 0; i < n_items; i++) exposure[(size_t)t * n_items + i] += exposure[(size_t)(t - 1) * n_items + i];
  }
  return RSPARSE_HIP_OK;
}

int rsparse_hip_list_diversity(const int32_t* pred, int n_users, int k, const int32_t* cutoffs, int n_cutoffs, const float* V,
                               int n_items, int ld, int c0, int c1, int32_t* counted, double* diversity) {
  return list_diversity_host(pred, n_users, k, cutoffs, n_cutoffs, V, false, n_items, ld, c0, c1, counted, diversity);
}
int rsparse_hip_list_diversity_f64(const int32_t* pred, int n_users, int k, const int32_t* cutoffs, int n_cutoffs, const double* V,
                                   int n_items, int ld, int c0, int c1, int32_t* counted, double* diversity) {
  return list_diversity_host(pred, n_users, k, cutoffs, n_cutoffs, V, true, n_items, ld, c0, c1, counted, diversity);
}

int rsparse_hip_mmr_rerank(const int32_t* lists, const double* scores, int n_users, int n_pool, int k, double trade_off,
                           const float* V, int n_items, int ld, int c0, int c1, int32_t* items, double* scores_out,
                           int32_t* positions, double* objective) {
  return mmr_rerank_host(lists, scores, n_users, n_pool, k, trade_off, V, false, n_items, ld, c0, c1, items, scores_out, positions,
                         objective);
}
int rsparse_hip_mmr_rerank_f64(const int32_t* lists, const double* scores, int n_users, int n_pool, int k, double trade_off,
                               const double* V, int n_items, int ld, int c0, int c1, int32_t* items, double* scores_out,
                               int32_t* positions, double* objective) {
  return mmr_rerank_host(lists, scores, n_users, n_pool, k, trade_off, V, true, n_items, ld, c0, c1, items, scores_out, positions,
                         objective);
}

int rsparse_hip_held_out_ranks(const double* x, const double* y, int nr, int nc, int rank, const int32_t* nr_p, const int32_t* nr_j,
                               const int32_t* exclude, int n_exclude, const int32_t* p, const int32_t* j, const double* ax,
                               int32_t* above, int32_t* tied, int32_t* n_adm, double* mpr, double* auc, double* mrr, double* sums) {
  int rc = held_out_ranks_args(x, y, nr, nc, rank, n_exclude, exclude, p, j, 0);
  if (rc) return rc;
  if (!above && !tied && !n_adm && !mpr && !auc && !mrr && !sums) return fail(RSPARSE_HIP_ERR_INVALID, "every output is NULL");
  if ((mpr || sums) && !ax) return fail(RSPARSE_HIP_ERR_INVALID, "mpr and sums need the weights: actual_x is NULL");
  if ((rc = check_csr(p, nr, "actual_p", j, "actual_j"))) return rc;
  if (nr == 0) return RSPARSE_HIP_OK;
  const size_t nnz = (size_t)p[nr], n = (size_t)nr;
  // x is nr x rank column-major -> row-major fp32; y (rank x nc column-major) already has item vectors contiguous
  const std::vector<float> U = row_major<float>(x, nr, rank), V(y, y + (size_t)nc * rank);
  std::vector<int32_t> ex;
  add_excluded(exclude, n_exclude, nc, ex);
  const int64_t nr_nnz = nr_p ? (int64_t)nr_p[nr] : 0;
  const bool filter = nr_nnz > 0 && nr_j;
  const bool weights = mpr || sums;
  DevBuf dU, dV, dNP, dNJ, dE, dP, dJ, dX, dA, dT, dN, dM;
  HIP_TRY(upload_host(dU, U.data(), U.size()));
  HIP_TRY(upload_host(dV, V.data(), V.size()));
  HIP_TRY(upload_host(dP, p, n + 1));
  HIP_TRY(upload_host(dJ, j, nnz));
  HIP_TRY(dA.alloc(nnz * 4));
  HIP_TRY(dT.alloc(nnz * 4));
  HIP_TRY(dN.alloc(n * 4));
  if (filter) {
    HIP_TRY(upload_host(dNP, nr_p, n + 1));
    HIP_TRY(upload_host(dNJ, nr_j, (size_t)nr_nnz));
  }
  if (!ex.empty()) HIP_TRY(upload_host(dE, ex.data(), ex.size()));
  rc = rsparse_hip_held_out_ranks_device(dU.as<float>(), dV.as<float>(), nr, nc, rank, opt<int32_t>(filter, dNP), opt<int32_t>(filter, dNJ),
                                         opt<int32_t>(!ex.empty(), dE), (int)ex.size(), dP.as<int32_t>(), dJ.as<int32_t>(), 0,
                                         dA.as<int32_t>(), dT.as<int32_t>(), dN.as<int32_t>(), nullptr);
  if (rc) return rc;
  double* dm = nullptr;   // mpr, auc, mrr (nr each), sums (3 nr)
  if (mpr || auc || mrr || sums) {
    HIP_TRY(dM.alloc(n * 6 * 8));
    dm = dM.as<double>();
    if (weights) HIP_TRY(upload_host(dX, ax, nnz));
    rc = rsparse_hip_rank_summary_device(nr, dP.as<int32_t>(), opt<double>(weights, dX), dA.as<int32_t>(), dT.as<int32_t>(),
                                         dN.as<int32_t>(), mpr ? dm : nullptr, auc ? dm + n : nullptr, mrr ? dm + 2 * n : nullptr,
                                         sums ? dm + 3 * n : nullptr, nullptr);
    if (rc) return rc;
  }
  HIP_TRY(hipDeviceSynchronize());
  if (above) HIP_TRY(download(above, dA, nnz));
  if (tied) HIP_TRY(download(tied, dT, nnz));
  if (n_adm) HIP_TRY(download(n_adm, dN, n));
  if (mpr) HIP_TRY(hipMemcpy(mpr, dm, n * 8, hipMemcpyDeviceToHost));
  if (auc) HIP_TRY(hipMemcpy(auc, dm + n, n * 8, hipMemcpyDeviceToHost));
  if (mrr) HIP_TRY(hipMemcpy(mrr, dm + 2 * n, n * 8, hipMemcpyDeviceToHost));
  if (sums) HIP_TRY(hipMemcpy(sums, dm + 3 * n, n * 3 * 8, hipMemcpyDeviceToHost));
  return RSPARSE_HIP_OK;
}

// cpp_make_sparse_approximation (src/utils.cpp:4-56): the values of X^T Y at the stored positions of a template.  CSR: position t
// of row i holds X[:, i] . Y[:, idx[t]]; CSC: position t of column c holds Y[:, c] . X[:, idx[t]] -- the two operands swap roles.
int rsparse_hip_sparse_approximation(int n_rows, int n_cols, const int32_t* p, const int32_t* idx, int sparse_matrix_type,
                                     const double* X, const double* Y, int rank, double* values_out) {
  if (sparse_matrix_type != 1 && sparse_matrix_type != 2)
    return fail(RSPARSE_HIP_ERR_INVALID, "sparse_matrix_type should be CSC = 1 or CSR = 2");
  if (n_rows < 0 || n_cols < 0 || rank < 1) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_rows < 0, n_cols < 0 or rank < 1)");
  if (rank > RSPARSE_HIP_MAX_RANK) return fail(RSPARSE_HIP_ERR_UNSUPPORTED, "rank > 256 is not on the device path");
  if (!p || !X || !Y) return fail(RSPARSE_HIP_ERR_INVALID, "p, X or Y is NULL");
  const bool csr = sparse_matrix_type == 2;
  const int n_outer = csr ? n_rows : n_cols, n_inner = csr ? n_cols : n_rows;
  int rc = check_csr(p, n_outer, "p");
  if (rc) return rc;
  const size_t nnz = (size_t)p[n_outer];
  if (nnz && (!idx || !values_out)) return fail(RSPARSE_HIP_ERR_INVALID, "the indices or values_out is NULL");
  for (size_t t = 0; t < nnz; t++)
    if (idx[t] < 0 || idx[t] >= n_inner) return fail(RSPARSE_HIP_ERR_INVALID, "an index is outside the matrix");
  if (nnz == 0) return RSPARSE_HIP_OK;
  DevBuf dO, dI, dP, dJ, dS;
  HIP_TRY(upload_host(dO, csr ? X : Y, (size_t)rank * n_outer));
  HIP_TRY(upload_host(dI, csr ? Y : X, (size_t)rank * n_inner));
  HIP_TRY(upload_host(dP, p, (size_t)n_outer + 1));
  HIP_TRY(upload_host(dJ, idx, nnz));
  HIP_TRY(dS.alloc(nnz * sizeof(double)));
  rc = rsparse_hip_score_pairs_f64_device(dO.as<double>(), dI.as<double>(), n_outer, n_inner, rank, dP.as<int32_t>(), dJ.as<int32_t>(),
                                          0.0, nullptr, dS.as<double>(), nullptr, nullptr, nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(download(values_out, dS, nnz));
  return RSPARSE_HIP_OK;
}

int rsparse_hip_sample_negatives(uint64_t seed, int64_t row0, int n_rows, int n_item, int n, const int32_t* seen_p,
                                 const int32_t* seen_j, const int32_t* keep_p, const int32_t* keep_j, int32_t* out_p, int32_t* out_j,
                                 int64_t out_capacity) {
  return sample_negatives_host(seed, row0, n_rows, n_item, n, seen_p, seen_j, keep_p, keep_j, nullptr, false, out_p, out_j, out_capacity,
                               nullptr);
}
int rsparse_hip_sample_negatives_weighted(uint64_t seed, int64_t row0, int n_rows, int n_item, int n, const int32_t* seen_p,
                                          const int32_t* seen_j, const int32_t* keep_p, const int32_t* keep_j, const uint32_t* w,
                                          int32_t* out_p, int32_t* out_j, int64_t out_capacity, int64_t* filled_rows) {
  return sample_negatives_host(seed, row0, n_rows, n_item, n, seen_p, seen_j, keep_p, keep_j, w, true, out_p, out_j, out_capacity,
                               filled_rows);
}

int rsparse_hip_split_rows(uint64_t seed, int64_t row0, int n_rows, int mode, uint64_t test_threshold, int leave_out, int min_train,
                           const int32_t* p, const int32_t* j, const void* v, int value_bytes, const double* by, int32_t* train_p,
                           int32_t* train_j, void* train_v, int32_t* test_p, int32_t* test_j, void* test_v, int64_t train_capacity,
                           int64_t test_capacity) {
  int rc = split_rows_args(row0, n_rows, mode, test_threshold, leave_out, min_train, p, j, v, value_bytes, by, train_p, train_j,
                           train_v, test_p, test_j, test_v, train_capacity, test_capacity);
  if (rc) return rc;
  // the dgRMatrix slots: p from 0, non-decreasing; j strictly ascending within a row; no NaN to order by
  if (p[0] != 0) return fail(RSPARSE_HIP_ERR_INVALID, "p[0] != 0");
  for (int u = 0; u < n_rows; u++) {
    if (p[u + 1] < p[u]) return fail(RSPARSE_HIP_ERR_INVALID, "p decreases");
    for (int32_t e = p[u]; e < p[u + 1]; e++) {
      if (j[e] < 0 || (e > p[u] && j[e] <= j[e - 1]))
        return fail(RSPARSE_HIP_ERR_INVALID, "an index is negative, or a row's indices are not strictly ascending");
      if (by && by[e] != by[e]) return fail(RSPARSE_HIP_ERR_INVALID, "NaN in `by`");
    }
  }
  train_p[0] = test_p[0] = 0;
  if (n_rows == 0) return RSPARSE_HIP_OK;
  const size_t nnz = (size_t)p[n_rows], np1 = (size_t)n_rows + 1, vb = (size_t)value_bytes;
  const bool write = train_j != nullptr;
  const char* vbytes = static_cast<const char*>(v);
  DevBuf dP, dJ, dV, dB, dTrP, dTeP, dTrJ, dTeJ, dTrV, dTeV;
  HIP_TRY(upload_host(dP, p, np1));
  HIP_TRY(upload_host(dJ, j, nnz));   // (never NULL, even when empty: the device form wants the slot)
  if (by) HIP_TRY(upload_host(dB, by, nnz));
  HIP_TRY(dTrP.alloc(np1 * 4));
  HIP_TRY(dTeP.alloc(np1 * 4));
  if (write) {
    // (the host form sizes the device outputs itself: either side holds at most every entry; the caller's capacities are
    // checked against the counts below)
    HIP_TRY(dTrJ.alloc(nnz * 4));
    HIP_TRY(dTeJ.alloc(nnz * 4));
    if (v) {
      HIP_TRY(upload_host(dV, vbytes, nnz * vb));
      HIP_TRY(dTrV.alloc(nnz * vb));
      HIP_TRY(dTeV.alloc(nnz * vb));
    }
  }
  // first the counts (NULL j outputs), so that the caller's capacities are judged before anything of theirs is written
  rc = rsparse_hip_split_rows_device(seed, row0, n_rows, mode, test_threshold, leave_out, min_train, dP.as<int32_t>(), dJ.as<int32_t>(),
                                     nullptr, 0, opt<double>(by, dB), dTrP.as<int32_t>(), nullptr, nullptr, dTeP.as<int32_t>(), nullptr,
                                     nullptr, 0, 0, nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(download(train_p, dTrP, np1));
  HIP_TRY(download(test_p, dTeP, np1));
  if (!write) return RSPARSE_HIP_OK;
  const int64_t n_tr = train_p[n_rows], n_te = test_p[n_rows];
  if (n_tr > train_capacity || n_te > test_capacity)
    return fail(RSPARSE_HIP_ERR_INVALID, "the capacities are " + std::to_string(train_capacity) + " / " + std::to_string(test_capacity) +
                                             ", the split needs " + std::to_string(n_tr) + " / " + std::to_string(n_te));
  if (nnz == 0) return RSPARSE_HIP_OK;
  rc = rsparse_hip_split_rows_device(seed, row0, n_rows, mode, test_threshold, leave_out, min_train, dP.as<int32_t>(), dJ.as<int32_t>(),
                                     opt<char>(v, dV), value_bytes, opt<double>(by, dB), dTrP.as<int32_t>(), dTrJ.as<int32_t>(),
                                     opt<char>(v, dTrV), dTeP.as<int32_t>(), dTeJ.as<int32_t>(), opt<char>(v, dTeV), n_tr, n_te, nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(download(train_j, dTrJ, (size_t)n_tr));
  HIP_TRY(download(test_j, dTeJ, (size_t)n_te));
  if (v) {
    HIP_TRY(download(static_cast<char*>(train_v), dTrV, (size_t)n_tr * vb));
    HIP_TRY(download(static_cast<char*>(test_v), dTeV, (size_t)n_te * vb));
  }
  return RSPARSE_HIP_OK;
}

int rsparse_hip_confidence(int kind, int n_rows, int n_cols, const int32_t* p, const int32_t* j, const double* x, double a, double b,
                           int norm, int by_columns, double* out) {
  if (n_rows < 0 || n_cols < 0) return fail(RSPARSE_HIP_ERR_INVALID, "bad dimensions (n_rows < 0 or n_cols < 0)");
  if (kind < RSPARSE_HIP_CONFIDENCE_LINEAR || kind > RSPARSE_HIP_CONFIDENCE_NORMALIZE)
    return fail(RSPARSE_HIP_ERR_INVALID, "unknown confidence kind " + std::to_string(kind));
  if (!p) return fail(RSPARSE_HIP_ERR_INVALID, "p is NULL");
  if (kind == RSPARSE_HIP_CONFIDENCE_NORMALIZE && norm != 1 && norm != 2) return fail(RSPARSE_HIP_ERR_INVALID, "norm must be 1 or 2");
  if (kind == RSPARSE_HIP_CONFIDENCE_LOG && !(b != 0.0)) return fail(RSPARSE_HIP_ERR_INVALID, "eps must not be 0");
  int rc = check_csr(p, n_rows, "p");
  if (rc) return rc;
  const int64_t nnz = p[n_rows];
  if (nnz == 0) return RSPARSE_HIP_OK;
  if (!j || !x || !out) return fail(RSPARSE_HIP_ERR_INVALID, "j, x or out is NULL");
  for (int64_t e = 0; e < nnz; e++)
    if (j[e] < 0 || j[e] >= n_cols) return fail(RSPARSE_HIP_ERR_INVALID, "a column index outside [0, n_cols)");
  // the item-major side on the host: the columns' counts, and their values where the columns are normalized
  const bool cols = kind == RSPARSE_HIP_CONFIDENCE_NORMALIZE && by_columns;
  const bool items = kind == RSPARSE_HIP_CONFIDENCE_TFIDF || kind == RSPARSE_HIP_CONFIDENCE_BM25 || cols;
  std::vector<int32_t> pt;
  std::vector<double> xt;
  if (items) {
    pt.assign((size_t)n_cols + 1, 0);
    for (int64_t e = 0; e < nnz; e++) pt[(size_t)j[e] + 1]++;
    for (int c = 0; c < n_cols; c++) pt[(size_t)c + 1] += pt[c];
    if (cols) {
      xt.resize((size_t)nnz);
      std::vector<int32_t> at(pt.begin(), pt.end() - 1);
      for (int64_t e = 0; e < nnz; e++) xt[(size_t)at[j[e]]++] = x[e];
    }
  }
  DevBuf dP, dJ, dX, dPt, dXt, dMom, dTot, dUser, dItem;
  HIP_TRY(upload_host(dP, p, (size_t)n_rows + 1));
  HIP_TRY(upload_host(dJ, j, (size_t)nnz));
  HIP_TRY(upload_host(dX, x, (size_t)nnz));
  HIP_TRY(dTot.alloc(8));
  const double *user_t = nullptr, *item_t = nullptr;
  if (items) {
    HIP_TRY(upload_host(dPt, pt.data(), pt.size()));
    HIP_TRY(dItem.alloc((size_t)n_cols * 8));
    item_t = dItem.as<double>();
  }
  if (kind == RSPARSE_HIP_CONFIDENCE_TFIDF || kind == RSPARSE_HIP_CONFIDENCE_BM25) {
    if ((rc = rsparse_hip_confidence_table_device(RSPARSE_HIP_CONFIDENCE_TABLE_IDF, n_cols, dPt.as<int32_t>(), nullptr, nullptr,
                                                  (double)n_rows, 0.0, 0.0, dItem.as<double>(), nullptr)))
      return rc;
  }
  if (kind == RSPARSE_HIP_CONFIDENCE_BM25 || (kind == RSPARSE_HIP_CONFIDENCE_NORMALIZE && !cols)) {
    HIP_TRY(dMom.alloc((size_t)n_rows * 8));
    HIP_TRY(dUser.alloc((size_t)n_rows * 8));
    user_t = dUser.as<double>();
    const bool bm = kind == RSPARSE_HIP_CONFIDENCE_BM25;
    if ((rc = rsparse_hip_confidence_moments_device(n_rows, nnz, dP.as<int32_t>(), dX.as<double>(), bm ? 1 : norm, dMom.as<double>(),
                                                    dTot.as<double>(), nullptr)))
      return rc;
    if ((rc = rsparse_hip_confidence_table_device(bm ? RSPARSE_HIP_CONFIDENCE_TABLE_BM25 : RSPARSE_HIP_CONFIDENCE_TABLE_NORM, n_rows,
                                                  nullptr, dMom.as<double>(), dTot.as<double>(), a, bm ? b : (double)norm,
                                                  (double)n_rows, dUser.as<double>(), nullptr)))
      return rc;
  } else if (cols) {
    HIP_TRY(upload_host(dXt, xt.data(), xt.size()));
    HIP_TRY(dMom.alloc((size_t)n_cols * 8));
    if ((rc = rsparse_hip_confidence_moments_device(n_cols, nnz, dPt.as<int32_t>(), dXt.as<double>(), norm, dMom.as<double>(),
                                                    dTot.as<double>(), nullptr)))
      return rc;
    if ((rc = rsparse_hip_confidence_table_device(RSPARSE_HIP_CONFIDENCE_TABLE_NORM, n_cols, nullptr, dMom.as<double>(), nullptr, a,
                                                  (double)norm, 0.0, dItem.as<double>(), nullptr)))
      return rc;
  }
  if ((rc = rsparse_hip_confidence_apply_device(kind, n_rows, nnz, dP.as<int32_t>(), dJ.as<int32_t>(), dX.as<double>(), user_t, item_t,
                                                n_cols, 0, a, b, dX.p, 0, nullptr)))
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(download(out, dX, (size_t)nnz));
  return RSPARSE_HIP_OK;
}

int rsparse_hip_events_to_csr(int64_t n_events, int n_users, int n_items, const int32_t* users, const int32_t* items,
                              const double* values, const double* timestamps, int aggregate, double half_life, double now, int has_now,
                              int32_t* p, int32_t* j, double* x, int32_t* count, double* latest, int64_t capacity, int64_t* n_cells) {
  int rc = events_args(n_events, n_users, n_items, users, items, timestamps, aggregate, half_life, p, j, x, capacity, n_cells);
  if (rc) return rc;
  for (int64_t e = 0; e < n_events; e++)
    if ((values && values[e] != values[e]) || (timestamps && timestamps[e] != timestamps[e]))
      return fail(RSPARSE_HIP_ERR_INVALID, "NaN in values or timestamps");
  *n_cells = 0;
  if (n_events == 0) {
    for (int64_t u = 0; u <= n_users; u++) p[u] = 0;
    return RSPARSE_HIP_OK;
  }
  const size_t n = (size_t)n_events, np1 = (size_t)n_users + 1;
  DevBuf dU, dI, dV, dT, dP, dJ, dX, dC, dL;
  HIP_TRY(upload_host(dU, users, n));
  HIP_TRY(upload_host(dI, items, n));
  if (values) HIP_TRY(upload_host(dV, values, n));
  if (timestamps) HIP_TRY(upload_host(dT, timestamps, n));
  // (the host form sizes the device outputs itself: n_events slots always suffice; the caller's capacity is judged below)
  const bool want_latest = latest && timestamps;
  HIP_TRY(dP.alloc(np1 * 4));
  HIP_TRY(dJ.alloc(n * 4));
  HIP_TRY(dX.alloc(n * 8));
  if (count) HIP_TRY(dC.alloc(n * 4));
  if (want_latest) HIP_TRY(dL.alloc(n * 8));
  rc = rsparse_hip_events_to_csr_device(n_events, n_users, n_items, dU.as<int32_t>(), dI.as<int32_t>(), opt<double>(values, dV),
                                        opt<double>(timestamps, dT), aggregate, half_life, now, has_now, dP.as<int32_t>(),
                                        dJ.as<int32_t>(), dX.as<double>(), opt<int32_t>(count, dC), opt<double>(want_latest, dL),
                                        n_events, n_cells, nullptr);
  if (rc) return rc;
  if (*n_cells > capacity)
    return fail(RSPARSE_HIP_ERR_INVALID, "the capacity is " + std::to_string(capacity) + ", the log has " + std::to_string(*n_cells) + " cells");
  HIP_TRY(hipDeviceSynchronize());
  const size_t nc = (size_t)*n_cells;
  HIP_TRY(download(p, dP, np1));
  HIP_TRY(download(j, dJ, nc));
  HIP_TRY(download(x, dX, nc));
  if (count) HIP_TRY(download(count, dC, nc));
  if (want_latest) HIP_TRY(download(latest, dL, nc));
  return RSPARSE_HIP_OK;
}

namespace {
// the item-major orientation of a checked pattern: a counting sort, users ascending within an item; l (nullable): a value per
// stored position, which moves with its entry into il
void item_major(const int32_t* p, const int32_t* j, int n_users, int n_items, std::vector<int32_t>& ip, std::vector<int32_t>& iu,
                const uint32_t* l, std::vector<uint32_t>* il) {
  const size_t nnz = (size_t)p[n_users];
  ip.assign((size_t)n_items + 1, 0);
  iu.resize(nnz);
  if (l) il->resize(nnz);
  for (size_t e = 0; e < nnz; e++) ip[(size_t)j[e] + 1]++;
  for (int i = 0; i < n_items; i++) ip[(size_t)i + 1] += ip[i];
  std::vector<int32_t> at(ip.begin(), ip.end() - 1);
  for (int u = 0; u < n_users; u++)
    for (int32_t e = p[u]; e < p[u + 1]; e++) {
      const size_t t = (size_t)at[j[e]]++;
      iu[t] = u;
      if (l) (*il)[t] = l[e];
    }
}
// The operands the host forms of the lists share -- the rows (x_p, x_j, x_v), the tables, not_recommend and exclude: check()
// judges the host arrays behind knn_recommend_args, upload() packs them for the device forms (row-major tables, 0-based ids).
struct KnnHostRows {
  DevBuf dXP, dXJ, dXV, dNb, dQ, dP, dJ, dE;
  std::vector<int32_t> ex;
  bool weighted = false, filter = false;

  int check(const int32_t* x_p, const int32_t* x_j, const uint32_t* x_v, int n_rows, int n_items, const uint32_t* q, int K,
            const int32_t* nr_p, const int32_t* nr_j) {
    if (int rc = check_csr(x_p, n_rows, "x_p")) return rc;
    if (x_p[n_rows] && !x_j) return fail(RSPARSE_HIP_ERR_INVALID, "x_j is NULL");
    if (int rc = check_columns(x_p, x_j, n_rows, n_items, "x_j")) return rc;
    if (x_v)
      for (int u = 0; u < n_rows; u++) {
        uint64_t sum = 0;
        for (int32_t e = x_p[u]; e < x_p[u + 1]; e++) {
          if (x_v[e] > 0xffffu) return fail(RSPARSE_HIP_ERR_INVALID, "a weight of x_v is above 2^16 - 1");
          sum += x_v[e];
        }
        if (sum >= (1ull << 31)) return fail(RSPARSE_HIP_ERR_INVALID, "the weights x_v of a row sum to 2^31 or more");
      }
    if (nr_p) {
      if (int rc = check_csr(nr_p, n_rows, "nr_p")) return rc;
      for (int32_t e = 0; e < nr_p[n_rows]; e++)
        if (nr_j[e] < 0 || nr_j[e] >= n_items) return fail(RSPARSE_HIP_ERR_INVALID, "nr_j has a column outside [0, n_items)");
    }
    for (size_t t = 0; t < (size_t)n_items * K; t++)
      if (q[t] > (1u << 30)) return fail(RSPARSE_HIP_ERR_INVALID, "a weight of q is above 2^30");
    return RSPARSE_HIP_OK;
  }

  int upload(const int32_t* x_p, const int32_t* x_j, const uint32_t* x_v, int n_rows, int n_items, const int32_t* neighbors,
             const uint32_t* q, int K, const int32_t* nr_p, const int32_t* nr_j, const int32_t* exclude, int n_exclude) {
    const size_t nnz = (size_t)x_p[n_rows], nt = (size_t)n_items * K, np1 = (size_t)n_rows + 1;
    std::vector<int32_t> nb = row_major<int32_t>(neighbors, n_items, K);
    for (size_t t = 0; t < nt; t++) nb[t] = (nb[t] >= 1 && nb[t] <= n_items) ? nb[t] - 1 : -1;
    const std::vector<uint32_t> qr = row_major<uint32_t>(q, n_items, K);
    add_excluded(exclude, n_exclude, n_items, ex);
    HIP_TRY(upload_host(dXP, x_p, np1));
    HIP_TRY(upload_host(dXJ, x_j, nnz));
    weighted = x_v && nnz;
    if (weighted) HIP_TRY(upload_host(dXV, x_v, nnz));
    HIP_TRY(upload_host(dNb, nb.data(), nt));
    HIP_TRY(upload_host(dQ, qr.data(), nt));
    filter = nr_p != nullptr;
    if (filter) {
      HIP_TRY(upload_host(dP, nr_p, np1));
      HIP_TRY(upload_host(dJ, nr_j, (size_t)nr_p[n_rows]));
    }
    if (!ex.empty()) HIP_TRY(upload_host(dE, ex.data(), ex.size()));
    return RSPARSE_HIP_OK;
  }

  const uint32_t* xv() { return opt<uint32_t>(weighted, dXV); }
  const int32_t* nr_p() { return opt<int32_t>(filter, dP); }
  const int32_t* nr_j() { return opt<int32_t>(filter, dJ); }
  const int32_t* excl() { return opt<int32_t>(!ex.empty(), dE); }
};
}  // namespace

int rsparse_hip_cooc_neighbors(const int32_t* p, const int32_t* j, int n_users, int n_items, int similarity, int K,
                               int32_t* neighbors, int32_t* counts) {
  int rc = cooc_neighbors_args(!p || !neighbors || !counts, n_users, n_items, 0, n_items, similarity, K, 0);
  if (rc) return rc;
  if ((rc = check_csr(p, n_users, "p"))) return rc;
  const size_t nnz = (size_t)p[n_users];
  if (nnz && !j) return fail(RSPARSE_HIP_ERR_INVALID, "j is NULL");
  if ((rc = check_columns(p, j, n_users, n_items, "j"))) return rc;
  if (n_items == 0) return RSPARSE_HIP_OK;
  std::vector<int32_t> ip, iu;
  item_major(p, j, n_users, n_items, ip, iu, nullptr, nullptr);
  DevBuf dIP, dIU, dUP, dUJ, dN, dC;
  HIP_TRY(upload_host(dIP, ip.data(), ip.size()));
  HIP_TRY(upload_host(dIU, iu.data(), nnz));
  HIP_TRY(upload_host(dUP, p, (size_t)n_users + 1));
  HIP_TRY(upload_host(dUJ, j, nnz));
  HIP_TRY(dN.alloc((size_t)n_items * K * 4));
  HIP_TRY(dC.alloc((size_t)n_items * K * 4));
  rc = rsparse_hip_cooc_neighbors_device(dIP.as<int32_t>(), dIU.as<int32_t>(), dUP.as<int32_t>(), dUJ.as<int32_t>(), n_users, n_items,
                                         0, n_items, similarity, K, 0, dN.as<int32_t>(), dC.as<int32_t>(), nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if ((rc = fetch_col_major(dN, n_items, K, neighbors))) return rc;
  for (size_t t = 0; t < (size_t)n_items * K; t++) neighbors[t] = neighbors[t] < 0 ? INT32_MIN : neighbors[t] + 1;   // R's ids
  return fetch_col_major(dC, n_items, K, counts);
}

int rsparse_hip_cooc_neighbors_weighted(const int32_t* p, const int32_t* j, const uint32_t* l, const uint32_t* r, int n_users,
                                        int n_items, const double* a, const double* b, double h, int K, int32_t* neighbors,
                                        uint64_t* sums) {
  int rc = cooc_neighbors_weighted_args(!p || !a || !b || !neighbors || !sums, n_users, n_items, 0, n_items, h, K, 0);
  if (rc) return rc;
  if ((rc = check_csr(p, n_users, "p"))) return rc;
  const size_t nnz = (size_t)p[n_users];
  if (nnz && !j) return fail(RSPARSE_HIP_ERR_INVALID, "j is NULL");
  if (nnz && (!l || !r)) return fail(RSPARSE_HIP_ERR_INVALID, "l or r is NULL");
  if ((rc = check_columns(p, j, n_users, n_items, "j"))) return rc;
  for (int i = 0; i < n_items; i++)
    if (!(a[i] >= 0x1p-200 && a[i] <= 0x1p200 && b[i] >= 0x1p-200 && b[i] <= 0x1p200))   // (NaN fails)
      return fail(RSPARSE_HIP_ERR_INVALID, "a table entry of a or b is not finite or outside [2^-200, 2^200]");
  if (n_items == 0) return RSPARSE_HIP_OK;
  std::vector<int32_t> ip, iu;
  std::vector<uint32_t> il;
  item_major(p, j, n_users, n_items, ip, iu, l, &il);
  uint32_t max_l = 0, max_r = 0;
  int32_t max_n = 0;
  for (size_t e = 0; e < nnz; e++) {
    max_l = std::max(max_l, l[e]);
    max_r = std::max(max_r, r[e]);
  }
  for (int i = 0; i < n_items; i++) max_n = std::max(max_n, ip[(size_t)i + 1] - ip[i]);
  if ((unsigned __int128)max_l * max_r * (unsigned __int128)max_n >= ((unsigned __int128)1 << 53))
    return fail(RSPARSE_HIP_ERR_INVALID, "max(l) max(r) max_j n_j >= 2^53: a sum would not be exact in double");
  DevBuf dIP, dIU, dIL, dUP, dUJ, dUR, dA, dB, dN, dS;
  HIP_TRY(upload_host(dIP, ip.data(), ip.size()));
  HIP_TRY(upload_host(dIU, iu.data(), nnz));
  HIP_TRY(upload_host(dIL, il.data(), nnz));
  HIP_TRY(upload_host(dUP, p, (size_t)n_users + 1));
  HIP_TRY(upload_host(dUJ, j, nnz));
  HIP_TRY(upload_host(dUR, r, nnz));
  HIP_TRY(upload_host(dA, a, (size_t)n_items));
  HIP_TRY(upload_host(dB, b, (size_t)n_items));
  HIP_TRY(dN.alloc((size_t)n_items * K * 4));
  HIP_TRY(dS.alloc((size_t)n_items * K * 8));
  rc = rsparse_hip_cooc_neighbors_weighted_device(dIP.as<int32_t>(), dIU.as<int32_t>(), dIL.as<uint32_t>(), dUP.as<int32_t>(),
                                                  dUJ.as<int32_t>(), dUR.as<uint32_t>(), n_users, n_items, 0, n_items, dA.as<double>(),
                                                  dB.as<double>(), h, K, 0, dN.as<int32_t>(), dS.as<uint64_t>(), nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if ((rc = fetch_col_major(dN, n_items, K, neighbors))) return rc;
  for (size_t t = 0; t < (size_t)n_items * K; t++) neighbors[t] = neighbors[t] < 0 ? INT32_MIN : neighbors[t] + 1;   // R's ids
  return fetch_col_major(dS, n_items, K, sums);
}

int rsparse_hip_knn_recommend(const int32_t* x_p, const int32_t* x_j, int n_rows, int n_items, const int32_t* neighbors,
                              const uint32_t* q, int K, const int32_t* nr_p, const int32_t* nr_j, const int32_t* exclude,
                              int n_exclude, int k, int32_t* res, int64_t* scores) {
  return rsparse_hip_knn_recommend_weighted(x_p, x_j, nullptr, n_rows, n_items, neighbors, q, K, nr_p, nr_j, exclude, n_exclude, k, res,
                                            scores);
}

int rsparse_hip_knn_recommend_weighted(const int32_t* x_p, const int32_t* x_j, const uint32_t* x_v, int n_rows, int n_items,
                                       const int32_t* neighbors, const uint32_t* q, int K, const int32_t* nr_p, const int32_t* nr_j,
                                       const int32_t* exclude, int n_exclude, int k, int32_t* res, int64_t* scores) {
  int rc = knn_recommend_args(!x_p || !neighbors || !q || !res || !scores, n_rows, n_items, K, nr_p, nr_j, exclude, n_exclude, k, 0);
  if (rc) return rc;
  KnnHostRows in;
  if ((rc = in.check(x_p, x_j, x_v, n_rows, n_items, q, K, nr_p, nr_j)) || n_rows == 0) return rc;
  if ((rc = in.upload(x_p, x_j, x_v, n_rows, n_items, neighbors, q, K, nr_p, nr_j, exclude, n_exclude))) return rc;
  const size_t nk = (size_t)n_rows * k;
  DevBuf dR, dS;
  HIP_TRY(dR.alloc(nk * 4));
  HIP_TRY(dS.alloc(nk * 8));
  rc = rsparse_hip_knn_recommend_weighted_device(in.dXP.as<int32_t>(), in.dXJ.as<int32_t>(), in.xv(), n_rows, n_items, in.dNb.as<int32_t>(),
                                                 in.dQ.as<uint32_t>(), K, in.nr_p(), in.nr_j(), in.excl(), (int)in.ex.size(), k, 0,
                                                 dR.as<int32_t>(), dS.as<int64_t>(), nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if ((rc = fetch_col_major(dR, n_rows, k, res))) return rc;
  return fetch_col_major(dS, n_rows, k, scores);
}

int rsparse_hip_knn_top_candidates(const int32_t* x_p, const int32_t* x_j, const uint32_t* x_v, int n_rows, int n_items,
                                   const int32_t* neighbors, const uint32_t* q, int K, const int32_t* cand_p, const int32_t* cand_j,
                                   const int32_t* nr_p, const int32_t* nr_j, const int32_t* exclude, int n_exclude, int k, int32_t* res,
                                   int64_t* scores) {
  int rc = knn_recommend_args(!x_p || !neighbors || !q || !cand_p || !res || !scores, n_rows, n_items, K, nr_p, nr_j, exclude, n_exclude,
                              k, 0);
  if (rc) return rc;
  KnnHostRows in;
  if ((rc = in.check(x_p, x_j, x_v, n_rows, n_items, q, K, nr_p, nr_j))) return rc;
  if ((rc = check_csr(cand_p, n_rows, "cand_p"))) return rc;
  const size_t n_cand = (size_t)cand_p[n_rows];
  if (n_cand && !cand_j) return fail(RSPARSE_HIP_ERR_INVALID, "cand_j is NULL");
  if ((rc = check_columns(cand_p, cand_j, n_rows, n_items, "cand_j"))) return rc;
  if (n_rows == 0) return RSPARSE_HIP_OK;
  if ((rc = in.upload(x_p, x_j, x_v, n_rows, n_items, neighbors, q, K, nr_p, nr_j, exclude, n_exclude))) return rc;
  const size_t nk = (size_t)n_rows * k;
  DevBuf dCP, dCJ, dR, dS;
  HIP_TRY(upload_host(dCP, cand_p, (size_t)n_rows + 1));
  HIP_TRY(upload_host(dCJ, cand_j, n_cand));
  HIP_TRY(dR.alloc(nk * 4));
  HIP_TRY(dS.alloc(nk * 8));
  rc = rsparse_hip_knn_top_candidates_device(in.dXP.as<int32_t>(), in.dXJ.as<int32_t>(), in.xv(), n_rows, n_items, in.dNb.as<int32_t>(),
                                             in.dQ.as<uint32_t>(), K, dCP.as<int32_t>(), dCJ.as<int32_t>(), in.nr_p(), in.nr_j(), in.excl(),
                                             (int)in.ex.size(), k, 0, dR.as<int32_t>(), dS.as<int64_t>(), nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if ((rc = fetch_col_major(dR, n_rows, k, res))) return rc;
  return fetch_col_major(dS, n_rows, k, scores);
}

int rsparse_hip_knn_held_out_ranks(const int32_t* x_p, const int32_t* x_j, const uint32_t* x_v, int n_rows, int n_items,
                                   const int32_t* neighbors, const uint32_t* q, int K, const int32_t* actual_p, const int32_t* actual_j,
                                   const int32_t* nr_p, const int32_t* nr_j, const int32_t* exclude, int n_exclude, int32_t* above,
                                   int32_t* tied, int32_t* n_adm) {
  int rc = knn_recommend_args(!x_p || !neighbors || !q || !actual_p || !above || !tied || !n_adm, n_rows, n_items, K, nr_p, nr_j, exclude,
                              n_exclude, 1, 0);
  if (rc) return rc;
  KnnHostRows in;
  if ((rc = in.check(x_p, x_j, x_v, n_rows, n_items, q, K, nr_p, nr_j))) return rc;
  if ((rc = check_csr(actual_p, n_rows, "actual_p"))) return rc;
  if (actual_p[n_rows] && !actual_j) return fail(RSPARSE_HIP_ERR_INVALID, "actual_j is NULL");
  if ((rc = check_csr(actual_p, n_rows, "actual_p", actual_j, "actual_j"))) return rc;
  if (n_rows == 0) return RSPARSE_HIP_OK;
  if ((rc = in.upload(x_p, x_j, x_v, n_rows, n_items, neighbors, q, K, nr_p, nr_j, exclude, n_exclude))) return rc;
  const size_t n_act = (size_t)actual_p[n_rows];
  DevBuf dAP, dAJ, dA, dT, dN;
  HIP_TRY(upload_host(dAP, actual_p, (size_t)n_rows + 1));
  HIP_TRY(upload_host(dAJ, actual_j, n_act));
  HIP_TRY(dA.alloc(n_act * 4));
  HIP_TRY(dT.alloc(n_act * 4));
  HIP_TRY(dN.alloc((size_t)n_rows * 4));
  rc = rsparse_hip_knn_held_out_ranks_device(in.dXP.as<int32_t>(), in.dXJ.as<int32_t>(), in.xv(), n_rows, n_items, in.dNb.as<int32_t>(),
                                             in.dQ.as<uint32_t>(), K, dAP.as<int32_t>(), dAJ.as<int32_t>(), in.nr_p(), in.nr_j(), in.excl(),
                                             (int)in.ex.size(), 0, dA.as<int32_t>(), dT.as<int32_t>(), dN.as<int32_t>(), nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(download(above, dA, n_act));
  HIP_TRY(download(tied, dT, n_act));
  HIP_TRY(download(n_adm, dN, (size_t)n_rows));
  return RSPARSE_HIP_OK;
}

int rsparse_hip_item_gram(const int32_t* p, const int32_t* j, int n_users, int n_items, double lambda, double* out) {
  int rc = item_gram_args(!p || !out, n_users, n_items, 0, n_items, lambda, (size_t)std::max(n_items, 0), 0);
  if (rc) return rc;
  if ((rc = check_csr(p, n_users, "p"))) return rc;
  const size_t nnz = (size_t)p[n_users];
  if (nnz && !j) return fail(RSPARSE_HIP_ERR_INVALID, "j is NULL");
  if ((rc = check_columns(p, j, n_users, n_items, "j"))) return rc;
  if (n_items == 0) return RSPARSE_HIP_OK;
  std::vector<int32_t> ip, iu;
  item_major(p, j, n_users, n_items, ip, iu, nullptr, nullptr);
  DevBuf dIP, dIU, dUP, dUJ, dG;
  HIP_TRY(upload_host(dIP, ip.data(), ip.size()));
  HIP_TRY(upload_host(dIU, iu.data(), nnz));
  HIP_TRY(upload_host(dUP, p, (size_t)n_users + 1));
  HIP_TRY(upload_host(dUJ, j, nnz));
  HIP_TRY(dG.alloc((size_t)n_items * n_items * sizeof(double)));
  rc = rsparse_hip_item_gram_device(dIP.as<int32_t>(), dIU.as<int32_t>(), dUP.as<int32_t>(), dUJ.as<int32_t>(), n_users, n_items, 0,
                                    n_items, lambda, dG.as<double>(), (size_t)n_items, 0, nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(download(out, dG, (size_t)n_items * n_items));
  return RSPARSE_HIP_OK;
}

int rsparse_hip_slim_fit(const int32_t* p, const int32_t* j, int n_users, int n_items, double l1, double l2, int max_iter, double tol,
                         double* W, int32_t* sweeps) {
  int rc = slim_args(!p || !W || !sweeps, n_items, n_users, l1, l2, max_iter, tol, (size_t)std::max(n_items, 0), W, 0, 0);
  if (rc) return rc;
  if ((rc = check_csr(p, n_users, "p"))) return rc;
  const size_t nnz = (size_t)p[n_users];
  if (nnz && !j) return fail(RSPARSE_HIP_ERR_INVALID, "j is NULL");
  if ((rc = check_columns(p, j, n_users, n_items, "j"))) return rc;
  if (n_items == 0) return RSPARSE_HIP_OK;
  std::vector<int32_t> ip, iu;
  item_major(p, j, n_users, n_items, ip, iu, nullptr, nullptr);
  // the popular items first: their supports are the long ones
  std::vector<int32_t> cols((size_t)n_items);
  for (int i = 0; i < n_items; i++) cols[(size_t)i] = i;
  std::stable_sort(cols.begin(), cols.end(), [&](int32_t a, int32_t b) { return ip[a + 1] - ip[a] > ip[b + 1] - ip[b]; });
  const size_t n = (size_t)n_items, ld = (n * sizeof(double) + 255) / 256 * 256 / sizeof(double);
  DevBuf dIP, dIU, dUP, dUJ, dG, dC, dW, dS;
  HIP_TRY(upload_host(dIP, ip.data(), ip.size()));
  HIP_TRY(upload_host(dIU, iu.data(), nnz));
  HIP_TRY(upload_host(dUP, p, (size_t)n_users + 1));
  HIP_TRY(upload_host(dUJ, j, nnz));
  HIP_TRY(upload_host(dC, cols.data(), n));
  HIP_TRY(dG.alloc(n * n * sizeof(double)));
  HIP_TRY(dW.alloc(n * ld * sizeof(double)));
  HIP_TRY(dS.alloc(n * sizeof(int32_t)));
  HIP_TRY(hipMemsetAsync(dW.p, 0, n * ld * sizeof(double), nullptr));
  rc = rsparse_hip_item_gram_device(dIP.as<int32_t>(), dIU.as<int32_t>(), dUP.as<int32_t>(), dUJ.as<int32_t>(), n_users, n_items, 0,
                                    n_items, 0.0, dG.as<double>(), n, 0, nullptr);
  if (rc) return rc;
  rc = rsparse_hip_slim_columns_device(dG.as<double>(), n, n_items, dC.as<int32_t>(), n_items, l1, l2, max_iter, tol, dW.p, ld, 1,
                                       dS.as<int32_t>(), nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  std::vector<double> rows(n * ld);
  std::vector<int32_t> sw(n);
  HIP_TRY(download(rows.data(), dW, n * ld));
  HIP_TRY(download(sw.data(), dS, n));
  for (size_t c = 0; c < n; c++) {
    sweeps[cols[c]] = sw[c];
    for (size_t i = 0; i < n; i++) W[c * n + i] = rows[i * ld + c];
  }
  return RSPARSE_HIP_OK;
}

int rsparse_hip_bpr_fit(const int32_t* p, const int32_t* j, int n_users, int n_items, uint64_t seed, int n_epochs, int batch, int rank,
                        double learning_rate, double lambda, double* U, double* V, double* aU, double* aV, int64_t* counts) {
  int rc = bpr_args(!p || !U || !V || !aU || !aV || !counts, n_users, n_items, 0, 0, 0, 0, n_epochs, batch, "batch", rank,
                    RSPARSE_HIP_MAX_RANK_F64, learning_rate, lambda);
  if (rc) return rc;
  if ((rc = check_csr(p, n_users, "p"))) return rc;
  const size_t nnz = (size_t)p[n_users];
  if (nnz && !j) return fail(RSPARSE_HIP_ERR_INVALID, "j is NULL");
  if ((rc = check_columns(p, j, n_users, n_items, "j"))) return rc;
  for (int e = 0; e < 2 * n_epochs; e++) counts[e] = 0;
  if (n_users == 0) return RSPARSE_HIP_OK;
  const size_t nu = (size_t)n_users, ni = (size_t)n_items, k = (size_t)rank;
  DevBuf dP, dJ, dU, dV, dAU, dAV, dC;
  HIP_TRY(upload_host(dP, p, nu + 1));
  HIP_TRY(upload_host(dJ, j, nnz));
  HIP_TRY(dU.alloc(nu * k * sizeof(double)));
  HIP_TRY(dV.alloc(ni * k * sizeof(double)));
  HIP_TRY(dAU.alloc(nu * sizeof(double)));
  HIP_TRY(dAV.alloc(ni * sizeof(double)));
  HIP_TRY(dC.alloc(2 * (size_t)n_epochs * sizeof(int64_t)));
  HIP_TRY(hipMemsetAsync(dAU.p, 0, nu * sizeof(double), nullptr));
  HIP_TRY(hipMemsetAsync(dAV.p, 0, ni * sizeof(double) + (ni ? 0 : 8), nullptr));
  if ((rc = rsparse_hip_init_factors_f64_device(seed, 0, 0, n_users, rank, rank, 0.01, 0, -1, dU.p, nullptr))) return rc;
  if (n_items && (rc = rsparse_hip_init_factors_f64_device(seed, 1, 0, n_items, rank, rank, 0.01, 0, -1, dV.p, nullptr))) return rc;
  rc = rsparse_hip_bpr_epochs_f64_device(dP.as<int32_t>(), dJ.as<int32_t>(), n_users, n_items, (int64_t)nnz, 0, seed, 0, 0, n_epochs, batch,
                                         rank, learning_rate, lambda, 1, dU.as<double>(), dV.as<double>(), dAU.as<double>(),
                                         dAV.as<double>(), dC.as<int64_t>(), nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(download(U, dU, nu * k));
  HIP_TRY(download(V, dV, ni * k));
  HIP_TRY(download(aU, dAU, nu));
  HIP_TRY(download(aV, dAV, ni));
  if (n_epochs) HIP_TRY(download(counts, dC, 2 * (size_t)n_epochs));
  return RSPARSE_HIP_OK;
}

extern "C++" {
namespace {
// B (n x n column-major, an R matrix) as n row-major rows of ld elements, zeros beyond n; a non-finite entry -> false
template <class T>
bool ease_pack_weights(const T* B, int n, size_t ld, std::vector<T>& rows) {
  rows.assign((size_t)n * ld, T(0));
  for (int c = 0; c < n; c++)
    for (int i = 0; i < n; i++) {
      const T v = B[(size_t)c * n + i];
      if (!(v - v == T(0))) return false;
      rows[(size_t)i * ld + c] = v;
    }
  return true;
}
}  // namespace
}  // extern "C++"

extern "C++" {
namespace {
// The operands the host forms of the EASE lists share -- the rows (x_p, x_j), B, not_recommend and exclude: check() judges the
// host arrays behind ease_recommend_args and packs B, upload() hands them to the device forms (0-based ids).
struct EaseHostRows {
  DevBuf dXP, dXJ, dB, dP, dJ, dE;
  std::vector<int32_t> ex;
  std::vector<float> b32;
  std::vector<double> b64;
  size_t ld = 0;
  bool filter = false;

  int check(const int32_t* x_p, const int32_t* x_j, int n_rows, int n_items, const void* B, int b_is_double, const int32_t* nr_p,
            const int32_t* nr_j) {
    if (int rc = check_csr(x_p, n_rows, "x_p")) return rc;
    if (x_p[n_rows] && !x_j) return fail(RSPARSE_HIP_ERR_INVALID, "x_j is NULL");
    if (int rc = check_columns(x_p, x_j, n_rows, n_items, "x_j")) return rc;
    if (nr_p) {
      if (int rc = check_csr(nr_p, n_rows, "nr_p")) return rc;
      for (int32_t e = 0; e < nr_p[n_rows]; e++)
        if (nr_j[e] < 0 || nr_j[e] >= n_items) return fail(RSPARSE_HIP_ERR_INVALID, "nr_j has a column outside [0, n_items)");
    }
    const size_t elem = b_is_double ? sizeof(double) : sizeof(float);
    ld = ((size_t)n_items * elem + 255) / 256 * 256 / elem;
    if (!(b_is_double ? ease_pack_weights(static_cast<const double*>(B), n_items, ld, b64)
                      : ease_pack_weights(static_cast<const float*>(B), n_items, ld, b32)))
      return fail(RSPARSE_HIP_ERR_INVALID, "an entry of B is not finite");
    return RSPARSE_HIP_OK;
  }

  int upload(const int32_t* x_p, const int32_t* x_j, int n_rows, int n_items, int b_is_double, const int32_t* nr_p, const int32_t* nr_j,
             const int32_t* exclude, int n_exclude) {
    const size_t np1 = (size_t)n_rows + 1;
    add_excluded(exclude, n_exclude, n_items, ex);
    HIP_TRY(upload_host(dXP, x_p, np1));
    HIP_TRY(upload_host(dXJ, x_j, (size_t)x_p[n_rows]));
    if (b_is_double) HIP_TRY(upload_host(dB, b64.data(), b64.size()));
    else HIP_TRY(upload_host(dB, b32.data(), b32.size()));
    filter = nr_p != nullptr;
    if (filter) {
      HIP_TRY(upload_host(dP, nr_p, np1));
      HIP_TRY(upload_host(dJ, nr_j, (size_t)nr_p[n_rows]));
    }
    if (!ex.empty()) HIP_TRY(upload_host(dE, ex.data(), ex.size()));
    return RSPARSE_HIP_OK;
  }

  const int32_t* nr_p() { return opt<int32_t>(filter, dP); }
  const int32_t* nr_j() { return opt<int32_t>(filter, dJ); }
  const int32_t* excl() { return opt<int32_t>(!ex.empty(), dE); }
};

// the lists of a device form (n_rows x k row-major: 1-based items, order keys) as the host forms return them
int fetch_ease_lists(const DevBuf& dR, const DevBuf& dS, int n_rows, int k, int32_t* res, double* scores) {
  const size_t nk = (size_t)n_rows * k;
  if (int rc = fetch_col_major(dR, n_rows, k, res)) return rc;
  std::vector<uint64_t> keys(nk);
  if (int rc = fetch_col_major(dS, n_rows, k, keys.data())) return rc;
  for (size_t t = 0; t < nk; t++) {   // the order key back to its double; NaN where the list has ended
    const uint64_t key = keys[t], bits = (key >> 63) ? key ^ (1ull << 63) : ~key;
    double v;
    std::memcpy(&v, &bits, sizeof v);
    scores[t] = res[t] == INT32_MIN ? std::nan("") : v;
  }
  return RSPARSE_HIP_OK;
}
}  // namespace
}  // extern "C++"

int rsparse_hip_ease_recommend(const int32_t* x_p, const int32_t* x_j, int n_rows, int n_items, const void* B, int b_is_double,
                               const int32_t* nr_p, const int32_t* nr_j, const int32_t* exclude, int n_exclude, int k, int32_t* res,
                               double* scores) {
  int rc = ease_recommend_args(!x_p || !B || !res || !scores, n_rows, n_items, B, 0, 0, nr_p, nr_j, exclude, n_exclude, k, 0);
  if (rc) return rc;
  EaseHostRows in;
  if ((rc = in.check(x_p, x_j, n_rows, n_items, B, b_is_double, nr_p, nr_j)) || n_rows == 0) return rc;
  if ((rc = in.upload(x_p, x_j, n_rows, n_items, b_is_double, nr_p, nr_j, exclude, n_exclude))) return rc;
  DevBuf dR, dS;
  HIP_TRY(dR.alloc((size_t)n_rows * k * 4));
  HIP_TRY(dS.alloc((size_t)n_rows * k * 8));
  rc = rsparse_hip_ease_recommend_device(in.dXP.as<int32_t>(), in.dXJ.as<int32_t>(), n_rows, n_items, in.dB.p, in.ld, b_is_double, in.nr_p(),
                                         in.nr_j(), in.excl(), (int)in.ex.size(), k, 0, dR.as<int32_t>(), dS.as<uint64_t>(), nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  return fetch_ease_lists(dR, dS, n_rows, k, res, scores);
}

int rsparse_hip_ease_top_candidates(const int32_t* x_p, const int32_t* x_j, int n_rows, int n_items, const void* B, int b_is_double,
                                    const int32_t* cand_p, const int32_t* cand_j, const int32_t* nr_p, const int32_t* nr_j,
                                    const int32_t* exclude, int n_exclude, int k, int32_t* res, double* scores) {
  int rc = ease_recommend_args(!x_p || !B || !cand_p || !res || !scores, n_rows, n_items, B, 0, 0, nr_p, nr_j, exclude, n_exclude, k, 0);
  if (rc) return rc;
  EaseHostRows in;
  if ((rc = in.check(x_p, x_j, n_rows, n_items, B, b_is_double, nr_p, nr_j))) return rc;
  if ((rc = check_csr(cand_p, n_rows, "cand_p"))) return rc;
  const size_t n_cand = (size_t)cand_p[n_rows];
  if (n_cand && !cand_j) return fail(RSPARSE_HIP_ERR_INVALID, "cand_j is NULL");
  if ((rc = check_columns(cand_p, cand_j, n_rows, n_items, "cand_j"))) return rc;
  if (n_rows == 0) return RSPARSE_HIP_OK;
  if ((rc = in.upload(x_p, x_j, n_rows, n_items, b_is_double, nr_p, nr_j, exclude, n_exclude))) return rc;
  DevBuf dCP, dCJ, dR, dS;
  HIP_TRY(upload_host(dCP, cand_p, (size_t)n_rows + 1));
  HIP_TRY(upload_host(dCJ, cand_j, n_cand));
  HIP_TRY(dR.alloc((size_t)n_rows * k * 4));
  HIP_TRY(dS.alloc((size_t)n_rows * k * 8));
  rc = rsparse_hip_ease_top_candidates_device(in.dXP.as<int32_t>(), in.dXJ.as<int32_t>(), n_rows, n_items, in.dB.p, in.ld, b_is_double,
                                              dCP.as<int32_t>(), dCJ.as<int32_t>(), in.nr_p(), in.nr_j(), in.excl(), (int)in.ex.size(), k, 0,
                                              dR.as<int32_t>(), dS.as<uint64_t>(), nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  return fetch_ease_lists(dR, dS, n_rows, k, res, scores);
}

int rsparse_hip_ease_held_out_ranks(const int32_t* x_p, const int32_t* x_j, int n_rows, int n_items, const void* B, int b_is_double,
                                    const int32_t* actual_p, const int32_t* actual_j, const int32_t* nr_p, const int32_t* nr_j,
                                    const int32_t* exclude, int n_exclude, int32_t* above, int32_t* tied, int32_t* n_adm) {
  int rc = ease_recommend_args(!x_p || !B || !actual_p || !above || !tied || !n_adm, n_rows, n_items, B, 0, 0, nr_p, nr_j, exclude,
                               n_exclude, 1, 0);
  if (rc) return rc;
  EaseHostRows in;
  if ((rc = in.check(x_p, x_j, n_rows, n_items, B, b_is_double, nr_p, nr_j))) return rc;
  if ((rc = check_csr(actual_p, n_rows, "actual_p"))) return rc;
  if (actual_p[n_rows] && !actual_j) return fail(RSPARSE_HIP_ERR_INVALID, "actual_j is NULL");
  if ((rc = check_csr(actual_p, n_rows, "actual_p", actual_j, "actual_j"))) return rc;
  if (n_rows == 0) return RSPARSE_HIP_OK;
  if ((rc = in.upload(x_p, x_j, n_rows, n_items, b_is_double, nr_p, nr_j, exclude, n_exclude))) return rc;
  const size_t n_act = (size_t)actual_p[n_rows];
  DevBuf dAP, dAJ, dA, dT, dN;
  HIP_TRY(upload_host(dAP, actual_p, (size_t)n_rows + 1));
  HIP_TRY(upload_host(dAJ, actual_j, n_act));
  HIP_TRY(dA.alloc(n_act * 4));
  HIP_TRY(dT.alloc(n_act * 4));
  HIP_TRY(dN.alloc((size_t)n_rows * 4));
  rc = rsparse_hip_ease_held_out_ranks_device(in.dXP.as<int32_t>(), in.dXJ.as<int32_t>(), n_rows, n_items, in.dB.p, in.ld, b_is_double,
                                              dAP.as<int32_t>(), dAJ.as<int32_t>(), in.nr_p(), in.nr_j(), in.excl(), (int)in.ex.size(), 0,
                                              dA.as<int32_t>(), dT.as<int32_t>(), dN.as<int32_t>(), nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(download(above, dA, n_act));
  HIP_TRY(download(tied, dT, n_act));
  HIP_TRY(download(n_adm, dN, (size_t)n_rows));
  return RSPARSE_HIP_OK;
}

}  // extern "C"
