/*
 * rsparse_wrmf_hip.h -- C ABI of librsparse_wrmf_hip.so: the MI355X (gfx950) implementation of
 * rsparse's WRMF / ALS hot path.
 *
 * Plain C: pointers and sizes only, no R (SEXP), Rcpp, Armadillo or torch types.  Every entry
 * point returns an int status (0 = ok); nothing throws or exits across the boundary.  After a
 * non-zero status rsparse_hip_last_error() returns a description (thread-local).
 *
 * Two layers:
 *
 *  (1) stateless drop-ins -- the argument lists of the four generated `.Call` targets
 *      _rsparse_als_implicit_{double,float} / _rsparse_als_explicit_{double,float}
 *      (reference: src/RcppExports.cpp:329-415, src/wrmf_implicit.cpp:4-31,
 *      src/wrmf_explicit.cpp:4-27) with the S4 / arma objects flattened to the raw buffers those
 *      functions extract (src/utils.cpp:69-78 dgCMatrix slots, :115-128 float32 payload).
 *      Host pointers in, `Y` mutated in place, loss returned -- exactly the reference contract
 *      (R/model_WRMF.R:492,513 "Y is modified in-place").  They upload, run, download.
 *
 *  (2) a device-resident layer for callers that keep the matrices in HBM across half-iterations
 *      (the reference re-passes host memory every call; at 10M x 1M that would re-upload >4 GB of
 *      CSC per half-iteration).  Device pointers + a HIP stream; no implicit synchronisation
 *      unless a host result is requested.
 *
 * Layouts (identical to the reference):
 *   Conf    CSC: col_ptrs int32[n_cols+1], row_indices int32[nnz] 0-based, values (f64 on the
 *           host boundary, f32 once resident); one CSC column = one row solved.
 *   X       rank x n_rows  column-major (entity vectors contiguous), read only
 *   Y       rank x n_cols  column-major, in: CG warm start, out: solution
 *   XtX     rank x rank, must already contain + lambda*I (R/model_WRMF.R:474-486)
 *
 * Arithmetic: the *_float entry points and the device-resident layer (2) compute in fp32 (the
 * reference's precision="float" build; stated tolerance vs the reference CPU path: 1e-4 relative
 * Frobenius on the factor matrices).  The *_double entry points and the fp64 device layer (3)
 * compute in double, as als_implicit<double> / als_explicit<double> do (src/wrmf_implicit.cpp:5-14,
 * src/wrmf_explicit.cpp:5-14; precision = "double" is the R constructor's default, R/model_WRMF.R:82).
 */
#ifndef RSPARSE_WRMF_HIP_H
#define RSPARSE_WRMF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes */
#define RSPARSE_HIP_OK 0
#define RSPARSE_HIP_ERR_INVALID 1     /* bad argument (NULL pointer, negative size, rank <= 0 ...) */
#define RSPARSE_HIP_ERR_UNSUPPORTED 2 /* variant not on the device path: caller keeps its CPU path   */
#define RSPARSE_HIP_ERR_RUNTIME 3     /* HIP runtime / out of memory / no device                    */
#define RSPARSE_HIP_ERR_NUMERIC 4     /* a per-row system was singular for the general solver too (the   */
                                      /* reference's arma::solve throws -> R error, RcppExports.cpp:374,392) */

/* solver codes: inst/include/wrmf.hpp:16-18 */
#define RSPARSE_SOLVER_CHOLESKY 0
#define RSPARSE_SOLVER_CONJUGATE_GRADIENT 1
#define RSPARSE_SOLVER_NNLS 2 /* sequential coordinate descent, inst/include/nnls.hpp:10-48 */

#define RSPARSE_HIP_MAX_RANK 256     /* fp32 entry points and layer (2); ranks 129..256 run on one generic kernel family */
#define RSPARSE_HIP_MAX_RANK_F64 128 /* the *_double entry points and layer (3) */

const char* rsparse_hip_last_error(void);
int rsparse_hip_abi_version(void);
/* number of visible HIP devices (0 if none / runtime unavailable) */
int rsparse_hip_device_count(void);
int rsparse_hip_set_device(int device);

/* ------------------------------------------------------------------------------------------------
 * (1) stateless drop-ins, host pointers
 * ---------------------------------------------------------------------------------------------- */

/* replaces als_implicit_float  (src/wrmf_implicit.cpp:17-31 -> als_implicit<float>,
 * inst/include/wrmf_implicit.hpp:90-305).  n_rows/n_cols/col_ptrs/row_indices/values are the
 * dgCMatrix slots Dim[0], Dim[1], p, i, x.  rank = nrow(X).  n_threads is accepted and ignored.
 * with_biases: Cholesky and NNLS only (XtX is then (rank-1) x (rank-1)); with conjugate_gradient -> ERR_UNSUPPORTED
 * (the reference cannot run that combination either, wrmf_implicit.hpp:189,197).
 * global_bias >= sqrt(epsilon of the element type) (wrmf_implicit.hpp:108-109; 3.45e-4 for _float, 1.49e-8 for _double;
 * smaller values count as zero): every solver -- Cholesky and NNLS with or without biases (:146-153, 228-229, 262-270),
 * conjugate gradient without biases (cg_solver_implicit_global_bias, :35-57, 203; marked "very poor numerical
 * precision" in the reference and restated as written: note that it solves  lhs y = X_nnz c + base - g X_nnz (c - 1),
 * the Cholesky branch  lhs y = X_nnz c + base).
 * global_bias_base (no biases only; may be NULL): the vector -global_bias * rowSums(X), `rank` entries (:111-112).
 * global_bias_base_len = the number of entries the caller's buffer holds.  The R driver allocates rank - 1
 * (R/model_WRMF.R:292) while the reference's C++ assigns and reads `rank` (a local re-allocation on the write, one
 * element past the R vector on the read); this library never touches more than the stated length: with
 * initialize_bias_base != 0 it writes min(len, rank) entries, with initialize_bias_base == 0 it reads the vector only
 * if len >= rank and otherwise recomputes it from X (its definition).
 * *loss_out = the value the reference returns (loss / nnz). */
int rsparse_hip_als_implicit_float(int n_rows, int n_cols, const int32_t* col_ptrs,
                                   const int32_t* row_indices, const double* values,
                                   const float* X, float* Y, const float* XtX, int rank,
                                   double lambda, int n_threads, unsigned solver,
                                   unsigned cg_steps, int with_biases, int is_x_bias_last_row,
                                   double global_bias, float* global_bias_base, int global_bias_base_len,
                                   int initialize_bias_base, double* loss_out);

/* replaces als_implicit_double (src/wrmf_implicit.cpp:5-14 -> als_implicit<double>).  Buffers are f64 like the
 * reference's and the device computes in f64 (layer 3 below): every solver, biases and the global bias as for _float. */
int rsparse_hip_als_implicit_double(int n_rows, int n_cols, const int32_t* col_ptrs,
                                    const int32_t* row_indices, const double* values,
                                    const double* X, double* Y, const double* XtX, int rank,
                                    double lambda, int n_threads, unsigned solver,
                                    unsigned cg_steps, int with_biases, int is_x_bias_last_row,
                                    double global_bias, double* global_bias_base, int global_bias_base_len,
                                    int initialize_bias_base, double* loss_out);

/* replaces als_explicit_float (src/wrmf_explicit.cpp:17-27 -> als_explicit<float>,
 * inst/include/wrmf_explicit.hpp:33-174).  cnt_X has n_rows entries (used only for the
 * dynamic_lambda regulariser term of the loss, :160-170); may be NULL when !dynamic_lambda. */
int rsparse_hip_als_explicit_float(int n_rows, int n_cols, const int32_t* col_ptrs,
                                   const int32_t* row_indices, const double* values,
                                   const float* X, float* Y, const float* cnt_X, int rank,
                                   double lambda, unsigned n_threads, unsigned solver,
                                   unsigned cg_steps, int dynamic_lambda, int with_biases,
                                   int is_x_bias_last_row, double* loss_out);

/* replaces als_explicit_double (src/wrmf_explicit.cpp:5-14 -> als_explicit<double>); f64 arithmetic on the device */
int rsparse_hip_als_explicit_double(int n_rows, int n_cols, const int32_t* col_ptrs,
                                    const int32_t* row_indices, const double* values,
                                    const double* X, double* Y, const double* cnt_X, int rank,
                                    double lambda, unsigned n_threads, unsigned solver,
                                    unsigned cg_steps, int dynamic_lambda, int with_biases,
                                    int is_x_bias_last_row, double* loss_out);

/* replaces the R-side Gramian  XtX = tcrossprod(X) + fl(diag(lambda))  (R/model_WRMF.R:474-486,
 * :347-353).  Host pointers; X is rank x n column-major; XtX_out rank x rank. */
int rsparse_hip_gramian_float(const float* X, int rank, int64_t n, double lambda, float* XtX_out);
/* the same in f64 (precision = "double": tcrossprod of a base matrix; the ridge still passes through fl()) */
int rsparse_hip_gramian_double(const double* X, int rank, int64_t n, double lambda, double* XtX_out);

/* replaces initialize_biases_float / initialize_biases_double (src/wrmf_init.cpp:5-34; .Call
 * _rsparse_initialize_biases_{float,double}, src/RcppExports.cpp:417-454): the 9 arguments of the reference with the
 * two S4 matrices flattened to their slots -- m_csc_r = users x items by item column (csc_p [n_items+1], csc_i, csc_x),
 * m_csr_r = the same matrix by user column (csr_p [n_users+1], csr_i, csr_x) -- plus the returned global bias.
 * user_bias (n_users) / item_bias (n_items) are read (initial values) and written.  With is_explicit_feedback and
 * calculate_global_bias the global mean is removed from csc_x and csr_x in place, as the reference does
 * (inst/include/wrmf_utils.hpp:41-52). */
int rsparse_hip_initialize_biases_float(int n_users, int n_items, const int32_t* csc_p, const int32_t* csc_i,
                                        double* csc_x, const int32_t* csr_p, const int32_t* csr_i, double* csr_x,
                                        float* user_bias, float* item_bias, double lambda, int dynamic_lambda,
                                        int non_negative, int calculate_global_bias, int is_explicit_feedback,
                                        double* global_bias_out);
int rsparse_hip_initialize_biases_double(int n_users, int n_items, const int32_t* csc_p, const int32_t* csc_i,
                                         double* csc_x, const int32_t* csr_p, const int32_t* csr_i, double* csr_x,
                                         double* user_bias, double* item_bias, double lambda, int dynamic_lambda,
                                         int non_negative, int calculate_global_bias, int is_explicit_feedback,
                                         double* global_bias_out);

/* ------------------------------------------------------------------------------------------------
 * (2) device-resident layer
 * ---------------------------------------------------------------------------------------------- */

/* A CSC matrix resident in HBM plus its launch schedule (row-length buckets).  Replaces the
 * non-owning MappedCSC view (inst/include/mapped_csc.hpp:8-29, src/utils.cpp:69-78). */
typedef struct rsparse_hip_csc rsparse_hip_csc;

/* upload from host dgCMatrix slots (values f64 -> f32 on the way) */
int rsparse_hip_csc_create_host(int n_rows, int n_cols, const int32_t* col_ptrs,
                                const int32_t* row_indices, const double* values,
                                rsparse_hip_csc** out);
/* adopt arrays that already live on the current device (not copied, not freed by destroy;
 * they must outlive the handle).  d_values are f32. */
int rsparse_hip_csc_create_device(int n_rows, int n_cols, const int32_t* d_col_ptrs,
                                  const int32_t* d_row_indices, const float* d_values,
                                  rsparse_hip_csc** out);
int rsparse_hip_csc_destroy(rsparse_hip_csc* m);

/* On-device ingest -- replaces the host-side second orientation of a fit,
 * c_iu = t_shallow(as.csr.matrix(c_ui)) (R/model_WRMF.R:184-191), and the per-column arma::conv_to of the
 * values (inst/include/wrmf_implicit.hpp:182-183): the caller hands over ONE orientation.
 *
 * rsparse_hip_csc_transpose_device: CSC (d_p int32[n_cols+1], d_i int32[nnz], d_x f32[nnz]) of an
 * n_rows x n_cols matrix -> CSC of its transpose (d_pt int32[n_rows+1], d_it int32[nnz], d_xt f32[nnz]), row
 * indices ascending inside every output column (stable counting sort by row index).  All pointers are device
 * pointers; outputs are caller-allocated.  A row index outside [0, n_rows) -> RSPARSE_HIP_ERR_INVALID.
 * rsparse_hip_values_to_float_device: d_dst[e] = (float)d_src[e] (dgCMatrix@x is f64 on the wire). */
int rsparse_hip_csc_transpose_device(int n_rows, int n_cols, const int32_t* d_p, const int32_t* d_i,
                                     const float* d_x, int32_t* d_pt, int32_t* d_it, float* d_xt, void* stream);
int rsparse_hip_values_to_float_device(int64_t n, const double* d_src, float* d_dst, void* stream);
/* frozen != 0: the caller promises that the values of the handle (its own copy, or the adopted device array) do not change until
 * the promise is withdrawn (frozen = 0) or the handle destroyed -- what holds for `c_ui@x` / `c_iu@x` during a fit with implicit
 * feedback (R/model_WRMF.R:184-191: the matrices are prepared once).  The half-iterations then take the statistics of the values
 * that the fp16 matrix-core kernels scale their operands by (max confidence, "some confidence < 1") from ONE scan per handle
 * instead of one per call (0.46 ms per half-iteration at 5e8 non-zeros).  Results do not depend on it.  Library calls that
 * change values through a handle (rsparse_hip_initialize_biases_explicit_device) require frozen = 0. */
int rsparse_hip_csc_freeze_values(rsparse_hip_csc* m, int frozen);

/* info_out: [0] n_rows, [1] n_cols, [2] nnz, [3] rows with more than [7] non-zeros ("long" rows),
 * [4] longest row, [5] non-zeros in long rows, [6] empty rows, [7] per-wave tile capacity (32),
 * [8..13] rows and [14..19] non-zeros per CG launch bucket, [20] launch-table id, [21] segments of the long rows that
 * are split across workgroups (0 = none is), [22..27] waves per row
 * (team size) of each bucket (0 = bucket unused), [28..33] resident quads (4 non-zeros) per wave,
 * [34..39] waves per workgroup (negative = the bucket streams rows longer than the resident capacity). */
int rsparse_hip_csc_info(const rsparse_hip_csc* m, int64_t info_out[40]);

/* XtX = X X^T + fl(lambda) I on the device (MFMA).  d_sumsq_out (nullable, device double[1])
 * receives sum(X^2) = trace before the ridge -- the `accu(X % X)` term of the loss
 * (inst/include/wrmf_implicit.hpp:299-301) for free.  stream: hipStream_t (NULL = default).  n = 0 gives fl(lambda) I and
 * a sum of 0; d_X is not read then and may be NULL (an empty slice of a torch tensor has no address). */
int rsparse_hip_gramian_device(const float* d_X, int rank, int64_t n, double lambda,
                               float* d_XtX_out, double* d_sumsq_out, void* stream);

/* The same, and *d_absmax_inout = max(*d_absmax_inout, max |X|) (device float, nullable; the caller zeroes it before the
 * first block): the matrix is read here anyway.  What it is for: the long-row kernel of the implicit half-iteration
 * (wrmf_ne.hip) scales its fp16 operands by a power of two taken from max |X|, which it otherwise finds by scanning X
 * once per half-iteration call -- see d_absmax of rsparse_hip_als_implicit_device. */
int rsparse_hip_gramian_absmax_device(const float* d_X, int rank, int64_t n, double lambda, float* d_XtX_out,
                                      double* d_sumsq_out, float* d_absmax_inout, void* stream);

/* One implicit half-iteration over the columns of `conf` (als_implicit<float>, no-bias branch).
 * d_Y points at column 0 of this matrix's block (rank x n_cols).  Writes to d_loss_rows_out
 * (nullable, device double[1]) the un-normalised row part of the loss:
 *     sum_i [ sum_j c_ij (1 - y_i.x_j)^2 + lambda |y_i|^2 ]          (wrmf_implicit.hpp:259-261)
 * the caller adds lambda*sum(X^2) and divides by nnz (:286-304) -- kept separate so that shards
 * on several GPUs can be summed.  Asynchronous on `stream`.
 * d_absmax (nullable, device float[1]): max |X| if the caller knows it (rsparse_hip_gramian_absmax_device yields it; a
 * sharded driver passes the all-reduced maximum of its ranks' blocks and solves all its sub-blocks under it).  Any
 * value >= the true maximum is correct, a tight one is accurate; it must stay valid until the call has executed on
 * `stream`.  NULL: the library scans X (0.5 ms per GB).  Per call, no state is kept. */
int rsparse_hip_als_implicit_device(const rsparse_hip_csc* conf, const float* d_X, float* d_Y,
                                    const float* d_XtX, int rank, double lambda, unsigned solver,
                                    unsigned cg_steps, const float* d_absmax, double* d_loss_rows_out, void* stream);

/* One explicit half-iteration (als_explicit<float>, no-bias branch).  Loss row part:
 *     sum_i [ sum_j (r_ij - y_i.x_j)^2 + lambda_use_i |y_i|^2 ]      (wrmf_explicit.hpp:131-132) */
int rsparse_hip_als_explicit_device(const rsparse_hip_csc* conf, const float* d_X, float* d_Y,
                                    int rank, double lambda, unsigned solver, unsigned cg_steps,
                                    int dynamic_lambda, double* d_loss_rows_out, void* stream);

/* als_implicit<T> with_biases = TRUE, global_bias = 0, Cholesky or NNLS (inst/include/wrmf_implicit.hpp:114-154,
 * 186-252,256-270), device-resident form.  Layout of X / Y as for the explicit variant below.  d_XtX is the
 * (rank-1) x (rank-1) Gramian of X without its x_bias row, ridge included (R/model_WRMF.R:463-486; use
 * rsparse_hip_gramian_device on the re-packed matrix).  Every row is solved, empty ones too (:178).  solver =
 * conjugate_gradient -> RSPARSE_HIP_ERR_UNSUPPORTED: the reference drops a row of the warm start twice on that path
 * (:189,197) and cannot run it.  The regulariser on X (all rows but the ones, :287-297) is the caller's. */
int rsparse_hip_als_implicit_bias_device(const rsparse_hip_csc* conf, const float* d_X, float* d_Y,
                                         const float* d_XtX, int rank, double lambda, unsigned solver,
                                         int is_x_bias_last_row, double* d_loss_rows_out, void* stream);

/* als_implicit<T> with a global bias (inst/include/wrmf_implicit.hpp:108-112,146-157,228-229,262-270),
 * device-resident form; with_biases selects the user/item-bias layout of rsparse_hip_als_implicit_bias_device (then
 * rhs_init = -X' (x_b + global_bias), :152; Cholesky / NNLS only), otherwise X / Y / XtX are the plain rank x n matrices
 * and every right-hand side gets global_bias_base = -global_bias * rowSums(X) (:111-112, computed on the device); every
 * column is solved, empty ones too (:178).  The loss compares x_j.y with 1 - global_bias (- x_b).  solver =
 * conjugate_gradient (no biases): cg_solver_implicit_global_bias (:35-57, 203) from the warm start in d_Y, cg_steps
 * steps.  global_bias itself is the caller's: sum(x) / (sum(x) + n_user n_item - nnz), R/model_WRMF.R:286-287.
 * double_threshold: which build's cut-off applies to a small global bias (:108-109) -- 0 = als_implicit<float>'s
 * sqrt(FLT_EPSILON) = 3.45e-4, non-zero = als_implicit<double>'s 1.49e-8 (a model declared with precision = "double" whose
 * arithmetic runs on this fp32 layer: on large sparse data sum / (sum + n_user n_item - nnz) is typically below 3.45e-4,
 * and the double build keeps it).  d_absmax: as for rsparse_hip_als_implicit_device. */
int rsparse_hip_als_implicit_global_bias_device(const rsparse_hip_csc* conf, const float* d_X, float* d_Y,
                                                const float* d_XtX, int rank, double lambda, unsigned solver,
                                                unsigned cg_steps, int with_biases, int is_x_bias_last_row,
                                                double global_bias, int double_threshold, const float* d_absmax,
                                                double* d_loss_rows_out, void* stream);

/* initialize_biases_implicit (inst/include/wrmf_utils.hpp:86-165; .Call _rsparse_initialize_biases_{double,float} with
 * is_explicit_feedback = FALSE).  calculate_global_bias: sum(x) / (sum(x) + n_users n_items - nnz) (:90-93), subtracted
 * inside the sweeps (:142,157) and returned through global_bias_out (may be NULL). */
int rsparse_hip_initialize_biases_implicit_device(const rsparse_hip_csc* c_ui, const rsparse_hip_csc* c_iu,
                                                  float* d_user_bias, float* d_item_bias, double lambda,
                                                  int non_negative, int calculate_global_bias,
                                                  double* global_bias_out, void* stream);

/* als_explicit<T> with_biases = TRUE (inst/include/wrmf_explicit.hpp:41-64,86-91,113-127), device-resident form.
 * rank counts the two extra coordinates (R/model_WRMF.R:160: rank + 2): X = [1, ..., x_bias] and
 * Y = [y_bias, ..., 1] when is_x_bias_last_row, X = [x_bias, ..., 1] and Y = [1, ..., y_bias] otherwise; the
 * placeholder entry of every Y row is left untouched.  d_loss_rows_out as for rsparse_hip_als_explicit_device;
 * the regulariser on X skips the row of ones (:147-159) and is the caller's (rsparse_hip_weighted_sumsq_device on
 * the other rank-1 rows). */
int rsparse_hip_als_explicit_bias_device(const rsparse_hip_csc* conf, const float* d_X, float* d_Y, int rank,
                                         double lambda, unsigned solver, unsigned cg_steps, int dynamic_lambda,
                                         int is_x_bias_last_row, double* d_loss_rows_out, void* stream);

/* with_global_bias without user/item biases, explicit feedback (R/model_WRMF.R:278-282): global_bias = mean(c_ui@x),
 * removed in place from the resident values of both orientations (d_x_other may be NULL).  *mean_out is a host double. */
int rsparse_hip_values_subtract_mean_device(int64_t n, float* d_x, float* d_x_other, double* mean_out, void* stream);

/* initialize_biases_explicit (inst/include/wrmf_utils.hpp:32-84; .Call _rsparse_initialize_biases_{double,float} with
 * is_explicit_feedback = TRUE, src/RcppExports.cpp:417-454).  c_ui: users x items by item column, c_iu: its transpose.
 * With calculate_global_bias the mean of the values is removed from the resident values of BOTH handles in place (as
 * the reference does to ConfCSC / ConfCSR) and returned in *global_bias_out (host).  d_user_bias [n_users] (read as
 * the starting point, the R driver passes zeros) and d_item_bias [n_items] are device vectors. */
int rsparse_hip_initialize_biases_explicit_device(rsparse_hip_csc* c_ui, rsparse_hip_csc* c_iu, float* d_user_bias,
                                                  float* d_item_bias, double lambda, int dynamic_lambda,
                                                  int non_negative, int calculate_global_bias,
                                                  double* global_bias_out, void* stream);

/* The bias initialisation one sweep at a time, over ONE block of columns: for drivers that shard the matrix (every rank
 * owns a block of items and a block of users and holds both bias vectors in full, exchanging the swept block after each
 * sweep).  initialize_biases_explicit (inst/include/wrmf_utils.hpp:54-82) is five times
 *     item sweep: item_bias[c] = sum_{e in c} (x_e - user_bias[idx_e]) / (lambda_use + n_c)     then the same for the users;
 * initialize_biases_implicit (:86-165) is, once, means / adjustments per column (prep; n_other = the TRUE size of the other
 * side), then five times an item sweep and a user sweep of the weighted running mean (:136-143, 152-159), each given the
 * SUM of the other side's current biases (d_other_sum, device double[1]; NULL = 0: the first item sweep, :131-135).
 * d_other_bias is indexed by conf's row indices; d_out / d_means / d_adj by conf's columns. */
int rsparse_hip_bias_sweep_explicit_device(const rsparse_hip_csc* conf, const float* d_other_bias, double lambda,
                                           int dynamic_lambda, int non_negative, float* d_out, void* stream);
int rsparse_hip_bias_prep_implicit_device(const rsparse_hip_csc* conf, int n_other, double lambda, double* d_means,
                                          double* d_adj, void* stream);
int rsparse_hip_bias_sweep_implicit_device(const rsparse_hip_csc* conf, const float* d_other_bias, int n_other,
                                           const double* d_other_sum, const double* d_means, const double* d_adj,
                                           int non_negative, double global_bias, float* d_out, void* stream);

/* sum_j w_j |X[:,j]|^2 on the device (w = NULL -> 1): the regulariser terms
 * lambda*accu(X%X) and lambda*accu((X%X)*cnt_X) (wrmf_explicit.hpp:160-170). */
int rsparse_hip_weighted_sumsq_device(const float* d_X, int rank, int64_t n, const float* d_w,
                                      double* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * `$predict`: top-k of the dense product (next step after the solve on the same operator boundary)
 * ---------------------------------------------------------------------------------------------- */

#define RSPARSE_HIP_NA_INTEGER INT32_MIN /* R's NA_integer_: fewer than k admissible items */
/* k up to RSPARSE_HIP_MAX_TOPK runs the fused path (wrmf_topk.hip: candidates in LDS / a per-workgroup scratch while the items
 * stream past); RSPARSE_HIP_MAX_TOPK < k <= RSPARSE_HIP_MAX_TOPK_LARGE runs the large-k path (wrmf_topk_large.hip): per chunk of
 * users the scores go to a key matrix in the workspace, a radix select finds every user's kc-th key, the items at or above it are
 * ordered in LDS (re-scored in double by the f64 form) and users whose list overflows (exact ties) replay the reference's heap.
 * Its workspace (the library's grow-only pad buffer) is chunk x (round_up(n_items, 4) + 2052 + 2 x cap) words with
 * cap = min(10240, max(the power of two >= k, round_up(2 kc, 256))) and chunk = the users that fit 2 GiB (at most 32768):
 * 2 GiB for any call with more than a few hundred users over a million items.  k above RSPARSE_HIP_MAX_TOPK_LARGE ->
 * ERR_UNSUPPORTED. */
#define RSPARSE_HIP_MAX_TOPK 256
#define RSPARSE_HIP_MAX_TOPK_LARGE 8192

/* replaces top_product (src/matrix_top_product.cpp:20-102; .Call `_rsparse_top_product`,
 * R/RcppExports.R).  x: nr x rank and y: rank x nc, both column-major doubles as arma::mat holds them;
 * not_recommend as dgRMatrix slots p (nr+1) / j (sorted per row), NULL = nothing to filter; exclude: 1-based
 * item indices excluded for every row.  res: nr x k column-major 1-based indices (NA_integer_ where fewer
 * than k items are admissible), scores: nr x k column-major (+ glob_mean), best first; equal scores keep the
 * reference's order (larger index first).  The candidates (k + max(8, k / 4) per row) come from an fp32 matrix-core pass,
 * their scores are recomputed in double from x and y as given and the reference's heap is replayed over them
 * (rsparse_hip_top_product_f64_device below).  k > 8192 -> ERR_UNSUPPORTED.  n_threads is accepted and ignored. */
int rsparse_hip_top_product(const double* x, const double* y, int nr, int nc, int rank, unsigned k,
                            unsigned n_threads, const int32_t* not_recommend_p,
                            const int32_t* not_recommend_j, const int32_t* exclude, int n_exclude,
                            double glob_mean, int32_t* res, double* scores);

/* device-resident form: d_U n_users x rank and d_V n_items x rank row-major fp32 (= rank x n column-major),
 * d_exclude0: sorted 0-based item indices, d_res / d_scores: n_users x k row-major.
 * A call for more than 128 users (rank <= 128) keeps its per-user candidate buffers in the library's grow-only workspace:
 * min(n_users, 131072) x 2 x (k + 32 + max(64, k)) words, 121 MB at k = 10, 570 MB at k = 256; longer calls run in chunks of
 * 131072 users on the stream and reuse it.  256 < k <= 8192: the large-k path (above) on the fp32 scores, kc = k. */
int rsparse_hip_top_product_device(const float* d_U, const float* d_V, int n_users, int n_items, int rank,
                                   int k, const int32_t* d_not_recommend_p, const int32_t* d_not_recommend_j,
                                   const int32_t* d_exclude0, int n_exclude, double glob_mean,
                                   int32_t* d_res, float* d_scores, void* stream);

/* `$predict` that ORDERS like the reference.  find_top_product casts both factor matrices to double before the product
 * (R/utils.R:35-36) and top_product takes arma::mat (src/matrix_top_product.cpp:20): the fp32 pass above only nominates -- it keeps
 * the k + extra best items of every user (extra < 0: max(8, k / 4); never more than 256 candidates for k <= 256, 10240 for the
 * large-k path) --, their scores are
 * recomputed in double from d_U64 / d_V64 (n x rank row-major doubles; both NULL: from the fp32 factors widened) and the
 * reference's heap is replayed over the candidates in ascending item order: strict `>` replacement, equal scores with the
 * larger index first, and when more candidates sit AT the k-th score than places, the ones the reference's heap keeps.
 * Exact whenever every item whose double score reaches the k-th best is among the candidates.  d_scores: n_users x k doubles. */
int rsparse_hip_top_product_f64_device(const float* d_U, const float* d_V, const double* d_U64, const double* d_V64,
                                       int n_users, int n_items, int rank, int k, int extra,
                                       const int32_t* d_not_recommend_p, const int32_t* d_not_recommend_j,
                                       const int32_t* d_exclude0, int n_exclude, double glob_mean, int32_t* d_res,
                                       double* d_scores, void* stream);

/* Which kernels a call of rsparse_hip_top_product_device (rescore = 0) or rsparse_hip_top_product_f64_device (rescore = 1, `extra`
 * as there; the stateless rsparse_hip_top_product is that call with extra = -1) of this shape launches: one text line per launch of a
 * product kernel, in order, "family=per_wave|shared|pipe KP= UB= W= buffers=lds|global users= threads= lds= k= user0= n_users=
 * grid=XxY slice_items= flagged= scratch_floats=" -- the padded rank, user blocks per wave, waves, where the candidate buffers live,
 * users per workgroup, threads, LDS bytes, the k of this launch, its users, its grid (Y = item slices), and whether it is a re-run
 * for flagged users (its workgroups return at once when nobody is flagged); scratch_floats: the workspace the call takes.  No
 * device call: the launch plan is host arithmetic, like the launch configuration rsparse_hip_csc_info reports.  text_len too small
 * -> ERR_INVALID; rank > 256 or k > 256 (the large-k path is not planned here) -> ERR_UNSUPPORTED. */
int rsparse_hip_top_product_plan(int n_users, int n_items, int rank, int k, int extra, int rescore, char* text, int text_len);

/* `$predict` WITHIN per-user candidate lists (two-stage serving, sampled-negative evaluation): what find_top_product returns when
 * every item that is not a stored position of the user's row of the candidate pattern is added to that user's not_recommend row.
 * d_cand_p (n_users + 1) / d_cand_j: the pattern as CSR slots, columns ascending and unique within a row; slots are absolute
 * positions into d_cand_j, so a caller may pass a slice of a larger pattern's row pointers.  d_not_recommend_p / _j (columns
 * ascending within a row; NULL = nothing) and d_exclude0 (ascending 0-based items) as above.  Admissible: candidates minus
 * not_recommend minus exclude.  The scores are those of rsparse_hip_score_pairs*_device at the same cells with add = glob_mean (the
 * double sum of the factors as they are, fp32 or fp64), the order is by exactly these doubles (-0 and +0 tie): best first, equal
 * scores with the larger index first, and at the k-th score the items the reference's heap keeps.  Exact: no nomination pass, no
 * margin, no overflow path; work and workspace (8 bytes + 1 bit per candidate, 8 bytes per user, in the library's grow-only
 * buffer) follow the number of candidates, not n_users x n_items.  d_res: n_users x k row-major, 1-based, NA_integer_ where fewer
 * than k candidates are admissible (d_scores NaN there).  1 <= k <= RSPARSE_HIP_MAX_TOPK_LARGE.  The call reads the two ends of
 * d_cand_p back (it waits for the stream once).
 * NULL where a pointer is required, n_users < 0, n_items < 0, rank < 1, k < 1, n_exclude < 0, row pointers that are negative or
 * end below their start -> ERR_INVALID; rank > RSPARSE_HIP_MAX_RANK (fp32) / RSPARSE_HIP_MAX_RANK_F64 (f64) or
 * k > RSPARSE_HIP_MAX_TOPK_LARGE -> ERR_UNSUPPORTED; all before any launch.  A column outside [0, n_items) breaks the
 * precondition: its score is NaN and nothing outside the factors is read for it. */
int rsparse_hip_top_candidates_device(const float* d_U, const float* d_V, int n_users, int n_items, int rank, int k,
                                      const int32_t* d_cand_p, const int32_t* d_cand_j, const int32_t* d_not_recommend_p,
                                      const int32_t* d_not_recommend_j, const int32_t* d_exclude0, int n_exclude,
                                      double glob_mean, int32_t* d_res, double* d_scores, void* stream);
int rsparse_hip_top_candidates_f64_device(const double* d_U, const double* d_V, int n_users, int n_items, int rank, int k,
                                          const int32_t* d_cand_p, const int32_t* d_cand_j, const int32_t* d_not_recommend_p,
                                          const int32_t* d_not_recommend_j, const int32_t* d_exclude0, int n_exclude,
                                          double glob_mean, int32_t* d_res, double* d_scores, void* stream);
/* the host-pointer form, shaped like rsparse_hip_top_product so that R can bind it: x, y, exclude, res, scores as there; cand_p /
 * cand_j and not_recommend_p / _j: dgRMatrix slots over the rows of x, 0-based columns.  cand_p[0] != 0, decreasing row pointers,
 * a candidate column outside [0, nc) or not strictly ascending within its row -> ERR_INVALID (checked on the host); rank >
 * RSPARSE_HIP_MAX_RANK_F64 -> ERR_UNSUPPORTED (the doubles are used as given).  not_recommend rows need not be sorted here. */
int rsparse_hip_top_candidates(const double* x, const double* y, int nr, int nc, int rank, unsigned k, unsigned n_threads,
                               const int32_t* cand_p, const int32_t* cand_j, const int32_t* not_recommend_p,
                               const int32_t* not_recommend_j, const int32_t* exclude, int n_exclude, double glob_mean,
                               int32_t* res, double* scores);

/* ------------------------------------------------------------------------------------------------
 * `$get_similar_items`: item-to-item cosine top-k (R/MatrixFactorizationRecommender.R:79-116)
 * ---------------------------------------------------------------------------------------------- */

/* The reference normalises the item embeddings once (L2 norm of every item's vector) and answers one item at a time with a
 * product against all of them.  Here: the normalised matrix is prepared once per model (rsparse_hip_normalize_items*_device),
 * and a batch of query items is ONE call of the `$predict` path above against it -- cosine(i, j) is the dot product of two unit
 * vectors, so fp32 nomination, re-scoring and ordering in double, the tie rule (larger index first) and both k ranges are
 * rsparse_hip_top_product_f64_device's, unchanged.
 *
 * rsparse_hip_normalize_items_device (fp32 factors) / rsparse_hip_normalize_items_f64_device (fp64 factors): d_V is
 * n_items x ld row-major (= ld x n_items column-major); the columns [c0, c1) are the latent coordinates (a model with user/item
 * biases keeps the item bias and the constant one outside the window), r = c1 - c0.  Per item the sum of squares over the window
 * is accumulated in double whatever the input type; d_Vn64 (n_items x r doubles, compact) = V[item, c0:c1] / sqrt(sum),
 * d_Vn32 = (float)d_Vn64, d_flags[item] = 0.  An item whose sum of squares is zero or not finite is DEGENERATE: its rows are
 * written as zeros and d_flags[item] = 1 (items without interactions keep zero factors under the conjugate-gradient solver, so
 * this is an ordinary case).  One streaming launch on `stream`: 4 r or 8 r bytes read, 12 r written per item.
 * not 0 <= c0 < c1 <= ld, n_items < 0, NULL where needed -> ERR_INVALID; r > RSPARSE_HIP_MAX_RANK -> ERR_UNSUPPORTED. */
int rsparse_hip_normalize_items_device(const float* d_V, int n_items, int ld, int c0, int c1, float* d_Vn32, double* d_Vn64,
                                       int32_t* d_flags, void* stream);
int rsparse_hip_normalize_items_f64_device(const double* d_V, int n_items, int ld, int c0, int c1, float* d_Vn32,
                                           double* d_Vn64, int32_t* d_flags, void* stream);

/* The k most similar items of n_q query items.  d_Vn32 / d_Vn64: the prepared operands (n_items x r); d_query: 0-based item ids
 * (repeats allowed); exclude_self != 0 removes every query from its own list; d_exclude0: sorted 0-based ids that are never
 * returned -- the caller puts the degenerate items there (the non-zeros of d_flags) next to its own exclusions.
 * d_res (n_q x k row-major, 1-based, NA_integer_ where fewer than k items are admissible) and d_scores (n_q x k doubles, the
 * cosines, best first, NaN beside NA_integer_).  A query that is degenerate (its row of d_Vn64 is all zeros) or out of range
 * gets a row of NA_integer_ / NaN; nothing is read out of bounds for it.  Asynchronous on `stream`.
 * Workspace (grow-only): the queries are scored in batches of 262144 (fewer above k = 256: the same rule as the callers of
 * rsparse_hip_top_product_f64_device use, so its workspace bounds above hold), and a batch keeps its gathered operands and
 * self-exclusion slots, min(n_q, batch) x (12 r + 12) bytes: 406 MB for a full batch at r = 128.
 * NULL where needed, n_items < 0, n_q < 0, k < 1, r < 1, n_exclude < 0 -> ERR_INVALID; r > RSPARSE_HIP_MAX_RANK or
 * k > RSPARSE_HIP_MAX_TOPK_LARGE -> ERR_UNSUPPORTED. */
int rsparse_hip_similar_items_device(const float* d_Vn32, const double* d_Vn64, int n_items, int r, const int32_t* d_query,
                                     int n_q, int k, int exclude_self, const int32_t* d_exclude0, int n_exclude,
                                     int32_t* d_res, double* d_scores, void* stream);

/* host form: components as R holds it (rank x n_items column-major doubles); the latent rows are first_row (0-based) ..
 * first_row + n_rows - 1 (all of them: 0, rank; a model with user/item biases: 1, rank - 2).  query (n_q) and exclude
 * (n_exclude; out-of-range entries are ignored, as rsparse_hip_top_product does) are 1-based item indices; res / scores are
 * n_q x k column-major like rsparse_hip_top_product's.  Degenerate items are excluded by the call itself.  A query id outside
 * 1..n_items, or first_row / n_rows outside components -> ERR_INVALID (before a device is touched, like every check above). */
int rsparse_hip_similar_items(const double* components, int rank, int n_items, int first_row, int n_rows, const int32_t* query,
                              int n_q, int k, int exclude_self, const int32_t* exclude, int n_exclude, int32_t* res,
                              double* scores);

/* ------------------------------------------------------------------------------------------------
 * ranking metrics of the `$predict` lists: ap_k() / ndcg_k() (R/metrics.R:31-127, NAMESPACE)
 * ---------------------------------------------------------------------------------------------- */

/* replaces the per-user loops of ap_k / ndcg_k.  predictions: n_users x k column-major 1-based item indices with NA_integer_
 * (R's integer matrix, what rsparse_hip_top_product writes); actual: the dgRMatrix slots p (n_users + 1), j (sorted 0-based
 * columns), x (relevances).  Per user, kk = min(k, stored entries of the row): ap = the mean over positions 1..kk of the hits
 * so far / position; ndcg = dcg / idcg over the first kk positions (idcg = 1 for an empty row; ap of an empty row is NaN).
 * NA, out-of-range and repeated predictions are looked up one by one like `%in%` / `match`; stored zeros are relevant items
 * of relevance 0.  Double arithmetic with a fixed reduction order: a repeated call returns the same bits.  Either output may
 * be NULL, not both; actual_x is read only for ndcg_out.  NULL where needed, n_users < 0, k < 1, p[0] != 0, a decreasing p or
 * j not strictly ascending within a row -> ERR_INVALID; k > RSPARSE_HIP_MAX_TOPK_LARGE -> ERR_UNSUPPORTED (the R loop
 * stays, as for k = 0). */
int rsparse_hip_ranking_metrics(const int32_t* predictions, int n_users, int k, const int32_t* actual_p,
                                const int32_t* actual_j, const double* actual_x, double* ap_out, double* ndcg_out);

/* device-resident form: d_predictions n_users x k ROW-major, as rsparse_hip_top_product_{,f64_}device write them; outputs
 * n_users doubles.  Enqueued on `stream`, no synchronisation.  Same status codes, except that a valid p and j strictly
 * ascending within every row are preconditions here, not checked (they live on the device).  Keeps n_users + 1 ints of the
 * library's grow-only workspace. */
int rsparse_hip_ranking_metrics_device(const int32_t* d_predictions, int n_users, int k, const int32_t* d_actual_p,
                                       const int32_t* d_actual_j, const double* d_actual_x, double* d_ap_out,
                                       double* d_ndcg_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * hit-based metrics of the same lists at several cutoffs in one pass: precision, recall, hit rate, reciprocal rank
 * and catalogue coverage.  The reference package has none of them: `hit_metrics_reference` of rsparse_amd/metrics.py
 * is the definition.
 * ---------------------------------------------------------------------------------------------- */

/* cutoffs: n_cutoffs <= RSPARSE_HIP_MAX_CUTOFFS strictly ascending integers c_1 < ... < c_T in 1 .. k, always on the HOST (they
 * travel as a kernel argument).  Per user u with n_u stored entries in its row of actual (p / j as above; the values play no
 * part, a stored zero is a relevant item), hit_i = the prediction at the 1-based position i is a stored column of the row --
 * looked up on its own, as for ap: NA, indices below 1 or outside the row are misses, a repeated index hits every time --:
 *   hits[u, t]      = sum over i <= c_t of hit_i                    first[u] = the smallest i <= c_T with hit_i, 0 without one
 *   precision[u, t] = hits / c_t  (c_t also where the list is shorter)            recall[u, t] = hits / n_u
 *   hit[u, t]       = 1 where hits > 0, else 0                      mrr[u, t] = 1 / first where 0 < first <= c_t, else 0
 * A user with n_u = 0 gets NaN in the four doubles (it is not evaluated, as in ap) and hits = first = 0.  Over ALL users, those
 * with n_u = 0 included: first_seen[item] = min(first_seen[item], the smallest position i <= c_T at which a list names the
 * item); only items in 1 .. n_items count.  The catalogue coverage at c_t is #{items with first_seen <= c_t} / n_items, left to
 * the caller.  Positions beyond c_T are never read.  Every double is one IEEE division of two integers and the only atomics
 * are integer minima: a repeated call returns the same bits, and they are the bits of the numpy statement.
 *
 * device form: d_predictions n_users x k ROW-major (k is the row stride), d_hits and the four doubles n_users x n_cutoffs
 * row-major, d_first n_users, d_first_seen n_items; every output nullable, not all.  d_first_seen is min-updated and
 * caller-initialised (INT32_MAX = never listed): calling the entry on successive row batches with the same d_first_seen
 * accumulates the coverage of all of them.  Enqueued on `stream`, no synchronisation, no workspace.  All before a device is
 * touched: NULL where a pointer is needed, every output NULL, n_users < 0, k < 1, n_cutoffs < 1, cutoffs not strictly ascending,
 * below 1 or above k, d_first_seen with n_items < 1 -> ERR_INVALID; n_cutoffs > RSPARSE_HIP_MAX_CUTOFFS or
 * k > RSPARSE_HIP_MAX_TOPK_LARGE -> ERR_UNSUPPORTED; n_users == 0 -> OK.  A valid p and j strictly ascending within every row
 * are preconditions, as for rsparse_hip_ranking_metrics_device. */
#define RSPARSE_HIP_MAX_CUTOFFS 16
int rsparse_hip_hit_metrics_device(const int32_t* d_predictions, int n_users, int k, const int32_t* d_actual_p,
                                   const int32_t* d_actual_j, const int32_t* cutoffs, int n_cutoffs, int32_t* d_hits,
                                   int32_t* d_first, double* d_precision, double* d_recall, double* d_hit, double* d_mrr,
                                   int32_t* d_first_seen, int n_items, void* stream);

/* host form: predictions as rsparse_hip_ranking_metrics takes them (n_users x k column-major, 1-based with NA_integer_), the
 * dgRMatrix slots p / j, and the same outputs as n_users x n_cutoffs COLUMN-major matrices (first: n_users).  first_seen
 * (n_items) is initialised by the call itself (INT32_MAX) and returned min-updated.  Also ERR_INVALID: p[0] != 0, a decreasing
 * p, j not strictly ascending within a row. */
int rsparse_hip_hit_metrics(const int32_t* predictions, int n_users, int k, const int32_t* actual_p, const int32_t* actual_j,
                            const int32_t* cutoffs, int n_cutoffs, int32_t* hits, int32_t* first, double* precision,
                            double* recall, double* hit, double* mrr, int32_t* first_seen, int n_items);

/* ------------------------------------------------------------------------------------------------
 * beyond-accuracy metrics of the same lists at the same cutoffs: popularity, novelty, exposure of the catalogue and
 * intra-list diversity.  The reference package has none of them: `list_metrics_reference` and
 * `list_diversity_reference` of rsparse_amd/metrics.py are the definitions.
 * ---------------------------------------------------------------------------------------------- */

/* Lists and cutoffs as for rsparse_hip_hit_metrics*.  A position is VALID when its item lies in 1 .. n_items; NA_integer_ and
 * anything else is skipped, a repeated item counts wherever it stands.  item_count: int32 of n_items, values >= 0 (e.g. the
 * interactions of every item in the training matrix).  item_info: int64 of n_items, fixed point in units of 2^-32, values
 * 0 <= v < 2^40 (e.g. the items' self-information in bits), so that a sum over 8192 positions stays below 2^53.
 *   valid[u, t]      = #{valid positions i <= c_t}  (int32)
 *   count_sum[u, t]  = sum of item_count[item_i] over them  (int64)      popularity = double(count_sum) / double(valid)
 *   info_sum[u, t]   = sum of item_info[item_i] over them   (int64)      novelty    = double(info_sum) / double(valid 2^32)
 * popularity and novelty are NaN where valid = 0; every double is one IEEE division of two exactly converted integers.
 * exposure[b, item] += 1 for every valid position i with c_(b-1) < i <= c_b, over all users: the histogram per cutoff INTERVAL.
 *
 * device form: d_predictions n_users x k ROW-major; the five per-row outputs n_users x n_cutoffs row-major; d_exposure
 * n_cutoffs x n_items int32, caller-ZEROED: calls on successive row batches accumulate, and the caller cumulates along b
 * afterwards (exposure at c_t = the sum of the intervals 1 .. t).  Every output is nullable, not all; a table is read only when it
 * is not NULL, and d_count_sum / d_popularity need d_item_count, d_info_sum / d_novelty need d_item_info.  Integer atomics only
 * and no floating-point sum: a repeated call returns the same bits.  Enqueued on `stream`, no synchronisation, no workspace.
 * All before a device is touched: NULL where a pointer is needed, every output NULL, n_users < 0, k < 1, n_cutoffs < 1, bad
 * cutoffs, n_items < 1 -> ERR_INVALID; n_cutoffs > RSPARSE_HIP_MAX_CUTOFFS or k > RSPARSE_HIP_MAX_TOPK_LARGE ->
 * ERR_UNSUPPORTED; n_users == 0 -> OK.  The value ranges of the two tables are preconditions here. */
int rsparse_hip_list_metrics_device(const int32_t* d_predictions, int n_users, int k, const int32_t* cutoffs, int n_cutoffs,
                                    const int32_t* d_item_count, const int64_t* d_item_info, int n_items, int32_t* d_valid,
                                    int64_t* d_count_sum, int64_t* d_info_sum, double* d_popularity, double* d_novelty,
                                    int32_t* d_exposure, void* stream);

/* host form: predictions n_users x k column-major (1-based, NA_integer_), the per-row outputs n_users x n_cutoffs COLUMN-major,
 * exposure n_items x n_cutoffs column-major, initialised by the call and returned CUMULATED: exposure[item, t] = the valid
 * positions i <= c_t that name the item.  Also ERR_INVALID: item_count < 0, item_info outside 0 <= v < 2^40. */
int rsparse_hip_list_metrics(const int32_t* predictions, int n_users, int k, const int32_t* cutoffs, int n_cutoffs,
                             const int32_t* item_count, const int64_t* item_info, int n_items, int32_t* valid,
                             int64_t* count_sum, int64_t* info_sum, double* popularity, double* novelty, int32_t* exposure);

/* d_inv[item] = 1 / sqrt(sum of squares of V[item, c0 : c1)) in double, 0.0 for a DEGENERATE item (sum zero or not finite: the
 * rule of rsparse_hip_normalize_items*_device; the zero is the flag).  d_V n_items x ld row-major, fp32 or fp64; one streaming
 * launch, the squares summed in double in a fixed order.  not 0 <= c0 < c1 <= ld, n_items < 0, NULL where needed ->
 * ERR_INVALID; c1 - c0 > RSPARSE_HIP_MAX_RANK -> ERR_UNSUPPORTED. */
int rsparse_hip_item_inv_norms_device(const float* d_V, int n_items, int ld, int c0, int c1, double* d_inv, void* stream);
int rsparse_hip_item_inv_norms_f64_device(const double* d_V, int n_items, int ld, int c0, int c1, double* d_inv, void* stream);

/* Intra-list distance.  With u_j = V[j, c0 : c1) d_inv[j] (a unit vector; items with d_inv = 0 are skipped like invalid ones):
 *   counted[u, t]   = #{valid, non-degenerate positions i <= c_t} = m  (int32)
 *   diversity[u, t] = the mean over the pairs i < j of those positions of 1 - <u_i, u_j>; NaN where m < 2
 * computed as 1 - (|S|^2 - m) / (m (m - 1)) with S the sum of the m unit vectors, accumulated in double from the factors AS
 * STORED (r sizeof(T) bytes and one double gathered per position) in an order that depends on (k, cutoffs, c1 - c0) alone: a
 * repeated call returns the same bits.  It differs from the pairwise form by at most about 2 (2 m + r) 2^-53.  d_inv must be what
 * rsparse_hip_item_inv_norms*_device made of the same d_V, c0, c1.  Outputs n_users x n_cutoffs row-major, either nullable.
 * Status codes as rsparse_hip_list_metrics_device, and those of rsparse_hip_item_inv_norms*_device for c0 / c1 / ld. */
int rsparse_hip_list_diversity_device(const int32_t* d_predictions, int n_users, int k, const int32_t* cutoffs, int n_cutoffs,
                                      const float* d_V, int n_items, int ld, int c0, int c1, const double* d_inv,
                                      int32_t* d_counted, double* d_diversity, void* stream);
int rsparse_hip_list_diversity_f64_device(const int32_t* d_predictions, int n_users, int k, const int32_t* cutoffs,
                                          int n_cutoffs, const double* d_V, int n_items, int ld, int c0, int c1,
                                          const double* d_inv, int32_t* d_counted, double* d_diversity, void* stream);

/* host forms: predictions n_users x k column-major, V n_items x ld row-major (= R's ld x n_items components) on the host, the
 * outputs n_users x n_cutoffs COLUMN-major; the norms are made by the call. */
int rsparse_hip_list_diversity(const int32_t* predictions, int n_users, int k, const int32_t* cutoffs, int n_cutoffs,
                               const float* V, int n_items, int ld, int c0, int c1, int32_t* counted, double* diversity);
int rsparse_hip_list_diversity_f64(const int32_t* predictions, int n_users, int k, const int32_t* cutoffs, int n_cutoffs,
                                   const double* V, int n_items, int ld, int c0, int c1, int32_t* counted, double* diversity);

/* ------------------------------------------------------------------------------------------------
 * MMR re-ranking: a pool of n_pool ranked positions per user (what rsparse_hip_top_product*_device / top_candidates*_device
 * write: 1-based items with NA_integer_, double scores) greedily re-ranked down to k for relevance AND dissimilarity.  The
 * reference package has nothing like it: `mmr_reference` of rsparse_amd/metrics.py is the definition.
 * ---------------------------------------------------------------------------------------------- */

/* A position is VALID when its item lies in 1 .. n_items and its score is finite; a repeated item is a position of its own.
 * With u_i = V[item_i, c0 : c1) d_inv[item_i] in double (the zero vector where d_inv is 0: a degenerate item), and over the valid
 * positions of a row rel_i = (s_i - s_min) / (s_max - s_min) (all 0 where s_max == s_min), step t = 0, 1, .. picks the valid,
 * untaken position that maximises
 *   (1 - trade_off) rel_i - trade_off max_{j picked} <u_i, u_j>        (the max over nothing is 0)
 * -- the LOWER position wins a tie -- until k are picked or no valid position is left.  One workgroup per user runs the k steps;
 * the dot products are accumulated in double from the factors AS STORED in an order that depends on c1 - c0 alone, so the
 * objective of a position depends only on the bits of its row, its score and the set already picked: exact ties are exact, a
 * repeated call returns the same bits, no atomics.  Every pick maximises the definition's objective along the call's own path
 * to within about (c1 - c0 + 8) 2^-53.
 *   d_items[u, t]      the item picked at step t, 1-based; NA_integer_ where fewer than k positions are valid  (int32)
 *   d_scores_out[u, t] its own score s_i; NaN there                                                            (double)
 *   d_positions[u, t]  its position in the pool, 1-based; NA_integer_ there                                    (int32)
 *   d_objective[u, t]  the maximised value of step t; NaN there                                                (double)
 * device form: d_lists / d_scores n_users x n_pool ROW-major, the outputs n_users x k row-major, each nullable except d_items;
 * d_inv must be what rsparse_hip_item_inv_norms*_device made of the same d_V, c0, c1.  Enqueued on `stream`, no
 * synchronisation, no workspace.  All before a device is touched: NULL lists, scores, V, inverse norms or d_items, n_users < 0,
 * k < 1, k > n_pool, trade_off outside [0, 1] or not finite, n_items < 1, not 0 <= c0 < c1 <= ld -> ERR_INVALID; n_pool >
 * RSPARSE_HIP_MAX_TOPK_LARGE or c1 - c0 > RSPARSE_HIP_MAX_RANK -> ERR_UNSUPPORTED; n_users == 0 -> OK. */
int rsparse_hip_mmr_rerank_device(const int32_t* d_lists, const double* d_scores, int n_users, int n_pool, int k, double trade_off,
                                  const float* d_V, int n_items, int ld, int c0, int c1, const double* d_inv, int32_t* d_items,
                                  double* d_scores_out, int32_t* d_positions, double* d_objective, void* stream);
int rsparse_hip_mmr_rerank_f64_device(const int32_t* d_lists, const double* d_scores, int n_users, int n_pool, int k,
                                      double trade_off, const double* d_V, int n_items, int ld, int c0, int c1, const double* d_inv,
                                      int32_t* d_items, double* d_scores_out, int32_t* d_positions, double* d_objective,
                                      void* stream);

/* host forms: lists / scores n_users x n_pool column-major, V n_items x ld row-major (= R's ld x n_items components) on the
 * host, the outputs n_users x k COLUMN-major; the norms are made by the call. */
int rsparse_hip_mmr_rerank(const int32_t* lists, const double* scores, int n_users, int n_pool, int k, double trade_off,
                           const float* V, int n_items, int ld, int c0, int c1, int32_t* items, double* scores_out,
                           int32_t* positions, double* objective);
int rsparse_hip_mmr_rerank_f64(const int32_t* lists, const double* scores, int n_users, int n_pool, int k, double trade_off,
                               const double* V, int n_items, int ld, int c0, int c1, int32_t* items, double* scores_out,
                               int32_t* positions, double* objective);

/* ------------------------------------------------------------------------------------------------
 * full-ranking metrics: where the held-out items stand among ALL items -- the expected percentile rank of
 * Hu, Koren and Volinsky (the measure of the method's own paper), AUC and MRR off the same per-item ranks
 * ---------------------------------------------------------------------------------------------- */

/* For user u the ADMISSIBLE set A_u is the items outside the user's not_recommend row and outside exclude; n_adm = |A_u|.
 * Scores are the fp32 scores of the large-k `$predict` path (exact fp32 product on the matrix cores), compared through their
 * order-preserving keys: -0 and +0 are one score; a global bias shifts every score alike and plays no part; non-finite factors
 * are undefined here as in `$predict`.  For a stored entry (u, h) of `actual` (CSR slots p / j, j strictly ascending within a row;
 * stored zeros are entries):
 *   above = #{j in A_u : s_j > s_h},     tied = #{j in A_u, j != h : s_j == s_h};
 *   h not in A_u (or outside 0..n_items-1): the entry is INADMISSIBLE, above = tied = -1, and it takes no part in any sum.
 * The midrank is r_h = above + tied / 2 (0-based).  Per user, with P the admissible entries, w_h the stored values and sums over
 * the admissible entries:
 *   pct_h = r_h / (n_adm - 1)                                   (NaN when n_adm <= 1)
 *   mpr   = sum w_h pct_h / sum w_h                             (NaN when sum w_h == 0 or P == 0; the expected percentile rank)
 *   auc   = 1 - (sum r_h - P (P - 1) / 2) / (P (n_adm - P))     (NaN when P == 0 or n_adm == P; the pairs between two held-out
 *                                                                items add exactly P (P - 1) / 2 to sum r_h whatever their order)
 *   mrr   = 1 / (1 + min r_h)                                   (NaN when P == 0)
 *
 * rsparse_hip_held_out_ranks_device: d_U n_users x rank, d_V n_items x rank, row-major fp32 (a double model passes its fp32
 * replica, as for the nominating pass of `$predict`); d_not_recommend_p / _j as rsparse_hip_top_product_device (NULL = none),
 * d_exclude0 sorted 0-based; d_above / d_tied: int32, one per stored entry of actual; d_n_adm: int32, one per user.  Users run in
 * chunks whose key matrix (chunk x round_up(n_items, 4) words) stays within 2 GiB of the library's grow-only workspace, at most
 * 32768; max_chunk_users > 0 lowers the chunk (0: the plan).  A held-out row is counted RSPARSE_HIP_RANKS_BATCH entries at a
 * time.  Integer atomics only: a repeated call returns the same bits.  Enqueued on `stream`, no synchronisation.
 * NULL where needed, negative dimensions, rank < 1, max_chunk_users < 0 -> ERR_INVALID; rank > RSPARSE_HIP_MAX_RANK ->
 * ERR_UNSUPPORTED; n_users == 0 -> OK, no device is touched.  A valid p is a precondition, as for
 * rsparse_hip_ranking_metrics_device. */
#define RSPARSE_HIP_RANKS_BATCH 1024
int rsparse_hip_held_out_ranks_device(const float* d_U, const float* d_V, int n_users, int n_items, int rank,
                                      const int32_t* d_not_recommend_p, const int32_t* d_not_recommend_j,
                                      const int32_t* d_exclude0, int n_exclude, const int32_t* d_actual_p,
                                      const int32_t* d_actual_j, int max_chunk_users, int32_t* d_above, int32_t* d_tied,
                                      int32_t* d_n_adm, void* stream);

/* The per-user numbers from those counts, one wave per user, double arithmetic in a fixed order (per lane over its positions,
 * then a butterfly over the wave): d_mpr, d_auc, d_mrr (n_users doubles) and d_sums (n_users x 3 row-major: sum w, sum w pct, P
 * -- what the data-set numbers are summed from).  Any output may be NULL, not all four; d_actual_x (the weights) is read for
 * d_mpr and d_sums only.  NULL where needed, n_users < 0 -> ERR_INVALID; n_users == 0 -> OK. */
int rsparse_hip_rank_summary_device(int n_users, const int32_t* d_actual_p, const double* d_actual_x, const int32_t* d_above,
                                    const int32_t* d_tied, const int32_t* d_n_adm, double* d_mpr, double* d_auc, double* d_mrr,
                                    double* d_sums, void* stream);

/* host form, both steps: x (nr x rank) and y (rank x nc) column-major doubles and not_recommend as rsparse_hip_top_product takes
 * them (converted to fp32: the scores are the fp32 ones), exclude 1-based (out-of-range entries are ignored); actual as dgRMatrix
 * slots.  above / tied (one int32 per stored entry), n_adm (nr int32), mpr / auc / mrr (nr doubles), sums (nr x 3 row-major): any
 * may be NULL, not all.  Besides the checks above: actual_p[0] != 0, a decreasing p, j not strictly ascending within a row ->
 * ERR_INVALID, before a device is touched. */
int rsparse_hip_held_out_ranks(const double* x, const double* y, int nr, int nc, int rank, const int32_t* not_recommend_p,
                               const int32_t* not_recommend_j, const int32_t* exclude, int n_exclude, const int32_t* actual_p,
                               const int32_t* actual_j, const double* actual_x, int32_t* above, int32_t* tied, int32_t* n_adm,
                               double* mpr, double* auc, double* mrr, double* sums);

/* ------------------------------------------------------------------------------------------------
 * pointwise predictions: the model's values at given (row, column) pairs -- cpp_make_sparse_approximation
 * (src/utils.cpp:4-56, src/RcppExports.cpp)
 * ---------------------------------------------------------------------------------------------- */

/* Per stored position t of a CSR pattern (d_p: n_rows + 1, d_j: 0-based columns), row(t) the row that owns it:
 *   d_scores[t] = add + sum_c d_U[row(t), c] * d_V[d_j[t], c]        d_U: n_rows x r, d_V: n_cols x r, both row-major.
 * Accumulated in double whatever the factors' type: with fp32 factors every product is exact in double and only the sum rounds
 * (the product find_top_product orders by, R/utils.R:35-36); `add` (a global bias) goes on once at the end
 * (src/matrix_top_product.cpp:98-99).  With d_actual (one double per stored position) every row also gets
 *   d_sse[row] = sum (score - actual)^2,   d_sae[row] = sum |score - actual|     over its stored positions, 0 for an empty row.
 * Each of d_scores (p[n_rows] doubles), d_sse, d_sae (n_rows doubles) may be NULL, not all three; d_actual is read only for the
 * sums.  The reduction order is fixed and there are no atomics: a repeated call returns the same bits.
 * Enqueued on `stream` without synchronisation, with one exception: without d_scores the scores live in the library's grow-only
 * workspace (8 bytes per stored position), and to size it the call reads p[n_rows] back, which waits for `stream`.
 * A valid p (from 0, non-decreasing) and j in [0, n_cols) are preconditions, not checked (they live on the device), as for
 * rsparse_hip_ranking_metrics_device; a position whose column is outside [0, n_cols) gets NaN and nothing outside d_U and d_V is
 * read for it.  j need not be sorted and may repeat.
 * Every output NULL, NULL among d_U, d_V, d_p, d_j, d_sse / d_sae without d_actual, n_rows < 0, n_cols < 0, r < 1 -> ERR_INVALID;
 * r > RSPARSE_HIP_MAX_RANK (both element types: there is no per-row system to fit) -> ERR_UNSUPPORTED; n_rows == 0 -> OK, no
 * device is touched.  A pattern without stored positions scores nothing and zeroes d_sse / d_sae. */
int rsparse_hip_score_pairs_device(const float* d_U, const float* d_V, int n_rows, int n_cols, int r, const int32_t* d_p,
                                   const int32_t* d_j, double add, const double* d_actual, double* d_scores, double* d_sse,
                                   double* d_sae, void* stream);
int rsparse_hip_score_pairs_f64_device(const double* d_U, const double* d_V, int n_rows, int n_cols, int r, const int32_t* d_p,
                                       const int32_t* d_j, double add, const double* d_actual, double* d_scores, double* d_sse,
                                       double* d_sae, void* stream);

/* host form, the drop-in for cpp_make_sparse_approximation: the values of X^T Y at the stored positions of a template matrix of
 * n_rows x n_cols, given by its slots p and idx (dgRMatrix p / j with sparse_matrix_type = 2 (CSR), dgCMatrix p / i with 1
 * (CSC), as the reference numbers them).  X: rank x n_rows, Y: rank x n_cols, column-major doubles; values_out: one double per
 * stored position, in the template's own order.  Runs the f64 kernel (for CSC the two operands swap roles).
 * Another sparse_matrix_type, p[0] != 0, a decreasing p, an index outside the matrix, NULL where needed, negative dimensions,
 * rank < 1 -> ERR_INVALID, before a device is touched; rank > RSPARSE_HIP_MAX_RANK -> ERR_UNSUPPORTED. */
int rsparse_hip_sparse_approximation(int n_rows, int n_cols, const int32_t* p, const int32_t* idx, int sparse_matrix_type,
                                     const double* X, const double* Y, int rank, double* values_out);

/* ------------------------------------------------------------------------------------------------
 * soft-ALS (soft_svd / soft_impute, R/SoftALS.R): one half-iteration as one fused pass over a CSR matrix
 * ---------------------------------------------------------------------------------------------- */

/* Edges of the kernel (wrmf_softals.hip), for callers that test it: a wave walks its stored positions in chunks of
 * RSPARSE_HIP_SOFTALS_CHUNK, and no wave takes fewer than (RSPARSE_HIP_SOFTALS_SPLIT - 1) consecutive positions of the launch,
 * so a row of RSPARSE_HIP_SOFTALS_SPLIT entries or more is always split between waves (a shorter one may be, where it lies). */
#define RSPARSE_HIP_SOFTALS_CHUNK 256
#define RSPARSE_HIP_SOFTALS_SPLIT 1025

/* Per row of a CSR pattern (d_p: n_rows + 1 slots from 0, d_j: 0-based columns, d_x: the values), with d_M (n_cols x r) and
 * d_W (n_rows x r, nullable) row-major and w, s, t HOST vectors of r doubles (w and t nullable):
 *   res_t          = x_t - (w ? sum_c w[c] * d_W[row, c] * d_M[j_t, c] : 0)
 *   d_out[row, c]  = s[c] * sum_t res_t * d_M[j_t, c]  +  (t ? t[c] * d_W[row, c] : 0)
 *   *d_sumsq       = sum over all stored positions of res_t^2          (nullable, device double[1])
 * w = t = NULL, s = 1: the product CSR x dense.  w = t = NULL, s = d / (d + lambda): a half-iteration of soft_svd
 * (R/SoftALS.R:99-102).  w = d, t = s o d: a half-iteration of soft_impute with the `%*% diag(sqrt(d))` that follows it
 * (:68-94, :157, :174); (*d_sumsq + lambda sum(d)) / nnz is its loss (:83).
 * Every sum is accumulated in double for both element types and rounded once at the store.  No atomics: partial sums of a row
 * that is split are added in an order fixed by the pattern and the launch geometry, a repeated call returns the same bits.
 * j need not be sorted and may repeat; a row with a column outside [0, n_cols) comes out NaN (and so does *d_sumsq) and nothing
 * outside the operands is read for it; a row without stored positions gets t o W, or zeros.  A valid p is a precondition.
 * w, s, t are copied before the call returns; the call is enqueued on `stream` without synchronisation and uses the library's
 * grow-only workspace for the partial sums (calls on one host thread are ordered by their stream, as everywhere here).
 * NULL among d_p, d_j, d_x, d_M, d_out, s; w or t without d_W; n_rows < 0, n_cols < 0, r < 1 -> ERR_INVALID;
 * r > RSPARSE_HIP_MAX_RANK (both element types) -> ERR_UNSUPPORTED; n_rows == 0 -> OK; all before a device is touched. */
int rsparse_hip_softals_half_device(const int32_t* d_p, const int32_t* d_j, const float* d_x, const float* d_M, const float* d_W,
                                    int n_rows, int n_cols, int r, const double* w, const double* s, const double* t,
                                    float* d_out, double* d_sumsq, void* stream);
int rsparse_hip_softals_half_f64_device(const int32_t* d_p, const int32_t* d_j, const double* d_x, const double* d_M,
                                        const double* d_W, int n_rows, int n_cols, int r, const double* w, const double* s,
                                        const double* t, double* d_out, double* d_sumsq, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ItemKNN: the neighbours of every item by the co-occurrence of items, and top-k lists scored by them
 * ---------------------------------------------------------------------------------------------- */

/* The definition (rsparse_amd/itemknn.py states it in numpy).  B is the PATTERN of a users x items matrix in canonical CSR
 * (columns ascending and unique within a row; values are not looked at), n_j the number of users of item j, c_ij = (B^T B)_ij
 * for i != j, n_users <= 2^26 so that c^2 and n_i n_j are exact in double.  The order key of neighbour j of item i is ONE
 * division of two integers, evaluated in double:
 *     RSPARSE_HIP_KNN_COUNT    c / 1
 *     RSPARSE_HIP_KNN_COSINE   c^2 / (n_i n_j)         (the cosine is its square root, which the caller takes)
 *     RSPARSE_HIP_KNN_JACCARD  c / (n_i + n_j - c)
 * The neighbours of i are the K items j != i with c_ij > 0 of largest key, ties to the smaller j: `neighbors` (0-based, -1
 * where an item has fewer than K) and `counts` (c_ij, 0 in the padding), n x K row-major.  The device returns integers only.
 *
 * A user (a row of a pattern x) is scored with an integer weight table q (n_items x K, uint32, q <= 2^30 so that no sum
 * overflows; the caller makes it, e.g. rint(similarity * 2^30)):
 *     score_u[j] = sum of q[i, s] over the items i of the row and the slots s with neighbors[i, s] == j       (int64)
 * The list of u is the k items of largest score among those that are neither in the row's not_recommend entries nor in
 * items_exclude, ties to the smaller item; items of score 0 are ranked too, so a list is shorter than k only when fewer than k
 * items are admissible.
 *
 * Both entries accumulate into dense rows of a grow-only workspace of this host thread, a batch of rows at a time: rows per
 * batch = ws_rows, or with ws_rows = 0 what RSPARSE_HIP_KNN_WS_BYTES holds (at least one row; a row is n_items cells of 4
 * bytes for the neighbours, of 8 for the lists).  The scatter cuts the stored entries of a batch into spans of
 * RSPARSE_HIP_KNN_SPAN per wave whatever the row lengths; the select of a row keeps up to RSPARSE_HIP_KNN_LDS_CAND non-empty
 * cells on chip and falls back to a radix select over the dense row beyond that (wrmf_itemknn.hip).  Integer atomics only: a
 * repeated call returns the same bits. */
#define RSPARSE_HIP_KNN_COUNT 0
#define RSPARSE_HIP_KNN_COSINE 1
#define RSPARSE_HIP_KNN_JACCARD 2
#define RSPARSE_HIP_KNN_MAX_USERS (1 << 26)
#define RSPARSE_HIP_KNN_MAX_NEIGHBORS 256
#define RSPARSE_HIP_KNN_MAX_TOPK 1024
#define RSPARSE_HIP_KNN_WS_BYTES (1ull << 30)
#define RSPARSE_HIP_KNN_SPAN 64
#define RSPARSE_HIP_KNN_LDS_CAND 4096

/* The neighbours of the items [item0, item1): d_ip / d_iu the item-major orientation (item -> its users, n_items + 1 slots),
 * d_up / d_uj the CSR rows of the users (n_users + 1 slots), both 0-based from 0 and of the same pattern.  d_neighbors, d_counts:
 * (item1 - item0) x K row-major.  Reads d_ip[item0 .. item1] back (waits for `stream` once), then enqueues without
 * synchronisation.  An index outside its range is skipped on the device.
 * NULL pointer, negative dimension, not 0 <= item0 <= item1 <= n_items, unknown similarity, K < 1, ws_rows < 0 -> ERR_INVALID;
 * K > RSPARSE_HIP_KNN_MAX_NEIGHBORS, n_users > RSPARSE_HIP_KNN_MAX_USERS -> ERR_UNSUPPORTED; all before a device is touched. */
int rsparse_hip_cooc_neighbors_device(const int32_t* d_ip, const int32_t* d_iu, const int32_t* d_up, const int32_t* d_uj, int n_users,
                                      int n_items, int item0, int item1, int similarity, int K, int64_t ws_rows,
                                      int32_t* d_neighbors, int32_t* d_counts, void* stream);

/* The lists of the n_rows rows of the pattern (d_xp, d_xj) under the tables d_neighbors / d_q (n_items x K row-major; -1 slots
 * are skipped).  d_nr_p / d_nr_j: not_recommend as CSR slots over the same rows (nullable: nothing is filtered); d_excl0:
 * n_exclude 0-based items.  d_items: n_rows x k row-major, 1-based with INT32_MIN where a list ends, like
 * rsparse_hip_top_product; d_scores: the int64 sums, 0 in the padding.  Reads d_xp back (waits for `stream` once).
 * NULL pointer, negative dimension, K < 1, k < 1, ws_rows < 0, nr_p without nr_j -> ERR_INVALID; K >
 * RSPARSE_HIP_KNN_MAX_NEIGHBORS, k > RSPARSE_HIP_KNN_MAX_TOPK -> ERR_UNSUPPORTED; all before a device is touched. */
int rsparse_hip_knn_recommend_device(const int32_t* d_xp, const int32_t* d_xj, int n_rows, int n_items, const int32_t* d_neighbors,
                                     const uint32_t* d_q, int K, const int32_t* d_nr_p, const int32_t* d_nr_j,
                                     const int32_t* d_excl0, int n_exclude, int k, int64_t ws_rows, int32_t* d_items,
                                     int64_t* d_scores, void* stream);

/* host-array forms.  p / j: the dgRMatrix slots of the users x items pattern (0-based, ascending and unique within a row).
 * neighbors / counts: n_items x K COLUMN-major, neighbors 1-based with NA_integer_ (INT32_MIN) where an item has fewer than K.
 * Besides the refusals of the device form: p[0] != 0, a decreasing p, a column outside [0, n_items) or a row that is not
 * strictly ascending -> ERR_INVALID, before a device is touched. */
int rsparse_hip_cooc_neighbors(const int32_t* p, const int32_t* j, int n_users, int n_items, int similarity, int K,
                               int32_t* neighbors, int32_t* counts);
/* x_p / x_j and nr_p / nr_j (nullable) as above over the n_rows users; neighbors (1-based, NA or anything outside 1 .. n_items =
 * an empty slot) and q: n_items x K column-major; exclude: 1-based items; res: n_rows x k column-major, 1-based with
 * NA_integer_; scores: the int64 sums, column-major.  The same refusals, and q > 2^30 -> ERR_INVALID. */
int rsparse_hip_knn_recommend(const int32_t* x_p, const int32_t* x_j, int n_rows, int n_items, const int32_t* neighbors,
                              const uint32_t* q, int K, const int32_t* nr_p, const int32_t* nr_j, const int32_t* exclude,
                              int n_exclude, int k, int32_t* res, int64_t* scores);

/* ItemKNN on weighted values (rsparse_amd/itemknn.py states it in numpy; its recipes turn BM25 / TF-IDF cosine, the dot product,
 * the asymmetric cosine and P3alpha / RP3beta into the operands below).  On the canonical CSR pattern of the users x items
 * matrix an entry (u, i) carries two uint32: l_ui, used when i is the item whose neighbours are sought, and r_ui, used when i is
 * the neighbour, with max(l) max(r) max_j n_j < 2^53 (n_j = the users of item j), so that
 *     c_ij = sum_u l_ui r_uj      (j != i; uint64, below 2^53: double(c_ij) is exact)
 * The order key is  key_ij = double(c_ij) / (a_i b_j + h)  with tables a, b of n_items doubles and one double h, made by the
 * host: exactly three roundings in double -- the product, the sum, the division -- and no fused multiply-add.  a, b finite and in
 * [2^-200, 2^200], h finite and in [0, 2^400]: every key of a non-empty cell is then a positive normal double and 0 stays the
 * mark of an empty cell.  The neighbours of i are the K items j != i with c_ij > 0 of largest key, ties to the smaller j:
 * `neighbors` as above, `sums` uint64 = c_ij with 0 in the padding.  The device returns integers only; the similarity of a slot
 * is its key, recomputed by the caller from `sums` and the tables.
 *
 * A weighted row is scored as  score_u[j] = sum of xv_ui q[i, s]  over the items i of the row and the slots s with
 * neighbors[i, s] == j, xv <= 2^16 - 1 and a row's sum of xv below 2^31, so that a score stays below 2^61.
 *
 * A dense row of the weighted neighbours is n_items cells of 8 bytes (half as many rows per batch as the binary entry holds);
 * ws_rows keeps its meaning.  64-bit integer atomics on global memory only. */

/* d_il: l by stored position of the item-major orientation (d_ip / d_iu), d_ur: r by stored position of the CSR rows (d_up /
 * d_uj); d_a, d_b: n_items doubles on the device.  d_neighbors (int32), d_sums (uint64): (item1 - item0) x K row-major.  Reads
 * d_ip[item0 .. item1] back (waits for `stream` once).  The ranges of a, b and the 2^53 bound are preconditions here (the host
 * form checks them); whatever the values hold, nothing outside the operands and the workspace is read or written.
 * NULL pointer, negative dimension, not 0 <= item0 <= item1 <= n_items, K < 1, ws_rows < 0, h not finite or outside [0, 2^400]
 * -> ERR_INVALID; K > RSPARSE_HIP_KNN_MAX_NEIGHBORS -> ERR_UNSUPPORTED; all before a device is touched.  (The n_users limit of
 * the binary entry does not apply: the 2^53 bound replaces it.) */
int rsparse_hip_cooc_neighbors_weighted_device(const int32_t* d_ip, const int32_t* d_iu, const uint32_t* d_il, const int32_t* d_up,
                                               const int32_t* d_uj, const uint32_t* d_ur, int n_users, int n_items, int item0,
                                               int item1, const double* d_a, const double* d_b, double h, int K, int64_t ws_rows,
                                               int32_t* d_neighbors, uint64_t* d_sums, void* stream);

/* rsparse_hip_knn_recommend_device with the rows' weights d_xv (one uint32 per stored position of d_xj; NULL = all ones, which
 * is rsparse_hip_knn_recommend_device itself).  The same refusals. */
int rsparse_hip_knn_recommend_weighted_device(const int32_t* d_xp, const int32_t* d_xj, const uint32_t* d_xv, int n_rows, int n_items,
                                              const int32_t* d_neighbors, const uint32_t* d_q, int K, const int32_t* d_nr_p,
                                              const int32_t* d_nr_j, const int32_t* d_excl0, int n_exclude, int k, int64_t ws_rows,
                                              int32_t* d_items, int64_t* d_scores, void* stream);

/* host-array forms, with the conventions of the pair above.  l, r: one uint32 per stored position of (p, j); a, b: n_items
 * doubles; neighbors / sums: n_items x K COLUMN-major, neighbors 1-based with NA_integer_.  Besides the refusals of the device
 * form and of rsparse_hip_cooc_neighbors' arrays: l or r NULL with stored entries, a or b not finite or outside [2^-200, 2^200],
 * max(l) max(r) max_j n_j >= 2^53 -> ERR_INVALID, before a device is touched. */
int rsparse_hip_cooc_neighbors_weighted(const int32_t* p, const int32_t* j, const uint32_t* l, const uint32_t* r, int n_users,
                                        int n_items, const double* a, const double* b, double h, int K, int32_t* neighbors,
                                        uint64_t* sums);
/* rsparse_hip_knn_recommend with x_v (nullable = all ones): besides its refusals, x_v above 2^16 - 1 and a row whose x_v sum to
 * 2^31 or more -> ERR_INVALID. */
int rsparse_hip_knn_recommend_weighted(const int32_t* x_p, const int32_t* x_j, const uint32_t* x_v, int n_rows, int n_items,
                                       const int32_t* neighbors, const uint32_t* q, int K, const int32_t* nr_p, const int32_t* nr_j,
                                       const int32_t* exclude, int n_exclude, int k, int32_t* res, int64_t* scores);

/* ItemKNN under the evaluation protocols of the factor models: the score at given cells, the lists within per-row candidates,
 * and where held-out items stand among all items.  Each entry scores the n_rows rows of the pattern (d_xp, d_xj) with the
 * weights d_xv (nullable: all ones) under d_neighbors / d_q exactly as rsparse_hip_knn_recommend_weighted_device does -- the same
 * scatter into the same dense rows, ws_rows with the same meaning -- and differs in what reads a row.  Its own pattern (d_*_p:
 * n_rows + 1 slots, d_*_j: 0-based columns) lies over the same rows; all row pointers are ABSOLUTE slots into their column
 * array, so that a caller can pass a slice of the pointers with the whole column array, and an output with one element per
 * stored position parallels the column array (element t belongs to column slot t).  Integers only on the device, integer
 * atomics only: a repeated call returns the same bits; the workspace is all zeros again when the enqueued work is done.
 * Each reads d_xp back (waits for `stream` once), then enqueues without synchronisation.
 * Refusals, all before a device is touched: NULL where a pointer is required, a negative dimension, K < 1, k < 1, ws_rows < 0,
 * nr_p without nr_j, n_exclude < 0 (or > 0 without d_excl0) -> ERR_INVALID; K > RSPARSE_HIP_KNN_MAX_NEIGHBORS,
 * k > RSPARSE_HIP_KNN_MAX_TOPK -> ERR_UNSUPPORTED; n_rows == 0 -> OK.  Row pointers read back that are negative or decrease ->
 * ERR_INVALID.
 *
 * rsparse_hip_knn_score_pairs_device: d_scores[t] = score_row(t)[d_pairs_j[t]] (int64) for every stored position t of the pairs
 * pattern; nothing is masked; a column outside [0, n_items) gives 0; j need not be sorted and may repeat.  Also reads d_pairs_p
 * back. */
int rsparse_hip_knn_score_pairs_device(const int32_t* d_xp, const int32_t* d_xj, const uint32_t* d_xv, int n_rows, int n_items,
                                       const int32_t* d_neighbors, const uint32_t* d_q, int K, const int32_t* d_pairs_p,
                                       const int32_t* d_pairs_j, int64_t ws_rows, int64_t* d_scores, void* stream);

/* The k best of every row's candidates: the admissible ones are the candidate columns inside [0, n_items) that are neither in
 * the row's not_recommend entries nor in d_excl0; order as rsparse_hip_knn_recommend_device -- score descending, equal scores to
 * the SMALLER item (not the heap's rule of rsparse_hip_top_candidates_device) --, candidates of score 0 are ranked, a list is
 * shorter than k only when fewer than k candidates are admissible.  d_items / d_scores as there: n_rows x k row-major, 1-based
 * with INT32_MIN, int64 sums with 0 in the padding.  Candidate columns are unique within a row (a repeated one may be listed
 * twice).  A row of up to RSPARSE_HIP_KNN_LDS_CAND candidates costs, behind the scatter, work in proportion to its candidates;
 * a longer one -- up to the whole catalogue -- is restricted to its candidates in the dense row and selected as
 * rsparse_hip_knn_recommend_device selects.  1 <= k <= RSPARSE_HIP_KNN_MAX_TOPK.  Also reads d_cand_p back. */
int rsparse_hip_knn_top_candidates_device(const int32_t* d_xp, const int32_t* d_xj, const uint32_t* d_xv, int n_rows, int n_items,
                                          const int32_t* d_neighbors, const uint32_t* d_q, int K, const int32_t* d_cand_p,
                                          const int32_t* d_cand_j, const int32_t* d_nr_p, const int32_t* d_nr_j, const int32_t* d_excl0,
                                          int n_exclude, int k, int64_t ws_rows, int32_t* d_items, int64_t* d_scores, void* stream);

/* above / tied / n_adm as rsparse_hip_held_out_ranks_device defines them, with s the integer score: A_u = the items outside the
 * row's not_recommend entries and outside d_excl0, d_n_adm[u] = |A_u|; for a stored entry (u, h) of actual, above = #{j in A_u :
 * s_j > s_h}, tied = #{j in A_u, j != h : s_j == s_h}; an entry outside A_u (or outside [0, n_items)) gets -1 / -1 and takes no
 * part.  d_above / d_tied: int32, one per stored entry; d_n_adm: int32, one per row.  A row's entries are counted
 * RSPARSE_HIP_RANKS_BATCH at a time, one pass over the row's n_items cells each; the entries need not be sorted and may repeat.
 * rsparse_hip_rank_summary_device turns the counts into mpr / auc / mrr.  A valid d_actual_p is a precondition. */
int rsparse_hip_knn_held_out_ranks_device(const int32_t* d_xp, const int32_t* d_xj, const uint32_t* d_xv, int n_rows, int n_items,
                                          const int32_t* d_neighbors, const uint32_t* d_q, int K, const int32_t* d_actual_p,
                                          const int32_t* d_actual_j, const int32_t* d_nr_p, const int32_t* d_nr_j, const int32_t* d_excl0,
                                          int n_exclude, int64_t ws_rows, int32_t* d_above, int32_t* d_tied, int32_t* d_n_adm,
                                          void* stream);

/* host-array forms, with the conventions of rsparse_hip_knn_recommend_weighted (x_p / x_j / x_v, neighbors and q column-major
 * with 1-based neighbours, nr_p / nr_j nullable, exclude 1-based) and all of its refusals.  cand_p / cand_j: dgRMatrix slots over
 * the rows of x, 0-based; cand_p[0] != 0, a decreasing cand_p, a candidate column outside [0, n_items) or a row that is not
 * strictly ascending -> ERR_INVALID, before a device is touched.  res / scores: n_rows x k column-major. */
int rsparse_hip_knn_top_candidates(const int32_t* x_p, const int32_t* x_j, const uint32_t* x_v, int n_rows, int n_items,
                                   const int32_t* neighbors, const uint32_t* q, int K, const int32_t* cand_p, const int32_t* cand_j,
                                   const int32_t* nr_p, const int32_t* nr_j, const int32_t* exclude, int n_exclude, int k, int32_t* res,
                                   int64_t* scores);
/* actual_p / actual_j: dgRMatrix slots over the rows of x; actual_p[0] != 0, a decreasing actual_p, columns not strictly
 * ascending within a row -> ERR_INVALID (a column outside the items is an inadmissible entry, not a refusal).  above / tied: one
 * int32 per stored entry; n_adm: n_rows int32. */
int rsparse_hip_knn_held_out_ranks(const int32_t* x_p, const int32_t* x_j, const uint32_t* x_v, int n_rows, int n_items,
                                   const int32_t* neighbors, const uint32_t* q, int K, const int32_t* actual_p, const int32_t* actual_j,
                                   const int32_t* nr_p, const int32_t* nr_j, const int32_t* exclude, int n_exclude, int32_t* above,
                                   int32_t* tied, int32_t* n_adm);

/* ------------------------------------------------------------------------------------------------
 * EASE (Steck 2019): the item Gram matrix on the device, and top-k lists scored by a dense items x items weight matrix
 * ---------------------------------------------------------------------------------------------- */

/* The definition (rsparse_amd/ease.py states it in numpy).  On the canonical binary pattern of a users x items matrix, G = X^T X:
 * c_ij off the diagonal (the co-occurrence count, an exact integer), n_j on it.  With P = (G + lambda I)^-1 the weights are
 * B_ij = -P_ij / P_jj, B_jj = 0; the factorisation is the caller's (dense linear algebra is not part of this library).  A user
 * (a row of a pattern x) is scored by
 *     score_u = sum over the stored items i of the row, in ascending stored order, of double(B[i, :])
 * a sequential sum in double, one rounding per step (a float B converts exactly).  The list of u is the k items of largest score
 * among those neither in the row's not_recommend entries nor in items_exclude, ties to the smaller item.  The order is that of
 * the 64-bit KEY of the double -- its bits flipped if it is negative, otherwise its sign bit set --, and the key is what
 * d_scores returns: key >> 63 ? key ^ (1 << 63) : ~key are the double's bits again.  An accumulator that starts at +0.0 never
 * becomes -0.0, and no finite score has the key 0 or all ones (B must be finite).
 *
 * Both entries work in the dense rows of the ItemKNN workspace, a batch at a time, with its kernels (wrmf_ease.hip,
 * wrmf_itemknn.hip): rows per batch = ws_rows, or with ws_rows = 0 what RSPARSE_HIP_KNN_WS_BYTES holds (a row is n_items cells of
 * 4 bytes for the Gram rows, of 8 for the lists).  The scoring kernel gives a workgroup one row and one tile of
 * RSPARSE_HIP_EASE_TILE_BYTES of columns, stages the row's indices RSPARSE_HIP_EASE_CHUNK at a time and keeps
 * RSPARSE_HIP_EASE_AHEAD rows of B in flight per thread.  No atomics on floats: a repeated call returns the same bits.
 * RSPARSE_HIP_EASE_MAX_ITEMS bounds the catalogue: an items x items matrix of doubles is 8 GiB there, and a fit holds three of
 * them at its peak (G + lambda I, its Cholesky factor, the inverse) beside B. */
#define RSPARSE_HIP_EASE_MAX_ITEMS 32768
#define RSPARSE_HIP_EASE_TILE_BYTES 4096
#define RSPARSE_HIP_EASE_CHUNK 1024
#define RSPARSE_HIP_EASE_AHEAD 8

/* Rows [item0, item1) of G + lambda I: d_out[(i - item0) ld_out + j] = c_ij for j != i, double(n_i) + lambda (one rounding) for
 * j == i.  d_ip / d_iu, d_up / d_uj: the two orientations of the pattern, as rsparse_hip_cooc_neighbors_device takes them.
 * Reads d_ip[item0 .. item1] back (waits for `stream` once), then enqueues without synchronisation.
 * NULL pointer, negative dimension, not 0 <= item0 <= item1 <= n_items, ws_rows < 0, ld_out < n_items, lambda < 0 or not finite
 * -> ERR_INVALID; n_items > RSPARSE_HIP_EASE_MAX_ITEMS -> ERR_UNSUPPORTED; all before a device is touched. */
int rsparse_hip_item_gram_device(const int32_t* d_ip, const int32_t* d_iu, const int32_t* d_up, const int32_t* d_uj, int n_users,
                                 int n_items, int item0, int item1, double lambda, double* d_out, size_t ld_out, int64_t ws_rows,
                                 void* stream);

/* The lists of the n_rows rows of the pattern (d_xp, d_xj) under d_B: n_items rows of ld_B elements (float, or double with
 * b_is_double), 16-byte aligned, ld_B >= n_items and a multiple of 16 bytes (a multiple of 256 bytes keeps every row aligned to
 * a cache line pair; what lies beyond n_items in a row is read and never used).  d_nr_p / d_nr_j / d_excl0 / d_items: as
 * rsparse_hip_knn_recommend_device; d_scores: the keys, 0 in the padding.  A column of d_xj outside [0, n_items) is skipped.
 * Reads d_xp back (waits for `stream` once).  NULL pointer, negative dimension, k < 1, ws_rows < 0, nr_p without nr_j, a bad exclude, a bad ld_B or
 * alignment -> ERR_INVALID; k > RSPARSE_HIP_KNN_MAX_TOPK, n_items > RSPARSE_HIP_EASE_MAX_ITEMS -> ERR_UNSUPPORTED; all before a
 * device is touched. */
int rsparse_hip_ease_recommend_device(const int32_t* d_xp, const int32_t* d_xj, int n_rows, int n_items, const void* d_B, size_t ld_B,
                                      int b_is_double, const int32_t* d_nr_p, const int32_t* d_nr_j, const int32_t* d_excl0,
                                      int n_exclude, int k, int64_t ws_rows, int32_t* d_items, uint64_t* d_scores, void* stream);

/* host-array forms.  p / j: the dgRMatrix slots of the users x items pattern, with the checks of rsparse_hip_cooc_neighbors;
 * out: n_items x n_items doubles (the matrix is symmetric: either layout). */
int rsparse_hip_item_gram(const int32_t* p, const int32_t* j, int n_users, int n_items, double lambda, double* out);
/* x_p / x_j, nr_p / nr_j (nullable), exclude (1-based), res (n_rows x k column-major, 1-based with NA_integer_): as
 * rsparse_hip_knn_recommend, with its refusals.  B: n_items x n_items COLUMN-major (an R matrix), float or double; a non-finite
 * entry -> ERR_INVALID.  scores: the doubles themselves, column-major, NaN where res is NA. */
int rsparse_hip_ease_recommend(const int32_t* x_p, const int32_t* x_j, int n_rows, int n_items, const void* B, int b_is_double,
                               const int32_t* nr_p, const int32_t* nr_j, const int32_t* exclude, int n_exclude, int k, int32_t* res,
                               double* scores);

/* EASE under the evaluation protocols of the other models: the score at given cells, the lists within per-row candidates, and
 * where held-out items stand among all items.  The arguments, conventions and refusals are those of the rsparse_hip_knn_*
 * entries of the same names (absolute row pointers, outputs parallel to the column arrays, d_xp and the entry's own row pointers
 * read back, n_rows == 0 -> OK) with d_B, ld_B, b_is_double in place of d_neighbors, d_q, K and d_xv, and with the checks of B of
 * rsparse_hip_ease_recommend_device (alignment and ld_B -> ERR_INVALID, n_items > RSPARSE_HIP_EASE_MAX_ITEMS -> ERR_UNSUPPORTED).
 * Scores are the 64-bit keys of the doubles, as there.
 *
 * A dense score row costs nnz(row) x n_items cells of B; a row that is asked for m cells needs nnz(row) x m of them.  The host
 * routes every row by its own m, from the row pointers it has read back:
 *     m <= RSPARSE_HIP_KNN_LDS_CAND  and  m * RSPARSE_HIP_EASE_CELLS_RATIO <= n_items      -> the CELL route
 *     otherwise                                                                            -> the DENSE route
 * Cell route: one kernel scores B at the row's cells only -- a lane owns a cell, a wave 64 consecutive cells of one row, so the
 * history index is wave-uniform and the lane's column its only vector address; RSPARSE_HIP_EASE_AHEAD loads in flight; the adds
 * in ascending stored order, the sequence the dense kernel takes for that column -- and, for the lists, a second one masks,
 * orders and cuts the row's (key, item) pairs in LDS.  Dense route: the scoring kernel of rsparse_hip_ease_recommend_device into
 * the workspace (ws_rows rows per batch, consecutive dense-route rows only), then ItemKNN's gather, or its mask, a restriction of
 * the row to its candidates and its select.  Both routes return the same bits; a scattered four-byte cell costs a whole cache
 * line, which is what the ratio prices (profiles/ease_eval holds the sweep).  No atomics on floats: repeat calls are identical. */
#ifndef RSPARSE_HIP_EASE_CELLS_RATIO   /* (a build may set another one: the sweep is made that way) */
#define RSPARSE_HIP_EASE_CELLS_RATIO 16
#endif

/* d_scores[t] = key(score_row(t)[d_pairs_j[t]]) for every stored position t of the pairs pattern; nothing is masked; a column
 * outside [0, n_items) gives the key of +0.0 (1 << 63); j need not be sorted and may repeat. */
int rsparse_hip_ease_score_pairs_device(const int32_t* d_xp, const int32_t* d_xj, int n_rows, int n_items, const void* d_B, size_t ld_B,
                                        int b_is_double, const int32_t* d_pairs_p, const int32_t* d_pairs_j, int64_t ws_rows,
                                        uint64_t* d_scores, void* stream);

/* The k best of every row's candidates, as rsparse_hip_knn_top_candidates_device defines them (score descending by key, equal
 * scores to the smaller item, candidates of score 0 ranked, a column outside [0, n_items) never listed); d_items / d_scores as
 * rsparse_hip_ease_recommend_device.  PRECONDITION: the candidate columns of a row are strictly ascending (the cell route finds
 * a row's not_recommend and excluded items among them by a lower bound; the host form refuses a violation). */
int rsparse_hip_ease_top_candidates_device(const int32_t* d_xp, const int32_t* d_xj, int n_rows, int n_items, const void* d_B, size_t ld_B,
                                           int b_is_double, const int32_t* d_cand_p, const int32_t* d_cand_j, const int32_t* d_nr_p,
                                           const int32_t* d_nr_j, const int32_t* d_excl0, int n_exclude, int k, int64_t ws_rows,
                                           int32_t* d_items, uint64_t* d_scores, void* stream);

/* above / tied / n_adm as rsparse_hip_knn_held_out_ranks_device defines them, with s the double score (compared by key): the
 * dense scoring kernel, ItemKNN's mask and its rank count on the key rows.  Every row takes the dense route. */
int rsparse_hip_ease_held_out_ranks_device(const int32_t* d_xp, const int32_t* d_xj, int n_rows, int n_items, const void* d_B, size_t ld_B,
                                           int b_is_double, const int32_t* d_actual_p, const int32_t* d_actual_j, const int32_t* d_nr_p,
                                           const int32_t* d_nr_j, const int32_t* d_excl0, int n_exclude, int64_t ws_rows, int32_t* d_above,
                                           int32_t* d_tied, int32_t* d_n_adm, void* stream);

/* host-array forms: x_p / x_j, B (column-major, a non-finite entry -> ERR_INVALID), nr_p / nr_j, exclude (1-based) as
 * rsparse_hip_ease_recommend; cand_p / cand_j and actual_p / actual_j with the checks of rsparse_hip_knn_top_candidates and
 * rsparse_hip_knn_held_out_ranks.  res / scores: n_rows x k column-major, the scores the doubles themselves, NaN where res is NA. */
int rsparse_hip_ease_top_candidates(const int32_t* x_p, const int32_t* x_j, int n_rows, int n_items, const void* B, int b_is_double,
                                    const int32_t* cand_p, const int32_t* cand_j, const int32_t* nr_p, const int32_t* nr_j,
                                    const int32_t* exclude, int n_exclude, int k, int32_t* res, double* scores);
int rsparse_hip_ease_held_out_ranks(const int32_t* x_p, const int32_t* x_j, int n_rows, int n_items, const void* B, int b_is_double,
                                    const int32_t* actual_p, const int32_t* actual_j, const int32_t* nr_p, const int32_t* nr_j,
                                    const int32_t* exclude, int n_exclude, int32_t* above, int32_t* tied, int32_t* n_adm);

/* ------------------------------------------------------------------------------------------------
 * SLIM (Ning and Karypis 2011): the non-negative elastic-net item-item weights, by coordinate descent on the Gram rows
 * ---------------------------------------------------------------------------------------------- */

/* The definition (rsparse_amd/slim.py states it in numpy).  G is the Gram matrix of the canonical binary pattern at lambda = 0,
 * as rsparse_hip_item_gram_device writes it: c_ij off the diagonal, n_i on it, exact integers in doubles.  Column j minimises,
 * over w >= 0 with w_j = 0,
 *     1/2 |h_j - H w|^2 + l2/2 |w|^2 + l1 |w|_1
 * (sklearn's ElasticNet: l1 = n_users alpha l1_ratio, l2 = n_users alpha (1 - l1_ratio)).  The support S_j is the set of i != j
 * with c_ij > 0, ascending; no other coordinate is visited (with G >= 0 and w >= 0 its update is max(0, <= 0 - l1) = 0: the
 * restriction is the problem itself).  State: w and r, doubles over S_j, from +0.0; r_s is (G w)_{S[s]}, kept by the updates.
 * One sweep visits t = 0 .. m - 1 in order, every operation a separately rounded double operation, nothing fused:
 *     i = S[t];  d = G[i, i];  c = G[j, i]
 *     u  = (c - (r[t] - d * w[t])) - l1
 *     wn = u / (d + l2)  if u > 0  else +0.0
 *     delta = wn - w[t]
 *     if delta != 0:  r[s] = r[s] + (delta * G[i, S[s]]) for every s;  w[t] = wn
 *     dmax = max(dmax, |delta|);  wmax = max(wmax, |wn|)
 * After a sweep: stop if wmax == 0 or dmax <= tol * wmax, otherwise go on, up to max_iter sweeps; an empty support takes 0 sweeps.
 * The column's weights are W[S[t], j] = w[t], rounded once into W's type; its other cells are +0.0.  W is scored as the B of EASE.
 *
 * The kernel (wrmf_slim.hip) gives a workgroup one column and keeps 36 bytes per support entry: in LDS for a support of up to
 * RSPARSE_HIP_SLIM_LDS_SUPPORT entries (72 KiB, two workgroups per CU), in a slice of a grow-only workspace beyond.  The sequence
 * above is kept exactly; its chain is shortened by evaluating 64 consecutive coordinates at once and applying the first that
 * changes.  No atomics: a repeated call returns the same bits. */
#define RSPARSE_HIP_SLIM_LDS_SUPPORT 2048

/* Columns d_cols[0 .. n_cols) (any order, repeats allowed; pass long supports first) of the n_items x n_items row-major d_G
 * (ld_G doubles per row) into the row-major d_W: d_W[i ld_W + j] for every i of S_j, zeros included, as float, or as double with
 * w_is_double; NO other cell is written, so the caller hands in a zeroed W.  d_W, ld_W: the rules of d_B of
 * rsparse_hip_ease_recommend_device.  d_sweeps[c]: the sweeps column d_cols[c] took.  Reads the support sizes back (waits for
 * `stream` once); a column outside [0, n_items) is found there -> ERR_INVALID, with nothing written.
 * NULL pointer, negative size, l1 / l2 / tol negative or not finite, max_iter < 1, ld_G < n_items, a bad ld_W or alignment
 * -> ERR_INVALID; n_items > RSPARSE_HIP_EASE_MAX_ITEMS -> ERR_UNSUPPORTED; all before a device is touched.  n_cols == 0 -> OK. */
int rsparse_hip_slim_columns_device(const double* d_G, size_t ld_G, int n_items, const int32_t* d_cols, int n_cols, double l1,
                                    double l2, int max_iter, double tol, void* d_W, size_t ld_W, int w_is_double, int32_t* d_sweeps,
                                    void* stream);

/* host-array form: the Gram matrix of the pattern (p / j: the dgRMatrix slots of the users x items matrix, with the checks of
 * rsparse_hip_cooc_neighbors), every column's fit, and the download.  W: n_items x n_items doubles, COLUMN-major (an R matrix:
 * W[j n_items + i] is the weight of item i in the column of item j); sweeps: n_items, by item. */
int rsparse_hip_slim_fit(const int32_t* p, const int32_t* j, int n_users, int n_items, double l1, double l2, int max_iter, double tol,
                         double* W, int32_t* sweeps);

/* ------------------------------------------------------------------------------------------------
 * BPR (Rendle et al. 2009): matrix factorisation on the pairwise ranking loss, by deterministic mini-batch SGD
 * ---------------------------------------------------------------------------------------------- */

/* The definition (rsparse_amd/bpr.py states it in numpy: bpr_triples, bpr_step_reference, bpr_fit_reference).  The input is a
 * canonical CSR pattern (p from 0, columns ascending and unique per row; nnz = p[n_rows] is handed in, nothing is read back).
 *
 * Triples: stream 6 of the Philox4x32-10 of the generators above.  An epoch has one triple per stored entry.  Slot s of the CSR
 * belongs to row u of L entries at position q = s - p[u]; counter (q, g, 6, epoch + 2^31 mode), key (lo32(seed), hi32(seed)) ->
 * o0..o3; mode 0 (the fit): g = row0 + u; mode 1 (the fold-in): g = row0 for EVERY row, so that a folded-in row depends on the
 * row alone (all rows of a fold-in epoch then share the words of a position q and with them its three negative candidates:
 * harmless with the items frozen, where no row sees another's update).  Positive i = j[p[u] + ((o0 L) >> 32)]; negative = the first of (o1 n_items) >> 32, (o2 n_items) >> 32,
 * (o3 n_items) >> 32 that is not in the row; all three in the row: the triple is VOID (-1) and takes no part in anything.
 *
 * Steps: step t of n_steps holds the slots s = t, t + n_steps, ... in ascending order, numbered k = 0, 1, ...
 *
 * One step, from the snapshot (U, V) at its start; every operation a separately rounded double operation, the factors widened:
 *     dot(a, b)  16 partial sums, partial l = the products of the coordinates l, l + 16, ... added in ascending order from +0.0;
 *                then v[0:8] + v[8:16], v[0:4] + v[4:8], v[0:2] + v[2:4], v[0] + v[1]
 *     d_k = dot(U[u], V[i] - V[j])
 *     E(d): d clamped to [-40, 40]; kk = rint(d * 1.4426950408889634);
 *           r = (d - kk * 6.93147180369123816490e-01) - kk * 1.90821492927058770002e-10;
 *           the polynomial sum_{n <= 13} r^n / n! in Horner form with the coefficients 1.0 / n!, then ldexp(., kk)
 *     z_k = 1 / (1 + E(d_k))
 *     user u receives z_k (V[i] - V[j]), item i receives z_k U[u], item j receives (-z_k) U[u]
 *     a destination sums its contributions in ascending k, the positive role before the negative one within a k; the list is cut
 *     into chunks of RSPARSE_HIP_BPR_CHUNK consecutive contributions, a chunk is summed sequentially from +0.0, the chunk sums
 *     are added sequentially to a total that starts at +0.0
 *     a destination with c >= 1 contributions: g = total - (lambda c) row;  a' = a + dot(g, g) / rank;
 *     row' = row + (learning_rate g) / sqrt(a') unless a' == 0, rounded once into the factors' type; the others keep their bits
 * a: one double per user and per item (Adagrad's state), part of the model.  counts: (n_valid, n_correct) per epoch -- the triples
 * that are not void, and those of them with d_k > 0.  update_items = 0 reads V only: d_aV is neither read nor written then (it
 * must still be a valid pointer).
 *
 * The kernels (wrmf_bpr.hip): a thread per triple samples; a 16-lane group per triple scores; a group per run of equal users
 * sums into a staging row; the item side is grouped by a stable radix sort of (item, 2k + role) and summed by a group per chunk
 * and a group per item.  No float atomics: a repeated call returns the same bits. */
#define RSPARSE_HIP_BPR_CHUNK 64

/* Common refusals, all before a device is touched: a NULL pointer, n_rows / n_items / nnz negative, nnz >= 2^31,
 * row0 + n_rows > 2^32, mode not 0 / 1, an epoch outside [0, 2^31), n_steps < 1 or batch < 1, step outside [0, n_steps), rank < 1,
 * learning_rate / lambda negative or not finite -> ERR_INVALID; rank > RSPARSE_HIP_MAX_RANK (_f64: RSPARSE_HIP_MAX_RANK_F64)
 * -> ERR_UNSUPPORTED, and so is a step of 2^30 or more triples with update_items (the item side numbers a step's 2 cnt
 * contributions in 32 bits): take a smaller batch.  n_rows == 0 -> OK with no device.  U: n_rows x rank, V: n_items x rank, row-major without padding. */

/* the triples of one step: d_u (the LOCAL row), d_i, d_neg (-1: void), ceil((nnz - step) / n_steps) entries each.  Integers only. */
int rsparse_hip_bpr_triples_device(const int32_t* d_p, const int32_t* d_j, int n_rows, int n_items, int64_t nnz, int64_t row0,
                                   uint64_t seed, int mode, int epoch, int step, int n_steps, int32_t* d_u, int32_t* d_i,
                                   int32_t* d_neg, void* stream);

/* one step, in place; d_counts[0] += n_valid, d_counts[1] += n_correct.  Waits for `stream` before it returns (its scratch: with
 * cnt the slots of the step, min(n_rows, cnt) staging rows of the factors' type, 28 bytes per slot, and with update_items 16 more
 * per slot plus the sort's and at most 4 cnt / 64 + 1 chunk sums of rank doubles). */
int rsparse_hip_bpr_step_device(const int32_t* d_p, const int32_t* d_j, int n_rows, int n_items, int64_t nnz, int64_t row0,
                                uint64_t seed, int mode, int epoch, int step, int n_steps, int rank, double learning_rate,
                                double lambda, int update_items, float* d_U, float* d_V, double* d_aU, double* d_aV,
                                int64_t* d_counts, void* stream);
int rsparse_hip_bpr_step_f64_device(const int32_t* d_p, const int32_t* d_j, int n_rows, int n_items, int64_t nnz, int64_t row0,
                                    uint64_t seed, int mode, int epoch, int step, int n_steps, int rank, double learning_rate,
                                    double lambda, int update_items, double* d_U, double* d_V, double* d_aU, double* d_aV,
                                    int64_t* d_counts, void* stream);

/* the epochs [epoch0, epoch0 + n_epochs), every step of each, on one stream without a host synchronisation between the steps;
 * n_steps = ceil(nnz / batch) in mode 0 and 1 in mode 1.  d_counts: 2 n_epochs slots, zeroed by the call: (n_valid, n_correct) of
 * every epoch. */
int rsparse_hip_bpr_epochs_device(const int32_t* d_p, const int32_t* d_j, int n_rows, int n_items, int64_t nnz, int64_t row0,
                                  uint64_t seed, int mode, int epoch0, int n_epochs, int batch, int rank, double learning_rate,
                                  double lambda, int update_items, float* d_U, float* d_V, double* d_aU, double* d_aV,
                                  int64_t* d_counts, void* stream);
int rsparse_hip_bpr_epochs_f64_device(const int32_t* d_p, const int32_t* d_j, int n_rows, int n_items, int64_t nnz, int64_t row0,
                                      uint64_t seed, int mode, int epoch0, int n_epochs, int batch, int rank, double learning_rate,
                                      double lambda, int update_items, double* d_U, double* d_V, double* d_aU, double* d_aV,
                                      int64_t* d_counts, void* stream);

/* host-array form: a fit in double from the initial factors of rsparse_hip_init_factors_f64_device (streams 0 and 1 of `seed`,
 * scale 0.01) with a = 0; p / j: the dgRMatrix slots of the users x items pattern, with the checks of rsparse_hip_cooc_neighbors.
 * U: n_users x rank and V: n_items x rank, ROW-major; aU, aV: their Adagrad states; counts: 2 n_epochs. */
int rsparse_hip_bpr_fit(const int32_t* p, const int32_t* j, int n_users, int n_items, uint64_t seed, int n_epochs, int batch, int rank,
                        double learning_rate, double lambda, double* U, double* V, double* aU, double* aV, int64_t* counts);

/* ------------------------------------------------------------------------------------------------
 * why this item: per-item contributions to a score (Hu, Koren and Volinsky, section 5; `explain` of the `implicit` library)
 * ---------------------------------------------------------------------------------------------- */

/* The folded-in embedding of a row is linear in the row's entries: with A_u = B + d I + sum_t a_t y_t y_t^T over the stored
 * positions t of row u (y_t = d_V[d_x_j[t]], d = diag + diag_per_nnz * len(row u)) and A_u z = y_i for a target item i,
 *   score(u, i) = sum_t b_t (z . y_t),
 * and term t is what the interaction with item d_x_j[t] contributes.  Implicit feedback: B = the Gramian with lambda in it, a = c -
 * 1, b = c, diag = diag_per_nnz = 0; explicit: B absent (NULL), a = 1, b = r, diag = lambda, or diag_per_nnz = lambda under
 * dynamic_lambda.
 *   d_V: n_items x r row-major; d_base: r x r symmetric or NULL; (d_x_p, d_x_j): the rows as CSR over n_users, d_wa / d_wb one per
 *   stored position; (d_t_p, d_t_j): the targets as CSR over the same users; d_out_p[q]: where the segment of target q starts in
 *   d_contrib (len(row of q's user) entries, in row order).
 *   d_contrib[d_out_p[q] + t] = b_t (z . y_t) in the factors' type; d_total[q] = the segment's sum, in double, in a fixed order;
 *   d_flags[u] = 1 when A_u is not positive definite to working precision (a Cholesky pivot d_j <= 2 r eps a_jj) -- every
 *   output of that user's targets is then NaN --, 0 for every other user that has a target.
 * A user with an empty row is not factored: totals 0, flag 0.  Of a user without targets nothing is written, its flag included.
 * The sums have a fixed order and there are no atomics: a repeated call returns the same bits.  Enqueued on `stream` without
 * synchronisation.  Valid p arrays and indices in [0, n_items) are preconditions, not checked (they live on the device), as for
 * rsparse_hip_score_pairs_device; nothing outside d_V is read for an index outside it, and what depends on it is NaN.
 * NULL among d_V, d_x_p, d_t_p, d_flags, or d_t_j given without d_x_j, d_wa, d_wb, d_out_p, d_contrib, d_total; n_items < 0,
 * n_users < 0, r < 1 -> ERR_INVALID, before a device is touched; r > 128 (both element types: the system lives in LDS) ->
 * ERR_UNSUPPORTED; n_users == 0, or d_t_j == NULL (no target at all) -> OK, nothing is launched. */
int rsparse_hip_explain_device(const float* d_V, int n_items, int r, const float* d_base, double diag, double diag_per_nnz,
                               int n_users, const int32_t* d_x_p, const int32_t* d_x_j, const float* d_wa, const float* d_wb,
                               const int32_t* d_t_p, const int32_t* d_t_j, const int64_t* d_out_p, float* d_contrib,
                               double* d_total, int32_t* d_flags, void* stream);
int rsparse_hip_explain_f64_device(const double* d_V, int n_items, int r, const double* d_base, double diag, double diag_per_nnz,
                                   int n_users, const int32_t* d_x_p, const int32_t* d_x_j, const double* d_wa, const double* d_wb,
                                   const int32_t* d_t_p, const int32_t* d_t_j, const int64_t* d_out_p, double* d_contrib,
                                   double* d_total, int32_t* d_flags, void* stream);

/* ------------------------------------------------------------------------------------------------
 * initial factors drawn on the device: a counter-based normal generator
 * ---------------------------------------------------------------------------------------------- */

/* The reference fills the two factor matrices on the host with R's generator before the first half-iteration
 * (large_rand_matrix, src/utils.cpp:130-151: rank x n column-major N(0, 1) / 100; R/model_WRMF.R:203-255: the draw, the rows of
 * ones of a model with user/item biases, abs() for NNLS, zeros for the items under conjugate gradient) and the half-iterations
 * take the factors as inputs only.  At 10M x 1M and rank 128 that is seconds of host work and a 5.6 GB upload; these two entries
 * write the same kind of matrix straight into device memory.  The stream is DEFINED here, so that any host (an R shim included)
 * can reproduce it; rsparse_amd/rng.py is the definition in numpy.
 *
 *   Bits.      Philox4x32-10, the standard Random123 rounds: per round  hi0:lo0 = 0xD2511F53 * c0,  hi1:lo1 = 0xCD9E8D57 * c2,
 *              (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); between rounds k0 += 0x9E3779B9, k1 += 0xBB67AE85.
 *   Index.     The matrix is n x rank row-major (= the reference's column-major rank x n).  Element (row, col) has the 64-bit
 *              linear index e = row * rank + col over the WHOLE matrix; the leading dimension ld is not used here.
 *   Counter.   (lo32(e >> 2), hi32(e >> 2), stream, 0); key (lo32(seed), hi32(seed)).  stream 0 = user factors, 1 = item factors.
 *   Outputs.   One Philox call gives four words o0..o3 and four numbers; element e takes number e & 3 (with rank % 4 != 0 a group
 *              of four straddles two rows).
 *   Uniforms.  From the top 24 bits, exact in fp32:  u_a = ((o0 >> 8) + 1) * 2^-24 in (0, 1],  u_b = (o1 >> 8) * 2^-24 in [0, 1).
 *   Normals.   r = sqrt(-2 ln u_a); numbers 0 and 1 are r cos(2 pi u_b) and r sin(2 pi u_b); numbers 2 and 3 the same from
 *              (o2, o3).  |z| <= sqrt(48 ln 2) = 5.77.
 *   Value.     scale * z (the reference: scale = 0.01), its absolute value if abs_values != 0; the column ones_col (-1 = none) is
 *              written as exactly 1.
 * A value therefore depends on (seed, stream, row, col, rank) only -- not on the launch, the row range asked for, the number of
 * devices that each draw their own rows, or the device.  The fp32 entry evaluates the transform in fp32 (within
 * 2^-21 * scale * max(1, r) of the double evaluation), the f64 entry in double.
 *
 * d_out points at the first element of row row0 (so a shard generates only its own rows): rows row0 .. row0 + n_rows - 1 are
 * written at d_out[(row - row0) * ld + col], col < rank; with ld > rank the padding is not touched.  One write-only launch on
 * hip_stream (a hipStream_t, NULL = default), no synchronisation.  There is no rank ceiling: nothing here depends on a solver.
 * n_rows < 0, row0 < 0, rank < 1, ld < rank, stream outside 0..1, ones_col outside -1..rank-1, (row0 + n_rows) * rank beyond
 * 63 bits, d_out NULL with n_rows > 0 -> ERR_INVALID, before a device is touched; n_rows == 0 -> OK, nothing is launched. */
int rsparse_hip_init_factors_device(uint64_t seed, int stream, int64_t row0, int n_rows, int rank, int64_t ld, double scale,
                                    int abs_values, int ones_col, void* d_out /* float */, void* hip_stream);
int rsparse_hip_init_factors_f64_device(uint64_t seed, int stream, int64_t row0, int n_rows, int rank, int64_t ld, double scale,
                                        int abs_values, int ones_col, void* d_out /* double */, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * negative sampling on the device: the candidate rows of a sampled-metric evaluation
 * ---------------------------------------------------------------------------------------------- */

/* Sampled-negative evaluation ranks every user's held-out items against n items the user has not interacted with
 * (rsparse_hip_top_candidates* on the rows, rsparse_hip_ranking_metrics* on the lists).  These entries make the rows: for row u of
 * the CSR pattern `seen` (the exclusion list: columns ascending, unique, inside [0, n_item)) the items of row u of `keep` (a
 * subset of the seen row, ascending and unique; both keep pointers NULL = nothing is kept) merged in ascending order with
 * min(n, M) items drawn uniformly WITHOUT replacement from the M = n_item - |seen_u| items outside the seen row.  The stream is
 * DEFINED here, so that any host can reproduce a row; rsparse_amd/rng.py (sample_negatives) is the definition in numpy.
 *
 *   Ranks.     The M admissible items of a row are numbered by rank 0 .. M - 1 in ascending item order:
 *              item(r) = r + #{i : seen_u[i] - i <= r}  (seen_u[i] - i does not decrease: a binary search).
 *   Draw t.    t = 0, 1, 2, ... of the row with GLOBAL index g = row0 + u: Philox4x32-10 (the rounds above) with key
 *              (lo32(seed), hi32(seed)) and counter (lo32(t >> 1), g, 2, hi32(t >> 1)) -- word 2 is the stream id, 0 and 1 are
 *              the factor streams -- gives o0..o3; w = o1 * 2^32 + o0 for even t, o3 * 2^32 + o2 for odd t; the drawn rank is
 *              floor(w * M / 2^64) = (o_hi * M + ((o_lo * M) >> 32)) >> 32, exact in 64-bit unsigned arithmetic for M < 2^31,
 *              with a bias of at most M / 2^64.
 *   Chosen.    n >= M: every rank.  Otherwise d = min(n, M - n) and D = the first d DISTINCT values of the draw sequence; the
 *              chosen ranks are D when 2 n <= M and every rank except D otherwise (the row draws what it leaves out, so no row
 *              needs more than about M ln 2 draws).
 *   Row.       keep_u and the items of the chosen ranks, ascending: |keep_u| + min(n, M) entries; out_p / out_j are a canonical
 *              CSR pattern from 0.
 * A row therefore depends on (seed, g, seen_u, keep_u, n_item, n) only -- not on the rows sampled with it (rows [a, b) sampled
 * with row0 = a are rows a .. b - 1 of the whole), the number of devices, or the device; and "the first d distinct values" does
 * not depend on the order in which draws are evaluated.
 *
 * _device: every pointer is device memory; seen_p / keep_p (n_rows + 1 slots) may be a slice of a larger pattern's row pointers
 * (absolute positions into seen_j / keep_j).  d_out_p (n_rows + 1) is computed on the device from the lengths of the rows; the
 * call then waits for the stream once to read back out_p[n_rows] and refuses, BEFORE anything is sampled, row pointers that are
 * negative or decrease, a seen row longer than n_item, a keep row longer than its seen row, a total beyond 2^31 - 1 or beyond
 * out_capacity (the entries d_out_j has room for: n_rows * n + the keep entries always suffices) -> ERR_INVALID.  Exactly
 * out_p[n_rows] entries of d_out_j are written.  The contents of the lists are the caller's contract here (a keep row that is no
 * subset of its seen row gives a wrong row, never a write outside it); the host form checks them.
 * 1 <= n <= RSPARSE_HIP_MAX_NEGATIVES, n_item < 2^31, row0 + n_rows <= 2^32, seen rows of any length.
 *
 * Host form: host pointers, p from 0.  out_p is always written; with out_j == NULL the call returns after that (out_p[n_rows] is
 * the capacity a second call needs), otherwise out_capacity must be at least out_p[n_rows].  seen / keep indices out of range,
 * not strictly ascending, or a keep row that is not a subset of its seen row -> ERR_INVALID.
 *
 * Both: a NULL seen_p, seen_j or out_p (the device form: or d_out_j), only one of keep_p / keep_j, n_rows < 0, n_item < 0, n < 1,
 * row0 < 0, out_capacity < 0 -> ERR_INVALID; n > RSPARSE_HIP_MAX_NEGATIVES -> ERR_UNSUPPORTED; all before a device is touched.
 * n_rows == 0 -> OK, nothing is launched. */
#define RSPARSE_HIP_MAX_NEGATIVES 8192
int rsparse_hip_sample_negatives_device(uint64_t seed, int64_t row0, int n_rows, int n_item, int n, const int32_t* d_seen_p,
                                        const int32_t* d_seen_j, const int32_t* d_keep_p, const int32_t* d_keep_j,
                                        int32_t* d_out_p, int32_t* d_out_j, int64_t out_capacity, void* hip_stream);
int rsparse_hip_sample_negatives(uint64_t seed, int64_t row0, int n_rows, int n_item, int n, const int32_t* seen_p,
                                 const int32_t* seen_j, const int32_t* keep_p, const int32_t* keep_j, int32_t* out_p, int32_t* out_j,
                                 int64_t out_capacity);

/* Popularity-weighted negatives: the rows of rsparse_hip_sample_negatives* with the negatives drawn in proportion to integer item
 * weights instead of uniformly (the "pop100" protocol of evaluation toolkits, count^0.75 sampling).  The stream is DEFINED here;
 * rsparse_amd/rng.py (sample_negatives_weighted) is the definition in numpy.
 *
 *   Weights.   w[0 .. n_item) are unsigned 32-bit integers, every one >= 1 (a zero is refused: "never a negative" is the job of
 *              the seen rows).  C[i] = w[0] + ... + w[i] in 64 bits, the inclusive prefix; W = C[n_item - 1] < 2^63, which always
 *              holds for n_item < 2^31.
 *   Draw t.    t = 0, 1, 2, ... of the row with GLOBAL index g = row0 + u: Philox4x32-10 with key (lo32(seed), hi32(seed)) and
 *              counter (lo32(t >> 1), g, 5, hi32(t >> 1)) -- stream id 5; 0 .. 4 are the factor, negatives and split streams --
 *              gives o0..o3; v = o1 * 2^32 + o0 for even t, o3 * 2^32 + o2 for odd t (the word pairing of stream 2);
 *              r = floor(v * W / 2^64), the high 64 bits of the 128-bit product; item = #{i : C[i] <= r}.
 *   Chosen.    M = n_item - |seen_u|.  n >= M: every admissible item, nothing is drawn.  Otherwise A = the first n DISTINCT
 *              values, in the order of the draw sequence, among the draws t = 0 .. B(n) - 1 that are NOT in seen_u, with the
 *              budget B(n) = 64 * n + 4096.  If the budget ends with |A| < n, the row is FILLED with the n - |A| admissible items
 *              of lowest item number that are not in A, and counts as a filled row.  The budget is part of the definition, so
 *              that no input can make a row spin: ordinary weights (Zipf counts to the power 0.75 or 1 over 1 M items, the most
 *              popular items in the seen row) complete within 2 n draws; weights such as [2^31, 1, 1, ...] fill, by design.
 *   Row.       keep_u and the chosen items, ascending: |keep_u| + min(n, M) entries, exactly as for the uniform sampler.
 * A row depends on (seed, g, seen_u, keep_u, w, n) only -- not on the rows sampled with it, the batch, the number of devices or
 * the device.
 *
 * rsparse_hip_weights_prefix_device writes C (n_item 64-bit words, device memory) from w (device memory) and waits for the stream
 * once to learn whether a weight is 0 -> ERR_INVALID.  n_item < 0, a NULL d_w or d_cum -> ERR_INVALID before a device is touched;
 * n_item == 0 -> OK, nothing is launched.  The prefix serves any number of sampling calls over the same weights.
 *
 * rsparse_hip_sample_negatives_weighted_device / rsparse_hip_sample_negatives_weighted are rsparse_hip_sample_negatives_device /
 * rsparse_hip_sample_negatives with that stream: the same arguments, checks (in the same order), status codes, out_p and
 * out_capacity rules.  In addition: d_cum (the device form: the prefix above, n_item words; its contents are the caller's
 * contract) or w (the host form: n_item weights, host memory) is NULL -> ERR_INVALID before a device is touched; the host form
 * refuses a zero weight -> ERR_INVALID, and checks the lists as the uniform host form does.  d_filled_rows (device memory, one
 * int32) / filled_rows (host, one int64) may be NULL; otherwise the call zeroes it and then counts the filled rows in it.
 * 1 <= n <= RSPARSE_HIP_MAX_NEGATIVES; n_rows == 0 -> OK, nothing is launched. */
int rsparse_hip_weights_prefix_device(const uint32_t* d_w, int n_item, uint64_t* d_cum, void* hip_stream);
int rsparse_hip_sample_negatives_weighted_device(uint64_t seed, int64_t row0, int n_rows, int n_item, int n, const int32_t* d_seen_p,
                                                 const int32_t* d_seen_j, const int32_t* d_keep_p, const int32_t* d_keep_j,
                                                 const uint64_t* d_cum, int32_t* d_out_p, int32_t* d_out_j, int64_t out_capacity,
                                                 int32_t* d_filled_rows, void* hip_stream);
int rsparse_hip_sample_negatives_weighted(uint64_t seed, int64_t row0, int n_rows, int n_item, int n, const int32_t* seen_p,
                                          const int32_t* seen_j, const int32_t* keep_p, const int32_t* keep_j, const uint32_t* w,
                                          int32_t* out_p, int32_t* out_j, int64_t out_capacity, int64_t* filled_rows);

/* Train / test split of an interaction matrix: every stored entry of the CSR (p, j, v) -- canonical: columns ascending and unique
 * within a row; stored zeros count as entries -- goes to exactly one of two CSR matrices, `train` and `test`, in its order, with
 * its index and its value (copied as an opaque word of value_bytes = 4 or 8 bytes; 0 = the pattern only, v and the value outputs
 * NULL).  The stream is DEFINED here, so that any host can reproduce a row; rsparse_amd/rng.py (split_flags) is the definition
 * in numpy.  Row u has the GLOBAL index g = row0 + u and L entries; an entry is named by its position t = 0 .. L - 1 in the row;
 * the key is (lo32(seed), hi32(seed)); word 2 of the counter is the stream id (0, 1 the factor streams, 2 the negatives).
 *
 *   RSPARSE_HIP_SPLIT_PROPORTION   Philox4x32-10 with counter (t >> 2, g, 3, 0) gives o0..o3; the entry takes word o[t & 3] and
 *              is TEST iff word < test_threshold, compared in 64 bits.  test_threshold = floor(p * 2^32) is an integer in
 *              [0, 2^32] (exact for a double p): 0 puts nothing in test, 2^32 everything.  Every entry is test independently
 *              with probability p.  leave_out, min_train are ignored; `by` must be NULL.
 *   RSPARSE_HIP_SPLIT_LEAVE_OUT    exactly h = min(leave_out, max(L - min_train, 0)) entries of the row are test (leave_out >= 1,
 *              min_train >= 0).  Every entry has a 64-bit key w; the test entries are the first h of the total order in which a
 *              comes before b iff w_a > w_b, or w_a = w_b and t_a < t_b.
 *                by == NULL: counter (t >> 1, g, 4, 0); w = o1 * 2^32 + o0 for even t, o3 * 2^32 + o2 for odd t (the word
 *                  pairing of the negatives' draw).
 *                by != NULL (one double per stored entry, addressed like j: a timestamp, for a temporal leave-last-out): with u =
 *                  the bits of by[t], w = ~u if the sign bit is set, else u | 2^63 -- the order-preserving map, so the h LARGEST
 *                  values are held out and ties go to the lower position; -0.0 therefore orders just below +0.0.  No random
 *                  word is used and seed is ignored.  NaN has no place in the order: the host form refuses it, the device form
 *                  leaves it to the caller (a NaN is then ordered by its bits; nothing is written out of place).
 * A flag depends on (seed, g, t, the mode's parameters) and, in leave-out mode, on the row's L or `by` values -- not on the rows
 * split together (rows [a, b) split with row0 = a are rows a .. b - 1 of the whole), the number of devices, or the device.
 * Limits: row0 + n_rows <= 2^32, L < 2^31, fewer than 2^31 entries in all (int32 row pointers).
 *
 * _device: every pointer is device memory; d_p (n_rows + 1 slots) may be a slice of a larger pattern's row pointers (absolute
 * positions into d_j / d_v / d_by).  d_train_p and d_test_p (n_rows + 1 each, from 0) are always written (n_rows >= 1), from counts made on
 * the device; the call then waits for the stream once to read both totals back and refuses, BEFORE anything else is written, row
 * pointers that are negative or decrease and a total beyond its capacity (the entries the train / test outputs have room for)
 * -> ERR_INVALID.  With d_train_j == NULL and d_test_j == NULL the call returns after the row pointers (train_p[n_rows] and
 * test_p[n_rows] are the capacities a second call needs).  Repeat calls are bit-identical.
 *
 * Host form: host pointers, p from 0; additionally checks that the columns of every row ascend strictly and that `by` holds no
 * NaN -> ERR_INVALID.
 *
 * Both: a NULL p, j, train_p or test_p; only one of the two j outputs; n_rows < 0; row0 < 0; row0 + n_rows > 2^32; a mode other
 * than the two; test_threshold > 2^32 or `by` in proportion mode; leave_out < 1 or min_train < 0 in leave-out mode; value_bytes
 * not in {0, 4, 8}; v without value_bytes (or value_bytes without v); value outputs missing where the j outputs and values are
 * given; a negative capacity -> ERR_INVALID, all before a device is touched.  n_rows == 0 -> OK, nothing is launched; the device form then
 * writes nothing at all (not even slot [0] of the row pointers), the host form writes train_p[0] = test_p[0] = 0. */
#define RSPARSE_HIP_SPLIT_PROPORTION 0
#define RSPARSE_HIP_SPLIT_LEAVE_OUT 1
int rsparse_hip_split_rows_device(uint64_t seed, int64_t row0, int n_rows, int mode, uint64_t test_threshold, int leave_out,
                                  int min_train, const int32_t* d_p, const int32_t* d_j, const void* d_v, int value_bytes,
                                  const double* d_by, int32_t* d_train_p, int32_t* d_train_j, void* d_train_v, int32_t* d_test_p,
                                  int32_t* d_test_j, void* d_test_v, int64_t train_capacity, int64_t test_capacity,
                                  void* hip_stream);
int rsparse_hip_split_rows(uint64_t seed, int64_t row0, int n_rows, int mode, uint64_t test_threshold, int leave_out, int min_train,
                           const int32_t* p, const int32_t* j, const void* v, int value_bytes, const double* by, int32_t* train_p,
                           int32_t* train_j, void* train_v, int32_t* test_p, int32_t* test_j, void* test_v, int64_t train_capacity,
                           int64_t test_capacity);

/* Confidence weighting of the interaction matrix (the reference's `preprocess` hook, R/model_WRMF.R:184-188, and its
 * ScaleNormalize): rsparse_amd/confidence.py (confidence_reference) is the definition in numpy.  A matrix is (p, i, x): n_seg
 * segments with p[0] = 0 and p[n_seg] = nnz (the rows of the user-major arrays, the columns of the item-major ones), int32
 * indices, double values.  x is users x items, v a stored value at (u, i); fitted on the training matrix: N its number of rows,
 * df_i the stored entries of column i, idf_i = log(N) - log1p(df_i), sbar = (sum of all values) / N.
 *
 *   RSPARSE_HIP_CONFIDENCE_LINEAR     1 + a v                                                     a = alpha
 *   RSPARSE_HIP_CONFIDENCE_LOG        1 + a log1p(v / b)                                          a = alpha, b = eps
 *   RSPARSE_HIP_CONFIDENCE_TFIDF      sqrt(v) idf_i
 *   RSPARSE_HIP_CONFIDENCE_BM25       ((v (a + 1)) / (K1L_u + v)) idf_i                           a = K1; the user table holds K1 L_u
 *   RSPARSE_HIP_CONFIDENCE_NORMALIZE  v t, t the entry of the ONE table that is given (of the segment or of the index)
 * in double, in the order written, without contraction.
 *
 * _moments_device: d_out[r] = sum over segment r of |x|^power (power 1 or 2; 0 for an empty segment), *d_total = the sum over
 * all entries.  Fixed summation order, no floating-point atomics: repeat calls are bit-identical; nothing is read back.
 * _table_device: d_out[r], r < n, from
 *   RSPARSE_HIP_CONFIDENCE_TABLE_IDF   log(a) - log1p(d_p[r + 1] - d_p[r])                        a = N; d_p of the item-major arrays
 *   RSPARSE_HIP_CONFIDENCE_TABLE_BM25  a ((1 - b) + (b d_moment[r]) / sbar), sbar = *d_total / c   a = K1, b = B, c = N of the fit;
 *                                      sbar == 0: (b d_moment[r]) / sbar is replaced by b
 *   RSPARSE_HIP_CONFIDENCE_TABLE_NORM  n^(a - 1) where n != 0, else 0; n = d_moment[r] (b = 1) or sqrt(d_moment[r]) (b = 2)   a = scale
 * _apply_device: d_out[e] = f_kind(d_x[e], user table, item table) for every stored entry.  d_seg_table has one entry per segment,
 * d_idx_table (n_idx entries) is gathered by d_i[e]; seg_is_item says which of the two is the item table (1: the item-major
 * arrays).  A kind takes the tables it needs and NULL for the others.  d_out: doubles (out_float = 0; may be d_x itself) or
 * floats (out_float = 1: the double result rounded once; must not overlap d_x).  The same cell gets the same bits from either
 * orientation.  An index outside [0, n_idx) gives NaN at its entry and reads nothing.
 *
 * rsparse_hip_confidence: host pointers; fits on the CSR (p, j, x) of an n_rows x n_cols matrix (p from 0) and writes the weighted
 * values in its order.  NORMALIZE: a = scale, norm in {1, 2}, along the rows (by_columns = 0) or the columns (1).
 *
 * All: a NULL array where a length is positive, negative dimensions, an unknown kind or table, a power / norm outside {1, 2}, a
 * missing or surplus table, b == 0 for LOG, an overlapping float output -> ERR_INVALID before a device is touched.  Nothing is
 * launched for n == 0 / nnz == 0 (moments then zero d_out and *d_total). */
#define RSPARSE_HIP_CONFIDENCE_LINEAR 0
#define RSPARSE_HIP_CONFIDENCE_LOG 1
#define RSPARSE_HIP_CONFIDENCE_TFIDF 2
#define RSPARSE_HIP_CONFIDENCE_BM25 3
#define RSPARSE_HIP_CONFIDENCE_NORMALIZE 4
#define RSPARSE_HIP_CONFIDENCE_TABLE_IDF 0
#define RSPARSE_HIP_CONFIDENCE_TABLE_BM25 1
#define RSPARSE_HIP_CONFIDENCE_TABLE_NORM 2
int rsparse_hip_confidence_moments_device(int n_seg, int64_t nnz, const int32_t* d_p, const double* d_x, int power, double* d_out,
                                          double* d_total, void* hip_stream);
int rsparse_hip_confidence_table_device(int table, int n, const int32_t* d_p, const double* d_moment, const double* d_total, double a,
                                        double b, double c, double* d_out, void* hip_stream);
int rsparse_hip_confidence_apply_device(int kind, int n_seg, int64_t nnz, const int32_t* d_p, const int32_t* d_i, const double* d_x,
                                        const double* d_seg_table, const double* d_idx_table, int n_idx, int seg_is_item, double a,
                                        double b, void* d_out, int out_float, void* hip_stream);
int rsparse_hip_confidence(int kind, int n_rows, int n_cols, const int32_t* p, const int32_t* j, const double* x, double a, double b,
                           int norm, int by_columns, double* out);

/* The interaction matrix from an event log: one record (user, item[, value][, timestamp]) per event -- a play, a click, a
 * purchase -- becomes the canonical CSR over the CELLS, the distinct (user, item) pairs that occur: rows in order, columns
 * ascending and unique within a row, empty rows included; a cell whose aggregate is 0 stays a stored entry.
 * rsparse_amd/events.py (events_reference) is the definition in numpy.  The events of a cell are taken in INPUT order.
 *
 *   count[c]    the number of events of the cell
 *   latest[c]   the largest timestamp of the cell, compared through the order-preserving 64-bit map of the double's bits that
 *               the split defines above (RSPARSE_HIP_SPLIT_LEAVE_OUT, by != NULL): exact, and -0.0 orders below +0.0
 *   x[c]        RSPARSE_HIP_EVENTS_SUM    the sum of the cell's terms in the order stated below
 *               RSPARSE_HIP_EVENTS_COUNT  count[c] as a double
 *               RSPARSE_HIP_EVENTS_MAX    the largest value, by the same bit map
 *               RSPARSE_HIP_EVENTS_LAST   the value of the event with the largest timestamp; ties go to the event LATER in the
 *                                         input (needs timestamps)
 * values == NULL means every value is 1.0.  The term of an event is its value v; with half_life > 0 (SUM only, needs timestamps)
 * it is v * exp2((t - now) / half_life), every operation in double, without contraction; now is the argument when has_now != 0,
 * else the largest timestamp of the log (by the bit map).  A cell of m <= 64 events is summed left to right in input order,
 * starting from its first term.  A longer cell is cut into consecutive chunks of 64 events counted from its first event; every
 * chunk is summed left to right, and the chunk sums are then summed left to right.  No floating-point atomics: the result is the
 * reference's bit for bit (with a half life: up to the two libraries' exp2), and repeat calls are bit-identical.
 *
 * _device: every pointer is device memory except n_cells.  d_users / d_items: n_events ids each; d_values, d_timestamps: n_events
 * doubles or NULL.  d_p has n_users + 1 slots; d_j, d_x, d_count, d_latest have `capacity` slots each (n_events always
 * suffices; d_count and d_latest may be NULL; d_latest is not written without timestamps).  *n_cells receives the number of
 * cells.  The call waits for the stream: after its first launch, to refuse an id outside [0, n_users) x [0, n_items) ->
 * ERR_INVALID with nothing else written; after the cells are counted, to refuse a capacity below *n_cells -> ERR_INVALID with no
 * output array written; and before it returns (its scratch, 16 or 24 bytes per event -- keys of 32 bits when
 * bits(n_users) + bits(n_items) <= 32, bits(n) = the bits that hold 0 .. n - 1 -- plus about one byte per event, is freed then).
 * A NaN has no place in the order of max / last / latest: the host form refuses it, the device form leaves it to the caller.
 *
 * Host form: host pointers; refuses a NaN in values or timestamps -> ERR_INVALID.
 *
 * Both: n_cells or p NULL; users or items NULL with n_events > 0; j or x NULL with n_events > 0; a negative n_events, n_users,
 * n_items or capacity; n_events >= 2^31; an aggregate other than the four; LAST or a half life without timestamps; a half life
 * with another aggregate than SUM (half_life <= 0 means none) -> ERR_INVALID before a device is touched.  n_events == 0 -> OK:
 * p is all zeros and *n_cells = 0. */
#define RSPARSE_HIP_EVENTS_SUM 0
#define RSPARSE_HIP_EVENTS_COUNT 1
#define RSPARSE_HIP_EVENTS_MAX 2
#define RSPARSE_HIP_EVENTS_LAST 3
int rsparse_hip_events_to_csr_device(int64_t n_events, int n_users, int n_items, const int32_t* d_users, const int32_t* d_items,
                                     const double* d_values, const double* d_timestamps, int aggregate, double half_life, double now,
                                     int has_now, int32_t* d_p, int32_t* d_j, double* d_x, int32_t* d_count, double* d_latest,
                                     int64_t capacity, int64_t* n_cells, void* hip_stream);
int rsparse_hip_events_to_csr(int64_t n_events, int n_users, int n_items, const int32_t* users, const int32_t* items,
                              const double* values, const double* timestamps, int aggregate, double half_life, double now, int has_now,
                              int32_t* p, int32_t* j, double* x, int32_t* count, double* latest, int64_t capacity, int64_t* n_cells);

/* ------------------------------------------------------------------------------------------------
 * (3) fp64 device layer: als_implicit<double> / als_explicit<double> with the data resident in HBM
 * ---------------------------------------------------------------------------------------------- */

/* What the `*_double` .Call targets compute (src/wrmf_implicit.cpp:5-14, src/wrmf_explicit.cpp:5-14), device-resident
 * like layer (2): CSC with f64 values, X / Y / XtX column-major f64.  One kernel family covers every variant -- implicit
 * and explicit feedback, Cholesky (general-solver fallback included) / conjugate gradient / NNLS, user/item biases, the
 * implicit global bias -- by assembling each row's system in LDS (wrmf_f64.hip); it is the parity path of
 * precision = "double", not the bench path. */
typedef struct rsparse_hip_csc_f64 rsparse_hip_csc_f64;

/* adopt arrays that live on the current device (not copied, not freed; they must outlive the handle); validated like
 * rsparse_hip_csc_create_device */
int rsparse_hip_csc_f64_create_device(int n_rows, int n_cols, const int32_t* d_col_ptrs, const int32_t* d_row_indices,
                                      const double* d_values, rsparse_hip_csc_f64** out);
int rsparse_hip_csc_f64_destroy(rsparse_hip_csc_f64* m);
/* Conjugate gradient in double: a row of more than min_len non-zeros is cut into chunks of chunk_len that run as waves of their
 * own, pass by pass (wrmf_f64.hip, "long rows": one wave per row left a half-iteration waiting for its longest row; sums in
 * chunk order, no atomics).  Defaults 2048 / 1024 (0 = restore the default); applies to the handles made -- and the stateless
 * *_double calls issued -- afterwards.  Results do not depend on it beyond rounding (1e-12); the tests lower it so that small
 * matrices take the path. */
int rsparse_hip_set_f64_long_rows(int min_len, int chunk_len);

/* XtX = X X^T + fl(lambda) I in f64 (the ridge is rounded to fp32 in the double build too: float::fl(diag(lambda)),
 * R/model_WRMF.R:476); d_sumsq_out (nullable) = sum(X^2) */
int rsparse_hip_gramian_f64_device(const double* d_X, int rank, int64_t n, double lambda, double* d_XtX_out,
                                   double* d_sumsq_out, void* stream);

/* One half-iteration in f64: als_implicit<double> (implicit != 0; inst/include/wrmf_implicit.hpp:90-305) or
 * als_explicit<double> (wrmf_explicit.hpp:33-174) over the columns of `conf`.  Arguments as in layer (2):
 * with_biases / is_x_bias_last_row select the user/item-bias layout (rank counts the two extra coordinates; d_XtX is
 * then (rank-1) x (rank-1)); global_bias (implicit feedback; below sqrt(DBL_EPSILON) = none, :108-109) is handled with
 * every solver, global_bias_base = -global_bias * rowSums(X) computed on the device; dynamic_lambda: explicit feedback
 * only.  implicit + with_biases + conjugate_gradient -> RSPARSE_HIP_ERR_UNSUPPORTED (:189,197).  d_loss_rows_out
 * (nullable, device double[1]): the row part of the loss as for rsparse_hip_als_{implicit,explicit}_device.  A system
 * that is not positive definite is re-solved by Gaussian elimination with partial pivoting inside the kernel and counted
 * in rsparse_hip_take_numeric_failures. */
int rsparse_hip_als_f64_device(const rsparse_hip_csc_f64* conf, int implicit, const double* d_X, double* d_Y,
                               const double* d_XtX, int rank, double lambda, unsigned solver, unsigned cg_steps,
                               int dynamic_lambda, int with_biases, int is_x_bias_last_row, double global_bias,
                               double* d_loss_rows_out, void* stream);

/* initialize_biases_double (src/wrmf_init.cpp:5-19 -> inst/include/wrmf_utils.hpp:32-165), device-resident: c_ui =
 * users x items by item column, c_iu = its transpose.  With is_explicit_feedback and calculate_global_bias the mean of
 * the values is removed from the resident values of BOTH handles in place. */
int rsparse_hip_initialize_biases_f64_device(rsparse_hip_csc_f64* c_ui, rsparse_hip_csc_f64* c_iu, double* d_user_bias,
                                             double* d_item_bias, double lambda, int dynamic_lambda, int non_negative,
                                             int calculate_global_bias, int is_explicit_feedback,
                                             double* global_bias_out, void* stream);

/* f64 counterparts of the single bias sweeps (rsparse_hip_bias_*_device above) */
int rsparse_hip_bias_sweep_explicit_f64_device(const rsparse_hip_csc_f64* conf, const double* d_other_bias, double lambda,
                                               int dynamic_lambda, int non_negative, double* d_out, void* stream);
int rsparse_hip_bias_prep_implicit_f64_device(const rsparse_hip_csc_f64* conf, int n_other, double lambda, double* d_means,
                                              double* d_adj, void* stream);
int rsparse_hip_bias_sweep_implicit_f64_device(const rsparse_hip_csc_f64* conf, const double* d_other_bias, int n_other,
                                               const double* d_other_sum, const double* d_means, const double* d_adj,
                                               int non_negative, double global_bias, double* d_out, void* stream);

/* f64 counterparts of rsparse_hip_values_subtract_mean_device / rsparse_hip_weighted_sumsq_device */
int rsparse_hip_values_subtract_mean_f64_device(int64_t n, double* d_x, double* d_x_other, double* mean_out, void* stream);
int rsparse_hip_weighted_sumsq_f64_device(const double* d_X, int rank, int64_t n, const double* d_w, double* d_out,
                                          void* stream);

/* Kernel timing for measurement harnesses (bench.py): when enabled, every device-layer call brackets
 * its kernels with HIP events on the caller's stream.  rsparse_hip_profile_last() waits for the last
 * call and returns milliseconds per segment in launch order:
 *   CG half-iterations -> [0..5] the launches of the row-length buckets of rsparse_hip_csc_info ([0] = the
 *     normal-equation kernel for the rows beyond 512 non-zeros), [6] loss reduction (with the LDS-tile fallback kernels
 *     for ranks that are not a multiple of 4: [0] short-row, [1] long-row, [2] loss);
 *   Cholesky -> [0] the normal-equation launch with the exact solve (long rows), [1] the low-rank kernel (short rows,
 *     incl. its one-workgroup preparation), [2] the k x k kernel, [3] loss reduction;
 *   NNLS -> [0] kernel, [2] loss reduction;   Gramian -> [0] MFMA partial kernel, [1] reduction.
 * rsparse_hip_profile_last_names() gives, for the same call, the name of the kernel each segment timed -- newline
 * separated, an empty line for a segment that launched nothing -- taken from the runtime's own symbol table
 * (hipKernelNameRefByPtr, demangled), i.e. exactly what rocprofv3 prints for it. */
int rsparse_hip_profile_enable(int on);
int rsparse_hip_profile_last_names(char* buf, int cap);
/* How the launches of one conjugate-gradient half-iteration (one per row-length bucket, disjoint rows) are issued:
 * 2 (default) = the long-row launch on the caller's stream, the others on side streams forked from / joined to it,
 * 1 = every launch on a side stream, 0 = all back to back on the caller's stream -- what a profiler needs for
 * well-defined per-kernel durations (bench.py --serial-launches).  Results do not depend on it. */
int rsparse_hip_set_launch_mode(int mode);
int rsparse_hip_profile_last(double ms_out[8]);

/* The exact (Cholesky) solver's bookkeeping since the last call of this function; resets.  A per-row system whose
 * factorisation meets a non-positive pivot is re-solved on the device by Gaussian elimination with partial pivoting -- what
 * arma::solve(lhs, rhs, fast + likely_sympd) falls back to behind a warning (inst/include/wrmf_implicit.hpp:236,
 * wrmf_explicit.hpp:108): *fallback_out (nullable) = the number of such rows, the reference's warnings.  *unresolved_out =
 * the rows whose general solve failed too (an exactly singular system; their solution was set to zero): the half-iteration
 * entry points report them as RSPARSE_HIP_ERR_NUMERIC (the stateless ones at once, the device-resident ones through this
 * call).  Reads device memory: synchronises. */
int rsparse_hip_take_numeric_failures(int64_t* unresolved_out, int64_t* fallback_out);

/* ------------------------------------------------------------------------------------------------
 * (4) multi-GPU context: the sharded driver inside the library (ABI version 6)
 * ---------------------------------------------------------------------------------------------- */

/* What the reference's host calls per half-iteration is ONE function that internally drives its OpenMP threads
 * (`als_implicit_double(c_ui, X, Y, XtX, ...)`, R/model_WRMF.R:111-147 -> src/RcppExports.cpp:371-415,
 * inst/include/wrmf_implicit.hpp:162-175 `#pragma omp parallel for`); this layer is the same contract over 1..8 GPUs: the caller
 * stays ONE host thread (an R session), the library runs one persistent host thread per device, shards users and items over
 * them in contiguous nnz-balanced blocks, keeps full factor replicas, and per half-iteration issues one fused exchange of the
 * k x k Gramian partials (+ sum(F^2), max |F|), an in-place all-gather of every solved sub-block (overlapped with the next
 * sub-block's solve on a second stream) and one all-reduce of the loss terms -- SURVEY.md 8(e).  The per-rank arithmetic is
 * layer (2)'s, row for row: results do not depend on the number of ranks except through the summation order of the Gramian
 * and of the loss (as the reference's do not depend on OMP_NUM_THREADS except through its loss reduction) -- and, with
 * implicit feedback on the matrix-core paths, through the power of two that scales their fp16 operand terms: it is taken from
 * the largest confidence among the values of a HANDLE, and the context holds one handle per rank and sub-block.  Explicit
 * feedback has neither a Gramian nor such a scale: its factors are the same bits at every number of ranks and sub-blocks
 * (tests/test_ctx_rows.py).
 *
 * comm_kind: RSPARSE_HIP_COMM_RCCL -- one device per rank, collectives = RCCL over xGMI (ncclCommInitAll; librccl is loaded
 * with dlopen when the context is created, a single-GPU user never needs it); RSPARSE_HIP_COMM_SHARED -- the ranks are threads
 * with streams of their own on ONE device (device_ids may repeat; default: all on device 0) and a collective is a host
 * barrier + device copies: the transport of the tests and of single-GPU dry runs, everything else is the production code.
 * device_ids: n_ranks entries, or NULL (RCCL: rank r on device r). */
typedef struct rsparse_hip_ctx rsparse_hip_ctx;
#define RSPARSE_HIP_COMM_RCCL 0
#define RSPARSE_HIP_COMM_SHARED 1
#define RSPARSE_HIP_SIDE_ITEMS 0 /* solve the item factors given the user factors (R/model_WRMF.R:321) */
#define RSPARSE_HIP_SIDE_USERS 1 /* solve the user factors given the item factors (:327) */
int rsparse_hip_ctx_create(int n_ranks, const int* device_ids, int comm_kind, rsparse_hip_ctx** out);
int rsparse_hip_ctx_destroy(rsparse_hip_ctx* ctx);

/* The interaction matrix in both orientations as the R driver holds them (R/model_WRMF.R:184-191): c_ui = users x items as
 * dgCMatrix slots (ui_p int32[n_item + 1], ui_i = user ids, ui_x), c_iu = its transpose (iu_p int32[n_user + 1], iu_i = item
 * ids, iu_x); host arrays, 0-based, row indices ascending inside a column.  Every rank uploads its own blocks only.
 * n_sub_users / n_sub_items: sub-blocks per rank and half-iteration (0 = default: 1 for one rank, else 4).
 * Both pointer arrays are checked before any rank is asked to do anything (from 0, non-decreasing, the same number of
 * non-zeros in the two orientations, indices inside the matrix): RSPARSE_HIP_ERR_INVALID with the array's name, and the
 * context is as it was before the call.  A call that passes these checks DROPS THE FACTORS of the context (the replicas are
 * stored in the order of the old matrix's blocks): until the next rsparse_hip_ctx_set_factors, half_iteration and
 * get_factors return RSPARSE_HIP_ERR_INVALID. */
int rsparse_hip_ctx_set_matrix(rsparse_hip_ctx* ctx, int n_user, int n_item, const int32_t* ui_p, const int32_t* ui_i,
                               const double* ui_x, const int32_t* iu_p, const int32_t* iu_i, const double* iu_x,
                               int n_sub_users, int n_sub_items);

/* Factor matrices as the reference passes them: U = rank x n_user, V = rank x n_item, column-major fp32 (every entity's vector
 * contiguous).  set: host -> every replica; get (either pointer may be NULL): rank 0's replica -> host. */
int rsparse_hip_ctx_set_factors(rsparse_hip_ctx* ctx, int rank, const float* U, const float* V);
int rsparse_hip_ctx_get_factors(rsparse_hip_ctx* ctx, float* U, float* V);

/* One half-iteration over all devices: als_implicit<float> / als_explicit<float>, no-bias branch, every solver of layer (2)
 * (the exact solve that ends a fit -- R/model_WRMF.R:355-359 -- is side = USERS with solver = cholesky after set_factors of
 * zeros for U).  implicit: the Gramian XtX + fl(lambda) I of the fixed side is formed inside (R/model_WRMF.R:474-486).
 * *loss_out (nullable) = the loss as the reference reports it: (row terms + lambda * regulariser) / nnz
 * (wrmf_implicit.hpp:286-304, wrmf_explicit.hpp:146-173).  Synchronous. */
int rsparse_hip_ctx_half_iteration(rsparse_hip_ctx* ctx, int side, int implicit, double lambda, unsigned solver,
                                   unsigned cg_steps, int dynamic_lambda, double* loss_out);

/* rsparse_hip_take_numeric_failures summed over the ranks (one decision for the whole context). */
int rsparse_hip_ctx_take_numeric_failures(rsparse_hip_ctx* ctx, int64_t* unresolved_out, int64_t* fallback_out);

/* info_out: [0] ranks, [1] comm_kind, [2] n_user, [3] n_item, [4] nnz, [5] rank of the factors, [6] / [7] sub-blocks per rank
 * (users / items), [8] / [9] rows per sub-block, [10] / [11] users / items owned by rank 0, [12] 1 = the collectives are RCCL.
 * times_out (nullable): of the last half-iteration, the slowest rank's [0] wall milliseconds, [1] milliseconds inside
 * collective calls (host side: issue time for RCCL, the whole exchange for SHARED). */
int rsparse_hip_ctx_info(const rsparse_hip_ctx* ctx, int64_t info_out[16], double times_out[2]);

#ifdef __cplusplus
}
#endif
#endif /* RSPARSE_WRMF_HIP_H */
