// Ranking metrics of top-k lists: ap@k and ndcg@k exactly as the reference's ap_k() / ndcg_k() define them (R/metrics.R:31-127),
// gfx950, wave64, double arithmetic throughout.
//
// Per user u with n_u stored entries in its row of `actual` (sorted column indices j, relevances x) and kk = min(k, n_u):
//   ap   = mean over i = 1..kk of (hits among the first i predictions) / i                          (ap_at_k, :93-98)
//   dcg  = sum over i <= kk of x[match(pred_i)] / log2(i + 1), misses contributing nothing            (dcg_at_k, :101-112)
//   idcg = sum over i <= kk of (the i-th largest x of the row) / log2(i + 1); 1 for an empty row      (idcg_at_k, :115-123)
//   ndcg = dcg / idcg.  An empty row: ap = NaN (mean(numeric(0))), ndcg = 0 / 1 = 0.
// A prediction is looked up on its own at every position (`%in%` / `match` are per element): NA_integer_ and indices outside the
// row are misses, a repeated index hits every time, a stored zero is a relevant item of relevance 0.
//
// Two launches:
//   1. metrics_rows_kernel: one wave per user, four users per workgroup.  A row of up to kMetRowCap entries is staged in LDS
//      (coalesced); lane l takes positions l, l + 64, ... of the user's list and binary-searches the row (LDS, or the row in
//      global memory when it is longer).  ap: a ballot prefix of the hits gives every position its running hit count.  idcg of
//      a staged row: its values sorted in LDS (bitonic, descending) after the lookups are done; a row whose values are all
//      equal skips the sort.  A longer row leaves dcg in ndcg_out[u] and appends u to a list for launch 2.
//   2. metrics_long_kernel: one 256-thread workgroup per listed user (grid-stride over the list, whose length only the device
//      knows).  The kk-th largest relevance by a radix select on order-preserving 64-bit keys (8 passes of 8 bits over the row
//      in global memory), the c < kk values strictly above it compacted into LDS and sorted (at most 8191 keys, 64 KiB), the
//      remaining kk - c places filled with the threshold value itself -- ties at the threshold do not change the sum.
// Sums are per-lane in a fixed position order, then a butterfly over the wave and, in launch 2, the four waves in order: no
// floating-point atomics, so a call repeats bit for bit.  (The list of launch 2 is filled in whatever order the waves reach it;
// every user's result depends on its own row alone.)
#include <algorithm>
#include <cmath>

#include "wrmf_internal.h"
#include "wrmf_device.h"

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kMetWaves = 4;            // users (waves) per workgroup of launch 1
constexpr int kMetRowCap = 512;         // rows up to this long: staged in LDS, idcg sorted there (a power of two)
constexpr int kMetLongThreads = 256;    // (what block_kth_largest is written for)
constexpr int kMetLongCap = 8192;       // keys launch 2 sorts in LDS: > the c < kk <= RSPARSE_HIP_MAX_TOPK_LARGE values above
constexpr int kMetLongGrid = 512;       // workgroups of launch 2 (two per CU: 66 KiB of LDS each)
constexpr int kNaInteger = INT32_MIN;   // RSPARSE_HIP_NA_INTEGER

__device__ __forceinline__ double discount(int i) {   // log2(i + 1), the divisor of the 1-based position i
  return log2((double)i + 1.0);
}

// first position in rj[0, n) holding t, or -1
__device__ __forceinline__ int row_find(const int32_t* rj, int n, int32_t t) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rj[mid] < t) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && rj[lo] == t) ? lo : -1;
}

template <bool AP, bool NDCG>
__global__ __launch_bounds__(64 * kMetWaves) void metrics_rows_kernel(const int32_t* __restrict__ pred, int n_users, int k,
                                                                       const int32_t* __restrict__ P, const int32_t* __restrict__ J,
                                                                       const double* __restrict__ X, double* __restrict__ ap_out,
                                                                       double* __restrict__ ndcg_out, int* __restrict__ long_list,
                                                                       int* __restrict__ long_count) {
  __shared__ int32_t s_j[kMetWaves][kMetRowCap];
  __shared__ double s_x[NDCG ? kMetWaves : 1][NDCG ? kMetRowCap : 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int u = blockIdx.x * kMetWaves + w;
  if (u >= n_users) return;   // (whole waves: nothing below synchronises across waves)
  const int p0 = P[u];
  const int n_u = max(P[u + 1] - p0, 0);
  const int kk = min(k, n_u);
  if (kk == 0) {
    if (lane == 0) {
      if (AP) ap_out[u] = __longlong_as_double(0x7ff8000000000000ll);   // mean(numeric(0))
      if (NDCG) ndcg_out[u] = 0.0;                                         // 0 / idcg, idcg = 1 (:118)
    }
    return;
  }
  const bool staged = n_u <= kMetRowCap;
  if (staged) {
    for (int e = lane; e < n_u; e += 64) {
      s_j[w][e] = J[p0 + e];
      if (NDCG) s_x[w][e] = X[p0 + e];
    }
    wave_sync();
  }
  const int32_t* rj = staged ? s_j[w] : J + p0;
  const double* rx = NDCG ? (staged ? s_x[w] : X + p0) : nullptr;
  const int32_t* prow = pred + (size_t)u * k;
  int carry = 0;
  double ap_acc = 0.0, dcg_acc = 0.0;
  for (int base = 0; base < kk; base += 64) {
    const int i = base + lane;
    int pos = -1;
    if (i < kk) {
      const int32_t c = prow[i];
      if (c != kNaInteger && c >= 1) pos = row_find(rj, n_u, c - 1);   // 1-based item -> 0-based column
    }
    if (AP) {
      const u64 m = __ballot(pos >= 0);
      const int cum = carry + __popcll(m & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull)));
      carry += __popcll(m);
      if (i < kk) ap_acc += (double)cum / (double)(i + 1);
    }
    if (NDCG && pos >= 0) dcg_acc += rx[pos] / discount(i + 1);
  }
  if (AP) {
    const double s = butterfly_sum(ap_acc);
    if (lane == 0) ap_out[u] = s / (double)kk;
  }
  if (!NDCG) return;
  const double dcg = butterfly_sum(dcg_acc);
  if (!staged) {   // idcg in launch 2; dcg waits in the output
    if (lane == 0) {
      ndcg_out[u] = dcg;
      long_list[atomicAdd(long_count, 1)] = u;
    }
    return;
  }
  // idcg: the row's values in descending order (every lookup above is done: sort them in place)
  double* sx = s_x[w];
  double lo = INFINITY, hi = -INFINITY;
  for (int e = lane; e < n_u; e += 64) {
    lo = fmin(lo, sx[e]);
    hi = fmax(hi, sx[e]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, o));
    hi = fmax(hi, __shfl_xor(hi, o));
  }
  double idcg_acc = 0.0;
  if (lo == hi) {   // all equal (binary hold-outs): v * sum 1 / log2(i + 1)
    for (int i = lane; i < kk; i += 64) idcg_acc += lo / discount(i + 1);
  } else {
    int n2 = 1;
    while (n2 < n_u) n2 <<= 1;   // <= kMetRowCap
    for (int e = n_u + lane; e < n2; e += 64) sx[e] = -INFINITY;
    wave_sync();
    for (int size = 2; size <= n2; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int t = lane; t < (n2 >> 1); t += 64) {
          const int a = 2 * t - (t & (stride - 1)), b = a + stride;
          const bool desc = (a & size) == 0;
          const double va = sx[a], vb = sx[b];
          if (desc ? (va < vb) : (va > vb)) {
            sx[a] = vb;
            sx[b] = va;
          }
        }
        wave_sync();
      }
    for (int i = lane; i < kk; i += 64) idcg_acc += sx[i] / discount(i + 1);
  }
  const double idcg = butterfly_sum(idcg_acc);
  if (lane == 0) ndcg_out[u] = dcg / idcg;
}

// workgroup (256) sum in a fixed order: per wave, then the waves in order, ((r0 + r1) + r2) + r3.  red: 4 doubles.
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  v = butterfly_sum(v);
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(kMetLongThreads) void metrics_long_kernel(int k, const int32_t* __restrict__ P,
                                                                       const double* __restrict__ X, double* __restrict__ ndcg_out,
                                                                       const int* __restrict__ long_list,
                                                                       const int* __restrict__ long_count) {
  __shared__ u64 s_key[kMetLongCap];
  __shared__ unsigned s_hist[256];
  __shared__ double s_red[4];
  __shared__ u64 s_res;
  __shared__ int s_rem, s_cnt;
  const int tid = threadIdx.x;
  const int n_long = *long_count;
  for (int q = blockIdx.x; q < n_long; q += gridDim.x) {
    const int u = long_list[q];
    const int p0 = P[u];
    const int n_u = P[u + 1] - p0;   // > kMetRowCap
    const int kk = min(k, n_u);
    const double* x = X + p0;
    // the kk-th largest: min / max first (an all-equal row needs no select)
    u64 kmin = ~0ull, kmax = 0ull;
    for (int e = tid; e < n_u; e += kMetLongThreads) {
      const u64 kx = f64_key(x[e]);
      kmin = min(kmin, kx);
      kmax = max(kmax, kx);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      kmin = min(kmin, (u64)__shfl_xor(kmin, o));
      kmax = max(kmax, (u64)__shfl_xor(kmax, o));
    }
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    if ((tid & 63) == 0) {
      s_key[2 * (tid >> 6)] = kmin;
      s_key[2 * (tid >> 6) + 1] = kmax;
    }
    __syncthreads();
    kmin = min(min(s_key[0], s_key[2]), min(s_key[4], s_key[6]));
    kmax = max(max(s_key[1], s_key[3]), max(s_key[5], s_key[7]));
    __syncthreads();
    const u64 thr = kmin == kmax ? kmin : block_kth_largest(n_u, kk, 64, [&](int e, bool& ok) { ok = true; return f64_key(x[e]); }, s_hist, &s_res, &s_rem);
    // the c < kk values strictly above the threshold, sorted descending by key (a total order: the result does not depend on
    // the order the compaction wrote them in)
    if (kmin != kmax) {
      for (int e = tid; e < n_u; e += kMetLongThreads) {
        const u64 kx = f64_key(x[e]);
        if (kx > thr) s_key[atomicAdd(&s_cnt, 1)] = kx;
      }
    }
    __syncthreads();
    const int c = s_cnt;   // < kk <= kMetLongCap
    int n2 = 1;
    while (n2 < c) n2 <<= 1;
    for (int e = c + tid; e < n2; e += kMetLongThreads) s_key[e] = 0ull;
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int t = tid; t < (n2 >> 1); t += kMetLongThreads) {
          const int a = 2 * t - (t & (stride - 1)), b = a + stride;
          const bool desc = (a & size) == 0;
          const u64 va = s_key[a], vb = s_key[b];
          if (desc ? (va < vb) : (va > vb)) {
            s_key[a] = vb;
            s_key[b] = va;
          }
        }
        __syncthreads();
      }
    const double tv = key_f64(thr);
    double acc = 0.0;
    for (int i = tid; i < kk; i += kMetLongThreads) acc += (i < c ? key_f64(s_key[i]) : tv) / discount(i + 1);
    const double idcg = block_sum(acc, s_red);
    if (tid == 0) ndcg_out[u] = ndcg_out[u] / idcg;
    __syncthreads();   // (s_key / s_cnt are reused by the next user)
  }
}

}  // namespace

hipError_t launch_ranking_metrics(const int32_t* pred, int n_users, int k, const int32_t* P, const int32_t* J, const double* X,
                                  double* ap_out, double* ndcg_out, int* long_buf, hipStream_t s) {
  if (n_users <= 0) return hipSuccess;
  int* long_count = long_buf;
  int* long_list = long_buf + 1;
  const dim3 grid((unsigned)((n_users + kMetWaves - 1) / kMetWaves)), block(64 * kMetWaves);
  if (ndcg_out) {
    hipError_t e = hipMemsetAsync(long_count, 0, sizeof(int), s);
    if (e != hipSuccess) return e;
  }
  if (ap_out && ndcg_out)
    hipLaunchKernelGGL((metrics_rows_kernel<true, true>), grid, block, 0, s, pred, n_users, k, P, J, X, ap_out, ndcg_out,
                       long_list, long_count);
  else if (ap_out)
    hipLaunchKernelGGL((metrics_rows_kernel<true, false>), grid, block, 0, s, pred, n_users, k, P, J, X, ap_out, ndcg_out,
                       long_list, long_count);
  else
    hipLaunchKernelGGL((metrics_rows_kernel<false, true>), grid, block, 0, s, pred, n_users, k, P, J, X, ap_out, ndcg_out,
                       long_list, long_count);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !ndcg_out) return e;
  hipLaunchKernelGGL(metrics_long_kernel, dim3((unsigned)std::min(n_users, kMetLongGrid)), dim3(kMetLongThreads), 0, s, k, P, X,
                     ndcg_out, long_list, long_count);
  return hipGetLastError();
}

}  // namespace rsparse_hip
