// EASE (rsparse_amd/ease.py is the definition): the rows of the item Gram matrix G + lambda I, and the top-k lists of users scored
// by a DENSE items x items weight matrix B.  gfx950, wave64.
//
// Gram rows.  The binary fit scatter of wrmf_itemknn.hip (launch_knn_fit_scatter, unchanged) counts the co-occurrences of a batch
// of items into dense uint32 rows of the ItemKNN workspace and leaves the diagonal out; ease_gram_rows_kernel turns the batch into
// rows of doubles -- double(c_ij) off the diagonal, double(n_i) + lambda (one rounding) on it -- and the rows are zeroed again
// behind it.  Integers below 2^32 convert exactly, so the rows equal the numpy definition bit for bit.
//
// Scores.  score_u = sum over the stored items i of row u, IN ASCENDING STORED ORDER, of double(B[i, :]): a sequential sum in a
// stated order, one rounding per step, no product (nothing to contract), no atomic.  This is a sparse row x dense matrix product
// that moves nnz x n_items x sizeof(B) bytes; it is bound by how the rows of B reach the CUs.
//   * a workgroup of 256 threads owns ONE row of x and ONE tile of 256 x 16 bytes of columns (1024 floats / 512 doubles); a
//     thread owns the 16 bytes at its place of the tile: one 16-byte load per item, a wave reads 1 KiB of a row of B at a time;
//   * the row's item indices are staged in LDS, kChunk at a time, and read from there wave-uniformly (readfirstlane: the row's
//     address is scalar, the thread's offset a constant);
//   * kAhead loads are issued before the first of them is added, so kAhead rows of B are in flight per thread; the adds then
//     follow in stored order into double registers;
//   * the grid is (rows of the batch, tiles) with the rows fastest: the workgroups resident at one time share a tile, so the
//     slab B[:, tile] (n_items x 4 KiB) is fetched from HBM about once per batch and otherwise comes from L2 / the Infinity Cache;
//   * ld_B is a multiple of 16 bytes (the class pads it to 256) and at least n_items, so a 16-byte load that starts inside the row
//     ends inside its padding: no column tail in the loads, the stores are guarded per column.
// A cell is written as the ORDER KEY of its double (bits flipped if negative, otherwise the sign bit set): keys order as unsigned
// integers the way the doubles order; an accumulator that starts at +0.0 never becomes -0.0; no finite score has the key 0 (the
// select's empty cell) or all ones (the mask's sentinel).  So the mask, the select (its kLists form) and the memset of
// wrmf_itemknn.hip run behind it as they are (launch_knn_mask_rows / launch_knn_select_lists / launch_knn_zero_rows): every unmasked cell is a
// candidate, a row of more than RSPARSE_HIP_KNN_LDS_CAND items takes the radix fallback, an empty row is the row of ties.
// A column index outside [0, n_items) is skipped (the host form refuses it).
#include <algorithm>

#include "../../include/rsparse_wrmf_hip.h"
#include "wrmf_internal.h"

namespace rsparse_hip {
namespace {

using u64 = unsigned long long;

constexpr int kThreads = 256;
constexpr int kChunk = RSPARSE_HIP_EASE_CHUNK;   // item indices of a row staged in LDS at a time
constexpr int kAhead = RSPARSE_HIP_EASE_AHEAD;   // rows of B a thread has in flight
static_assert(kChunk % kAhead == 0, "a staged chunk is whole groups of loads");
static_assert(kThreads * 16 == RSPARSE_HIP_EASE_TILE_BYTES, "a thread owns 16 bytes of the tile");
static_assert(RSPARSE_HIP_EASE_MAX_ITEMS <= 65535, "ease_gram_rows_kernel: a batch of item rows is the grid's y dimension");

// rows [0, n_batch) of the uint32 workspace are the co-occurrence counts of the items row0 + r, diagonal excluded
__global__ __launch_bounds__(kThreads) void ease_gram_rows_kernel(const unsigned* __restrict__ dense, int n_items, int row0,
                                                                  const int32_t* __restrict__ IP, double lambda,
                                                                  double* __restrict__ out, size_t ld_out) {
  const int i = row0 + (int)blockIdx.y;
  const unsigned* src = dense + (size_t)blockIdx.y * n_items;
  double* dst = out + (size_t)blockIdx.y * ld_out;
  const int j = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (j >= n_items) return;
  dst[j] = j == i ? (double)(IP[i + 1] - IP[i]) + lambda : (double)src[j];
}

template <class T>
struct Vec;
template <>
struct Vec<float> {
  using type = float4;
  static constexpr int n = 4;
};
template <>
struct Vec<double> {
  using type = double2;
  static constexpr int n = 2;
};

__device__ __forceinline__ void add_row(double (&acc)[4], const float4& v) {
  acc[0] += (double)v.x;
  acc[1] += (double)v.y;
  acc[2] += (double)v.z;
  acc[3] += (double)v.w;
}
__device__ __forceinline__ void add_row(double (&acc)[2], const double2& v) {
  acc[0] += v.x;
  acc[1] += v.y;
}

// the order key of a double: unsigned comparison of keys is the comparison of the doubles
__device__ __forceinline__ u64 order_key(double v) {
  const u64 b = (u64)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}

// grid: (rows of the batch, column tiles).  xp: the slots of this batch's rows (absolute positions into xj).
template <class T>
__global__ __launch_bounds__(kThreads) void ease_score_kernel(const int32_t* __restrict__ xp, const int32_t* __restrict__ xj,
                                                              int n_items, const T* __restrict__ B, size_t ld_B,
                                                              u64* __restrict__ dense, size_t ld) {
  using V = typename Vec<T>::type;
  constexpr int W = Vec<T>::n;
  __shared__ int s_idx[kChunk];
  const int tid = threadIdx.x;
  const int c0 = ((int)blockIdx.y * kThreads + tid) * W;   // the thread's first column
  const bool live = c0 < n_items;                          // (its 16 bytes start inside the row: they end inside ld_B)
  const int e0 = xp[blockIdx.x], e1 = xp[blockIdx.x + 1];
  double acc[W];
#pragma unroll
  for (int c = 0; c < W; c++) acc[c] = 0.0;
  const T* mine = B + c0;
  for (int base = e0, m = 0; base < e1; base += m) {
    m = min(kChunk, e1 - base);
    __syncthreads();   // (the chunk before is read to its end)
    bool bad = false;
    for (int t = tid; t < m; t += kThreads) {
      const int i = xj[base + t];
      const bool in = (unsigned)i < (unsigned)n_items;
      s_idx[t] = in ? i : -1;
      bad |= !in;
    }
    const int full = __syncthreads_or(bad) ? 0 : m - m % kAhead;   // the entries taken kAhead at a time without a look at them
    if (!live) continue;   // (behind the barriers: every thread of the workgroup reaches them)
    int t0 = 0;
    for (; t0 < full; t0 += kAhead) {
      V v[kAhead];
#pragma unroll
      for (int a = 0; a < kAhead; a++)
        v[a] = *reinterpret_cast<const V*>(mine + (size_t)__builtin_amdgcn_readfirstlane(s_idx[t0 + a]) * ld_B);
#pragma unroll
      for (int a = 0; a < kAhead; a++) add_row(acc, v[a]);
    }
    // the last, shorter group, and a chunk with an index to skip: the same loads in flight (row 0 stands in for an entry that
    // is not there), the adds under a select
    for (; t0 < m; t0 += kAhead) {
      V v[kAhead];
      bool has[kAhead];
#pragma unroll
      for (int a = 0; a < kAhead; a++) {
        const int i = t0 + a < m ? __builtin_amdgcn_readfirstlane(s_idx[t0 + a]) : -1;
        has[a] = i >= 0;
        v[a] = *reinterpret_cast<const V*>(mine + (size_t)max(i, 0) * ld_B);
      }
#pragma unroll
      for (int a = 0; a < kAhead; a++) {
        double was[W];
#pragma unroll
        for (int c = 0; c < W; c++) was[c] = acc[c];
        add_row(acc, v[a]);
#pragma unroll
        for (int c = 0; c < W; c++) acc[c] = has[a] ? acc[c] : was[c];
      }
    }
  }
  if (!live) return;
  u64* d = dense + (size_t)blockIdx.x * ld + c0;
#pragma unroll
  for (int c = 0; c < W; c++)
    if (c0 + c < n_items) d[c] = order_key(acc[c]);
}

}  // namespace

hipError_t launch_ease_item_gram(const int32_t* ip, const int32_t* iu, const int32_t* up, const int32_t* uj, int n_users, int n_items,
                                 int item0, int item1, const int32_t* h_ip, double lambda, int64_t rows, unsigned* ws, double* out,
                                 size_t ld_out, hipStream_t s) {
  for (int64_t r0 = item0; r0 < item1; r0 += rows) {
    const int r1 = (int)std::min<int64_t>(r0 + rows, item1);
    const unsigned t0 = (unsigned)h_ip[r0 - item0], t1 = (unsigned)h_ip[r1 - item0];
    if (t1 > t0) launch_knn_fit_scatter(ip, iu, up, uj, n_users, n_items, (int)r0, r1, t0, t1, ws, s);
    hipLaunchKernelGGL(ease_gram_rows_kernel, dim3((unsigned)((n_items + kThreads - 1) / kThreads), (unsigned)(r1 - r0)), dim3(kThreads),
                       0, s, ws, n_items, (int)r0, ip, lambda, out + (size_t)(r0 - item0) * ld_out, ld_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (t1 > t0 && (e = launch_knn_zero_rows(ws, (size_t)(r1 - r0) * n_items * sizeof(unsigned), s)) != hipSuccess) return e;
  }
  return hipSuccess;
}

template <class T>
hipError_t launch_ease_recommend(const int32_t* xp, const int32_t* xj, int n_rows, int n_items, const T* B, size_t ld_B,
                                 const int32_t* nr_p, const int32_t* nr_j, const int32_t* excl, int n_excl, int k, int64_t rows,
                                 unsigned long long* ws, int32_t* items, long long* scores, hipStream_t s) {
  constexpr int tile = kThreads * Vec<T>::n;
  const size_t ld = (size_t)n_items;
  const unsigned tiles = (unsigned)((n_items + tile - 1) / tile);
  for (int64_t r0 = 0; r0 < n_rows; r0 += rows) {
    const int n_batch = (int)(std::min<int64_t>(r0 + rows, n_rows) - r0);
    if (tiles)   // (no item: nothing to score, every list is padding)
      hipLaunchKernelGGL(ease_score_kernel<T>, dim3((unsigned)n_batch, tiles), dim3(kThreads), 0, s, xp + r0, xj, n_items, B, ld_B, ws, ld);
    if (nr_p || n_excl > 0) launch_knn_mask_rows(ws, ld, n_items, n_batch, nr_p ? nr_p + r0 : nullptr, nr_j, excl, n_excl, s);
    launch_knn_select_lists(ws, ld, n_items, n_batch, k, items + (size_t)r0 * k, scores + (size_t)r0 * k, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (tiles && (e = launch_knn_zero_rows(ws, (size_t)n_batch * ld * sizeof(unsigned long long), s)) != hipSuccess) return e;
  }
  return hipSuccess;
}

template hipError_t launch_ease_recommend<float>(const int32_t*, const int32_t*, int, int, const float*, size_t, const int32_t*,
                                                 const int32_t*, const int32_t*, int, int, int64_t, unsigned long long*, int32_t*,
                                                 long long*, hipStream_t);
template hipError_t launch_ease_recommend<double>(const int32_t*, const int32_t*, int, int, const double*, size_t, const int32_t*,
                                                  const int32_t*, const int32_t*, int, int, int64_t, unsigned long long*, int32_t*,
                                                  long long*, hipStream_t);

}  // namespace rsparse_hip
