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
//
// Evaluation: the same scores at given cells, within per-row candidates and against held-out items.  A dense
// row costs nnz(row) x n_items cells of B where a row of m pairs or candidates needs nnz(row) x m, so the host routes every row by
// its own m (cell_route): few cells go to ease_cells_kernel -- a lane owns a cell, a wave 64 cells of ONE row, so the history
// index and the row address are scalar and the lane's column the only vector address; kAhead loads in flight; the adds of
// ease_score_kernel for that column, in its order, so both give the same bits -- and, for the lists, to
// ease_cand_select_kernel, which masks and orders the row's (key, item) pairs in LDS.  Many cells go through ease_score_kernel
// as it is, then ItemKNN's gather (score), or its mask, ease_restrict_kernel and its select (lists).  The held-out ranks always
// take the dense row: the scoring kernel, the mask, ItemKNN's rank count.
#include <algorithm>
#include <climits>

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

// ---- evaluation: the scores at given cells, the lists within candidates ---------------------------------------------

constexpr int kWaves = kThreads / 64;
constexpr int kCand = RSPARSE_HIP_KNN_LDS_CAND;
constexpr u64 kMasked = ~0ull;
static_assert((kCand & (kCand - 1)) == 0 && kCand >= RSPARSE_HIP_KNN_MAX_TOPK, "the pair buffer is a power of two (bitonic sort) and holds k");
static_assert(RSPARSE_HIP_EASE_MAX_ITEMS % 32 == 0, "ease_restrict_kernel: one bit per item in LDS words");

// whether a row that is asked for m cells is scored at those cells (the host's rule, which the kernels repeat: a workgroup of a
// launch over all rows leaves the rows of the other route alone)
__host__ __device__ inline bool cell_route(long long m, int n_items) {
  return m <= kCand && m * RSPARSE_HIP_EASE_CELLS_RATIO <= (long long)n_items;
}

// One key per stored position of the pattern (cp, cj) over the rows of x: the key of sum_i double(B[i, cj[t]]) over the row's
// stored items in ascending stored order -- per cell the adds that ease_score_kernel makes for that column.  grid: the rows; a
// workgroup owns a row, its waves stride over the row's groups of 64 cells, a lane owns a cell: the history index and the row
// address B + i ld_B are wave-uniform (scalar loads of xj), the lane's column is the only vector address; kAhead loads of one
// element are in flight before the first add.  LISTS: a column outside the items is the masked cell, otherwise the key of +0.0.
template <class T, bool LISTS>
__global__ __launch_bounds__(kThreads) void ease_cells_kernel(const int32_t* __restrict__ xp, const int32_t* __restrict__ xj,
                                                              int n_items, const T* __restrict__ B, size_t ld_B,
                                                              const int32_t* __restrict__ cp, const int32_t* __restrict__ cj,
                                                              u64* __restrict__ out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c0 = cp[blockIdx.x], c1 = cp[blockIdx.x + 1];
  if (!cell_route((long long)c1 - c0, n_items)) return;   // (uniform over the workgroup)
  const int e0 = xp[blockIdx.x], e1 = xp[blockIdx.x + 1];
  for (int g = c0 + w * 64; g < c1; g += kWaves * 64) {
    const int t = g + lane;
    const int j = t < c1 ? cj[t] : -1;
    const bool in = (unsigned)j < (unsigned)n_items;   // (n_items > 0 where any lane is in: B has a row 0 and a column 0)
    const T* mine = B + (in ? j : 0);
    double acc = 0.0;
    if (__ballot(in)) {
      int e = e0;
      for (; e + kAhead <= e1; e += kAhead) {
        T v[kAhead];
        bool has[kAhead];
#pragma unroll
        for (int a = 0; a < kAhead; a++) {
          const int i = __builtin_amdgcn_readfirstlane(xj[e + a]);
          has[a] = (unsigned)i < (unsigned)n_items;
          v[a] = mine[(size_t)(has[a] ? i : 0) * ld_B];
        }
#pragma unroll
        for (int a = 0; a < kAhead; a++) acc = has[a] ? acc + (double)v[a] : acc;
      }
      // the last, shorter group: the same loads in flight (row 0 stands in for an entry that is not there)
      if (e < e1) {
        T v[kAhead];
        bool has[kAhead];
#pragma unroll
        for (int a = 0; a < kAhead; a++) {
          const int i = e + a < e1 ? __builtin_amdgcn_readfirstlane(xj[e + a]) : -1;
          has[a] = (unsigned)i < (unsigned)n_items;
          v[a] = mine[(size_t)(has[a] ? i : 0) * ld_B];
        }
#pragma unroll
        for (int a = 0; a < kAhead; a++) acc = has[a] ? acc + (double)v[a] : acc;
      }
    }
    if (t < c1) out[t] = in ? order_key(acc) : (LISTS ? kMasked : order_key(0.0));
  }
}

// (key a, item ia) comes before (key b, item ib) in a list
__device__ __forceinline__ bool before(u64 a, int ia, u64 b, int ib) { return a > b || (a == b && ia < ib); }

// first position in t[0, hi) (ascending) whose value is >= j
__device__ __forceinline__ int lower_bound_item(const int* t, int hi, int j) {
  int lo = 0;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t[mid] < j) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The list of a cell-route row from its keys (ease_cells_kernel<T, true>, parallel to cj): one workgroup per row.  The row's
// not_recommend entries and excl are looked up by lower bound among the row's candidate columns -- STRICTLY ASCENDING, the
// entry's precondition -- and a cell that is found becomes masked; the pairs that are left are ordered by (key descending, item
// ascending) with the bitonic network of wrmf_itemknn.hip's select and the first k written, padded as the dense select pads.
// In LDS a masked pair holds the key 0, which no score has and which sorts behind every score.
// cp / nr_p: n_rows + 1 absolute slots.
__global__ __launch_bounds__(kThreads) void ease_cand_select_kernel(const u64* __restrict__ keys, int n_items,
                                                                    const int32_t* __restrict__ cp, const int32_t* __restrict__ cj,
                                                                    const int32_t* __restrict__ nr_p, const int32_t* __restrict__ nr_j,
                                                                    const int32_t* __restrict__ excl, int n_excl, int k,
                                                                    int32_t* __restrict__ out_items, long long* __restrict__ out_scores) {
  __shared__ u64 s_key[kCand];
  __shared__ int s_idx[kCand];
  const int tid = threadIdx.x;
  const int c0 = cp[blockIdx.x], m = cp[blockIdx.x + 1] - c0;
  if (!cell_route(m, n_items)) return;   // (uniform over the workgroup; m <= kCand below)
  int P = 1;
  while (P < m) P <<= 1;
  for (int t = tid; t < P; t += kThreads) {
    const u64 v = t < m ? keys[c0 + t] : kMasked;
    s_key[t] = v == kMasked ? 0 : v;
    s_idx[t] = t < m ? cj[c0 + t] : INT_MAX;
  }
  __syncthreads();
  auto drop = [&](int j) {
    const int pos = lower_bound_item(s_idx, m, j);
    if (pos < m && s_idx[pos] == j) s_key[pos] = 0;   // (several threads may store the same 0)
  };
  if (nr_p) {
    const int e1 = nr_p[blockIdx.x + 1];
    for (int e = nr_p[blockIdx.x] + tid; e < e1; e += kThreads) drop(nr_j[e]);
  }
  for (int e = tid; e < n_excl; e += kThreads) drop(excl[e]);
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (P >> 1); t += kThreads) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const u64 ka = s_key[lo], kb = s_key[hi];
        const int ia = s_idx[lo], ib = s_idx[hi];
        const bool first_half = (lo & size) == 0;
        if (first_half ? before(kb, ib, ka, ia) : before(ka, ia, kb, ib)) {
          s_key[lo] = kb;
          s_idx[lo] = ib;
          s_key[hi] = ka;
          s_idx[hi] = ia;
        }
      }
      __syncthreads();
    }
  }
  const size_t o = (size_t)blockIdx.x * k;
  for (int t = tid; t < k; t += kThreads) {
    const bool have = t < m && s_key[t] != 0;
    out_items[o + t] = have ? s_idx[t] + 1 : INT_MIN;
    out_scores[o + t] = have ? (long long)s_key[t] : 0;
  }
}

// A dense-route row (scored and masked) restricted to its candidates: every unmasked cell whose column is not a candidate of
// the row becomes masked, and the dense select runs behind it.  One workgroup per row of the batch; the candidates set one bit
// per item in LDS (n_items <= RSPARSE_HIP_EASE_MAX_ITEMS: 4 KiB), so nothing is written into a cell but the sentinel and the
// candidates need no order here.  cp: the slots of this batch's rows (absolute positions into cj).
__global__ __launch_bounds__(kThreads) void ease_restrict_kernel(u64* __restrict__ dense, size_t ld, int n_items,
                                                                 const int32_t* __restrict__ cp, const int32_t* __restrict__ cj) {
  __shared__ unsigned s_bits[RSPARSE_HIP_EASE_MAX_ITEMS / 32];
  const int tid = threadIdx.x;
  const int words = (n_items + 31) / 32;
  for (int t = tid; t < words; t += kThreads) s_bits[t] = 0;
  __syncthreads();
  const int c1 = cp[blockIdx.x + 1];
  for (int e = cp[blockIdx.x] + tid; e < c1; e += kThreads) {
    const int j = cj[e];
    if ((unsigned)j < (unsigned)n_items) atomicOr(&s_bits[j >> 5], 1u << (j & 31));
  }
  __syncthreads();
  u64* row = dense + (size_t)blockIdx.x * ld;
  for (int j = tid; j < n_items; j += kThreads)
    if (!((s_bits[j >> 5] >> (j & 31)) & 1u)) row[j] = kMasked;
}

// the cells of a gathered span that lay outside the items (knn_gather_kernel gives them 0, which no score's key is): the key of +0.0
__global__ __launch_bounds__(kThreads) void ease_outside_cells_kernel(u64* __restrict__ out, unsigned t0, unsigned t1) {
  const long long t = (long long)t0 + (long long)blockIdx.x * kThreads + threadIdx.x;
  if (t < (long long)t1 && out[t] == 0) out[t] = 1ull << 63;
}

// the maximal runs [a, b) of rows of [0, n_rows) for which `dense(r)` holds, at most `rows` of them at a time
template <class IsDense, class Fn>
hipError_t for_dense_batches(int n_rows, int64_t rows, IsDense dense, Fn fn) {
  for (int a = 0; a < n_rows;) {
    if (!dense(a)) {
      a++;
      continue;
    }
    int b = a + 1;
    while (b < n_rows && b - a < rows && dense(b)) b++;
    if (hipError_t e = fn(a, b)) return e;
    a = b;
  }
  return hipSuccess;
}

template <class T>
void launch_score_rows(const int32_t* xp, const int32_t* xj, int n_items, const T* B, size_t ld_B, int a, int b, unsigned long long* ws,
                       hipStream_t s) {
  constexpr int tile = kThreads * Vec<T>::n;
  hipLaunchKernelGGL(ease_score_kernel<T>, dim3((unsigned)(b - a), (unsigned)((n_items + tile - 1) / tile)), dim3(kThreads), 0, s, xp + a,
                     xj, n_items, B, ld_B, ws, (size_t)n_items);
}

}  // namespace

template <class T>
hipError_t launch_ease_score_pairs(const int32_t* xp, const int32_t* xj, int n_rows, int n_items, const T* B, size_t ld_B,
                                   const int32_t* pp, const int32_t* pj, const int32_t* h_pp, int64_t rows, unsigned long long* ws,
                                   unsigned long long* scores, hipStream_t s) {
  auto dense = [&](int r) { return !cell_route((long long)h_pp[r + 1] - h_pp[r], n_items); };
  bool any_cell = false;
  for (int r = 0; r < n_rows && !any_cell; r++) any_cell = h_pp[r + 1] > h_pp[r] && !dense(r);
  if (any_cell) hipLaunchKernelGGL((ease_cells_kernel<T, false>), dim3((unsigned)n_rows), dim3(kThreads), 0, s, xp, xj, n_items, B, ld_B, pp, pj, scores);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // (a dense-route row has more than n_items / ratio >= 0 pairs, so it is never empty; n_items == 0 makes its cells all `outside`)
  return for_dense_batches(n_rows, rows, dense, [&](int a, int b) -> hipError_t {
    const unsigned t0 = (unsigned)h_pp[a], t1 = (unsigned)h_pp[b];
    if (n_items > 0) launch_score_rows(xp, xj, n_items, B, ld_B, a, b, ws, s);
    launch_knn_gather_rows(pp, pj, n_rows, a, b - a, t0, t1, ws, (size_t)n_items, n_items, reinterpret_cast<long long*>(scores), s);
    hipLaunchKernelGGL(ease_outside_cells_kernel, dim3((t1 - t0 + kThreads - 1) / kThreads), dim3(kThreads), 0, s, scores, t0, t1);
    hipError_t e2 = hipGetLastError();
    if (e2 != hipSuccess || n_items == 0) return e2;
    return launch_knn_zero_rows(ws, (size_t)(b - a) * n_items * sizeof(unsigned long long), s);
  });
}

template <class T>
hipError_t launch_ease_top_candidates(const int32_t* xp, const int32_t* xj, int n_rows, int n_items, const T* B, size_t ld_B,
                                      const int32_t* cp, const int32_t* cj, const int32_t* h_cp, const int32_t* nr_p, const int32_t* nr_j,
                                      const int32_t* excl, int n_excl, int k, int64_t rows, unsigned long long* ws,
                                      unsigned long long* keys, int32_t* items, long long* scores, hipStream_t s) {
  auto dense = [&](int r) { return !cell_route((long long)h_cp[r + 1] - h_cp[r], n_items); };
  bool any_cell = false;
  for (int r = 0; r < n_rows && !any_cell; r++) any_cell = !dense(r);
  if (any_cell) {   // (an empty candidate row is a cell-route row: its list is all padding)
    hipLaunchKernelGGL((ease_cells_kernel<T, true>), dim3((unsigned)n_rows), dim3(kThreads), 0, s, xp, xj, n_items, B, ld_B, cp, cj, keys);
    hipLaunchKernelGGL(ease_cand_select_kernel, dim3((unsigned)n_rows), dim3(kThreads), 0, s, keys, n_items, cp, cj, nr_p, nr_j, excl, n_excl,
                       k, items, scores);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t ld = (size_t)n_items;
  // (a dense-route row has candidates, so n_items > 0 unless they all lie outside the items: then the select pads the whole list)
  return for_dense_batches(n_rows, rows, dense, [&](int a, int b) -> hipError_t {
    if (n_items > 0) {
      launch_score_rows(xp, xj, n_items, B, ld_B, a, b, ws, s);
      if (nr_p || n_excl > 0) launch_knn_mask_rows(ws, ld, n_items, b - a, nr_p ? nr_p + a : nullptr, nr_j, excl, n_excl, s);
      hipLaunchKernelGGL(ease_restrict_kernel, dim3((unsigned)(b - a)), dim3(kThreads), 0, s, ws, ld, n_items, cp + a, cj);
    }
    launch_knn_select_lists(ws, ld, n_items, b - a, k, items + (size_t)a * k, scores + (size_t)a * k, s);
    hipError_t e2 = hipGetLastError();
    if (e2 != hipSuccess || n_items == 0) return e2;
    return launch_knn_zero_rows(ws, (size_t)(b - a) * ld * sizeof(unsigned long long), s);
  });
}

template <class T>
hipError_t launch_ease_held_out_ranks(const int32_t* xp, const int32_t* xj, int n_rows, int n_items, const T* B, size_t ld_B,
                                      const int32_t* ap, const int32_t* aj, const int32_t* nr_p, const int32_t* nr_j, const int32_t* excl,
                                      int n_excl, int64_t rows, unsigned long long* ws, int32_t* above, int32_t* tied, int32_t* n_adm,
                                      hipStream_t s) {
  const size_t ld = (size_t)n_items;
  for (int64_t r0 = 0; r0 < n_rows; r0 += rows) {
    const int a = (int)r0, b = (int)std::min<int64_t>(r0 + rows, n_rows);
    if (n_items > 0) {
      launch_score_rows(xp, xj, n_items, B, ld_B, a, b, ws, s);
      if (nr_p || n_excl > 0) launch_knn_mask_rows(ws, ld, n_items, b - a, nr_p ? nr_p + a : nullptr, nr_j, excl, n_excl, s);
    }
    launch_knn_ranks_rows(ws, ld, n_items, b - a, ap + a, aj, above, tied, n_adm + a, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (n_items > 0 && (e = launch_knn_zero_rows(ws, (size_t)(b - a) * ld * sizeof(unsigned long long), s)) != hipSuccess) return e;
  }
  return hipSuccess;
}

#define RSPARSE_EASE_EVAL_INSTANCES(T)                                                                                                    \
  template hipError_t launch_ease_score_pairs<T>(const int32_t*, const int32_t*, int, int, const T*, size_t, const int32_t*,             \
                                                 const int32_t*, const int32_t*, int64_t, unsigned long long*, unsigned long long*,      \
                                                 hipStream_t);                                                                           \
  template hipError_t launch_ease_top_candidates<T>(const int32_t*, const int32_t*, int, int, const T*, size_t, const int32_t*,          \
                                                    const int32_t*, const int32_t*, const int32_t*, const int32_t*, const int32_t*, int, \
                                                    int, int64_t, unsigned long long*, unsigned long long*, int32_t*, long long*,        \
                                                    hipStream_t);                                                                        \
  template hipError_t launch_ease_held_out_ranks<T>(const int32_t*, const int32_t*, int, int, const T*, size_t, const int32_t*,          \
                                                    const int32_t*, const int32_t*, const int32_t*, const int32_t*, int, int64_t,        \
                                                    unsigned long long*, int32_t*, int32_t*, int32_t*, hipStream_t);
RSPARSE_EASE_EVAL_INSTANCES(float)
RSPARSE_EASE_EVAL_INSTANCES(double)
#undef RSPARSE_EASE_EVAL_INSTANCES


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
