// ItemKNN (rsparse_amd/itemknn.py is the definition): the co-occurrence neighbour table of a binary users x items matrix, the
// same table on integer-weighted values (c_ij = sum_u l_ui r_uj), and the top-k lists of users scored by either.  gfx950,
// wave64.  All are ONE operation: an integer product of two sparse operands accumulated into a batch of DENSE rows of a
// workspace, then an exact select per row.  Everything the device computes is an integer, one IEEE division of two exact doubles
// or (weighted fit) the stated product, sum and division in double, so the result equals the numpy definition bit for bit and
// the atomics below (integer, vector, on global memory; no floating-point atomic anywhere) leave the same bits whatever their order.
//
// Launch 1, knn_scatter_kernel: parallel over the STORED ENTRIES of the outer operand for a batch of its rows [row0, row1):
//   * wave `v` of the launch owns the span of RSPARSE_HIP_KNN_SPAN consecutive entries [t0 + v span, ...), whatever the row
//     lengths: a column of 1e6 users is 1e6 / span waves.  It finds the row of its first entry by the wave-wide search of
//     wrmf_csr_rows.h, a lane group the rows of its own entries by stepping on from there;
//   * a lane group of 16 takes an outer entry and walks the INNER list of its column, one atomicAdd per inner element into
//     dense[(row - row0) ld + j].
//     fit:          outer = item -> its users, inner = the CSR row of the user, addend 1, rows of uint32 (the diagonal is left out);
//     weighted fit: the same walk; the outer entry brings its l, the addend is (u64)l * r[e], rows of uint64;
//     predict:      outer = the CSR row of the user, inner = the (neighbors, q) row of the item (-1 slots skipped), rows of
//                   uint64; with a value array the addend is (u64)xq * q.
//   An index outside its range is skipped (the host-array forms refuse it before the upload).
// Launch 2 (predict), knn_mask_kernel: the cells of the row's not_recommend entries and of items_exclude get the all-ones
//   sentinel, which no sum reaches (a score is below 2^61).
// Launch 3, knn_select_kernel: one workgroup per dense row.
//   * the key of a cell: fit, the bits of the double c / 1, c^2 / (n_i n_j) or c / (n_i + n_j - c) (positive, so they order
//     as integers), 0 for an empty cell; weighted fit, the bits of double(c) / (a_i b_j + h): three roundings, the product, the
//     sum, the division (c < 2^53 converts exactly; a, b in [2^-200, 2^200] and h in [0, 2^400] keep the key a positive normal
//     double); predict, the score itself, 0 for a masked cell and for a score of 0;
//   * the cells with a key are compacted into an LDS buffer of RSPARSE_HIP_KNN_LDS_CAND candidates (fit rows are mostly
//     zeros) and sorted there by (key descending, index ascending) with a bitonic network;
//   * more candidates than the buffer holds: a radix select over the dense row, most significant byte first, narrows down the
//     k-th largest key T.  As soon as the keys above the resolved bytes' range and the keys that share them fit the buffer
//     together, one pass collects them and the sort finishes the job; if all eight bytes are resolved and more cells of key T
//     remain than fit (a row of ties), one pass collects the keys above T and, in index order, as many cells of key T as are
//     still missing, and those k are sorted;
//   * predict ranks items of score 0 too: a row with fewer than k scored cells is filled with its first unmasked zero
//     cells in ascending order.
// The rows of a batch are zeroed again by a hipMemsetAsync behind the select (not by the select: the fallback reads the row
// several times), so the workspace is all zeros between calls.
#include <algorithm>
#include <climits>

#include "../../include/rsparse_wrmf_hip.h"
#include "wrmf_csr_rows.h"
#include "wrmf_internal.h"
#include "wrmf_wave.h"

// the weighted key is the definition's three roundings, double(c) / (a_i * b_j + h): no contraction into a fused multiply-add
#pragma clang fp contract(off)

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kThreads = 256;   // 4 waves
constexpr int kWaves = kThreads / 64;
constexpr int kGroup = 16, kGroups = 64 / kGroup;   // lanes that walk one inner list; outer entries a wave has in hand
constexpr int kSpan = RSPARSE_HIP_KNN_SPAN;
constexpr int kCand = RSPARSE_HIP_KNN_LDS_CAND;
constexpr u64 kMasked = ~0ull;
// the forms of the two kernels: the lists, the binary fit, the weighted fit, the lists of weighted rows (scatter only)
enum : int { kLists = 0, kFit = 1, kFitW = 2, kListsW = 3 };
static_assert(kSpan % kGroups == 0, "a wave's span is shared out evenly between its lane groups");
static_assert((kCand & (kCand - 1)) == 0 && kCand >= RSPARSE_HIP_KNN_MAX_TOPK && kCand >= RSPARSE_HIP_KNN_MAX_NEIGHBORS,
              "the candidate buffer is a power of two (bitonic sort) and holds the k entries of the fallback");

// OV: the outer entries' values (kFitW: l, kListsW: xq); Q: the inner elements' (kFitW: r by stored position, lists: q by slot)
template <int MODE>
__global__ __launch_bounds__(kThreads) void knn_scatter_kernel(const int32_t* __restrict__ OP, const int32_t* __restrict__ OJ,
                                                               int n_outer, int row0, int n_batch, unsigned t0, unsigned t1,
                                                               const int32_t* __restrict__ IP, const int32_t* __restrict__ IJ,
                                                               const uint32_t* __restrict__ Q, int K, int n_inner, int n_items,
                                                               size_t ld, void* __restrict__ dense,
                                                               const uint32_t* __restrict__ OV) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long b0l = (long long)t0 + ((long long)blockIdx.x * kWaves + w) * kSpan;
  if (b0l >= (long long)t1) return;   // (whole waves; nothing below synchronises across waves)
  const unsigned b0 = (unsigned)b0l, b1 = (unsigned)min(b0l + kSpan, (long long)t1);
  const int g = lane / kGroup, l = lane % kGroup;
  int row = wave_find_row(OP, n_outer, b0, lane);
  for (unsigned t = b0 + g; t < b1; t += kGroups) {
    row = find_row_from(OP, n_outer, t, row);
    const int c = OJ[t];
    // (a row outside the batch: only row pointers that decrease somewhere else in the array can lead the search there)
    if ((unsigned)c >= (unsigned)n_inner || (unsigned)(row - row0) >= (unsigned)n_batch) continue;
    const size_t base = (size_t)(row - row0) * ld;
    if constexpr (MODE == kFit) {
      unsigned* d = static_cast<unsigned*>(dense) + base;
      const int e1 = IP[c + 1];
      for (int e = IP[c] + l; e < e1; e += kGroup) {
        const int j = IJ[e];
        if ((unsigned)j < (unsigned)n_items && j != row) atomicAdd(d + j, 1u);
      }
    } else if constexpr (MODE == kFitW) {
      u64* d = static_cast<u64*>(dense) + base;
      const u64 lv = OV[t];
      const int e1 = IP[c + 1];
      for (int e = IP[c] + l; e < e1; e += kGroup) {
        const int j = IJ[e];
        if ((unsigned)j < (unsigned)n_items && j != row) atomicAdd(d + j, lv * Q[e]);
      }
    } else {
      u64* d = static_cast<u64*>(dense) + base;
      u64 xv = 1;
      if constexpr (MODE == kListsW) xv = OV[t];
      for (int s = l; s < K; s += kGroup) {
        const int j = IJ[(size_t)c * K + s];
        if ((unsigned)j < (unsigned)n_items) atomicAdd(d + j, xv * Q[(size_t)c * K + s]);
      }
    }
  }
}

// nr_p: the slots of this batch's rows (absolute positions into nr_j), or null
__global__ __launch_bounds__(kThreads) void knn_mask_kernel(u64* __restrict__ dense, size_t ld, int n_items,
                                                            const int32_t* __restrict__ nr_p, const int32_t* __restrict__ nr_j,
                                                            const int32_t* __restrict__ excl, int n_excl) {
  u64* d = dense + (size_t)blockIdx.x * ld;
  if (nr_p) {
    const int e1 = nr_p[blockIdx.x + 1];
    for (int e = nr_p[blockIdx.x] + (int)threadIdx.x; e < e1; e += kThreads) {
      const int j = nr_j[e];
      if ((unsigned)j < (unsigned)n_items) d[j] = kMasked;
    }
  }
  for (int e = threadIdx.x; e < n_excl; e += kThreads) {
    const int j = excl[e];
    if ((unsigned)j < (unsigned)n_items) d[j] = kMasked;
  }
}

// (key a, index ia) comes before (key b, index ib) in a list
__device__ __forceinline__ bool before(u64 a, int ia, u64 b, int ib) { return a > b || (a == b && ia < ib); }

// the number of threads of the workgroup in front of this one whose `flag` is set, and the workgroup's count; every thread
// calls it (two barriers), s_w: kWaves ints
__device__ __forceinline__ int block_rank(bool flag, int* s_w, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const u64 b = __ballot(flag);
  if (lane == 0) s_w[w] = __popcll(b);
  __syncthreads();
  int off = 0;
  total = 0;
#pragma unroll
  for (int q = 0; q < kWaves; q++) {
    off += q < w ? s_w[q] : 0;
    total += s_w[q];
  }
  __syncthreads();
  return off + __popcll(b & ((1ull << lane) - 1));
}

// out_scores: the lists' scores, or the weighted fit's sums (as uint64 bits); A, B, h: the weighted key's tables
template <int MODE>
__global__ __launch_bounds__(kThreads) void knn_select_kernel(const void* __restrict__ dense, size_t ld, int n, int row0,
                                                              const int32_t* __restrict__ IP, int sim, int k,
                                                              int32_t* __restrict__ out_items, int32_t* __restrict__ out_counts,
                                                              long long* __restrict__ out_scores, const double* __restrict__ A,
                                                              const double* __restrict__ B, double h) {
  constexpr bool FIT = MODE != kLists;
  __shared__ u64 s_key[kCand];
  __shared__ int s_idx[kCand];
  __shared__ int s_hist[256];
  __shared__ int s_w[kWaves];
  __shared__ int s_cnt, s_digit, s_rem, s_meq;
  const int tid = threadIdx.x;
  const int i = row0 + (int)blockIdx.x;   // fit: the item whose neighbours these are
  const unsigned* row32 = static_cast<const unsigned*>(dense) + (size_t)blockIdx.x * ld;
  const u64* row64 = static_cast<const u64*>(dense) + (size_t)blockIdx.x * ld;
  const long long ni = MODE == kFit ? (long long)IP[i + 1] - IP[i] : 0;
  const double ai = MODE == kFitW ? A[i] : 0.0;   // (read once per workgroup)
  auto cell_key = [&](int j) -> u64 {
    if constexpr (MODE == kFitW) {
      const u64 c = row64[j];
      if (c == 0 || j == i) return 0;
      const double den = ai * B[j] + h;
      return (u64)__double_as_longlong((double)c / den);
    } else if constexpr (FIT) {
      const unsigned c = row32[j];
      if (c == 0 || j == i) return 0;
      const long long nj = (long long)IP[j + 1] - IP[j];
      double key;
      if (sim == RSPARSE_HIP_KNN_COSINE) key = (double)((u64)c * c) / (double)(ni * nj);
      else if (sim == RSPARSE_HIP_KNN_JACCARD) key = (double)c / (double)(ni + nj - (long long)c);
      else key = (double)c;
      return (u64)__double_as_longlong(key);
    } else {
      const u64 v = row64[j];
      return v == kMasked ? 0 : v;
    }
  };
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  for (int j = tid; j < n; j += kThreads) {
    const u64 key = cell_key(j);
    if (key) {
      const int slot = atomicAdd(&s_cnt, 1);
      if (slot < kCand) {
        s_key[slot] = key;
        s_idx[slot] = j;
      }
    }
  }
  __syncthreads();
  int m = s_cnt;   // entries to sort, in s_key / s_idx
  __syncthreads();
  if (m > kCand) {
    // the k-th largest key T (m > kCand >= k of them): most significant byte first
    u64 prefix = 0;
    int rem = k, few = -1;
    for (int shift = 56; shift >= 0; shift -= 8) {
      s_hist[tid] = 0;
      __syncthreads();
      const u64 hi = shift == 56 ? 0 : (~0ull << (shift + 8));
      for (int j = tid; j < n; j += kThreads) {
        const u64 key = cell_key(j);
        if (key && (key & hi) == prefix) atomicAdd(&s_hist[(int)((key >> shift) & 255)], 1);
      }
      __syncthreads();
      if (tid == 0) {
        int cum = 0, b = 255;
        for (; b > 0; b--) {
          if (cum + s_hist[b] >= rem) break;
          cum += s_hist[b];
        }
        s_digit = b;
        s_rem = rem - cum;
        s_meq = s_hist[b];
      }
      __syncthreads();
      prefix |= (u64)s_digit << shift;
      rem = s_rem;
      const int n_at = (k - rem) + s_meq;   // keys above the prefix's range, and keys that share the prefix
      __syncthreads();
      if (n_at <= kCand) {                  // they fit the buffer: no further byte has to be resolved
        few = n_at;
        break;
      }
    }
    const u64 T = prefix;
    const int n_gt = k - rem;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    if (few >= 0) {
      // every key at or above the prefix (its unresolved bytes zero), in any order: the sort below puts the k first
      for (int j = tid; j < n; j += kThreads) {
        const u64 key = cell_key(j);
        if (key && key >= T) {
          const int slot = atomicAdd(&s_cnt, 1);
          if (slot < kCand) {
            s_key[slot] = key;
            s_idx[slot] = j;
          }
        }
      }
      m = few;
    } else {
      // all eight bytes resolved and still more cells of key T than the buffer holds: the k - rem keys above T in any order,
      // and the first `rem` cells of key T in index order
      int eq_seen = 0;
      for (int base = 0; base < n; base += kThreads) {
        const int j = base + tid;
        const u64 key = j < n ? cell_key(j) : 0;
        if (key > T) {
          const int slot = atomicAdd(&s_cnt, 1);
          if (slot < n_gt) {
            s_key[slot] = key;
            s_idx[slot] = j;
          }
        }
        const bool eq = key == T;   // (T > 0: never an empty cell)
        int total;
        const int rank = eq_seen + block_rank(eq, s_w, total);
        if (eq && rank < rem) {
          s_key[n_gt + rank] = key;
          s_idx[n_gt + rank] = j;
        }
        eq_seen += total;
      }
      m = k;
    }
    __syncthreads();
  }
  // sort the m entries: (key descending, index ascending)
  int P = 1;
  while (P < m) P <<= 1;
  for (int t = m + tid; t < P; t += kThreads) {
    s_key[t] = 0;
    s_idx[t] = INT_MAX;
  }
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
  const int have = min(m, k);
  const size_t o = (size_t)blockIdx.x * k;
  for (int t = tid; t < have; t += kThreads) {
    const int j = s_idx[t];
    if constexpr (MODE == kFitW) {
      out_items[o + t] = j;
      out_scores[o + t] = (long long)row64[j];
    } else if constexpr (FIT) {
      out_items[o + t] = j;
      out_counts[o + t] = (int32_t)row32[j];
    } else {
      out_items[o + t] = j + 1;
      out_scores[o + t] = (long long)s_key[t];
    }
  }
  if constexpr (FIT) {
    for (int t = have + tid; t < k; t += kThreads) {
      out_items[o + t] = -1;
      if constexpr (MODE == kFitW) out_scores[o + t] = 0;
      else out_counts[o + t] = 0;
    }
  } else {
    // the unmasked cells of score 0, ascending, behind the scored ones
    const int need = k - have;
    int filled = 0;
    for (int base = 0; base < n && filled < need; base += kThreads) {
      const int j = base + tid;
      const bool z = j < n && row64[j] == 0;
      int total;
      const int rank = filled + block_rank(z, s_w, total);
      if (z && rank < need) {
        out_items[o + have + rank] = j + 1;
        out_scores[o + have + rank] = 0;
      }
      filled += total;
    }
    for (int t = have + min(filled, need) + tid; t < k; t += kThreads) {
      out_items[o + t] = INT_MIN;
      out_scores[o + t] = 0;
    }
  }
}

unsigned scatter_grid(unsigned t0, unsigned t1) {
  const long long per = (long long)kSpan * kWaves;
  return (unsigned)(((long long)t1 - t0 + per - 1) / per);
}

}  // namespace

hipError_t launch_cooc_neighbors(const int32_t* ip, const int32_t* iu, const int32_t* up, const int32_t* uj, int n_users,
                                 int n_items, int item0, int item1, const int32_t* h_ip, int sim, int K, int64_t rows,
                                 unsigned* ws, int32_t* neighbors, int32_t* counts, hipStream_t s) {
  const size_t ld = (size_t)n_items;
  for (int64_t r0 = item0; r0 < item1; r0 += rows) {
    const int r1 = (int)std::min<int64_t>(r0 + rows, item1);
    const unsigned t0 = (unsigned)h_ip[r0 - item0], t1 = (unsigned)h_ip[r1 - item0];
    if (t1 > t0)
      hipLaunchKernelGGL(knn_scatter_kernel<kFit>, dim3(scatter_grid(t0, t1)), dim3(kThreads), 0, s, ip, iu, n_items, (int)r0,
                         (int)(r1 - r0), t0, t1, up, uj, nullptr, 0, n_users, n_items, ld, ws, nullptr);
    hipLaunchKernelGGL(knn_select_kernel<kFit>, dim3((unsigned)(r1 - r0)), dim3(kThreads), 0, s, ws, ld, n_items, (int)r0, ip, sim, K,
                       neighbors + (size_t)(r0 - item0) * K, counts + (size_t)(r0 - item0) * K, nullptr, nullptr, nullptr, 0.0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (t1 > t0 && (e = hipMemsetAsync(ws, 0, (size_t)(r1 - r0) * ld * sizeof(unsigned), s)) != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_cooc_neighbors_weighted(const int32_t* ip, const int32_t* iu, const uint32_t* il, const int32_t* up, const int32_t* uj,
                                          const uint32_t* ur, int n_users, int n_items, int item0, int item1, const int32_t* h_ip,
                                          const double* a, const double* b, double h, int K, int64_t rows, unsigned long long* ws,
                                          int32_t* neighbors, unsigned long long* sums, hipStream_t s) {
  const size_t ld = (size_t)n_items;
  for (int64_t r0 = item0; r0 < item1; r0 += rows) {
    const int r1 = (int)std::min<int64_t>(r0 + rows, item1);
    const unsigned t0 = (unsigned)h_ip[r0 - item0], t1 = (unsigned)h_ip[r1 - item0];
    if (t1 > t0)
      hipLaunchKernelGGL(knn_scatter_kernel<kFitW>, dim3(scatter_grid(t0, t1)), dim3(kThreads), 0, s, ip, iu, n_items, (int)r0,
                         (int)(r1 - r0), t0, t1, up, uj, ur, 0, n_users, n_items, ld, ws, il);
    hipLaunchKernelGGL(knn_select_kernel<kFitW>, dim3((unsigned)(r1 - r0)), dim3(kThreads), 0, s, ws, ld, n_items, (int)r0, nullptr, 0, K,
                       neighbors + (size_t)(r0 - item0) * K, nullptr, reinterpret_cast<long long*>(sums) + (size_t)(r0 - item0) * K, a, b, h);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (t1 > t0 && (e = hipMemsetAsync(ws, 0, (size_t)(r1 - r0) * ld * sizeof(unsigned long long), s)) != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_knn_recommend(const int32_t* xp, const int32_t* xj, const uint32_t* xv, int n_rows, int n_items, const int32_t* h_xp,
                                const int32_t* neighbors, const uint32_t* q, int K, const int32_t* nr_p, const int32_t* nr_j,
                                const int32_t* excl, int n_excl, int k, int64_t rows, unsigned long long* ws, int32_t* items,
                                long long* scores, hipStream_t s) {
  const size_t ld = (size_t)n_items;
  for (int64_t r0 = 0; r0 < n_rows; r0 += rows) {
    const int r1 = (int)std::min<int64_t>(r0 + rows, n_rows);
    const unsigned t0 = (unsigned)h_xp[r0], t1 = (unsigned)h_xp[r1];
    const bool mask = nr_p || n_excl > 0;
    if (t1 > t0 && xv)
      hipLaunchKernelGGL(knn_scatter_kernel<kListsW>, dim3(scatter_grid(t0, t1)), dim3(kThreads), 0, s, xp, xj, n_rows, (int)r0,
                         (int)(r1 - r0), t0, t1, nullptr, neighbors, q, K, n_items, n_items, ld, ws, xv);
    else if (t1 > t0)
      hipLaunchKernelGGL(knn_scatter_kernel<kLists>, dim3(scatter_grid(t0, t1)), dim3(kThreads), 0, s, xp, xj, n_rows, (int)r0,
                         (int)(r1 - r0), t0, t1, nullptr, neighbors, q, K, n_items, n_items, ld, ws, nullptr);
    if (mask)
      hipLaunchKernelGGL(knn_mask_kernel, dim3((unsigned)(r1 - r0)), dim3(kThreads), 0, s, ws, ld, n_items, nr_p ? nr_p + r0 : nullptr,
                         nr_j, excl, n_excl);
    hipLaunchKernelGGL(knn_select_kernel<kLists>, dim3((unsigned)(r1 - r0)), dim3(kThreads), 0, s, ws, ld, n_items, (int)r0, nullptr, 0, k,
                       items + (size_t)r0 * k, nullptr, scores + (size_t)r0 * k, nullptr, nullptr, 0.0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((t1 > t0 || mask) && (e = hipMemsetAsync(ws, 0, (size_t)(r1 - r0) * ld * sizeof(unsigned long long), s)) != hipSuccess)
      return e;
  }
  return hipSuccess;
}

}  // namespace rsparse_hip
