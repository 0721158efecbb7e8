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
//
// Evaluation: three more consumers of a batch's dense uint64 rows, behind the same scatter and mask launches.
//   * knn_gather_kernel (score_pairs; no mask): parallel over the stored positions of a second pattern, cut into spans and
//     searched for their rows like the scatter's; out[t] = the cell of (row, j[t]), 0 for a column outside the items.
//   * knn_cand_select_kernel (top_candidates): one workgroup per row reads the row's cells at its candidate slots only, drops
//     the masked ones, and sorts up to RSPARSE_HIP_KNN_LDS_CAND (score, item) pairs in LDS: work follows the candidates, not
//     n_items.  A longer candidate row is restricted in place instead -- every candidate cell gets a mark bit no score reaches,
//     then one pass over the row clears the marks and masks the cells without one -- and the host runs knn_select_kernel on
//     such rows: exact up to the whole catalogue, whatever the order of the candidates.
//   * knn_ranks_kernel (held_out_ranks): one workgroup per masked row, the counting of wrmf_ranks.hip on 64-bit scores: the
//     row's held-out scores RSPARSE_HIP_RANKS_BATCH at a time, sorted in LDS; every unmasked cell finds its place among them
//     by a lower bound and bumps an LDS integer bin; a suffix sum turns the bins into `above`.
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

// ---- evaluation: consumers of a batch's dense rows of scores ------------------------------------------------------------------
// (Templates without a use for their parameter: hipcc emits a template behind every plain kernel of the file and in the order of
// first use, so these three come behind the kernels above, whose listings -- the labels of a listing carry the number of their
// function -- stay byte for byte what they were; profiles/device_helpers/compare_listings.py shows it.)

// the cells at the stored positions [t0, t1) of the pattern (PP, PJ) over the same rows: a wave takes kSpan consecutive
// positions, one per lane.  out parallels PJ (absolute slots).
template <int>
__global__ __launch_bounds__(kThreads) void knn_gather_kernel(const int32_t* __restrict__ PP, const int32_t* __restrict__ PJ,
                                                              int n_outer, int row0, int n_batch, unsigned t0, unsigned t1,
                                                              const u64* __restrict__ dense, size_t ld, int n_items,
                                                              long long* __restrict__ out) {
  static_assert(kSpan == 64, "one position per lane");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long b0l = (long long)t0 + ((long long)blockIdx.x * kWaves + w) * kSpan;
  if (b0l >= (long long)t1) return;   // (whole waves)
  int row = wave_find_row(PP, n_outer, (unsigned)b0l, lane);
  const long long tl = b0l + lane;
  if (tl >= (long long)t1) return;
  const unsigned t = (unsigned)tl;
  row = find_row_from(PP, n_outer, t, row);
  const int j = PJ[t];
  u64 v = 0;
  if ((unsigned)j < (unsigned)n_items && (unsigned)(row - row0) < (unsigned)n_batch) v = dense[(size_t)(row - row0) * ld + j];
  out[t] = (long long)v;
}

// the m entries of s_key / s_idx (m <= kCand) sorted by (key descending, index ascending): the select's bitonic network
__device__ __forceinline__ void sort_entries(u64* s_key, int* s_idx, int m) {
  const int tid = threadIdx.x;
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
}

constexpr u64 kMark = 1ull << 62;   // on a candidate's cell while a long row is restricted (a score is below 2^61)

// cp: the slots of this batch's rows (absolute positions into cj).  A row of at most kCand candidates gets its list here; a
// longer one is restricted to its candidates in place and left to knn_select_kernel.
template <int>
__global__ __launch_bounds__(kThreads) void knn_cand_select_kernel(u64* __restrict__ dense, size_t ld, int n_items,
                                                                   const int32_t* __restrict__ cp, const int32_t* __restrict__ cj,
                                                                   int k, int32_t* __restrict__ out_items,
                                                                   long long* __restrict__ out_scores) {
  __shared__ u64 s_key[kCand];
  __shared__ int s_idx[kCand];
  __shared__ int s_cnt;
  const int tid = threadIdx.x;
  u64* row = dense + (size_t)blockIdx.x * ld;
  const int c0 = cp[blockIdx.x], c1 = cp[blockIdx.x + 1];
  if (c1 - c0 > kCand) {   // (uniform over the workgroup)
    for (int e = c0 + tid; e < c1; e += kThreads) {
      const int j = cj[e];
      if ((unsigned)j < (unsigned)n_items && row[j] != kMasked) row[j] |= kMark;   // (a repeated column stores the same value)
    }
    __syncthreads();   // the marks of this workgroup's own stores are visible to it behind the barrier
    for (int j = tid; j < n_items; j += kThreads) {
      const u64 v = row[j];
      if (v != kMasked) row[j] = (v & kMark) ? (v & ~kMark) : kMasked;
    }
    return;
  }
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  for (int e = c0 + tid; e < c1; e += kThreads) {
    const int j = cj[e];
    if ((unsigned)j >= (unsigned)n_items) continue;
    const u64 v = row[j];
    if (v == kMasked) continue;
    const int slot = atomicAdd(&s_cnt, 1);   // (at most c1 - c0 <= kCand of them)
    s_key[slot] = v;
    s_idx[slot] = j;
  }
  __syncthreads();
  const int m = s_cnt;
  sort_entries(s_key, s_idx, m);   // (a score of 0 sorts behind the scored ones and, by its item, in front of the padding)
  const int have = min(m, k);
  const size_t o = (size_t)blockIdx.x * k;
  for (int t = tid; t < k; t += kThreads) {
    out_items[o + t] = t < have ? s_idx[t] + 1 : INT_MIN;
    out_scores[o + t] = t < have ? (long long)s_key[t] : 0;
  }
}

constexpr int kRankT = RSPARSE_HIP_RANKS_BATCH;   // held-out scores per pass over the row
static_assert(kRankT == 4 * kThreads, "knn_ranks_kernel: a thread owns four bins of the suffix sum");

// first position in t[0, hi) (ascending) whose value is >= k
__device__ __forceinline__ int lower_bound64(const u64* t, int hi, u64 k) {
  int lo = 0;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the score of the held-out item `it` in the masked row, kMasked for an inadmissible one (masked, or outside the items)
__device__ __forceinline__ u64 held_score(const u64* row, int n_items, int it) {
  return (unsigned)it < (unsigned)n_items ? row[it] : kMasked;
}

// ap: the slots of this batch's rows (absolute positions into aj / above / tied); n_adm: of this batch's rows
template <int>
__global__ __launch_bounds__(kThreads) void knn_ranks_kernel(const u64* __restrict__ dense, size_t ld, int n_items,
                                                             const int32_t* __restrict__ ap, const int32_t* __restrict__ aj,
                                                             int32_t* __restrict__ above, int32_t* __restrict__ tied,
                                                             int32_t* __restrict__ n_adm) {
  __shared__ u64 s_own[kRankT];   // the batch's scores in the order of the entries
  __shared__ u64 s_thr[kRankT];   // ... sorted ascending: the admissible ones, then kMasked (inadmissible entries, padding)
  __shared__ int s_gt[kRankT];    // bin b: cells above exactly the thresholds 0..b; after the suffix sum: cells above threshold b
  __shared__ int s_eq[kRankT];    // bin b: cells equal to the run of thresholds that starts at b
  __shared__ int s_w[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const u64* row = dense + (size_t)blockIdx.x * ld;
  const int p1 = ap[blockIdx.x], n_held = max(ap[blockIdx.x + 1] - p1, 0);
  for (int b0 = 0; b0 == 0 || b0 < n_held; b0 += kRankT) {
    const int nb = min(kRankT, n_held - b0);
    int P = 1;
    while (P < nb) P <<= 1;
    for (int e = tid; e < P; e += kThreads) {
      const u64 key = e < nb ? held_score(row, n_items, aj[p1 + b0 + e]) : kMasked;
      s_own[e] = key;
      s_thr[e] = key;
      s_gt[e] = 0;
      s_eq[e] = 0;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int i = tid; i < P / 2; i += kThreads) {
          const int a = 2 * i - (i & (stride - 1)), b = a + stride;
          const u64 ka = s_thr[a], kb = s_thr[b];
          if (((a & size) == 0) == (kb < ka)) {
            s_thr[a] = kb;
            s_thr[b] = ka;
          }
        }
        __syncthreads();
      }
    const int n1 = lower_bound64(s_thr, P, kMasked);   // the admissible thresholds: [0, n1)
    const u64 tmin = n1 > 0 ? s_thr[0] : kMasked;
    // (consecutive cells of one bin -- the zeros of a sparse row, a lone threshold -- cost one atomic)
    int na = 0, gt_bin = -1, gt_cnt = 0, eq_bin = -1, eq_cnt = 0;
    for (int j = tid; j < n_items; j += kThreads) {
      const u64 v = row[j];
      if (v == kMasked) continue;
      na++;
      if (v < tmin) continue;   // (also: no admissible threshold)
      const int pos = lower_bound64(s_thr, n1, v);
      if (pos < n1 && s_thr[pos] == v) {
        if (pos != eq_bin) {
          if (eq_cnt) atomicAdd(&s_eq[eq_bin], eq_cnt);
          eq_bin = pos;
          eq_cnt = 0;
        }
        eq_cnt++;
      }
      if (pos > 0) {
        if (pos - 1 != gt_bin) {
          if (gt_cnt) atomicAdd(&s_gt[gt_bin], gt_cnt);
          gt_bin = pos - 1;
          gt_cnt = 0;
        }
        gt_cnt++;
      }
    }
    if (eq_cnt) atomicAdd(&s_eq[eq_bin], eq_cnt);
    if (gt_cnt) atomicAdd(&s_gt[gt_bin], gt_cnt);
    if (b0 == 0) {
      for (int o = 32; o > 0; o >>= 1) na += __shfl_xor(na, o);
      if (lane == 0) s_w[wv] = na;
      __syncthreads();
      if (tid == 0) {
        int sum = 0;
        for (int q = 0; q < kWaves; q++) sum += s_w[q];
        n_adm[blockIdx.x] = sum;
      }
    }
    __syncthreads();
    // inclusive suffix sum of s_gt[0, P): thread t owns the bins 4t .. 4t + 3
    int v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = 4 * tid + j < P ? s_gt[4 * tid + j] : 0;
    v[2] += v[3];
    v[1] += v[2];
    v[0] += v[1];
    int incl = v[0];   // over the lanes above, then the waves above
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_down(incl, o);
      if (lane + o < 64) incl += t;
    }
    if (lane == 0) s_w[wv] = incl;
    __syncthreads();
    int off = incl - v[0];
    for (int q = wv + 1; q < kWaves; q++) off += s_w[q];
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (4 * tid + j < P) s_gt[4 * tid + j] = v[j] + off;
    __syncthreads();
    for (int e = tid; e < nb; e += kThreads) {
      const u64 key = s_own[e];
      const int pos = key == kMasked ? 0 : lower_bound64(s_thr, n1, key);   // the start of the entry's run of equal scores
      above[p1 + b0 + e] = key == kMasked ? -1 : s_gt[pos];
      tied[p1 + b0 + e] = key == kMasked ? -1 : s_eq[pos] - 1;               // (its own cell is one of the equal ones)
    }
    __syncthreads();   // (the arrays are reused by the next batch)
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

namespace {

// the rows to score and what filters them: the operands every consumer of the lists' dense rows shares
struct KnnRows {
  const int32_t *xp, *xj;
  const uint32_t* xv;
  int n_rows, n_items;
  const int32_t *h_xp, *neighbors;
  const uint32_t* q;
  int K;
  const int32_t *nr_p, *nr_j, *excl;
  int n_excl;
  size_t ld() const { return (size_t)n_items; }
  int batch_end(int64_t r0, int64_t rows) const { return (int)std::min<int64_t>(r0 + rows, n_rows); }
};

// the first launches of a batch of rows [r0, r1): the scatter of the rows' entries and (with_mask) the mask -> whether the rows
// hold anything now
bool fill_list_rows(const KnnRows& in, bool with_mask, int r0, int r1, unsigned long long* ws, hipStream_t s) {
  const unsigned t0 = (unsigned)in.h_xp[r0], t1 = (unsigned)in.h_xp[r1];
  const bool mask = with_mask && (in.nr_p || in.n_excl > 0);
  if (t1 > t0 && in.xv)
    hipLaunchKernelGGL(knn_scatter_kernel<kListsW>, dim3(scatter_grid(t0, t1)), dim3(kThreads), 0, s, in.xp, in.xj, in.n_rows, r0, r1 - r0,
                       t0, t1, nullptr, in.neighbors, in.q, in.K, in.n_items, in.n_items, in.ld(), ws, in.xv);
  else if (t1 > t0)
    hipLaunchKernelGGL(knn_scatter_kernel<kLists>, dim3(scatter_grid(t0, t1)), dim3(kThreads), 0, s, in.xp, in.xj, in.n_rows, r0, r1 - r0,
                       t0, t1, nullptr, in.neighbors, in.q, in.K, in.n_items, in.n_items, in.ld(), ws, nullptr);
  if (mask) launch_knn_mask_rows(ws, in.ld(), in.n_items, r1 - r0, in.nr_p ? in.nr_p + r0 : nullptr, in.nr_j, in.excl, in.n_excl, s);
  return t1 > t0 || mask;
}

// the last step of a batch, behind its consumer: the launches' status, and the rows zeroed again if anything was written to them
hipError_t zero_list_rows(const KnnRows& in, bool written, int r0, int r1, unsigned long long* ws, hipStream_t s) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess || !written) return e;
  return hipMemsetAsync(ws, 0, (size_t)(r1 - r0) * in.ld() * sizeof(unsigned long long), s);
}

}  // namespace

hipError_t launch_knn_recommend(const int32_t* xp, const int32_t* xj, const uint32_t* xv, int n_rows, int n_items, const int32_t* h_xp,
                                const int32_t* neighbors, const uint32_t* q, int K, const int32_t* nr_p, const int32_t* nr_j,
                                const int32_t* excl, int n_excl, int k, int64_t rows, unsigned long long* ws, int32_t* items,
                                long long* scores, hipStream_t s) {
  const KnnRows in{xp, xj, xv, n_rows, n_items, h_xp, neighbors, q, K, nr_p, nr_j, excl, n_excl};
  for (int64_t r0 = 0; r0 < n_rows; r0 += rows) {
    const int r1 = in.batch_end(r0, rows);
    const bool written = fill_list_rows(in, true, (int)r0, r1, ws, s);
    hipLaunchKernelGGL(knn_select_kernel<kLists>, dim3((unsigned)(r1 - r0)), dim3(kThreads), 0, s, ws, in.ld(), n_items, (int)r0, nullptr, 0,
                       k, items + (size_t)r0 * k, nullptr, scores + (size_t)r0 * k, nullptr, nullptr, 0.0);
    if (hipError_t e = zero_list_rows(in, written, (int)r0, r1, ws, s)) return e;
  }
  return hipSuccess;
}

hipError_t launch_knn_score_pairs(const int32_t* xp, const int32_t* xj, const uint32_t* xv, int n_rows, int n_items, const int32_t* h_xp,
                                  const int32_t* neighbors, const uint32_t* q, int K, const int32_t* pp, const int32_t* pj,
                                  const int32_t* h_pp, int64_t rows, unsigned long long* ws, long long* scores, hipStream_t s) {
  const KnnRows in{xp, xj, xv, n_rows, n_items, h_xp, neighbors, q, K, nullptr, nullptr, nullptr, 0};
  for (int64_t r0 = 0; r0 < n_rows; r0 += rows) {
    const int r1 = in.batch_end(r0, rows);
    const bool written = fill_list_rows(in, false, (int)r0, r1, ws, s);
    const unsigned t0 = (unsigned)h_pp[r0], t1 = (unsigned)h_pp[r1];
    if (t1 > t0)
      hipLaunchKernelGGL(knn_gather_kernel<0>, dim3(scatter_grid(t0, t1)), dim3(kThreads), 0, s, pp, pj, n_rows, (int)r0, r1 - (int)r0, t0,
                         t1, ws, in.ld(), n_items, scores);
    if (hipError_t e = zero_list_rows(in, written, (int)r0, r1, ws, s)) return e;
  }
  return hipSuccess;
}

hipError_t launch_knn_top_candidates(const int32_t* xp, const int32_t* xj, const uint32_t* xv, int n_rows, int n_items, const int32_t* h_xp,
                                     const int32_t* neighbors, const uint32_t* q, int K, const int32_t* cp, const int32_t* cj,
                                     const int32_t* h_cp, const int32_t* nr_p, const int32_t* nr_j, const int32_t* excl, int n_excl, int k,
                                     int64_t rows, unsigned long long* ws, int32_t* items, long long* scores, hipStream_t s) {
  const KnnRows in{xp, xj, xv, n_rows, n_items, h_xp, neighbors, q, K, nr_p, nr_j, excl, n_excl};
  auto is_long = [&](int r) { return (int64_t)h_cp[r + 1] - h_cp[r] > kCand; };
  for (int64_t r0 = 0; r0 < n_rows; r0 += rows) {
    const int r1 = in.batch_end(r0, rows);
    bool written = fill_list_rows(in, true, (int)r0, r1, ws, s);
    hipLaunchKernelGGL(knn_cand_select_kernel<0>, dim3((unsigned)(r1 - r0)), dim3(kThreads), 0, s, ws, in.ld(), n_items, cp + r0, cj, k,
                       items + (size_t)r0 * k, scores + (size_t)r0 * k);
    // the rows it restricted instead (more candidates than the LDS buffer holds): the full select, a run of such rows at a time
    for (int a = (int)r0; a < r1; a++) {
      if (!is_long(a)) continue;
      int b = a + 1;
      while (b < r1 && is_long(b)) b++;
      hipLaunchKernelGGL(knn_select_kernel<kLists>, dim3((unsigned)(b - a)), dim3(kThreads), 0, s, ws + (size_t)(a - r0) * in.ld(), in.ld(),
                         n_items, a, nullptr, 0, k, items + (size_t)a * k, nullptr, scores + (size_t)a * k, nullptr, nullptr, 0.0);
      written = true;   // (the cells outside the candidates are masked now)
      a = b;
    }
    if (hipError_t e = zero_list_rows(in, written, (int)r0, r1, ws, s)) return e;
  }
  return hipSuccess;
}

hipError_t launch_knn_held_out_ranks(const int32_t* xp, const int32_t* xj, const uint32_t* xv, int n_rows, int n_items, const int32_t* h_xp,
                                     const int32_t* neighbors, const uint32_t* q, int K, const int32_t* ap, const int32_t* aj,
                                     const int32_t* nr_p, const int32_t* nr_j, const int32_t* excl, int n_excl, int64_t rows,
                                     unsigned long long* ws, int32_t* above, int32_t* tied, int32_t* n_adm, hipStream_t s) {
  const KnnRows in{xp, xj, xv, n_rows, n_items, h_xp, neighbors, q, K, nr_p, nr_j, excl, n_excl};
  for (int64_t r0 = 0; r0 < n_rows; r0 += rows) {
    const int r1 = in.batch_end(r0, rows);
    const bool written = fill_list_rows(in, true, (int)r0, r1, ws, s);
    hipLaunchKernelGGL(knn_ranks_kernel<0>, dim3((unsigned)(r1 - r0)), dim3(kThreads), 0, s, ws, in.ld(), n_items, ap + r0, aj, above, tied,
                       n_adm + r0);
    if (hipError_t e = zero_list_rows(in, written, (int)r0, r1, ws, s)) return e;
  }
  return hipSuccess;
}

// ---- the steps another scorer of dense rows shares (wrmf_ease.hip): host functions only, the kernels above are what they were ----

void launch_knn_fit_scatter(const int32_t* ip, const int32_t* iu, const int32_t* up, const int32_t* uj, int n_users, int n_items, int r0,
                            int r1, unsigned t0, unsigned t1, unsigned* ws, hipStream_t s) {
  hipLaunchKernelGGL(knn_scatter_kernel<kFit>, dim3(scatter_grid(t0, t1)), dim3(kThreads), 0, s, ip, iu, n_items, r0, r1 - r0, t0, t1, up,
                     uj, nullptr, 0, n_users, n_items, (size_t)n_items, ws, nullptr);
}

void launch_knn_mask_rows(unsigned long long* ws, size_t ld, int n_items, int n_batch, const int32_t* nr_p, const int32_t* nr_j,
                          const int32_t* excl, int n_excl, hipStream_t s) {
  hipLaunchKernelGGL(knn_mask_kernel, dim3((unsigned)n_batch), dim3(kThreads), 0, s, ws, ld, n_items, nr_p, nr_j, excl, n_excl);
}

void launch_knn_select_lists(const unsigned long long* ws, size_t ld, int n_items, int n_batch, int k, int32_t* items, long long* scores,
                             hipStream_t s) {
  hipLaunchKernelGGL(knn_select_kernel<kLists>, dim3((unsigned)n_batch), dim3(kThreads), 0, s, ws, ld, n_items, 0, nullptr, 0, k, items,
                     nullptr, scores, nullptr, nullptr, 0.0);
}

hipError_t launch_knn_zero_rows(void* ws, size_t bytes, hipStream_t s) { return hipMemsetAsync(ws, 0, bytes, s); }

void launch_knn_gather_rows(const int32_t* pp, const int32_t* pj, int n_rows, int row0, int n_batch, unsigned t0, unsigned t1,
                            const unsigned long long* ws, size_t ld, int n_items, long long* out, hipStream_t s) {
  hipLaunchKernelGGL(knn_gather_kernel<0>, dim3(scatter_grid(t0, t1)), dim3(kThreads), 0, s, pp, pj, n_rows, row0, n_batch, t0, t1, ws, ld,
                     n_items, out);
}

void launch_knn_ranks_rows(const unsigned long long* ws, size_t ld, int n_items, int n_batch, const int32_t* ap, const int32_t* aj,
                           int32_t* above, int32_t* tied, int32_t* n_adm, hipStream_t s) {
  hipLaunchKernelGGL(knn_ranks_kernel<0>, dim3((unsigned)n_batch), dim3(kThreads), 0, s, ws, ld, n_items, ap, aj, above, tied, n_adm);
}

}  // namespace rsparse_hip
