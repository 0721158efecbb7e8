// Popularity-weighted negative sampling on the device: the rows of wrmf_sample.hip -- for every row of a CSR exclusion pattern, n
// items from outside the row merged with the row's `keep` items -- with the negatives drawn in proportion to integer item weights
// (the "pop100" protocol, count^0.75 sampling).  gfx950, wave64, integers only.
//
// The stream is a FUNCTION of (seed, global row, exclusion list, weights, n), not a state (rsparse_amd/rng.py
// sample_negatives_weighted is the same definition in numpy, include/rsparse_wrmf_hip.h states it for C hosts).  w[0 .. n_item)
// unsigned 32-bit weights >= 1, C[i] = w[0] + ... + w[i] in 64 bits (weights_prefix_*_kernel below), W = C[n_item - 1] < 2^63:
//   draw t    Philox4x32-10, key (lo32(seed), hi32(seed)), counter (lo32(t >> 1), g, 5, hi32(t >> 1)) -> o0..o3;
//             v = o1 2^32 + o0 (t even), o3 2^32 + o2 (t odd);  r = floor(v W / 2^64);  item = #{i : C[i] <= r}
//   chosen    M = n_item - |seen|.  n >= M: every admissible item.  Otherwise A = the first n DISTINCT values among the draws
//             t = 0 .. B(n) - 1 that are not in seen, B(n) = 64 n + 4096; if the budget ends with |A| < n, the row is FILLED
//             with the n - |A| admissible items of lowest item number outside A
//   row       the ascending merge of keep and the chosen items: |keep| + min(n, M) entries -- the lengths of the uniform
//             sampler, so the row pointers are its launch_sample_row_pointers
//
// sample_weighted_kernel<BS>, one team of BS threads per row (BS = 64, one wave, for n <= 64; 256 beyond), LDS: tr[T] items,
// ti[T] first draw indices, T = the power of two at or above 2 (n + 2 BS), at most 16384:
//   1. draw: a thread makes ONE Philox call per round and takes its two draws; a round covers twice the draws that are still
//      missing (at least 64, at most 2 BS: the threads past that sit the round out -- "the first n distinct" does not depend
//      on how the sequence is cut into rounds, and a draw nobody needs is a 20-level search nobody needs).  A draw's item is
//      a binary search over C in global memory (8 bytes per item: the top levels are the same few lines for every thread of
//      the device, the last levels are the scattered ones).  A draw at or past B(n), or whose item is in seen (a binary
//      search over the seen row, global memory), is dropped; its index still counts.  The others go into the open-addressing
//      table (linear probing from a multiplicative hash of the item -- popular items often have ids in an arithmetic
//      progression, which `item & (T - 1)` would pile on one slot): a compare-and-swap claims or finds the slot, an atomic
//      min keeps the SMALLEST draw index of the item -- both order-free.  A draw is a first occurrence iff the slot holds its
//      own index afterwards; the prefix over the draws in index order finds the draw t_cut of the n-th distinct admissible
//      item.  At most n - 1 + 2 BS entries are ever in the table, fewer than its slots.
//   2. compact the entries first drawn up to t_cut into ti[0, a) and sort them ascending (bitonic, LDS): A as items.
//   3. fill, only if a < min(n, M) (the budget ended, or n >= M with a = 0): tr[i] = the RANK of A[i] among the admissible items,
//      A[i] - #{seen < A[i]}, still ascending.  The f-th lowest admissible item outside A has rank f + #{i : tr[i] - i <= f},
//      the complement map of the uniform kernel.  One atomicAdd per filled row on an integer counter (order-free).
//   4. write: A[i] is the (i + min(tr[i] - i, fill))-th chosen item, fill item f the (f + #{i : tr[i] - i <= f})-th; a keep item
//      goes to its own index + the chosen items below it.  Every place lies in [0, |keep| + min(n, M)) whatever the lists hold.
// No float arithmetic, no atomic whose order matters: a call repeats bit for bit and a row does not depend on the rows around it.
#include <algorithm>

#include "wrmf_internal.h"
#include "wrmf_device.h"
#include "wrmf_sample_team.h"

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kWeightedShort = 64;     // n up to this: a wave per row
constexpr int kWeightedMaxTable = 16384;
constexpr unsigned kEmpty = 0xffffffffu;
constexpr unsigned kCutAll = 0xfffffffeu;   // t_cut of a row whose budget ended: every entry of the table is chosen

// ---- the prefix of the weights ----------------------------------------------------------------------------------------------------
// bsum[block] = the sum of the block's 256 weights; *flag != 0: a zero weight
__global__ __launch_bounds__(256) void weights_prefix_sum_kernel(const uint32_t* __restrict__ w, int n_item, long long* __restrict__ bsum,
                                                                 int* __restrict__ flag) {
  __shared__ long long sw[4];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  long long v = 0;
  if (i < n_item) {
    v = (long long)w[i];
    if (v == 0) atomicOr(flag, 1);
  }
  long long tot;
  team_scan<256>(v, sw, &tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// boff[b] = the sum of bsum[0, b) (one workgroup)
__global__ __launch_bounds__(256) void weights_prefix_scan_kernel(const long long* __restrict__ bsum, int nb, long long* __restrict__ boff) {
  __shared__ long long sw[4];
  long long carry = 0;
  for (int c0 = 0; c0 < nb; c0 += 256) {
    const int b = c0 + threadIdx.x;
    const long long v = b < nb ? bsum[b] : 0;
    long long tot;
    const long long off = team_scan<256>(v, sw, &tot);
    if (b < nb) boff[b] = carry + off;
    carry += tot;
  }
}

__global__ __launch_bounds__(256) void weights_prefix_write_kernel(const uint32_t* __restrict__ w, int n_item, const long long* __restrict__ boff,
                                                                   uint64_t* __restrict__ cum) {
  __shared__ long long sw[4];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long v = i < n_item ? (long long)w[i] : 0;
  long long tot;
  const long long off = team_scan<256>(v, sw, &tot);
  if (i < n_item) cum[i] = (uint64_t)(boff[blockIdx.x] + off + v);
}

// ---- the rows ---------------------------------------------------------------------------------------------------------------------
// #{i < n_item : C[i] <= r}, at most n_item - 1 (r < W = C[n_item - 1] for a prefix of weights >= 1)
__device__ __forceinline__ int item_of(const uint64_t* __restrict__ cum, int n_item, u64 r) {
  int lo = 0, hi = n_item - 1;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (cum[mid] <= r) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the items of draw t (a 32-bit draw index: hi32(t >> 1) = 0) and of draw t + 1, t even, of global row g
__device__ __forceinline__ void draw_pair_weighted(unsigned t, unsigned g, unsigned k0, unsigned k1, const uint64_t* __restrict__ cum,
                                                   int n_item, u64 W, int& i0, int& i1) {
  unsigned o[4];
  philox4x32_10(t >> 1, g, 5u, 0u, k0, k1, o);
  i0 = item_of(cum, n_item, __umul64hi(((u64)o[1] << 32) | o[0], W));
  i1 = item_of(cum, n_item, __umul64hi(((u64)o[3] << 32) | o[2], W));
}

// item v, drawn as draw t, into the table -> its slot
__device__ __forceinline__ unsigned table_insert_hashed(unsigned* tr, unsigned* ti, unsigned mask, int shift, unsigned v, unsigned t) {
  unsigned h = (v * 2654435761u) >> shift;
  for (;;) {   // (fewer entries than slots: an empty slot exists)
    const unsigned old = atomicCAS(&tr[h], kEmpty, v);
    if (old == kEmpty || old == v) break;
    h = (h + 1) & mask;
  }
  atomicMin(&ti[h], t);
  return h;
}

template <int BS>
__global__ __launch_bounds__(BS) void sample_weighted_kernel(unsigned k0, unsigned k1, unsigned g0, int n_item, int n,
                                                             const int32_t* __restrict__ seen_p, const int32_t* __restrict__ seen_j,
                                                             const int32_t* __restrict__ keep_p, const int32_t* __restrict__ keep_j,
                                                             const uint64_t* __restrict__ cum, const int32_t* __restrict__ out_p,
                                                             int32_t* __restrict__ out_j, int* __restrict__ filled_rows, int T, int shift) {
  extern __shared__ __attribute__((aligned(16))) unsigned smem_weighted[];
  unsigned* tr = smem_weighted;
  unsigned* ti = smem_weighted + T;
  int* sw = reinterpret_cast<int*>(ti + T);   // [4] team_scan, [4] t_cut
  const int tid = threadIdx.x;
  const int row = blockIdx.x;
  const int s0 = seen_p[row], S = seen_p[row + 1] - s0;
  const int kb = keep_p ? keep_p[row] : 0, K = keep_p ? keep_p[row + 1] - kb : 0;
  const int32_t* seen = seen_j + s0;
  const int32_t* keep = keep_j + kb;   // (not read when K == 0)
  const int M = max(n_item - S, 0);
  const int cnt = min(n, M);
  int a = 0;   // |A|: the chosen items that were drawn
  if (n < M) {
    // 1. the first n distinct admissible items of the draw sequence, within the budget
    const unsigned mask = (unsigned)T - 1u;
    for (int e = tid; e < T; e += BS) {
      tr[e] = kEmpty;
      ti[e] = kEmpty;
    }
    __syncthreads();
    const unsigned g = g0 + (unsigned)row;
    const u64 W = cum[n_item - 1];   // (n_item > M > n >= 1)
    const unsigned budget = 64u * (unsigned)n + 4096u;
    int have = 0;
    unsigned t_cut = kCutAll;
    for (unsigned base = 0; base < budget;) {
      // the round's draws [base, base + span): twice what is still missing, at least a wave's worth, at most two per thread
      const unsigned span = min(2u * BS, max(2u * (unsigned)(n - have), 64u));   // (even)
      const unsigned t0 = base + 2u * (unsigned)tid;
      const bool act = 2u * (unsigned)tid < span;
      bool ok0 = false, ok1 = false;
      unsigned h0 = 0, h1 = 0;
      if (act) {
        int i0, i1;
        draw_pair_weighted(t0, g, k0, k1, cum, n_item, W, i0, i1);
        const int p0 = count_less(seen, S, i0), p1 = count_less(seen, S, i1);
        ok0 = t0 < budget && !(p0 < S && seen[p0] == i0);
        ok1 = t0 + 1u < budget && !(p1 < S && seen[p1] == i1);
        if (ok0) h0 = table_insert_hashed(tr, ti, mask, shift, (unsigned)i0, t0);
        if (ok1) h1 = table_insert_hashed(tr, ti, mask, shift, (unsigned)i1, t0 + 1u);
      }
      __syncthreads();
      const int f0 = ok0 && ti[h0] == t0 ? 1 : 0, f1 = ok1 && ti[h1] == t0 + 1u ? 1 : 0;   // first occurrences
      int tot;
      const int off = team_scan<BS>(f0 + f1, sw, &tot);
      if (have + tot >= n) {   // (uniform) the n-th distinct admissible item is drawn in this round
        const int need = n - have;   // its number among the round's new items, from 1
        if (f0 && off + 1 == need) sw[4] = (int)t0;
        if (f1 && off + f0 + 1 == need) sw[4] = (int)(t0 + 1u);
        __syncthreads();
        t_cut = (unsigned)sw[4];
        have = n;
        break;
      }
      have += tot;
      base += span;
    }
    a = have;
    // 2. A = the entries first drawn up to t_cut, compacted into ti[0, a) and sorted
    int dst0 = 0;
    for (int c0 = 0; c0 < T; c0 += BS) {
      const int e = c0 + tid;
      const unsigned v = tr[e];
      const bool kept = v != kEmpty && ti[e] <= t_cut;
      int tot;
      const int off = team_scan<BS>(kept ? 1 : 0, sw, &tot);   // (its barriers put every read of this chunk before the writes)
      if (kept && dst0 + off < a) ti[dst0 + off] = v;          // (dst0 + off <= e; < a by construction)
      dst0 += tot;
    }
    const int P = pow2_at_least(max(a, 1));   // <= T / 2
    for (int e = min(dst0, a) + tid; e < P; e += BS) ti[e] = kEmpty;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int i = tid; i < P / 2; i += BS) {
          const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
          const unsigned x = ti[lo], y = ti[hi];
          if ((x > y) == ((lo & size) == 0)) {
            ti[lo] = y;
            ti[hi] = x;
          }
        }
        __syncthreads();
      }
    if (a < n && tid == 0 && filled_rows) atomicAdd(filled_rows, 1);
  }
  // 3. the ranks of A among the admissible items, where the row is filled from the complement
  const unsigned* A = ti;
  const unsigned* Ar = tr;
  const int fill = cnt - a;   // (uniform over the team)
  if (fill > 0 && a > 0) {
    for (int i = tid; i < a; i += BS) tr[i] = A[i] - (unsigned)count_less(seen, S, (long long)A[i]);
    __syncthreads();
  }
  // 4. the row: drawn items, fill items and keep items, each to its place in the ascending merge
  int32_t* out = out_j + out_p[row];
  for (int i = tid; i < a; i += BS) {
    const int item = (int)A[i];
    const int j = fill > 0 ? i + min(max((int)Ar[i] - i, 0), fill) : i;
    out[j + count_less(keep, K, item)] = item;
  }
  for (int f = tid; f < fill; f += BS) {
    const int c = count_shifted_le(Ar, a, f);
    const int r = f + c;
    const int item = r + count_shifted_le(seen, S, r);
    out[r + count_less(keep, K, item)] = item;
  }
  for (int k = tid; k < K; k += BS) {
    const int kv = keep[k];
    int below;   // the chosen items below kv
    if (fill > 0) {
      const int q = kv - count_less(seen, S, kv);   // the admissible items below kv
      const int lb = count_less(Ar, a, q);
      below = lb + min(max(q - lb, 0), fill);
    } else {
      below = count_less(A, a, kv);
    }
    out[k + min(max(below, 0), cnt)] = kv;
  }
}

int log2_host(int p) {
  int l = 0;
  while ((1 << l) < p) l++;
  return l;
}

}  // namespace

size_t weights_prefix_ws_bytes(int n_item) {
  const size_t nb = ((size_t)std::max(n_item, 0) + 255) / 256;
  return 2 * nb * 8 + 8;
}

hipError_t launch_weights_prefix(const uint32_t* w, int n_item, uint64_t* cum, void* ws, int** d_flag, hipStream_t s) {
  const int nb = (n_item + 255) / 256;
  long long* bsum = static_cast<long long*>(ws);
  long long* boff = bsum + nb;
  int* flag = reinterpret_cast<int*>(boff + nb);
  *d_flag = flag;
  hipError_t err;
  if ((err = hipMemsetAsync(flag, 0, 8, s)) != hipSuccess) return err;
  hipLaunchKernelGGL(weights_prefix_sum_kernel, dim3((unsigned)nb), dim3(256), 0, s, w, n_item, bsum, flag);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  hipLaunchKernelGGL(weights_prefix_scan_kernel, dim3(1), dim3(256), 0, s, bsum, nb, boff);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  hipLaunchKernelGGL(weights_prefix_write_kernel, dim3((unsigned)nb), dim3(256), 0, s, w, n_item, boff, cum);
  return hipGetLastError();
}

template <int BS>
static hipError_t launch_weighted_rows(unsigned k0, unsigned k1, unsigned g0, int n_rows, int n_item, int n, const int32_t* seen_p,
                                       const int32_t* seen_j, const int32_t* keep_p, const int32_t* keep_j, const uint64_t* cum,
                                       const int32_t* out_p, int32_t* out_j, int* filled_rows, hipStream_t s) {
  int T = 2;
  while (T < 2 * (n + 2 * BS)) T <<= 1;
  T = std::min(kWeightedMaxTable, T);
  const size_t lds = (size_t)T * 8 + 8 * sizeof(int);
  hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(sample_weighted_kernel<BS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(sample_weighted_kernel<BS>, dim3((unsigned)n_rows), dim3(BS), lds, s, k0, k1, g0, n_item, n, seen_p, seen_j, keep_p,
                     keep_j, cum, out_p, out_j, filled_rows, T, 32 - log2_host(T));
  return hipGetLastError();
}

hipError_t launch_sample_negatives_weighted(uint64_t seed, int64_t row0, int n_rows, int n_item, int n, const int32_t* seen_p,
                                            const int32_t* seen_j, const int32_t* keep_p, const int32_t* keep_j, const uint64_t* cum,
                                            const int32_t* out_p, int32_t* out_j, int* filled_rows, hipStream_t s) {
  if (n_rows <= 0) return hipSuccess;
  if (n < 1 || n > kSampleMaxNegatives || n_item < 0 || row0 < 0 || row0 + n_rows > (1ll << 32)) return hipErrorInvalidValue;
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), g0 = (unsigned)row0;
  return n <= kWeightedShort
             ? launch_weighted_rows<64>(k0, k1, g0, n_rows, n_item, n, seen_p, seen_j, keep_p, keep_j, cum, out_p, out_j, filled_rows, s)
             : launch_weighted_rows<256>(k0, k1, g0, n_rows, n_item, n, seen_p, seen_j, keep_p, keep_j, cum, out_p, out_j, filled_rows, s);
}

}  // namespace rsparse_hip
