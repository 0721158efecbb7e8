// BPR (Rendle et al. 2009) by deterministic mini-batch SGD, on the device (gfx950): one step takes its triples from a
// counter-based stream, its scores from a snapshot of the factors, and sums the gradient rows per destination in a fixed order.
// rsparse_amd/bpr.py (bpr_triples, bpr_step_reference) is the definition in numpy, the C header states it for other hosts;
// DESIGN.md 3.34 has the scheme.
//
//   1. sample    a thread per slot k of the step (CSR slot p = step + k n_steps): the row by bisection of the row pointers, one
//                Philox call, the positive, the first of three candidates outside the row (bisection of the row).  Integers only.
//                Writes (u, i, j), j = -1 for a void triple, and the item-side sort keys: key = item, payload = 2k / 2k + 1
//                (positive / negative role); a void triple is keyed n_items, behind every item.
//   2. z         a 16-lane group per triple: lane l owns the coordinates c = l, l + 16, ...; d = <U[u], V[i] - V[j]> in the
//                definition's order (16 partial sums, then xor-shuffles 8, 4, 2, 1: the halving of the definition),
//                z = 1 / (1 + E(d)) with the stated exponential.  The epoch's counts by ballot and integer atomics.
//   3. users     a group per run of equal u (a user's triples are consecutive in k; the group at the run's first k works, the
//                others leave): z_k (V[i] - V[j]) added in k order in double registers, chunk by chunk; the new row and a' go
//                into a staging slot (the user's, or the run's first k: min(n_rows, slots) rows), because step 5 still reads
//                the snapshot of U.
//   4. index     rocprim::radix_sort_pairs on exactly the key bits in use (stable: ascending k, positive before negative, per
//                item); a thread per item bisects the sorted keys for its segment; a scan numbers the chunks of the segments
//                longer than RSPARSE_HIP_BPR_CHUNK.
//   5. items     a group per chunk of a long segment writes the chunk's sum; then a group per item walks a short segment
//                directly or adds a long one's chunk sums in order, and updates V and its `a` in place.  Nothing else reads V
//                in this pass.
//   6. copy      the staged rows go into U.
// update_items = false skips the keys of 1, and 4 and 5.  No float atomics, no host synchronisation between the steps of a
// call, every grid sized by the step's slot count or the item count with early exit, every loop bounded by the data sizes.
// The file is built with contraction off: every product, sum, quotient and root is its own rounded float64 operation.
//
// WARP (rsparse_amd/warp.py is its definition) replaces 1 and 2 by one launch, warp_search_kernel: per slot up to
// max_trials dependent draw-and-score trials that stop at the first candidate inside the margin; 3 - 6 run behind it unchanged.
//
// Item features (the kernels are in wrmf_bpr_features.hip): V is composed from the feature rows H before a step,
// and 5b is replaced by the item totals without the update and a backward pass through F into H.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/rsparse_wrmf_hip.h"
#include "wrmf_internal.h"
#include "wrmf_device.h"
#include "wrmf_bpr_device.h"

#pragma clang fp contract(off)

namespace rsparse_hip {
namespace {

using namespace dev;
using namespace bprdev;

static_assert(kWarpMaxTrials == RSPARSE_HIP_WARP_MAX_TRIALS && kWarpMaxTrials <= kBprThreads, "the weights are staged by one pass of a workgroup");

struct BprStep {
  const int32_t* p;
  const int32_t* j;
  int n_rows, n_items;
  int64_t row0;
  unsigned k0, k1, c3;   // the key and the counter's last word: epoch + 2^31 mode
  int mode, step, n_steps, cnt;
};

__global__ __launch_bounds__(kBprThreads) void bpr_sample_kernel(BprStep a, int32_t* __restrict__ tu, int32_t* __restrict__ ti,
                                                                 int32_t* __restrict__ tj, uint32_t* __restrict__ keys,
                                                                 uint32_t* __restrict__ pay) {
  const int k = blockIdx.x * kBprThreads + threadIdx.x;
  if (k >= a.cnt) return;
  const int64_t p = (int64_t)a.step + (int64_t)k * a.n_steps;
  int lo = 0, hi = a.n_rows;   // p[lo] <= p < p[hi]
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((int64_t)a.p[mid] <= p) lo = mid; else hi = mid;
  }
  const int u = lo, b = a.p[u], L = a.p[u + 1] - b;
  const unsigned g = (unsigned)((u64)a.row0 + (a.mode == 0 ? (u64)u : 0ull));
  unsigned o[4];
  philox4x32_10((unsigned)(p - b), g, 6u, a.c3, a.k0, a.k1, o);
  const int pos = a.j[b + (int)(((u64)o[0] * (u64)(unsigned)L) >> 32)];
  int neg = -1;
#pragma unroll
  for (int t = 1; t < 4; t++) {
    const int cand = (int)(((u64)o[t] * (u64)(unsigned)a.n_items) >> 32);
    int l = 0, h = L;   // the first entry of the row that is >= cand
    while (l < h) {
      const int mid = l + ((h - l) >> 1);
      if (a.j[b + mid] < cand) l = mid + 1; else h = mid;
    }
    const bool inside = l < L && a.j[b + l] == cand;
    if (neg < 0 && !inside) neg = cand;
  }
  tu[k] = u;
  ti[k] = pos;
  tj[k] = neg;
  if (keys) {
    keys[2 * (size_t)k] = neg < 0 ? (uint32_t)a.n_items : (uint32_t)pos;
    keys[2 * (size_t)k + 1] = neg < 0 ? (uint32_t)a.n_items : (uint32_t)neg;
    pay[2 * (size_t)k] = 2u * (uint32_t)k;
    pay[2 * (size_t)k + 1] = 2u * (uint32_t)k + 1u;
  }
}

// E(d) of the definition: plain arithmetic, no library exponential
__device__ __forceinline__ double bpr_exp(double d) {
  d = d < -40.0 ? -40.0 : (d > 40.0 ? 40.0 : d);
  const double kk = rint(d * 1.4426950408889634);
  const double r = (d - kk * 6.93147180369123816490e-01) - kk * 1.90821492927058770002e-10;
  double q = 1.0 / 6227020800.0;
  q = q * r + 1.0 / 479001600.0;
  q = q * r + 1.0 / 39916800.0;
  q = q * r + 1.0 / 3628800.0;
  q = q * r + 1.0 / 362880.0;
  q = q * r + 1.0 / 40320.0;
  q = q * r + 1.0 / 5040.0;
  q = q * r + 1.0 / 720.0;
  q = q * r + 1.0 / 120.0;
  q = q * r + 1.0 / 24.0;
  q = q * r + 1.0 / 6.0;
  q = q * r + 1.0 / 2.0;
  q = q * r + 1.0;
  q = q * r + 1.0;
  return ldexp(q, (int)kk);
}

template <class T>
__global__ __launch_bounds__(kBprThreads) void bpr_z_kernel(const int32_t* __restrict__ tu, const int32_t* __restrict__ ti,
                                                            const int32_t* __restrict__ tj, int cnt, int rank,
                                                            const T* __restrict__ U, const T* __restrict__ V, double* __restrict__ z,
                                                            unsigned long long* __restrict__ counts) {
  const int k = blockIdx.x * kBprGroups + (threadIdx.x >> 4), lane = threadIdx.x & 15;
  bool valid = false, correct = false;
  if (k < cnt) {
    const int jn = tj[k];
    if (jn >= 0) {
      const T* ur = U + (size_t)tu[k] * rank;
      const T* vi = V + (size_t)ti[k] * rank;
      const T* vj = V + (size_t)jn * rank;
      double part = 0.0;
#pragma unroll 4
      for (int c = lane; c < rank; c += kBprLanes) {
        const double diff = (double)vi[c] - (double)vj[c];
        part = part + (double)ur[c] * diff;
      }
      const double d = bpr_reduce16(part);
      if (lane == 0) {
        z[k] = 1.0 / (1.0 + bpr_exp(d));
        valid = true;
        correct = d > 0.0;
      }
    } else if (lane == 0) {
      z[k] = 0.0;
    }
  }
  const u64 bv = __ballot(valid), bc = __ballot(correct);
  if ((threadIdx.x & 63) == 0) {
    if (bv) atomicAdd(counts, (unsigned long long)__popcll(bv));
    if (bc) atomicAdd(counts + 1, (unsigned long long)__popcll(bc));
  }
}

// WARP's search: steps 1 and 2 in one launch.  A 16-lane group owns a slot (four slots per wave) and keeps U[u] and V[i] in
// registers, lane l the coordinates l + 16 q, so that the 16 lanes ARE the 16 partial sums of the definition's dot product.
// Trials are drawn lazily in rounds of 16: in round r lane l draws trial t = 16 r + l + 1 (one Philox call per lane: call t >> 2,
// word t & 3) and bisects the row for membership; the group's 16 bits of the wave's ballot are the admissible trials of the
// round.  The group walks them in ascending t with the row of the NEXT admissible candidate already requested while the current
// one is multiplied and halved, and stops at the first d <= margin.  Every loop is wave-uniform (a group that is done idles with
// an empty mask: the ballots, the shuffles and the barrier need it) and bounded by max_trials and the row length.  The four
// counts are added in LDS per wave and leave as one integer atomic per counter and workgroup.
template <class T, int R16>
__device__ __forceinline__ void warp_row(const T* __restrict__ row, int rank, int lane, T (&out)[R16]) {
#pragma unroll
  for (int q = 0; q < R16; q++) {
    const int c = lane + kBprLanes * q;
    if (c < rank) out[q] = row[c];
  }
}

template <class T, int R16>
__global__ __launch_bounds__(kBprThreads) void warp_search_kernel(BprStep a, WarpSearch w, int rank, const T* __restrict__ U,
                                                                  const T* __restrict__ V, int32_t* __restrict__ tu,
                                                                  int32_t* __restrict__ ti, int32_t* __restrict__ tj,
                                                                  int32_t* __restrict__ tt, double* __restrict__ z,
                                                                  uint32_t* __restrict__ keys, uint32_t* __restrict__ pay,
                                                                  unsigned long long* __restrict__ counts) {
  __shared__ double s_w[kWarpMaxTrials];
  __shared__ unsigned s_cnt[4];
  if (threadIdx.x < kWarpMaxTrials) s_w[threadIdx.x] = (int)threadIdx.x < w.max_trials ? w.weights[threadIdx.x] : 0.0;
  if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  const int k = blockIdx.x * kBprGroups + (threadIdx.x >> 4), lane = threadIdx.x & 15;
  const int shift = threadIdx.x & 48;   // where the group's 16 bits stand in the wave's ballot
  const bool has = k < a.cnt;
  int u = 0, b = 0, L = 0, pos = 0;
  unsigned q0 = 0, g = 0;
  T ur[R16], vi[R16], cur[R16], nxt[R16];
#pragma unroll
  for (int q = 0; q < R16; q++) ur[q] = vi[q] = cur[q] = nxt[q] = (T)0;
  if (has) {
    const int64_t p = (int64_t)a.step + (int64_t)k * a.n_steps;
    int lo = 0, hi = a.n_rows;   // p[lo] <= p < p[hi]
    while (hi - lo > 1) {
      const int mid = lo + ((hi - lo) >> 1);
      if ((int64_t)a.p[mid] <= p) lo = mid; else hi = mid;
    }
    u = lo; b = a.p[u]; L = a.p[u + 1] - b;
    q0 = (unsigned)(p - b);
    g = (unsigned)((u64)a.row0 + (a.mode == 0 ? (u64)u : 0ull));
    unsigned o[4];
    philox4x32_10(q0, g, 7u, a.c3, a.k0, a.k1, o);
    pos = a.j[b + (int)(((u64)o[0] * (u64)(unsigned)L) >> 32)];
    warp_row<T, R16>(U + (size_t)u * rank, rank, lane, ur);
    warp_row<T, R16>(V + (size_t)pos * rank, rank, lane, vi);
  }
  bool done = false, seen = false, correct = false;   // (the same in the 16 lanes of a group)
  int jn = -1, tk = 0;
  double dk = 0.0;
  unsigned scored = 0u;                               // (the same in the 64 lanes of a wave)
  const int n_rounds = (w.max_trials + kBprLanes - 1) / kBprLanes;
  for (int r = 0; r < n_rounds; r++) {
    const bool active = has && !done;
    if (!__any(active)) break;
    const int t = kBprLanes * r + lane + 1;
    int cand = 0;
    bool admissible = false;
    if (active && t <= w.max_trials) {
      unsigned o[4];
      philox4x32_10(q0, g, 7u + 256u * (unsigned)(t >> 2), a.c3, a.k0, a.k1, o);
      const int wi = t & 3;
      const unsigned word = wi == 0 ? o[0] : (wi == 1 ? o[1] : (wi == 2 ? o[2] : o[3]));
      cand = (int)(((u64)word * (u64)(unsigned)a.n_items) >> 32);
      int l = 0, h = L;   // the first entry of the row that is >= cand
      while (l < h) {
        const int mid = l + ((h - l) >> 1);
        if (a.j[b + mid] < cand) l = mid + 1; else h = mid;
      }
      admissible = !(l < L && a.j[b + l] == cand);
    }
    unsigned mask = (unsigned)(__ballot(admissible) >> shift) & 0xffffu;
    bool live = mask != 0u;
    int lcur = live ? __ffs(mask) - 1 : 0;
    int ccur = __shfl(cand, lcur, kBprLanes);
    if (live) warp_row<T, R16>(V + (size_t)ccur * rank, rank, lane, cur);
    u64 lb;
    while ((lb = __ballot(live)) != 0ull) {
      scored += (unsigned)__popcll(lb) >> 4;
      const unsigned rest = mask & (mask - 1u);
      const bool more = live && rest != 0u;
      const int lnext = more ? __ffs(rest) - 1 : 0;
      const int cnext = __shfl(cand, lnext, kBprLanes);
      if (more) warp_row<T, R16>(V + (size_t)cnext * rank, rank, lane, nxt);   // in flight during the products and the halving
      double part = 0.0;
#pragma unroll
      for (int q = 0; q < R16; q++) {
        if (lane + kBprLanes * q < rank) {
          const double diff = (double)vi[q] - (double)cur[q];
          part = part + (double)ur[q] * diff;
        }
      }
      const double d = bpr_reduce16(part);
      if (live) {
        if (!seen) {
          seen = true;
          correct = d > 0.0;
        }
        if (d <= w.margin) {
          done = true;
          jn = ccur;
          tk = kBprLanes * r + lcur + 1;
          dk = d;
        }
      }
      mask = rest; lcur = lnext; ccur = cnext;
#pragma unroll
      for (int q = 0; q < R16; q++) cur[q] = nxt[q];
      live = !done && mask != 0u;
    }
  }
  const bool lead = has && lane == 0;
  const u64 bv = __ballot(lead && done), bl = __ballot(lead && seen), bc = __ballot(lead && correct);
  if ((threadIdx.x & 63) == 0) {
    if (bv) atomicAdd(&s_cnt[0], (unsigned)__popcll(bv));
    if (bl) atomicAdd(&s_cnt[1], (unsigned)__popcll(bl));
    if (bc) atomicAdd(&s_cnt[2], (unsigned)__popcll(bc));
    if (scored) atomicAdd(&s_cnt[3], scored);
  }
  if (lead) {
    tu[k] = u;
    ti[k] = pos;
    tj[k] = jn;
    if (tt) tt[k] = tk;
    z[k] = done ? s_w[tk - 1] / (1.0 + bpr_exp(dk)) : 0.0;
    if (keys) {
      keys[2 * (size_t)k] = done ? (uint32_t)pos : (uint32_t)a.n_items;
      keys[2 * (size_t)k + 1] = done ? (uint32_t)jn : (uint32_t)a.n_items;
      pay[2 * (size_t)k] = 2u * (uint32_t)k;
      pay[2 * (size_t)k + 1] = 2u * (uint32_t)k + 1u;
    }
  }
  __syncthreads();
  if (counts && threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

// 3. a group per run of equal u; the staging slot of a run is its user (by_user) or its first k, whichever array is smaller
template <class T, int R16>
__global__ __launch_bounds__(kBprThreads) void bpr_users_kernel(const int32_t* __restrict__ tu, const int32_t* __restrict__ ti,
                                                                const int32_t* __restrict__ tj, const double* __restrict__ z, int cnt,
                                                                int rank, const T* __restrict__ U, const T* __restrict__ V,
                                                                const double* __restrict__ aU, double lr, double lambda,
                                                                int by_user, T* __restrict__ stage, double* __restrict__ stage_a,
                                                                int32_t* __restrict__ scount) {
  const int k = blockIdx.x * kBprGroups + (threadIdx.x >> 4), lane = threadIdx.x & 15;
  if (k >= cnt) return;
  const int u = tu[k];
  if (k > 0 && tu[k - 1] == u) {
    if (lane == 0) scount[k] = 0;
    return;
  }
  double acc[R16], tot[R16];
#pragma unroll
  for (int q = 0; q < R16; q++) acc[q] = tot[q] = 0.0;
  int count = 0, in_chunk = 0;
  for (int e = k; e < cnt && tu[e] == u; e++) {
    const int jn = tj[e];
    if (jn < 0) continue;
    const double zz = z[e];
    const T* vi = V + (size_t)ti[e] * rank;
    const T* vj = V + (size_t)jn * rank;
#pragma unroll
    for (int q = 0; q < R16; q++) {
      const int c = lane + kBprLanes * q;
      if (c < rank) acc[q] = acc[q] + zz * ((double)vi[c] - (double)vj[c]);
    }
    count++;
    if (++in_chunk == kBprChunk) {
#pragma unroll
      for (int q = 0; q < R16; q++) {
        tot[q] = tot[q] + acc[q];
        acc[q] = 0.0;
      }
      in_chunk = 0;
    }
  }
  if (in_chunk) {
#pragma unroll
    for (int q = 0; q < R16; q++) tot[q] = tot[q] + acc[q];
  }
  const size_t slot = by_user ? (size_t)u : (size_t)k;
  if (count) bpr_update<T, R16>(tot, count, U + (size_t)u * rank, stage + slot * rank, aU[u], stage_a + slot, rank, lr, lambda, lane);
  if (lane == 0) scount[k] = count;
}

// 6. the staged rows of the runs that had a contribution
template <class T>
__global__ __launch_bounds__(kBprThreads) void bpr_copy_kernel(const int32_t* __restrict__ tu, const int32_t* __restrict__ scount, int cnt,
                                                               int rank, int by_user, const T* __restrict__ stage, const double* __restrict__ stage_a,
                                                               T* __restrict__ U, double* __restrict__ aU) {
  const int k = blockIdx.x * kBprGroups + (threadIdx.x >> 4), lane = threadIdx.x & 15;
  if (k >= cnt || scount[k] <= 0) return;
  const int u = tu[k];
  const size_t slot = by_user ? (size_t)u : (size_t)k;
  for (int c = lane; c < rank; c += kBprLanes) U[(size_t)u * rank + c] = stage[slot * rank + c];
  if (lane == 0) aU[u] = stage_a[slot];
}

// 4. seg[t] = the first sorted position whose key is >= t, t = 0 .. n_items (seg[n_items]: where the void triples begin);
// nch[t] = the chunks of a segment longer than one chunk, else 0 (nch[n_items] = 0: its scan slot holds the total)
__global__ __launch_bounds__(kBprThreads) void bpr_segments_kernel(const uint32_t* __restrict__ skeys, int n, int n_items,
                                                                   int32_t* __restrict__ seg) {
  const int t = blockIdx.x * kBprThreads + threadIdx.x;
  if (t > n_items) return;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (skeys[mid] < (uint32_t)t) lo = mid + 1; else hi = mid;
  }
  seg[t] = lo;
}
__global__ __launch_bounds__(kBprThreads) void bpr_chunks_kernel(const int32_t* __restrict__ seg, int n_items, int32_t* __restrict__ nch) {
  const int t = blockIdx.x * kBprThreads + threadIdx.x;
  if (t > n_items) return;
  const int len = t < n_items ? seg[t + 1] - seg[t] : 0;
  nch[t] = len > kBprChunk ? (len + kBprChunk - 1) / kBprChunk : 0;
}

// 5a. a group per chunk slot of the long segments
template <class T, int R16>
__global__ __launch_bounds__(kBprThreads) void bpr_item_chunks_kernel(const uint32_t* __restrict__ spay, const int32_t* __restrict__ seg,
                                                                      const int32_t* __restrict__ choff, int n_items,
                                                                      const int32_t* __restrict__ tu, const double* __restrict__ z,
                                                                      const T* __restrict__ U, int rank, double* __restrict__ csum) {
  const int g = blockIdx.x * kBprGroups + (threadIdx.x >> 4), lane = threadIdx.x & 15;
  if (g >= choff[n_items]) return;
  int lo = 0, hi = n_items;   // choff[lo] <= g < choff[hi]
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (choff[mid] <= g) lo = mid; else hi = mid;
  }
  const int start = seg[lo] + (g - choff[lo]) * kBprChunk, left = seg[lo + 1] - start;
  double acc[R16];
  bpr_item_walk<T, R16>(spay, tu, z, U, rank, start, left < kBprChunk ? left : kBprChunk, lane, acc);
#pragma unroll
  for (int q = 0; q < R16; q++) {
    const int c = lane + kBprLanes * q;
    if (c < rank) csum[(size_t)g * rank + c] = acc[q];
  }
}

// 5b. a group per item
template <class T, int R16>
__global__ __launch_bounds__(kBprThreads) void bpr_items_kernel(const uint32_t* __restrict__ spay, const int32_t* __restrict__ seg,
                                                                const int32_t* __restrict__ choff, int n_items,
                                                                const int32_t* __restrict__ tu, const double* __restrict__ z,
                                                                const T* __restrict__ U, int rank, const double* __restrict__ csum,
                                                                double lr, double lambda, T* __restrict__ V, double* __restrict__ aV) {
  const int t = blockIdx.x * kBprGroups + (threadIdx.x >> 4), lane = threadIdx.x & 15;
  if (t >= n_items) return;
  const int e0 = seg[t], len = seg[t + 1] - e0;
  if (len <= 0) return;
  double acc[R16], tot[R16];
  bpr_item_total<T, R16>(spay, choff, tu, z, U, rank, csum, t, e0, len, lane, acc, tot);
  T* row = V + (size_t)t * rank;
  bpr_update<T, R16>(tot, len, row, row, aV[t], aV + t, rank, lr, lambda, lane);
}

inline int bpr_bits(int n) {   // bits that hold 0 .. n
  int b = 1;
  while (b < 32 && ((int64_t)1 << b) <= (int64_t)n) b++;
  return b;
}

inline int bpr_cnt(int64_t nnz, int step, int n_steps) { return (int)((nnz - step + n_steps - 1) / n_steps); }

#define RSP_TRY(e) do { if ((err = (e)) != hipSuccess) return err; } while (0)

inline BprStep bpr_step_of(const BprRun& r, int epoch, int step) {
  BprStep a;
  a.p = r.p; a.j = r.j; a.n_rows = r.n_rows; a.n_items = r.n_items; a.row0 = r.row0;
  a.k0 = (unsigned)r.seed; a.k1 = (unsigned)(r.seed >> 32);
  a.c3 = (unsigned)epoch + (r.mode ? 0x80000000u : 0u);
  a.mode = r.mode; a.step = step; a.n_steps = r.n_steps; a.cnt = bpr_cnt(r.nnz, step, r.n_steps);
  return a;
}

template <class T, int R16>
hipError_t bpr_run(const BprRun& r, const WarpSearch* w, int epoch0, int n_epochs, int only_step, T* U, T* V, double* aU, double* aV,
                   unsigned long long* counts, hipStream_t s, const BprFeatures* ft) {
  hipError_t err;
  const int cmax = bpr_cnt(r.nnz, only_step < 0 ? 0 : only_step, r.n_steps), rank = r.rank, ni = r.n_items;
  if (cmax <= 0) return hipSuccess;
  const size_t cm = (size_t)cmax, slots = 4 * cm / kBprChunk + 1;
  DevBuf tu, ti, tj, z, stage, stage_a, scount, keys, keys_out, pay, pay_out, tmp, seg, nch, choff, scan_tmp, csum;
  RSP_TRY(tu.alloc(cm * 4));
  RSP_TRY(ti.alloc(cm * 4));
  RSP_TRY(tj.alloc(cm * 4));
  RSP_TRY(z.alloc(cm * 8));
  // one staging row per run: indexed by user when the rows are fewer than the step's slots (the fold-in, small batches of long
  // rows), by the run's first slot otherwise
  const int by_user = (size_t)r.n_rows < cm ? 1 : 0;
  const size_t n_stage = by_user ? (size_t)r.n_rows : cm;
  RSP_TRY(stage.alloc(n_stage * rank * sizeof(T)));
  RSP_TRY(stage_a.alloc(n_stage * 8));
  RSP_TRY(scount.alloc(cm * 4));
  size_t tmp_bytes = 0, scan_bytes = 0;
  const int key_bits = bpr_bits(ni);
  if (r.update_items) {
    RSP_TRY(keys.alloc(2 * cm * 4));
    RSP_TRY(keys_out.alloc(2 * cm * 4));
    RSP_TRY(pay.alloc(2 * cm * 4));
    RSP_TRY(pay_out.alloc(2 * cm * 4));
    // (the steps of an epoch hold cmax or cmax - 1 slots: the scratch is sized for either)
    for (size_t c = cm > 1 ? cm - 1 : cm; c <= cm; c++) {
      size_t bytes = 0;
      RSP_TRY(rocprim::radix_sort_pairs(nullptr, bytes, keys.as<uint32_t>(), keys_out.as<uint32_t>(), pay.as<uint32_t>(),
                                        pay_out.as<uint32_t>(), 2 * c, 0, key_bits, s));
      tmp_bytes = bytes > tmp_bytes ? bytes : tmp_bytes;
    }
    RSP_TRY(tmp.alloc(tmp_bytes));
    RSP_TRY(seg.alloc(((size_t)ni + 2) * 4));
    RSP_TRY(nch.alloc(((size_t)ni + 1) * 4));
    RSP_TRY(choff.alloc(((size_t)ni + 1) * 4));
    RSP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, nch.as<int32_t>(), choff.as<int32_t>(), (int32_t)0, (size_t)ni + 1,
                                    rocprim::plus<int32_t>(), s));
    RSP_TRY(scan_tmp.alloc(scan_bytes));
    RSP_TRY(csum.alloc(slots * rank * 8));
  }
  const dim3 block(kBprThreads);
  // item features: V is composed from H here and again behind every step that moved H.  The chunk offsets of the long columns
  // depend on F alone and are made once; a column of len > 64 positions has ceil(len / 64) < len / 32 slots, so nnz_f / 32 + 1
  // slots bound the workspace and the grid without reading the count back.
  const bool feat = ft && r.update_items;
  const int nf = ft ? ft->n_feat : 0;
  const size_t fslots = ft ? (size_t)(ft->nnz_f / 32) + 1 : 0;
  DevBuf G, icnt, fnch, fchoff, fscan_tmp, fsum, fcnt;
  size_t fscan_bytes = 0;
  if (ft) RSP_TRY(launch_compose_rows<T>(ft->fp, ft->fj, (const T*)ft->fx, ni, rank, (const T*)ft->H, V, s));
  if (feat) {
    RSP_TRY(G.alloc((size_t)ni * rank * 8));
    RSP_TRY(icnt.alloc((size_t)ni * 4));
    RSP_TRY(fnch.alloc(((size_t)nf + 1) * 4));
    RSP_TRY(fchoff.alloc(((size_t)nf + 1) * 4));
    RSP_TRY(fsum.alloc(fslots * rank * 8));
    RSP_TRY(fcnt.alloc(fslots * 4));
    RSP_TRY(rocprim::exclusive_scan(nullptr, fscan_bytes, fnch.as<int32_t>(), fchoff.as<int32_t>(), (int32_t)0, (size_t)nf + 1,
                                    rocprim::plus<int32_t>(), s));
    RSP_TRY(fscan_tmp.alloc(fscan_bytes));
    hipLaunchKernelGGL(bpr_chunks_kernel, bpr_grid((int64_t)nf + 1, kBprThreads), block, 0, s, ft->cp, nf, fnch.as<int32_t>());
    RSP_TRY(hipGetLastError());
    RSP_TRY(rocprim::exclusive_scan(fscan_tmp.p, fscan_bytes, fnch.as<int32_t>(), fchoff.as<int32_t>(), (int32_t)0, (size_t)nf + 1,
                                    rocprim::plus<int32_t>(), s));
  }
  for (int e = 0; e < n_epochs; e++) {
    for (int st = only_step < 0 ? 0 : only_step; st < (only_step < 0 ? r.n_steps : only_step + 1); st++) {
      const BprStep a = bpr_step_of(r, epoch0 + e, st);
      if (a.cnt <= 0) continue;
      const int cnt = a.cnt;
      const dim3 per_k = bpr_grid(cnt, kBprThreads), per_group = bpr_grid(cnt, kBprGroups);
      if (w) {   // WARP: the search writes what the sample and score kernels write
        hipLaunchKernelGGL((warp_search_kernel<T, R16>), per_group, block, 0, s, a, *w, rank, (const T*)U, (const T*)V, tu.as<int32_t>(),
                           ti.as<int32_t>(), tj.as<int32_t>(), (int32_t*)nullptr, z.as<double>(),
                           r.update_items ? keys.as<uint32_t>() : (uint32_t*)nullptr, r.update_items ? pay.as<uint32_t>() : (uint32_t*)nullptr,
                           counts + 4 * (size_t)e);
      } else {
        hipLaunchKernelGGL(bpr_sample_kernel, per_k, block, 0, s, a, tu.as<int32_t>(), ti.as<int32_t>(), tj.as<int32_t>(),
                           r.update_items ? keys.as<uint32_t>() : (uint32_t*)nullptr, r.update_items ? pay.as<uint32_t>() : (uint32_t*)nullptr);
        hipLaunchKernelGGL((bpr_z_kernel<T>), per_group, block, 0, s, (const int32_t*)tu.as<int32_t>(), (const int32_t*)ti.as<int32_t>(),
                           (const int32_t*)tj.as<int32_t>(), cnt, rank, (const T*)U, (const T*)V, z.as<double>(), counts + 2 * (size_t)e);
      }
      hipLaunchKernelGGL((bpr_users_kernel<T, R16>), per_group, block, 0, s, (const int32_t*)tu.as<int32_t>(),
                         (const int32_t*)ti.as<int32_t>(), (const int32_t*)tj.as<int32_t>(), (const double*)z.as<double>(), cnt, rank,
                         (const T*)U, (const T*)V, (const double*)aU, r.lr, r.lambda, by_user, stage.as<T>(), stage_a.as<double>(),
                         scount.as<int32_t>());
      RSP_TRY(hipGetLastError());
      if (r.update_items) {
        RSP_TRY(rocprim::radix_sort_pairs(tmp.p, tmp_bytes, keys.as<uint32_t>(), keys_out.as<uint32_t>(), pay.as<uint32_t>(),
                                          pay_out.as<uint32_t>(), 2 * (size_t)cnt, 0, key_bits, s));
        const dim3 per_item = bpr_grid((int64_t)ni + 1, kBprThreads);
        hipLaunchKernelGGL(bpr_segments_kernel, per_item, block, 0, s, (const uint32_t*)keys_out.as<uint32_t>(), 2 * cnt, ni,
                           seg.as<int32_t>());
        hipLaunchKernelGGL(bpr_chunks_kernel, per_item, block, 0, s, (const int32_t*)seg.as<int32_t>(), ni, nch.as<int32_t>());
        RSP_TRY(hipGetLastError());
        RSP_TRY(rocprim::exclusive_scan(scan_tmp.p, scan_bytes, nch.as<int32_t>(), choff.as<int32_t>(), (int32_t)0, (size_t)ni + 1,
                                        rocprim::plus<int32_t>(), s));
        const size_t step_slots = 4 * (size_t)cnt / kBprChunk + 1;
        hipLaunchKernelGGL((bpr_item_chunks_kernel<T, R16>), bpr_grid((int64_t)step_slots, kBprGroups), block, 0, s,
                           (const uint32_t*)pay_out.as<uint32_t>(), (const int32_t*)seg.as<int32_t>(), (const int32_t*)choff.as<int32_t>(),
                           ni, (const int32_t*)tu.as<int32_t>(), (const double*)z.as<double>(), (const T*)U, rank, csum.as<double>());
        if (feat) {
          RSP_TRY(launch_bpr_feat_backward<T>(*ft, ni, rank, fslots, fchoff.as<int32_t>(), pay_out.as<uint32_t>(), seg.as<int32_t>(),
                                              choff.as<int32_t>(), tu.as<int32_t>(), z.as<double>(), (const T*)U, csum.as<double>(),
                                              G.as<double>(), icnt.as<int32_t>(), fsum.as<double>(), fcnt.as<int32_t>(), r.lr, r.lambda, s));
          RSP_TRY(launch_compose_rows<T>(ft->fp, ft->fj, (const T*)ft->fx, ni, rank, (const T*)ft->H, V, s));
        } else {
          hipLaunchKernelGGL((bpr_items_kernel<T, R16>), bpr_grid(ni, kBprGroups), block, 0, s, (const uint32_t*)pay_out.as<uint32_t>(),
                             (const int32_t*)seg.as<int32_t>(), (const int32_t*)choff.as<int32_t>(), ni, (const int32_t*)tu.as<int32_t>(),
                             (const double*)z.as<double>(), (const T*)U, rank, (const double*)csum.as<double>(), r.lr, r.lambda, V, aV);
        }
      }
      hipLaunchKernelGGL((bpr_copy_kernel<T>), per_group, block, 0, s, (const int32_t*)tu.as<int32_t>(),
                         (const int32_t*)scount.as<int32_t>(), cnt, rank, by_user, (const T*)stage.as<T>(), (const double*)stage_a.as<double>(), U,
                         aU);
      RSP_TRY(hipGetLastError());
    }
  }
  RSP_TRY(hipStreamSynchronize(s));   // the scratch is freed on return
  return hipSuccess;
}

}  // namespace

hipError_t launch_bpr_triples(const BprRun& r, int epoch, int step, int32_t* tu, int32_t* ti, int32_t* tj, hipStream_t s) {
  const BprStep a = bpr_step_of(r, epoch, step);
  if (a.cnt <= 0) return hipSuccess;
  hipLaunchKernelGGL(bpr_sample_kernel, bpr_grid(a.cnt, kBprThreads), dim3(kBprThreads), 0, s, a, tu, ti, tj, (uint32_t*)nullptr,
                     (uint32_t*)nullptr);
  return hipGetLastError();
}

namespace {
template <class T>
hipError_t bpr_run_any(const BprRun& r, const WarpSearch* w, int epoch0, int n_epochs, int only_step, T* U, T* V, double* aU, double* aV,
                       unsigned long long* counts, hipStream_t s, const BprFeatures* ft) {
  const int r16 = (r.rank + kBprLanes - 1) / kBprLanes;
  if (r16 <= 1) return bpr_run<T, 1>(r, w, epoch0, n_epochs, only_step, U, V, aU, aV, counts, s, ft);
  if (r16 <= 2) return bpr_run<T, 2>(r, w, epoch0, n_epochs, only_step, U, V, aU, aV, counts, s, ft);
  if (r16 <= 4) return bpr_run<T, 4>(r, w, epoch0, n_epochs, only_step, U, V, aU, aV, counts, s, ft);
  if (r16 <= 8) return bpr_run<T, 8>(r, w, epoch0, n_epochs, only_step, U, V, aU, aV, counts, s, ft);
  return bpr_run<T, 16>(r, w, epoch0, n_epochs, only_step, U, V, aU, aV, counts, s, ft);
}

template <class T, int R16>
void warp_search(const BprStep& a, const WarpSearch& w, int rank, const T* U, const T* V, int32_t* tu, int32_t* ti, int32_t* tj,
                 int32_t* tt, double* z, hipStream_t s) {
  hipLaunchKernelGGL((warp_search_kernel<T, R16>), bpr_grid(a.cnt, kBprGroups), dim3(kBprThreads), 0, s, a, w, rank, U, V, tu, ti, tj, tt,
                     z, (uint32_t*)nullptr, (uint32_t*)nullptr, (unsigned long long*)nullptr);
}
}  // namespace

template <class T>
hipError_t launch_bpr_run(const BprRun& r, int epoch0, int n_epochs, int only_step, T* U, T* V, double* aU, double* aV,
                          unsigned long long* counts, hipStream_t s, const BprFeatures* ft) {
  return bpr_run_any<T>(r, nullptr, epoch0, n_epochs, only_step, U, V, aU, aV, counts, s, ft);
}
template hipError_t launch_bpr_run<float>(const BprRun&, int, int, int, float*, float*, double*, double*, unsigned long long*, hipStream_t,
                                          const BprFeatures*);
template hipError_t launch_bpr_run<double>(const BprRun&, int, int, int, double*, double*, double*, double*, unsigned long long*,
                                           hipStream_t, const BprFeatures*);

template <class T>
hipError_t launch_warp_run(const BprRun& r, const WarpSearch& w, int epoch0, int n_epochs, int only_step, T* U, T* V, double* aU,
                           double* aV, unsigned long long* counts, hipStream_t s, const BprFeatures* ft) {
  return bpr_run_any<T>(r, &w, epoch0, n_epochs, only_step, U, V, aU, aV, counts, s, ft);
}
template hipError_t launch_warp_run<float>(const BprRun&, const WarpSearch&, int, int, int, float*, float*, double*, double*,
                                           unsigned long long*, hipStream_t, const BprFeatures*);
template hipError_t launch_warp_run<double>(const BprRun&, const WarpSearch&, int, int, int, double*, double*, double*, double*,
                                            unsigned long long*, hipStream_t, const BprFeatures*);

template <class T>
hipError_t launch_warp_triples(const BprRun& r, const WarpSearch& w, int epoch, int step, const T* U, const T* V, int32_t* tu, int32_t* ti,
                               int32_t* tj, int32_t* tt, double* z, hipStream_t s) {
  const BprStep a = bpr_step_of(r, epoch, step);
  if (a.cnt <= 0) return hipSuccess;
  const int r16 = (r.rank + kBprLanes - 1) / kBprLanes;
  if (r16 <= 1) warp_search<T, 1>(a, w, r.rank, U, V, tu, ti, tj, tt, z, s);
  else if (r16 <= 2) warp_search<T, 2>(a, w, r.rank, U, V, tu, ti, tj, tt, z, s);
  else if (r16 <= 4) warp_search<T, 4>(a, w, r.rank, U, V, tu, ti, tj, tt, z, s);
  else if (r16 <= 8) warp_search<T, 8>(a, w, r.rank, U, V, tu, ti, tj, tt, z, s);
  else warp_search<T, 16>(a, w, r.rank, U, V, tu, ti, tj, tt, z, s);
  return hipGetLastError();
}
template hipError_t launch_warp_triples<float>(const BprRun&, const WarpSearch&, int, int, const float*, const float*, int32_t*, int32_t*,
                                               int32_t*, int32_t*, double*, hipStream_t);
template hipError_t launch_warp_triples<double>(const BprRun&, const WarpSearch&, int, int, const double*, const double*, int32_t*,
                                                int32_t*, int32_t*, int32_t*, double*, hipStream_t);

#undef RSP_TRY

}  // namespace rsparse_hip
