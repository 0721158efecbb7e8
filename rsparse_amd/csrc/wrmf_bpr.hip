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
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/rsparse_wrmf_hip.h"
#include "wrmf_internal.h"
#include "wrmf_device.h"

#pragma clang fp contract(off)

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kBprThreads = 256;
constexpr int kBprLanes = 16;                          // lanes of a group: the 16 partial sums of the definition's dot product
constexpr int kBprGroups = kBprThreads / kBprLanes;    // groups per workgroup
constexpr int kBprChunk = RSPARSE_HIP_BPR_CHUNK;

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

// the definition's halving of the 16 partial sums: every lane of the group ends with the same bits
__device__ __forceinline__ double bpr_reduce16(double v) {
  v = v + __shfl_xor(v, 8, kBprLanes);
  v = v + __shfl_xor(v, 4, kBprLanes);
  v = v + __shfl_xor(v, 2, kBprLanes);
  v = v + __shfl_xor(v, 1, kBprLanes);
  return v;
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

// The update of a destination row with `count` >= 1 contributions whose total the group holds (lane l: the coordinates
// l + 16 q): g = total - (lambda count) row, a' = a + <g, g> / rank, row' = row + (lr g) / sqrt(a') unless a' == 0.
// out may be the row itself; another place receives the unchanged row when a' == 0.
template <class T, int R16>
__device__ __forceinline__ void bpr_update(double (&tot)[R16], int count, const T* row, T* out, double a, double* a_out, int rank,
                                           double lr, double lambda, int lane) {
  const double lc = lambda * (double)count;
  double part = 0.0;
#pragma unroll
  for (int q = 0; q < R16; q++) {
    const int c = lane + kBprLanes * q;
    if (c < rank) {
      const double g = tot[q] - lc * (double)row[c];
      tot[q] = g;
      part = part + g * g;
    }
  }
  const double an = a + bpr_reduce16(part) / (double)rank;
  const double root = sqrt(an);
#pragma unroll
  for (int q = 0; q < R16; q++) {
    const int c = lane + kBprLanes * q;
    if (c < rank) {
      const T old = row[c];
      if (an != 0.0) out[c] = (T)((double)old + (lr * tot[q]) / root);
      else if (out != row) out[c] = old;
    }
  }
  if (lane == 0) *a_out = an;
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

// the sum of the m <= kBprChunk contributions at the sorted positions e0 .. of an item, sequentially from +0.0
template <class T, int R16>
__device__ __forceinline__ void bpr_item_walk(const uint32_t* __restrict__ spay, const int32_t* __restrict__ tu,
                                              const double* __restrict__ z, const T* __restrict__ U, int rank, int e0, int m, int lane,
                                              double (&acc)[R16]) {
#pragma unroll
  for (int q = 0; q < R16; q++) acc[q] = 0.0;
  for (int e = e0; e < e0 + m; e++) {
    const uint32_t pay = spay[e];
    const int k = (int)(pay >> 1);
    const double zk = z[k], zz = (pay & 1u) ? -zk : zk;
    const T* ur = U + (size_t)tu[k] * rank;
#pragma unroll
    for (int q = 0; q < R16; q++) {
      const int c = lane + kBprLanes * q;
      if (c < rank) acc[q] = acc[q] + zz * (double)ur[c];
    }
  }
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
  if (len <= kBprChunk) {
    bpr_item_walk<T, R16>(spay, tu, z, U, rank, e0, len, lane, acc);
#pragma unroll
    for (int q = 0; q < R16; q++) tot[q] = 0.0 + acc[q];
  } else {
#pragma unroll
    for (int q = 0; q < R16; q++) tot[q] = 0.0;
    const int g0 = choff[t], n = choff[t + 1] - g0;
    for (int g = g0; g < g0 + n; g++) {
#pragma unroll
      for (int q = 0; q < R16; q++) {
        const int c = lane + kBprLanes * q;
        if (c < rank) tot[q] = tot[q] + csum[(size_t)g * rank + c];
      }
    }
  }
  T* row = V + (size_t)t * rank;
  bpr_update<T, R16>(tot, len, row, row, aV[t], aV + t, rank, lr, lambda, lane);
}

inline int bpr_bits(int n) {   // bits that hold 0 .. n
  int b = 1;
  while (b < 32 && ((int64_t)1 << b) <= (int64_t)n) b++;
  return b;
}

inline int bpr_cnt(int64_t nnz, int step, int n_steps) { return (int)((nnz - step + n_steps - 1) / n_steps); }

inline dim3 bpr_grid(int64_t n, int per) { return dim3((unsigned)((n + per - 1) / per)); }

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
hipError_t bpr_run(const BprRun& r, int epoch0, int n_epochs, int only_step, T* U, T* V, double* aU, double* aV,
                   unsigned long long* counts, hipStream_t s) {
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
  for (int e = 0; e < n_epochs; e++) {
    for (int st = only_step < 0 ? 0 : only_step; st < (only_step < 0 ? r.n_steps : only_step + 1); st++) {
      const BprStep a = bpr_step_of(r, epoch0 + e, st);
      if (a.cnt <= 0) continue;
      const int cnt = a.cnt;
      const dim3 per_k = bpr_grid(cnt, kBprThreads), per_group = bpr_grid(cnt, kBprGroups);
      hipLaunchKernelGGL(bpr_sample_kernel, per_k, block, 0, s, a, tu.as<int32_t>(), ti.as<int32_t>(), tj.as<int32_t>(),
                         r.update_items ? keys.as<uint32_t>() : (uint32_t*)nullptr, r.update_items ? pay.as<uint32_t>() : (uint32_t*)nullptr);
      hipLaunchKernelGGL((bpr_z_kernel<T>), per_group, block, 0, s, (const int32_t*)tu.as<int32_t>(), (const int32_t*)ti.as<int32_t>(),
                         (const int32_t*)tj.as<int32_t>(), cnt, rank, (const T*)U, (const T*)V, z.as<double>(), counts + 2 * (size_t)e);
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
        hipLaunchKernelGGL((bpr_items_kernel<T, R16>), bpr_grid(ni, kBprGroups), block, 0, s, (const uint32_t*)pay_out.as<uint32_t>(),
                           (const int32_t*)seg.as<int32_t>(), (const int32_t*)choff.as<int32_t>(), ni, (const int32_t*)tu.as<int32_t>(),
                           (const double*)z.as<double>(), (const T*)U, rank, (const double*)csum.as<double>(), r.lr, r.lambda, V, aV);
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

template <class T>
hipError_t launch_bpr_run(const BprRun& r, int epoch0, int n_epochs, int only_step, T* U, T* V, double* aU, double* aV,
                          unsigned long long* counts, hipStream_t s) {
  const int r16 = (r.rank + kBprLanes - 1) / kBprLanes;
  if (r16 <= 1) return bpr_run<T, 1>(r, epoch0, n_epochs, only_step, U, V, aU, aV, counts, s);
  if (r16 <= 2) return bpr_run<T, 2>(r, epoch0, n_epochs, only_step, U, V, aU, aV, counts, s);
  if (r16 <= 4) return bpr_run<T, 4>(r, epoch0, n_epochs, only_step, U, V, aU, aV, counts, s);
  if (r16 <= 8) return bpr_run<T, 8>(r, epoch0, n_epochs, only_step, U, V, aU, aV, counts, s);
  return bpr_run<T, 16>(r, epoch0, n_epochs, only_step, U, V, aU, aV, counts, s);
}
template hipError_t launch_bpr_run<float>(const BprRun&, int, int, int, float*, float*, double*, double*, unsigned long long*, hipStream_t);
template hipError_t launch_bpr_run<double>(const BprRun&, int, int, int, double*, double*, double*, double*, unsigned long long*,
                                           hipStream_t);

#undef RSP_TRY

}  // namespace rsparse_hip
