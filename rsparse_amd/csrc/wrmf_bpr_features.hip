// BPR / WARP through item features, on the device (gfx950): an item's row is F[i, :] H, and a step's gradient goes through F to
// the feature rows H.  rsparse_amd/bpr.py (compose_reference, bpr_feat_step_reference) is the definition in numpy, the C header
// states it for other hosts; DESIGN.md 3.36 has the scheme.  wrmf_bpr.hip runs the steps and calls in here for the compose before
// a step and, behind its sort and chunk launch, for the item totals and the backward pass.  Built with contraction off, as
// wrmf_bpr.hip: every product and sum is its own rounded float64 operation.
#include "wrmf_bpr_device.h"

#pragma clang fp contract(off)

namespace rsparse_hip {
namespace {

using namespace bprdev;

//
//   compose   a group per item walks its row of F in ascending feature order with the next feature's row of H requested while
//             the current one is multiplied: V[i] = sum_f F[i, f] H[f] in double registers from +0.0, one rounded store.  Where
//             rank % 4 == 0 (and H, V stand on 16 bytes) a lane owns four consecutive coordinates and moves them with one
//             16-byte access (two for doubles); the sum of a coordinate does not depend on which lane holds it.
//   totals    5b without the update: G[i] (doubles) and c[i], the item's total BEFORE the regularisation term, and its count
//             (0 for an item the step does not touch: every c is written, G only where c >= 1).
//   backward  F by feature (CSC, items ascending).  A column is cut into chunks of kBprChunk STORED POSITIONS, a cut that depends
//             on F alone: the chunk offsets of the columns longer than one chunk are made once per call.  A group per chunk slot
//             writes the slot's sum and count; a group per feature walks a short column itself or adds a long one's slots in
//             order, and updates H[f] and its `a` in place.  In a walk the 16 lanes read 16 positions' items and their c at once
//             (an untouched item costs its index and 4 bytes of c, never a row of G); the group's bits of the ballot are the
//             positions that contribute, walked in ascending order with the next row of G in flight.
template <class T> struct alignas(16) BprVec4 { T v[4]; };

template <int R16, bool VEC> constexpr int bpr_vec_regs() { return VEC ? 4 * ((R16 + 3) / 4) : R16; }

// a row of `rank` elements into a lane's registers.  VEC: element 4 m + i is the coordinate 4 (lane + 16 m) + i; else element q
// is the coordinate lane + 16 q
template <class T, int NE, bool VEC>
__device__ __forceinline__ void bpr_row_load(const T* __restrict__ row, int rank, int lane, T (&out)[NE]) {
  if constexpr (VEC) {
#pragma unroll
    for (int m = 0; m < NE / 4; m++) {
      const int c = 4 * (lane + kBprLanes * m);
      if (c < rank) {
        const BprVec4<T> v = *reinterpret_cast<const BprVec4<T>*>(row + c);
#pragma unroll
        for (int i = 0; i < 4; i++) out[4 * m + i] = v.v[i];
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < NE; q++) {
      const int c = lane + kBprLanes * q;
      if (c < rank) out[q] = row[c];
    }
  }
}

template <class T, int R16, bool VEC>
__global__ __launch_bounds__(kBprThreads) void bpr_compose_kernel(const int32_t* __restrict__ fp, const int32_t* __restrict__ fj,
                                                                  const T* __restrict__ fx, int n_items, int rank,
                                                                  const T* __restrict__ H, T* __restrict__ V) {
  constexpr int NE = bpr_vec_regs<R16, VEC>();
  const int t = blockIdx.x * kBprGroups + (threadIdx.x >> 4), lane = threadIdx.x & 15;
  if (t >= n_items) return;
  const int b = fp[t], e = fp[t + 1];
  double acc[NE];
  T cur[NE], nxt[NE];
#pragma unroll
  for (int q = 0; q < NE; q++) {
    acc[q] = 0.0;
    cur[q] = nxt[q] = (T)0;
  }
  if (b < e) bpr_row_load<T, NE, VEC>(H + (size_t)fj[b] * rank, rank, lane, cur);
  for (int s = b; s < e; s++) {
    const double x = (double)fx[s];
    if (s + 1 < e) bpr_row_load<T, NE, VEC>(H + (size_t)fj[s + 1] * rank, rank, lane, nxt);   // in flight during the products
#pragma unroll
    for (int q = 0; q < NE; q++) acc[q] = acc[q] + x * (double)cur[q];
#pragma unroll
    for (int q = 0; q < NE; q++) cur[q] = nxt[q];
  }
  T* row = V + (size_t)t * rank;
  if constexpr (VEC) {
#pragma unroll
    for (int m = 0; m < NE / 4; m++) {
      const int c = 4 * (lane + kBprLanes * m);
      if (c < rank) {
        BprVec4<T> v;
#pragma unroll
        for (int i = 0; i < 4; i++) v.v[i] = (T)acc[4 * m + i];
        *reinterpret_cast<BprVec4<T>*>(row + c) = v;
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < NE; q++) {
      const int c = lane + kBprLanes * q;
      if (c < rank) row[c] = (T)acc[q];
    }
  }
}

// 5b of the feature path: the item's total and count leave as they are
template <class T, int R16>
__global__ __launch_bounds__(kBprThreads) void bpr_item_totals_kernel(const uint32_t* __restrict__ spay, const int32_t* __restrict__ seg,
                                                                      const int32_t* __restrict__ choff, int n_items,
                                                                      const int32_t* __restrict__ tu, const double* __restrict__ z,
                                                                      const T* __restrict__ U, int rank, const double* __restrict__ csum,
                                                                      double* __restrict__ G, int32_t* __restrict__ icnt) {
  const int t = blockIdx.x * kBprGroups + (threadIdx.x >> 4), lane = threadIdx.x & 15;
  if (t >= n_items) return;
  const int e0 = seg[t], len = seg[t + 1] - e0;
  if (lane == 0) icnt[t] = len > 0 ? len : 0;
  if (len <= 0) return;
  double acc[R16], tot[R16];
  bpr_item_total<T, R16>(spay, choff, tu, z, U, rank, csum, t, e0, len, lane, acc, tot);
#pragma unroll
  for (int q = 0; q < R16; q++) {
    const int c = lane + kBprLanes * q;
    if (c < rank) G[(size_t)t * rank + c] = tot[q];
  }
}

__device__ __forceinline__ int bpr_sum16(int v) {
  v += __shfl_xor(v, 8, kBprLanes);
  v += __shfl_xor(v, 4, kBprLanes);
  v += __shfl_xor(v, 2, kBprLanes);
  v += __shfl_xor(v, 1, kBprLanes);
  return v;
}

// the sum of F[i, f] G[i] over the m <= kBprChunk stored positions s0 .. of a column whose item has c >= 1, sequentially from
// +0.0 in ascending position -> the sum of those c.  Every branch and loop is uniform over the group (s0 and m are), which is
// what the shuffles need; the ballot gives each group its own 16 bits.
template <class T, int R16>
__device__ __forceinline__ int bpr_feat_walk(const int32_t* __restrict__ ci, const T* __restrict__ cx, const int32_t* __restrict__ icnt,
                                             const double* __restrict__ G, int rank, int s0, int m, int lane, int shift,
                                             double (&acc)[R16]) {
  double cur[R16], nxt[R16];
#pragma unroll
  for (int q = 0; q < R16; q++) acc[q] = cur[q] = nxt[q] = 0.0;
  int total = 0;
  for (int r = 0; r < m; r += kBprLanes) {
    int item = 0, c = 0;
    double x = 0.0;
    if (r + lane < m) {
      item = ci[s0 + r + lane];
      c = icnt[item];
      if (c > 0) x = (double)cx[s0 + r + lane];
    }
    total += bpr_sum16(c);
    unsigned mask = (unsigned)(__ballot(c > 0) >> shift) & 0xffffu;
    const int first = __shfl(item, mask ? __ffs(mask) - 1 : 0, kBprLanes);
    if (mask) bpr_row_load<double, R16, false>(G + (size_t)first * rank, rank, lane, cur);
    while (mask) {
      const unsigned rest = mask & (mask - 1u);
      const double xx = __shfl(x, __ffs(mask) - 1, kBprLanes);
      const int next = __shfl(item, rest ? __ffs(rest) - 1 : 0, kBprLanes);
      if (rest) bpr_row_load<double, R16, false>(G + (size_t)next * rank, rank, lane, nxt);   // in flight during the products
#pragma unroll
      for (int q = 0; q < R16; q++) acc[q] = acc[q] + xx * cur[q];
#pragma unroll
      for (int q = 0; q < R16; q++) cur[q] = nxt[q];
      mask = rest;
    }
  }
  return total;
}

// backward a. a group per chunk slot of the columns longer than one chunk
template <class T, int R16>
__global__ __launch_bounds__(kBprThreads) void bpr_feat_chunks_kernel(const int32_t* __restrict__ cp, const int32_t* __restrict__ ci,
                                                                      const T* __restrict__ cx, const int32_t* __restrict__ fchoff,
                                                                      int n_feat, const int32_t* __restrict__ icnt,
                                                                      const double* __restrict__ G, int rank, double* __restrict__ fsum,
                                                                      int32_t* __restrict__ fcnt) {
  const int g = blockIdx.x * kBprGroups + (threadIdx.x >> 4), lane = threadIdx.x & 15;
  if (g >= fchoff[n_feat]) return;
  int lo = 0, hi = n_feat;   // fchoff[lo] <= g < fchoff[hi]
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (fchoff[mid] <= g) lo = mid; else hi = mid;
  }
  const int start = cp[lo] + (g - fchoff[lo]) * kBprChunk, left = cp[lo + 1] - start;
  double acc[R16];
  const int total = bpr_feat_walk<T, R16>(ci, cx, icnt, G, rank, start, left < kBprChunk ? left : kBprChunk, lane, threadIdx.x & 48, acc);
#pragma unroll
  for (int q = 0; q < R16; q++) {
    const int c = lane + kBprLanes * q;
    if (c < rank) fsum[(size_t)g * rank + c] = acc[q];
  }
  if (lane == 0) fcnt[g] = total;
}

// backward b. a group per feature
template <class T, int R16>
__global__ __launch_bounds__(kBprThreads) void bpr_feat_finish_kernel(const int32_t* __restrict__ cp, const int32_t* __restrict__ ci,
                                                                      const T* __restrict__ cx, const int32_t* __restrict__ fchoff,
                                                                      int n_feat, const int32_t* __restrict__ icnt,
                                                                      const double* __restrict__ G, int rank,
                                                                      const double* __restrict__ fsum, const int32_t* __restrict__ fcnt,
                                                                      double lr, double lambda, T* __restrict__ H,
                                                                      double* __restrict__ aH) {
  const int f = blockIdx.x * kBprGroups + (threadIdx.x >> 4), lane = threadIdx.x & 15;
  if (f >= n_feat) return;
  const int s0 = cp[f], len = cp[f + 1] - s0;
  if (len <= 0) return;
  double acc[R16], tot[R16];
  int total = 0;
  if (len <= kBprChunk) {
    total = bpr_feat_walk<T, R16>(ci, cx, icnt, G, rank, s0, len, lane, threadIdx.x & 48, acc);
#pragma unroll
    for (int q = 0; q < R16; q++) tot[q] = 0.0 + acc[q];
  } else {
#pragma unroll
    for (int q = 0; q < R16; q++) tot[q] = 0.0;
    // the slot sums are added in order, but kAhead of them are requested at once: a popular feature has hundreds of slots, and
    // one load per add would make its group the tail of the launch
    constexpr int kAhead = R16 <= 8 ? 4 : 2;
    const int g0 = fchoff[f], g1 = fchoff[f + 1];
    for (int g = g0; g < g1; g += kAhead) {
      double v[kAhead][R16];
#pragma unroll
      for (int k = 0; k < kAhead; k++) {
        if (g + k < g1) {
          total += fcnt[g + k];
#pragma unroll
          for (int q = 0; q < R16; q++) {
            const int c = lane + kBprLanes * q;
            v[k][q] = c < rank ? fsum[(size_t)(g + k) * rank + c] : 0.0;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < kAhead; k++) {
        if (g + k < g1) {
#pragma unroll
          for (int q = 0; q < R16; q++) tot[q] = tot[q] + v[k][q];
        }
      }
    }
  }
  if (total <= 0) return;
  T* row = H + (size_t)f * rank;
  bpr_update<T, R16>(tot, total, row, row, aH[f], aH + f, rank, lr, lambda, lane);
}
// V = F H; vec: the 16-byte form (rank % 4 == 0, H and V on 16 bytes)
template <class T, int R16>
void bpr_compose(const int32_t* fp, const int32_t* fj, const T* fx, int n_items, int rank, const T* H, T* V, hipStream_t s) {
  if (n_items <= 0) return;
  const bool vec = rank % 4 == 0 && (uintptr_t)H % 16 == 0 && (uintptr_t)V % 16 == 0;
  if (vec) hipLaunchKernelGGL((bpr_compose_kernel<T, R16, true>), bpr_grid(n_items, kBprGroups), dim3(kBprThreads), 0, s, fp, fj, fx, n_items, rank, H, V);
  else hipLaunchKernelGGL((bpr_compose_kernel<T, R16, false>), bpr_grid(n_items, kBprGroups), dim3(kBprThreads), 0, s, fp, fj, fx, n_items, rank, H, V);
}
}  // namespace

template <class T>
hipError_t launch_compose_rows(const int32_t* fp, const int32_t* fj, const T* fx, int n_items, int rank, const T* H, T* V, hipStream_t s) {
  const int r16 = (rank + kBprLanes - 1) / kBprLanes;
  if (r16 <= 1) bpr_compose<T, 1>(fp, fj, fx, n_items, rank, H, V, s);
  else if (r16 <= 2) bpr_compose<T, 2>(fp, fj, fx, n_items, rank, H, V, s);
  else if (r16 <= 4) bpr_compose<T, 4>(fp, fj, fx, n_items, rank, H, V, s);
  else if (r16 <= 8) bpr_compose<T, 8>(fp, fj, fx, n_items, rank, H, V, s);
  else bpr_compose<T, 16>(fp, fj, fx, n_items, rank, H, V, s);
  return hipGetLastError();
}
template hipError_t launch_compose_rows<float>(const int32_t*, const int32_t*, const float*, int, int, const float*, float*, hipStream_t);
template hipError_t launch_compose_rows<double>(const int32_t*, const int32_t*, const double*, int, int, const double*, double*, hipStream_t);

// the item totals (G, icnt) of a step whose sorted payloads, segments and chunk sums stand ready, then the backward pass through
// F by feature into H and aH.  fchoff: the chunk offsets of the columns longer than one chunk (n_feat + 1), made once per call;
// fslots: their bound nnz_f / 32 + 1 -- the chunk launch is sized by it on every step, because the true count fchoff[n_feat]
// would cost the call a read-back; the groups past it leave at once.
template <class T, int R16>
static void bpr_feat_backward(const BprFeatures& ft, int ni, int rank, size_t fslots, const int32_t* fchoff, const uint32_t* spay,
                              const int32_t* seg, const int32_t* choff, const int32_t* tu, const double* z, const T* U, const double* csum,
                              double* G, int32_t* icnt, double* fsum, int32_t* fcnt, double lr, double lambda, hipStream_t s) {
  const dim3 block(kBprThreads);
  const int nf = ft.n_feat;
  hipLaunchKernelGGL((bpr_item_totals_kernel<T, R16>), bpr_grid(ni, kBprGroups), block, 0, s, spay, seg, choff, ni, tu, z, U, rank, csum, G, icnt);
  hipLaunchKernelGGL((bpr_feat_chunks_kernel<T, R16>), bpr_grid((int64_t)fslots, kBprGroups), block, 0, s, ft.cp, ft.ci, (const T*)ft.cx, fchoff,
                     nf, (const int32_t*)icnt, (const double*)G, rank, fsum, fcnt);
  hipLaunchKernelGGL((bpr_feat_finish_kernel<T, R16>), bpr_grid(nf, kBprGroups), block, 0, s, ft.cp, ft.ci, (const T*)ft.cx, fchoff, nf,
                     (const int32_t*)icnt, (const double*)G, rank, (const double*)fsum, (const int32_t*)fcnt, lr, lambda, (T*)ft.H, ft.aH);
}

template <class T>
hipError_t launch_bpr_feat_backward(const BprFeatures& ft, int ni, int rank, size_t fslots, const int32_t* fchoff, const uint32_t* spay,
                                    const int32_t* seg, const int32_t* choff, const int32_t* tu, const double* z, const T* U,
                                    const double* csum, double* G, int32_t* icnt, double* fsum, int32_t* fcnt, double lr, double lambda,
                                    hipStream_t s) {
  const int r16 = (rank + kBprLanes - 1) / kBprLanes;
  if (r16 <= 1) bpr_feat_backward<T, 1>(ft, ni, rank, fslots, fchoff, spay, seg, choff, tu, z, U, csum, G, icnt, fsum, fcnt, lr, lambda, s);
  else if (r16 <= 2) bpr_feat_backward<T, 2>(ft, ni, rank, fslots, fchoff, spay, seg, choff, tu, z, U, csum, G, icnt, fsum, fcnt, lr, lambda, s);
  else if (r16 <= 4) bpr_feat_backward<T, 4>(ft, ni, rank, fslots, fchoff, spay, seg, choff, tu, z, U, csum, G, icnt, fsum, fcnt, lr, lambda, s);
  else if (r16 <= 8) bpr_feat_backward<T, 8>(ft, ni, rank, fslots, fchoff, spay, seg, choff, tu, z, U, csum, G, icnt, fsum, fcnt, lr, lambda, s);
  else bpr_feat_backward<T, 16>(ft, ni, rank, fslots, fchoff, spay, seg, choff, tu, z, U, csum, G, icnt, fsum, fcnt, lr, lambda, s);
  return hipGetLastError();
}
template hipError_t launch_bpr_feat_backward<float>(const BprFeatures&, int, int, size_t, const int32_t*, const uint32_t*, const int32_t*,
                                                    const int32_t*, const int32_t*, const double*, const float*, const double*, double*,
                                                    int32_t*, double*, int32_t*, double, double, hipStream_t);
template hipError_t launch_bpr_feat_backward<double>(const BprFeatures&, int, int, size_t, const int32_t*, const uint32_t*, const int32_t*,
                                                     const int32_t*, const int32_t*, const double*, const double*, const double*, double*,
                                                     int32_t*, double*, int32_t*, double, double, hipStream_t);

}  // namespace rsparse_hip
