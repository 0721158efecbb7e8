// Device pieces that the BPR kernel files share (wrmf_bpr.hip: the steps; wrmf_bpr_features.hip: the pass through item features):
// the group geometry, the definition's halving, the ordered walk over an item's contributions and the Adagrad update.
#pragma once
#include "../../include/rsparse_wrmf_hip.h"
#include "wrmf_internal.h"

namespace rsparse_hip {
namespace bprdev {

constexpr int kBprThreads = 256;
constexpr int kBprLanes = 16;                          // lanes of a group: the 16 partial sums of the definition's dot product
constexpr int kBprGroups = kBprThreads / kBprLanes;    // groups per workgroup
constexpr int kBprChunk = RSPARSE_HIP_BPR_CHUNK;

inline dim3 bpr_grid(int64_t n, int per) { return dim3((unsigned)((n + per - 1) / per)); }

// the definition's halving of the 16 partial sums: every lane of the group ends with the same bits
__device__ __forceinline__ double bpr_reduce16(double v) {
  v = v + __shfl_xor(v, 8, kBprLanes);
  v = v + __shfl_xor(v, 4, kBprLanes);
  v = v + __shfl_xor(v, 2, kBprLanes);
  v = v + __shfl_xor(v, 1, kBprLanes);
  return v;
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
// the total of item t's segment of len >= 1 contributions from the sorted position e0: a short segment walked directly, a long
// one's chunk sums added in order
template <class T, int R16>
__device__ __forceinline__ void bpr_item_total(const uint32_t* __restrict__ spay, const int32_t* __restrict__ choff,
                                               const int32_t* __restrict__ tu, const double* __restrict__ z, const T* __restrict__ U,
                                               int rank, const double* __restrict__ csum, int t, int e0, int len, int lane,
                                               double (&acc)[R16], double (&tot)[R16]) {
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
}

}  // namespace bprdev
}  // namespace rsparse_hip
