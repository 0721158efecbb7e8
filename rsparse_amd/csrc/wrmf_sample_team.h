// What the sampling kernels share (wrmf_sample.hip, wrmf_sample_weighted.hip): the prefix over a team's threads and the binary
// searches over ascending lists.  Device code only; include after wrmf_device.h.
#pragma once

namespace rsparse_hip {
namespace dev {

// exclusive prefix of v over the BS threads of the team in thread order; *total = the sum.  Uses sw[4]; every thread calls it.
template <int BS, class T>
__device__ __forceinline__ T team_scan(T v, T* sw, T* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  T incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if constexpr (BS == 64) {
    *total = __shfl(incl, 63);
    return incl - v;
  } else {
    if (lane == 63) sw[wv] = incl;
    __syncthreads();
    T off = 0, tot = 0;
    for (int w = 0; w < BS / 64; w++) {
      if (w < wv) off += sw[w];
      tot += sw[w];
    }
    __syncthreads();
    *total = tot;
    return off + incl - v;
  }
}

// #{i < len : a[i] - i <= r} for an ascending, unique a (a[i] - i does not decrease)
template <class A>
__device__ __forceinline__ int count_shifted_le(const A* a, int len, int r) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((long long)a[mid] - mid <= (long long)r) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// #{i < len : a[i] < v} for an ascending a
template <class A>
__device__ __forceinline__ int count_less(const A* a, int len, long long v) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((long long)a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

}  // namespace dev
}  // namespace rsparse_hip
