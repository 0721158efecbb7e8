// Which row owns a stored position of a CSR pattern, for the kernels that run over positions instead of rows (wrmf_score.hip,
// wrmf_softals.hip), and the 4-coordinate piece of a factor row a lane of such a kernel owns.
#pragma once
#include "wrmf_wave.h"

namespace rsparse_hip {
namespace dev {

typedef double f64x2 __attribute__((ext_vector_type(2)));

// largest row in [0, n_rows) with P[row] <= t, for a wave-uniform t < P[n_rows] (and P[0] = 0 <= t).  Needs full EXEC.
__device__ __forceinline__ int wave_find_row(const int32_t* __restrict__ P, int n_rows, unsigned t, int lane) {
  int lo = 0, hi = n_rows;   // P[lo] <= t < P[hi]
  while (hi - lo > 1) {
    const int step = (hi - lo + 63) >> 6;
    const long long at = (long long)lo + (long long)(lane + 1) * step;
    const int idx = at < hi ? (int)at : hi;
    const int c = __popcll(__ballot((unsigned)P[idx] <= t));   // P ascends: the first c lanes (c < 64: lane 63 probes hi)
    const long long nlo = (long long)lo + (long long)c * step, nhi = nlo + step;
    lo = nlo < hi ? (int)nlo : hi;
    hi = nhi < hi ? (int)nhi : hi;
  }
  return lo;
}

// the same for one lane's own t, from a row `lo` with P[lo] <= t: doubling steps forward, then bisection
__device__ __forceinline__ int find_row_from(const int32_t* __restrict__ P, int n_rows, unsigned t, int lo) {
  int hi = lo + 1, step = 1;
  while (hi < n_rows && (unsigned)P[hi] <= t) {
    lo = hi;
    step <<= 1;
    hi = (n_rows - hi > step) ? hi + step : n_rows;
  }
  hi = min(hi, n_rows);   // P[n_rows] > t
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((unsigned)P[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

// coordinates c0 .. c0 + 3 of a row of r, zeros at and beyond r.  Without a branch: a lane beyond the row reads the row's first
// piece (its last element in the element-wise form) and drops it, so that the compiler keeps every gather of a step in flight.
template <class T, bool VEC>
__device__ __forceinline__ void load4(const T* __restrict__ row, int c0, int r, T (&x)[4]) {
  if constexpr (VEC) {   // r is a multiple of 4 and the row 16-byte aligned
    const bool in = c0 < r;
    const T* at = row + (in ? c0 : 0);
    if constexpr (std::is_same<T, float>::value) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(at);
      x[0] = v[0]; x[1] = v[1]; x[2] = v[2]; x[3] = v[3];
    } else {
      const f64x2 a = *reinterpret_cast<const f64x2*>(at), b = *reinterpret_cast<const f64x2*>(at + 2);
      x[0] = a[0]; x[1] = a[1]; x[2] = b[0]; x[3] = b[1];
    }
#pragma unroll
    for (int e = 0; e < 4; e++) x[e] = in ? x[e] : T(0);
  } else {
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const T v = row[min(c0 + e, r - 1)];
      x[e] = c0 + e < r ? v : T(0);
    }
  }
}

}  // namespace dev
}  // namespace rsparse_hip
