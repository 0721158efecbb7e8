// The initial factor matrices drawn on the device -- what the reference fills on the host with R's generator
// (large_rand_matrix, src/utils.cpp:130-151; R/model_WRMF.R:203-255: N(0, 1) / 100, |.| for NNLS, the rows of ones of the
// bias models).  gfx950, wave64; a streaming, write-only kernel.  The stream is a FUNCTION of the element, not a state:
//   bits      Philox4x32-10 (Random123): multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85
//   index     the matrix is (n_rows, rank) row-major (= the reference's column-major rank x n); e = row * rank + col, 64 bits,
//             over the WHOLE matrix -- the leading dimension of the output plays no part
//   counter   (lo32(e >> 2), hi32(e >> 2), stream, 0),  key (lo32(seed), hi32(seed));  stream 0 = users, 1 = items
//   outputs   one call gives o0..o3 and four normals; element e takes number e & 3 (rank % 4 != 0: a group straddles two rows)
//   uniforms  u_a = ((o0 >> 8) + 1) 2^-24 in (0, 1],  u_b = (o1 >> 8) 2^-24 in [0, 1): 24 bits, exact in fp32
//   normals   r = sqrt(-2 ln u_a); numbers 0, 1 = r cos(2 pi u_b), r sin(2 pi u_b); 2, 3 the same from (o2, o3)
//   value     scale * z, |.| with abs_values; the column ones_col (-1: none) is exactly 1
// so a value depends on (seed, stream, row, col, rank) alone: not on the launch geometry, the row range asked for, the number
// of ranks that each draw their own rows, or the device.  rsparse_amd/rng.py is the same definition in numpy.
//
// Geometry.  A lane owns whole Philox groups (4 consecutive elements) and a grid of at most kInitMaxBlocks workgroups strides
// over the groups of the row range, consecutive lanes on consecutive groups:
//   * VEC (ld == rank, the range starts on a group and the output is 16-byte aligned): a group that lies inside the range is
//     one 16-byte store of fp32 (two of fp64, adjacent): a wave instruction writes 1 KiB contiguous, the widest store there
//     is.  The column of an element is only needed for ones_col, one 64-bit remainder per group when it is asked for.
//   * otherwise, and for the group the range ends in: element by element, (row, col) from one 64-bit division per group and
//     carried from there; stores of 4 / 8 bytes at (row - row0) * ld + col.  Nothing outside the range's rank columns is
//     written: the padding of ld > rank is not touched.
// All index arithmetic is 64 bits wide (a 10M x 128 matrix has 1.28e9 elements, a shard may start past 2^32).
// The fp32 output is computed in fp32 (logf / sqrtf / sincospif, the accurate forms: <= 1, <= 0.5 and <= 2 ulp), the fp64
// output in double; nothing is read from memory.
#include <algorithm>

#include "wrmf_internal.h"
#include "wrmf_device.h"

namespace rsparse_hip {
namespace {

using namespace dev;

typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int kInitThreads = 256;
// (at 8 waves per SIMD 2048 workgroups of 256 are resident on 256 CUs: 32 rounds of them, enough to even out the tail)
constexpr unsigned kInitMaxBlocks = 1u << 16;

// one Box-Muller pair from two words, in the arithmetic of the output type
__device__ __forceinline__ void normal_pair(unsigned a, unsigned b, float& z0, float& z1) {
  const float ua = (float)((a >> 8) + 1u) * 0x1p-24f, ub2 = (float)(b >> 8) * 0x1p-23f;   // (2 u_b: exact)
  const float r = sqrtf(-2.0f * logf(ua));
  float s, c;
  sincospif(ub2, &s, &c);
  z0 = r * c;
  z1 = r * s;
}
__device__ __forceinline__ void normal_pair(unsigned a, unsigned b, double& z0, double& z1) {
  const double ua = (double)((a >> 8) + 1u) * 0x1p-24, ub2 = (double)(b >> 8) * 0x1p-23;
  const double r = sqrt(-2.0 * log(ua));
  double s, c;
  sincospi(ub2, &s, &c);
  z0 = r * c;
  z1 = r * s;
}

template <class T>
__device__ __forceinline__ void store4(T* at, const T (&v)[4]) {
  if constexpr (std::is_same<T, float>::value) {
    f32x4 x = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(at) = x;
  } else {
    f64x2 x = {v[0], v[1]}, y = {v[2], v[3]};
    *reinterpret_cast<f64x2*>(at) = x;
    *reinterpret_cast<f64x2*>(at + 2) = y;
  }
}

// out: row row0's first element; the elements [e0, e1) = [row0 * rank, (row0 + n_rows) * rank) of the whole matrix, their
// groups [g0, g0 + n_groups)
template <class T, bool VEC>
__global__ __launch_bounds__(kInitThreads) void init_factors_kernel(T* __restrict__ out, u64 e0, u64 e1, u64 g0, u64 n_groups,
                                                                    unsigned rank, u64 ld, u64 row0, unsigned k0, unsigned k1,
                                                                    unsigned stream, double scale, int abs_values, int ones_col) {
  const u64 stride = (u64)gridDim.x * kInitThreads;
  for (u64 i = (u64)blockIdx.x * kInitThreads + threadIdx.x; i < n_groups; i += stride) {
    const u64 g = g0 + i, first = g << 2;
    unsigned o[4];
    philox4x32_10((unsigned)g, (unsigned)(g >> 32), stream, 0u, k0, k1, o);
    T v[4];
    normal_pair(o[0], o[1], v[0], v[1]);
    normal_pair(o[2], o[3], v[2], v[3]);
#pragma unroll
    for (int t = 0; t < 4; t++) {
      v[t] = (T)(scale * (double)v[t]);   // (one rounding: `scale` itself is not an fp32 number)
      if (abs_values) v[t] = fabs(v[t]);
    }
    if (VEC && first + 4 <= e1) {   // (VEC: first >= e0, and out + (first - e0) is 16-byte aligned)
      if (ones_col >= 0) {
        unsigned col = (unsigned)(first % rank);
#pragma unroll
        for (int t = 0; t < 4; t++) {
          if (col == (unsigned)ones_col) v[t] = T(1);
          col = col + 1 == rank ? 0u : col + 1;
        }
      }
      store4(out + (first - e0), v);
    } else {
      const u64 lo = first > e0 ? first : e0;   // the group's elements inside the range: [lo, hi)
      const u64 hi = first + 4 < e1 ? first + 4 : e1;
      u64 row = lo / rank;
      unsigned col = (unsigned)(lo - row * rank);
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const u64 e = first + t;
        if (e >= lo && e < hi) {
          out[(row - row0) * ld + col] = col == (unsigned)ones_col ? T(1) : v[t];
          if (++col == rank) {
            col = 0;
            row++;
          }
        }
      }
    }
  }
}

}  // namespace

template <class T>
hipError_t launch_init_factors(uint64_t seed, int stream, int64_t row0, int n_rows, int rank, int64_t ld, double scale,
                               int abs_values, int ones_col, T* out, hipStream_t s) {
  if (n_rows <= 0) return hipSuccess;
  const u64 e0 = (u64)row0 * (u64)rank, e1 = ((u64)row0 + (u64)n_rows) * (u64)rank;
  const u64 g0 = e0 >> 2, n_groups = ((e1 + 3) >> 2) - g0;
  const bool vec = ld == rank && e0 % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
  const u64 blocks = (n_groups + kInitThreads - 1) / kInitThreads;
  const dim3 grid((unsigned)std::min<u64>(blocks, kInitMaxBlocks)), block(kInitThreads);
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
  if (vec)
    hipLaunchKernelGGL((init_factors_kernel<T, true>), grid, block, 0, s, out, e0, e1, g0, n_groups, (unsigned)rank, (u64)ld,
                       (u64)row0, k0, k1, (unsigned)stream, scale, abs_values, ones_col);
  else
    hipLaunchKernelGGL((init_factors_kernel<T, false>), grid, block, 0, s, out, e0, e1, g0, n_groups, (unsigned)rank, (u64)ld,
                       (u64)row0, k0, k1, (unsigned)stream, scale, abs_values, ones_col);
  return hipGetLastError();
}
template hipError_t launch_init_factors<float>(uint64_t, int, int64_t, int, int, int64_t, double, int, int, float*, hipStream_t);
template hipError_t launch_init_factors<double>(uint64_t, int, int64_t, int, int, int64_t, double, int, int, double*, hipStream_t);

}  // namespace rsparse_hip
