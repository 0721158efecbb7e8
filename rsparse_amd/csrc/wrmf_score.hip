// Pointwise predictions at the stored positions of a sparse pattern -- the values of U V^T at the non-zeros of a template, what
// the reference's cpp_make_sparse_approximation computes (src/utils.cpp:4-56) -- and their squared / absolute error sums per row
// against given values.  gfx950, wave64, a sampled dense-dense product (SDDMM):
//   score[t] = add + sum_c U[row(t), c] * V[j[t], c]        U: n_rows x r, V: n_cols x r, row-major; (p, j): a CSR pattern
// Accumulated in DOUBLE in both instantiations: with fp32 factors every product of two floats is exact in double and only the sum
// rounds (the "double product" find_top_product orders by, R/utils.R:35-36); fp64 factors: a double dot with FMA.  `add` (the
// global bias) goes on once at the end (matrix_top_product.cpp:98-99).
//
// Launch 1, score_pairs_kernel: parallel over STORED POSITIONS, not rows -- row lengths run from 0 to more than 1e5 here, a wave
// per row waits for the longest row and wastes 60 lanes on rows of 1-3 entries (wrmf_f64.hip, "long rows").
//   * A lane group of G = pow2ceil(ceil(r / 4)) lanes holds one pair; lane l of the group owns the coordinates 4 l .. 4 l + 3:
//     one 16-byte load of the item vector with fp32 factors (two with fp64), so a group reads a row as one contiguous piece.
//     Ranks that are no multiple of 4 (rows not 16-byte aligned), or operands that are not 16-byte aligned themselves, take the
//     element-wise instantiation (VEC = false): no unaligned wide load anywhere.
//   * A wave walks a chunk of kWavePairs consecutive positions in steps of (64 / G) x kGroupPairs; a group takes kGroupPairs
//     consecutive positions per step and issues all their gathers before the first use (4 x 16 bytes in flight per lane).
//   * row(t): the wave finds the row of its chunk's first position with a 64-way search over p (one probe per lane and round: 4
//     rounds for a million rows); from there every group follows its own, ascending, positions -- a position past the end of the
//     current row gallops forward from it (the next row in the common case: one load).  p is 4 bytes per row against 4 r per
//     pair gathered and sits in L2.  The user vector is re-read per pair; neighbouring pairs share it from L1 / L2.
//   * The G partial sums (ascending coordinates inside a lane) are added by a butterfly over the group, distances G / 2 .. 1: an
//     order fixed by the lane numbers alone.  No atomics; the score of a position does not depend on how the launch was cut.
//   * The grid is what is resident at once (at most 8 workgroups per CU) and strides over the chunks: the number of stored
//     positions is p[n_rows], which only the device knows.
//   * A column index outside [0, n_cols) breaks the precondition: its score is NaN and nothing outside U and V is read for it.
// Launch 2, score_error_sums_kernel (only when sums are asked for): per row, sse = sum (score - actual)^2 and sae = sum |score -
// actual| over the stored scores.  A wave takes 64 consecutive rows: rows of at most kSumLaneMax entries are summed by their own
// lane in ascending position; longer rows one after the other by the whole wave (lane l: positions l, l + 64, ... ascending,
// then a butterfly).  Fixed order, independent of launch 1's shape; an empty row gets 0.
#include <algorithm>

#include "wrmf_csr_rows.h"
#include "wrmf_internal.h"
#include "wrmf_wave.h"

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kScoreThreads = 256;                   // 4 waves
constexpr int kGroupPairs = 4;                       // consecutive positions a lane group holds per step
constexpr int kWavePairs = 256;                      // positions per wave and chunk (a multiple of every step: 64 / G * 4 <= 256)
constexpr int kScoreChunk = kWavePairs * (kScoreThreads / 64);
constexpr int kScoreMaxPerCu = 8;                    // workgroups per CU at most (8 waves per SIMD)
constexpr int kSumLaneMax = 32;                      // launch 2: rows up to this long are summed by one lane

template <class T, int G, bool VEC>
__global__ __launch_bounds__(kScoreThreads) void score_pairs_kernel(const T* __restrict__ U, const T* __restrict__ V, int n_rows,
                                                                    int n_cols, int r, const int32_t* __restrict__ P,
                                                                    const int32_t* __restrict__ J, double add,
                                                                    double* __restrict__ out) {
  constexpr int kStep = (64 / G) * kGroupPairs;   // positions per wave and step
  const unsigned nnz = (unsigned)max(P[n_rows], 0);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int gi = lane / G, lig = lane % G, c0 = lig * 4;
  for (long long cb = (long long)blockIdx.x * kScoreChunk + (long long)w * kWavePairs; cb < (long long)nnz;
       cb += (long long)gridDim.x * kScoreChunk) {   // (whole waves: nothing below synchronises across waves)
    const unsigned tw = (unsigned)cb;
    int row = wave_find_row(P, n_rows, tw, lane);
    unsigned pend = (unsigned)P[row + 1];
    for (unsigned ts = tw; ts < tw + kWavePairs && ts < nnz; ts += kStep) {
      const unsigned t0 = ts + (unsigned)(gi * kGroupPairs);
      // a position at or past the end stands in for the last one (nnz > 0 here) and is not stored
      int j[kGroupPairs], rows[kGroupPairs];
#pragma unroll
      for (int q = 0; q < kGroupPairs; q++) j[q] = J[min(t0 + q, nnz - 1)];
#pragma unroll
      for (int q = 0; q < kGroupPairs; q++) {
        const unsigned t = min(t0 + q, nnz - 1);
        if (t >= pend) {
          row = find_row_from(P, n_rows, t, row);
          pend = (unsigned)P[row + 1];
        }
        rows[q] = row;
      }
      T u[kGroupPairs][4], v[kGroupPairs][4];
      bool ok[kGroupPairs];
#pragma unroll
      for (int q = 0; q < kGroupPairs; q++) {
        const T* urow = U + (size_t)rows[q] * r;
        ok[q] = (unsigned)j[q] < (unsigned)n_cols;
        load4<T, VEC>(ok[q] ? V + (size_t)j[q] * r : urow, c0, r, v[q]);   // (a bad index reads nothing outside U and V)
        load4<T, VEC>(urow, c0, r, u[q]);
      }
      double s[kGroupPairs];
#pragma unroll
      for (int q = 0; q < kGroupPairs; q++) {
        double acc = 0.0;
#pragma unroll
        for (int e = 0; e < 4; e++) acc = fma((double)u[q][e], (double)v[q][e], acc);
#pragma unroll
        for (int m = G >> 1; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
        s[q] = ok[q] ? acc + add : __longlong_as_double(0x7ff8000000000000ll);
      }
      if (lig == 0) {
#pragma unroll
        for (int q = 0; q < kGroupPairs; q++)
          if (t0 + q < nnz) out[t0 + q] = s[q];
      }
    }
  }
}

__global__ __launch_bounds__(kScoreThreads) void score_error_sums_kernel(const double* __restrict__ sc, const double* __restrict__ act,
                                                                         const int32_t* __restrict__ P, int n_rows,
                                                                         double* __restrict__ sse, double* __restrict__ sae) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long row0 = ((long long)blockIdx.x * (kScoreThreads / 64) + w) * 64;
  if (row0 >= n_rows) return;   // (whole waves)
  const int row = (int)row0 + lane;
  const bool in = row < n_rows;
  const int p0 = in ? P[row] : 0;
  const int len = in ? max(P[row + 1] - p0, 0) : 0;
  double s2 = 0.0, s1 = 0.0;
  if (len <= kSumLaneMax)
    for (int e = 0; e < len; e++) {
      const double d = sc[p0 + e] - act[p0 + e];
      s2 = fma(d, d, s2);
      s1 += fabs(d);
    }
  u64 longm = __ballot(len > kSumLaneMax);
  while (longm) {   // (wave-uniform)
    const int l = __builtin_ctzll(longm);
    longm &= longm - 1;
    const int q0 = __shfl(p0, l), n = __shfl(len, l);
    double a2 = 0.0, a1 = 0.0;
    for (int e = lane; e < n; e += 64) {
      const double d = sc[q0 + e] - act[q0 + e];
      a2 = fma(d, d, a2);
      a1 += fabs(d);
    }
    a2 = butterfly_sum(a2);
    a1 = butterfly_sum(a1);
    if (lane == l) {
      s2 = a2;
      s1 = a1;
    }
  }
  if (in) {
    if (sse) sse[row] = s2;
    if (sae) sae[row] = s1;
  }
}

// workgroups that are resident at once (the fp64 instantiations hold 8 gathers of 32 bytes per lane: 4-5 waves per SIMD, the
// fp32 ones 7-8): a larger grid would run its last workgroups alone after the others
template <class K>
int resident_grid(K kernel) {
  int per_cu = 0, dev = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kScoreThreads, 0) != hipSuccess || per_cu < 1) per_cu = 4;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      cus < 1)
    cus = 256;
  return std::min(per_cu, kScoreMaxPerCu) * cus;
}

template <class T, int G, bool VEC>
hipError_t launch_gv(const T* U, const T* V, int n_rows, int n_cols, int r, const int32_t* P, const int32_t* J, double add,
                     double* out, hipStream_t s) {
  static const int grid = resident_grid(score_pairs_kernel<T, G, VEC>);
  hipLaunchKernelGGL((score_pairs_kernel<T, G, VEC>), dim3((unsigned)grid), dim3(kScoreThreads), 0, s, U, V, n_rows, n_cols, r, P,
                     J, add, out);
  return hipGetLastError();
}

template <class T, int G>
hipError_t launch_g(bool vec, const T* U, const T* V, int n_rows, int n_cols, int r, const int32_t* P, const int32_t* J,
                    double add, double* out, hipStream_t s) {
  return vec ? launch_gv<T, G, true>(U, V, n_rows, n_cols, r, P, J, add, out, s)
             : launch_gv<T, G, false>(U, V, n_rows, n_cols, r, P, J, add, out, s);
}

}  // namespace

template <class T>
hipError_t launch_score_pairs(const T* U, const T* V, int n_rows, int n_cols, int r, const int32_t* P, const int32_t* J, double add,
                              double* scores, hipStream_t s) {
  if (n_rows <= 0) return hipSuccess;
  const bool vec = r % 4 == 0 && (reinterpret_cast<uintptr_t>(U) | reinterpret_cast<uintptr_t>(V)) % 16 == 0;
  const int quads = (r + 3) / 4;
  if (quads <= 1) return launch_g<T, 1>(vec, U, V, n_rows, n_cols, r, P, J, add, scores, s);
  if (quads <= 2) return launch_g<T, 2>(vec, U, V, n_rows, n_cols, r, P, J, add, scores, s);
  if (quads <= 4) return launch_g<T, 4>(vec, U, V, n_rows, n_cols, r, P, J, add, scores, s);
  if (quads <= 8) return launch_g<T, 8>(vec, U, V, n_rows, n_cols, r, P, J, add, scores, s);
  if (quads <= 16) return launch_g<T, 16>(vec, U, V, n_rows, n_cols, r, P, J, add, scores, s);
  if (quads <= 32) return launch_g<T, 32>(vec, U, V, n_rows, n_cols, r, P, J, add, scores, s);
  return launch_g<T, 64>(vec, U, V, n_rows, n_cols, r, P, J, add, scores, s);   // r <= 256
}
template hipError_t launch_score_pairs<float>(const float*, const float*, int, int, int, const int32_t*, const int32_t*, double,
                                              double*, hipStream_t);
template hipError_t launch_score_pairs<double>(const double*, const double*, int, int, int, const int32_t*, const int32_t*, double,
                                               double*, hipStream_t);

hipError_t launch_score_error_sums(const double* scores, const double* actual, const int32_t* P, int n_rows, double* sse,
                                   double* sae, hipStream_t s) {
  if (n_rows <= 0) return hipSuccess;
  const unsigned grid = (unsigned)(((long long)n_rows + kScoreThreads - 1) / kScoreThreads);
  hipLaunchKernelGGL(score_error_sums_kernel, dim3(grid), dim3(kScoreThreads), 0, s, scores, actual, P, n_rows, sse, sae);
  return hipGetLastError();
}

}  // namespace rsparse_hip
