// One half-iteration of soft-ALS (soft_svd / soft_impute, R/SoftALS.R:68-102 with the `%*% diag(sqrt(d))` of :157,174) as ONE
// pass over a CSR matrix, where the reference makes three (cpp_make_sparse_approximation at the pattern, a subtraction, CSR x
// dense).  gfx950, wave64.  Per row of the pattern (P, J, X), M: n_cols x r and W: n_rows x r row-major:
//   res_t       = x_t - (w ? sum_c w_c W[row, c] M[j_t, c] : 0)
//   out[row, c] = s_c * sum_t res_t M[j_t, c]  +  (t ? t_c W[row, c] : 0)                  sumsq = sum_t res_t^2
// Every sum in DOUBLE in both instantiations (with fp32 operands every product is exact in double); one rounding at the store.
//
// Launch 1, softals_span_kernel: parallel over STORED POSITIONS (row lengths run from 0 to beyond 1e5; wrmf_score.hip).
//   * Wave `v` of the launch owns the SPAN of positions [v span, (v + 1) span): span = the positions per wave rounded up to
//     whole chunks of kChunk, at least kMinSpanChunks chunks.  It depends on the number of stored positions and on the grid
//     alone, so a row of more than kMinSpanChunks * kChunk entries is always cut between waves.
//   * A lane group of G = pow2ceil(ceil(r / 4)) lanes owns 4 G consecutive positions of every chunk; lane l of the group owns
//     the coordinates 4 l .. 4 l + 3: one 16-byte load of M[j_t] with fp32 operands (two with fp64), kGather of them issued
//     before the first use.  That ONE gather serves the dot product with the row's own factor (a butterfly over the group)
//     and, scaled by the residual, the accumulation.  Ranks that are no multiple of 4 and misaligned operands take the
//     element-wise instantiation (VEC = false).
//   * The row's own factor is loaded when a group enters a row -- once per row and group, not per position -- and handed from
//     position to position in registers; the same copy gives t o W at the store.  A step's four dot products are formed first
//     and their butterflies run side by side.
//   * Registers bound the gathers in flight (three waves per SIMD with the residual in fp32, four without): s and t are read
//     where a row is stored, the wave's running row lives in LDS.
//   * A row that lies inside one group's positions is stored by the group.  A row cut by a group boundary leaves its partial
//     sums in LDS (a group has at most two: the row it found begun, and the row it leaves unfinished); after the chunk the wave
//     adds them in ascending group order -- lane l now owns the coordinates 4 l .. of the whole row -- and carries an unfinished
//     row into its next chunk.  A row cut by a SPAN boundary leaves the wave's partial sum in the workspace.
// Launch 2, softals_finish_kernel: workgroup k looks at the boundary between the spans k - 1 and k.  If it cuts a row and is the
//   first boundary to do so, the workgroup adds that row's partial sums in ascending span order and stores the row.  Workgroup 0
//   adds the waves' sums of squared residuals, again in a fixed order.
// Launch 0, softals_empty_rows_kernel: rows without a stored position get t o W, or zeros.
// No atomics anywhere: the order of every sum is fixed by the pattern and the launch geometry, a repeated call returns the same
// bits.  A column outside [0, n_cols) makes the residual NaN -- and with it the row and the sum of squares -- and reads row 0.
#include <algorithm>

#include "../../include/rsparse_wrmf_hip.h"
#include "wrmf_csr_rows.h"
#include "wrmf_internal.h"
#include "wrmf_wave.h"

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kThreads = 256;                               // 4 waves
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = RSPARSE_HIP_SOFTALS_CHUNK;           // positions per wave and chunk: 4 G per lane group
constexpr int kMinSpanChunks = (RSPARSE_HIP_SOFTALS_SPLIT - 1) / RSPARSE_HIP_SOFTALS_CHUNK;
constexpr int kGather = 4;                                  // gathers a lane group issues before the first use
constexpr int kMaxPerCu = 8;                                // workgroups per CU at most
static_assert(kChunk == 256, "a chunk is 4 positions per lane: 64 / G groups of 4 G positions");
static_assert(kMinSpanChunks >= 1 && kMinSpanChunks * kChunk + 1 == RSPARSE_HIP_SOFTALS_SPLIT, "SPLIT = whole chunks + 1");

// positions per wave: the same in both launches
__device__ __forceinline__ long long span_of(long long nnz, int n_waves) {
  long long per = (nnz + n_waves - 1) / n_waves;
  per = (per + kChunk - 1) / kChunk * kChunk;
  return per > (long long)kMinSpanChunks * kChunk ? per : (long long)kMinSpanChunks * kChunk;
}

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// coef: w, s, t at strides of 256 doubles, zeros beyond r.  ws_ssq: one double per wave; ws_head / ws_tail: ld = 4 G doubles per
// wave, the partial sums of the row a span begins inside / ends inside
template <class T, int G, bool VEC, bool RES>
__global__ __launch_bounds__(kThreads) void softals_span_kernel(const int32_t* __restrict__ P, const int32_t* __restrict__ J,
                                                                const T* __restrict__ X, const T* __restrict__ M,
                                                                const T* __restrict__ W, int n_rows, int n_cols, int r,
                                                                const double* __restrict__ coef, int has_t, T* __restrict__ out,
                                                                double* __restrict__ ws_ssq, double* __restrict__ ws_head,
                                                                double* __restrict__ ws_tail) {
  constexpr int NG = 64 / G, S = 4 * G, LD = 4 * G;   // groups per wave; positions per group and chunk; padded rank
  __shared__ double s_acc[kWaves][2 * NG * LD];       // slot 2 g: the row group g found begun, 2 g + 1: the one it leaves unfinished
  __shared__ double s_own[kWaves][NG * LD];           // t o W of the rows in the odd slots
  __shared__ int s_row[kWaves][2 * NG];
  __shared__ double s_run[kWaves][2 * LD];            // the wave's running row across groups and chunks: its sums, its t o W
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int gi = lane / G, lig = lane % G, c0 = lig * 4;
  const long long nnz = max(P[n_rows], 0);
  const int n_waves = (int)gridDim.x * kWaves, wv = (int)blockIdx.x * kWaves + w;
  const long long span = span_of(nnz, n_waves);
  const long long b0l = (long long)wv * span;
  if (b0l >= nnz) {   // (whole waves; nothing below synchronises across waves)
    if (lane == 0) ws_ssq[wv] = 0.0;
    return;
  }
  const unsigned b0 = (unsigned)b0l, b1 = (unsigned)min(b0l + span, nnz);
  // w stays in registers (every position uses it); s and t are read where a row is stored: registers are what bounds the
  // number of gathers in flight here
  double wc[4];
#pragma unroll
  for (int e = 0; e < 4; e++) wc[e] = RES ? coef[c0 + e] : 0.0;
  const double* sm = coef + 256 + c0;
  const double* tc = coef + 512 + c0;
  double sr[4];   // (without the residual there is room: s stays in registers)
#pragma unroll
  for (int e = 0; e < 4; e++) sr[e] = RES ? 0.0 : sm[e];
  auto sc_at = [&](int e) { return RES ? sm[e] : sr[e]; };
  double* acc_s = s_acc[w];
  double* own_s = s_own[w];
  int* row_s = s_row[w];
  // the wave's running row across groups and chunks: lane l < G owns the coordinates 4 l .. 4 l + 3 (the same as in group 0)
  // (in LDS, not in registers: they would be live across the gather loop, where registers bound the gathers in flight)
  int cur_row = -1;
  double* run = s_run[w] + c0;
  double* own = s_run[w] + LD + c0;
  double ssq = 0.0;
  auto flush_wave = [&]() {   // cur_row is complete as far as this wave sees it
    const unsigned p0 = (unsigned)P[cur_row], p1 = (unsigned)P[cur_row + 1];
    if (lane < G) {
      if (p0 >= b0 && p1 <= b1) {
#pragma unroll
        for (int e = 0; e < 4; e++)
          if (c0 + e < r) out[(size_t)cur_row * r + c0 + e] = (T)fma(sc_at(e), run[e], own[e]);
      } else {
        double* dst = (p0 < b0 ? ws_head : ws_tail) + (size_t)wv * LD + c0;
#pragma unroll
        for (int e = 0; e < 4; e++) dst[e] = run[e];
      }
    }
  };

  for (unsigned cb = b0; cb < b1; cb += kChunk) {
    const int row_cb = wave_find_row(P, n_rows, cb, lane);
    const unsigned g0 = cb + (unsigned)(gi * S);
    const bool active = g0 < b1;
    const unsigned g1 = active ? min(g0 + (unsigned)S, b1) : b1;   // (an idle group walks the wave's last position, unused)
    const unsigned tlast = g1 - 1;
    int row = find_row_from(P, n_rows, min(g0, tlast), row_cb);
    unsigned pend = (unsigned)P[row + 1];
    const bool head0 = (unsigned)P[row] < g0;   // the first row began before this group's positions
    if (lig == 0) {
      row_s[2 * gi] = -1;
      row_s[2 * gi + 1] = -1;
    }
    int grow = -1, prev = -1;
    bool ghead = false;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    T wraw[4] = {T(0), T(0), T(0), T(0)}, wlast[4] = {T(0), T(0), T(0), T(0)};
    auto group_row_done = [&]() {   // the row `grow` ended inside this group's positions
      if (ghead) {
#pragma unroll
        for (int e = 0; e < 4; e++) acc_s[(2 * gi) * LD + c0 + e] = acc[e];
        if (lig == 0) row_s[2 * gi] = grow;
      } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
          if (c0 + e < r) out[(size_t)grow * r + c0 + e] = (T)fma(sc_at(e), acc[e], has_t ? tc[e] * (double)wraw[e] : 0.0);
      }
    };
#pragma unroll 1
    for (int st = 0; st < S / kGather; st++) {   // (the same count in every group: the butterflies below run converged)
      const unsigned ts = g0 + (unsigned)(st * kGather);
      int j[kGather], rows[kGather];
      T xv[kGather];
      bool valid[kGather], need[kGather];
#pragma unroll
      for (int q = 0; q < kGather; q++) {
        const unsigned t = min(ts + q, tlast);
        valid[q] = active && ts + q < g1;
        j[q] = J[t];
        xv[q] = X[t];
      }
#pragma unroll
      for (int q = 0; q < kGather; q++) {
        const unsigned t = min(ts + q, tlast);
        if (t >= pend) {
          row = find_row_from(P, n_rows, t, row);
          pend = (unsigned)P[row + 1];
        }
        rows[q] = row;
        need[q] = RES && row != prev;
        prev = row;
      }
      T m[kGather][4], wq[kGather][4];
      bool ok[kGather];
#pragma unroll
      for (int q = 0; q < kGather; q++) {
        ok[q] = (unsigned)j[q] < (unsigned)n_cols;
        load4<T, VEC>(M + (ok[q] ? (size_t)j[q] * r : (size_t)0), c0, r, m[q]);
      }
      double res[kGather];
      if constexpr (RES) {
        // the own factor of every position's row: loaded where the row changes, handed on otherwise (wlast: the last step's)
#pragma unroll
        for (int q = 0; q < kGather; q++) {
#pragma unroll
          for (int e = 0; e < 4; e++) wq[q][e] = q ? wq[q - 1][e] : wlast[e];
          if (need[q]) load4<T, VEC>(W + (size_t)rows[q] * r, c0, r, wq[q]);
        }
#pragma unroll
        for (int e = 0; e < 4; e++) wlast[e] = wq[kGather - 1][e];
        // the step's dot products first, their butterflies side by side: four round trips in flight, not one after the other
        double dot[kGather];
#pragma unroll
        for (int q = 0; q < kGather; q++) {
          dot[q] = 0.0;
#pragma unroll
          for (int e = 0; e < 4; e++) dot[q] = fma(wc[e] * (double)wq[q][e], (double)m[q][e], dot[q]);
        }
#pragma unroll
        for (int d = G >> 1; d >= 1; d >>= 1) {
#pragma unroll
          for (int q = 0; q < kGather; q++) dot[q] += __shfl_xor(dot[q], d);
        }
#pragma unroll
        for (int q = 0; q < kGather; q++) res[q] = (double)xv[q] - dot[q];
      } else {
#pragma unroll
        for (int q = 0; q < kGather; q++) res[q] = (double)xv[q];
      }
#pragma unroll
      for (int q = 0; q < kGather; q++) {
        if (valid[q] && rows[q] != grow) {
          if (grow >= 0) group_row_done();
          ghead = grow < 0 && head0;
          grow = rows[q];
#pragma unroll
          for (int e = 0; e < 4; e++) {
            acc[e] = 0.0;
            if constexpr (RES) wraw[e] = wq[q][e];
          }
        }
        const double rq = ok[q] ? res[q] : quiet_nan();
        if (valid[q]) {
#pragma unroll
          for (int e = 0; e < 4; e++) acc[e] = fma(rq, (double)m[q][e], acc[e]);
          if (lig == 0) ssq = fma(rq, rq, ssq);
        }
      }
    }
    if (grow >= 0) {   // the group's last row
      if (!ghead && (unsigned)P[grow + 1] > g1) {   // goes on behind the group's positions
#pragma unroll
        for (int e = 0; e < 4; e++) {
          acc_s[(2 * gi + 1) * LD + c0 + e] = acc[e];
          own_s[gi * LD + c0 + e] = has_t ? tc[e] * (double)wraw[e] : 0.0;
        }
        if (lig == 0) row_s[2 * gi + 1] = grow;
      } else {
        group_row_done();
      }
    }
    wave_sync();
    // the cut rows of the chunk, slots ascending (64 slots at a time: r <= 4 has 128)
#pragma unroll
    for (int base = 0; base < 2 * NG; base += 64) {
      const int slot_row = base + lane < 2 * NG ? row_s[base + lane] : -1;
      u64 slots = __ballot(slot_row >= 0);
      while (slots) {   // (wave-uniform)
        const int sb = __builtin_ctzll(slots), sl = base + sb;
        slots &= slots - 1;
        const int srow = __shfl(slot_row, sb);
        if (srow != cur_row) {
          if (cur_row >= 0) flush_wave();
          cur_row = srow;
          if (lane < G) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
              run[e] = 0.0;
              own[e] = (sl & 1) ? own_s[(sl >> 1) * LD + c0 + e] : 0.0;
            }
          }
        }
        if (lane < G) {
#pragma unroll
          for (int e = 0; e < 4; e++) run[e] += acc_s[sl * LD + c0 + e];
        }
      }
    }
    wave_sync();
  }
  if (cur_row >= 0) flush_wave();
  ssq = butterfly_sum(lig == 0 ? ssq : 0.0);
  if (lane == 0) ws_ssq[wv] = ssq;
}

// largest row with P[row] <= t, t < P[n_rows], by one thread
__device__ __forceinline__ int bisect_row(const int32_t* __restrict__ P, int n_rows, unsigned t) {
  int lo = 0, hi = n_rows;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((unsigned)P[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

template <class T>
__global__ __launch_bounds__(kThreads) void softals_finish_kernel(const int32_t* __restrict__ P, const T* __restrict__ W, int n_rows,
                                                                  int r, int ld, int n_waves, const double* __restrict__ coef,
                                                                  int has_t, const double* __restrict__ ws_ssq,
                                                                  const double* __restrict__ ws_head,
                                                                  const double* __restrict__ ws_tail, T* __restrict__ out,
                                                                  double* __restrict__ sumsq) {
  const int k = blockIdx.x, c = threadIdx.x;
  if (k == 0) {   // the waves' sums of squares: thread c adds the waves c, c + 256, ... ascending, then a tree over the threads
    if (!sumsq) return;
    __shared__ double sh[kThreads];
    double v = 0.0;
    for (int i = c; i < n_waves; i += kThreads) v += ws_ssq[i];
    sh[c] = v;
    __syncthreads();
    for (int st = kThreads / 2; st > 0; st >>= 1) {
      if (c < st) sh[c] += sh[c + st];
      __syncthreads();
    }
    if (c == 0) *sumsq = sh[0];
    return;
  }
  const long long nnz = max(P[n_rows], 0);
  const long long span = span_of(nnz, n_waves);
  const long long b0 = (long long)k * span;
  if (b0 >= nnz || c >= r) return;
  const int row = bisect_row(P, n_rows, (unsigned)b0);
  const long long p0 = P[row], p1 = P[row + 1];
  if (p0 == b0 || p0 < b0 - span) return;   // no row is cut here, or an earlier boundary cut it first
  double sum = ws_tail[(size_t)(k - 1) * ld + c];
  for (int m = k; m < n_waves && (long long)m * span < p1; m++) sum += ws_head[(size_t)m * ld + c];
  const double ownv = has_t ? coef[512 + c] * (double)W[(size_t)row * r + c] : 0.0;
  out[(size_t)row * r + c] = (T)fma(coef[256 + c], sum, ownv);
}

template <class T>
__global__ __launch_bounds__(kThreads) void softals_empty_rows_kernel(const int32_t* __restrict__ P, const T* __restrict__ W,
                                                                      int n_rows, int r, const double* __restrict__ coef, int has_t,
                                                                      T* __restrict__ out) {
  const long long row = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (row >= n_rows || P[row + 1] > P[row]) return;
  for (int c = 0; c < r; c++)
    out[(size_t)row * r + c] = has_t ? (T)(coef[512 + c] * (double)W[(size_t)row * r + c]) : T(0);
}

int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      cus < 1)
    cus = 256;
  return cus;
}

// workgroups that are resident at once (wrmf_score.hip): a larger grid would run its last workgroups alone after the others
template <class K>
int resident_grid(K kernel) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kThreads, 0) != hipSuccess || per_cu < 1) per_cu = 4;
  return std::min(per_cu, kMaxPerCu) * device_cus();
}

template <class T>
struct SpanArgs {
  const int32_t *P, *J;
  const T *X, *M, *W;
  int n_rows, n_cols, r;
  const double* coef;
  int has_t;
  T* out;
  double *ssq, *head, *tail;
};

template <class T, int G, bool VEC, bool RES>
hipError_t launch_span(const SpanArgs<T>& a, int& n_waves, hipStream_t s) {
  static const int grid = resident_grid(softals_span_kernel<T, G, VEC, RES>);
  n_waves = grid * kWaves;
  hipLaunchKernelGGL((softals_span_kernel<T, G, VEC, RES>), dim3((unsigned)grid), dim3(kThreads), 0, s, a.P, a.J, a.X, a.M, a.W,
                     a.n_rows, a.n_cols, a.r, a.coef, a.has_t, a.out, a.ssq, a.head, a.tail);
  return hipGetLastError();
}

template <class T, int G>
hipError_t launch_span_g(bool vec, bool res, const SpanArgs<T>& a, int& n_waves, hipStream_t s) {
  if (vec) return res ? launch_span<T, G, true, true>(a, n_waves, s) : launch_span<T, G, true, false>(a, n_waves, s);
  return res ? launch_span<T, G, false, true>(a, n_waves, s) : launch_span<T, G, false, false>(a, n_waves, s);
}

int group_lanes(int r) {
  int g = 1;
  while (4 * g < r) g <<= 1;
  return g;
}

}  // namespace

size_t softals_ws_doubles(int r) {
  const size_t waves = (size_t)kMaxPerCu * kWaves * device_cus();
  return 768 + waves * (1 + 2 * (size_t)4 * group_lanes(r));
}

template <class T>
hipError_t launch_softals_half(const int32_t* P, const int32_t* J, const T* X, const T* M, const T* W, int n_rows, int n_cols, int r,
                               bool res, bool has_t, T* out, double* sumsq, double* ws, hipStream_t s) {
  if (n_rows <= 0) return hipSuccess;
  const int G = group_lanes(r), ld = 4 * G;
  const size_t waves = (size_t)kMaxPerCu * kWaves * device_cus();
  const double* coef = ws;
  double* ssq = ws + 768;
  double* head = ssq + waves;
  double* tail = head + waves * ld;
  if (n_cols <= 0) M = reinterpret_cast<const T*>(coef);   // (every column is outside the matrix: row 0 of `coef` is what is read)
  const bool own = res || has_t;
  uintptr_t align = reinterpret_cast<uintptr_t>(M);
  if (own) align |= reinterpret_cast<uintptr_t>(W);
  const bool vec = r % 4 == 0 && align % 16 == 0 && n_cols > 0;
  const unsigned row_grid = (unsigned)(((long long)n_rows + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(softals_empty_rows_kernel<T>, dim3(row_grid), dim3(kThreads), 0, s, P, W, n_rows, r, coef, (int)has_t, out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const SpanArgs<T> a{P, J, X, M, W, n_rows, n_cols, r, coef, (int)has_t, out, ssq, head, tail};
  int n_waves = 0;
  switch (G) {
    case 1: e = launch_span_g<T, 1>(vec, own, a, n_waves, s); break;
    case 2: e = launch_span_g<T, 2>(vec, own, a, n_waves, s); break;
    case 4: e = launch_span_g<T, 4>(vec, own, a, n_waves, s); break;
    case 8: e = launch_span_g<T, 8>(vec, own, a, n_waves, s); break;
    case 16: e = launch_span_g<T, 16>(vec, own, a, n_waves, s); break;
    case 32: e = launch_span_g<T, 32>(vec, own, a, n_waves, s); break;
    default: e = launch_span_g<T, 64>(vec, own, a, n_waves, s); break;   // r <= 256
  }
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(softals_finish_kernel<T>, dim3((unsigned)n_waves), dim3(kThreads), 0, s, P, W, n_rows, r, ld, n_waves, coef,
                     (int)has_t, ssq, head, tail, out, sumsq);
  return hipGetLastError();
}
template hipError_t launch_softals_half<float>(const int32_t*, const int32_t*, const float*, const float*, const float*, int, int,
                                               int, bool, bool, float*, double*, double*, hipStream_t);
template hipError_t launch_softals_half<double>(const int32_t*, const int32_t*, const double*, const double*, const double*, int,
                                                int, int, bool, bool, double*, double*, double*, hipStream_t);

}  // namespace rsparse_hip
