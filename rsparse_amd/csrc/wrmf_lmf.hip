// Logistic matrix factorisation (Johnson 2014) by its EXACT full gradient -- no sampled negatives, no atomics; the definition is
// rsparse_amd/lmf.py in numpy, include/rsparse_wrmf_hip.h repeats it for C hosts; DESIGN.md 3.37.  gfx950, wave64, fp32 factors.
// One half-iteration over the rows A (n_rows x K) against the fixed side B (n_str x K), K <= 128, is two launches:
//
// Launch 1, lmf_dense_kernel<KT, SP, VEC>: D[r, :] = sum over ALL t of sigma(A[r] . B[t]) B[t, :] -- two chained dense products with
// the sigmoid between them, on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation), the n_rows x n_str scores never
// leaving the registers.  KT = ceil(K / 32), KP = 32 KT.
//   * Work split: a wave owns 32 rows of A, a workgroup of 4 waves 128; blockIdx.y is a SLICE of B's rows (below).  B is streamed
//     in tiles of 32 rows x KP columns, zero padded, staged in LDS with row stride KP + 1 (odd: both read patterns below are free
//     of bank conflicts) in two buffers: the global loads of tile i + 1 are issued before the products of tile i and written to
//     the other buffer after them -- one barrier per tile.  All four waves read every staged tile.
//   * First product, TRANSPOSED: S' = B_tile A_tile' (B's rows the M side, read from LDS as tile[lane % 32][2 kk + lane / 32]; A's
//     rows the N side, held in 16 KT registers for the whole launch: register kk of lane l = A[row(l % 32)][2 kk + l / 32]).  In the
//     accumulator layout of the 32 x 32 instruction lane l then holds A row l % 32 and register q the B rows
//     q % 4 + 8 (q / 4) + 4 (l / 32).
//   * Sigmoid in place on those 16 registers: v_exp_f32 and v_rcp_f32, 1 / (1 + 2^(-s log2 e)); the exponential's overflow to
//     +inf gives 0 and its underflow 1, no NaN at any finite s.
//   * Second product: register q AS IT STANDS is the N-side operand (k = l / 32, n = the A row) of one instruction per 32-column
//     block of D' (K x 32 rows); the M-side operand is B_tile' at the two B rows the register pair holds, read from the same LDS
//     tile as tile[q % 4 + 8 (q / 4) + 4 (l / 32)][32 cb + l % 32].  No shuffle, no LDS round trip of the probabilities.  D' stays
//     in 16 KT accumulator registers until the end of the stream; a lane then holds 4 consecutive coordinates per register quad
//     (one 16-byte store with VEC: K % 4 == 0 and aligned operands).
//   * SP adds, per row of A, sum_t softplus(s_rt) = max(s, 0) + log(1 + exp(-|s|)) (the dense part of the log-likelihood), each
//     term fp32, summed in DOUBLE; the zero rows that pad B's last tile would add log 2 each and are masked.
//   * Slices: when ceil(n_rows / 128) workgroups would leave the device idle, B's rows are cut into n_slices pieces of slice_rows
//     (a multiple of 32; lmf_plan: a function of n_rows and n_str alone, never of the device) and slice s writes its own fp32
//     partial D[s] (n_rows x K); the consumer adds them in ascending s.  No float atomics: a repeated call returns the same bits.
//   * Padded A rows are never stored; padded B rows and columns are zeros in LDS and add 0 to D.
//
// Launch 2, lmf_step_kernel<VEC, LL>: the sparse term and the update in one pass over the side's CSR (p, j, x), c = alpha x:
//     Sp[r, :] = sum over the stored t of c (1 - sigma(A[r] . B[j_t])) B[j_t, :],    g = Sp - sum_s D[s] - lambda A[r] (first `rank`
//     coordinates), g[frozen] = 0,    a' = a + g g,    A'[r, c] = A[r, c] + lr g / sqrt(a') where a' > 0 and g != 0
//   everything in DOUBLE registers (fp32 products are exact in double), one rounding into A.  A 16-lane group takes a row; a lane
//   owns 8 coordinates: with VEC 4 l .. 4 l + 3 and 64 + 4 l .. (16-byte gathers of B[j]), else l, l + 16, ... (4-byte gathers);
//   two entries' gathers are in flight per group.  The dot product is a butterfly over the group, an order fixed by the lane
//   numbers.  Rows longer than kLmfLongRow entries are not one group's serial walk: the 16 groups of the workgroup that holds the
//   row take its entries g, g + 16, ... and their partial sums are added through LDS in ascending g.  The row is updated in place
//   (row-local: no other row reads it in this launch).  LL writes the row's sum_stored (c s - c softplus(s)) minus its dense
//   softplus sums.  A column index outside [0, n_str) breaks the precondition: the row's gradient is NaN, nothing outside A and B
//   is read.  Built with -ffp-contract=off like the BPR files.
#include <algorithm>

#include "../../include/rsparse_wrmf_hip.h"
#include "wrmf_internal.h"
#include "wrmf_wave.h"

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kLmfThreads = 256;      // 4 waves
constexpr int kLmfRows = 128;         // rows of A per workgroup (32 per wave)
constexpr int kLmfTile = 32;          // rows of B per staged tile
constexpr int kLmfTargetGroups = 2048;   // lmf_plan slices B until the launch has about this many workgroups ...
constexpr int kLmfMinSliceTiles = 8;     // ... of at least this many tiles each
constexpr int kLmfMaxSlices = 64;
constexpr int kLmfStepRows = kLmfThreads / 16;   // rows per workgroup of the step kernel
constexpr float kLog2e = 1.44269504088896340736f, kLn2 = 0.69314718055994530942f;

// ---- launch 1 -------------------------------------------------------------------------------------------------------------------
// the global loads of one tile (rows t0 .. t0 + 31 of B below t_end, zeros elsewhere) into 4 KT registers per thread
template <int KT, bool VEC>
__device__ __forceinline__ void lmf_tile_load(const float* __restrict__ B, int K, int t0, int t_end, int tid, float (&st)[4 * KT]) {
  constexpr int KP = 32 * KT;
  if constexpr (VEC) {
#pragma unroll
    for (int i = 0; i < KT; i++) {
      const int e = tid + kLmfThreads * i, row = e / (KP / 4), c = 4 * (e % (KP / 4));
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t0 + row < t_end && c < K) v = *reinterpret_cast<const float4*>(B + (size_t)(t0 + row) * K + c);
      st[4 * i] = v.x; st[4 * i + 1] = v.y; st[4 * i + 2] = v.z; st[4 * i + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4 * KT; i++) {
      const int e = tid + kLmfThreads * i, row = e / KP, c = e % KP;
      st[i] = t0 + row < t_end && c < K ? B[(size_t)(t0 + row) * K + c] : 0.f;
    }
  }
}
template <int KT, bool VEC>
__device__ __forceinline__ void lmf_tile_store(float* buf, int tid, const float (&st)[4 * KT]) {
  constexpr int KP = 32 * KT, LD = KP + 1;
  if constexpr (VEC) {
#pragma unroll
    for (int i = 0; i < KT; i++) {
      const int e = tid + kLmfThreads * i, row = e / (KP / 4), c = 4 * (e % (KP / 4));
#pragma unroll
      for (int u = 0; u < 4; u++) buf[row * LD + c + u] = st[4 * i + u];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4 * KT; i++) {
      const int e = tid + kLmfThreads * i;
      buf[(e / KP) * LD + e % KP] = st[i];
    }
  }
}

template <int KT, bool SP, bool VEC>
__global__ __launch_bounds__(kLmfThreads) void lmf_dense_kernel(const float* __restrict__ A, int n_rows, const float* __restrict__ B,
                                                                int n_str, int K, int slice_rows, float* __restrict__ D,
                                                                double* __restrict__ softplus) {
  constexpr int KP = 32 * KT, LD = KP + 1;
  __shared__ float sB[2][kLmfTile * LD];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, ln = lane & 31, hi = lane >> 5;
  const int row = blockIdx.x * kLmfRows + wv * 32 + ln;
  const int t_begin = blockIdx.y * slice_rows, t_end = min(n_str, t_begin + slice_rows);   // (lmf_plan: t_begin < n_str)
  const int n_tiles = (t_end - t_begin + kLmfTile - 1) / kLmfTile;

  float st[4 * KT];
  lmf_tile_load<KT, VEC>(B, K, t_begin, t_end, tid, st);
  float a[16 * KT];   // the N-side operands of the first product
#pragma unroll
  for (int kk = 0; kk < 16 * KT; kk++) {
    const int c = 2 * kk + hi;
    a[kk] = row < n_rows && c < K ? A[(size_t)row * K + c] : 0.f;
  }
  f32x16 acc[KT];
#pragma unroll
  for (int cb = 0; cb < KT; cb++)
#pragma unroll
    for (int q = 0; q < 16; q++) acc[cb][q] = 0.f;
  double sp_sum = 0.0;
  lmf_tile_store<KT, VEC>(sB[0], tid, st);
  __syncthreads();

  for (int it = 0; it < n_tiles; it++) {
    const float* buf = sB[it & 1];
    const int t0 = t_begin + it * kLmfTile;
    const bool more = it + 1 < n_tiles;   // (uniform)
    if (more) lmf_tile_load<KT, VEC>(B, K, t0 + kLmfTile, t_end, tid, st);
    f32x16 s;
#pragma unroll
    for (int q = 0; q < 16; q++) s[q] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 16 * KT; kk++) s = __builtin_amdgcn_mfma_f32_32x32x2f32(buf[ln * LD + 2 * kk + hi], a[kk], s, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const float v = s[q];
      if constexpr (SP) {
        const float e = __builtin_amdgcn_exp2f(-fabsf(v) * kLog2e);
        const float term = fmaxf(v, 0.f) + kLn2 * __builtin_amdgcn_logf(1.f + e);
        if (t0 + (q & 3) + 8 * (q >> 2) + 4 * hi < t_end) sp_sum += (double)term;
      }
      s[q] = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-v * kLog2e));
    }
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const float* brow = buf + ((q & 3) + 8 * (q >> 2) + 4 * hi) * LD + ln;
#pragma unroll
      for (int cb = 0; cb < KT; cb++) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(brow[32 * cb], s[q], acc[cb], 0, 0, 0);
    }
    if (more) lmf_tile_store<KT, VEC>(sB[(it + 1) & 1], tid, st);   // (last read in iteration it - 1, before its barrier)
    __syncthreads();
  }

  if (row < n_rows) {
    float* out = D + ((size_t)blockIdx.y * n_rows + row) * K;
#pragma unroll
    for (int cb = 0; cb < KT; cb++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int c = 32 * cb + 8 * j + 4 * hi;
        if constexpr (VEC) {
          if (c < K) *reinterpret_cast<float4*>(out + c) = make_float4(acc[cb][4 * j], acc[cb][4 * j + 1], acc[cb][4 * j + 2], acc[cb][4 * j + 3]);
        } else {
#pragma unroll
          for (int u = 0; u < 4; u++)
            if (c + u < K) out[c + u] = acc[cb][4 * j + u];
        }
      }
  }
  if constexpr (SP) {
    sp_sum += __shfl_xor(sp_sum, 32);   // (both halves hold the row; whole waves get here)
    if (hi == 0 && row < n_rows) softplus[(size_t)blockIdx.y * n_rows + row] = sp_sum;
  }
}

template <int KT, bool SP>
hipError_t lmf_dense_kt(bool vec, dim3 grid, const float* A, int n_rows, const float* B, int n_str, int K, int slice_rows, float* D,
                        double* softplus, hipStream_t s) {
  if (vec)
    hipLaunchKernelGGL((lmf_dense_kernel<KT, SP, true>), grid, dim3(kLmfThreads), 0, s, A, n_rows, B, n_str, K, slice_rows, D, softplus);
  else
    hipLaunchKernelGGL((lmf_dense_kernel<KT, SP, false>), grid, dim3(kLmfThreads), 0, s, A, n_rows, B, n_str, K, slice_rows, D, softplus);
  return hipGetLastError();
}
template <bool SP>
hipError_t lmf_dense_sp(int KT, bool vec, dim3 grid, const float* A, int n_rows, const float* B, int n_str, int K, int slice_rows,
                        float* D, double* softplus, hipStream_t s) {
  switch (KT) {
    case 1: return lmf_dense_kt<1, SP>(vec, grid, A, n_rows, B, n_str, K, slice_rows, D, softplus, s);
    case 2: return lmf_dense_kt<2, SP>(vec, grid, A, n_rows, B, n_str, K, slice_rows, D, softplus, s);
    case 3: return lmf_dense_kt<3, SP>(vec, grid, A, n_rows, B, n_str, K, slice_rows, D, softplus, s);
    default: return lmf_dense_kt<4, SP>(vec, grid, A, n_rows, B, n_str, K, slice_rows, D, softplus, s);
  }
}

// ---- launch 2 -------------------------------------------------------------------------------------------------------------------
constexpr int kLmfLongRow = RSPARSE_HIP_LMF_LONG_ROW;

// coordinate i (< 8) of lane `lig` of a 16-lane group
template <bool VEC>
__device__ __forceinline__ int lmf_coord(int i, int lig) {
  return VEC ? 64 * (i >> 2) + 4 * lig + (i & 3) : 16 * i + lig;
}
template <bool VEC>
__device__ __forceinline__ void lmf_row_load(const float* __restrict__ src, int K, int lig, float (&v)[8]) {
  if constexpr (VEC) {
#pragma unroll
    for (int h = 0; h < 2; h++) {
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (64 * h + 4 * lig < K) x = *reinterpret_cast<const float4*>(src + 64 * h + 4 * lig);
      v[4 * h] = x.x; v[4 * h + 1] = x.y; v[4 * h + 2] = x.z; v[4 * h + 3] = x.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = 16 * i + lig < K ? src[16 * i + lig] : 0.f;
  }
}

__device__ __forceinline__ double lmf_softplus(double s) { return fmax(s, 0.0) + log1p(exp(-fabs(s))); }

// the entries first, first + stride, ... below end of one row: sp += c (1 - sigma) B[j], ll += c s - c softplus(s)
template <bool VEC, bool LL>
__device__ __forceinline__ void lmf_walk(const int32_t* __restrict__ J, const float* __restrict__ X, const float* __restrict__ B,
                                         const float* __restrict__ arow, int n_str, int K, int lig, double alpha, int first, int end,
                                         int stride, const double (&a)[8], double (&sp)[8], double& ll) {
#pragma unroll 1
  for (int e = first; e < end; e += 2 * stride) {
    const int e1 = e + stride;
    const bool two = e1 < end;   // (uniform over the group)
    const int j0 = J[e], j1 = J[two ? e1 : e];
    const float x0 = X[e], x1 = X[two ? e1 : e];
    const bool ok0 = (unsigned)j0 < (unsigned)n_str, ok1 = (unsigned)j1 < (unsigned)n_str;
    float b0[8], b1[8];
    lmf_row_load<VEC>(ok0 ? B + (size_t)j0 * K : arow, K, lig, b0);   // (a bad index reads nothing outside A and B)
    lmf_row_load<VEC>(ok1 ? B + (size_t)j1 * K : arow, K, lig, b1);
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      s0 += a[i] * (double)b0[i];
      s1 += a[i] * (double)b1[i];
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) {
      s0 += __shfl_xor(s0, m);
      s1 += __shfl_xor(s1, m);
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double c0 = alpha * (double)x0, c1 = alpha * (double)x1;
    const double w0 = ok0 ? c0 * (1.0 - 1.0 / (1.0 + exp(-s0))) : nan;
    const double w1 = !two ? 0.0 : ok1 ? c1 * (1.0 - 1.0 / (1.0 + exp(-s1))) : nan;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      sp[i] += w0 * (double)b0[i];
      if (two) sp[i] += w1 * (double)b1[i];
    }
    if constexpr (LL) {
      ll += c0 * s0 - c0 * lmf_softplus(s0);
      if (two) ll += c1 * s1 - c1 * lmf_softplus(s1);
    }
  }
}

// the gradient, the Adagrad state and the row from the finished sums of row `row`
template <bool VEC, bool LL>
__device__ __forceinline__ void lmf_finish(int row, int n_rows, int K, int rank, int frozen, int lig, double lr, double lambda,
                                           const float* __restrict__ D, int n_slices, const double* __restrict__ softplus,
                                           float* __restrict__ A, double* __restrict__ aA, double* __restrict__ rowsum,
                                           const double (&a)[8], const double (&sp)[8], double ll) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int c = lmf_coord<VEC>(i, lig);
    if (c >= K) continue;
    double d = 0.0;
#pragma unroll 1
    for (int s = 0; s < n_slices; s++) d += (double)D[((size_t)s * n_rows + row) * K + c];
    double g = sp[i] - d;
    if (c < rank) g -= lambda * a[i];
    if (c == frozen) g = 0.0;
    const size_t at = (size_t)row * K + c;
    const double st = aA[at] + g * g;
    aA[at] = st;
    if (st > 0.0 && g != 0.0) A[at] = (float)(a[i] + lr * g / sqrt(st));
  }
  if constexpr (LL) {
    if (lig == 0) {
      if (softplus)
#pragma unroll 1
        for (int s = 0; s < n_slices; s++) ll -= softplus[(size_t)s * n_rows + row];
      rowsum[row] = ll;
    }
  }
}

template <bool VEC, bool LL>
__global__ __launch_bounds__(kLmfThreads) void lmf_step_kernel(const int32_t* __restrict__ P, const int32_t* __restrict__ J,
                                                               const float* __restrict__ X, int n_rows, int n_str, double alpha,
                                                               float* __restrict__ A, double* __restrict__ aA,
                                                               const float* __restrict__ B, const float* __restrict__ D, int n_slices,
                                                               const double* __restrict__ softplus, int K, int rank, int frozen,
                                                               double lr, double lambda, double* __restrict__ rowsum) {
  __shared__ double sh[kLmfStepRows][129];   // a long row's partial sums per group: 128 coordinates and the log-likelihood
  const int gi = threadIdx.x >> 4, lig = threadIdx.x & 15;
  const int row0 = blockIdx.x * kLmfStepRows;
  // pass 0: every group its own row unless it is long; pass 1 + i: row row0 + i by the whole workgroup if it is long (uniform)
#pragma unroll 1
  for (int pass = 0; pass <= kLmfStepRows; pass++) {
    const bool lng = pass > 0;
    const int r = lng ? row0 + pass - 1 : row0 + gi;
    if (lng && r >= n_rows) break;
    const int p0 = r < n_rows ? P[r] : 0, len = r < n_rows ? P[r + 1] - p0 : 0;
    if (lng && len <= kLmfLongRow) continue;
    const bool act = r < n_rows && (lng || len <= kLmfLongRow);
    float af[8];
    double a[8], sp[8], ll = 0.0;
#pragma unroll
    for (int i = 0; i < 8; i++) a[i] = sp[i] = 0.0;
    if (act) {
      lmf_row_load<VEC>(A + (size_t)r * K, K, lig, af);
#pragma unroll
      for (int i = 0; i < 8; i++) a[i] = (double)af[i];
      lmf_walk<VEC, LL>(J, X, B, A + (size_t)r * K, n_str, K, lig, alpha, lng ? p0 + gi : p0, p0 + max(len, 0), lng ? kLmfStepRows : 1, a,
                        sp, ll);
    }
    if (lng) {
#pragma unroll
      for (int i = 0; i < 8; i++) sh[gi][lmf_coord<VEC>(i, lig)] = sp[i];
      if (lig == 0) sh[gi][128] = ll;
      __syncthreads();
      if (gi == 0) {   // (every group has read the row before the barrier; it is written only below)
#pragma unroll
        for (int i = 0; i < 8; i++) sp[i] = 0.0;
        ll = 0.0;
#pragma unroll 1
        for (int g = 0; g < kLmfStepRows; g++) {
#pragma unroll
          for (int i = 0; i < 8; i++) sp[i] += sh[g][lmf_coord<VEC>(i, lig)];
          ll += sh[g][128];
        }
      }
    }
    if (act && (!lng || gi == 0))
      lmf_finish<VEC, LL>(r, n_rows, K, rank, frozen, lig, lr, lambda, D, n_slices, softplus, A, aA, rowsum, a, sp, ll);
    if (lng) __syncthreads();
  }
}

}  // namespace

LmfPlan lmf_plan(int n_rows, int n_str, int slice_rows) {
  LmfPlan p;
  const long long tiles = ((long long)n_str + kLmfTile - 1) / kLmfTile;
  if (slice_rows <= 0) {
    const long long groups = std::max(1ll, ((long long)n_rows + kLmfRows - 1) / kLmfRows);
    const long long want = groups >= kLmfTargetGroups ? 1 : (kLmfTargetGroups + groups - 1) / groups;
    const long long n = std::max(1ll, std::min<long long>({want, (long long)kLmfMaxSlices, tiles / kLmfMinSliceTiles}));
    slice_rows = (int)(kLmfTile * ((tiles + n - 1) / n));
  }
  p.slice_rows = slice_rows;
  p.n_slices = (int)(((long long)n_str + slice_rows - 1) / slice_rows);
  return p;
}

hipError_t launch_lmf_dense(const float* A, int n_rows, const float* B, int n_str, int K, const LmfPlan& plan, float* D, double* softplus,
                            hipStream_t s) {
  if (n_rows <= 0 || n_str <= 0) return hipSuccess;
  const bool vec = K % 4 == 0 && (reinterpret_cast<uintptr_t>(B) | reinterpret_cast<uintptr_t>(D)) % 16 == 0;
  const dim3 grid((unsigned)((n_rows + kLmfRows - 1) / kLmfRows), (unsigned)plan.n_slices);
  const int KT = (K + 31) / 32;
  return softplus ? lmf_dense_sp<true>(KT, vec, grid, A, n_rows, B, n_str, K, plan.slice_rows, D, softplus, s)
                  : lmf_dense_sp<false>(KT, vec, grid, A, n_rows, B, n_str, K, plan.slice_rows, D, nullptr, s);
}

hipError_t launch_lmf_step(const int32_t* P, const int32_t* J, const float* X, int n_rows, int n_str, double alpha, float* A, double* aA,
                           const float* B, const float* D, int n_slices, const double* softplus, int K, int rank, int frozen, double lr,
                           double lambda, double* rowsum, hipStream_t s) {
  if (n_rows <= 0) return hipSuccess;
  const bool vec = K % 4 == 0 && (reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) % 16 == 0;
  const dim3 grid((unsigned)((n_rows + kLmfStepRows - 1) / kLmfStepRows));
#define RSPARSE_LMF_STEP(VEC, LL)                                                                                                    \
  hipLaunchKernelGGL((lmf_step_kernel<VEC, LL>), grid, dim3(kLmfThreads), 0, s, P, J, X, n_rows, n_str, alpha, A, aA, B, D, n_slices, \
                     softplus, K, rank, frozen, lr, lambda, rowsum)
  if (vec && rowsum) RSPARSE_LMF_STEP(true, true);
  else if (vec) RSPARSE_LMF_STEP(true, false);
  else if (rowsum) RSPARSE_LMF_STEP(false, true);
  else RSPARSE_LMF_STEP(false, false);
#undef RSPARSE_LMF_STEP
  return hipGetLastError();
}

}  // namespace rsparse_hip
