// Why this item: the contributions of a user's interactions to the score of a target item (Hu, Koren and Volinsky, section 5; the
// `explain` of the `implicit` library).  gfx950, wave64.  The folded-in embedding solves A_u x_u = sum_t b_t y_{j_t} with
// A_u = B + d I + sum_t a_t y_{j_t} y_{j_t}^T over the row's non-zeros t, so that
//   score(u, i) = y_i . x_u = sum_t b_t (z . y_{j_t}),     A_u z = y_i                                   (A_u is symmetric)
// and term t is what the interaction with item j_t contributes.  a, b: per non-zero (implicit feedback: c - 1 and c; explicit: 1
// and r); B: r x r symmetric or absent; d = diag + diag_per_nnz * len(row).
//
// One workgroup of 4 waves per user that has a target; the kernel is templated on the element type, on the rank class KP (32 /
// 64 / 128: the rank padded by zero columns and a unit diagonal) and on VEC (16-byte gathers: rank a multiple of the 16-byte
// piece and 16-byte aligned factors; otherwise the element-wise instantiation, no unaligned wide load anywhere).
//   1. Assemble.  The lower triangle of A_u is cut into 16 x 17 / 2 = 136 tiles of TS x TS (TS = KP / 16); thread t < 136 owns
//      tile t (row-major over the tile rows) in registers from here to the end of the factorisation.  The row's factor vectors
//      pass through an LDS chunk of CH vectors (row stride KP + one 16-byte piece), gathered one chunk ahead into registers, so
//      that the gather of chunk c + 1 is in flight while chunk c is accumulated; a row of any length is a loop over chunks.  Every
//      element is one chain of FMAs in the row's order, started from B, d added once at the end: a repeat call gives the same bits.
//   2. Factor.  Blocked right-looking Cholesky on the register tiles, 16 steps of (diagonal tile: in-register Cholesky by its
//      owner; panel: each tile of the block column solved against it by its owner; trailing tiles: minus panel x panel^T), two
//      barriers per step.  A tile is written to LDS once, when it is final.  L lies in LDS as a lower triangle whose rows start
//      at multiples of 4 elements (row i at 4 (g + 1) (2 g + w), g = i / 4, w = i % 4): every run of a tile row is aligned for a
//      wide LDS read.  The panel reads are the only LDS traffic of the update: 2 TS^2 words per TS^3 FMAs.
//      A pivot that is not positive TO WORKING PRECISION -- d_j <= 2 r eps a_jj, a_jj the assembled diagonal entry: the size the
//      rounding of its own sum can reach -- sets the user's flag; every output of the user's pairs is then NaN.
//   3. Solve.  The user's targets are dealt to the 4 waves, one target per wave at a time.  z sits in registers (in double), element i on
//      lane i % 64; a forward and a backward substitution by columns, the solved element read from its lane (v_readlane) and
//      the column of L (forward) or its row (backward: contiguous) from LDS.
//   4. Contributions.  z goes to the wave's LDS slot; lane l takes the non-zeros l, l + 64, ... of the row: gathers the factor
//      vector once more (L2-resident), one dot product with z IN DOUBLE, times b.  contrib[out_p[q] + t] in the element type; total[q] in
//      double: every lane adds its own contributions in ascending position, then a butterfly over the wave -- a fixed order.
// A user with an empty row is not factored (explicit feedback: A_u = 0): totals 0, flag 0.  A user without targets is not touched.
// An item index outside [0, n_items) breaks the precondition: nothing outside V is read for it and what depends on it is NaN.
//
// LDS at KP = 128: float 33.0 KB triangle + 8.3 KB chunk (CH = 16) + 0.6 KB = 41.8 KB, double 66.0 + 8.1 (CH = 8) + 1.1 = 75.2
// KB; the wave slots of z alias the chunk.  Two workgroups per CU in both: in double the LDS allows no more, in float the
// registers (229 at KP = 128, the tile and the panel pieces of the update; LDS alone would take three).  No scratch.
#include <cmath>
#include <limits>

#include "wrmf_internal.h"
#include "wrmf_wave.h"

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kThreads = 256, kWaves = 4;
constexpr int kTiles = 136;   // 16 x 17 / 2

template <class T>
struct Ex {
  static constexpr int EV = 16 / (int)sizeof(T);   // elements per 16-byte piece
  static constexpr int CH = 64 / (int)sizeof(T);   // vectors per chunk: 16 (float), 8 (double)
};

// start of row i of the lower triangle whose rows are padded to multiples of 4 elements
__host__ __device__ constexpr int tri4(int i) { return 4 * ((i >> 2) + 1) * (2 * (i >> 2) + (i & 3)); }

// N consecutive elements from / to an address aligned to min(16, N sizeof(T)) bytes
template <class T, int N>
__device__ __forceinline__ void ld_run(const T* p, T (&v)[N]) {
  constexpr int B = N * (int)sizeof(T) >= 16 ? 16 : N * (int)sizeof(T);
  __builtin_memcpy(v, __builtin_assume_aligned(p, B), N * sizeof(T));
}
template <class T, int N>
__device__ __forceinline__ void st_run(T* p, const T (&v)[N]) {
  constexpr int B = N * (int)sizeof(T) >= 16 ? 16 : N * (int)sizeof(T);
  __builtin_memcpy(__builtin_assume_aligned(p, B), v, N * sizeof(T));
}

// the 16-byte piece of a factor row at column c0 (a multiple of EV), zeros at and beyond r; without a branch, so that the
// gathers of a step stay in flight together (a piece beyond the row reads the row's start and drops it)
template <class T, bool VEC>
__device__ __forceinline__ void load_piece(const T* __restrict__ row, int c0, int r, T (&x)[Ex<T>::EV]) {
  constexpr int EV = Ex<T>::EV;
  if constexpr (VEC) {
    const bool in = c0 < r;
    ld_run<T, EV>(row + (in ? c0 : 0), x);
#pragma unroll
    for (int e = 0; e < EV; e++) x[e] = in ? x[e] : T(0);
  } else {
#pragma unroll
    for (int e = 0; e < EV; e++) {
      const T v = row[min(c0 + e, r - 1)];
      x[e] = c0 + e < r ? v : T(0);
    }
  }
}

__device__ __forceinline__ float lane_value(float v, int l) { return readlane_f(v, l); }
__device__ __forceinline__ double lane_value(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

template <class T>
struct ExplainArgs {
  const T* V;
  int n_items, r;
  const T* base;
  double diag, diag_per_nnz;
  const int32_t* x_p;
  const int32_t* x_j;
  const T* wa;
  const T* wb;
  const int32_t* t_p;
  const int32_t* t_j;
  const int64_t* out_p;
  T* contrib;
  double* total;
  int32_t* flags;
};

template <class T, int KP, bool VEC>
__global__ __launch_bounds__(kThreads, 2) void explain_kernel(const ExplainArgs<T> a) {
  constexpr int EV = Ex<T>::EV, CH = Ex<T>::CH;
  constexpr int TS = KP / 16;          // tile edge
  constexpr int LD = KP + EV;          // chunk row stride
  constexpr int LPV = KP / EV;         // lanes that gather one vector
  constexpr int VPP = kThreads / LPV;  // vectors per pass of the workgroup
  constexpr int NQ = (CH + VPP - 1) / VPP;
  constexpr int EPL = KP >= 64 ? KP / 64 : 1;
  constexpr int MC = TS < EV ? TS : EV;   // panel columns per read of the trailing update
  static_assert(kWaves * KP <= CH * LD, "the wave slots of z alias the chunk");

  __shared__ __attribute__((aligned(16))) T sL[tri4(KP)];
  __shared__ __attribute__((aligned(16))) T sY[CH * LD];
  __shared__ T sInvD[KP];
  __shared__ T sWa[CH];
  __shared__ int sBad;

  const int u = blockIdx.x;
  const int tp0 = a.t_p[u], tp1 = a.t_p[u + 1];
  if (tp1 <= tp0) return;   // no target: nothing of this user is touched
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int p0 = a.x_p[u], len = max(a.x_p[u + 1] - p0, 0);
  const int r = a.r;
  const T nan = std::numeric_limits<T>::quiet_NaN();
  if (len == 0) {   // nothing to factor: empty segments, totals 0
    for (int q = tp0 + tid; q < tp1; q += kThreads) a.total[q] = 0.0;
    if (tid == 0) a.flags[u] = 0;
    return;
  }
  if (tid == 0) sBad = 0;

  // ---------------- 1. assemble ----------------
  int ti = 0, tj = 0;
  const bool owner = tid < kTiles;
  if (owner) tile_of(tid, ti, tj);
  const int row0 = ti * TS, col0 = tj * TS;
  T acc[TS][TS];   // starts from B (zero without one) and the identity of the padding; d I goes on after the row's sum
#pragma unroll
  for (int i = 0; i < TS; i++)
#pragma unroll
    for (int j = 0; j < TS; j++) {
      const int gi = row0 + i, gj = col0 + j;
      const bool in = owner && gi < r && gj < r;
      acc[i][j] = (in && a.base) ? a.base[(size_t)gi * r + gj] : ((gi == gj && gi >= r) ? T(1) : T(0));
    }
  const int c4 = tid % LPV, v0 = tid / LPV;
  T pre[NQ][EV];
  T wa_pre = T(0);
  auto fetch = [&](int at, int cnt) {   // the chunk of `cnt` non-zeros from position `at` of the row, into registers
    int ids[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) ids[q] = a.x_j[p0 + at + min(q * VPP + v0, cnt - 1)];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const bool inr = (unsigned)ids[q] < (unsigned)a.n_items;
      load_piece<T, VEC>(a.V + (size_t)(inr ? ids[q] : 0) * r, c4 * EV, r, pre[q]);
    }
    if (tid < CH) {
      const int e = p0 + at + min(tid, cnt - 1);
      wa_pre = (unsigned)a.x_j[e] < (unsigned)a.n_items ? a.wa[e] : nan;
    }
  };
  fetch(0, min(CH, len));
  for (int at = 0; at < len; at += CH) {
    const int cnt = min(CH, len - at);
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const int v = q * VPP + v0;
      if (v < CH) st_run<T, EV>(sY + v * LD + c4 * EV, pre[q]);   // (vectors at and beyond cnt: copies of the last, not read)
    }
    if (tid < CH) sWa[tid] = wa_pre;
    __syncthreads();
    if (at + CH < len) fetch(at + CH, min(CH, len - at - CH));
    if (owner) {
      for (int c = 0; c < cnt; c++) {
        const T w = sWa[c];
        T yi[TS], yj[TS];
        ld_run<T, TS>(sY + c * LD + row0, yi);
        ld_run<T, TS>(sY + c * LD + col0, yj);
#pragma unroll
        for (int i = 0; i < TS; i++) {
          const T wy = w * yi[i];
#pragma unroll
          for (int j = 0; j < TS; j++) acc[i][j] = fma(wy, yj[j], acc[i][j]);
        }
      }
    }
    __syncthreads();
  }

  {   // + d I, once, on top of the row's sum: the row's small terms are not added one by one to a large start
    const T d = (T)(a.diag + a.diag_per_nnz * (double)len);
#pragma unroll
    for (int i = 0; i < TS; i++)
      if (row0 + i == col0 + i && row0 + i < r) acc[i][i] += d;
  }

  // ---------------- 2. factor ----------------
  T dorig[TS];
#pragma unroll
  for (int i = 0; i < TS; i++) dorig[i] = acc[i][i];   // (read by the owners of the diagonal tiles only)
  const T tol = (T)(2.0 * (double)r) * std::numeric_limits<T>::epsilon();
  for (int kb = 0; kb < 16; kb++) {
    if (owner && ti == kb && tj == kb) {   // the diagonal tile, in registers
      bool bad = false;
#pragma unroll
      for (int c = 0; c < TS; c++) {
        const T d = acc[c][c];
        bad = bad || !(d > tol * dorig[c]);
        const T s = sqrt(d), inv = T(1) / s;
        acc[c][c] = s;
        sInvD[row0 + c] = inv;
#pragma unroll
        for (int i = c + 1; i < TS; i++) acc[i][c] *= inv;
#pragma unroll
        for (int i = c + 1; i < TS; i++)
#pragma unroll
          for (int j = c + 1; j <= i; j++) acc[i][j] = fma(-acc[i][c], acc[j][c], acc[i][j]);
      }
#pragma unroll
      for (int i = 0; i < TS; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) sL[tri4(row0 + i) + col0 + j] = acc[i][j];
      if (bad) sBad = 1;
    }
    __syncthreads();
    if (owner && tj == kb && ti > kb) {   // the panel: X L_kk^T = A_ik, row by row
      T lkk[TS][TS], invd[TS];
#pragma unroll
      for (int c = 0; c < TS; c++) {
        invd[c] = sInvD[col0 + c];
#pragma unroll
        for (int m = 0; m < c; m++) lkk[c][m] = sL[tri4(col0 + c) + col0 + m];
      }
#pragma unroll
      for (int i = 0; i < TS; i++) {   // (a row at a time, stored as soon as it is solved: the rows are independent)
#pragma unroll
        for (int c = 0; c < TS; c++) {
          T v = acc[i][c];
#pragma unroll
          for (int m = 0; m < c; m++) v = fma(-acc[i][m], lkk[c][m], v);
          acc[i][c] = v * invd[c];
        }
        st_run<T, TS>(sL + tri4(row0 + i) + col0, acc[i]);
      }
    }
    __syncthreads();
    if (owner && tj > kb) {   // the trailing tiles: minus (block row ti of the panel) x (block row tj)^T
#pragma unroll 1   // (unrolled, every read of the panel is hoisted to the top and the tile spills)
      for (int m0 = 0; m0 < TS; m0 += MC) {
        T li[TS][MC], lj[TS][MC];
#pragma unroll
        for (int i = 0; i < TS; i++) {
          ld_run<T, MC>(sL + tri4(row0 + i) + kb * TS + m0, li[i]);
          ld_run<T, MC>(sL + tri4(col0 + i) + kb * TS + m0, lj[i]);
        }
#pragma unroll
        for (int i = 0; i < TS; i++)
#pragma unroll
          for (int j = 0; j < TS; j++)
#pragma unroll
            for (int m = 0; m < MC; m++) acc[i][j] = fma(-li[i][m], lj[j][m], acc[i][j]);
      }
    }
  }
  __syncthreads();
  if (sBad) {   // (workgroup-uniform) not positive definite: NaN to every output of the user's pairs
    for (int q = tp0 + wv; q < tp1; q += kWaves) {
      const size_t o = (size_t)a.out_p[q];
      for (int t = lane; t < len; t += 64) a.contrib[o + t] = nan;
      if (lane == 0) a.total[q] = std::numeric_limits<double>::quiet_NaN();
    }
    if (tid == 0) a.flags[u] = 1;
    return;
  }
  if (tid == 0) a.flags[u] = 0;

  // ---------------- 3. + 4. per target: solve, contributions ----------------
  // (the substitutions run in double in both instantiations: L is what the element type made it, but the two sweeps add no
  // rounding of their own at the element type's size -- z meets y_j in a dot product whose terms largely cancel)
  double dinv[EPL];
#pragma unroll
  for (int s = 0; s < EPL; s++) {
    const int i = s * 64 + lane;
    if constexpr (sizeof(T) == 8) dinv[s] = i < KP ? sInvD[i] : 1.0;   // (the factorisation's own reciprocals)
    else dinv[s] = i < KP ? 1.0 / (double)sL[tri4(i) + i] : 1.0;
  }
  T* sZ = sY + wv * KP;
  for (int q = tp0 + wv; q < tp1; q += kWaves) {   // (whole waves)
    const int item = a.t_j[q];
    const bool item_ok = (unsigned)item < (unsigned)a.n_items;
    double x[EPL];
#pragma unroll
    for (int s = 0; s < EPL; s++) {
      const int i = s * 64 + lane;
      x[s] = i < r ? (item_ok ? (double)a.V[(size_t)item * r + i] : (double)nan) : 0.0;
    }
    // L w = y: column j once w_j is known
#pragma unroll 2
    for (int j = 0; j < r; j++) {
      const int sj = j >> 6, lj = j & 63;
      double t = x[0] * dinv[0];
      if constexpr (EPL == 2) t = sj ? x[1] * dinv[1] : t;
      const double w = lane_value(t, lj);
#pragma unroll
      for (int s = 0; s < EPL; s++) {
        const int i = s * 64 + lane;
        const double l = (i > j && i < r) ? (double)sL[tri4(i) + j] : 0.0;
        x[s] = (i == j) ? w : fma(-l, w, x[s]);
      }
    }
    // L^T z = w: row i once z_i is known
#pragma unroll 2
    for (int i = r - 1; i >= 0; i--) {
      const int si = i >> 6, li = i & 63;
      double t = x[0] * dinv[0];
      if constexpr (EPL == 2) t = si ? x[1] * dinv[1] : t;
      const double z = lane_value(t, li);
      const T* rowL = sL + tri4(i);
#pragma unroll
      for (int s = 0; s < EPL; s++) {
        const int j = s * 64 + lane;
        const double l = j < i ? (double)rowL[j] : 0.0;
        x[s] = (j == i) ? z : fma(-l, z, x[s]);
      }
    }
#pragma unroll
    for (int s = 0; s < EPL; s++)
      if (s * 64 + lane < KP) sZ[s * 64 + lane] = (T)x[s];   // (zeros at and beyond r)
    wave_sync();
    const size_t o = (size_t)a.out_p[q];
    double tot = 0.0;
    for (int t0 = 0; t0 < len; t0 += 64) {
      const int t = t0 + lane;
      const bool ok = t < len;
      const int e = p0 + min(t, len - 1);
      const int j = a.x_j[e];
      const bool inr = (unsigned)j < (unsigned)a.n_items;
      const T* yrow = a.V + (size_t)(inr ? j : 0) * r;
      double d4[EV];   // in double, as the scores of wrmf_score.hip: a product of two floats is exact, only the sum rounds
#pragma unroll
      for (int k = 0; k < EV; k++) d4[k] = 0.0;
#pragma unroll 4
      for (int c0 = 0; c0 < r; c0 += EV) {
        T y[EV], z[EV];
        load_piece<T, VEC>(yrow, c0, r, y);
        ld_run<T, EV>(sZ + c0, z);
#pragma unroll
        for (int k = 0; k < EV; k++) d4[k] = fma((double)y[k], (double)z[k], d4[k]);
      }
      double dot = d4[0] + d4[1];
      if constexpr (EV == 4) dot += d4[2] + d4[3];
      const T c = inr ? (T)((double)a.wb[e] * dot) : nan;
      if (ok) {
        a.contrib[o + t] = c;
        tot += (double)c;
      }
    }
    tot = butterfly_sum(tot);
    if (lane == 0) a.total[q] = tot;
    wave_sync();   // the slot is rewritten for the wave's next target
  }
}

template <class T, int KP>
hipError_t launch_kp(bool vec, const ExplainArgs<T>& a, int n_users, hipStream_t s) {
  if (vec) hipLaunchKernelGGL((explain_kernel<T, KP, true>), dim3((unsigned)n_users), dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL((explain_kernel<T, KP, false>), dim3((unsigned)n_users), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace

template <class T>
hipError_t launch_explain(const T* V, int n_items, int r, const T* base, double diag, double diag_per_nnz, int n_users,
                          const int32_t* x_p, const int32_t* x_j, const T* wa, const T* wb, const int32_t* t_p, const int32_t* t_j,
                          const int64_t* out_p, T* contrib, double* total, int32_t* flags, hipStream_t s) {
  if (n_users <= 0) return hipSuccess;
  const ExplainArgs<T> a{V, n_items, r, base, diag, diag_per_nnz, x_p, x_j, wa, wb, t_p, t_j, out_p, contrib, total, flags};
  const bool vec = r % Ex<T>::EV == 0 && reinterpret_cast<uintptr_t>(V) % 16 == 0;
  if (r <= 32) return launch_kp<T, 32>(vec, a, n_users, s);
  if (r <= 64) return launch_kp<T, 64>(vec, a, n_users, s);
  return launch_kp<T, 128>(vec, a, n_users, s);   // r <= 128
}
template hipError_t launch_explain<float>(const float*, int, int, const float*, double, double, int, const int32_t*, const int32_t*,
                                          const float*, const float*, const int32_t*, const int32_t*, const int64_t*, float*, double*,
                                          int32_t*, hipStream_t);
template hipError_t launch_explain<double>(const double*, int, int, const double*, double, double, int, const int32_t*,
                                           const int32_t*, const double*, const double*, const int32_t*, const int32_t*,
                                           const int64_t*, double*, double*, int32_t*, hipStream_t);

}  // namespace rsparse_hip
