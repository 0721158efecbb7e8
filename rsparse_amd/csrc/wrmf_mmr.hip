// Greedy Maximal-Marginal-Relevance re-ranking of a pool of N ranked positions per user down to k.  gfx950, wave64.  The
// definition is the numpy statement `mmr_reference` of rsparse_amd/metrics.py: with u_i = V[item_i, c0:c1) inv_i
// (the zero vector for a degenerate item) and rel_i the scores of the valid positions brought into [0, 1], step t picks the valid,
// untaken position that maximises (1 - theta) rel_i - theta max_{j picked} <u_i, u_j>, the lower position winning a tie.
//
//   mmr_kernel   one workgroup of 256 threads per user, k dependent steps.  In LDS for the whole call: lead_i = (1 - theta) rel_i
//                (kGone for a position that is invalid or taken: the flag) and the running maximum similarity, one double each
//                per position, and the unit row of the item just picked as r doubles.  A step: the 256 / G lane groups (G = the
//                power of two >= r / 4, four consecutive coordinates per lane) walk the open positions round-robin, kMmrAhead
//                rows per group in flight, and form <u_i, u_pick> as fma((double)v inv_i, p, .) over a lane's four coordinates
//                followed by a fixed xor-butterfly over the G lanes -- every lane of a group ends with the same bits, and they
//                depend on the row, its inverse norm and the picked row alone, not on the position, the group or the workgroup.
//                The group updates the maximum, evaluates the objective and keeps its best (value, position); a shuffle
//                reduction over the wave and one over the four waves through LDS give the pick, the position deciding a tie at
//                every level.  Step 0 needs no dot products (the maximum over nothing is 0): 256 threads scan lead_i.
//                The rows are gathered from the factors AS STORED in every step (16-byte loads when the rows are 16-byte
//                aligned, scalar otherwise: a window that starts at the bias column, odd ranks), the items of the next batch
//                read while the rows of this one are in flight.  A form that copied the pool's rows into LDS once was built and
//                measured slower at the pool it fits; it is not here.
// No atomics; a repeated call returns the same bits.  LDS: 16 N + 2144 bytes.
#include <hip/hip_runtime.h>

#include "wrmf_internal.h"
#include "wrmf_device.h"

// the objective is the definition's two roundings, (1 - theta) rel - theta m: no contraction into a fused multiply-add
#pragma clang fp contract(off)

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kMmrThreads = 256;
constexpr int kMmrWaves = kMmrThreads / 64;
constexpr int kMmrAhead = 4;                    // rows a lane group has in flight before the first of them is used
constexpr int kMmrMaxPool = 8192;               // RSPARSE_HIP_MAX_TOPK_LARGE
constexpr int kMmrFixedBytes = 256 * 8 + 96;    // the picked row, the waves' candidates and the row's extremes
constexpr int kNaInteger = INT32_MIN;           // RSPARSE_HIP_NA_INTEGER
constexpr double kGone = -1.0;                  // lead_i of a position that is invalid or taken (a live one lies in [0, 1])

__device__ __forceinline__ double nan_f64() { return __longlong_as_double(0x7ff8000000000000ll); }

// four consecutive elements at p as they are stored; `valid` (1 .. 4) of them exist, the others read as zero
template <typename T, bool VEC>
__device__ __forceinline__ void load4_raw(const T* __restrict__ p, int valid, T x[4]) {
  if (VEC && valid >= 4) {
    if constexpr (sizeof(T) == 4) {
      const float4 v = *reinterpret_cast<const float4*>(p);
      x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
      const double2 a = *reinterpret_cast<const double2*>(p);
      const double2 b = *reinterpret_cast<const double2*>(p + 2);
      x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; e++) x[e] = e < valid ? p[e] : (T)0;
  }
}

// <u, p> over the G lanes of a group: this lane's four coordinates, then the butterfly (a + b == b + a: the same bits in every
// lane).  x: the row as stored, iv its inverse norm, p the picked unit row at the same coordinates.
template <typename T, int G>
__device__ __forceinline__ double group_dot(const T x[4], double iv, const double p[4]) {
  double d = 0.0;
#pragma unroll
  for (int e = 0; e < 4; e++) d = fma((double)x[e] * iv, p[e], d);
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, G);
  return d;
}

// (value, position): the larger value, the lower position among equal values
__device__ __forceinline__ void take_better(double& v, int& p, double ov, int op) {
  if (ov > v || (ov == v && op < p)) {
    v = ov;
    p = op;
  }
}

template <typename T, int G, bool VEC>
__global__ void __launch_bounds__(kMmrThreads)
mmr_kernel(const int32_t* __restrict__ lists, const double* __restrict__ scores, int N, int k, double theta,
           const T* __restrict__ V, int n_items, int64_t ld, int c0, int r, const double* __restrict__ inv,
           int32_t* __restrict__ out_items, double* __restrict__ out_scores, int32_t* __restrict__ out_pos,
           double* __restrict__ out_obj) {
  constexpr int NGRP = kMmrThreads / G;   // lane groups of the workgroup
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* sLead = reinterpret_cast<double*>(smem);   // [N]
  double* sMax = sLead + N;                          // [N]
  double* sPick = sMax + N;                          // [256]: the picked unit row, zero beyond r
  double* sRedV = sPick + 256;                       // [4] a wave's best value (setup: its smallest score)
  double* sRedW = sRedV + kMmrWaves;                 // [4] setup: a wave's largest score
  int* sRedI = reinterpret_cast<int*>(sRedW + kMmrWaves);   // [4] a wave's best position (+ 4 ints of padding)

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int gid = tid / G, gl = tid % G, j0 = 4 * gl;
  const int nco = min(4, r - j0);   // coordinates of this lane; <= 0: none
  const size_t u = blockIdx.x;
  const int32_t* lrow = lists + u * (size_t)N;
  const double* srow = scores + u * (size_t)N;
  const T* Vw = V + c0;             // row 0 of the window: what a lane without an open position reads and drops

  // ---- the row's extremes over its valid positions ----
  double lo = INFINITY, hi = -INFINITY;
  for (int i = tid; i < N; i += kMmrThreads) {
    const int32_t c = lrow[i];
    const double s = srow[i];
    if (c != kNaInteger && c >= 1 && c <= n_items && s - s == 0.0) {   // (s - s: NaN for a NaN or an infinite score)
      lo = fmin(lo, s);
      hi = fmax(hi, s);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, o));
    hi = fmax(hi, __shfl_xor(hi, o));
  }
  if (lane == 0) {
    sRedV[w] = lo;
    sRedW[w] = hi;
  }
  __syncthreads();
  lo = fmin(fmin(sRedV[0], sRedV[1]), fmin(sRedV[2], sRedV[3]));
  hi = fmax(fmax(sRedW[0], sRedW[1]), fmax(sRedW[2], sRedW[3]));
  const double span = hi - lo, omt = 1.0 - theta;
  for (int i = tid; i < N; i += kMmrThreads) {
    const int32_t c = lrow[i];
    const double s = srow[i];
    const bool ok = c != kNaInteger && c >= 1 && c <= n_items && s - s == 0.0;
    const double rel = hi != lo ? (s - lo) / span : 0.0;
    sLead[i] = ok ? omt * rel : kGone;
    sMax[i] = -INFINITY;
  }
  __syncthreads();   // (also: the extremes are read before the first step writes its candidates over them)

  int t = 0;
  for (; t < k; t++) {
    double bv = -INFINITY;
    int bp = INT32_MAX;
    if (t == 0) {   // nothing is picked: the objective is lead_i
      for (int i = tid; i < N; i += kMmrThreads) {
        const double a = sLead[i];
        if (a != kGone && a > bv) {
          bv = a;
          bp = i;
        }
      }
    } else {
      double p[4];
#pragma unroll
      for (int e = 0; e < 4; e++) p[e] = sPick[j0 + e];
      // every lane of the workgroup makes the same number of passes (the shuffles below run with all lanes present)
      int32_t nxt[kMmrAhead];
#pragma unroll
      for (int q = 0; q < kMmrAhead; q++) {
        const int i = q * NGRP + gid;
        nxt[q] = i < N ? lrow[i] : kNaInteger;
      }
      for (int base = 0; base < N; base += NGRP * kMmrAhead) {
        T x[kMmrAhead][4];
        double iv[kMmrAhead], a[kMmrAhead];
#pragma unroll
        for (int q = 0; q < kMmrAhead; q++) {   // every load of the batch before the first use
          const int i = base + q * NGRP + gid;
          a[q] = i < N ? sLead[i] : kGone;
          const int32_t c = nxt[q];
          const bool open = a[q] != kGone && c >= 1 && c <= n_items;
          if (!open) a[q] = kGone;
          iv[q] = open ? inv[c - 1] : 0.0;
          if (nco > 0)
            load4_raw<T, VEC>(open ? V + (int64_t)(c - 1) * ld + c0 + j0 : Vw + j0, nco, x[q]);
          else
            x[q][0] = x[q][1] = x[q][2] = x[q][3] = (T)0;
        }
#pragma unroll
        for (int q = 0; q < kMmrAhead; q++) {   // the items of the next batch
          const int i = base + NGRP * kMmrAhead + q * NGRP + gid;
          nxt[q] = i < N ? lrow[i] : kNaInteger;
        }
#pragma unroll
        for (int q = 0; q < kMmrAhead; q++) {
          const int i = base + q * NGRP + gid;
          const bool open = a[q] != kGone;
          const bool use = open && iv[q] != 0.0;   // (a dropped or degenerate row may hold anything: not 0 * x)
#pragma unroll
          for (int e = 0; e < 4; e++) x[q][e] = use ? x[q][e] : (T)0;
          const double d = group_dot<T, G>(x[q], iv[q], p);
          if (open) {
            const double m = fmax(sMax[i], d);
            if (gl == 0) sMax[i] = m;
            const double obj = a[q] - theta * m;
            if (obj > bv) {   // (a group meets its positions in ascending order)
              bv = obj;
              bp = i;
            }
          }
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(bv, o);
      const int op = __shfl_xor(bp, o);
      take_better(bv, bp, ov, op);
    }
    if (lane == 0) {
      sRedV[w] = bv;
      sRedI[w] = bp;
    }
    __syncthreads();
    bv = sRedV[0];
    bp = sRedI[0];
#pragma unroll
    for (int q = 1; q < kMmrWaves; q++) take_better(bv, bp, sRedV[q], sRedI[q]);
    if (bp == INT32_MAX) break;   // no valid position is left (the same in every thread)
    const int32_t item = lrow[bp];
    if (tid == 0) {
      const size_t o = u * (size_t)k + t;
      out_items[o] = item;
      if (out_scores) out_scores[o] = srow[bp];
      if (out_pos) out_pos[o] = bp + 1;
      if (out_obj) out_obj[o] = bv;
      sLead[bp] = kGone;
    }
    if (t + 1 < k) {   // the picked unit row for the next step
      double val = 0.0;
      if (tid < r) {
        const double ivp = item >= 1 && item <= n_items ? inv[item - 1] : 0.0;
        if (ivp != 0.0) val = (double)V[(int64_t)(item - 1) * ld + c0 + tid] * ivp;   // (the zero vector for a degenerate item)
      }
      sPick[tid] = val;
    }
    __syncthreads();   // the flag, the picked row, and the waves' candidates are free to be written again
  }
  for (int q = t + tid; q < k; q += kMmrThreads) {   // fewer than k valid positions: NA from here on
    const size_t o = u * (size_t)k + q;
    out_items[o] = kNaInteger;
    if (out_scores) out_scores[o] = nan_f64();
    if (out_pos) out_pos[o] = kNaInteger;
    if (out_obj) out_obj[o] = nan_f64();
  }
}

template <typename T>
bool rows_aligned16(const T* V, int64_t ld, int c0) {
  constexpr int per16 = 16 / (int)sizeof(T);
  return (reinterpret_cast<uintptr_t>(V) & 15u) == 0 && ld % per16 == 0 && c0 % per16 == 0;
}

template <typename T, int G, bool VEC>
hipError_t launch_mmr_form(const int32_t* lists, const double* scores, int n_users, int N, int k, double theta, const T* V,
                           int n_items, int64_t ld, int c0, int r, const double* inv, int32_t* items, double* picked, int32_t* pos,
                           double* obj, hipStream_t s) {
  const size_t lds = (size_t)16 * N + kMmrFixedBytes;
  auto kern = mmr_kernel<T, G, VEC>;
  if (lds > 64 * 1024) {
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)n_users), dim3(kMmrThreads), lds, s, lists, scores, N, k, theta, V, n_items, ld, c0, r, inv,
                     items, picked, pos, obj);
  return hipGetLastError();
}

template <typename T, int G>
hipError_t launch_mmr_g(const int32_t* lists, const double* scores, int n_users, int N, int k, double theta, const T* V, int n_items,
                        int64_t ld, int c0, int r, const double* inv, int32_t* items, double* picked, int32_t* pos, double* obj,
                        hipStream_t s) {
  if (rows_aligned16(V, ld, c0))
    return launch_mmr_form<T, G, true>(lists, scores, n_users, N, k, theta, V, n_items, ld, c0, r, inv, items, picked, pos, obj, s);
  return launch_mmr_form<T, G, false>(lists, scores, n_users, N, k, theta, V, n_items, ld, c0, r, inv, items, picked, pos, obj, s);
}

// G = the power of two >= r / 4
template <typename T>
hipError_t launch_mmr_t(const int32_t* lists, const double* scores, int n_users, int N, int k, double theta, const T* V, int n_items,
                        int64_t ld, int c0, int r, const double* inv, int32_t* items, double* picked, int32_t* pos, double* obj,
                        hipStream_t s) {
#define RSPARSE_MMR_G(G) \
  launch_mmr_g<T, G>(lists, scores, n_users, N, k, theta, V, n_items, ld, c0, r, inv, items, picked, pos, obj, s)
  if (r <= 4) return RSPARSE_MMR_G(1);
  if (r <= 8) return RSPARSE_MMR_G(2);
  if (r <= 16) return RSPARSE_MMR_G(4);
  if (r <= 32) return RSPARSE_MMR_G(8);
  if (r <= 64) return RSPARSE_MMR_G(16);
  if (r <= 128) return RSPARSE_MMR_G(32);
  return RSPARSE_MMR_G(64);
#undef RSPARSE_MMR_G
}

}  // namespace

hipError_t launch_mmr_rerank(const int32_t* lists, const double* scores, int n_users, int n_pool, int k, double theta, const void* V,
                             bool f64, int n_items, int64_t ld, int c0, int r, const double* inv, int32_t* items, double* picked,
                             int32_t* positions, double* objective, hipStream_t s) {
  if (n_users <= 0) return hipSuccess;
  if (n_pool < 1 || n_pool > kMmrMaxPool || k < 1 || k > n_pool || !(theta >= 0.0 && theta <= 1.0) || n_items < 1 || r < 1 ||
      r > 256 || c0 < 0 || (int64_t)c0 + r > ld)
    return hipErrorInvalidValue;
  return f64 ? launch_mmr_t(lists, scores, n_users, n_pool, k, theta, static_cast<const double*>(V), n_items, ld, c0, r, inv, items,
                            picked, positions, objective, s)
             : launch_mmr_t(lists, scores, n_users, n_pool, k, theta, static_cast<const float*>(V), n_items, ld, c0, r, inv, items,
                            picked, positions, objective, s);
}

}  // namespace rsparse_hip
