// FTRL-proximal elastic-net GLM (McMahan et al. 2013) by deterministic mini-batches, on the device (gfx950).  rsparse_amd/ftrl.py
// (ftrl_forward_reference, ftrl_step_reference) is the definition in numpy, the C header states it for other hosts; DESIGN.md 3.41
// has the scheme.  The model has NO rank dimension: a feature is the pair (z_j, n_j), stored interleaved as one 8-byte (float) or
// 16-byte (double) element so that an entry's whole state comes from one gather instruction.  So a lane owns stored ENTRIES, not
// coordinates (the factorization machine's 16 lanes per row would leave 15 idle here):
//
//   tsum      the definition's sum: chunks of 64 terms, a chunk reduced by the tree v[t] += v[t + h], h = 32, 16, .., 1, the chunk
//             sums added in order from +0.0.  A group of G lanes (4, 16 or 64) holds a chunk as v[i] = term l + G i in lane l: the
//             levels h >= G pair registers of one lane, the levels below pair lanes -- lane-swap instructions for 32 and 16, a DPP
//             row rotation for 8, ds_swizzle for 4, DPP quad permutations for 2 and 1.  Every G therefore adds the same pairs in the
//             same order.  A term slot beyond the row is +0.0 and is skipped (no load, no root): it can only turn a -0.0 into
//             +0.0, which the total's own "+0.0 + chunk" does as well.
//   forward   a group per row of the step; G by the host's rule: the narrowest of 4 / 16 / 64 with 2 G >= nnz / n_rows.  The
//             columns of chunk c + 2 and the values and the zn gather of chunk c + 1 are in flight while chunk c is reduced.  w is
//             formed per lane (one root, one quotient), the Philox call of the keep flag is compiled out at dropout 0.  The
//             group's first lane evaluates the link and d and writes p[r] and d[k].  No LDS on this path; one workgroup-wide vote
//             finds out whether a row of more than RSPARSE_HIP_FTRL_LONG_ROW entries is there: such a row is spread over the four
//             waves of the workgroup, a run of whole chunks each (as 64-lane groups), and its owner adds the chunk sums in order
//             from LDS.  The same kernel without y is `predict`.
//   chunks    a wave per chunk of a (step, column) segment of more than 64 positions: (G, Q, kept) of the chunk.
//   update    a group per (step, column) segment of the index that rsparse_hip_fm_index_device builds (wrmf_fm_index.h).  A lane
//             takes sorted positions: the CSR position, k, d[k] and x are gathered, the keep flag recomputed from (row, position in
//             the row, epoch), g clipped; g, g g and the kept count reduced by the same tree; a long segment's chunk sums added in
//             order.  The group's first lane forms w_j, nn, sigma and z' and writes the pair with ONE store.  Only column j's
//             segment touches zn[j] behind the forward launch.
//   weights   a streaming pass zn -> w with 16-byte loads.
// No float atomics, no host synchronisation between the steps or epochs of a call, every loop bounded by the data sizes.  There is
// no dense operand anywhere, so the matrix instructions have nothing to do.  The file is built with contraction off: every product,
// sum, quotient and root is its own rounded float64 operation.
#include <algorithm>
#include <type_traits>
#include <vector>

#include "../../include/rsparse_wrmf_hip.h"
#include "wrmf_internal.h"
#include "wrmf_device.h"
#include "wrmf_fm_index.h"

#pragma clang fp contract(off)

namespace rsparse_hip {
namespace {

using namespace dev;
using namespace fmidx;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 64;                            // the terms of a chunk of tsum
constexpr int kLongRow = RSPARSE_HIP_FTRL_LONG_ROW;
constexpr int kRound = 64;                            // chunk sums of a long row per round through LDS: 16 per wave
static_assert(kChunk == RSPARSE_HIP_BPR_CHUNK, "the index numbers the chunks of the long segments by RSPARSE_HIP_BPR_CHUNK");

template <class T> struct ZnOf;
template <> struct ZnOf<float> { typedef float2 type; };     // (z, n): one 8-byte gather
template <> struct ZnOf<double> { typedef double2 type; };   // one 16-byte gather

struct FtrlPar {
  double alpha, beta, l1, l2, keep_scale;
  uint32_t drop_t, k0, k1, epoch;
  int step, n_steps, cnt, n_feat, family;
};

// ---- the tree ------------------------------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ double dpp64(const double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
// v(l) + v(l ^ H) in both lanes, the same bits (a + b == b + a); the lanes of a group are active together
template <int H>
__device__ __forceinline__ double lane_pair_sum(const double v) {
  if constexpr (H == 32 || H == 16) {
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    if constexpr (H == 32) {
      const auto sl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);   // halves (0, 0) and (1, 1)
      const auto sh = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
      return __hiloint2double((int)sh[0], (int)sl[0]) + __hiloint2double((int)sh[1], (int)sl[1]);
    } else {
      const auto sl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);   // rows (0, 0, 2, 2) and (1, 1, 3, 3)
      const auto sh = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
      return __hiloint2double((int)sh[0], (int)sl[0]) + __hiloint2double((int)sh[1], (int)sl[1]);
    }
  } else if constexpr (H == 8) {
    return v + dpp64<0x128>(v);   // row_ror:8 = the lane 8 away inside the row of 16
  } else if constexpr (H == 4) {
    // ds_swizzle, bit mode: lane = ((l & 0x1f) | 0) ^ 4 -- pattern = xor << 10 | or << 5 | and.  The LDS crossbar, no LDS memory.
    const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(v), (4 << 10) | 0x1f);
    const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(v), (4 << 10) | 0x1f);
    return v + __hiloint2double(hi, lo);
  } else if constexpr (H == 2) {
    return v + dpp64<0x4E>(v);    // quad_perm:[2,3,0,1]
  } else {
    return v + dpp64<0xB1>(v);    // quad_perm:[1,0,3,2]
  }
}
// the tree of a chunk held as v[i] = term l + G i in lane l of a group of G: every lane of the group ends with the chunk's sum
template <int G>
__device__ __forceinline__ double chunk_tree(double (&v)[kChunk / G]) {
#pragma unroll
  for (int m = kChunk / G / 2; m >= 1; m >>= 1)   // h = G m >= G: terms t and t + h sit in one lane
#pragma unroll
    for (int i = 0; i < m; i++) v[i] = v[i] + v[i + m];
  double s = v[0];
  if constexpr (G > 32) s = lane_pair_sum<32>(s);
  if constexpr (G > 16) s = lane_pair_sum<16>(s);
  if constexpr (G > 8) s = lane_pair_sum<8>(s);
  if constexpr (G > 4) s = lane_pair_sum<4>(s);
  s = lane_pair_sum<2>(s);
  s = lane_pair_sum<1>(s);
  return s;
}

// ---- the pieces of the definition ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ double ftrl_w(const double z, const double n, const FtrlPar& o) {
  if (fabs(z) <= o.l1) return 0.0;
  return (-1.0 / ((o.beta + sqrt(n)) / o.alpha + o.l2)) * (z - (z < 0.0 ? -o.l1 : o.l1));
}
// whether the entry at position t of row r is kept in this epoch
__device__ __forceinline__ bool ftrl_keep(const unsigned t, const unsigned r, const FtrlPar& o) {
  unsigned w[4];
  philox4x32_10(t >> 2, r, 8u, o.epoch, o.k0, o.k1, w);
  const unsigned a = (t & 2u) ? w[2] : w[0], b = (t & 2u) ? w[3] : w[1];
  return ((t & 1u) ? b : a) >= o.drop_t;
}
__device__ __forceinline__ double ftrl_link(const double raw, const int family) {
  if (family == RSPARSE_HIP_FTRL_BINOMIAL) return 1.0 / (1.0 + fm_exp(-raw));
  if (family == RSPARSE_HIP_FTRL_POISSON) return fm_exp(raw);
  return raw;
}

// ---- the forward pass ----------------------------------------------------------------------------------------------------------------
// the chunks [c_lo, c_hi) of the row at CSR position e0 with len entries, by a group of G lanes; emit(c, the chunk's sum) in order
template <class T, int G, bool DROPOUT, class Emit>
__device__ __forceinline__ void row_chunks(const int32_t* __restrict__ J, const T* __restrict__ X,
                                           const typename ZnOf<T>::type* __restrict__ zn, const FtrlPar& o, const unsigned r,
                                           const int e0, const int len, const int c_lo, const int c_hi, const int lane, Emit&& emit) {
  constexpr int NT = kChunk / G;
  typedef typename ZnOf<T>::type ZN;
  if (c_lo >= c_hi) return;
  int jn[NT];
  T xn[NT], xc[NT];
  ZN sn[NT], sc[NT];
  const auto cols = [&](const int c) {   // the columns of chunk c
#pragma unroll
    for (int i = 0; i < NT; i++) {
      const int t = c * kChunk + lane + G * i;
      if (t < len) jn[i] = fm_col(J[e0 + t], o.n_feat);
    }
  };
  const auto vals = [&](const int c) {   // the values and the state of chunk c, whose columns jn holds
#pragma unroll
    for (int i = 0; i < NT; i++) {
      const int t = c * kChunk + lane + G * i;
      if (t < len) {
        xn[i] = X[e0 + t];
        sn[i] = zn[jn[i]];
      }
    }
  };
  // G = 4 keeps nothing in flight across chunks: its rows are one chunk in all but rare cases (the rule picks it for a mean row
  // of at most 8 entries) and the 16 slots of a chunk are 16 independent gathers per lane already; a second set of 16 pairs
  // would take the double kernel past 256 registers
  constexpr bool AHEAD = NT <= 4;
  if (AHEAD) {
    cols(c_lo);
    vals(c_lo);
    if (c_lo + 1 < c_hi) cols(c_lo + 1);
  }
  for (int c = c_lo; c < c_hi; c++) {
    if (!AHEAD) {
      cols(c);
      vals(c);
    }
#pragma unroll
    for (int i = 0; i < NT; i++) {
      xc[i] = xn[i];
      sc[i] = sn[i];
    }
    if (AHEAD && c + 1 < c_hi) {
      vals(c + 1);
      if (c + 2 < c_hi) cols(c + 2);
    }
    double v[NT];
#pragma unroll
    for (int i = 0; i < NT; i++) {
      const int t = c * kChunk + lane + G * i;
      v[i] = 0.0;
      if (t < len) {
        if (!DROPOUT || ftrl_keep((unsigned)t, r, o)) {
          const double xd = DROPOUT ? (double)xc[i] * o.keep_scale : (double)xc[i];
          v[i] = ftrl_w((double)sc[i].x, (double)sc[i].y, o) * xd;
        }
      }
    }
    emit(c, chunk_tree<G>(v));
  }
}

template <class T, int G, int FAMILY, bool DROPOUT>
__global__ __launch_bounds__(kThreads) void ftrl_forward_kernel(const FtrlPar o, const int32_t* __restrict__ P, const int32_t* __restrict__ J,
                                                                const T* __restrict__ X,
                                                                const typename ZnOf<T>::type* __restrict__ zn,
                                                                const double* __restrict__ y, const double* __restrict__ omega,
                                                                double* __restrict__ p_out, double* __restrict__ dk) {
  constexpr int GPB = kThreads / G;
  __shared__ int s_len[GPB], s_e0[GPB];   // (read on the long-row path only)
  __shared__ double s_sum[kRound];
  const int grp = threadIdx.x / G, lane = threadIdx.x % G;
  const int k = blockIdx.x * GPB + grp;
  const bool has = k < o.cnt;
  int64_t r = 0;
  int e0 = 0, len = 0;
  if (has) {
    r = (int64_t)o.step + (int64_t)k * o.n_steps;
    e0 = P[r];
    len = P[r + 1] - e0;
  }
  double total = 0.0;
  if (len <= kLongRow)
    row_chunks<T, G, DROPOUT>(J, X, zn, o, (unsigned)r, e0, len, 0, (len + kChunk - 1) / kChunk, lane,
                              [&](int, const double s) { total = total + s; });
  if (__syncthreads_or(len > kLongRow)) {   // (rare: the long rows of the workgroup, one after the other, on all four waves)
    if (lane == 0) {
      s_len[grp] = len;
      s_e0[grp] = e0;
    }
    __syncthreads();
    const int wv = threadIdx.x >> 6, wl = threadIdx.x & 63;
    for (int g = 0; g < GPB; g++) {   // (every test below is workgroup-uniform)
      const int L = s_len[g];
      if (L <= kLongRow) continue;
      const int ge0 = s_e0[g], n_chunks = (L + kChunk - 1) / kChunk;
      const unsigned gr = (unsigned)((int64_t)o.step + (int64_t)(blockIdx.x * GPB + g) * o.n_steps);
      for (int c0 = 0; c0 < n_chunks; c0 += kRound) {
        const int lo = c0 + wv * (kRound / kWaves);
        row_chunks<T, 64, DROPOUT>(J, X, zn, o, gr, ge0, L, lo, min(lo + kRound / kWaves, n_chunks), wl,
                                   [&](const int c, const double s) { if (wl == 0) s_sum[c - c0] = s; });
        __syncthreads();
        if (grp == g && lane == 0) {
          const int n = min(kRound, n_chunks - c0);
          for (int i = 0; i < n; i++) total = total + s_sum[i];
        }
        __syncthreads();
      }
    }
  }
  if (has && lane == 0) {
    const double pr = ftrl_link(total, FAMILY);
    p_out[r] = pr;
    if (y) dk[k] = omega[r] * (pr - y[r]);
  }
}

// ---- the backward pass ---------------------------------------------------------------------------------------------------------------
struct FtrlBack {
  const int32_t* p;
  const uint32_t* spay;
  const int32_t *sk, *seg_ptr, *seg_col, *choff;
  int seg0, seg1, ch0, n_ch;
};

// (G, Q, whether an entry is kept) of the m <= 64 sorted positions from i0, in every lane of the group of G
template <class T, int G, bool DROPOUT>
__device__ __forceinline__ void col_chunk(const FtrlBack& b, const FtrlPar& o, const T* __restrict__ X, const double* __restrict__ dk,
                                          const int i0, const int m, const int lane, double& gs, double& qs, bool& kept) {
  constexpr int NT = kChunk / G;
  double v[NT], q[NT];
  bool mine = false;
#pragma unroll
  for (int i = 0; i < NT; i++) {
    const int t = lane + G * i;
    v[i] = q[i] = 0.0;
    if (t < m) {
      const uint32_t pos = b.spay[i0 + t];
      const int k = b.sk[i0 + t];
      const double xv = (double)X[pos], d = dk[k];
      bool keep = true;
      if (DROPOUT) {
        const int64_t r = (int64_t)o.step + (int64_t)k * o.n_steps;
        keep = ftrl_keep(pos - (uint32_t)b.p[r], (unsigned)r, o);
      }
      if (keep) {
        const double gx = d * (DROPOUT ? xv * o.keep_scale : xv);
        const double g = gx < -RSPARSE_HIP_FTRL_CLIP ? -RSPARSE_HIP_FTRL_CLIP : (gx > RSPARSE_HIP_FTRL_CLIP ? RSPARSE_HIP_FTRL_CLIP : gx);
        v[i] = g;
        q[i] = g * g;
        mine = true;
      }
    }
  }
  gs = chunk_tree<G>(v);
  qs = chunk_tree<G>(q);
  const u64 all = __ballot(mine);
  const int base = (int)(threadIdx.x & 63u) & ~(G - 1);
  kept = ((all >> base) & (G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull))) != 0ull;
}

// a wave per chunk of the step's long segments: csum[3 (g - ch0)] = (G, Q, kept) of the chunk
template <class T, bool DROPOUT>
__global__ __launch_bounds__(kThreads) void ftrl_chunks_kernel(const FtrlBack b, const FtrlPar o, const T* __restrict__ X,
                                                               const double* __restrict__ dk, double* __restrict__ csum) {
  const int gl = blockIdx.x * kWaves + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (gl >= b.n_ch) return;   // (a whole wave)
  const int g = b.ch0 + gl;
  int lo = b.seg0, hi = b.seg1;   // choff[lo] <= g < choff[hi]
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (b.choff[mid] <= g) lo = mid; else hi = mid;
  }
  const int start = b.seg_ptr[lo] + (g - b.choff[lo]) * kChunk, left = b.seg_ptr[lo + 1] - start;
  double gs, qs;
  bool kept;
  col_chunk<T, 64, DROPOUT>(b, o, X, dk, start, left < kChunk ? left : kChunk, lane, gs, qs, kept);
  if (lane == 0) {
    csum[(size_t)gl * 3] = gs;
    csum[(size_t)gl * 3 + 1] = qs;
    csum[(size_t)gl * 3 + 2] = kept ? 1.0 : 0.0;
  }
}

// a group per segment of the step: the totals, then the update of column j's pair in place
template <class T, int G, bool DROPOUT>
__global__ __launch_bounds__(kThreads) void ftrl_update_kernel(const FtrlBack b, const FtrlPar o, const T* __restrict__ X,
                                                               const double* __restrict__ dk, const double* __restrict__ csum,
                                                               typename ZnOf<T>::type* __restrict__ zn) {
  typedef typename ZnOf<T>::type ZN;
  const int sg = b.seg0 + blockIdx.x * (kThreads / G) + (int)threadIdx.x / G, lane = threadIdx.x % G;
  if (sg >= b.seg1) return;   // (a whole group)
  const int i0 = b.seg_ptr[sg], len = b.seg_ptr[sg + 1] - i0;
  double gt = 0.0, qt = 0.0;
  bool kept = false;
  if (len <= kChunk) {
    double gs, qs;
    col_chunk<T, G, DROPOUT>(b, o, X, dk, i0, len, lane, gs, qs, kept);
    gt = gt + gs;
    qt = qt + qs;
  } else {
    for (int g = b.choff[sg] - b.ch0; g < b.choff[sg + 1] - b.ch0; g++) {
      gt = gt + csum[(size_t)g * 3];
      qt = qt + csum[(size_t)g * 3 + 1];
      kept = kept || csum[(size_t)g * 3 + 2] != 0.0;
    }
  }
  if (lane == 0 && kept) {
    const int j = b.seg_col[sg];
    const ZN old = zn[j];
    const double z = (double)old.x, n = (double)old.y;
    const double w = ftrl_w(z, n, o);
    const double nn = n + qt;
    const double sigma = (sqrt(nn) - sqrt(n)) / o.alpha;
    ZN out;
    out.x = (T)(z + (gt - sigma * w));
    out.y = (T)nn;
    zn[j] = out;
  }
}

// ---- coef() --------------------------------------------------------------------------------------------------------------------------
// 16 bytes per thread: two pairs (float) or one (double); a last odd pair of floats by its own 8-byte load
template <class T>
__global__ __launch_bounds__(kThreads) void ftrl_weights_kernel(const FtrlPar o, const T* __restrict__ zn, double* __restrict__ w) {
  constexpr int PER = 16 / (2 * (int)sizeof(T));
  const int64_t j0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * PER;
  if (j0 >= o.n_feat) return;
  if constexpr (std::is_same<T, float>::value) {
    if (j0 + 1 < o.n_feat) {
      const float4 v = *reinterpret_cast<const float4*>(zn + 2 * j0);
      double2 out;
      out.x = ftrl_w((double)v.x, (double)v.y, o);
      out.y = ftrl_w((double)v.z, (double)v.w, o);
      *reinterpret_cast<double2*>(w + j0) = out;
    } else {
      const float2 v = *reinterpret_cast<const float2*>(zn + 2 * j0);
      w[j0] = ftrl_w((double)v.x, (double)v.y, o);
    }
  } else {
    const double2 v = *reinterpret_cast<const double2*>(zn + 2 * j0);
    w[j0] = ftrl_w(v.x, v.y, o);
  }
}

// ---- the host side -------------------------------------------------------------------------------------------------------------------
#define RSP_TRY(e) do { if ((err = (e)) != hipSuccess) return err; } while (0)

inline dim3 grid_of(int64_t n, int per) { return dim3((unsigned)((n + per - 1) / per)); }
inline int cnt_of(int n_rows, int step, int n_steps) { return (int)(((int64_t)n_rows - step + n_steps - 1) / n_steps); }
// the group width: the narrowest of 4 / 16 / 64 with 2 G >= the mean length (of a row: forward; of a segment: update)
inline int width_of(int64_t entries, int64_t lists) {
  if (entries <= 8 * lists) return 4;
  return entries <= 32 * lists ? 16 : 64;
}
template <class F>
inline void with_width(int g, F&& f) {
  if (g == 4) f(std::integral_constant<int, 4>{});
  else if (g == 16) f(std::integral_constant<int, 16>{});
  else f(std::integral_constant<int, 64>{});
}

inline FtrlPar par_of(const FmData& d, const FtrlOpt& o, int step, uint32_t epoch) {
  FtrlPar a;
  a.alpha = o.alpha; a.beta = o.beta; a.l1 = o.l1; a.l2 = o.l2; a.keep_scale = o.keep_scale;
  a.drop_t = o.drop_t; a.k0 = o.k0; a.k1 = o.k1; a.epoch = epoch;
  a.step = step; a.n_steps = d.n_steps; a.cnt = cnt_of(d.n_rows, step, d.n_steps); a.n_feat = d.n_feat; a.family = o.family;
  return a;
}

template <class T, int G, bool DROPOUT>
void forward_family(const FtrlPar& a, const FmData& d, const typename ZnOf<T>::type* zn, const double* y, const double* omega,
                    double* p_out, double* dk, hipStream_t s) {
  const dim3 grid = grid_of(a.cnt, kThreads / G), block(kThreads);
  const T* X = static_cast<const T*>(d.x);
  if (a.family == RSPARSE_HIP_FTRL_BINOMIAL)
    hipLaunchKernelGGL((ftrl_forward_kernel<T, G, RSPARSE_HIP_FTRL_BINOMIAL, DROPOUT>), grid, block, 0, s, a, d.p, d.j, X, zn, y, omega, p_out, dk);
  else if (a.family == RSPARSE_HIP_FTRL_GAUSSIAN)
    hipLaunchKernelGGL((ftrl_forward_kernel<T, G, RSPARSE_HIP_FTRL_GAUSSIAN, DROPOUT>), grid, block, 0, s, a, d.p, d.j, X, zn, y, omega, p_out, dk);
  else
    hipLaunchKernelGGL((ftrl_forward_kernel<T, G, RSPARSE_HIP_FTRL_POISSON, DROPOUT>), grid, block, 0, s, a, d.p, d.j, X, zn, y, omega, p_out, dk);
}

// the forward launch of one step; dropout acts only with y (predict keeps everything)
template <class T>
void forward_launch(const FtrlPar& a, const FmData& d, const T* zn, const double* y, const double* omega, double* p_out, double* dk,
                    hipStream_t s) {
  const auto* z2 = reinterpret_cast<const typename ZnOf<T>::type*>(zn);
  const bool drop = y && a.drop_t != 0u;
  with_width(width_of(d.nnz, d.n_rows), [&](auto G) {
    if (drop) forward_family<T, decltype(G)::value, true>(a, d, z2, y, omega, p_out, dk, s);
    else forward_family<T, decltype(G)::value, false>(a, d, z2, y, omega, p_out, dk, s);
  });
}

template <class T, bool DROPOUT>
void backward_launch(const FtrlBack& b, const FtrlPar& a, int width, const T* X, const double* dk, double* csum, T* zn, hipStream_t s) {
  auto* z2 = reinterpret_cast<typename ZnOf<T>::type*>(zn);
  const dim3 block(kThreads);
  if (b.n_ch > 0)
    hipLaunchKernelGGL((ftrl_chunks_kernel<T, DROPOUT>), grid_of(b.n_ch, kWaves), block, 0, s, b, a, X, dk, csum);
  if (b.seg1 > b.seg0)
    with_width(width, [&](auto G) {
      hipLaunchKernelGGL((ftrl_update_kernel<T, decltype(G)::value, DROPOUT>), grid_of(b.seg1 - b.seg0, kThreads / decltype(G)::value),
                         block, 0, s, b, a, X, dk, (const double*)csum, z2);
    });
}

}  // namespace

template <class T>
hipError_t launch_ftrl_forward(const FmData& d, const FtrlOpt& o, int step, uint32_t epoch, const T* zn, const double* y,
                               const double* omega, double* p_out, double* dk, hipStream_t s) {
  const FtrlPar a = par_of(d, o, step, epoch);
  if (a.cnt <= 0) return hipSuccess;
  forward_launch<T>(a, d, zn, y, omega, p_out, dk, s);
  return hipGetLastError();
}
template hipError_t launch_ftrl_forward<float>(const FmData&, const FtrlOpt&, int, uint32_t, const float*, const double*, const double*,
                                               double*, double*, hipStream_t);
template hipError_t launch_ftrl_forward<double>(const FmData&, const FtrlOpt&, int, uint32_t, const double*, const double*, const double*,
                                                double*, double*, hipStream_t);

template <class T>
hipError_t launch_ftrl_run(const FmData& d, const void* index, const FtrlOpt& o, int n_epochs, int only_step, uint32_t epoch0,
                           const double* y, const double* omega, T* zn, double* p_out, hipStream_t s) {
  hipError_t err;
  const FmIndex ix = fm_index_of(const_cast<void*>(index), d.nnz, d.n_steps);
  const size_t ns = (size_t)d.n_steps + 1;
  std::vector<int32_t> head(4 + 2 * ns);
  RSP_TRY(hipMemcpyAsync(head.data(), ix.hdr, head.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  RSP_TRY(hipStreamSynchronize(s));
  if (head[0] != kFmMagic || head[1] != d.n_steps || head[2] != (int32_t)d.nnz) return hipErrorInvalidValue;   // (another x or n_steps)
  const int32_t *step_seg = head.data() + 4, *step_ch = step_seg + ns;
  const int first = only_step < 0 ? 0 : only_step, last = only_step < 0 ? d.n_steps : only_step + 1;
  int max_ch = 0;
  for (int st = first; st < last; st++) max_ch = std::max(max_ch, step_ch[st + 1] - step_ch[st]);
  const int width = width_of(d.nnz, std::max(head[3], 1));
  DevBuf dk, csum;   // the workspace of a step: its rows' d and the long segments' chunk sums
  RSP_TRY(dk.alloc((size_t)cnt_of(d.n_rows, first, d.n_steps) * 8));
  RSP_TRY(csum.alloc((size_t)max_ch * 3 * 8));
  const T* X = static_cast<const T*>(d.x);
  FtrlBack b;
  b.p = d.p; b.spay = ix.spay; b.sk = ix.sk; b.seg_ptr = ix.seg_ptr; b.seg_col = ix.seg_col; b.choff = ix.choff;
  for (int e = 0; e < n_epochs; e++) {
    for (int st = first; st < last; st++) {
      const FtrlPar a = par_of(d, o, st, epoch0 + (uint32_t)e);
      if (a.cnt <= 0) continue;
      forward_launch<T>(a, d, (const T*)zn, y, omega, p_out, dk.as<double>(), s);
      b.seg0 = step_seg[st]; b.seg1 = step_seg[st + 1]; b.ch0 = step_ch[st]; b.n_ch = step_ch[st + 1] - b.ch0;
      if (a.drop_t != 0u) backward_launch<T, true>(b, a, width, X, dk.as<double>(), csum.as<double>(), zn, s);
      else backward_launch<T, false>(b, a, width, X, dk.as<double>(), csum.as<double>(), zn, s);
      RSP_TRY(hipGetLastError());
    }
  }
  RSP_TRY(hipStreamSynchronize(s));   // the scratch is freed on return
  return hipSuccess;
}
template hipError_t launch_ftrl_run<float>(const FmData&, const void*, const FtrlOpt&, int, int, uint32_t, const double*, const double*,
                                           float*, double*, hipStream_t);
template hipError_t launch_ftrl_run<double>(const FmData&, const void*, const FtrlOpt&, int, int, uint32_t, const double*, const double*,
                                            double*, double*, hipStream_t);

template <class T>
hipError_t launch_ftrl_weights(const T* zn, int n_feat, const FtrlOpt& o, double* w, hipStream_t s) {
  if (n_feat <= 0) return hipSuccess;
  FmData d{};
  d.n_feat = n_feat; d.n_steps = 1;
  const FtrlPar a = par_of(d, o, 0, 0u);
  constexpr int per = 16 / (2 * (int)sizeof(T));
  hipLaunchKernelGGL((ftrl_weights_kernel<T>), grid_of(((int64_t)n_feat + per - 1) / per, kThreads), dim3(kThreads), 0, s, a, zn, w);
  return hipGetLastError();
}
template hipError_t launch_ftrl_weights<float>(const float*, int, const FtrlOpt&, double*, hipStream_t);
template hipError_t launch_ftrl_weights<double>(const double*, int, const FtrlOpt&, double*, hipStream_t);

#undef RSP_TRY

}  // namespace rsparse_hip
