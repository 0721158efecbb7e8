// Intra-list diversity of top-k lists at up to kHitMaxCutoffs cutoffs: the mean cosine distance 1 - <v_i, v_j> / (|v_i| |v_j|)
// over the pairs of items of a list.  gfx950, wave64.  The definition is the numpy statement `list_diversity_reference` of
// rsparse_amd/metrics.py.  With S the sum of the m unit vectors of a list's first c positions, the sum over all
// ordered pairs of their dot products is |S|^2, of which m are the items with themselves, so
//   diversity = 1 - (|S|^2 - m) / (m (m - 1))
// -- O(k r) work per list, not O(k^2 r).  Two kernels:
//
//   item_inv_norms_kernel   V[:, c0:c1) (fp32 or fp64, n_items x ld row-major) -> inv[item] = 1 / sqrt(sum of squares) in double,
//                           0.0 for a degenerate item (sum zero or not finite; the zero is the flag).  The shape of
//                           normalize_items_kernel (wrmf_similar.hip): G lanes per item (G = the power of two >= r / 4), four
//                           consecutive coordinates per lane, 16-byte loads when the rows are 16-byte aligned (scalar otherwise:
//                           a window that starts at the bias column, odd ranks), the squares summed in double by a butterfly
//                           within the G lanes.  8 bytes written per item, against the 12 r of the normalised replicas.
//   list_diversity_kernel   one wave per user, four users per workgroup.  The wave reads the list in chunks of 64 positions (a
//                           lane holds one item and gathers inv[item]: one double per position); a position is counted when
//                           its item lies in 1 .. n_items and its inv is not 0.  The 64 / G lane groups then gather the rows of
//                           the factors AS STORED -- r sizeof(T) bytes per position, a quarter of what the unit rows in double
//                           would move --, kDivAhead rows per group in flight, and accumulate double(v) * inv into their part of
//                           S in registers.  The positions of a cutoff interval (inside one chunk) go round-robin to the
//                           groups; where an interval ends, the groups' partial sums are combined by a fixed xor-butterfly into
//                           the running S, |S|^2 is reduced over the G lanes of a group by another, and lane t writes cutoff t.
// No atomics, no LDS; the order of every sum depends on (k, cutoffs, r) alone: a repeated call returns the same bits.
#include <hip/hip_runtime.h>

#include "wrmf_internal.h"
#include "wrmf_device.h"

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kDivThreads = 256;
constexpr int kDivWaves = kDivThreads / 64;   // users (waves) per workgroup
constexpr int kDivAhead = 4;                  // rows a lane group gathers before the first of them is used
constexpr int kDivMaxGrid = 256 * 8;          // workgroups of the norms launch (grid-stride over the items beyond)
constexpr int kNaInteger = INT32_MIN;         // RSPARSE_HIP_NA_INTEGER

struct DivCutoffs {
  int n;
  int c[kHitMaxCutoffs];
};

// four consecutive elements at p -> double; `valid` (1 .. 4) of them exist, the others read as zero
template <typename T, bool VEC>
__device__ __forceinline__ void load4(const T* __restrict__ p, int valid, double x[4]) {
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
    for (int e = 0; e < 4; e++) x[e] = e < valid ? (double)p[e] : 0.0;
  }
}

// G lanes per item, two items per group and pass (both loads are issued before either sum)
template <typename T, int G, bool VEC>
__global__ void __launch_bounds__(kDivThreads)
item_inv_norms_kernel(const T* __restrict__ V, int n_items, int64_t ld, int c0, int r, double* __restrict__ inv) {
  constexpr int GPB = kDivThreads / G;   // groups per workgroup
  const int gl = threadIdx.x % G;
  const int j0 = 4 * gl;
  const int valid = min(4, r - j0);      // <= 0: this lane holds no coordinate of the row
  const int64_t slots = (int64_t)gridDim.x * GPB;
  // every lane of the workgroup makes the same number of passes (the shuffles below run with all lanes present)
  for (int64_t base = (int64_t)blockIdx.x * GPB; base < n_items; base += 2 * slots) {
    double x[2][4];
    int64_t item[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
      item[u] = base + threadIdx.x / G + u * slots;
      if (item[u] < n_items && valid > 0)
        load4<T, VEC>(V + item[u] * ld + c0 + j0, valid, x[u]);
      else
        x[u][0] = x[u][1] = x[u][2] = x[u][3] = 0.0;
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
      double ss = (x[u][0] * x[u][0] + x[u][1] * x[u][1]) + (x[u][2] * x[u][2] + x[u][3] * x[u][3]);
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, G);
      const bool ok = ss > 0.0 && ss < INFINITY;   // (a NaN fails both)
      if (item[u] < n_items && gl == 0) inv[item[u]] = ok ? 1.0 / sqrt(ss) : 0.0;
    }
  }
}

template <typename T, int G, bool VEC>
__global__ void __launch_bounds__(kDivThreads)
list_diversity_kernel(const int32_t* __restrict__ pred, int n_users, int k, const DivCutoffs cut, const T* __restrict__ V,
                      int n_items, int64_t ld, int c0, int r, const double* __restrict__ inv, int32_t* __restrict__ counted_out,
                      double* __restrict__ div_out) {
  constexpr int NG = 64 / G;   // lane groups of the wave
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int u = blockIdx.x * kDivWaves + w;
  if (u >= n_users) return;   // (whole waves: nothing below synchronises across waves)
  const int T_ = cut.n;
  int my_c = 0;               // lane t < T: cutoff t
#pragma unroll
  for (int t = 0; t < kHitMaxCutoffs; t++)
    if (t < T_ && lane == t) my_c = cut.c[t];
  int c_last = 0;
#pragma unroll
  for (int t = 0; t < kHitMaxCutoffs; t++)
    if (t < T_) c_last = cut.c[t];   // ascending: the largest
  const int gi = lane / G, j0 = 4 * (lane % G);
  const int nco = min(4, r - j0);    // coordinates of this lane; <= 0: none (it gathers nothing and adds zeros)
  const T* Vw = V + c0;              // row 0 of the window: what a lane without a position reads and drops
  const int32_t* prow = pred + (size_t)u * k;
  double S[4] = {0.0, 0.0, 0.0, 0.0};   // the running sum of the unit vectors, this lane's coordinates (the same in every group)
  double P[4] = {0.0, 0.0, 0.0, 0.0};   // this group's part of the open interval
  int m = 0;                            // counted positions so far (uniform)
  int tcur = 0;                         // the open interval (uniform)
  int cend = rfl(__shfl(my_c, 0));      // ... ends behind the 0-based position cend - 1
  for (int base = 0; base < c_last; base += 64) {
    const int i = base + lane;
    const int32_t c = i < c_last ? prow[i] : kNaInteger;
    const bool in = c != kNaInteger && c >= 1 && c <= n_items;
    const double my_inv = in ? inv[c - 1] : 0.0;
    const u64 okm = __ballot(in && my_inv != 0.0);
    int a = 0;   // chunk-relative start of the segment: the part of an interval inside this chunk
    while (a < 64 && base + a < c_last) {
      const int bnd = min(cend - base, 64);   // ... and its end
      for (int s0 = a; s0 < bnd; s0 += NG * kDivAhead) {
        double x[kDivAhead][4], sc[kDivAhead];
#pragma unroll
        for (int q = 0; q < kDivAhead; q++) {   // every gather of the step before the first use
          const int pos = s0 + q * NG + gi;
          const int from = min(pos, 63);
          const int32_t item = __shfl(c, from);
          const double iv = __shfl(my_inv, from);
          const bool act = pos < bnd && ((okm >> from) & 1ull) != 0ull;
          sc[q] = act ? iv : 0.0;
          if (nco > 0)
            load4<T, VEC>(act ? V + (int64_t)(item - 1) * ld + c0 + j0 : Vw + j0, nco, x[q]);
          else
            x[q][0] = x[q][1] = x[q][2] = x[q][3] = 0.0;
#pragma unroll
          for (int e = 0; e < 4; e++) x[q][e] = act ? x[q][e] : 0.0;   // (a dropped row may hold anything: not 0 * x)
        }
#pragma unroll
        for (int q = 0; q < kDivAhead; q++)
#pragma unroll
          for (int e = 0; e < 4; e++) P[e] = fma(x[q][e], sc[q], P[e]);
      }
      {
        const int lo = a, hi = bnd;   // counted positions of the segment
        const u64 upto = hi >= 64 ? ~0ull : ((1ull << hi) - 1ull);
        const u64 from0 = lo >= 64 ? 0ull : ~((1ull << lo) - 1ull);
        m += __popcll(okm & upto & from0);
      }
      a = bnd;
      if (base + bnd == cend) {   // the interval ends here: fold the groups' parts into S and write the cutoff
#pragma unroll
        for (int d = G; d < 64; d <<= 1)
#pragma unroll
          for (int e = 0; e < 4; e++) P[e] += __shfl_xor(P[e], d);
        double ss;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          S[e] += P[e];
          P[e] = 0.0;
        }
        ss = (S[0] * S[0] + S[1] * S[1]) + (S[2] * S[2] + S[3] * S[3]);
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
        if (lane == tcur) {
          const size_t o = (size_t)u * T_ + tcur;
          const double md = (double)m;
          if (counted_out) counted_out[o] = m;
          if (div_out)
            div_out[o] = m < 2 ? __longlong_as_double(0x7ff8000000000000ll) : 1.0 - (ss - md) / (md * (md - 1.0));
        }
        tcur++;
        cend = tcur < T_ ? rfl(__shfl(my_c, tcur)) : INT32_MAX;
      }
    }
  }
}

int div_grid(int64_t n, int G) {
  const int gpb = kDivThreads / G;
  const int64_t blocks = (n + gpb - 1) / gpb;
  return (int)(blocks < 1 ? 1 : (blocks > kDivMaxGrid ? kDivMaxGrid : blocks));
}

template <typename T>
bool rows_aligned16(const T* V, int64_t ld, int c0) {
  constexpr int per16 = 16 / (int)sizeof(T);
  return (reinterpret_cast<uintptr_t>(V) & 15u) == 0 && ld % per16 == 0 && c0 % per16 == 0;
}

template <typename T, int G>
hipError_t launch_inv_g(const T* V, int n_items, int64_t ld, int c0, int r, double* inv, hipStream_t s) {
  // (two items per group and pass: half the workgroups of one item per group)
  const dim3 grid(div_grid(((int64_t)n_items + 1) / 2, G)), block(kDivThreads);
  if (rows_aligned16(V, ld, c0))
    hipLaunchKernelGGL((item_inv_norms_kernel<T, G, true>), grid, block, 0, s, V, n_items, ld, c0, r, inv);
  else
    hipLaunchKernelGGL((item_inv_norms_kernel<T, G, false>), grid, block, 0, s, V, n_items, ld, c0, r, inv);
  return hipGetLastError();
}

template <typename T, int G>
hipError_t launch_div_g(const int32_t* pred, int n_users, int k, const DivCutoffs& cut, const T* V, int n_items, int64_t ld, int c0,
                        int r, const double* inv, int32_t* counted, double* diversity, hipStream_t s) {
  const dim3 grid((unsigned)((n_users + kDivWaves - 1) / kDivWaves)), block(kDivThreads);
  if (rows_aligned16(V, ld, c0))
    hipLaunchKernelGGL((list_diversity_kernel<T, G, true>), grid, block, 0, s, pred, n_users, k, cut, V, n_items, ld, c0, r, inv,
                       counted, diversity);
  else
    hipLaunchKernelGGL((list_diversity_kernel<T, G, false>), grid, block, 0, s, pred, n_users, k, cut, V, n_items, ld, c0, r, inv,
                       counted, diversity);
  return hipGetLastError();
}

// G = the power of two >= r / 4
#define RSPARSE_DIV_BY_RANK(CALL) \
  if (r <= 4) return CALL(1);     \
  if (r <= 8) return CALL(2);     \
  if (r <= 16) return CALL(4);    \
  if (r <= 32) return CALL(8);    \
  if (r <= 64) return CALL(16);   \
  if (r <= 128) return CALL(32);  \
  return CALL(64)

template <typename T>
hipError_t launch_inv_t(const T* V, int n_items, int64_t ld, int c0, int r, double* inv, hipStream_t s) {
#define RSPARSE_DIV_INV(G) launch_inv_g<T, G>(V, n_items, ld, c0, r, inv, s)
  RSPARSE_DIV_BY_RANK(RSPARSE_DIV_INV);
#undef RSPARSE_DIV_INV
}

template <typename T>
hipError_t launch_div_t(const int32_t* pred, int n_users, int k, const DivCutoffs& cut, const T* V, int n_items, int64_t ld, int c0,
                        int r, const double* inv, int32_t* counted, double* diversity, hipStream_t s) {
#define RSPARSE_DIV_LIST(G) launch_div_g<T, G>(pred, n_users, k, cut, V, n_items, ld, c0, r, inv, counted, diversity, s)
  RSPARSE_DIV_BY_RANK(RSPARSE_DIV_LIST);
#undef RSPARSE_DIV_LIST
}
#undef RSPARSE_DIV_BY_RANK

}  // namespace

hipError_t launch_item_inv_norms(const void* V, bool f64, int n_items, int64_t ld, int c0, int r, double* inv, hipStream_t s) {
  if (n_items <= 0) return hipSuccess;
  if (r < 1 || r > 256 || c0 < 0 || (int64_t)c0 + r > ld) return hipErrorInvalidValue;
  return f64 ? launch_inv_t(static_cast<const double*>(V), n_items, ld, c0, r, inv, s)
             : launch_inv_t(static_cast<const float*>(V), n_items, ld, c0, r, inv, s);
}

hipError_t launch_list_diversity(const int32_t* pred, int n_users, int k, const int32_t* cutoffs, int n_cutoffs, const void* V,
                                 bool f64, int n_items, int64_t ld, int c0, int r, const double* inv, int32_t* counted,
                                 double* diversity, hipStream_t s) {
  if (n_users <= 0) return hipSuccess;
  if (n_cutoffs < 1 || n_cutoffs > kHitMaxCutoffs || n_items < 1 || r < 1 || r > 256 || c0 < 0 || (int64_t)c0 + r > ld)
    return hipErrorInvalidValue;
  DivCutoffs cut;
  cut.n = n_cutoffs;
  for (int t = 0; t < kHitMaxCutoffs; t++) cut.c[t] = t < n_cutoffs ? cutoffs[t] : 0;
  return f64 ? launch_div_t(pred, n_users, k, cut, static_cast<const double*>(V), n_items, ld, c0, r, inv, counted, diversity, s)
             : launch_div_t(pred, n_users, k, cut, static_cast<const float*>(V), n_items, ld, c0, r, inv, counted, diversity, s);
}

}  // namespace rsparse_hip
