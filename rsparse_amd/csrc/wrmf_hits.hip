// Hit-based metrics of top-k lists at up to kHitMaxCutoffs cutoffs in one pass: hit counts, the first hit, precision, recall, hit
// rate and reciprocal rank per user, and the catalogue coverage of the lists.  gfx950, wave64.  The definition is the numpy
// statement `hit_metrics_reference` of rsparse_amd/metrics.py; every double is ONE division of two exactly
// converted integers, so the kernel equals it bit for bit.
//
// Per user u with n_u stored entries in its row of `actual` (sorted column indices j) and the cutoffs c_1 < ... < c_T <= k:
//   hit_i     = the prediction at the 1-based position i is a stored column of the row (looked up on its own, as ap_k does: NA,
//               indices below 1 and outside the row are misses, a repeated index hits every time, a stored zero is relevant)
//   hits[t]   = sum over i <= c_t of hit_i          first = the smallest i <= c_T with hit_i, 0 without one
//   precision = hits / c_t   recall = hits / n_u   hit = hits > 0   mrr = 1 / first where 0 < first <= c_t, else 0
//   n_u = 0: NaN in the four doubles (the user is not evaluated), hits = first = 0.
// Over all users, n_u = 0 included: first_seen[item] = min(first_seen[item], the smallest position i <= c_T listing the item).
//
// One launch, one wave per user, four users per workgroup (the layout of metrics_rows_kernel).  A row of up to kHitRowCap
// entries is staged in LDS, a longer one is binary-searched where it lies.  The wave walks the positions 0 .. c_T - 1 -- not k --
// in chunks of 64: one ballot of the hits per chunk; lane t < T owns cutoff t and adds the popcount of the ballot under the lanes
// of the chunk that its cutoff covers; the first non-zero ballot gives `first`.  Lanes 0 .. T - 1 write their cutoff's column.
// The loads of kHitAhead chunks are issued before the first of their lookups: the launch is bound by the read of the lists, and
// one 256-byte load in flight per wave left a fifth of the time on the table.
// Coverage: a lane holding an item of 1 .. n_items reads first_seen[item] and issues atomicMin only where its position is
// smaller (a stale read can only cost a needless atomic: the slot never grows).  Integer atomics only, no sums across lanes:
// a call repeats bit for bit.
#include "wrmf_internal.h"
#include "wrmf_device.h"

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kHitWaves = 4;            // users (waves) per workgroup
constexpr int kHitAhead = 4;            // chunks of 64 positions whose loads are issued together
constexpr int kHitRowCap = 512;         // rows up to this long are staged in LDS
constexpr int kNaInteger = INT32_MIN;   // RSPARSE_HIP_NA_INTEGER

// the cutoffs travel by value: nothing is uploaded for them
struct HitCutoffs {
  int n;
  int c[kHitMaxCutoffs];
};

// rj[0, n) ascending: does it hold t?
__device__ __forceinline__ bool row_has(const int32_t* rj, int n, int32_t t) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rj[mid] < t) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && rj[lo] == t;
}

template <bool COVERAGE>
__global__ __launch_bounds__(64 * kHitWaves) void hit_metrics_kernel(const int32_t* __restrict__ pred, int n_users, int k,
                                                                      const int32_t* __restrict__ P, const int32_t* __restrict__ J,
                                                                      const HitCutoffs cut, int32_t* __restrict__ hits_out,
                                                                      int32_t* __restrict__ first_out, double* __restrict__ prec_out,
                                                                      double* __restrict__ rec_out, double* __restrict__ hit_out,
                                                                      double* __restrict__ mrr_out, int32_t* first_seen, int n_items) {
  __shared__ int32_t s_j[kHitWaves][kHitRowCap];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int u = blockIdx.x * kHitWaves + w;
  if (u >= n_users) return;   // (whole waves: nothing below synchronises across waves)
  const int T = cut.n;
  int my_c = 0;               // lane t < T: cutoff t; the other lanes count nothing
#pragma unroll
  for (int t = 0; t < kHitMaxCutoffs; t++)
    if (t < T && lane == t) my_c = cut.c[t];
  int c_last = 0;
#pragma unroll
  for (int t = 0; t < kHitMaxCutoffs; t++)
    if (t < T) c_last = cut.c[t];   // ascending: the largest
  const int p0 = P[u];
  const int n_u = max(P[u + 1] - p0, 0);
  int cnt = 0, first = 0;
  if (COVERAGE || n_u > 0) {   // (a user with nothing held out still walks its list when coverage is wanted)
    const bool staged = n_u <= kHitRowCap;
    if (staged) {
      for (int e = lane; e < n_u; e += 64) s_j[w][e] = J[p0 + e];
      wave_sync();
    }
    const int32_t* rj = staged ? s_j[w] : J + p0;
    const int32_t* prow = pred + (size_t)u * k;
    for (int base4 = 0; base4 < c_last; base4 += 64 * kHitAhead) {
      int32_t cs[kHitAhead];   // the loads of kHitAhead chunks are in flight before the first lookup
#pragma unroll
      for (int q = 0; q < kHitAhead; q++) {
        const int i = base4 + 64 * q + lane;
        cs[q] = i < c_last ? prow[i] : kNaInteger;
      }
#pragma unroll
      for (int q = 0; q < kHitAhead; q++) {
        const int base = base4 + 64 * q;
        if (base >= c_last) break;
        const int i = base + lane;
        const int32_t c = cs[q];
        bool h = false;
        if (c != kNaInteger && c >= 1) {
          h = n_u > 0 && row_has(rj, n_u, c - 1);   // 1-based item -> 0-based column
          if (COVERAGE && c <= n_items && first_seen[c - 1] > i + 1) atomicMin(&first_seen[c - 1], i + 1);
        }
        const u64 m = __ballot(h);
        if (first == 0 && m != 0ull) first = base + __ffsll((long long)m);   // 1-based position of the lowest hit lane
        const int cover = min(max(my_c - base, 0), 64);   // lanes of this chunk under my cutoff
        cnt += __popcll(m & (cover == 64 ? ~0ull : ((1ull << cover) - 1ull)));
      }
    }
  }
  if (lane == 0 && first_out) first_out[u] = first;
  if (lane >= T) return;
  const size_t o = (size_t)u * T + lane;
  if (hits_out) hits_out[o] = cnt;
  const bool none = n_u == 0;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (prec_out) prec_out[o] = none ? nan : (double)cnt / (double)my_c;
  if (rec_out) rec_out[o] = none ? nan : (double)cnt / (double)n_u;
  if (hit_out) hit_out[o] = none ? nan : (cnt > 0 ? 1.0 : 0.0);
  if (mrr_out) mrr_out[o] = none ? nan : ((first > 0 && first <= my_c) ? 1.0 / (double)first : 0.0);
}

}  // namespace

hipError_t launch_hit_metrics(const int32_t* pred, int n_users, int k, const int32_t* P, const int32_t* J, const int32_t* cutoffs,
                              int n_cutoffs, int32_t* hits, int32_t* first, double* precision, double* recall, double* hit,
                              double* mrr, int32_t* first_seen, int n_items, hipStream_t s) {
  if (n_users <= 0) return hipSuccess;
  HitCutoffs cut;
  cut.n = n_cutoffs;
  for (int t = 0; t < kHitMaxCutoffs; t++) cut.c[t] = t < n_cutoffs ? cutoffs[t] : 0;
  const dim3 grid((unsigned)((n_users + kHitWaves - 1) / kHitWaves)), block(64 * kHitWaves);
  if (first_seen)
    hipLaunchKernelGGL((hit_metrics_kernel<true>), grid, block, 0, s, pred, n_users, k, P, J, cut, hits, first, precision, recall, hit,
                       mrr, first_seen, n_items);
  else
    hipLaunchKernelGGL((hit_metrics_kernel<false>), grid, block, 0, s, pred, n_users, k, P, J, cut, hits, first, precision, recall, hit,
                       mrr, first_seen, n_items);
  return hipGetLastError();
}

}  // namespace rsparse_hip
