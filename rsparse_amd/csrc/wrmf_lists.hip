// Beyond-accuracy metrics of top-k lists at up to kHitMaxCutoffs cutoffs in one pass: how many positions of a list name an item
// of the catalogue, the sums of two per-item integer tables over them (an interaction count -> popularity, a fixed-point
// self-information -> novelty) and the exposure histogram of the catalogue.  gfx950, wave64.  The definition is the numpy
// statement `list_metrics_reference` of rsparse_amd/metrics.py; every sum is an integer sum and every double ONE
// division of two exactly converted integers, so the kernel equals it bit for bit.
//
// Per user u and the cutoffs c_1 < ... < c_T <= k, a position i (1-based) is VALID when its item lies in 1 .. n_items:
//   valid[t] = #{valid i <= c_t}    count_sum[t] = sum item_count[item_i]    info_sum[t] = sum item_info[item_i]   (valid i <= c_t)
//   popularity = count_sum / valid                novelty = info_sum / (valid 2^32)                NaN where valid = 0
// Over all users: exposure[b][item] += 1 for every valid position of the cutoff INTERVAL b (c_(b-1) < i <= c_b); the caller
// cumulates along b, so a position costs one atomic and not T.
//
// One launch, one wave per user, four users per workgroup (the layout of hit_metrics_kernel).  The wave walks the positions
// 0 .. c_T - 1 -- not k -- in chunks of 64, the loads of kListAhead chunks issued together.  Per chunk a lane holds one item and
// gathers its table entries (0 for an invalid lane); the wave makes ONE inclusive scan per table (six shuffle steps); the
// validity bit needs none: its scan at a lane is the popcount of the ballot below it.  Lane t < T owns cutoff t and fetches the
// prefix at its cutoff with one shuffle -- no T masked reductions.  Integer atomics only, no floating-point sum: a call
// repeats bit for bit.  A table that is null is not gathered.
#include "wrmf_internal.h"
#include "wrmf_device.h"

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kListWaves = 4;           // users (waves) per workgroup
constexpr int kListAhead = 4;           // chunks of 64 positions whose loads are issued together
constexpr int kNaInteger = INT32_MIN;   // RSPARSE_HIP_NA_INTEGER

// the cutoffs travel by value: nothing is uploaded for them
struct ListCutoffs {
  int n;
  int c[kHitMaxCutoffs];
};

// inclusive scan over the 64 lanes (lane l: the sum of the lanes 0 .. l).  Needs full EXEC.
__device__ __forceinline__ long long wave_scan(long long v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

template <bool EXPOSURE>
__global__ __launch_bounds__(64 * kListWaves) void list_metrics_kernel(const int32_t* __restrict__ pred, int n_users, int k,
                                                                       const ListCutoffs cut,
                                                                       const int32_t* __restrict__ item_count,
                                                                       const int64_t* __restrict__ item_info, int n_items,
                                                                       int32_t* __restrict__ valid_out,
                                                                       int64_t* __restrict__ count_out,
                                                                       int64_t* __restrict__ info_out, double* __restrict__ pop_out,
                                                                       double* __restrict__ nov_out, int32_t* exposure) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int u = blockIdx.x * kListWaves + w;
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
  const bool want_count = item_count != nullptr, want_info = item_info != nullptr;
  int cnt = 0;
  long long csum = 0, isum = 0;
  const int32_t* prow = pred + (size_t)u * k;
  for (int base4 = 0; base4 < c_last; base4 += 64 * kListAhead) {
    int32_t cs[kListAhead];   // the loads of kListAhead chunks are in flight before the first gather
#pragma unroll
    for (int q = 0; q < kListAhead; q++) {
      const int i = base4 + 64 * q + lane;
      cs[q] = i < c_last ? prow[i] : kNaInteger;
    }
    bool ok[kListAhead];
    long long gc[kListAhead], gi[kListAhead];
#pragma unroll
    for (int q = 0; q < kListAhead; q++) {   // ... and the gathers of all of them before the first scan
      const int32_t c = cs[q];
      ok[q] = c != kNaInteger && c >= 1 && c <= n_items;
      gc[q] = (want_count && ok[q]) ? (long long)item_count[c - 1] : 0ll;
      gi[q] = (want_info && ok[q]) ? (long long)item_info[c - 1] : 0ll;
    }
#pragma unroll
    for (int q = 0; q < kListAhead; q++) {
      const int base = base4 + 64 * q;
      if (base >= c_last) break;
      if (EXPOSURE && ok[q]) {
        const int pos = base + lane + 1;
        int b = 0;   // the cutoff interval of the position: the cutoffs below it
#pragma unroll
        for (int t = 0; t < kHitMaxCutoffs; t++) b += (t < T && cut.c[t] < pos) ? 1 : 0;
        atomicAdd(&exposure[(size_t)b * (size_t)n_items + (size_t)(cs[q] - 1)], 1);
      }
      const int cover = min(max(my_c - base, 0), 64);   // lanes of this chunk under my cutoff
      const int src = max(cover - 1, 0);
      const u64 m = __ballot(ok[q]);
      cnt += __popcll(m & (cover == 64 ? ~0ull : ((1ull << cover) - 1ull)));
      if (want_count) {
        const long long at = __shfl(wave_scan(gc[q], lane), src);
        csum += cover > 0 ? at : 0ll;
      }
      if (want_info) {
        const long long at = __shfl(wave_scan(gi[q], lane), src);
        isum += cover > 0 ? at : 0ll;
      }
    }
  }
  if (lane >= T) return;
  const size_t o = (size_t)u * T + lane;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (valid_out) valid_out[o] = cnt;
  if (count_out) count_out[o] = csum;
  if (info_out) info_out[o] = isum;
  if (pop_out) pop_out[o] = cnt == 0 ? nan : (double)csum / (double)cnt;
  if (nov_out) nov_out[o] = cnt == 0 ? nan : (double)isum / ((double)cnt * 4294967296.0);
}

}  // namespace

hipError_t launch_list_metrics(const int32_t* pred, int n_users, int k, const int32_t* cutoffs, int n_cutoffs,
                               const int32_t* item_count, const int64_t* item_info, int n_items, int32_t* valid, int64_t* count_sum,
                               int64_t* info_sum, double* popularity, double* novelty, int32_t* exposure, hipStream_t s) {
  if (n_users <= 0) return hipSuccess;
  if (n_cutoffs < 1 || n_cutoffs > kHitMaxCutoffs || n_items < 1) return hipErrorInvalidValue;
  ListCutoffs cut;
  cut.n = n_cutoffs;
  for (int t = 0; t < kHitMaxCutoffs; t++) cut.c[t] = t < n_cutoffs ? cutoffs[t] : 0;
  const dim3 grid((unsigned)((n_users + kListWaves - 1) / kListWaves)), block(64 * kListWaves);
  if (exposure)
    hipLaunchKernelGGL((list_metrics_kernel<true>), grid, block, 0, s, pred, n_users, k, cut, item_count, item_info, n_items, valid,
                       count_sum, info_sum, popularity, novelty, exposure);
  else
    hipLaunchKernelGGL((list_metrics_kernel<false>), grid, block, 0, s, pred, n_users, k, cut, item_count, item_info, n_items, valid,
                       count_sum, info_sum, popularity, novelty, exposure);
  return hipGetLastError();
}

}  // namespace rsparse_hip
