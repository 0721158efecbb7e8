// Full-ranking metrics: where every held-out item of a user stands among ALL the items the user could be shown, gfx950, wave64.
//
// Semantics (include/rsparse_wrmf_hip.h).  For user u the admissible set A_u is the items outside the user's
// not_recommend row and outside items_exclude -- exactly the items whose key is non-zero after topl_mask_kernel --, n_adm = |A_u|.
// Scores are the fp32 scores of the large-k path (wrmf_topk_large.hip), compared through their order-preserving 32-bit keys:
// -0 and +0 are one score, a global bias shifts every score alike and plays no part.  For a stored entry (u, h) of `actual`:
//   above = #{j in A_u : s_j > s_h},   tied = #{j in A_u, j != h : s_j == s_h};   h not in A_u: above = tied = -1.
//
// Per chunk of users (sized so that the key matrix stays under the 2 GiB of the large-k path's workspace):
//   1. launch_topl_score + launch_topl_mask: the key matrix [users][items] of the large-k path, its stages unchanged.
//   2. ranks_init_kernel: one workgroup per user looks its held-out items up in the key row: above = 0, tied = -1 (the entry's
//      own match, which step 3 counts once) for an admissible entry, above = tied = -1 for the others.
//   3. ranks_count_kernel: grid = (item slices, users), like topl_hist_kernel.  A workgroup fetches the keys of the user's
//      held-out items ("thresholds"), at most kRankT at a time, sorts them in LDS, and streams its slice of the key row once per
//      batch (16-byte vectors; the slice stays in L2 between the batches).  Every non-zero key finds by a lower bound how many
//      thresholds it exceeds and whether it starts a run of equal thresholds, and counts into two arrays of LDS integer bins;
//      a suffix sum over the first turns "keys above exactly the first b + 1 thresholds" into "keys above threshold i".  The
//      batch's entries then look their own key up in the sorted array and add their bins to the outputs with integer atomics.
//      Keys below the smallest admissible threshold -- nearly all of them when the model ranks the held-out items high -- leave
//      after one comparison.  The first batch also counts the slice's non-zero keys into n_adm.
//   4. ranks_summary_kernel (its own entry point): one wave per user, the per-user numbers from the counts in double.
// The only atomics are integer ones, so a repeated call returns the same bits.
#include <algorithm>

#include "../../include/rsparse_wrmf_hip.h"
#include "wrmf_internal.h"
#include "wrmf_device.h"

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kRankT = RSPARSE_HIP_RANKS_BATCH;     // thresholds per batch (a power of two: the bitonic sort's width; 4 bins per thread)
static_assert(kRankT == 1024, "ranks_count_kernel: 256 threads own four bins each");
constexpr size_t kRankWorkspaceWords = (size_t)1 << 29;   // 2 GiB, as lg_plan (wrmf_topk_large.hip)
constexpr int kRankMaxChunk = 32768;
constexpr int kSumWaves = 4;                        // users (waves) per workgroup of the summary kernel

// key of the held-out item `it` in the user's row: 0 (inadmissible) for an index outside the items too
__device__ __forceinline__ unsigned held_key(const unsigned* row, int n_items, int it) {
  return (it >= 0 && it < n_items) ? row[it] : 0u;
}

__global__ __launch_bounds__(256) void ranks_init_kernel(const unsigned* __restrict__ keys, size_t ld, int n_items,
                                                         const int32_t* __restrict__ act_ptr, const int32_t* __restrict__ act_idx,
                                                         int32_t* __restrict__ above, int32_t* __restrict__ tied) {
  const int u = blockIdx.x;
  const unsigned* row = keys + (size_t)u * ld;
  const int p1 = act_ptr[u], p2 = act_ptr[u + 1];
  for (int e = p1 + threadIdx.x; e < p2; e += 256) {
    const bool adm = held_key(row, n_items, act_idx[e]) != 0u;
    above[e] = adm ? 0 : -1;
    tied[e] = -1;
  }
}

// first position in t[lo, hi) (ascending) whose value is >= k
__device__ __forceinline__ int lower_bound(const unsigned* t, int lo, int hi, unsigned k) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void ranks_count_kernel(const unsigned* __restrict__ keys, size_t ld, int n_items, int slice_items,
                                                          const int32_t* __restrict__ act_ptr, const int32_t* __restrict__ act_idx,
                                                          int32_t* __restrict__ above, int32_t* __restrict__ tied,
                                                          int32_t* __restrict__ n_adm) {
  __shared__ unsigned s_own[kRankT];   // the batch's keys in the order of the entries
  __shared__ unsigned s_thr[kRankT];   // ... sorted ascending
  __shared__ int s_gt[kRankT];         // bin b: keys above exactly the thresholds 0..b; after the suffix sum: keys above threshold b
  __shared__ int s_eq[kRankT];         // bin b: keys equal to the run of thresholds that starts at b
  __shared__ int s_w[4];
  const int u = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned* row = keys + (size_t)u * ld;
  const int lo = blockIdx.x * slice_items, hi = min(n_items, lo + slice_items);
  const int p1 = act_ptr[u], n_held = max(act_ptr[u + 1] - p1, 0);
  for (int b0 = 0; b0 == 0 || b0 < n_held; b0 += kRankT) {
    const int nb = min(kRankT, n_held - b0);
    int P = 1;
    while (P < nb) P <<= 1;
    for (int e = tid; e < P; e += 256) {
      const unsigned k = e < nb ? held_key(row, n_items, act_idx[p1 + b0 + e]) : 0xffffffffu;   // (the padding sorts last)
      s_own[e] = k;
      s_thr[e] = k;
      s_gt[e] = 0;
      s_eq[e] = 0;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int i = tid; i < P / 2; i += 256) {
          const int a = 2 * i - (i & (stride - 1)), b = a + stride;
          const unsigned ka = s_thr[a], kb = s_thr[b];
          if (((a & size) == 0) == (kb < ka)) {
            s_thr[a] = kb;
            s_thr[b] = ka;
          }
        }
        __syncthreads();
      }
    const int n0 = lower_bound(s_thr, 0, nb, 1u);   // the inadmissible entries (key 0) sort first
    const bool any = n0 < nb;
    const unsigned tmin = any ? s_thr[n0] : 0u;
    int na = 0, run_bin = -1, run_cnt = 0;   // (consecutive keys of one bin -- a lone threshold -- cost one atomic)
    for (int i = lo + 4 * tid; i < hi; i += 1024) {
      const uint4 q = *reinterpret_cast<const uint4*>(row + i);
      const unsigned kv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const unsigned k = kv[j];
        if (i + j >= hi || k == 0u) continue;
        na++;
        if (!any || k < tmin) continue;
        const int pos = lower_bound(s_thr, n0, nb, k);
        if (pos < nb && s_thr[pos] == k) atomicAdd(&s_eq[pos], 1);
        if (pos > n0) {
          if (pos - 1 != run_bin) {
            if (run_cnt) atomicAdd(&s_gt[run_bin], run_cnt);
            run_bin = pos - 1;
            run_cnt = 0;
          }
          run_cnt++;
        }
      }
    }
    if (run_cnt) atomicAdd(&s_gt[run_bin], run_cnt);
    if (b0 == 0) {
      for (int o = 32; o > 0; o >>= 1) na += __shfl_xor(na, o);
      if (lane == 0 && na) atomicAdd(&n_adm[u], na);
    }
    __syncthreads();
    // inclusive suffix sum of s_gt[0, P): thread t owns the bins 4t .. 4t + 3
    int v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = 4 * tid + j < P ? s_gt[4 * tid + j] : 0;
    v[2] += v[3];
    v[1] += v[2];
    v[0] += v[1];
    int incl = v[0];   // over the lanes above, then the waves above
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_down(incl, o);
      if (lane + o < 64) incl += t;
    }
    if (lane == 0) s_w[wv] = incl;
    __syncthreads();
    int off = incl - v[0];
    for (int w = wv + 1; w < 4; w++) off += s_w[w];
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (4 * tid + j < P) s_gt[4 * tid + j] = v[j] + off;
    __syncthreads();
    for (int e = tid; e < nb; e += 256) {
      const unsigned k = s_own[e];
      if (k == 0u) continue;
      const int pos = lower_bound(s_thr, n0, nb, k);   // the start of the entry's run of equal keys
      const int g = s_gt[pos], q = s_eq[pos];
      if (g) atomicAdd(&above[p1 + b0 + e], g);
      if (q) atomicAdd(&tied[p1 + b0 + e], q);
    }
    __syncthreads();   // (the arrays are reused by the next batch)
  }
}

// One wave per user.  Lane l takes the user's positions l, l + 64, ... in order, then a butterfly over the wave: a fixed order,
// so a call repeats bit for bit.  r = above + tied / 2 is exact in double.
__global__ __launch_bounds__(64 * kSumWaves) void ranks_summary_kernel(int n_users, const int32_t* __restrict__ P,
                                                                       const double* __restrict__ X,
                                                                       const int32_t* __restrict__ above,
                                                                       const int32_t* __restrict__ tied,
                                                                       const int32_t* __restrict__ n_adm, double* __restrict__ mpr,
                                                                       double* __restrict__ auc, double* __restrict__ mrr,
                                                                       double* __restrict__ sums) {
  const int lane = threadIdx.x & 63, u = blockIdx.x * kSumWaves + (threadIdx.x >> 6);
  if (u >= n_users) return;   // (whole waves)
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int na = n_adm[u];
  const double denom = (double)na - 1.0;
  double sw = 0.0, swp = 0.0, sr = 0.0, rmin = INFINITY;
  int cnt = 0;
  for (int e = P[u] + lane; e < P[u + 1]; e += 64) {
    const int a = above[e];
    if (a < 0) continue;
    const double r = (double)a + 0.5 * (double)tied[e];
    const double w = X ? X[e] : 0.0;
    sw += w;
    swp += w * (na > 1 ? r / denom : nan);
    sr += r;
    rmin = fmin(rmin, r);
    cnt++;
  }
  sw = butterfly_sum(sw);
  swp = butterfly_sum(swp);
  sr = butterfly_sum(sr);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    rmin = fmin(rmin, __shfl_xor(rmin, o));
    cnt += __shfl_xor(cnt, o);
  }
  if (lane != 0) return;
  const double Pd = (double)cnt;
  if (mpr) mpr[u] = (cnt == 0 || sw == 0.0) ? nan : swp / sw;
  if (auc) auc[u] = (cnt == 0 || na == cnt) ? nan : 1.0 - (sr - Pd * (Pd - 1.0) * 0.5) / (Pd * (double)(na - cnt));
  if (mrr) mrr[u] = cnt == 0 ? nan : 1.0 / (1.0 + rmin);
  if (sums) {
    sums[3 * (size_t)u] = sw;
    sums[3 * (size_t)u + 1] = swp;
    sums[3 * (size_t)u + 2] = Pd;
  }
}

struct RankPlan {
  int chunk;    // users per chunk
  size_t ld;    // key row stride (a multiple of 4)
};

RankPlan rank_plan(int n_users, int n_items, int max_chunk_users) {
  RankPlan p;
  p.ld = ((size_t)std::max(n_items, 1) + 3) / 4 * 4;
  size_t c = kRankWorkspaceWords / p.ld;
  if (c > 256) c = c / 256 * 256;
  c = std::min<size_t>({c, (size_t)kRankMaxChunk, (size_t)std::max(n_users, 1)});
  if (max_chunk_users > 0) c = std::min<size_t>(c, (size_t)max_chunk_users);
  p.chunk = (int)std::max<size_t>(1, c);
  return p;
}

}  // namespace

size_t held_out_ranks_ws_floats(int n_users, int n_items, int max_chunk_users, int* chunk_users) {
  const RankPlan p = rank_plan(n_users, n_items, max_chunk_users);
  if (chunk_users) *chunk_users = p.chunk;
  return (size_t)p.chunk * p.ld + 64;
}

hipError_t launch_held_out_ranks(const float* U, const float* V, int n_users, int n_items, int rank, const int32_t* nr_ptr,
                                 const int32_t* nr_idx, const int32_t* excl, int n_excl, const int32_t* act_ptr,
                                 const int32_t* act_idx, int max_chunk_users, int32_t* above, int32_t* tied, int32_t* n_adm,
                                 hipStream_t s, float* ws) {
  if (n_users <= 0) return hipSuccess;
  if (rank < 1 || rank > 256 || n_items < 0 || !ws || !act_ptr || !act_idx || !above || !tied || !n_adm) return hipErrorInvalidValue;
  if (rank <= 128 && !padded_rank(rank)) return hipErrorInvalidValue;
  const RankPlan p = rank_plan(n_users, n_items, max_chunk_users);
  unsigned* keys = reinterpret_cast<unsigned*>(ws);
  hipError_t err;
  if ((err = hipMemsetAsync(n_adm, 0, (size_t)n_users * 4, s)) != hipSuccess) return err;
  for (int c0 = 0; c0 < n_users; c0 += p.chunk) {
    const int nu = std::min(p.chunk, n_users - c0);
    const int32_t* ap = act_ptr + c0;   // (absolute slots into act_idx / above / tied: a chunk passes its slice of the pointers)
    if (n_items > 0) {
      if ((err = launch_topl_score(U + (size_t)c0 * rank, V, nu, n_items, rank, keys, p.ld, s)) != hipSuccess) return err;
      if (nr_ptr || n_excl > 0)
        if ((err = launch_topl_mask(keys, p.ld, n_items, nu, nr_ptr ? nr_ptr + c0 : nullptr, nr_idx, excl, n_excl, s)) != hipSuccess)
          return err;
    }
    hipLaunchKernelGGL(ranks_init_kernel, dim3(nu), dim3(256), 0, s, keys, p.ld, n_items, ap, act_idx, above, tied);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    if (n_items > 0) {
      // slices of the rows as the large-k path cuts them: about 4096 workgroups, a multiple of 1024 keys each
      const int max_sl = std::max(1, (n_items + 4095) / 4096);
      const int nsl = std::max(1, std::min(max_sl, (4096 + nu - 1) / nu));
      const int sl = ((n_items + nsl - 1) / nsl + 1023) / 1024 * 1024;
      hipLaunchKernelGGL(ranks_count_kernel, dim3((n_items + sl - 1) / sl, nu), dim3(256), 0, s, keys, p.ld, n_items, sl, ap, act_idx,
                         above, tied, n_adm + c0);
      if ((err = hipGetLastError()) != hipSuccess) return err;
    }
  }
  return hipSuccess;
}

hipError_t launch_rank_summary(int n_users, const int32_t* act_ptr, const double* act_x, const int32_t* above, const int32_t* tied,
                               const int32_t* n_adm, double* mpr, double* auc, double* mrr, double* sums, hipStream_t s) {
  if (n_users <= 0) return hipSuccess;
  hipLaunchKernelGGL(ranks_summary_kernel, dim3((unsigned)((n_users + kSumWaves - 1) / kSumWaves)), dim3(64 * kSumWaves), 0, s, n_users,
                     act_ptr, act_x, above, tied, n_adm, mpr, auc, mrr, sums);
  return hipGetLastError();
}

}  // namespace rsparse_hip
