// top-k WITHIN per-user candidate lists: the k best items of every user among the stored positions of a CSR pattern -- what the
// reference's find_top_product returns (R/utils.R:31-59 -> src/matrix_top_product.cpp:20-102) when every item outside the user's
// candidate row is added to the user's not_recommend row.  gfx950, wave64.  Work and memory follow the number of candidates, not
// users x items.
//
//   1. scores: launch_score_pairs (wrmf_score.hip) on the candidate pattern, position-parallel, the double sum plus the global
//      bias, 8 bytes per candidate in the workspace.  Not forked: the scores are those of rsparse_hip_score_pairs*_device, bit
//      for bit.
//   2. cand_keys_kernel, position-parallel: every score becomes its order key f64_key(score + 0.0) IN PLACE (-0 and +0 tie), and
//      a wave writes the 64 admissibility bits of its 64 consecutive positions as one word (a ballot): a position is inadmissible
//      when its item is in the user's not_recommend row or in the exclusion list (both sorted: one binary search each).  The bit,
//      not a sentinel key, says what takes part: no real score can collide with it.
//   3. cand_plan_kernel: the rows by length class into one list, short rows (at most 64 candidates) from the front, the others
//      from the back, counted on the device.  The select launches walk their part of the list: neither is sized by the longest
//      row, and no row waits behind a row of another class.
//   4. cand_short_kernel, a wave per row, four rows per workgroup: a lane holds one candidate (key, item, admissible) in registers
//      and ranks it by counting the admissible candidates that order before it (64 lane reads, no LDS).  The k boundary in closed
//      form (below) on ballot masks: candidates of a row are in ascending item order, so "the first k of A u G in item order" is
//      the first k set bits.
//      cand_long_kernel, a workgroup per row: the keys stay in the workspace (L2) and are read once per radix pass through the
//      key function of dev::block_kth_largest -> v_k; two counts -> |A|, |G|; the two index selects of topl_order_kernel ->
//      cut_lo / cut_hi; the kk <= 8192 survivors compacted into LDS (12 bytes each) and ordered by dev::block_bitonic.  A row of
//      at most 2048 candidates is staged in LDS first (one read of the workspace, its loads in flight together) and the same
//      code reads it from there: the passes of a row of 1000 were bound by the latency of their dependent L2 reads.
//
// The k boundary (wrmf_topk_large.hip has the derivation from the reference's heap): with v_k the kk-th best admissible score,
// A the admissible items strictly above it and G those equal to it, the result is all of A plus the m = kk - |A| LARGEST indices
// among the G items that fall into the first kk of A u G in ascending item order; output best first, equal scores with the larger
// index first.  Exactly kk = min(k, admissible) entries survive whatever the row length or the number of ties: no candidate cap,
// no overflow path, nothing approximate.  Integer keys and a fixed-order double sum: a call repeats bit for bit, and a row's
// result does not depend on its class (both classes evaluate the same definition on the same keys).
#include <algorithm>

#include "wrmf_internal.h"
#include "wrmf_device.h"

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kCandShort = 64;   // rows up to this many candidates: one wave, one candidate per lane
constexpr int kCandStage = 2048;   // longer rows up to this many: staged in LDS once (24 KB), the select reads LDS

__device__ __forceinline__ bool cand_ok(const u64* __restrict__ mask, unsigned t) { return (mask[t >> 6] >> (t & 63u)) & 1ull; }

// is `it` in the ascending list a[lo, hi)?
__device__ __forceinline__ bool sorted_has(const int32_t* __restrict__ a, int lo, int hi, int it) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int v = a[mid];
    if (v == it) return true;
    if (v < it) lo = mid + 1;
    else hi = mid;
  }
  return false;
}

// P shifted so that it starts at 0 (a caller's slice of a larger pattern's row pointers)
__global__ __launch_bounds__(256) void cand_rebase_kernel(const int32_t* __restrict__ P, int n_rows, int32_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i <= n_rows) out[i] = P[i] - P[0];
}

// ---- 2. keys and admissibility bits (sk: the scores on entry, their keys on exit) --------------------------------------------
__global__ __launch_bounds__(256) void cand_keys_kernel(u64* __restrict__ sk, u64* __restrict__ mask, unsigned nnz,
                                                        const int32_t* __restrict__ P, int n_rows, const int32_t* __restrict__ J,
                                                        const int32_t* __restrict__ nr_ptr, const int32_t* __restrict__ nr_idx,
                                                        const int32_t* __restrict__ excl, int n_excl) {
  const int lane = threadIdx.x & 63;
  const unsigned words = (nnz + 63u) >> 6;
  const unsigned w0 = blockIdx.x * 4u + (threadIdx.x >> 6), nw = gridDim.x * 4u;
  for (unsigned w = w0; w < words; w += nw) {   // (whole waves: the ballot below needs every lane)
    const unsigned t = (w << 6) + (unsigned)lane;
    bool ok = t < nnz;
    if (ok) {
      sk[t] = f64_key(__longlong_as_double((long long)sk[t]) + 0.0);
      const int it = J[t];
      if (n_excl > 0 && sorted_has(excl, 0, n_excl, it)) ok = false;
      if (ok && nr_ptr) {
        int lo = 0, hi = n_rows;   // P[lo] <= t < P[hi]: the row of position t
        while (hi - lo > 1) {
          const int mid = lo + ((hi - lo) >> 1);
          if ((unsigned)P[mid] <= t) lo = mid;
          else hi = mid;
        }
        if (sorted_has(nr_idx, nr_ptr[lo], nr_ptr[lo + 1], it)) ok = false;
      }
    }
    const u64 m = __ballot(ok);
    if (lane == 0) mask[w] = m;
  }
}

// ---- 3. the rows by class: list[0, cnt[0]) the short rows, list[n_rows - cnt[1], n_rows) the others --------------------------
__global__ __launch_bounds__(256) void cand_plan_kernel(const int32_t* __restrict__ P, int n_rows, int32_t* __restrict__ list,
                                                        int* __restrict__ cnt) {
  const int row = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const bool in = row < n_rows;
  const int len = in ? P[row + 1] - P[row] : 0;
  const bool is_short = in && len <= kCandShort, is_long = in && len > kCandShort;
  const u64 ms = __ballot(is_short), ml = __ballot(is_long);
  const u64 below = (1ull << lane) - 1ull;
  int bs = 0, bl = 0;
  if (lane == 0) {   // one atomic per wave and class
    if (ms) bs = atomicAdd(&cnt[0], __popcll(ms));
    if (ml) bl = atomicAdd(&cnt[1], __popcll(ml));
  }
  bs = __shfl(bs, 0);
  bl = __shfl(bl, 0);
  if (is_short) list[bs + __popcll(ms & below)] = row;
  if (is_long) list[n_rows - 1 - (bl + __popcll(ml & below))] = row;
}

// ---- 4a. short rows: a wave per row ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cand_short_kernel(const u64* __restrict__ keys, const u64* __restrict__ mask,
                                                         const int32_t* __restrict__ P, const int32_t* __restrict__ J,
                                                         const int32_t* __restrict__ list, const int* __restrict__ cnt, int topk,
                                                         int32_t* __restrict__ res, double* __restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const int w0 = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
  const int n_short = cnt[0];
  const u64 above_me = lane == 63 ? 0ull : (~0ull << (lane + 1)), below_me = (1ull << lane) - 1ull;
  for (int i = w0; i < n_short; i += nw) {   // (whole waves)
    const int row = rfl(list[i]);
    const int base = rfl(P[row]), len = min(rfl(P[row + 1]) - base, kCandShort);
    u64 key = 0ull;
    int it = -1;
    bool ok = false;
    if (lane < len) {
      const unsigned t = (unsigned)(base + lane);
      key = keys[t];
      it = J[t];
      ok = cand_ok(mask, t);
    }
    const u64 mok = __ballot(ok);
    const int kk = min(topk, (int)__popcll(mok));
    // the admissible candidates that order before this one: a larger key, or the same key and a larger item (a later lane)
    const int klo = (int)(unsigned)key, khi = (int)(unsigned)(key >> 32);
    int before = 0;
    for (int m = 0; m < len; m++) {
      const u64 km = ((u64)(unsigned)__builtin_amdgcn_readlane(khi, m) << 32) | (u64)(unsigned)__builtin_amdgcn_readlane(klo, m);
      const bool okm = (mok >> m) & 1ull;
      before += (okm && (km > key || (km == key && m > lane))) ? 1 : 0;
    }
    int32_t* ru = res + (size_t)row * topk;
    double* su = scores + (size_t)row * topk;
    if (kk > 0) {
      const int src = __builtin_ctzll(__ballot(ok && before == kk - 1)) & 63;   // holds v_k
      const u64 vk = ((u64)(unsigned)__builtin_amdgcn_readlane(khi, src) << 32) | (u64)(unsigned)__builtin_amdgcn_readlane(klo, src);
      const bool isA = ok && key > vk, isG = ok && key == vk;
      const u64 mA = __ballot(isA), mG = __ballot(isG);
      const int g = __popcll(mA), nt = __popcll(mG);
      // t = the G items among the first kk of A u G in item (= lane) order; the m = kk - |A| largest of them stay
      const bool in_first = g + nt <= kk || (int)__popcll((mA | mG) & below_me) < kk;
      const u64 mT = __ballot(isG && in_first);
      const bool keepG = isG && in_first && (int)__popcll(mT & above_me) < kk - g;
      const u64 mK = __ballot(keepG);
      if (isA || keepG) {
        const int pos = isA ? before : g + (int)__popcll(mK & above_me);
        ru[pos] = it + 1;   // 1-based, like R
        su[pos] = key_f64(key);
      }
    }
    for (int p = kk + lane; p < topk; p += 64) {
      ru[p] = INT32_MIN;   // NA_integer_ / NA_real_
      su[p] = __longlong_as_double(0x7ff8000000000000ll);
    }
  }
}

// ---- 4b. all other rows: a workgroup per row --------------------------------------------------------------------------------------
// sum of v over the 256 threads, in every thread.  Uses sw[4].
__device__ __forceinline__ int block_sum(int v, int* sw) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
  __syncthreads();
  const int tot = sw[0] + sw[1] + sw[2] + sw[3];
  __syncthreads();
  return tot;
}

// a row as the select reads it: from the workspace (keys, admissibility bits) and the pattern, or staged in LDS
struct CandGlobalRow {
  const u64* rk;
  const int32_t* rj;
  const u64* mask;
  unsigned base;
  __device__ __forceinline__ bool ok(int e) const { return cand_ok(mask, base + e); }
  __device__ __forceinline__ u64 key(int e) const { return rk[e]; }
  __device__ __forceinline__ int item(int e) const { return rj[e]; }
};
struct CandLdsRow {   // (an inadmissible entry holds item -1)
  const u64* lk;
  const int* li;
  __device__ __forceinline__ bool ok(int e) const { return li[e] >= 0; }
  __device__ __forceinline__ u64 key(int e) const { return lk[e]; }
  __device__ __forceinline__ int item(int e) const { return li[e]; }
};

// the best min(topk, admissible) entries of a row of n, ordered, to ru / su (all 256 threads)
template <class Row>
__device__ __forceinline__ void cand_order_row(const Row row, int n, int topk, int P2, u64* sk, int* si, unsigned* hist, u64* sres,
                                               int* sint, int32_t* ru, double* su) {
  const int tid = threadIdx.x;
  int c = 0;
  for (int e = tid; e < n; e += 256) c += row.ok(e) ? 1 : 0;
  const int kk = min(topk, block_sum(c, sint + 4));
  if (kk <= 0) {   // (uniform)
    topl_emit(sk, si, 0, topk, 0.0, ru, su);
    return;
  }
  // v_k, |A| (g) and |G| (nt)
  const u64 vk = block_kth_largest(n, kk, 64, [&](int e, bool& ok) { ok = row.ok(e); return row.key(e); }, hist, sres, sint);
  int ca = 0, cg = 0;
  for (int e = tid; e < n; e += 256)
    if (row.ok(e)) {
      const u64 k = row.key(e);
      ca += k > vk ? 1 : 0;
      cg += k == vk ? 1 : 0;
    }
  const int g = block_sum(ca, sint + 4), nt = block_sum(cg, sint + 4);
  int cut_hi = 0x7fffffff, cut_lo = -1;   // the G items kept: cut_lo <= item <= cut_hi
  if (g + nt > kk) {
    // c = the kk-th smallest item of A u G (the last of the first kk in ascending order) ...
    const u64 cc = block_kth_largest(n, kk, 32, [&](int e, bool& ok) { ok = row.ok(e) && row.key(e) >= vk; return (u64)(0xffffffffu - (unsigned)row.item(e)); },
                                     hist, sres, sint);
    cut_hi = (int)(0xffffffffu - (unsigned)cc);
    // ... t = the G items up to it; keep the m = kk - |A| largest of them
    cut_lo = (int)block_kth_largest(n, kk - g, 32, [&](int e, bool& ok) { ok = row.ok(e) && row.key(e) == vk && row.item(e) <= cut_hi; return (u64)(unsigned)row.item(e); },
                                    hist, sres, sint);
  }
  // the kk survivors into LDS
  int dst0 = 0, tot;
  for (int c0 = 0; c0 < n; c0 += 256) {
    const int e = c0 + tid;
    u64 k = 0;
    int ix = -1;
    bool keep = false;
    if (e < n && row.ok(e)) {
      k = row.key(e);
      ix = row.item(e);
      keep = k > vk || (k == vk && ix >= cut_lo && ix <= cut_hi);
    }
    const int off = block_prefix(keep, sint + 4, &tot);
    if (keep && dst0 + off < P2) {   // (dst0 + off < kk <= P2 by the closed form; the bound keeps a broken precondition in LDS)
      sk[dst0 + off] = k;
      si[dst0 + off] = ix;
    }
    dst0 += tot;
  }
  const int PP = pow2_at_least(kk);   // <= P2
  for (int e = kk + tid; e < PP; e += 256) {
    sk[e] = 0ull;
    si[e] = -1;
  }
  __syncthreads();
  block_bitonic(sk, si, PP, false);
  topl_emit(sk, si, kk, topk, 0.0, ru, su);
}

// LDS: sk[P2] keys, lk[kCandStage] staged keys, sres, hist[256], sint[12], si[P2] items, li[kCandStage] staged items; P2 = the
// power of two at or above topk.  A row of at most kCandStage candidates is read from the workspace ONCE, all its loads in
// flight together, and the select's passes read LDS; a longer row is read from L2 in every pass.
__global__ __launch_bounds__(256) void cand_long_kernel(const u64* __restrict__ keys, const u64* __restrict__ mask,
                                                        const int32_t* __restrict__ P, const int32_t* __restrict__ J,
                                                        const int32_t* __restrict__ list, const int* __restrict__ cnt, int n_rows,
                                                        int topk, int P2, int32_t* __restrict__ res, double* __restrict__ scores) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u64* sk = reinterpret_cast<u64*>(smem);
  u64* lk = sk + P2;
  u64* sres = lk + kCandStage;
  unsigned* hist = reinterpret_cast<unsigned*>(sres + 1);   // [256]
  int* sint = reinterpret_cast<int*>(hist + 256);           // [12]: [0] block_kth_largest, [4..7] block_prefix / block_sum
  int* si = sint + 12;
  int* li = si + P2;
  const int tid = threadIdx.x;
  const int n_long = cnt[1];
  for (int i = blockIdx.x; i < n_long; i += gridDim.x) {
    const int row = list[n_rows - 1 - i];
    const unsigned base = (unsigned)P[row];
    const int n = P[row + 1] - (int)base;
    int32_t* ru = res + (size_t)row * topk;
    double* su = scores + (size_t)row * topk;
    if (n <= kCandStage) {   // (uniform)
      constexpr int NS = kCandStage / 256;
      u64 k[NS];
      int it[NS];
#pragma unroll
      for (int q = 0; q < NS; q++) {
        const int e = q * 256 + tid;
        k[q] = 0ull;
        it[q] = -1;
        if (e < n) {
          k[q] = keys[base + e];
          it[q] = cand_ok(mask, base + e) ? J[base + e] : -1;
        }
      }
#pragma unroll
      for (int q = 0; q < NS; q++) {
        const int e = q * 256 + tid;
        if (e < n) {
          lk[e] = k[q];
          li[e] = it[q];
        }
      }
      __syncthreads();
      cand_order_row(CandLdsRow{lk, li}, n, topk, P2, sk, si, hist, sres, sint, ru, su);
    } else {
      cand_order_row(CandGlobalRow{keys + base, J + base, mask, base}, n, topk, P2, sk, si, hist, sres, sint, ru, su);
    }
    __syncthreads();   // the next row reuses the LDS
  }
}

int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
    cus = 256;
  return cus;
}

size_t align8(size_t b) { return (b + 7) / 8 * 8; }

int pow2_host(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

}  // namespace

size_t top_candidates_ws_bytes(int n_users, int64_t nnz) {
  const size_t n = (size_t)std::max(n_users, 0), z = (size_t)std::max<int64_t>(nnz, 0);
  return 8 * z + 8 * ((z + 63) / 64) + align8(4 * n) + 16 + align8(4 * (n + 1)) + 64;
}

template <class T>
hipError_t launch_top_candidates(const T* U, const T* V, int n_users, int n_items, int rank, int topk, const int32_t* cand_p,
                                 const int32_t* cand_j, int32_t p0, int64_t nnz, const int32_t* nr_ptr, const int32_t* nr_idx,
                                 const int32_t* excl, int n_excl, double glob_mean, int32_t* res, double* scores, hipStream_t s,
                                 void* ws) {
  if (n_users <= 0) return hipSuccess;
  if (topk < 1 || topk > kTopLargeMax || rank < 1 || rank > 256 || nnz < 0 || nnz > 0x7fffffffll || !ws) return hipErrorInvalidValue;
  static const int cus = device_cus();
  const size_t z = (size_t)nnz;
  char* w = static_cast<char*>(ws);
  double* sc = reinterpret_cast<double*>(w);
  u64* mask = reinterpret_cast<u64*>(w + 8 * z);
  int32_t* list = reinterpret_cast<int32_t*>(w + 8 * z + 8 * ((z + 63) / 64));
  int* cnt = reinterpret_cast<int*>(reinterpret_cast<char*>(list) + align8(4 * (size_t)n_users));
  int32_t* pz = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(cnt) + 16);
  hipError_t err;
  const int32_t* P = cand_p;
  const int32_t* J = cand_j;
  if (p0 != 0) {   // a slice of a larger pattern's row pointers: the same rows from position 0
    hipLaunchKernelGGL(cand_rebase_kernel, dim3((unsigned)(n_users / 256 + 1)), dim3(256), 0, s, cand_p, n_users, pz);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    P = pz;
    J = cand_j + p0;
  }
  if ((err = hipMemsetAsync(cnt, 0, 16, s)) != hipSuccess) return err;
  if (nnz > 0) {
    if ((err = launch_score_pairs(U, V, n_users, n_items, rank, P, J, glob_mean, sc, s)) != hipSuccess) return err;
    const long long words = ((long long)nnz + 63) / 64;
    const unsigned kg = (unsigned)std::min<long long>((words + 3) / 4, (long long)cus * 32);
    hipLaunchKernelGGL(cand_keys_kernel, dim3(kg), dim3(256), 0, s, reinterpret_cast<u64*>(sc), mask, (unsigned)nnz, P, n_users, J, nr_ptr, nr_idx, excl,
                       excl ? n_excl : 0);
    if ((err = hipGetLastError()) != hipSuccess) return err;
  }
  hipLaunchKernelGGL(cand_plan_kernel, dim3((unsigned)((n_users + 255) / 256)), dim3(256), 0, s, P, n_users, list, cnt);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  const u64* keys = reinterpret_cast<const u64*>(sc);
  const unsigned sg = (unsigned)std::min((n_users + 3) / 4, cus * 16);
  hipLaunchKernelGGL(cand_short_kernel, dim3(sg), dim3(256), 0, s, keys, mask, P, J, list, cnt, topk, res, scores);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  if (nnz > kCandShort) {   // (otherwise no row is long)
    const int P2 = pow2_host(topk);
    const size_t lds = ((size_t)P2 + kCandStage) * 12 + 8 + 256 * 4 + 12 * 4;
    if ((err = hipFuncSetAttribute(reinterpret_cast<const void*>(cand_long_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) !=
        hipSuccess)
      return err;
    const unsigned lg = (unsigned)std::min((long long)n_users, std::min((long long)cus * 16, (long long)nnz / (kCandShort + 1)));
    hipLaunchKernelGGL(cand_long_kernel, dim3(std::max(lg, 1u)), dim3(256), lds, s, keys, mask, P, J, list, cnt, n_users, topk, P2, res,
                       scores);
    if ((err = hipGetLastError()) != hipSuccess) return err;
  }
  return hipSuccess;
}
template hipError_t launch_top_candidates<float>(const float*, const float*, int, int, int, int, const int32_t*, const int32_t*, int32_t,
                                                 int64_t, const int32_t*, const int32_t*, const int32_t*, int, double, int32_t*, double*,
                                                 hipStream_t, void*);
template hipError_t launch_top_candidates<double>(const double*, const double*, int, int, int, int, const int32_t*, const int32_t*, int32_t,
                                                  int64_t, const int32_t*, const int32_t*, const int32_t*, int, double, int32_t*, double*,
                                                  hipStream_t, void*);

}  // namespace rsparse_hip
