// top-k of the dense product for 256 < k <= 8192 (RSPARSE_HIP_MAX_TOPK_LARGE), gfx950, wave64.
//
// The fused kernels of wrmf_topk.hip keep every user's candidates in LDS (or a per-workgroup slot) sized by k, and settle them
// with a per-wave radix select over at most 576 entries: none of that scales to thousands of items per user.  This path keeps
// no state that grows with k while it scans the items.  Per chunk of users (sized so that the workspace stays under 2 GiB):
//   1. topl_score_kernel: scores = U V^T on the matrix cores (v_mfma_f32_32x32x2_f32, the exact fp32 product of the fused
//      path), every score mapped to an order-preserving 32-bit key and written to a global key matrix [users][items];
//      topl_mask_kernel then zeroes the keys of the user's not_recommend row and of the excluded items (0 sorts below every
//      admissible key).
//   2. topl_hist_kernel / topl_resolve_kernel, three times: the kc-th largest admissible key of every user by a radix select
//      on 11 + 11 + 10 bits -- a workgroup histograms one slice of one user's row in LDS and adds it to the user's global
//      histogram, so one user over a million items is read by a few hundred workgroups, not by one CU.
//   3. topl_compact_kernel: every item whose key is >= the kc-th key -- every item tied at it included -- into a bounded
//      per-user list (idx, key).  kc = min(k + extra, admissible items).
//   4. topl_order_kernel: one workgroup per user re-scores its list in double (f64 form) or decodes the fp32 keys (fp32 form)
//      and applies the reference heap's result in closed form (below), then sorts the k survivors in LDS (bitonic).
//      A user whose list overflowed (ties: a zero embedding ties every item) is left to topl_heap_kernel, which replays the
//      reference's heap itself over the user's items at or above the kc-th key in ascending item order.
//
// The reference (src/matrix_top_product.cpp:66-95) pushes the items in ascending order into a min-heap of (score, index) pairs
// that replaces its top only on a strictly larger score, then pops the heap from the end.  Its result in closed form: let v_k
// be the k-th best score, A the items strictly above v_k and G the admissible items equal to v_k.  Items below v_k are smaller
// pairs than any of A u G -- they are evicted before any of them and never keep one out --, so the heap sees A u G alone: the
// first k of them in ascending item order fill it (t = the G items among those k), a later G item never enters (not strictly
// larger than the top), and every later A item evicts the smallest pair, i.e. the G item of smallest index still held.  So all
// of A is kept, plus the m = k - |A| LARGEST indices of t; output best first, equal scores with the larger index first.
#include <algorithm>

#include "wrmf_internal.h"
#include "wrmf_device.h"

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kLgMaxCand = 10240;          // the largest candidate list one workgroup orders in LDS (12 bytes an entry)
constexpr int kLgHistBins = 2048;          // bins of the global per-user histogram (11 bits)
constexpr size_t kLgWorkspaceWords = (size_t)1 << 29;   // 2 GiB: a chunk of users is sized to stay under it
constexpr int kLgMaxChunk = 32768;

__device__ __forceinline__ unsigned f32_key(float s) {
  const unsigned u = __float_as_uint(s + 0.f);   // (-0 -> +0: equal scores, equal keys)
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_f32(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// ---- 1. scores -> keys ------------------------------------------------------------------------------------------------------
// The four waves share a 32-item tile in LDS (the next tile's 16-byte loads fly during this tile's MFMAs) and own 32 UB users
// each as register-resident A operands; grid = (user blocks, item slices), user blocks fastest so that the workgroups reading
// the same item slice run together.  Lane (col, half) holds item `col` of the tile for the users (e & 3) + 8 (e >> 2) + 4 half:
// for one accumulator entry the wave writes 32 consecutive keys of two users (two 128-byte segments).
template <int KP, int UB, bool VEC>
__global__ __launch_bounds__(256) void topl_score_kernel(const float* __restrict__ U, const float* __restrict__ V, int n_users,
                                                         int n_items, int k_rank, int slice_items, unsigned* __restrict__ keys,
                                                         size_t ld) {
  constexpr int LDT = KP + 4, NK2 = KP / 2, USERS = 4 * 32 * UB, UPW = 32 * UB, NLD = KP / 32;
  __shared__ __attribute__((aligned(16))) float tile[32 * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wv = rfl(tid >> 6);
  const int col = lane & 31, half = lane >> 5;
  const int u0 = blockIdx.x * USERS, uw = wv * UPW;
  const int item_lo = blockIdx.y * slice_items, item_hi = min(n_items, item_lo + slice_items);
  float afrag[UB][NK2];
#pragma unroll
  for (int ub = 0; ub < UB; ub++) {
    const int u = u0 + uw + 32 * ub + col;
#pragma unroll
    for (int t = 0; t < NK2; t++) {
      const int kk = 2 * t + half;
      afrag[ub][t] = (u < n_users && kk < k_rank) ? U[(size_t)u * k_rank + kk] : 0.f;
    }
  }
  for (int e = tid; e < 32 * LDT; e += 256) tile[e] = 0.f;
  const int n_tiles = (item_hi - item_lo + 31) / 32;
  float4 pf[VEC ? NLD : 1];
  auto load_tile = [&](const int tl) {
    if constexpr (VEC) {
      const int i0 = item_lo + tl * 32;
#pragma unroll
      for (int j = 0; j < NLD; j++) {
        const int e4 = j * 256 + tid, it = e4 / (KP / 4), c4 = e4 % (KP / 4);
        pf[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tl < n_tiles && i0 + it < item_hi && 4 * c4 < k_rank)
          pf[j] = *reinterpret_cast<const float4*>(V + (size_t)(i0 + it) * k_rank + 4 * c4);
      }
    }
  };
  auto store_tile = [&](const int tl) {
    if constexpr (VEC) {
#pragma unroll
      for (int j = 0; j < NLD; j++) {
        const int e4 = j * 256 + tid, it = e4 / (KP / 4), c4 = e4 % (KP / 4);
        *reinterpret_cast<float4*>(tile + it * LDT + 4 * c4) = pf[j];
      }
    } else {   // any rank / alignment: scalar staging
      const int i0 = item_lo + tl * 32;
      for (int it = wv; it < 32; it += 4)
        for (int kk = lane; kk < k_rank; kk += 64)
          tile[it * LDT + kk] = (i0 + it < item_hi) ? V[(size_t)(i0 + it) * k_rank + kk] : 0.f;
    }
  };
  load_tile(0);
  for (int tl = 0; tl < n_tiles; tl++) {
    __syncthreads();   // every wave has read the previous tile (and the zero fill is done)
    store_tile(tl);
    __syncthreads();
    load_tile(tl + 1);
    f32x16 acc[UB];
#pragma unroll
    for (int ub = 0; ub < UB; ub++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[ub][e] = 0.f;
#pragma unroll
    for (int t = 0; t < NK2; t++) {
      const float b = tile[col * LDT + 2 * t + half];
#pragma unroll
      for (int ub = 0; ub < UB; ub++) acc[ub] = __builtin_amdgcn_mfma_f32_32x32x2f32(afrag[ub][t], b, acc[ub], 0, 0, 0);
    }
    const int item = item_lo + tl * 32 + col;
    if (item < item_hi) {
#pragma unroll
      for (int ub = 0; ub < UB; ub++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
          const int u = u0 + uw + 32 * ub + (e & 3) + 8 * (e >> 2) + 4 * half;
          if (u < n_users) keys[(size_t)u * ld + item] = f32_key(acc[ub][e]);
        }
    }
  }
}

// the user's not_recommend row and the globally excluded items: key 0, below every admissible key (one workgroup per user)
__global__ __launch_bounds__(256) void topl_mask_kernel(unsigned* __restrict__ keys, size_t ld, int n_items,
                                                        const int32_t* __restrict__ nr_ptr, const int32_t* __restrict__ nr_idx,
                                                        const int32_t* __restrict__ excl, int n_excl) {
  const int u = blockIdx.x;
  unsigned* row = keys + (size_t)u * ld;
  if (nr_ptr) {
    const int p1 = nr_ptr[u], p2 = nr_ptr[u + 1];
    for (int j = p1 + threadIdx.x; j < p2; j += 256) {
      const int it = nr_idx[j];
      if (it >= 0 && it < n_items) row[it] = 0u;
    }
  }
  for (int j = threadIdx.x; j < n_excl; j += 256) {
    const int it = excl[j];
    if (it >= 0 && it < n_items) row[it] = 0u;
  }
}

// ---- 2. the kc-th largest admissible key: radix select, 11 + 11 + 10 bits ---------------------------------------------------
// pass 0 histograms bits 21..31 of every admissible key (and counts them), pass 1 bits 10..20 of the keys whose top 11 bits are
// the chosen bin, pass 2 bits 0..9 of those whose top 22 bits are.  grid = (item slices, users): a slice is a multiple of 1024
// keys, read as 16-byte vectors (rows start 16-byte aligned: ld % 4 == 0).
__global__ __launch_bounds__(256) void topl_hist_kernel(const unsigned* __restrict__ keys, size_t ld, int n_items, int slice_items,
                                                        int pass, const unsigned* __restrict__ pref, unsigned* __restrict__ hist,
                                                        int* __restrict__ adm) {
  __shared__ unsigned h[kLgHistBins];
  __shared__ int s_adm;
  const int u = blockIdx.y, tid = threadIdx.x;
  const int nb = pass == 2 ? 1024 : 2048;
  const int shift = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
  const int pshift = pass == 1 ? 21 : 10;
  const unsigned p = pass ? pref[u] : 0u;
  if (pass && p == 0u) return;   // no admissible item (topl_resolve_kernel left the prefix at 0)
  for (int b = tid; b < nb; b += 256) h[b] = 0u;
  if (tid == 0) s_adm = 0;
  __syncthreads();
  const unsigned* row = keys + (size_t)u * ld;
  const int lo = blockIdx.x * slice_items, hi = min(n_items, lo + slice_items);
  int na = 0;
  for (int i = lo + 4 * tid; i < hi; i += 1024) {
    const uint4 q = *reinterpret_cast<const uint4*>(row + i);
    const unsigned kv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const unsigned k = kv[j];
      if (i + j < hi && k != 0u && (pass == 0 || (k >> pshift) == p)) {
        atomicAdd(&h[(k >> shift) & (unsigned)(nb - 1)], 1u);
        na++;
      }
    }
  }
  if (pass == 0) {
    for (int o = 32; o > 0; o >>= 1) na += __shfl_xor(na, o);
    if ((tid & 63) == 0 && na) atomicAdd(&s_adm, na);
  }
  __syncthreads();
  for (int b = tid; b < nb; b += 256)
    if (h[b]) atomicAdd(&hist[(size_t)u * kLgHistBins + b], h[b]);
  if (pass == 0 && tid == 0 && s_adm) atomicAdd(&adm[u], s_adm);
}

// One wave per user: the bin of the histogram that holds the rem-th largest key (bins walked from the top), appended to the
// prefix; the histogram row is cleared for the next pass.  pass 0 starts from rem = min(kc, admissible items).
__global__ __launch_bounds__(64) void topl_resolve_kernel(unsigned* __restrict__ hist, int pass, int kc, unsigned* __restrict__ pref,
                                                          int* __restrict__ rem, const int* __restrict__ adm) {
  const int u = blockIdx.x, lane = threadIdx.x;
  const int nb = pass == 2 ? 1024 : 2048, width = pass == 2 ? 10 : 11, per = nb / 64;
  unsigned* h = hist + (size_t)u * kLgHistBins;
  int r = pass == 0 ? min(kc, adm[u]) : rem[u];
  if (r <= 0) {
    if (pass == 0 && lane == 0) {
      pref[u] = 0u;
      rem[u] = 0;
    }
    return;
  }
  // lane l holds the bins nb-1-l*per .. nb-per-l*per (descending)
  unsigned s = 0;
  for (int j = 0; j < per; j++) s += h[nb - 1 - lane * per - j];
  unsigned incl = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  const unsigned excl = incl - s;
  const bool mine = excl < (unsigned)r && incl >= (unsigned)r;
  if (mine) {
    unsigned cum = excl;
    for (int j = 0; j < per; j++) {
      const int b = nb - 1 - lane * per - j;
      const unsigned c = h[b];
      if (cum + c >= (unsigned)r) {
        pref[u] = pass == 0 ? (unsigned)b : ((pref[u] << width) | (unsigned)b);
        rem[u] = r - (int)cum;
        break;
      }
      cum += c;
    }
  }
  wave_sync();
  for (int b = lane; b < nb; b += 64) h[b] = 0u;
}

// ---- 3. the candidates: every key >= the kc-th key ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void topl_compact_kernel(const unsigned* __restrict__ keys, size_t ld, int n_items, int slice_items,
                                                           const unsigned* __restrict__ thr, int* __restrict__ cnt, int cap,
                                                           int32_t* __restrict__ cidx, unsigned* __restrict__ ckey) {
  const int u = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const unsigned t = thr[u];
  if (t == 0u) return;
  const unsigned* row = keys + (size_t)u * ld;
  const int lo = blockIdx.x * slice_items, hi = min(n_items, lo + slice_items);
  for (int i0 = lo; i0 < hi; i0 += 1024) {
    const int i = i0 + 4 * tid;
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    if (i < hi) q = *reinterpret_cast<const uint4*>(row + i);
    const unsigned kv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const bool ok = i + j < hi && kv[j] >= t;
      const u64 m = __ballot(ok);
      if (m) {   // wave-uniform: one atomic per wave
        int base = 0;
        if (lane == __builtin_ctzll(m)) base = atomicAdd(&cnt[u], __popcll(m));
        base = __shfl(base, __builtin_ctzll(m));
        if (ok) {
          const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
          if (pos < cap) {
            cidx[(size_t)u * cap + pos] = i + j;
            ckey[(size_t)u * cap + pos] = kv[j];
          }
        }
      }
    }
  }
}

// ---- 4. order -----------------------------------------------------------------------------------------------------------------
// (block_prefix, block_bitonic, pow2_at_least and topl_emit: wrmf_device.h, shared with wrmf_candidates.hip)
// the double score u . v_it: 16 lanes per item, lane gl takes the elements gl, gl + 16, ... (uu: the user's vector in LDS)
template <class TF>
__device__ __forceinline__ double dot16(const double* uu, const TF* __restrict__ V, int it, int rank, int gl) {
  double acc = 0.0;
  for (int r = gl; r < rank; r += 16) acc = fma(uu[r], (double)V[(size_t)it * rank + r], acc);
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  return acc;
}

// One workgroup per user whose list did not overflow.  LDS: sk[cap] keys (the double score's order key), si[cap] items.
template <bool RESCORE, class TF, class TO>
__global__ __launch_bounds__(256) void topl_order_kernel(const TF* __restrict__ U, const TF* __restrict__ V, int rank, int topk,
                                                         int cap, const int* __restrict__ cnt, const int* __restrict__ adm,
                                                         const int32_t* __restrict__ cidx, const unsigned* __restrict__ ckey,
                                                         TO glob_mean, int32_t* __restrict__ res, TO* __restrict__ scores) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u64* sk = reinterpret_cast<u64*>(smem);
  int* si = reinterpret_cast<int*>(sk + cap);
  double* uu = reinterpret_cast<double*>(si + cap);   // [256]
  unsigned* hist = reinterpret_cast<unsigned*>(uu + 256);   // [256]
  u64* sres = reinterpret_cast<u64*>(hist + 256);
  int* sint = reinterpret_cast<int*>(sres + 1);   // [8]
  const int u = blockIdx.x, tid = threadIdx.x;
  const int n = cnt[u];
  if (n > cap) return;   // topl_heap_kernel's user
  const int kk = min(topk, adm[u]);
  int32_t* ru = res + (size_t)u * topk;
  TO* su = scores + (size_t)u * topk;
  if (kk <= 0) {
    topl_emit(sk, si, 0, topk, glob_mean, ru, su);
    return;
  }
  if constexpr (RESCORE)
    for (int r = tid; r < rank; r += 256) uu[r] = (double)U[(size_t)u * rank + r];
  for (int e = tid; e < n; e += 256) {
    si[e] = cidx[(size_t)u * cap + e];
    if constexpr (!RESCORE) sk[e] = f64_key((double)key_f32(ckey[(size_t)u * cap + e]) + 0.0);
  }
  __syncthreads();
  if constexpr (RESCORE) {
    const int grp = tid >> 4, gl = tid & 15;
    for (int e = grp; e < n; e += 16) {
      const double s = dot16(uu, V, si[e], rank, gl);
      if (gl == 0) sk[e] = f64_key(s + 0.0);
    }
    __syncthreads();
  }
  // v_k, |A| (g) and |G| (nt)
  const u64 vk = block_kth_largest(n, kk, 64, [&](int e, bool& ok) { ok = true; return sk[e]; }, hist, sres, sint);
  int g = 0, nt = 0, tot;
  for (int c0 = 0; c0 < n; c0 += 256) {
    const int e = c0 + tid;
    block_prefix(e < n && sk[e] > vk, sint + 4, &tot);
    g += tot;
    block_prefix(e < n && sk[e] == vk, sint + 4, &tot);
    nt += tot;
  }
  int cut_hi = 0x7fffffff, cut_lo = -1;   // the G items kept: cut_lo <= item <= cut_hi
  if (g + nt > kk) {
    // c = the kk-th smallest item of A u G (the last of the first kk in ascending order) ...
    const u64 c = block_kth_largest(n, kk, 32, [&](int e, bool& ok) { ok = sk[e] >= vk; return (u64)(0xffffffffu - (unsigned)si[e]); },
                                    hist, sres, sint);
    cut_hi = (int)(0xffffffffu - (unsigned)c);
    // ... t = the G items up to it; keep the m = kk - |A| largest of them
    const int m = kk - g;
    cut_lo = (int)block_kth_largest(n, m, 32, [&](int e, bool& ok) { ok = sk[e] == vk && si[e] <= cut_hi; return (u64)(unsigned)si[e]; },
                                     hist, sres, sint);
  }
  // the kk survivors to the front (in place: a chunk is read before any of it is written, writes land below it)
  int dst0 = 0;
  for (int c0 = 0; c0 < n; c0 += 256) {
    const int e = c0 + tid;
    u64 k = 0;
    int ix = -1;
    bool keep = false;
    if (e < n) {
      k = sk[e];
      ix = si[e];
      keep = k > vk || (k == vk && ix >= cut_lo && ix <= cut_hi);
    }
    const int off = block_prefix(keep, sint + 4, &tot);
    if (keep) {
      sk[dst0 + off] = k;
      si[dst0 + off] = ix;
    }
    dst0 += tot;
    __syncthreads();
  }
  const int P = pow2_at_least(kk);   // <= cap (the launcher sizes cap >= the power of two above topk)
  for (int e = kk + tid; e < P; e += 256) {
    sk[e] = 0ull;
    si[e] = -1;
  }
  __syncthreads();
  block_bitonic(sk, si, P, false);
  topl_emit(sk, si, kk, topk, glob_mean, ru, su);
}

// A user whose list overflowed: the reference's heap replayed over the user's items with key >= the kc-th key, in ascending
// item order (the items below it are below v_k: they never change the final heap).  Batches of 256 items: their scores in
// parallel, the ones that can enter compacted in item order; while the heap fills they are appended, and once it holds k
// entries it is sorted ascending -- a sorted array is a min-heap -- and thread 0 pushes the rest one by one (replacement only on
// a strictly larger score, sift-down on (score, index) pairs, as std::priority_queue<pair, greater> does).  Slow by design:
// exact ties at the bound of more items than the list holds.
template <bool RESCORE, class TF, class TO>
__global__ __launch_bounds__(256) void topl_heap_kernel(const TF* __restrict__ U, const TF* __restrict__ V, int rank,
                                                        const unsigned* __restrict__ keys, size_t ld, int n_items, int topk, int cap,
                                                        const int* __restrict__ cnt, const int* __restrict__ adm,
                                                        const unsigned* __restrict__ thr, TO glob_mean, int32_t* __restrict__ res,
                                                        TO* __restrict__ scores) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int P = pow2_at_least(topk);
  u64* hk = reinterpret_cast<u64*>(smem);          // [P]
  int* hi = reinterpret_cast<int*>(hk + P);        // [P]
  u64* bk = reinterpret_cast<u64*>(hi + P);        // [256] the batch's entrants
  int* bi = reinterpret_cast<int*>(bk + 256);      // [256]
  u64* sc = reinterpret_cast<u64*>(bi + 256);      // [256] the batch's keys
  double* uu = reinterpret_cast<double*>(sc + 256);   // [256]
  int* sint = reinterpret_cast<int*>(uu + 256);    // [8]
  const int u = blockIdx.x, tid = threadIdx.x;
  if (cnt[u] <= cap) return;
  const int kk = min(topk, adm[u]);
  const unsigned t = thr[u];
  const unsigned* row = keys + (size_t)u * ld;
  if constexpr (RESCORE)
    for (int r = tid; r < rank; r += 256) uu[r] = (double)U[(size_t)u * rank + r];
  __syncthreads();
  int size = 0;
  for (int b0 = 0; b0 < n_items; b0 += 256) {
    const int i = b0 + tid;
    const unsigned k32 = i < n_items ? row[i] : 0u;
    const bool ok = k32 != 0u && k32 >= t;
    u64 mk = 0;
    if constexpr (RESCORE) {
      const int grp = tid >> 4, gl = tid & 15;
      for (int j = grp; j < 256 && b0 + j < n_items; j += 16) {
        const unsigned kj = row[b0 + j];
        if (kj != 0u && kj >= t) {   // (uniform over the 16 lanes)
          const double s = dot16(uu, V, b0 + j, rank, gl);
          if (gl == 0) sc[j] = f64_key(s + 0.0);
        }
      }
      __syncthreads();
      if (ok) mk = sc[tid];
    } else {
      mk = f64_key((double)key_f32(k32) + 0.0);
    }
    const bool enter = ok && (size < kk || mk > hk[0]);
    int ns;
    const int pos = block_prefix(enter, sint, &ns);
    if (enter) {
      bk[pos] = mk;
      bi[pos] = i;
    }
    __syncthreads();
    int j0 = 0;
    if (size < kk) {
      const int take = min(ns, kk - size);
      for (int j = tid; j < take; j += 256) {
        hk[size + j] = bk[j];
        hi[size + j] = bi[j];
      }
      size += take;
      j0 = take;
      __syncthreads();
      if (size == kk) {
        for (int e = kk + tid; e < P; e += 256) {
          hk[e] = ~0ull;
          hi[e] = 0x7fffffff;
        }
        __syncthreads();
        block_bitonic(hk, hi, P, true);
      }
    }
    if (tid == 0 && size == kk) {
      for (int j = j0; j < ns; j++) {
        const u64 v = bk[j];
        if (!(hk[0] < v)) continue;
        const int ix = bi[j];
        int p = 0;
        for (;;) {   // sift the new entry down from the root
          const int l = 2 * p + 1;
          if (l >= kk) break;
          int c = l;
          if (l + 1 < kk && (hk[l + 1] < hk[l] || (hk[l + 1] == hk[l] && hi[l + 1] < hi[l]))) c = l + 1;
          if (!(hk[c] < v || (hk[c] == v && hi[c] < ix))) break;
          hk[p] = hk[c];
          hi[p] = hi[c];
          p = c;
        }
        hk[p] = v;
        hi[p] = ix;
      }
    }
    __syncthreads();
  }
  for (int e = size + tid; e < P; e += 256) {
    hk[e] = 0ull;
    hi[e] = -1;
  }
  __syncthreads();
  block_bitonic(hk, hi, P, false);
  topl_emit(hk, hi, size, topk, glob_mean, res + (size_t)u * topk, scores + (size_t)u * topk);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
struct LgPlan {
  int chunk;     // users per chunk
  size_t ld;     // key row stride (a multiple of 4)
  int cap;       // candidate list per user
  size_t words_per_user;
};

LgPlan lg_plan(int n_users, int n_items, int topk, int kc) {
  LgPlan p;
  p.ld = ((size_t)std::max(n_items, 1) + 3) / 4 * 4;
  int pw = 1;
  while (pw < topk) pw <<= 1;
  p.cap = std::min(kLgMaxCand, std::max(pw, (2 * kc + 255) / 256 * 256));
  p.words_per_user = p.ld + kLgHistBins + 4 + 2 * (size_t)p.cap;
  size_t c = kLgWorkspaceWords / p.words_per_user;
  if (c > 256) c = c / 256 * 256;
  p.chunk = (int)std::max<size_t>(1, std::min<size_t>({c, (size_t)kLgMaxChunk, (size_t)std::max(n_users, 1)}));
  return p;
}

size_t lds_order(int cap) { return (size_t)cap * 12 + 256 * 8 + 256 * 4 + 8 + 8 * 4; }
size_t lds_heap(int topk) {
  int P = 1;
  while (P < topk) P <<= 1;
  return (size_t)P * 12 + 256 * 12 + 256 * 8 + 256 * 8 + 8 * 4;
}

template <int KP, int UB>
hipError_t go_score(const float* U, const float* V, int nu, int n_items, int rank, int slice, unsigned* keys, size_t ld, hipStream_t s) {
  const bool vec = rank % 4 == 0 && (reinterpret_cast<uintptr_t>(V) & 15) == 0;
  const dim3 grid((nu + 128 * UB - 1) / (128 * UB), (n_items + slice - 1) / slice);
  if (vec) hipLaunchKernelGGL((topl_score_kernel<KP, UB, true>), grid, dim3(256), 0, s, U, V, nu, n_items, rank, slice, keys, ld);
  else hipLaunchKernelGGL((topl_score_kernel<KP, UB, false>), grid, dim3(256), 0, s, U, V, nu, n_items, rank, slice, keys, ld);
  return hipGetLastError();
}

hipError_t launch_score(const float* U, const float* V, int nu, int n_items, int rank, unsigned* keys, size_t ld, hipStream_t s) {
  const int KP = rank > 128 ? 256 : padded_rank(rank);
  const int UB = (KP <= 128 && nu > 128) ? 2 : 1;
  const int ublocks = (nu + 128 * UB - 1) / (128 * UB);
  // about 2048 workgroups per launch, slices of at least 1024 items (a multiple of the 32-item tile)
  const int max_slices = std::max(1, (n_items + 1023) / 1024);
  const int slices = std::max(1, std::min(max_slices, (2048 + ublocks - 1) / ublocks));
  const int slice = ((n_items + slices - 1) / slices + 31) / 32 * 32;
#define RSP_TOPL_SCORE(KPV)                                                                                     \
  if (KP == KPV) return UB == 2 ? go_score<KPV, 2>(U, V, nu, n_items, rank, slice, keys, ld, s)               \
                                : go_score<KPV, 1>(U, V, nu, n_items, rank, slice, keys, ld, s);
  RSP_TOPL_SCORE(32)
  RSP_TOPL_SCORE(64)
  RSP_TOPL_SCORE(128)
#undef RSP_TOPL_SCORE
  if (KP == 256) return go_score<256, 1>(U, V, nu, n_items, rank, slice, keys, ld, s);
  return hipErrorInvalidValue;
}

template <bool RESCORE, class TF, class TO>
hipError_t launch_large_t(const float* U32, const float* V32, const TF* U, const TF* V, int n_users, int n_items, int rank, int topk,
                          int kc, const int32_t* nr_ptr, const int32_t* nr_idx, const int32_t* excl, int n_excl, TO glob_mean,
                          int32_t* res, TO* scores, hipStream_t s, float* ws) {
  if (n_users <= 0) return hipSuccess;
  if (topk <= kTopLargeMin || topk > kTopLargeMax || kc < topk || kc > kLgMaxCand || rank < 1 || rank > 256 || !ws)
    return hipErrorInvalidValue;
  if (rank <= 128 && !padded_rank(rank)) return hipErrorInvalidValue;
  const LgPlan p = lg_plan(n_users, n_items, topk, kc);
  // workspace: keys [chunk][ld], then hist [chunk][2048], pref, rem, adm, cnt [chunk] (zeroed together), then the lists
  unsigned* keys = reinterpret_cast<unsigned*>(ws);
  unsigned* hist = keys + (size_t)p.chunk * p.ld;
  unsigned* pref = hist + (size_t)p.chunk * kLgHistBins;
  int* rem = reinterpret_cast<int*>(pref + p.chunk);
  int* adm = rem + p.chunk;
  int* cnt = adm + p.chunk;
  int32_t* cidx = cnt + p.chunk;
  unsigned* ckey = reinterpret_cast<unsigned*>(cidx + (size_t)p.chunk * p.cap);
  const size_t lds_o = lds_order(p.cap), lds_h = lds_heap(topk);
  auto ko = topl_order_kernel<RESCORE, TF, TO>;
  auto kh = topl_heap_kernel<RESCORE, TF, TO>;
  hipError_t err;
  if ((err = hipFuncSetAttribute(reinterpret_cast<const void*>(ko), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_o)) != hipSuccess)
    return err;
  if ((err = hipFuncSetAttribute(reinterpret_cast<const void*>(kh), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_h)) != hipSuccess)
    return err;
  for (int c0 = 0; c0 < n_users; c0 += p.chunk) {
    const int nu = std::min(p.chunk, n_users - c0);
    const int32_t* nrp = nr_ptr ? nr_ptr + c0 : nullptr;
    if ((err = hipMemsetAsync(hist, 0, (size_t)nu * kLgHistBins * 4, s)) != hipSuccess ||
        (err = hipMemsetAsync(pref, 0, (size_t)4 * p.chunk * 4, s)) != hipSuccess)
      return err;
    if (n_items > 0) {
      if ((err = launch_score(U32 + (size_t)c0 * rank, V32, nu, n_items, rank, keys, p.ld, s)) != hipSuccess) return err;
      if (nrp || n_excl > 0) {
        hipLaunchKernelGGL(topl_mask_kernel, dim3(nu), dim3(256), 0, s, keys, p.ld, n_items, nrp, nr_idx, excl, n_excl);
        if ((err = hipGetLastError()) != hipSuccess) return err;
      }
      // slices of the rows: about 4096 workgroups per pass, a multiple of 1024 keys each
      const int max_sl = std::max(1, (n_items + 4095) / 4096);
      const int nsl = std::max(1, std::min(max_sl, (4096 + nu - 1) / nu));
      const int sl = ((n_items + nsl - 1) / nsl + 1023) / 1024 * 1024;
      const dim3 hg((n_items + sl - 1) / sl, nu);
      for (int pass = 0; pass < 3; pass++) {
        hipLaunchKernelGGL(topl_hist_kernel, hg, dim3(256), 0, s, keys, p.ld, n_items, sl, pass, pref, hist, adm);
        hipLaunchKernelGGL(topl_resolve_kernel, dim3(nu), dim3(64), 0, s, hist, pass, kc, pref, rem, adm);
      }
      hipLaunchKernelGGL(topl_compact_kernel, hg, dim3(256), 0, s, keys, p.ld, n_items, sl, pref, cnt, p.cap, cidx, ckey);
      if ((err = hipGetLastError()) != hipSuccess) return err;
    }
    const TF* Uc = RESCORE ? U + (size_t)c0 * rank : nullptr;
    hipLaunchKernelGGL(ko, dim3(nu), dim3(256), lds_o, s, Uc, V, rank, topk, p.cap, cnt, adm, cidx, ckey, glob_mean,
                       res + (size_t)c0 * topk, scores + (size_t)c0 * topk);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    if (n_items > 0) {
      hipLaunchKernelGGL(kh, dim3(nu), dim3(256), lds_h, s, Uc, V, rank, keys, p.ld, n_items, topk, p.cap, cnt, adm, pref, glob_mean,
                         res + (size_t)c0 * topk, scores + (size_t)c0 * topk);
      if ((err = hipGetLastError()) != hipSuccess) return err;
    }
  }
  return hipSuccess;
}

}  // namespace

// the first two stages on their own (wrmf_ranks.hip counts over the same key matrix)
hipError_t launch_topl_score(const float* U, const float* V, int nu, int n_items, int rank, unsigned* keys, size_t ld, hipStream_t s) {
  return launch_score(U, V, nu, n_items, rank, keys, ld, s);
}

hipError_t launch_topl_mask(unsigned* keys, size_t ld, int n_items, int nu, const int32_t* nr_ptr, const int32_t* nr_idx,
                            const int32_t* excl, int n_excl, hipStream_t s) {
  hipLaunchKernelGGL(topl_mask_kernel, dim3(nu), dim3(256), 0, s, keys, ld, n_items, nr_ptr, nr_idx, excl, n_excl);
  return hipGetLastError();
}

size_t top_product_large_ws_floats(int n_users, int n_items, int topk, int kc, int* chunk_users) {
  const LgPlan p = lg_plan(n_users, n_items, topk, kc);
  if (chunk_users) *chunk_users = p.chunk;
  return (size_t)p.chunk * p.words_per_user + 64;
}

int top_product_large_kc(int topk, int extra, int n_items) {
  if (extra < 0) extra = std::max(8, topk / 4);
  return std::max(topk, std::min(std::min(topk + extra, kLgMaxCand), std::max(n_items, 1)));
}

hipError_t launch_top_product_large(const float* U, const float* V, int n_users, int n_items, int rank, int topk,
                                    const int32_t* nr_ptr, const int32_t* nr_idx, const int32_t* excl, int n_excl, float glob_mean,
                                    int32_t* res, float* scores, hipStream_t s, float* ws) {
  return launch_large_t<false, float, float>(U, V, U, V, n_users, n_items, rank, topk, topk, nr_ptr, nr_idx, excl, n_excl, glob_mean,
                                             res, scores, s, ws);
}

hipError_t launch_top_product_large_f64(const float* U32, const float* V32, const double* U64, const double* V64, int n_users,
                                        int n_items, int rank, int topk, int kc, const int32_t* nr_ptr, const int32_t* nr_idx,
                                        const int32_t* excl, int n_excl, double glob_mean, int32_t* res, double* scores,
                                        hipStream_t s, float* ws) {
  if (U64 && V64)
    return launch_large_t<true, double, double>(U32, V32, U64, V64, n_users, n_items, rank, topk, kc, nr_ptr, nr_idx, excl, n_excl,
                                                glob_mean, res, scores, s, ws);
  return launch_large_t<true, float, double>(U32, V32, U32, V32, n_users, n_items, rank, topk, kc, nr_ptr, nr_idx, excl, n_excl,
                                             glob_mean, res, scores, s, ws);
}

}  // namespace rsparse_hip
