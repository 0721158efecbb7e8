// top-k of the dense product  scores = U * V^T  per user, fused (gfx950, wave64).
//
// Replaces top_product() (src/matrix_top_product.cpp:20-102), the C++ behind find_top_product()
// (R/utils.R:31-59) and `$predict` (R/MatrixFactorizationRecommender.R:24-78): for every user row j,
// scores_i = u_j . v_i over all items, skip the items of the user's `not_recommend` row (sorted CSR) and the
// globally excluded items, keep the k best in a min-heap (`q.top().first < val` -> on ties the earlier item
// stays), emit them best first -- equal scores come out with the larger index first, because the heap pops
// (score, index) pairs in ascending pair order and the output is filled from the end (:88-95).
//
// A map of this file.  Three kernel families multiply 32-user blocks (the MFMA A operands, in registers) with 32-item tiles
// staged through LDS (v_mfma_f32_32x32x2_f32: exact fp32) and keep per-user candidate buffers of the scores that beat the
// user's current k-th best:
//   top_product_kernel         a tile per wave against the workgroup's 32 / 64 users (calls for up to 64 users, or a large k);
//   top_product_shared_kernel  the four waves share one tile and own 32 users each (a narrow band of k where two tiles do not fit);
//   top_product_pipe_kernel    the same with two tiles resident and the epilogue hidden behind the next tile's matrix
//                              instructions; GBUF: the candidate buffers in a global scratch (every call for more than 128 users).
// Few users over many items are split over the items and merged (top_merge_kernel); top_rescore_kernel re-scores candidates in
// double.  WHICH kernel runs, how a call is sliced and what scratch it wants is decided in one place, wrmf_topk_plan.h
// (top_product_plan: an ordered table of rows per rank); launch_top_product{,_f64} below walk that plan and launch_top_row
// launches one of its rows.
#include <algorithm>

#include "wrmf_internal.h"
#include "wrmf_device.h"
#include "wrmf_topk_plan.h"

namespace rsparse_hip {
namespace {

using namespace dev;

// is `item` in the sorted list a[0..n) ?
__device__ __forceinline__ bool sorted_contains(const int32_t* __restrict__ a, int n, int item) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int v = a[mid];
    if (v < item) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && a[lo] == item;
}

// Reduce one user's over-full candidate buffer (n > topk entries: bv / bi) to its top k by rank counting (tv / ti: scratch
// of the calling wave), and return the new threshold (the k-th best score).  `old` = how many leading entries are the heap
// as the previous reduction left it.  One wave; every lane gets the result.
__device__ __forceinline__ float topk_reduce_user(float* bv, int* bi, float* tv, int* ti, const int n, const int topk,
                                                  const int old, const int lane) {
  // A full heap and a handful of arrivals (the steady state: after the first tiles a user sees a survivor every few hundred
  // tiles): the arrivals go through the heap one by one -- the reference's own loop, src/matrix_top_product.cpp:61-86, and
  // the code below for the tie case -- at O(k / 64) each, instead of the O(n^2 / 64) rank counting that pays for big batches.
  const bool few = old == topk && n - old <= 8;
  float kth = 0.f;
  int ge = topk + 1;
  // (round 6) The k-th best score by a radix select over the entries held in registers -- 32 bit positions x a ballot per register
  // -- instead of ranking every entry against every other (O(n^2 / 64): 15 us at n = 220, and the batched settles of the global
  // buffers made it the whole cost of top-100).  The buffer's order carries no meaning (the heap is a set: the replay below scans
  // it for its minimum, the emission ranks it), so the survivors -- the entries at or above the k-th score, exactly k of them
  // unless the bound is tied -- are compacted to the front in place.
  constexpr int NE = (kTopMaxCap + 63) / 64;
  unsigned key[NE];
  int eix[NE];
  if (!few) {
#pragma unroll
    for (int j = 0; j < NE; j++) {
      const int c = lane + 64 * j;
      key[j] = 0u;   // (below every score's key: a finite float maps to a key >= 0x00800000)
      eix[j] = 0;
      if (c < n) {
        const unsigned u = __float_as_uint(bv[c] + 0.f);   // (-0 -> +0: equal scores, equal keys)
        key[j] = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        eix[j] = bi[c];
      }
    }
    unsigned kk = 0u;   // the k-th largest key, bit by bit
    for (int bit = 31; bit >= 0; bit--) {
      const unsigned trial = kk | (1u << bit);
      int cnt = 0;
#pragma unroll
      for (int j = 0; j < NE; j++)
        if (64 * j < n) cnt += __popcll(__ballot(key[j] >= trial));
      if (cnt >= topk) kk = trial;
    }
    ge = 0;
#pragma unroll
    for (int j = 0; j < NE; j++)
      if (64 * j < n) ge += __popcll(__ballot(key[j] >= kk));
    kth = __uint_as_float((kk & 0x80000000u) ? (kk & 0x7fffffffu) : ~kk);
    // More candidates at the k-th score than places for them?  Then WHICH of them survive depends on the order in
    // which the reference's heap met them (it evicts the smallest index among tied minima, but a tied newcomer
    // never enters a full heap: scores [1,1,5], k = 2 -> {2,1}; [1,5,1] -> {1,0}), and the arrivals since the last
    // reduction are replayed through that heap in index order.  Everything that arrived before was reduced the
    // same way, so the buffer's first `old` entries ARE the reference's heap at that point.
    if (ge == topk) {
      wave_sync();   // (every lane holds its entries; the buffer is rewritten in place)
      int base = 0;
#pragma unroll
      for (int j = 0; j < NE; j++) {
        if (64 * j < n) {
          const bool keep = key[j] >= kk;
          const unsigned long long m = __ballot(keep);
          if (keep) {
            const int dst = base + __popcll(m & ((1ull << lane) - 1ull));
            const unsigned kj = key[j];
            bv[dst] = __uint_as_float((kj & 0x80000000u) ? (kj & 0x7fffffffu) : ~kj);
            bi[dst] = eix[j];
          }
          base += __popcll(m);
        }
      }
      wave_sync();
      return kth;
    }
  }
  if (ge > topk) {   // wave-uniform
    wave_sync();
    for (int c = lane; c < n; c += 64) {   // heap as it is, then the new arrivals sorted by item index
      int dst = c;
      if (c >= old) {
        const int ix = bi[c];
        int r = 0;
        for (int c2 = old; c2 < n; c2++) r += bi[c2] < ix ? 1 : 0;
        dst = old + r;
      }
      tv[dst] = bv[c];
      ti[dst] = bi[c];
    }
    wave_sync();
    int h = old;
    for (int c = old; c < n; c++) {
      const float v = tv[c];
      const int ix = ti[c];
      if (h < topk) {
        if (lane == 0) {
          bv[h] = v;
          bi[h] = ix;
        }
        h++;
      } else {
        // smallest (score, index) of the heap: what std::priority_queue<pair, greater> has on top
        float mv = INFINITY;
        int mi = 0x7fffffff, mp = -1;
        for (int e = lane; e < topk; e += 64) {
          const float hv = bv[e];
          const int hi = bi[e];
          if (hv < mv || (hv == mv && hi < mi)) { mv = hv; mi = hi; mp = e; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const float ov = __shfl_xor(mv, off);
          const int oi = __shfl_xor(mi, off), op = __shfl_xor(mp, off);
          if (ov < mv || (ov == mv && oi < mi)) { mv = ov; mi = oi; mp = op; }
        }
        if (mv < v && lane == 0) {
          bv[mp] = v;
          bi[mp] = ix;
        }
      }
      wave_sync();
    }
    float mn = INFINITY;
    for (int e = lane; e < topk; e += 64) mn = fminf(mn, bv[e]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mn = fminf(mn, __shfl_xor(mn, off));
    return mn;
  }
  return kth;   // (not reached: ge >= topk whenever n > topk)
}

// The tile-sharing kernels append a score that beats its user's threshold WITHOUT looking at the exclusion lists (the
// unrolled epilogue stays a compare and an append per accumulator entry: with two binary searches inlined 32 times the loop
// outgrew the instruction cache); the lists are consulted here, one lane per arrival, before a buffer is reduced or emitted.
// Drops the entries [from, n) of a user's buffer that `nr_row` (the user's not_recommend row) or `excl` rules out, closes
// the gaps, returns the new count.  One wave.
__device__ __forceinline__ int topk_verify_arrivals(float* bv, int* bi, const int from, const int n,
                                                    const int32_t* __restrict__ nr_row, const int nr_len,
                                                    const int32_t* __restrict__ excl, const int n_excl, const int lane) {
  if (nr_len <= 0 && n_excl <= 0) return n;
  int kept = from;
  for (int c0 = from; c0 < n; c0 += 64) {
    const int c = c0 + lane;
    float v = 0.f;
    int ix = 0;
    bool ok = false;
    if (c < n) {
      v = bv[c];
      ix = bi[c];
      ok = !(nr_len > 0 && sorted_contains(nr_row, nr_len, ix)) && !(n_excl > 0 && sorted_contains(excl, n_excl, ix));
    }
    const unsigned long long m = __ballot(ok);
    wave_sync();   // every lane has read its entry before any is overwritten
    if (ok) {
      const int dst = kept + __popcll(m & ((1ull << lane) - 1ull));
      bv[dst] = v;
      bi[dst] = ix;
    }
    kept += __popcll(m);
    wave_sync();
  }
  return kept;
}

// arrivals verified, then the buffer reduced if it is over-full: what the tile-sharing kernels do for a user whose count
// passed k.  Updates the user's count / threshold / verified length.  One wave.
__device__ __forceinline__ void topk_settle_user(float* bv, int* bi, float* tv, int* ti, int* cnt, float* thr, int* need,
                                                 const int topk, const int32_t* __restrict__ nr_ptr,
                                                 const int32_t* __restrict__ nr_idx, const int u,
                                                 const int32_t* __restrict__ excl, const int n_excl, const int lane) {
  const int old = *need;
  int p1 = 0, len = 0;
  if (nr_ptr) {
    p1 = nr_ptr[u];
    len = nr_ptr[u + 1] - p1;
  }
  const int n = topk_verify_arrivals(bv, bi, old, *cnt, nr_idx + p1, len, excl, n_excl, lane);
  float t = *thr;
  int nn = n;
  if (n > topk) {   // wave-uniform
    t = topk_reduce_user(bv, bi, tv, ti, n, topk, old, lane);
    nn = topk;
  }
  wave_sync();
  if (lane == 0) {
    *cnt = nn;
    *thr = t;
    *need = nn;
  }
  wave_sync();
}

// final output of one user: best first; equal scores with the larger index first (heap pop order of the reference)
__device__ __forceinline__ void topk_emit_user(const float* bv, const int* bi, const int n, const int topk, const int lane,
                                               const float glob_mean, int32_t* res_u, float* scores_u) {
  for (int c = lane; c < topk; c += 64) {
    if (c < n) {
      const float v = bv[c];
      const int ix = bi[c];
      int rank = 0;
      for (int c2 = 0; c2 < n; c2++) {
        const float v2 = bv[c2];
        rank += (v2 > v || (v2 == v && bi[c2] > ix)) ? 1 : 0;
      }
      res_u[rank] = ix + 1;               // 1-based, like R
      scores_u[rank] = v + glob_mean;
    } else {
      res_u[c] = INT32_MIN;                // NA_integer_
      scores_u[c] = __int_as_float(0x7fc00000);
    }
  }
}

// GBUF: a user's buffer (global: gv / gi, n entries) through the wave's LDS work area (wv_ / wi_): arrivals verified, the buffer
// reduced when it is over-full, what is left written back.  One wave.
__device__ __forceinline__ void topk_settle_user_g(float* gv, int* gi, float* wv_, int* wi_, float* tv, int* ti, int* cnt,
                                                   float* thr, int* need, const int topk, const int32_t* __restrict__ nr_ptr,
                                                   const int32_t* __restrict__ nr_idx, const int u,
                                                   const int32_t* __restrict__ excl, const int n_excl, const int lane) {
  const int n0 = *cnt;
  for (int c = lane; c < n0; c += 64) {
    wv_[c] = gv[c];
    wi_[c] = gi[c];
  }
  wave_sync();
  topk_settle_user(wv_, wi_, tv, ti, cnt, thr, need, topk, nr_ptr, nr_idx, u, excl, n_excl, lane);
  const int nn = *cnt;
  for (int c = lane; c < nn; c += 64) {
    gv[c] = wv_[c];
    gi[c] = wi_[c];
  }
}

// ---- the steps the kernel families share ------------------------------------------------------------------------------------------
// A split launch (few users, many items: blockIdx.y = item slice): the workgroup sees its slice as the matrix -- item ids are
// item_base (returned) + local -- and writes to the slice's block of the scratch.  See launch_top_first.
__device__ __forceinline__ int top_enter_slice(const float* __restrict__& V, int& n_items, int32_t* __restrict__& res,
                                               float* __restrict__& scores_out, const int slice_items, const int n_users,
                                               const int k_rank, const int topk) {
  if (slice_items <= 0) return 0;
  const int item_base = (int)blockIdx.y * slice_items;
  V += (size_t)item_base * k_rank;
  n_items = max(0, min(n_items - item_base, slice_items));
  res += (size_t)blockIdx.y * n_users * topk;
  scores_out += (size_t)blockIdx.y * n_users * topk;
  return item_base;
}
// the fall-back launch of the unsplit kernel (user_flags given) runs only the workgroups that hold a flagged user: does the block
// of USERS users from u0 hold one?  (A barrier: every thread of the workgroup calls it.)
template <int USERS, int THREADS>
__device__ __forceinline__ bool top_block_flagged(const int* __restrict__ user_flags, const int u0, const int n_users) {
  int f = 0;
  for (int e = threadIdx.x; e < USERS; e += THREADS)
    if (u0 + e < n_users) f |= user_flags[u0 + e];
  return __syncthreads_or(f);
}

// A operands: lane holds U[ubase + 32 ub + (lane & 31)][2t + half], t = 0..KP/2-1 (zero beyond the matrix)
template <int UB, int NK2>
__device__ __forceinline__ void top_load_users(float (&afrag)[UB][NK2], const float* __restrict__ U, const int ubase,
                                               const int n_users, const int k_rank, const int col, const int half) {
#pragma unroll
  for (int ub = 0; ub < UB; ub++) {
    const int u = ubase + 32 * ub + col;
#pragma unroll
    for (int t = 0; t < NK2; t++) {
      const int kk = 2 * t + half;
      afrag[ub][t] = (u < n_users && kk < k_rank) ? U[(size_t)u * k_rank + kk] : 0.f;
    }
  }
}

// Item tile tl -> registers (load) -> LDS (store), by THREADS threads (64: every wave stages its own tiles).  VEC = rank a multiple of 4 and V
// 16-byte aligned: NLD 16-byte loads per thread, all in flight together (piece e4 = j * THREADS + t: item e4 / (KP / 4), floats
// 4 (e4 % (KP / 4)) ..+3): load() goes before the matrix instructions of the resident tile, store() after the last reader of the
// LDS tile it replaces.  Else (any rank / alignment) scalar staging in store(), the slow path: a row per wave and step.
template <int KP, bool VEC, int THREADS>
struct TopStager {
  static constexpr int LDT = KP + 4, NLD = 8 * KP / THREADS;
  const float* __restrict__ V;
  int n_tiles, n_items, k_rank;
  float4 pf[VEC ? NLD : 1];   // the tile in flight
  __device__ __forceinline__ TopStager(const float* __restrict__ V_, int n_tiles_, int n_items_, int k_rank_)
      : V(V_), n_tiles(n_tiles_), n_items(n_items_), k_rank(k_rank_) {}
  __device__ __forceinline__ void load(const int tl) {
    if constexpr (VEC) {
      const int i0 = tl * 32;
#pragma unroll
      for (int j = 0; j < NLD; j++) {
        const int e4 = j * THREADS + threadIdx.x % THREADS, it = e4 / (KP / 4), c4 = e4 % (KP / 4);
        pf[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tl < n_tiles && i0 + it < n_items && 4 * c4 < k_rank)
          pf[j] = *reinterpret_cast<const float4*>(V + (size_t)(i0 + it) * k_rank + 4 * c4);
      }
    }
  }
  __device__ __forceinline__ void store(float* tile, const int tl) {
    if constexpr (VEC) {
#pragma unroll
      for (int j = 0; j < NLD; j++) {
        const int e4 = j * THREADS + threadIdx.x % THREADS, it = e4 / (KP / 4), c4 = e4 % (KP / 4);
        *reinterpret_cast<float4*>(tile + it * LDT + 4 * c4) = pf[j];
      }
    } else {
      const int i0 = tl * 32, row0 = THREADS == 64 ? 0 : rfl(threadIdx.x >> 6);
      for (int it = row0; it < 32; it += THREADS / 64)
        for (int kk = threadIdx.x & 63; kk < k_rank; kk += 64)
          tile[it * LDT + kk] = (tl < n_tiles && i0 + it < n_items) ? V[(size_t)(i0 + it) * k_rank + kk] : 0.f;
    }
  }
};

// the products of a resident tile with the wave's user blocks, exact fp32: tp = the tile's row `col` + half, so that tp[2 t] is
// B[kk = 2t + half][item = col]; the lane then holds item `col` for users row(e) = (e & 3) + 8 (e >> 2) + 4 half of each block
template <int UB, int NK2>
__device__ __forceinline__ void top_sweep(f32x16 (&acc)[UB], const float (&afrag)[UB][NK2], const float* tp) {
#pragma unroll
  for (int ub = 0; ub < UB; ub++)
#pragma unroll
    for (int e = 0; e < 16; e++) acc[ub][e] = 0.f;
#pragma unroll
  for (int t = 0; t < NK2; t++) {
    const float b = tp[2 * t];
#pragma unroll
    for (int ub = 0; ub < UB; ub++) acc[ub] = __builtin_amdgcn_mfma_f32_32x32x2f32(afrag[ub][t], b, acc[ub], 0, 0, 0);
  }
}

// The LDS of a workgroup (top_lds_bytes, wrmf_topk_plan.h, is its size): the item tiles (rows of KP + 4 floats: 16-byte aligned for
// ds_write_b128; the 4-way bank conflict of the fragment reads is invisible next to a 64-cycle MFMA) | per user `cap` candidate
// scores | as many items | counts | thresholds | `need_words` words, the first per user = how many leading entries of its buffer
// are the heap as the last reduction left it | per wave a scratch of cap scores and cap items | GBUF: per wave a work area of the
// same size, and the candidate buffers themselves are the workgroup's slot of the global scratch
struct TopLds {
  float *tiles, *val;
  int *idx, *cnt;
  float* thr;
  int* need;
  float* tmpv;
  int* tmpi;
  float* wrkv;
  int* wrki;
};
template <bool GBUF>
__device__ __forceinline__ TopLds top_carve(char* smem, const size_t tile_floats, const int users, const int cap,
                                            const int need_words, const int waves, float* gslot) {
  TopLds s;
  s.tiles = reinterpret_cast<float*>(smem);
  s.val = GBUF ? gslot : s.tiles + tile_floats;
  s.idx = reinterpret_cast<int*>(s.val + (size_t)users * cap);
  s.cnt = GBUF ? reinterpret_cast<int*>(s.tiles + tile_floats) : s.idx + (size_t)users * cap;
  s.thr = reinterpret_cast<float*>(s.cnt + users);
  s.need = reinterpret_cast<int*>(s.thr + users);
  s.tmpv = reinterpret_cast<float*>(s.need + need_words);
  s.tmpi = reinterpret_cast<int*>(s.tmpv + waves * cap);
  s.wrkv = reinterpret_cast<float*>(s.tmpi + waves * cap);
  s.wrki = reinterpret_cast<int*>(s.wrkv + waves * cap);
  return s;
}
__device__ __forceinline__ void top_reset_users(const TopLds& s, const int users, const int threads) {
  for (int e = threadIdx.x; e < users; e += threads) {
    s.cnt[e] = 0;
    s.thr[e] = -INFINITY;
    s.need[e] = 0;
  }
}

// ---- ... and the steps of the two tile-sharing kernels, in which a wave owns its users' buffers outright ----------------------------
// the thresholds of this lane's users (thr_w: the wave's first), four 16-byte reads per block in flight together (one read and one
// wait per accumulator entry left the matrix cores idle for a third of the tile)
template <int UB>
__device__ __forceinline__ void top_load_thresholds(float4 (&thr4)[UB][4], const float* thr_w, const int half) {
#pragma unroll
  for (int ub = 0; ub < UB; ub++)
#pragma unroll
    for (int q = 0; q < 4; q++) thr4[ub][q] = *reinterpret_cast<const float4*>(thr_w + 32 * ub + 8 * q + 4 * half);
}
// Accumulator entry e of user block ub: a score that beats its user's threshold is appended WITHOUT looking at the exclusion
// lists (lanes of this wave only: at most 32 per user and tile) -- topk_settle_user consults them.  ok: the item and the user exist
template <int UB>
__device__ __forceinline__ void top_append(const TopLds& s, const bool ok, const float sc, const float4 (&thr4)[UB][4], const int ub,
                                           const int e, const int ul, const int gitem, const int cap) {
  const float* tq = reinterpret_cast<const float*>(&thr4[ub][e >> 2]);
  if (ok && sc > tq[e & 3]) {
    const int pos = atomicAdd(&s.cnt[ul], 1);
    s.val[ul * cap + pos] = sc;
    s.idx[ul * cap + pos] = gitem;
  }
}
// this wave's buffers whose count passed settle_at: arrivals verified, top k kept, threshold raised (after the first tiles almost
// nothing survives)
template <bool GBUF, int UPW>
__device__ __forceinline__ void top_settle_wave(const TopLds& s, const int uw, const int settle_at, const int cap, const int topk,
                                                const int32_t* __restrict__ nr_ptr, const int32_t* __restrict__ nr_idx, const int u0,
                                                const int32_t* __restrict__ excl, const int n_excl, const int wv, const int lane) {
  for (int b0 = 0; b0 < UPW; b0 += 64) {
    const int ulq = uw + b0 + lane;
    unsigned long long over = __ballot(b0 + lane < UPW && s.cnt[ulq] > settle_at);
    if constexpr (GBUF) {
      // (the appends are this wave's own stores: complete, and not served from a stale line of the vector cache)
      if (over) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    }
    while (over) {
      const int ul = uw + b0 + __builtin_ctzll(over);
      over &= over - 1;
      if constexpr (GBUF)
        topk_settle_user_g(s.val + (size_t)ul * cap, s.idx + (size_t)ul * cap, s.wrkv + wv * cap, s.wrki + wv * cap, s.tmpv + wv * cap,
                           s.tmpi + wv * cap, s.cnt + ul, s.thr + ul, s.need + ul, topk, nr_ptr, nr_idx, u0 + ul, excl, n_excl, lane);
      else
        topk_settle_user(s.val + (size_t)ul * cap, s.idx + (size_t)ul * cap, s.tmpv + wv * cap, s.tmpi + wv * cap, s.cnt + ul,
                         s.thr + ul, s.need + ul, topk, nr_ptr, nr_idx, u0 + ul, excl, n_excl, lane);
    }
  }
}
// after the last tile: this wave's users settled where arrivals are left that no reduction has looked at (the buffer never filled
// up again), and emitted.  GBUF: always through the work area -- the last arrivals are verified / reduced there, and the
// emission reads LDS
template <bool GBUF, int UPW>
__device__ __forceinline__ void top_finish_wave(const TopLds& s, const int uw, const int cap, const int topk, const int n_users,
                                                const int32_t* __restrict__ nr_ptr, const int32_t* __restrict__ nr_idx, const int u0,
                                                const int32_t* __restrict__ excl, const int n_excl, const float glob_mean,
                                                int32_t* __restrict__ res, float* __restrict__ scores_out, const int wv,
                                                const int lane) {
  if constexpr (GBUF) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
  for (int ul = uw; ul < uw + UPW; ul++) {
    const int u = u0 + ul;
    if (u >= n_users) break;
    const float* gv = s.val + (size_t)ul * cap;
    const int* gi = s.idx + (size_t)ul * cap;
    float* bv = GBUF ? s.wrkv + wv * cap : s.val + (size_t)ul * cap;
    int* bi = GBUF ? s.wrki + wv * cap : s.idx + (size_t)ul * cap;
    const int n0 = s.cnt[ul];
    if constexpr (GBUF) {
      wave_sync();
      for (int c = lane; c < n0; c += 64) {
        bv[c] = gv[c];
        bi[c] = gi[c];
      }
      wave_sync();
    }
    if (n0 > s.need[ul])
      topk_settle_user(bv, bi, s.tmpv + wv * cap, s.tmpi + wv * cap, s.cnt + ul, s.thr + ul, s.need + ul, topk, nr_ptr, nr_idx, u, excl,
                       n_excl, lane);
    topk_emit_user(bv, bi, min(s.cnt[ul], topk), topk, lane, glob_mean, res + (size_t)u * topk, scores_out + (size_t)u * topk);
  }
}

// ---- a tile per wave: every wave walks its own item tiles against the workgroup's 32 UB users (W waves = W tiles per round) ----------
// One workgroup per block of 32 UB users; while the matrix cores work on a wave's tile n, the loads of its tile n + 1 are in
// flight into registers (one wave per SIMD: nothing else would hide them).  A score survives only if it beats the user's current
// k-th best; survivors that pass the exclusion checks (binary searches) are appended to the user's buffer (the heap + everything
// one round of W tiles can add); once per round, buffers holding more than k entries are reduced to their top k and the threshold
// is raised.  After the first few tiles almost nothing survives.  (Round 3: the staging loop used to be 4-byte loads with a
// run-time division per element and no load in flight during the MFMAs -- 8.6 TFLOP/s at 1M x 1M, rank 128; see profiles/r03.)
template <int KP, int UB, bool VEC, int W>
__global__ __launch_bounds__(W * 64) void top_product_kernel(const float* __restrict__ U, const float* __restrict__ V,
                                                          int n_users, int n_items, int k_rank, int topk,
                                                          const int32_t* __restrict__ nr_ptr,
                                                          const int32_t* __restrict__ nr_idx,
                                                          const int32_t* __restrict__ excl, int n_excl,
                                                          float glob_mean, int32_t* __restrict__ res,
                                                          float* __restrict__ scores_out, int slice_items,
                                                          const int* __restrict__ user_flags) {
  constexpr int LDT = KP + 4, NK2 = KP / 2, kTopUsers = kTopBlock * UB, kTopWaves = W;
  const int kTopCap = top_cap(topk, W);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const TopLds s = top_carve<false>(smem, (size_t)W * 32 * LDT, kTopUsers, kTopCap, 2 * kTopUsers + 4, W, nullptr);
  float *sVal = s.val, *sThr = s.thr;
  int *sIdx = s.idx, *sCnt = s.cnt, *sNeed = s.need;

  const int tid = threadIdx.x, lane = tid & 63, wv = rfl(tid >> 6);
  const int u0 = blockIdx.x * kTopUsers;
  const int item_base = top_enter_slice(V, n_items, res, scores_out, slice_items, n_users, k_rank, topk);
  if (user_flags && !top_block_flagged<kTopUsers, W * 64>(user_flags, u0, n_users)) return;
  const int col = lane & 31, half = lane >> 5;
  top_reset_users(s, kTopUsers, W * 64);
  float afrag[UB][NK2];
  top_load_users(afrag, U, u0, n_users, k_rank, col, half);
  float* tile = s.tiles + wv * 32 * LDT;
  for (int e = lane; e < 32 * LDT; e += 64) tile[e] = 0.f;
  __syncthreads();

  const int n_tiles = (n_items + 31) / 32;
  const int rounds = (n_tiles + kTopWaves - 1) / kTopWaves;
  TopStager<KP, VEC, 64> stage(V, n_tiles, n_items, k_rank);
  stage.load(wv);
  stage.store(tile, wv);
  wave_sync();
  for (int rd = 0; rd < rounds; rd++) {
    const int tl = rd * kTopWaves + wv;
    stage.load(tl + kTopWaves);   // the next tile's loads fly during this tile's MFMAs
    if (tl < n_tiles) {
      const int i0 = tl * 32;
      f32x16 acc[UB];
      top_sweep(acc, afrag, tile + col * LDT + half);
      const int item = i0 + col, gitem = item + item_base;
      const bool item_ok = item < n_items && !(n_excl > 0 && sorted_contains(excl, n_excl, gitem));
#pragma unroll
      for (int ub = 0; ub < UB; ub++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
          const int ul = 32 * ub + (e & 3) + 8 * (e >> 2) + 4 * half;
          const int u = u0 + ul;
          const float sc = acc[ub][e];
          if (item_ok && u < n_users && sc > sThr[ul]) {
            bool skip = false;
            if (nr_ptr) {
              const int p1 = nr_ptr[u], p2 = nr_ptr[u + 1];
              skip = sorted_contains(nr_idx + p1, p2 - p1, gitem);
            }
            if (!skip) {
              const int pos = atomicAdd(&sCnt[ul], 1);
              if (pos < kTopCap) {
                sVal[ul * kTopCap + pos] = sc;
                sIdx[ul * kTopCap + pos] = gitem;
              }
            }
          }
        }
    }
    wave_sync();                 // this wave has read its tile for the last time
    stage.store(tile, tl + kTopWaves);
    __syncthreads();
    // reduce over-full buffers to their top k (one wave per user), raise the threshold
    for (int ul = wv; ul < kTopUsers; ul += kTopWaves) {
      const int n = min(sCnt[ul], kTopCap);
      if (n > topk) {  // wave-uniform
        const float thr = topk_reduce_user(sVal + ul * kTopCap, sIdx + ul * kTopCap, s.tmpv + wv * kTopCap, s.tmpi + wv * kTopCap, n,
                                           topk, sNeed[ul], lane);
        if (lane == 0) {
          sCnt[ul] = topk;
          sThr[ul] = thr;
          sNeed[ul] = topk;
        }
      }
    }
    __syncthreads();
  }
  for (int ul = wv; ul < kTopUsers; ul += kTopWaves) {
    const int u = u0 + ul;
    if (u >= n_users) continue;
    topk_emit_user(sVal + ul * kTopCap, sIdx + ul * kTopCap, min(min(sCnt[ul], kTopCap), topk), topk, lane, glob_mean,
                   res + (size_t)u * topk, scores_out + (size_t)u * topk);
  }
}

// Round 4: the four waves SHARE one item tile and own 32 users each (128 users per workgroup).  The kernel above
// reads every item vector once per 32 UB users -- at 1M x 1M, rank 128 that is 8 TB through the L2 for 64 users per
// workgroup, and the matrix cores wait for it (52.7 TFLOP/s; one user block, as top-100 needs there, 9) --, this one once per
// 128: the tile is staged cooperatively (the next tile's 16-byte loads fly during this tile's MFMAs, as above), every
// wave multiplies it with its own user block, and because a wave owns its users' candidate buffers outright the buffers
// need room for ONE tile's survivors only (cap = k + 32) and are reduced by their wave without a workgroup barrier.
template <int KP, bool VEC>
__global__ __launch_bounds__(256) void top_product_shared_kernel(const float* __restrict__ U, const float* __restrict__ V,
                                                                 int n_users, int n_items, int k_rank, int topk,
                                                                 const int32_t* __restrict__ nr_ptr,
                                                                 const int32_t* __restrict__ nr_idx,
                                                                 const int32_t* __restrict__ excl, int n_excl,
                                                                 float glob_mean, int32_t* __restrict__ res,
                                                                 float* __restrict__ scores_out, int slice_items,
                                                                 const int* __restrict__ user_flags) {
  constexpr int UB = 1;   // user blocks per wave (two never fit where the two-tile kernel with one does not)
  constexpr int LDT = KP + 4, NK2 = KP / 2, USERS = 4 * kTopBlock * UB, UPW = 32 * UB;   // users per wave
  const int cap = top_cap(topk, 1);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const TopLds s = top_carve<false>(smem, (size_t)32 * LDT, USERS, cap, USERS, 4, nullptr);
  float* tile = s.tiles;

  const int tid = threadIdx.x, lane = tid & 63, wv = rfl(tid >> 6);
  const int u0 = blockIdx.x * USERS, uw = wv * UPW;                 // this wave's users: [u0 + uw, u0 + uw + UPW)
  const int item_base = top_enter_slice(V, n_items, res, scores_out, slice_items, n_users, k_rank, topk);
  if (user_flags && !top_block_flagged<USERS, 256>(user_flags, u0, n_users)) return;
  const int col = lane & 31, half = lane >> 5;
  top_reset_users(s, USERS, 256);
  float afrag[UB][NK2];
  top_load_users(afrag, U, u0 + uw, n_users, k_rank, col, half);
  for (int e = tid; e < 32 * LDT; e += 256) tile[e] = 0.f;
  __syncthreads();

  const int n_tiles = (n_items + 31) / 32;
  TopStager<KP, VEC, 256> stage(V, n_tiles, n_items, k_rank);
  stage.load(0);
  stage.store(tile, 0);
  __syncthreads();
  for (int tl = 0; tl < n_tiles; tl++) {
    stage.load(tl + 1);   // the next tile's loads fly during this tile's MFMAs
    f32x16 acc[UB];
    top_sweep(acc, afrag, tile + col * LDT + half);
    const int item = tl * 32 + col;
    const bool item_ok = item < n_items;
    float4 thr4[UB][4];
    top_load_thresholds(thr4, s.thr + uw, half);
#pragma unroll
    for (int ub = 0; ub < UB; ub++)
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int ul = uw + 32 * ub + (e & 3) + 8 * (e >> 2) + 4 * half;
        top_append(s, item_ok && u0 + ul < n_users, acc[ub][e], thr4, ub, e, ul, item + item_base, cap);
      }
    wave_sync();
    top_settle_wave<false, UPW>(s, uw, topk, cap, topk, nr_ptr, nr_idx, u0, excl, n_excl, wv, lane);
    __syncthreads();             // every wave has read the tile for the last time
    stage.store(tile, tl + 1);
    __syncthreads();
  }
  top_finish_wave<false, UPW>(s, uw, cap, topk, n_users, nr_ptr, nr_idx, u0, excl, n_excl, glob_mean, res, scores_out, wv, lane);
}

// The same with the epilogue hidden behind the NEXT tile's matrix instructions (round 4).  One wave per SIMD (the user blocks
// take 128 registers, the accumulators 32): nothing else runs while a wave compares its 32 scores per lane with the users'
// thresholds, so in the kernel above the matrix cores idle for that part of every tile.  Here two tiles are resident in LDS
// and two accumulator sets alternate: the MFMAs of tile t + 1 are issued in chunks of KP / 32 k-steps between the
// accumulator entries of tile t (a matrix instruction executes for 64 cycles after it has been issued; the compares, the rare
// appends and the buffer reductions of tile t run meanwhile), and one barrier per tile is enough -- tile t + 2 lands in the
// buffer whose last reader finished before the previous barrier.
// GBUF: the candidate buffers are this workgroup's slot of the global scratch ([USERS][cap] scores, then as many indices), with
// room for a batch of arrivals (top_gcap): a user is settled when its count passes cap - 32 (room for one tile's arrivals).
template <int KP, int UB, bool VEC, bool GBUF = false>
__global__ __launch_bounds__(256) void top_product_pipe_kernel(const float* __restrict__ U, const float* __restrict__ V,
                                                               int n_users, int n_items, int k_rank, int topk,
                                                               const int32_t* __restrict__ nr_ptr,
                                                               const int32_t* __restrict__ nr_idx,
                                                               const int32_t* __restrict__ excl, int n_excl,
                                                               float glob_mean, int32_t* __restrict__ res,
                                                               float* __restrict__ scores_out, int slice_items,
                                                               const int* __restrict__ user_flags, float* gbuf) {
  constexpr int LDT = KP + 4, NK2 = KP / 2, USERS = 4 * kTopBlock * UB, UPW = 32 * UB;
  constexpr int CH = NK2 / 16;   // k-steps (x UB matrix instructions) issued per accumulator entry of the previous tile
  const int cap = GBUF ? top_gcap(topk) : top_cap(topk, 1);
  const int settle_at = GBUF ? cap - 32 : topk;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const TopLds s = top_carve<GBUF>(smem, (size_t)2 * 32 * LDT, USERS, cap, USERS, 4,
                                       GBUF ? gbuf + (size_t)blockIdx.x * 2 * USERS * cap : nullptr);
  float* tiles = s.tiles;                                           // [2][32][LDT]

  const int tid = threadIdx.x, lane = tid & 63, wv = rfl(tid >> 6);
  const int uw = wv * UPW;
  const int item_base = top_enter_slice(V, n_items, res, scores_out, slice_items, n_users, k_rank, topk);
  // A workgroup takes the user blocks blockIdx.x, + gridDim.x, ...: one block each in the ordinary launch; the fall-back launch for
  // flagged users (user_flags) comes with a grid of at most 512 and every workgroup walks its blocks' flags -- a workgroup that only
  // finds out that it has nothing to do still costs 6..12 us of a CU that it owns alone (150 KB of LDS, 512 registers per lane),
  // and a grid of one such workgroup per block was 7 % (top-10) / 11 % (top-100) of a call that flags nobody (round 6, rocprof)
  const int n_blocks = (n_users + USERS - 1) / USERS;
  for (int blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
  const int u0 = blk * USERS;
  if (user_flags && !top_block_flagged<USERS, 256>(user_flags, u0, n_users)) continue;
  const int col = lane & 31, half = lane >> 5;
  top_reset_users(s, USERS, 256);
  float afrag[UB][NK2];
  top_load_users(afrag, U, u0 + uw, n_users, k_rank, col, half);
  for (int e = tid; e < 2 * 32 * LDT; e += 256) tiles[e] = 0.f;
  __syncthreads();

  const int n_tiles = (n_items + 31) / 32;
  TopStager<KP, VEC, 256> stage(V, n_tiles, n_items, k_rank);
  // tile 0 -> LDS, its products (nothing to hide them behind), tile 1 -> LDS
  stage.load(0);
  stage.store(tiles, 0);
  stage.load(1);
  __syncthreads();
  f32x16 acc[2][UB];   // [tile parity]
  top_sweep(acc[0], afrag, tiles + col * LDT + half);
  stage.store(tiles + 32 * LDT, 1);
  __syncthreads();

  auto body = [&](const int tl, f32x16 (&cur)[UB], f32x16 (&nxt)[UB]) {
    // cur: scores of tile tl; LDS buffer (tl + 1) & 1 holds tile tl + 1
    stage.load(tl + 2);
    const float* tn = tiles + ((tl + 1) & 1) * 32 * LDT + col * LDT + half;
    const int item = tl * 32 + col;
    const bool item_ok = item < n_items;
    float4 thr4[UB][4];
    top_load_thresholds(thr4, s.thr + uw, half);
#pragma unroll
    for (int ub = 0; ub < UB; ub++)
#pragma unroll
      for (int e = 0; e < 16; e++) nxt[ub][e] = 0.f;
    float bq[CH];
#pragma unroll
    for (int c = 0; c < CH; c++) bq[c] = tn[2 * c];
#pragma unroll
    for (int el = 0; el < 16; el++) {
      // the next tile's k-steps [el CH, el CH + CH) for every user block, then the operands of the chunk after it
#pragma unroll
      for (int c = 0; c < CH; c++)
#pragma unroll
        for (int ub = 0; ub < UB; ub++)
          nxt[ub] = __builtin_amdgcn_mfma_f32_32x32x2f32(afrag[ub][el * CH + c], bq[c], nxt[ub], 0, 0, 0);
      if (el + 1 < 16) {
#pragma unroll
        for (int c = 0; c < CH; c++) bq[c] = tn[2 * ((el + 1) * CH + c)];
      }
      __builtin_amdgcn_sched_barrier(0);
      // ... and entry el of every user block of the current tile
#pragma unroll
      for (int ub = 0; ub < UB; ub++) {
        const int ul = uw + 32 * ub + (el & 3) + 8 * (el >> 2) + 4 * half;
        top_append(s, item_ok && u0 + ul < n_users, cur[ub][el], thr4, ub, el, ul, item + item_base, cap);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    wave_sync();
    top_settle_wave<GBUF, UPW>(s, uw, settle_at, cap, topk, nr_ptr, nr_idx, u0, excl, n_excl, wv, lane);
    stage.store(tiles + (tl & 1) * 32 * LDT, tl + 2);   // into the buffer of tile tl: its last reader finished before the previous barrier
    __syncthreads();
  };
  for (int tl = 0; tl < n_tiles; tl += 2) {
    body(tl, acc[0], acc[1]);
    if (tl + 1 < n_tiles) body(tl + 1, acc[1], acc[0]);
  }
  top_finish_wave<GBUF, UPW>(s, uw, cap, topk, n_users, nr_ptr, nr_idx, u0, excl, n_excl, glob_mean, res, scores_out, wv, lane);
  __syncthreads();   // (the next block of this workgroup starts from the LDS areas again)
  }
}


// ---- few users, many items: the items split over the workgroups, the slices' lists merged (end of round 4) --------------------
// A call for a handful of users (the serving case) used to be ONE workgroup walking every item: 4.4 ms for one user over 100 k
// items, 33 ms for 1000 users, on 1..4 of 256 CUs.  Split launch: grid = (user blocks, item slices), every slice produces its own
// top k (exclusion lists applied, global item ids); one wave per user merges the S sorted lists.  The reference's result depends
// on the order of arrival only through candidates AT the k-th score (its heap replaces on strict >): the merged list is the
// sequential one whenever membership at that score is unambiguous -- no candidate left over at the k-th score, and no slice whose
// own k-th entry sits at it (that slice may have dropped equals).  Otherwise the user is flagged and the unsplit kernel, launched
// behind the merge with the flags, recomputes the workgroups that hold a flagged user (exact ties are degenerate inputs:
// tests/test_top_product.py has them).
__global__ __launch_bounds__(64) void top_merge_kernel(const float* __restrict__ sl_scores, const int32_t* __restrict__ sl_idx,
                                                       int n_slices, int n_users, int topk, float glob_mean,
                                                       int32_t* __restrict__ res, float* __restrict__ scores_out,
                                                       int* __restrict__ user_flags) {
  const int u = blockIdx.x, lane = threadIdx.x;
  const size_t ustride = (size_t)n_users * topk;
  const float* ls = sl_scores + (size_t)lane * ustride + (size_t)u * topk;
  const int32_t* li = sl_idx + (size_t)lane * ustride + (size_t)u * topk;
  const bool mine = lane < n_slices;
  int pos = 0;
  auto head = [&](float& hv, int& hi) {   // this slice's best unused entry (-inf: none)
    hv = -INFINITY;
    hi = INT32_MIN;
    if (mine && pos < topk) {
      const int ix = li[pos];
      if (ix != INT32_MIN) {
        hv = ls[pos];
        hi = ix;
      }
    }
  };
  float tau = -INFINITY;
  for (int out = 0; out < topk; out++) {
    float hv;
    int hi;
    head(hv, hi);
    float best = hv;
    for (int o = 32; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o));
    int bi = (hv == best && hi != INT32_MIN) ? hi : INT32_MIN;   // equal scores: the larger index first
    for (int o = 32; o > 0; o >>= 1) bi = max(bi, __shfl_xor(bi, o));
    if (bi == INT32_MIN) {   // fewer admissible items than k
      if (lane == 0) {
        res[(size_t)u * topk + out] = INT32_MIN;
        scores_out[(size_t)u * topk + out] = __int_as_float(0x7fc00000);
      }
      tau = -INFINITY;
    } else {
      if (lane == 0) {
        res[(size_t)u * topk + out] = bi;
        scores_out[(size_t)u * topk + out] = best + glob_mean;
      }
      if (hi == bi && hv == best) pos++;
      tau = best;
    }
  }
  // ambiguity at the k-th score
  float hv;
  int hi;
  head(hv, hi);
  bool amb = false;
  if (tau > -INFINITY) {
    amb = hv == tau;                                                      // a candidate left over at tau
    if (mine && li[topk - 1] != INT32_MIN && ls[topk - 1] == tau) amb = true;   // a full slice list that ends at tau
  }
  if (__any(amb) && lane == 0) user_flags[u] = 1;
}

}  // namespace

namespace {
// the product kernel of a plan row (VEC: rank a multiple of 4 and V 16-byte aligned -- a property of the pointers, not of the plan)
template <int KP, bool VEC>
const void* top_kernel_of(const TopGeo& g) {
  if (g.family == kTopShared) return reinterpret_cast<const void*>(top_product_shared_kernel<KP, VEC>);
  if (g.family == kTopPipe) {
    if constexpr (KP <= 128) {
      if (g.UB == 2 && g.gbuf) return reinterpret_cast<const void*>(top_product_pipe_kernel<KP, 2, VEC, true>);
      if (g.UB == 2) return reinterpret_cast<const void*>(top_product_pipe_kernel<KP, 2, VEC>);
    }
    return reinterpret_cast<const void*>(top_product_pipe_kernel<KP, 1, VEC>);
  }
  if constexpr (KP <= 128) {
    if (g.UB == 2) return reinterpret_cast<const void*>(top_product_kernel<KP, 2, VEC, 4>);
    if (g.W == 4) return reinterpret_cast<const void*>(top_product_kernel<KP, 1, VEC, 4>);
  }
  if constexpr (KP >= 128) return reinterpret_cast<const void*>(top_product_kernel<KP, 1, VEC, 2>);
  return nullptr;
}
template <bool VEC>
const void* top_kernel_of(const TopGeo& g) {
  return g.KP == 32 ? top_kernel_of<32, VEC>(g) : g.KP == 64 ? top_kernel_of<64, VEC>(g) : g.KP == 128 ? top_kernel_of<128, VEC>(g)
                                                                                                        : top_kernel_of<256, VEC>(g);
}

struct TopArgs {   // what every launch of a call shares
  const float* V;
  int n_items, k_rank;
  const int32_t *nr_ptr, *nr_idx, *excl;
  int n_excl;
  hipStream_t s;
};
// one row of the plan: U / nr_ptr / res / scores of the whole call (the row's first user is applied here), `scratch` where the
// row keeps its candidate buffers there
hipError_t launch_top_row(const TopLaunch& l, const TopArgs& a, const float* U, float glob_mean, int32_t* res, float* scores,
                          const int* user_flags, float* scratch) {
  const float* V = a.V;
  const bool vec = a.k_rank % 4 == 0 && (reinterpret_cast<uintptr_t>(V) & 15) == 0;
  const void* kern = vec ? top_kernel_of<true>(l.geo) : top_kernel_of<false>(l.geo);
  if (!kern) return hipErrorInvalidValue;
  hipError_t err;
  if ((err = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.geo.lds)) != hipSuccess) return err;
  U += (size_t)l.user0 * a.k_rank;
  res += (size_t)l.user0 * l.topk;
  scores += (size_t)l.user0 * l.topk;
  const int32_t *nr_ptr = a.nr_ptr ? a.nr_ptr + l.user0 : nullptr, *nr_idx = a.nr_idx, *excl = a.excl;
  int n_users = l.n_users, n_items = a.n_items, k_rank = a.k_rank, topk = l.topk, n_excl = a.n_excl, slice_items = l.slice_items;
  float* gbuf = l.geo.gbuf ? scratch : nullptr;
  // (the two-tile kernel takes the global candidate scratch as its last parameter; the others have no such parameter)
  void* args[] = {&U,      &V,          &n_users, &n_items, &k_rank,      &topk,       &nr_ptr, &nr_idx,
                  &excl,   &n_excl,     &glob_mean, &res,   &scores,      &slice_items, &user_flags, &gbuf};
  return hipLaunchKernel(kern, dim3(l.grid_x, l.n_slices), dim3(l.geo.threads), args, l.geo.lds, a.s);
}

// the nominating pass of a plan.  scratch (nullable): what the plan was made with
hipError_t launch_top_first(const TopPlan& p, const TopArgs& a, const float* U, int n_users, float glob_mean, int32_t* res,
                            float* scores, float* scratch) {
  if (!p.valid) return hipErrorInvalidValue;
  hipError_t err = hipSuccess;
  if (p.n_slices <= 1) {
    for (int i = 0; i < p.n_first && err == hipSuccess; i++)
      err = launch_top_row(p.launches[i], a, U, glob_mean, res, scores, nullptr, scratch);
    return err;
  }
  const TopLaunch& sliced = p.launches[0];
  const size_t ent = (size_t)p.n_slices * n_users * sliced.topk;
  float* sl_scores = scratch;
  int32_t* sl_idx = reinterpret_cast<int32_t*>(scratch + ent);
  int* flags = reinterpret_cast<int*>(sl_idx + ent);
  if ((err = hipMemsetAsync(flags, 0, (size_t)n_users * sizeof(int), a.s)) != hipSuccess) return err;
  if ((err = launch_top_row(sliced, a, U, 0.f, sl_idx, sl_scores, nullptr, nullptr)) != hipSuccess) return err;
  hipLaunchKernelGGL(top_merge_kernel, dim3(n_users), dim3(64), 0, a.s, sl_scores, sl_idx, p.n_slices, n_users, sliced.topk,
                     glob_mean, res, scores, flags);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  return launch_top_row(p.launches[1], a, U, glob_mean, res, scores, flags, nullptr);
}
}  // namespace

// ---- `$predict` that orders like the reference: candidates re-scored in double ----
// find_top_product casts both factor matrices to double before the product (R/utils.R:35-36) and top_product takes arma::mat
// (src/matrix_top_product.cpp:20): fp32 scores can swap items whose scores differ by ~1e-7 relative.  The fp32 matrix-core pass
// therefore only NOMINATES: it keeps the kc = k + extra best items of every user; one wave per user then recomputes those kc
// scores in double (from the double factors where the model holds them, else from the fp32 ones widened), and replays the
// reference's heap over the candidates in ascending item order.  That replay is the reference's result as long as every
// item whose double score reaches the k-th best is among the candidates: the final heap depends only on those items (items
// below the k-th score are evicted before any of them and never block one).  Equal scores: the larger index first; more
// candidates AT the k-th score than places: the survivors are the ones the heap keeps -- an arrival at the bound does not
// enter a full heap, a better arrival evicts the bound's smallest index.
// amb_out (pass 1, nullable): set for a user whose candidate list may not hold every item at the k-th score -- the list is full,
// its last entry sits AT that score, better items exist and the bound has more candidates than places: items of the bound
// that the larger heap of the fp32 pass evicted would have changed which of them the reference's heap keeps.  Such users are
// recomputed by the fp32 kernel with the reference's heap at capacity k (launch_top_product_f64) and only sorted here
// (pass 2: only_flagged = the same array, kc == topk).
template <class TF>
__global__ __launch_bounds__(256) void top_rescore_kernel(const TF* __restrict__ U, const TF* __restrict__ V, int n_users,
                                                          int rank, int kc, int topk, const int32_t* __restrict__ cand,
                                                          double glob_mean, int32_t* __restrict__ res,
                                                          double* __restrict__ scores, int* __restrict__ amb_out,
                                                          const int* __restrict__ only_flagged) {
  __shared__ double sU[4][256];
  __shared__ double sS[4][kTopMaxK];      // candidate scores
  __shared__ int sI[4][kTopMaxK];         // candidate items (0-based; -1 = none)
  __shared__ int sO[4][kTopMaxK];         // S (score >= v_k) in ascending item order: candidate slots
  __shared__ int sQ[4][kTopMaxK];         // replay: the bound's candidates inside the heap, oldest first
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int u = blockIdx.x * 4 + wv;
  if (u >= n_users) return;
  if (only_flagged && !only_flagged[u]) return;
  double* uu = sU[wv];
  double* cs = sS[wv];
  int* ci = sI[wv];
  for (int r = lane; r < rank; r += 64) uu[r] = (double)U[(size_t)u * rank + r];
  for (int c = lane; c < kc; c += 64) {
    const int ix = cand[(size_t)u * kc + c];
    ci[c] = ix == INT32_MIN ? -1 : ix - 1;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  // scores: the wave walks the candidates, lane l takes the elements l, l + 64, ... of the item's vector
  for (int c = 0; c < kc; c++) {
    const int it = ci[c];
    double acc = 0.0;
    if (it >= 0)
      for (int r = lane; r < rank; r += 64) acc = fma(uu[r], (double)V[(size_t)it * rank + r], acc);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) cs[c] = acc;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  // position of every candidate in the order (score descending, item descending); n_valid of them exist
  int n_valid = 0;
  for (int c = 0; c < kc; c++) n_valid += ci[c] >= 0 ? 1 : 0;
  const int kk = min(topk, n_valid);
  auto before = [&](const int a, const int b) {   // a ahead of b
    return cs[a] > cs[b] || (cs[a] == cs[b] && ci[a] > ci[b]);
  };
  constexpr int PER = kTopMaxK / 64;
  int pos[PER];
#pragma unroll
  for (int e = 0; e < PER; e++) {
    const int c = lane + 64 * e;
    int p = -1;
    if (c < kc && ci[c] >= 0) {
      p = 0;
      for (int o = 0; o < kc; o++) p += (ci[o] >= 0 && o != c && before(o, c)) ? 1 : 0;
    }
    pos[e] = p;
  }
  // the k-th best score, how many candidates beat it (g) and how many sit at it (nt)
  double vk = 0.0;
  int g = 0, nt = 0;
  if (kk > 0) {
    int who = -1;
#pragma unroll
    for (int e = 0; e < PER; e++)
      if (pos[e] == kk - 1) who = lane + 64 * e;
    const unsigned long long m = __ballot(who >= 0);
    const int src = __ffsll((long long)m) - 1;
    who = __shfl(who, src);
    vk = cs[who];
    double vmin = vk;
    for (int c = 0; c < kc; c++) {
      g += (ci[c] >= 0 && cs[c] > vk) ? 1 : 0;
      nt += (ci[c] >= 0 && cs[c] == vk) ? 1 : 0;
      if (ci[c] >= 0) vmin = fmin(vmin, cs[c]);
    }
    if (amb_out && lane == 0 && n_valid == kc && kc > topk && vmin == vk && g > 0 && g + nt > kk) amb_out[u] = 1;
  }
  int32_t* ru = res + (size_t)u * topk;
  double* su = scores + (size_t)u * topk;
  if (g + nt <= kk) {
    // no more candidates at the bound than places: the first kk positions are the answer
#pragma unroll
    for (int e = 0; e < PER; e++) {
      const int c = lane + 64 * e;
      if (pos[e] >= 0 && pos[e] < kk) {
        ru[pos[e]] = ci[c] + 1;
        su[pos[e]] = cs[c] + glob_mean;
      }
    }
  } else {
    // replay of the heap over S = {score >= v_k} in ascending item order (rare: exact ties at the bound)
    int* so = sO[wv];
    int* q = sQ[wv];
#pragma unroll
    for (int e = 0; e < PER; e++) {
      const int c = lane + 64 * e;
      if (c < kc && ci[c] >= 0 && cs[c] >= vk) {
        int r = 0;
        for (int o = 0; o < kc; o++) r += (ci[o] >= 0 && cs[o] >= vk && ci[o] < ci[c]) ? 1 : 0;
        so[r] = c;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    int head = 0, tail = 0;
    if (lane == 0) {
      int cnt = 0;
      for (int e = 0; e < g + nt; e++) {
        const int c = so[e];
        if (cs[c] > vk) {
          if (cnt < kk) cnt++;
          else head++;               // evicts the smallest (score, item) pair: the bound's oldest = smallest index
        } else if (cnt < kk) {
          q[tail++] = c;
          cnt++;
        }
      }
    }
    head = __shfl(head, 0);
    tail = __shfl(tail, 0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int e = 0; e < PER; e++) {
      const int c = lane + 64 * e;
      if (pos[e] >= 0 && cs[c] > vk) {   // better than the bound: positions 0 .. g - 1 as they stand
        ru[pos[e]] = ci[c] + 1;
        su[pos[e]] = cs[c] + glob_mean;
      }
    }
    // the survivors at the bound, larger index first: q[head .. tail) is ascending in item
    for (int e = head + lane; e < tail; e += 64) {
      const int c = q[e];
      const int at = g + (tail - 1 - e);
      ru[at] = ci[c] + 1;
      su[at] = cs[c] + glob_mean;
    }
  }
  for (int c = kk + lane; c < topk; c += 64) {   // fewer admissible items than k: NA_integer_ / NA_real_
    ru[c] = INT32_MIN;
    su[c] = __longlong_as_double(0x7ff8000000000000ll);
  }
}

// The whole `$predict` that orders like the reference.  U32 / V32: the fp32 factors (the nominating pass); U64 / V64: the double
// ones (nullable as a pair: the fp32 factors widened).  scratch: n_users * (kc + topk) ints + as many floats + n_users ints
// (top_product_f64_scratch_words).  Steps: (1) the fp32 kernel keeps kc = k + extra candidates per user; (2) one wave per user
// recomputes their scores in double and replays the reference's heap (top_rescore_kernel), flagging the users whose candidate
// list may be missing items at the k-th score; (3) the workgroups of the fp32 kernel that hold a flagged user run again at
// capacity k -- the reference's own heap, exact ties included -- and (4) those users' k items are re-scored and sorted.  No host
// round trip: without flagged users (3) and (4) are launches whose workgroups return at once.
size_t top_product_f64_scratch_words(int n_users, int kc, int topk) {
  return (size_t)n_users * ((size_t)2 * kc + 2 * topk + 1) + 64;
}
template <class TF>
hipError_t launch_top_product_f64_t(const float* U32, const float* V32, const TF* U, const TF* V, int n_users, int n_items,
                                    int rank, int topk, int kc, const int32_t* nr_ptr, const int32_t* nr_idx, const int32_t* excl,
                                    int n_excl, double glob_mean, int32_t* res, double* scores, hipStream_t s, float* scratch,
                                    float* split_scratch) {
  if (n_users <= 0) return hipSuccess;
  if (kc < topk || kc > kTopMaxK || topk < 1 || rank < 1 || rank > 256) return hipErrorInvalidValue;
  int32_t* cand = reinterpret_cast<int32_t*>(scratch);
  float* cand_sc = scratch + (size_t)n_users * kc;
  int32_t* res2 = reinterpret_cast<int32_t*>(cand_sc + (size_t)n_users * kc);
  float* sc2 = reinterpret_cast<float*>(res2 + (size_t)n_users * topk);
  int* flags = reinterpret_cast<int*>(sc2 + (size_t)n_users * topk);
  const TopPlan plan = top_product_plan(n_users, n_items, rank, kc, topk, true, split_scratch != nullptr);
  const TopArgs a{V32, n_items, rank, nr_ptr, nr_idx, excl, n_excl, s};
  hipError_t err;
  if ((err = launch_top_first(plan, a, U32, n_users, 0.f, cand, cand_sc, split_scratch)) != hipSuccess) return err;
  if ((err = hipMemsetAsync(flags, 0, (size_t)n_users * sizeof(int), s)) != hipSuccess) return err;
  const dim3 grid((n_users + 3) / 4);
  hipLaunchKernelGGL(top_rescore_kernel<TF>, grid, dim3(256), 0, s, U, V, n_users, rank, kc, topk, cand, glob_mean, res, scores,
                     flags, static_cast<const int*>(nullptr));
  if ((err = hipGetLastError()) != hipSuccess) return err;
  if (kc > topk) {
    if ((err = launch_top_row(plan.launches.back(), a, U32, 0.f, res2, sc2, flags, split_scratch)) != hipSuccess) return err;
    hipLaunchKernelGGL(top_rescore_kernel<TF>, grid, dim3(256), 0, s, U, V, n_users, rank, topk, topk, res2, glob_mean, res, scores,
                       static_cast<int*>(nullptr), flags);
    if ((err = hipGetLastError()) != hipSuccess) return err;
  }
  return hipSuccess;
}
hipError_t launch_top_product_f64(const float* U32, const float* V32, const double* U64, const double* V64, int n_users,
                                  int n_items, int rank, int topk, int kc, const int32_t* nr_ptr, const int32_t* nr_idx,
                                  const int32_t* excl, int n_excl, double glob_mean, int32_t* res, double* scores, hipStream_t s,
                                  float* scratch, float* split_scratch) {
  if (U64 && V64)
    return launch_top_product_f64_t<double>(U32, V32, U64, V64, n_users, n_items, rank, topk, kc, nr_ptr, nr_idx, excl, n_excl,
                                            glob_mean, res, scores, s, scratch, split_scratch);
  return launch_top_product_f64_t<float>(U32, V32, U32, V32, n_users, n_items, rank, topk, kc, nr_ptr, nr_idx, excl, n_excl,
                                         glob_mean, res, scores, s, scratch, split_scratch);
}

// scratch (nullable): top_product_plan(...).scratch_floats floats
hipError_t launch_top_product(const float* U, const float* V, int n_users, int n_items, int k_rank, int topk,
                              const int32_t* nr_ptr, const int32_t* nr_idx, const int32_t* excl, int n_excl,
                              float glob_mean, int32_t* res, float* scores, hipStream_t s, float* scratch) {
  const TopPlan plan = top_product_plan(n_users, n_items, k_rank, topk, topk, false, scratch != nullptr);
  return launch_top_first(plan, TopArgs{V, n_items, k_rank, nr_ptr, nr_idx, excl, n_excl, s}, U, n_users, glob_mean, res, scores,
                          scratch);
}

}  // namespace rsparse_hip
