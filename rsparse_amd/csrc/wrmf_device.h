// Device-side building blocks shared by the ALS kernels (gfx950 / wave64 only).
//
// Lane <-> data mappings used throughout (KP = rank padded to 32/64/128, T = tile capacity in
// non-zeros, one tile row = one gathered factor vector, row stride LDT = KP + 4 floats):
//
//   "k-mode"    lane l owns vector elements [l*EPL, l*EPL+EPL), EPL = KP/64 (1 for KP <= 64):
//               CG state x, r, p, Ap live in registers this way; u = X_nnz * w is an AXPY over
//               tile rows (contiguous ds_read_b64 per lane, conflict free).
//   "nnz-mode"  lane l owns non-zero j = l % T and the k-range split h = l / T:
//               t = X_nnz^T v is a per-lane dot product down a tile row (ds_read_b128; the +4 pad
//               makes the 16-lane service groups hit distinct banks) followed by a log2(64/T)-step
//               cross-split shuffle.  Lane j then holds t_j, c_j, w_j.
//
// The two GEMVs of every CG step therefore read the same LDS tile in its two orientations and
// nothing is transposed or re-gathered.
#pragma once
#include <hip/hip_runtime.h>

#include "wrmf_internal.h"
#include "wrmf_wave.h"

namespace rsparse_hip {
namespace dev {

template <int KP>
struct Geo {
  static constexpr int EPL = KP >= 64 ? KP / 64 : 1;
  static constexpr int LDT = KP + 4;
};

// t_j = sum_k tile[j][k] * vec[k]; returned in every lane whose (lane % T) == j.
template <int KP, int T>
__device__ __forceinline__ float tile_dot(const float* tile, const float* vec, int lane) {
  constexpr int S = 64 / T, HK = KP / S, LDT = Geo<KP>::LDT;
  static_assert(HK % 4 == 0, "k-range per split must be a multiple of 4");
  const int j = lane % T, h = lane / T;
  const float4* a = reinterpret_cast<const float4*>(tile + j * LDT + h * HK);
  const float4* b = reinterpret_cast<const float4*>(vec + h * HK);
  float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
#pragma unroll
  for (int q = 0; q < HK / 4; q++) {
    const float4 av = a[q], bv = b[q];
    t0 = fmaf(av.x, bv.x, t0);
    t1 = fmaf(av.y, bv.y, t1);
    t2 = fmaf(av.z, bv.z, t2);
    t3 = fmaf(av.w, bv.w, t3);
  }
  float t = (t0 + t1) + (t2 + t3);
#pragma unroll
  for (int m = T; m < 64; m <<= 1) t += __shfl_xor(t, m);
  return t;
}

// acc += sum_{j<cnt} w_j * tile[j][:]   (k-mode); w_j is read from lane j.
template <int KP>
__device__ __forceinline__ void tile_axpy(const float* tile, float w, int cnt, int lane, bool active,
                                          float (&acc)[Geo<KP>::EPL]) {
  constexpr int EPL = Geo<KP>::EPL, LDT = Geo<KP>::LDT;
  const float* col = tile + lane * EPL;
  auto step = [&](int j) {
    const float wj = readlane_f(w, j);
    if constexpr (EPL == 2) {
      const float2 xv = *reinterpret_cast<const float2*>(col + j * LDT);
      acc[0] = fmaf(wj, xv.x, acc[0]);
      acc[1] = fmaf(wj, xv.y, acc[1]);
    } else {
      const float xv = active ? col[j * LDT] : 0.f;
      acc[0] = fmaf(wj, xv, acc[0]);
    }
  };
  int j = 0;
  for (; j + 4 <= cnt; j += 4) {  // hand-unrolled: the readlane keeps the compiler from doing it
    step(j);
    step(j + 1);
    step(j + 2);
    step(j + 3);
  }
  for (; j < cnt; j++) step(j);
}

// acc += sign * sum_{kk in [kk0,kk1)} G[kk][:] * vec[kk]   (G symmetric KP x KP in LDS, k-mode).
template <int KP>
__device__ __forceinline__ void gram_mv(const float* sG, const float* vec, int kk0, int kk1, int lane,
                                        bool active, float sign, float (&acc)[Geo<KP>::EPL]) {
  constexpr int EPL = Geo<KP>::EPL;
  float part[EPL];
#pragma unroll
  for (int u = 0; u < EPL; u++) part[u] = 0.f;
  const float* col = sG + lane * EPL;
#pragma unroll 2
  for (int kk = kk0; kk < kk1; kk += 4) {
    const float4 vb = *reinterpret_cast<const float4*>(vec + kk);
    const float vv[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
    for (int u4 = 0; u4 < 4; u4++) {
      if constexpr (EPL == 2) {
        const float2 g = *reinterpret_cast<const float2*>(col + (kk + u4) * KP);
        part[0] = fmaf(vv[u4], g.x, part[0]);
        part[1] = fmaf(vv[u4], g.y, part[1]);
      } else {
        const float g = active ? col[(kk + u4) * KP] : 0.f;
        part[0] = fmaf(vv[u4], g, part[0]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < EPL; u++) acc[u] = fmaf(sign, part[u], acc[u]);
}

template <int KP>
__device__ __forceinline__ void put_vec(float* vec, const float (&v)[Geo<KP>::EPL], int lane,
                                        bool active) {
  constexpr int EPL = Geo<KP>::EPL;
  if constexpr (EPL == 2) {
    *reinterpret_cast<float2*>(vec + lane * 2) = make_float2(v[0], v[1]);
  } else {
    if (active) vec[lane] = v[0];
  }
}

// Gather `cnt` (<= T) factor vectors X[:, idx_j] into tile rows 0..cnt-1.  idx_j is held by lane j.
// VEC: rank % 4 == 0 and X 16-byte aligned -> 16 B per lane, 64*16/(4*KP) vectors per instruction.
// Columns [k, KP) of the tile are never written with non-zeros (they were zeroed at kernel start).
template <int KP, int T, bool VEC>
__device__ __forceinline__ void gather_chunk(const float* __restrict__ X, int k, int myidx, int cnt,
                                             float* tile, int lane) {
  constexpr int LDT = Geo<KP>::LDT;
  if constexpr (VEC) {
    constexpr int LPV = KP / 4, VPI = 64 / LPV, NLD = T / VPI;
    const int c4 = lane % LPV, jo = lane / LPV;
    float4 buf[NLD];
#pragma unroll
    for (int q = 0; q < NLD; q++) {
      const int j = q * VPI + jo;
      const int id = __shfl(myidx, j);
      buf[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q * VPI < cnt) {  // wave-uniform
        if (j < cnt && c4 * 4 < k)
          buf[q] = *reinterpret_cast<const float4*>(X + (size_t)id * k + c4 * 4);
      }
    }
#pragma unroll
    for (int q = 0; q < NLD; q++) {
      const int j = q * VPI + jo;
      if (q * VPI < cnt) {
        if (j < cnt) *reinterpret_cast<float4*>(tile + j * LDT + c4 * 4) = buf[q];
      }
    }
  } else {
    for (int j = 0; j < cnt; j++) {
      const int id = __builtin_amdgcn_readlane(myidx, j);
      const float* src = X + (size_t)id * k;
      for (int e = lane; e < k; e += 64) tile[j * LDT + e] = src[e];
    }
  }
}

// The four waves of a workgroup gather one chunk of TC factor vectors of a row (non-zeros base .. base + ccnt - 1) into the tile
// sT, row stride KP + 4: wave wv fetches tile rows [TC/4 wv, TC/4 wv + TC/4).  VEC: all index loads, then all 16-byte vector loads
// of the wave are in flight together (2 dependent round trips per chunk).
template <int KP, bool VEC, int TC>
__device__ __forceinline__ void gather_chunk4(const AlsArgs& a, int base, int ccnt, float* sT, int wv, int lane) {
  constexpr int LDT = KP + 4, TCW = TC / 4;   // (TCW vectors of the chunk per wave)
  const int k = a.k;
  if constexpr (VEC) {
    constexpr int LPV = KP / 4, VPI = 64 / LPV, NQ = TCW / VPI;
    static_assert(NQ >= 1, "a wave's share of the chunk is at least one load instruction");
    const int c4 = lane % LPV, jo = lane / LPV;
    int ids[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) ids[q] = a.row_idx[base + min(TCW * wv + q * VPI + jo, ccnt - 1)];
    float4 v[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) v[q] = *reinterpret_cast<const float4*>(a.X + (size_t)ids[q] * k + min(c4 * 4, k - 4));
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const int j = TCW * wv + q * VPI + jo;
      if (j < ccnt && c4 * 4 < k) *reinterpret_cast<float4*>(sT + j * LDT + c4 * 4) = v[q];
    }
  } else {
    for (int j = TCW * wv; j < min(TCW * wv + TCW, ccnt); j++) {
      const int id = rfl(a.row_idx[base + j]);
      const float* src = a.X + (size_t)id * k;
      for (int e = lane; e < k; e += 64) sT[j * LDT + e] = src[e];
    }
  }
}

// The kth largest of the keys key(e, ok) (e < n; ok = false leaves the entry out) by a radix select on `nbits` bits, 8 per pass.
// A workgroup of 256 threads, all of which must call it.  Needs 1 <= kth <= the number of valid entries.  hist: 256 words,
// sres / srem: one each.  Integer arithmetic throughout: the result does not depend on the order of the atomics.
template <class KeyFn>
__device__ u64 block_kth_largest(int n, int kth, int nbits, KeyFn key, unsigned* hist, u64* sres, int* srem) {
  const int tid = threadIdx.x, lane = tid & 63;
  u64 prefix = 0;
  int rem = kth;
  for (int shift = nbits - 8; shift >= 0; shift -= 8) {
    hist[tid] = 0u;
    __syncthreads();
    const u64 hmask = shift + 8 >= 64 ? 0ull : (~0ull << (shift + 8));
    for (int e = tid; e < n; e += 256) {
      bool ok;
      const u64 k = key(e, ok);
      if (ok && (k & hmask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {   // bins from the top: lane l holds bins 255 - 4l .. 252 - 4l
      unsigned s = 0;
      for (int j = 0; j < 4; j++) s += hist[255 - 4 * lane - j];
      unsigned incl = s;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
      }
      const unsigned excl = incl - s;
      if (excl < (unsigned)rem && incl >= (unsigned)rem) {
        unsigned cum = excl;
        for (int j = 0; j < 4; j++) {
          const int b = 255 - 4 * lane - j;
          if (cum + hist[b] >= (unsigned)rem) {
            *sres = prefix | ((u64)b << shift);
            *srem = rem - (int)cum;
            break;
          }
          cum += hist[b];
        }
      }
    }
    __syncthreads();
    prefix = *sres;
    rem = *srem;
  }
  return prefix;
}

// ---- Philox4x32-10 (Random123; wrmf_init.hip, wrmf_sample.hip): counter (c0, c1, c2, c3), key (k0, k1) -> o[0..3] ----
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&o)[4]) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// ---- ordering a selection in LDS (wrmf_topk_large.hip, wrmf_candidates.hip) ----
// workgroup-wide exclusive prefix of a flag (256 threads); *total = the sum.  Uses sw[4].
__device__ __forceinline__ int block_prefix(bool f, int* sw, int* total) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const u64 m = __ballot(f);
  if (lane == 0) sw[wv] = __popcll(m);
  __syncthreads();
  int off = 0, tot = 0;
  for (int w = 0; w < 4; w++) {
    if (w < wv) off += sw[w];
    tot += sw[w];
  }
  __syncthreads();
  *total = tot;
  return off + __popcll(m & ((1ull << lane) - 1ull));
}

// bitonic sort of sk / si [0, P) (P a power of two): descending by (key, index), or ascending
__device__ inline void block_bitonic(u64* sk, int* si, int P, bool asc) {
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < P / 2; i += 256) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const u64 ka = sk[lo], kb = sk[hi];
        const int ia = si[lo], ib = si[hi];
        const bool b_first = asc ? (kb < ka || (kb == ka && ib < ia)) : (kb > ka || (kb == ka && ib > ia));
        if (((lo & size) == 0) == b_first) {
          sk[lo] = kb;
          sk[hi] = ka;
          si[lo] = ib;
          si[hi] = ia;
        }
      }
      __syncthreads();
    }
}

__device__ __forceinline__ int pow2_at_least(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// the kk ordered survivors (sk: order keys of double scores, si: 0-based items) and the padding of a row of topk outputs
template <class TO>
__device__ __forceinline__ void topl_emit(const u64* sk, const int* si, int kk, int topk, TO glob_mean, int32_t* ru, TO* su) {
  for (int p = threadIdx.x; p < topk; p += 256) {
    if (p < kk) {
      ru[p] = si[p] + 1;   // 1-based, like R
      su[p] = (TO)key_f64(sk[p]) + glob_mean;
    } else {
      ru[p] = INT32_MIN;   // NA_integer_ / NA_real_
      su[p] = (TO)__longlong_as_double(0x7ff8000000000000ll);
    }
  }
}

}  // namespace dev
}  // namespace rsparse_hip
