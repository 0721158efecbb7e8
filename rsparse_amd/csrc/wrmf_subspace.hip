// iALS++ (Rendle, Krichene, Zhang, Koren 2021): one BLOCK STEP of implicit ALS by subspace optimisation (gfx950, wave64, fp32;
// DESIGN.md 3.39; rsparse_amd/ialspp.py: ialspp_block_reference is the definition, include/rsparse_wrmf_hip.h repeats it).
//
// For the block pi = [c0, c0 + width) of the coordinates, width <= B, B = 32 or 64, and every row u of the side's CSR (P, J, X = c):
//     g = D[u] + lambda w_u,pi + sum_{i in row} ((c_ui - 1) e_ui - c_ui) h_i,pi
//     A = G_pi,pi + lambda I + sum_{i in row} (c_ui - 1) h_i,pi h_i,pi^T
//     delta = A^-1 g;   w_u,pi -= delta;   e_ui -= h_i,pi . delta for the row's entries
// D = W G[:, pi] (n x width) and G_pi,pi come from outside; e (one float per stored entry) and W are updated in place.  H is
// addressed by (ldh, c0, width) alone: nothing here knows the rank.
//
// Lane maps (n = lane % 32, hf = lane / 32; NT = B / 32 tiles per side):
//   gather    16-byte form (H 16-byte aligned, ldh, c0 and width multiples of 4): one instruction fetches 256 / B entries, lane l
//             the coordinates 4 (l % (B / 4)) .. + 3 of entry l / (B / 4) of the group; 4-byte form: lane l coordinate l % B of
//             entry l / B.  A chunk of TS entries is fetched into registers while the chunk before it is consumed, its indices
//             and values one chunk further ahead; it is then written to the LDS tile sT[entry][B + 4].
//   operands  entries are the K dimension of v_mfma_f32_32x32x2_f32: for the pair (2 s, 2 s + 1) lane (n, hf) reads
//             x_tb = sT[2 s + hf][32 tb + n]; the A operand is (c - 1) x_ta, the B operand x_tb, both exact fp32.
//   tiles     t[ta][tb], register v of lane (n, hf) = A[32 ta + 8 (v / 4) + 4 hf + v % 4][32 tb + n]: four tiles at B = 64 (the
//             two off-diagonal ones are each other's transpose: one more matrix instruction instead of a transposition), one at
//             B = 32.  Seeded with G_pi,pi + lambda I; rows and columns >= width: the identity.
//   g         lane (n, hf) sums coef x_tb over its entries (coef = (c - 1) e - c); the two halves are added by one lane swap.
//   solve     one lane swap per register pair turns the tiles into rows: lane i holds row i of A in B registers, then the
//             right-looking LDL^T of wrmf_chol_wave.hip (pivot row by DPP row broadcast inside the FMA) and both substitutions.
//   e         lane j takes entry j: h_j,pi . delta from the LDS tile where the row has at most kSubTile entries (it is still
//             there), else from a second gather of the row (16-byte loads, delta broadcast from LDS).
//
// Rows of more than kSubLongLen = 4 * kSubTile entries -- every wave of a workgroup then has more than one full tile of the short
// form to stream -- go to subspace_long_kernel: a SEGMENT of at most seg_len entries per workgroup, a quarter of it per wave
// (tiles of kSubLongTile entries: four of them and the partial fit the 64 KiB of a workgroup), the four waves' (A, g) added in
// LDS in ascending wave order.  A row of one segment is solved by wave 0 and e updated by the whole workgroup; a row of several
// segments writes its partials, subspace_finish_kernel adds them in ascending segment order and solves once, and
// subspace_apply_kernel updates e with one workgroup per segment.  seg_len grows with nnz (launch_subspace_block) so that the
// partials stay below 4096 + 2 slots: a row holding a tenth of the entries is still spread over ~200 workgroups.
// No float atomics; the integer atomics of the plan only decide WHERE a partial lies, never the order of a sum: repeated calls
// return the same bits.  A non-positive pivot leaves the row and its e untouched and is counted in *fails.
#include <algorithm>

#include "../../include/rsparse_wrmf_hip.h"
#include "wrmf_internal.h"
#include "wrmf_device.h"

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kSubTile = 64;       // entries in the short form's LDS tile
constexpr int kSubLongTile = 32;   // ... and in each wave's tile of the workgroup form
constexpr int kSubLongLen = RSPARSE_HIP_SUBSPACE_LONG_ROW;
static_assert(kSubLongLen == 4 * kSubTile, "the long-row edge is four waves' tiles of the short form");

struct SubArgs {
  const int32_t* P; const int32_t* J; const float* X;
  int n_rows;
  const float* H; int ldh;
  int c0, width;
  const float* G; int ldg;
  const float* D; int ldd;
  float lambda;
  float* W; int ldw;
  float* e;
  int* fails;
  // long rows (all in the workspace)
  int seg_len, cap_seg, cap_multi, cap_mseg;
  int* counters;   // [0] segments, [1] rows of several segments, [2] their segments, [3] rows the plan had no room for
  int* seg_row; int* seg_idx; int* seg_pslot; int* seg_m;
  int* multi_row; int* multi_first; int* multi_nseg;
  float* delta;      // 64 per row of several segments
  float* partials;   // PART per segment of such a row
};

template <int B>
struct SubGeo {
  static constexpr int NT = B / 32, LDT = B + 4, NREG = 16 * NT * NT + NT, PART = NREG * 64;
};

__device__ __forceinline__ bool sub_vec(const SubArgs& a) {
  return ((reinterpret_cast<uintptr_t>(a.H) & 15) == 0) && a.ldh % 4 == 0 && a.c0 % 4 == 0 && a.width % 4 == 0;
}

// t = G_pi,pi + lambda I, padded with the identity (seed) or zeros
template <int B>
__device__ __forceinline__ void sub_seed(const SubArgs& a, const bool seed, f32x16 (&t)[B / 32][B / 32], float (&u)[B / 32], const int lane) {
  constexpr int NT = B / 32;
  const int n = lane & 31, hf = lane >> 5;
#pragma unroll
  for (int ta = 0; ta < NT; ta++)
#pragma unroll
    for (int tb = 0; tb < NT; tb++)
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const int i = 32 * ta + 8 * (v >> 2) + 4 * hf + (v & 3), j = 32 * tb + n;
        float g = 0.f;
        if (seed) {
          if (i < a.width && j < a.width) g = a.G[(size_t)i * a.ldg + j] + (i == j ? a.lambda : 0.f);
          else g = i == j ? 1.f : 0.f;
        }
        t[ta][tb][v] = g;
      }
#pragma unroll
  for (int tb = 0; tb < NT; tb++) u[tb] = 0.f;
}

// (A, g) += the entries [q1, q2) of the CSR; sT: TS x (B + 4) floats, sW / sC: TS floats each, this wave's own
template <int B, int TS>
__device__ __forceinline__ void sub_assemble(const SubArgs& a, const int q1, const int q2, const bool vec, float* sT, float* sW, float* sC,
                                             f32x16 (&t)[B / 32][B / 32], float (&u)[B / 32], const int lane) {
  constexpr int NT = B / 32, LDT = B + 4, NR = TS * B / 64, LPV = B / 4, VPI = 64 / LPV, EPI = 64 / B;
  if (q2 <= q1) return;   // (wave-uniform)
  const int n = lane & 31, hf = lane >> 5;
  const int c4 = lane % LPV, jo = lane / LPV, ce = lane % B, je = lane / B;
  // a coordinate beyond the block reads coordinate 0 (in bounds) and is stored as 0
  const int voff = a.c0 + (4 * c4 < a.width ? 4 * c4 : 0), soff = a.c0 + (ce < a.width ? ce : 0);
  float buf[NR];
#pragma unroll
  for (int r = 0; r < NR; r++) buf[r] = 0.f;
  int idj = 0, idn = 0;
  float xv = 0.f, ev = 0.f, xn = 0.f, en = 0.f;
  auto meta = [&](const int base, int& id, float& x, float& e_) {
    const int jl = base + min(lane, q2 - base - 1);
    id = a.J[jl];
    x = a.X[jl];
    e_ = a.e[jl];
  };
  auto rows = [&](const int id, const int ccnt) {
    if (vec) {
#pragma unroll
      for (int q = 0; q < NR / 4; q++)
        if (q * VPI < ccnt) {   // (wave-uniform)
          const int idq = __shfl(id, min(q * VPI + jo, ccnt - 1));
          const float4 v = *reinterpret_cast<const float4*>(a.H + (size_t)idq * a.ldh + voff);
          buf[4 * q] = v.x; buf[4 * q + 1] = v.y; buf[4 * q + 2] = v.z; buf[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
      for (int r = 0; r < NR; r++)
        if (r * EPI < ccnt) {
          const int idq = __shfl(id, min(r * EPI + je, ccnt - 1));
          buf[r] = a.H[(size_t)idq * a.ldh + soff];
        }
    }
  };
  const int nch = (q2 - q1 + TS - 1) / TS;
  meta(q1, idj, xv, ev);
  rows(idj, min(TS, q2 - q1));
  if (nch > 1) meta(q1 + TS, idn, xn, en);
  for (int c = 0; c < nch; c++) {
    const int base = q1 + c * TS, ccnt = min(TS, q2 - base), ce2 = (ccnt + 1) & ~1;
    wave_sync();
    // the chunk into the tile: entries [ccnt, ce2) and the coordinates beyond the block as zeros
    if (vec) {
#pragma unroll
      for (int q = 0; q < NR / 4; q++)
        if (q * VPI < ce2) {
          const int j = q * VPI + jo;
          const bool ok = j < ccnt && 4 * c4 < a.width;
          *reinterpret_cast<float4*>(sT + j * LDT + 4 * c4) =
              make_float4(ok ? buf[4 * q] : 0.f, ok ? buf[4 * q + 1] : 0.f, ok ? buf[4 * q + 2] : 0.f, ok ? buf[4 * q + 3] : 0.f);
        }
    } else {
#pragma unroll
      for (int r = 0; r < NR; r++)
        if (r * EPI < ce2) {
          const int j = r * EPI + je;
          sT[j * LDT + ce] = (j < ccnt && ce < a.width) ? buf[r] : 0.f;
        }
    }
    if (lane < TS) {
      const bool in = lane < ccnt;
      sW[lane] = in ? xv - 1.f : 0.f;
      sC[lane] = in ? fmaf(xv - 1.f, ev, -xv) : 0.f;
    }
    wave_sync();
    if (c + 1 < nch) {
      idj = idn; xv = xn; ev = en;
      rows(idj, min(TS, q2 - base - TS));
      if (c + 2 < nch) meta(base + 2 * TS, idn, xn, en);
    }
    for (int s = 0; s < ce2 / 2; s++) {
      const int j = 2 * s + hf;
      const float wj = sW[j], cj = sC[j];
      float x[NT], aw[NT];
#pragma unroll
      for (int tb = 0; tb < NT; tb++) {
        x[tb] = sT[j * LDT + 32 * tb + n];
        aw[tb] = wj * x[tb];
        u[tb] = fmaf(cj, x[tb], u[tb]);
      }
#pragma unroll
      for (int ta = 0; ta < NT; ta++)
#pragma unroll
        for (int tb = 0; tb < NT; tb++) t[ta][tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[ta], x[tb], t[ta][tb], 0, 0, 0);
    }
  }
}

// the tiles and the entry sums -> delta_c in lane c (0 in the lanes >= width); w: the row's own w_u,pi in lane c.
// Returns true (wave-uniform) when a pivot was not positive: nothing may then be written.
template <int B>
__device__ __forceinline__ bool sub_solve(const SubArgs& a, const int row, f32x16 (&t)[B / 32][B / 32], float (&us)[B / 32], const int lane,
                                          float& w, float& z) {
  constexpr int NT = B / 32;
  int ln = lane;
  asm volatile("" : "+v"(ln));   // (as in als_chol_wave_kernel: keeps the lane-dependent compares out of registers)
  const bool lk = ln < a.width;
  float r[B];
  if constexpr (NT == 2) {
#pragma unroll
    for (int ta = 0; ta < 2; ta++)
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const auto sw2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(t[ta][0][v]), __float_as_uint(t[ta][1][v]), false, false);
        const int c = 32 * ta + 8 * (v >> 2) + (v & 3);
        r[c] = __uint_as_float(sw2[0]);
        r[c + 4] = __uint_as_float(sw2[1]);
      }
  } else {
#pragma unroll
    for (int v = 0; v < 16; v++) {
      const unsigned tv = __float_as_uint(t[0][0][v]);
      const auto sw2 = __builtin_amdgcn_permlane32_swap(tv, tv, false, false);
      const int c = 8 * (v >> 2) + (v & 3);
      r[c] = ln < 32 ? __uint_as_float(sw2[0]) : 0.f;   // (lanes 32..63 hold no row: zeros, they never reach a pivot)
      r[c + 4] = ln < 32 ? __uint_as_float(sw2[1]) : 0.f;
    }
  }
  float usum = half_sum(us[0]);
  if constexpr (NT == 2) {
    const float u1 = half_sum(us[1]);
    usum = ln < 32 ? usum : u1;
  }
  w = lk ? a.W[(size_t)row * a.ldw + a.c0 + ln] : 0.f;
  float u = lk ? (a.D[(size_t)row * a.ldd + ln] + a.lambda * w) + usum : 0.f;

  // LDL^T, lane i = row i (wrmf_chol_wave.hip has the remarks)
  bool bad = false;
  float dinv = 1.f;
  float pj = readlane_f(r[0], 0);
  static_for<B>([&](auto jt) {
    constexpr int j = decltype(jt)::value;
    bad = bad || !(pj > 0.f);
    const float i0 = __builtin_amdgcn_rcpf(pj);
    const float inv = fmaf(fmaf(-pj, i0, 1.f), i0, i0);
    const float uj = readlane_f(u, j);
    if (ln == j) dinv = inv;
    const float lij = ln > j ? r[j] * inv : 0.f;
    u = fmaf(-lij, uj, u);
    if constexpr (j + 1 < B) {
      r[j + 1] = fmaf(-lij, readlane_f(r[j], j + 1), r[j + 1]);
      pj = readlane_f(r[j + 1], j + 1);
      if constexpr (j + 2 < B) {
        float rep[4];
        dpp_ready(r[j]);
        rows_to_all<(B > 32 ? 4 : 2)>(r[j], rep);
        dpp_ready(rep[0], rep[1], rep[2], rep[3]);
        static_for<B - j - 2>([&](auto ct) {
          constexpr int c = j + 2 + decltype(ct)::value;
          fnma_row_bcast<c % 16>(r[c], rep[c / 16], lij);
        });
      }
    }
  });
  float acc = 0.f;
  z = 0.f;
#pragma unroll
  for (int c = B - 1; c >= 0; c--) {
    if (ln == c) z = (u - acc) * dinv;
    const float zc = readlane_f(z, c);
    acc = fmaf(ln < c ? r[c] : 0.f, zc, acc);
  }
  if (!lk) z = 0.f;
  return bad;
}

// h_j,pi . delta for the entry at CSR position pos, gathered again; sD: delta, zeros beyond the block
__device__ __forceinline__ float sub_dot_global(const SubArgs& a, const int pos, const bool vec, const float* sD) {
  const float* h = a.H + (size_t)a.J[pos] * a.ldh + a.c0;
  float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
  if (vec) {
    for (int m4 = 0; m4 < a.width / 4; m4++) {
      const float4 xv = *reinterpret_cast<const float4*>(h + 4 * m4);
      const float4 b = *reinterpret_cast<const float4*>(sD + 4 * m4);
      d0 = fmaf(xv.x, b.x, d0); d1 = fmaf(xv.y, b.y, d1); d2 = fmaf(xv.z, b.z, d2); d3 = fmaf(xv.w, b.w, d3);
    }
  } else {
    for (int m = 0; m < a.width; m++) d0 = fmaf(h[m], sD[m], d0);
  }
  return (d0 + d1) + (d2 + d3);
}

__device__ __forceinline__ void sub_count_failure(const SubArgs& a, const int lane) {
  if (lane == 0) atomicAdd(a.fails, 1);
}

// ---------------- rows of at most kSubLongLen entries: one wave per row ----------------
template <int B>
__global__ __launch_bounds__(64, 2) void subspace_wave_kernel(const SubArgs a) {
  constexpr int NT = B / 32, LDT = B + 4;
  __shared__ __attribute__((aligned(16))) float sT[kSubTile * LDT];
  __shared__ __attribute__((aligned(16))) float sD[64];
  __shared__ float sW[kSubTile], sC[kSubTile];
  const int lane = threadIdx.x & 63;
  const bool vec = sub_vec(a);
  // (a row per workgroup, not a loop over rows: hipcc hoists the lane-dependent addresses of the unrolled loops out of a row loop
  // and spills them)
  const int row = blockIdx.x;
  {
    const int p1 = rfl(a.P[row]), p2 = rfl(a.P[row + 1]), cnt = p2 - p1;
    if (cnt > kSubLongLen) return;   // subspace_long_kernel owns it
    f32x16 t[NT][NT];
    float u[NT], w, z;
    sub_seed<B>(a, true, t, u, lane);
    sub_assemble<B, kSubTile>(a, p1, p2, vec, sT, sW, sC, t, u, lane);
    if (sub_solve<B>(a, row, t, u, lane, w, z)) {
      sub_count_failure(a, lane);
      return;
    }
    if (lane < a.width) a.W[(size_t)row * a.ldw + a.c0 + lane] = w - z;
    wave_sync();
    sD[lane] = z;
    wave_sync();
    if (cnt <= kSubTile) {   // the row's slice is still in the tile
      if (lane < cnt) {
        float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
#pragma unroll
        for (int m4 = 0; m4 < B / 4; m4++) {
          const float4 xv = *reinterpret_cast<const float4*>(sT + lane * LDT + 4 * m4);
          const float4 b = *reinterpret_cast<const float4*>(sD + 4 * m4);
          d0 = fmaf(xv.x, b.x, d0); d1 = fmaf(xv.y, b.y, d1); d2 = fmaf(xv.z, b.z, d2); d3 = fmaf(xv.w, b.w, d3);
        }
        a.e[p1 + lane] -= (d0 + d1) + (d2 + d3);
      }
    } else {
      for (int pos = p1 + lane; pos < p2; pos += 64) a.e[pos] -= sub_dot_global(a, pos, vec, sD);
    }
  }
}

// ---------------- the long rows ----------------
// one thread per row: its segments, and for a row of several segments its slots of partials
__global__ void subspace_plan_kernel(const SubArgs a) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= a.n_rows) return;
  const int cnt = a.P[row + 1] - a.P[row];
  if (cnt <= kSubLongLen) return;
  const int nseg = (cnt + a.seg_len - 1) / a.seg_len;
  const int pos = atomicAdd(&a.counters[0], nseg);
  // (the capacities are bounds for a CSR of the stated nnz; a row beyond them -- the caller's nnz was wrong -- is dropped and counted)
  bool room = pos + nseg <= a.cap_seg;
  int m = -1, first = -1;
  if (room && nseg > 1) {
    m = atomicAdd(&a.counters[1], 1);
    first = atomicAdd(&a.counters[2], nseg);
    room = m < a.cap_multi && first + nseg <= a.cap_mseg;
  }
  if (!room) {
    atomicAdd(&a.counters[3], 1);
    atomicAdd(a.fails, 1);
    for (int s = 0; s < nseg && pos + s < a.cap_seg; s++) a.seg_row[pos + s] = -1;
    if (m >= 0 && m < a.cap_multi) a.multi_row[m] = -1;
    return;
  }
  for (int s = 0; s < nseg; s++) {
    a.seg_row[pos + s] = row;
    a.seg_idx[pos + s] = s;
    a.seg_pslot[pos + s] = nseg > 1 ? first + s : -1;
    a.seg_m[pos + s] = m;
  }
  if (m >= 0) {
    a.multi_row[m] = row;
    a.multi_first[m] = first;
    a.multi_nseg[m] = nseg;
  }
}

template <int B>
__device__ __forceinline__ void sub_to_regs(const float* src, f32x16 (&t)[B / 32][B / 32], float (&u)[B / 32], const int lane, const bool add) {
  constexpr int NT = B / 32;
#pragma unroll
  for (int ta = 0; ta < NT; ta++)
#pragma unroll
    for (int tb = 0; tb < NT; tb++)
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const float x = src[((ta * NT + tb) * 16 + v) * 64 + lane];
        t[ta][tb][v] = add ? t[ta][tb][v] + x : x;
      }
#pragma unroll
  for (int tb = 0; tb < NT; tb++) {
    const float x = src[(16 * NT * NT + tb) * 64 + lane];
    u[tb] = add ? u[tb] + x : x;
  }
}

// the entries [s1, s2) of a row: e -= h . delta, one entry per thread of the workgroup
__device__ __forceinline__ void sub_apply_span(const SubArgs& a, const int s1, const int s2, const bool vec, const float* sD) {
  for (int pos = s1 + (int)threadIdx.x; pos < s2; pos += 256) a.e[pos] -= sub_dot_global(a, pos, vec, sD);
}

template <int B>
__global__ __launch_bounds__(256) void subspace_long_kernel(const SubArgs a) {
  constexpr int NT = B / 32, LDT = B + 4, PART = SubGeo<B>::PART, NREG = SubGeo<B>::NREG;
  __shared__ __attribute__((aligned(16))) float sT[4][kSubLongTile * LDT];
  __shared__ __attribute__((aligned(16))) float sP[PART];
  __shared__ __attribute__((aligned(16))) float sD[64];
  __shared__ float sW[4][kSubLongTile], sC[4][kSubLongTile];
  __shared__ int sBad;
  const int seg = blockIdx.x;
  if (seg >= min(a.counters[0], a.cap_seg)) return;
  const int row = a.seg_row[seg];
  if (row < 0) return;
  const int si = a.seg_idx[seg], pslot = a.seg_pslot[seg];
  const int lane = threadIdx.x & 63, wv = rfl((int)threadIdx.x >> 6);
  const bool vec = sub_vec(a);
  const int p1 = a.P[row], p2 = a.P[row + 1];
  const int s1 = p1 + si * a.seg_len, s2 = min(p2, s1 + a.seg_len);
  // a quarter of the segment per wave, whole tiles
  const int per = ((s2 - s1 + 3) / 4 + kSubLongTile - 1) / kSubLongTile * kSubLongTile;
  const int q1 = rfl(min(s2, s1 + wv * per)), q2 = rfl(min(s2, q1 + per));
  f32x16 t[NT][NT];
  float u[NT];
  sub_seed<B>(a, si == 0 && wv == 0, t, u, lane);
  sub_assemble<B, kSubLongTile>(a, q1, q2, vec, sT[wv], sW[wv], sC[wv], t, u, lane);
  // ((w0 + w1) + w2) + w3, every lane on its own words
  for (int ww = 0; ww < 4; ww++) {
    if (wv == ww) {
#pragma unroll
      for (int ta = 0; ta < NT; ta++)
#pragma unroll
        for (int tb = 0; tb < NT; tb++)
#pragma unroll
          for (int v = 0; v < 16; v++) {
            float* d = sP + ((ta * NT + tb) * 16 + v) * 64 + lane;
            *d = ww ? *d + t[ta][tb][v] : t[ta][tb][v];
          }
#pragma unroll
      for (int tb = 0; tb < NT; tb++) {
        float* d = sP + (16 * NT * NT + tb) * 64 + lane;
        *d = ww ? *d + u[tb] : u[tb];
      }
    }
    __syncthreads();
  }
  if (pslot >= 0) {   // one of several segments: subspace_finish_kernel adds them
    float* dst = a.partials + (size_t)pslot * PART;
    for (int x = threadIdx.x; x < NREG * 64; x += 256) dst[x] = sP[x];
    return;
  }
  if (wv == 0) {
    float w, z;
    sub_to_regs<B>(sP, t, u, lane, false);
    const bool bad = sub_solve<B>(a, row, t, u, lane, w, z);
    if (bad) sub_count_failure(a, lane);
    else if (lane < a.width) a.W[(size_t)row * a.ldw + a.c0 + lane] = w - z;
    sD[lane] = z;
    if (lane == 0) sBad = bad;
  }
  __syncthreads();
  if (sBad) return;
  sub_apply_span(a, p1, p2, vec, sD);
}

// one wave per row of several segments: the partials in ascending order, one solve
template <int B>
__global__ __launch_bounds__(64) void subspace_finish_kernel(const SubArgs a) {
  constexpr int NT = B / 32, PART = SubGeo<B>::PART;
  const int m = blockIdx.x;
  if (m >= min(a.counters[1], a.cap_multi)) return;
  const int row = a.multi_row[m];
  if (row < 0) return;
  const int lane = threadIdx.x & 63;
  const int first = a.multi_first[m], nseg = a.multi_nseg[m];
  f32x16 t[NT][NT];
  float u[NT], w, z;
  sub_to_regs<B>(a.partials + (size_t)first * PART, t, u, lane, false);
  for (int s = 1; s < nseg; s++) sub_to_regs<B>(a.partials + (size_t)(first + s) * PART, t, u, lane, true);
  const bool bad = sub_solve<B>(a, row, t, u, lane, w, z);
  if (bad) sub_count_failure(a, lane);
  else if (lane < a.width) a.W[(size_t)row * a.ldw + a.c0 + lane] = w - z;
  a.delta[(size_t)m * 64 + lane] = bad ? 0.f : z;   // (a zero step leaves e as it is)
}

__global__ __launch_bounds__(256) void subspace_apply_kernel(const SubArgs a) {
  __shared__ __attribute__((aligned(16))) float sD[64];
  const int seg = blockIdx.x;
  if (seg >= min(a.counters[0], a.cap_seg)) return;
  const int row = a.seg_row[seg], m = row < 0 ? -1 : a.seg_m[seg];
  if (m < 0) return;
  if (threadIdx.x < 64) sD[threadIdx.x] = a.delta[(size_t)m * 64 + threadIdx.x];
  __syncthreads();
  const int p1 = a.P[row], p2 = a.P[row + 1];
  const int s1 = p1 + a.seg_idx[seg] * a.seg_len, s2 = min(p2, s1 + a.seg_len);
  sub_apply_span(a, s1, s2, sub_vec(a), sD);
}

// the long rows' capacities from nnz alone (no row can be seen from the host): see the header
struct SubCaps {
  int seg_len, cap_seg, cap_multi, cap_mseg;
};
SubCaps sub_caps(int n_rows, int64_t nnz) {
  SubCaps c;
  const int64_t sl = std::max<int64_t>(RSPARSE_HIP_SUBSPACE_SEGMENT, ((nnz + 2047) / 2048 + 63) / 64 * 64);
  c.seg_len = (int)sl;
  c.cap_multi = (int)(nnz / sl + 1);
  c.cap_mseg = (int)(2 * (nnz / sl) + 2);
  c.cap_seg = (int)(std::min<int64_t>(n_rows, nnz / (kSubLongLen + 1)) + nnz / sl + 2);
  return c;
}
size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace

size_t subspace_ws_bytes(int n_rows, int64_t nnz) {
  if (nnz <= kSubLongLen) return 16;
  const SubCaps c = sub_caps(n_rows, nnz);
  return align16(4 * sizeof(int)) + align16((size_t)4 * c.cap_seg * sizeof(int)) + align16((size_t)3 * c.cap_multi * sizeof(int)) +
         align16((size_t)64 * c.cap_multi * sizeof(float)) + (size_t)c.cap_mseg * SubGeo<64>::PART * sizeof(float);
}

hipError_t launch_subspace_block(const int32_t* P, const int32_t* J, const float* X, int n_rows, int64_t nnz, const float* H, int ldh,
                                 int c0, int width, const float* G, int ldg, const float* D, int ldd, float lambda, float* W, int ldw,
                                 float* e, int* fails, void* ws, hipStream_t s) {
  if (n_rows <= 0) return hipSuccess;
  SubArgs a{};
  a.P = P; a.J = J; a.X = X; a.n_rows = n_rows;
  a.H = H; a.ldh = ldh; a.c0 = c0; a.width = width;
  a.G = G; a.ldg = ldg; a.D = D; a.ldd = ldd; a.lambda = lambda;
  a.W = W; a.ldw = ldw; a.e = e; a.fails = fails;
  const bool wide = width > 32;   // (a block of at most 32 coordinates takes the one-tile kernels whatever b is)
  const bool longs = nnz > kSubLongLen;
  if (longs) {
    const SubCaps c = sub_caps(n_rows, nnz);
    a.seg_len = c.seg_len; a.cap_seg = c.cap_seg; a.cap_multi = c.cap_multi; a.cap_mseg = c.cap_mseg;
    char* p = static_cast<char*>(ws);
    a.counters = reinterpret_cast<int*>(p); p += align16(4 * sizeof(int));
    a.seg_row = reinterpret_cast<int*>(p);
    a.seg_idx = a.seg_row + c.cap_seg; a.seg_pslot = a.seg_idx + c.cap_seg; a.seg_m = a.seg_pslot + c.cap_seg;
    p += align16((size_t)4 * c.cap_seg * sizeof(int));
    a.multi_row = reinterpret_cast<int*>(p);
    a.multi_first = a.multi_row + c.cap_multi; a.multi_nseg = a.multi_first + c.cap_multi;
    p += align16((size_t)3 * c.cap_multi * sizeof(int));
    a.delta = reinterpret_cast<float*>(p); p += align16((size_t)64 * c.cap_multi * sizeof(float));
    a.partials = reinterpret_cast<float*>(p);
    hipError_t e0 = hipMemsetAsync(a.counters, 0, 4 * sizeof(int), s);
    if (e0 != hipSuccess) return e0;
    hipLaunchKernelGGL(subspace_plan_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, s, a);
  }
  const int grid = n_rows;
  if (wide) hipLaunchKernelGGL(subspace_wave_kernel<64>, dim3(grid), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(subspace_wave_kernel<32>, dim3(grid), dim3(64), 0, s, a);
  if (longs) {
    if (wide) {
      hipLaunchKernelGGL(subspace_long_kernel<64>, dim3(a.cap_seg), dim3(256), 0, s, a);
      hipLaunchKernelGGL(subspace_finish_kernel<64>, dim3(a.cap_multi), dim3(64), 0, s, a);
    } else {
      hipLaunchKernelGGL(subspace_long_kernel<32>, dim3(a.cap_seg), dim3(256), 0, s, a);
      hipLaunchKernelGGL(subspace_finish_kernel<32>, dim3(a.cap_multi), dim3(64), 0, s, a);
    }
    hipLaunchKernelGGL(subspace_apply_kernel, dim3(a.cap_seg), dim3(256), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace rsparse_hip
