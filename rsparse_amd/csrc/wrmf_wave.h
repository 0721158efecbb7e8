// Lane-level primitives shared by every kernel file (gfx950 / wave64 only): the vector types, the compile-time loop, the sums
// and copies across the lanes of a wave, the fp16 two-term split and the LDS-DMA wrappers.  One definition each -- a wrong DPP
// control, swap pairing or scale exponent does silent damage, so a fix or a remark made here reaches every kernel.
// A wave is four DPP rows ("groups") of 16 lanes; "needs full EXEC" = call it from converged code only.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

namespace rsparse_hip {
namespace dev {

typedef unsigned long long u64;
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), in order: a loop whose index is a constant expression
// (register names in inline asm, template arguments, if constexpr)
template <class F, int... I>
__device__ __forceinline__ void static_for_seq(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_seq(f, std::make_integer_sequence<int, N>{});
}

__device__ __forceinline__ void wave_sync() {
  // LDS traffic of one wave is executed in order; this only pins the compiler's ordering.
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float readlane_f(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ int rfl(int v) { return __builtin_amdgcn_readfirstlane(v); }

// the lane number, or (ON) a copy of it that the compiler has to take as a new value: what is computed from it is computed where
// it is used instead of living in a register across a loop (WIDEQ in als_cgq_kernel, QUAD in als_cgp_kernel)
template <bool ON>
__device__ __forceinline__ int opaque_lane(int l) {
  if constexpr (ON) asm volatile("" : "+v"(l));
  return l;
}

// ---- LDS-DMA ----
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(reinterpret_cast<uintptr_t>(p));  // low 32 bits of a generic LDS pointer = LDS byte address
}
// One dword (dma4) or one 16-byte piece (dma16) per lane: LDS destination = M0 + lane * 4 / lane * 16 (wave-uniform base),
// source = each lane's own pointer.  Counts in vmcnt like a load; the compiler does not know about it, which is harmless as
// long as nothing is issued between it and the explicit wait that precedes the first read of its destination (older
// operations complete first).  Issued from asm so that a loop's s_waitcnt can be COUNTED, wait_vm<N>: hipcc would otherwise
// drain the queue (vmcnt(0)) at every use and serialise gather and compute (wrmf_ne.hip's header).
__device__ __forceinline__ void dma4(const void* g, unsigned lds_base) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" : : "v"(g), "s"(lds_base) : "memory", "m0");
}
__device__ __forceinline__ void dma16(const void* g, unsigned lds_base) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(g), "s"(lds_base) : "memory", "m0");
}
// at most N vector-memory operations of this wave still in flight (vmcnt is a 6-bit field: N <= 63)
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- DPP ----
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// acc -= u(lane E of the row of 16 lanes this lane sits in) * l: v_fmac_f32 with a DPP row broadcast on its first operand.
// 4.8 cycles per wave against 8.4 + 4.3 for v_readlane + v_fma (tools/probes/valu_rate_probe.hip).  Needs EXEC = all ones.
template <int E>
__device__ __forceinline__ void fnma_row_bcast(float& acc, const float u, const float l) {
  asm("v_fmac_f32_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(u), "v"(l), "n"(E));
}
// A register that a DPP operand (or a lane swap) is about to read must not have been written by the one or two vector
// instructions before it (2 wait states).  hipcc inserts them between instructions it knows; it does not look inside inline
// asm, neither as the writer nor as the reader -- these tie an s_nop to the registers (the asm "rewrites" them, so the real
// writers stay in front of it and the readers behind).
__device__ __forceinline__ void dpp_ready(float& a) { asm("s_nop 1" : "+v"(a)); }
__device__ __forceinline__ void dpp_ready(float& a, float& b) { asm("s_nop 1" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ void dpp_ready(float& a, float& b, float& c, float& d) {
  asm("s_nop 1" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}

// ---- sums over the lanes ----
// sum / max over the 16 lanes of a DPP row; every lane of the row gets the result (needs full EXEC)
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp<0xB1>(v);   // quad_perm:[1,0,3,2]
  v += dpp<0x4E>(v);   // quad_perm:[2,3,0,1]
  v += dpp<0x141>(v);  // row_half_mirror
  v += dpp<0x140>(v);  // row_mirror
  return v;
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dpp<0xB1>(v));
  v = fmaxf(v, dpp<0x4E>(v));
  v = fmaxf(v, dpp<0x141>(v));
  v = fmaxf(v, dpp<0x140>(v));
  return v;
}
// v_permlane16_swap exchanges the odd rows of its first operand with the even rows of its second, v_permlane32_swap the upper
// half of the first with the lower half of the second; fed two copies of v they leave {v_even, v_even | ...} and
// {v_odd, v_odd | ...}, whose sum is the pairwise all-reduce -- pure VALU, no LDS round trip (ds_bpermute costs ~100+ cycles
// of latency per stage).
// v(l) + v(l ^ 16): the sum over the two groups of a half-wave, result in both, bitwise identical
__device__ __forceinline__ float pair_sum(float v) {
  const unsigned u = __float_as_uint(v);
  const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// v(l) + v(l ^ 32): the same across the two halves of the wave
__device__ __forceinline__ float half_sum(float v) {
  const unsigned u = __float_as_uint(v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// sum over the 4 groups (lanes l, l^16, l^32, l^48), result in all 4, bitwise identical everywhere: (0 + 1) + (2 + 3)
__device__ __forceinline__ float groups_sum(float v) { return half_sum(pair_sum(v)); }

// Sum over the 64 lanes, result uniform.  Needs EXEC = all ones.  Fixed order -> deterministic.  The four row sums are READ
// from lanes 0, 16, 32, 48 (scalar registers) and added as (s0 + s1) + (s2 + s3): the value, in every lane, that
// groups_sum(row16_sum(v)) leaves too, but uniform for the compiler; butterfly_sum adds in another order.
__device__ __forceinline__ float wave_sum(float v) {
  v = row16_sum(v);
  const float s0 = readlane_f(v, 0), s1 = readlane_f(v, 16);
  const float s2 = readlane_f(v, 32), s3 = readlane_f(v, 48);
  return (s0 + s1) + (s2 + s3);
}
// Butterfly over the wave with __shfl_xor (ds_bpermute), distances 32, 16, .., 1: every lane ends with the same bits
// (a + b == b + a), in an order fixed by the lane numbers -- NOT wave_sum's order.  float or double.
template <class T>
__device__ __forceinline__ T butterfly_sum(T v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// Sixteen per-lane partial sums -> lane L holds the wave's sum of v[(L >> 2) & 15] (the four lanes of a quad hold copies):
// every stage halves the number of values a lane carries by exchanging the half it does not keep with the lane across
// (15 exchanges for 16 sums where sixteen butterflies take 96).  v is destroyed.  The double overload (wrmf_f64.hip) makes the
// same exchanges with lane swaps and DPP moves and is kept next to the f64 DPP helpers it is built from.
__device__ __forceinline__ float transposed_sum16(float (&v)[16], const int lane) {
#pragma unroll
  for (int st = 0; st < 4; st++) {
    const int m = 32 >> st, n = 8 >> st;   // lane bit 5, 4, 3, 2 <-> value bit 3, 2, 1, 0
    const bool up = (lane & m) != 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      if (i < n) {
        const float keep = up ? v[i + n] : v[i];
        const float send = up ? v[i] : v[i + n];
        v[i] = keep + __shfl_xor(send, m);
      }
    }
  }
  float s = v[0];
  s += __shfl_xor(s, 2);
  s += __shfl_xor(s, 1);
  return s;
}

// ---- copies across the rows ----
// rep[g] = row g (lanes 16 g .. 16 g + 15) of v in every row of 16 lanes, g < NG (two or three lane-swap instructions)
template <int NG>
__device__ __forceinline__ void rows_to_all(const float v, float (&rep)[4]) {
  const unsigned u = __float_as_uint(v);
  const auto h = __builtin_amdgcn_permlane32_swap(u, u, false, false);   // h[0] = rows (0, 1, 0, 1), h[1] = rows (2, 3, 2, 3)
  const auto lo = __builtin_amdgcn_permlane16_swap(h[0], h[0], false, false);   // rows (0, 0, 0, 0), (1, 1, 1, 1)
  rep[0] = __uint_as_float(lo[0]);
  rep[1] = __uint_as_float(lo[1]);
  if constexpr (NG > 2) {
    const auto hi = __builtin_amdgcn_permlane16_swap(h[1], h[1], false, false);
    rep[2] = __uint_as_float(hi[0]);
    rep[3] = __uint_as_float(hi[1]);
  } else {
    rep[2] = rep[3] = 0.f;
  }
}
// The same inside GROUPS of SL lanes: lane t of a group is lane t % 16 of rep[t / 16] in every lane of the group (SL = 64: the
// wave; 32; 16: a row of 16 lanes)
template <int SL>
__device__ __forceinline__ void group_rows_to_all(const float v, float (&rep)[4]) {
  if constexpr (SL == 64) {
    rows_to_all<4>(v, rep);
  } else if constexpr (SL == 32) {
    const unsigned uu = __float_as_uint(v);
    const auto sw = __builtin_amdgcn_permlane16_swap(uu, uu, false, false);   // rows (0, 0, 2, 2) and (1, 1, 3, 3)
    rep[0] = __uint_as_float(sw[0]);
    rep[1] = __uint_as_float(sw[1]);
    rep[2] = rep[3] = 0.f;
  } else {
    rep[0] = v;
    rep[1] = rep[2] = rep[3] = 0.f;
  }
}

// ---- fp32 -> two fp16 terms for the matrix cores ----
// biased exponent e (1..253, so that the inverse is normal too) of the power of two that brings `vmax` into [2^13, 2^14);
// pow2(e) = 2^(e - 127) is the scale
__device__ __forceinline__ int fp16_scale_exp(float vmax) {
  const int eb = (int)((__float_as_uint(vmax) >> 23) & 0xffu);
  return min(253, max(1, 267 - eb));
}
__device__ __forceinline__ float pow2(int biased) { return __uint_as_float((unsigned)biased << 23); }
// x (already scaled into fp16's range) -> fl16(x), fl16(x - fl16(x)) for a pair; the residual is exact in fp32.  One PACKED
// subtraction: wrmf_mf.h keeps mf_split, the same with scalar subtractions, for the kernels that issue it behind matrix
// instructions; wrmf_ne.hip's split_stage / split_stage_h are another scheme (a chain of terms, bf16 or a mixed-precision FMA).
__device__ __forceinline__ void split_f16(const float x0, const float x1, unsigned& hi, unsigned& lo) {
  const f32x2 v = {x0, x1};
  const f16x2 h = __builtin_convertvector(v, f16x2);
  const f32x2 r = v - __builtin_convertvector(h, f32x2);
  const f16x2 l = __builtin_convertvector(r, f16x2);
  hi = __builtin_bit_cast(unsigned, h);
  lo = __builtin_bit_cast(unsigned, l);
}
// four dwords of packed halves -> one matrix-core operand
__device__ __forceinline__ f16x8 pack_f16x8(const unsigned a, const unsigned b, const unsigned c, const unsigned d) {
  const u32x4 v = {a, b, c, d};
  return __builtin_bit_cast(f16x8, v);
}

// ---- the packed lower triangle ----
__device__ __forceinline__ int tri(const int i) { return (i * (i + 1)) >> 1; }   // entries (tiles) before row i
// t-th tile of the lower triangle, row-major over the tile rows: (ti, tj), tj <= ti
__device__ __forceinline__ void tile_of(int t, int& ti, int& tj) {
  ti = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
  while ((ti + 1) * (ti + 2) / 2 <= t) ti++;
  while (ti * (ti + 1) / 2 > t) ti--;
  tj = t - ti * (ti + 1) / 2;
}

// ---- order-preserving keys ----
// key of a double: larger value <=> larger key (-0.0 just below +0.0; a caller for whom the zeros are equal passes v + 0.0),
// and its inverse
__device__ __forceinline__ u64 f64_key(double v) {
  const u64 b = (u64)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double key_f64(u64 k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

}  // namespace dev
}  // namespace rsparse_hip
