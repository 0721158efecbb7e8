// CG half-iteration for the SHORT rows (at most 16 or 32 non-zeros, and empty ones), two or four rows per wave (gfx950, wave64).
//
// Same arithmetic as als_cgq_kernel (wrmf_cgq.hip: cg_solver_implicit<T>, inst/include/wrmf_implicit.hpp:8-32, column loop
// :160-283; with a global bias cg_solver_implicit_global_bias, :35-57).  Half of the rows of the <= 32 bucket of the bench
// matrix have at most 16 non-zeros; in the one-wave kernel such a row fills 4 of the wave's 8 quads and still pays the
// whole fixed cost of a CG sweep (the shared dense product and its two barriers, the 16-lane and cross-group reductions,
// the scalar chain of alpha and beta): the kernel is bound by VALU issue, not by HBM (profiles/README.md).  Here a wave
// solves TWO rows side by side: lanes 0..31 one row, lanes 32..63 the other, every instruction serves both.
//
// Layout: a rank-128 vector is spread over the 16 lanes of a DPP row exactly as in wrmf_cgq.hip (8 floats per lane: floats
// [4i, 4i+4) and [64+4i, 64+4i+4) for lane i); a half-wave is two such groups, which hold two DIFFERENT non-zeros of the
// half's row at a time: slot s = 2 q + (group & 1), q = 0..7 -> 16 non-zeros in 64 registers per lane.  CG state is
// replicated in the two groups of a half and differs between the halves; all per-row scalars (row id, pointers, alpha,
// beta, convergence) are per-lane values that are uniform inside a half.  The dense product G v is shared by the
// workgroup's EIGHT rows on the matrix cores (G as two fp16 terms in registers, the vectors published as two fp16 terms
// through LDS, three products of order < 2: the DMF scheme of wrmf_cgq.hip with 8 instead of 4 live columns of the
// 16-column tile).  Slots beyond a row's length read the all-zero row and carry c = 0.
//
// NQ = 16 (rows of 17..32 non-zeros, rank 128, no global bias): slot s = 2 q + (group & 1), q = 0..15 -> 32 non-zeros in 128
// registers per lane.  G's fp16 terms then do not fit beside them and sit in LDS in fragment order (the DMF = 2 layout of
// wrmf_cgq.hip: [wave][tile][k-step][term] x 1 KB, lane l's 16 bytes at l * 16, conflict-free), and the next pair's indices /
// confidences are not prefetched into registers but copied by LDS-DMA into one of two LDS slots of the wave (one
// global_load_lds_dword each for the 64 entries of the two rows), from which the row switch reads the indices and the sweeps
// the confidences.
//
// QUAD (rows of at most 16 non-zeros, rank 128, no global bias; NQ = 16): FOUR rows per wave, one 16-lane group per row.  Slot q
// (q = 0..15) of the group holds non-zero q of its row, 128 registers of vectors as above; CG state, row id, pointers, alpha,
// beta and the convergence flag are per-lane values that are uniform inside a GROUP.  There is no cross-group sum (pair_sum
// and its lane swaps are not instantiated), t_acc / t_cur take 16 slots per group, and a block of four quads is skipped when
// none of the wave's four rows reaches it.  The workgroup's SIXTEEN rows are the 16 columns of the matrix-core tile -- the same
// 24 instructions per wave and sweep serve twice the rows; each group publishes both pieces of its vector and folds its own
// column.  G in LDS and the indices / confidences of the next four rows by LDS-DMA as with NQ = 16 (lane l copies entry l & 15
// of its group's row).  LDS is what decides the layout: two workgroups per CU leave 81 920 B each, G's fragments (64 KB), the
// index slots (4 KB) and t_acc / t_cur (2 KB) leave 10 224 B, and sixteen published columns (8704 B) beside sixteen columns of
// products (8448 B) do not fit.  So column c's products lie OVER column c's two published terms: every wave reads all its B
// operands right after the barrier that follows the publish, a second barrier directly behind it (the waves are still aligned)
// frees the bytes for the products, and the next sweep's publish overwrites only what the same lanes folded (PairSmem<16, true>:
// 80 400 B).  The addresses of a sweep are formed from an opaque copy of the lane number: kept across the row loop they cost a
// dozen registers and 8 spilled ones (245 registers, no spill, no scratch; rsparse_amd/build.py NO_SPILL).
#include "wrmf_internal.h"
#include "wrmf_device.h"

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kPairMaxSweeps = 4;

template <int NQ, bool QUAD = false>
struct PairSmem {
  static constexpr int KP = 128, ps = KP + 8, os = QUAD ? KP + 8 : KP + 4;
  static constexpr int cols = QUAD ? 16 : 8;        // live columns of the 16-column tile = rows of the workgroup
  static constexpr int pcs = QUAD ? 2 * ps : ps;    // halfs from one published column to the next
  static constexpr size_t gfrag = NQ == 16 ? (size_t)4 * 16 * 1024 : 0;   // G's fp16 fragments (NQ = 16)
  static constexpr size_t nxt = NQ == 16 ? (size_t)4 * 2 * 2 * 64 * 4 : 0;   // NQ = 16: [wave][slot][index, value][64]
  static constexpr size_t pub = (size_t)2 * cols * ps * 2, out = (size_t)cols * os * 4;
  // QUAD: column c's products (os floats) lie over column c's two published terms (2 ps halfs): see the kernel's sweep
  static_assert(!QUAD || (pub == out && (size_t)pcs * 2 == (size_t)os * 4), "QUAD: one column, one stretch of LDS");
  static constexpr size_t bytes = gfrag + (QUAD ? pub : pub + out) + (size_t)4 * 8 * NQ * 4 + nxt + 16;
};
// two workgroups per CU (what hides the gather) leave 80 KB each
static_assert(PairSmem<16>::bytes <= 81920 && PairSmem<16, true>::bytes <= 81920, "two workgroups per CU");

// KFULL (rank 128): unconditional vector loads and the warm start requested before them -- the first sweep's publish / dense
// product run while the vectors are in flight and its quad pass takes them as they arrive (als_cgq_kernel's KFULL)
template <bool GB, bool KFULL = false, int NQ = 8, bool QUAD = false>
__global__ __launch_bounds__(256, 2) void als_cgp_kernel(AlsArgs a, const int32_t* __restrict__ rows, int n_rows, int iters,
                                                        size_t loss_slot0) {
  constexpr int KP = 128, RPN = 8, VW = 4, NV = 2;
  static_assert(NQ == 8 || (NQ == 16 && KFULL && !GB), "the 32-slot kernel: rank 128, no global bias");
  static_assert(!QUAD || NQ == 16, "four rows per wave: 16 slots per group, G in LDS");
  constexpr bool GREG = NQ == 8;   // G's fp16 terms and the prefetched indices in registers (else in LDS)
  constexpr int RW = QUAD ? 4 : 2, GL = 64 / RW;   // rows per wave, lanes per row
  constexpr int SS = QUAD ? 1 : 2;                 // a group's slots are gs + SS q
  using SM = PairSmem<NQ, QUAD>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sGf = smem + (size_t)(threadIdx.x >> 6) * 16 * 1024;     // NQ = 16: this wave's G fragments, [tile][step][term] x 1 KB
  // QUAD: [16][2][KP + 8], a column's two terms side by side, and the column's G v in the SAME bytes once the terms are read
  _Float16* sPh = reinterpret_cast<_Float16*>(smem + SM::gfrag); // [8][KP + 8] leading fp16 terms of the published vectors
  _Float16* sPl = QUAD ? sPh + SM::ps : sPh + 8 * SM::ps;       // [8][KP + 8] second terms
  float* sOut = QUAD ? reinterpret_cast<float*>(sPh) : reinterpret_cast<float*>(sPl + 8 * SM::ps);   // [8][KP + 4] G v (times the scales)
  float* sTsv = QUAD ? reinterpret_cast<float*>(sPh + 16 * SM::pcs) : sOut + 8 * SM::os;   // [4][2][2 NQ]  x_j . y accumulated / of the current step
  float* sNx = sTsv + 4 * 8 * NQ + (threadIdx.x >> 6) * 256;     // NQ = 16: this wave's [2][index, value][64]
  const int tid = threadIdx.x, lane = tid & 63, wv = rfl(tid >> 6);
  const int g = lane >> 4, i = lane & 15, H = lane >> 5, g2 = g & 1;
  const int R = QUAD ? g : H;     // this lane's row of the wave's RW
  const int gs = QUAD ? 0 : g2;   // this group's first slot
  const int k = KFULL ? KP : a.k;
  const float gbias = GB ? a.gbias : 0.f, ltgt = GB ? a.loss_tgt_const : 1.f;
  for (int e = tid; e < 4 * 8 * NQ; e += 256) sTsv[e] = 0.f;
  // this wave's 32 rows of G as A operands of v_mfma_f32_16x16x32_f16 (tile t = rows 32 wv + 16 t + (lane & 15), step ks =
  // columns 32 ks + 8 (lane >> 4) + 0..7), two fp16 terms of G * 2^ge; ginv = 2^-ge
  f16x8 gAh[GREG ? 2 : 1][GREG ? 4 : 1], gAl[GREG ? 2 : 1][GREG ? 4 : 1];
  float ginv;
  {
    const int m = lane & 15, kb = lane >> 4;
    float gmax = 0.f;
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
      for (int ks = 0; ks < 4; ks++)
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const int r = 32 * wv + 16 * t + m, c = 32 * ks + 8 * kb + e;
          {   // (clamped address, select afterwards: a per-lane `cond ? load : 0` is a branch with a wait per element)
            // (... and a MULTIPLY by the 0 / 1 mask, not a select: hipcc sinks a load whose value only one side of a select uses
            //  back under the condition)
            const float gv = a.XtX[(size_t)min(r, k - 1) * k + min(c, k - 1)];
            gmax = fmaxf(gmax, fabsf(gv) * ((r < k && c < k) ? 1.f : 0.f));
          }
        }
    for (int o = 32; o > 0; o >>= 1) gmax = fmaxf(gmax, __shfl_xor(gmax, o));
    const int ge = fp16_scale_exp(gmax);
    const float gs = __uint_as_float((unsigned)ge << 23);
    ginv = __uint_as_float((unsigned)(254 - ge) << 23);
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        unsigned hi[4], lo[4];
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
          const int r = 32 * wv + 16 * t + m, c = 32 * ks + 8 * kb + e;
          const float g0v = a.XtX[(size_t)min(r, k - 1) * k + min(c, k - 1)];
          const float g0 = g0v * ((r < k && c < k) ? 1.f : 0.f);
          const float g1v = a.XtX[(size_t)min(r, k - 1) * k + min(c + 1, k - 1)];
          const float g1 = g1v * ((r < k && c + 1 < k) ? 1.f : 0.f);
          split_f16(g0 * gs, g1 * gs, hi[e / 2], lo[e / 2]);
        }
        const uint4 h4 = {hi[0], hi[1], hi[2], hi[3]}, l4 = {lo[0], lo[1], lo[2], lo[3]};
        if constexpr (GREG) {
          gAh[t][ks] = __builtin_bit_cast(f16x8, h4);
          gAl[t][ks] = __builtin_bit_cast(f16x8, l4);
        } else {
          *reinterpret_cast<uint4*>(sGf + ((t * 4 + ks) * 2 + 0) * 1024 + lane * 16) = h4;
          *reinterpret_cast<uint4*>(sGf + ((t * 4 + ks) * 2 + 1) * 1024 + lane * 16) = l4;
        }
      }
  }
  __syncthreads();
  float* tacc = sTsv + wv * 8 * NQ + (QUAD ? NQ * g : 2 * NQ * H);   // this half's 2 NQ (QUAD: this group's NQ) slots: x_j . y accumulated over the CG steps
  float* tcur = tacc + 4 * NQ;                     // ... x_j . p of the current step
  // the slot whose x_j . y this lane holds for the loss: group 0 slots 0..15, with NQ = 16 group 1 slots 16..31
  const int lslot = (NQ == 16 && !QUAD) ? i + 16 * g2 : i;
  const bool lgrp = NQ == 16 || g2 == 0;
  const int col = RW * wv + R;             // this row's column of the shared dense product
  double wloss = 0.0;
  const int wave_global = blockIdx.x * 4 + wv, total_waves = gridDim.x * 4;
  auto ridx = [&](const int itn) { return (wave_global + itn * total_waves) * RW + R; };   // position in `rows`, per half (QUAD: per group)
  // row ids run two iterations ahead, pointers one ahead (per-lane values, uniform inside a half)
  int row_c = 0, p1_c = 0, p2_c = 0, row_n = 0;
  if (iters > 0 && ridx(0) < n_rows) {
    row_c = rows[ridx(0)];
    p1_c = a.col_ptrs[row_c];
    p2_c = a.col_ptrs[row_c + 1];
  }
  if (iters > 1 && ridx(1) < n_rows) row_n = rows[ridx(1)];

  // KFULL: the indices / values of a pair of rows are requested during the PREVIOUS pair's sweeps (the first pair's here): the
  // gather at the row switch is then one HBM round trip -- the vectors -- instead of two (what the one- and two-wave kernels of
  // wrmf_cgq.hip have done since round 2; this kernel sits at 238 registers: 17 more).  All NQ
  // slots of a lane are requested whatever the rows' lengths (a slot outside its row reads entry 0 and is dropped).
  int idn[GREG ? NQ : 1];
  float cvn[GREG ? NQ : 1], cln = 0.f;
#pragma unroll
  for (int q = 0; q < (GREG ? NQ : 1); q++) {
    idn[q] = 0;
    cvn[q] = 0.f;
  }
  // NQ = 16: lane l copies entry l & 31 of its half's row (QUAD: l & 15 of its group's) into slot `buf` (entries beyond the row:
  // index 0, confidence 0)
  auto request_indices = [&](const bool valid, const int np1, const int ncnt, const int buf) {
    if constexpr (!GREG) {
      const int e = lane & (GL - 1);
      const bool in = valid && e < ncnt;
      float* slot = sNx + buf * 128;
      dma4(in ? static_cast<const void*>(a.row_idx + np1 + e) : static_cast<const void*>(a.zero_row), (unsigned)rfl((int)lds_addr(slot)));
      dma4(in ? static_cast<const void*>(a.vals + np1 + e) : static_cast<const void*>(a.zero_row), (unsigned)rfl((int)lds_addr(slot + 64)));
      return;
    }
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const int s = 2 * q + g2;
      const int j = (valid && s < ncnt) ? np1 + s : 0;
      idn[q] = a.row_idx[j];
      cvn[q] = a.vals[j];
    }
    cln = a.vals[(valid && lslot < ncnt) ? np1 + lslot : 0];
  };
  auto settle_indices = [&]() {   // a use the compiler cannot move: the wait for the request sits HERE
    if constexpr (!GREG) {
      wait_vm<0>();
      return;
    }
#pragma unroll
    for (int q = 0; q < NQ; q += 8) {
      asm volatile("" : "+v"(idn[q]), "+v"(idn[q + 1]), "+v"(idn[q + 2]), "+v"(idn[q + 3]), "+v"(idn[q + 4]), "+v"(idn[q + 5]), "+v"(idn[q + 6]), "+v"(idn[q + 7]));
      asm volatile("" : "+v"(cvn[q]), "+v"(cvn[q + 1]), "+v"(cvn[q + 2]), "+v"(cvn[q + 3]), "+v"(cvn[q + 4]), "+v"(cvn[q + 5]), "+v"(cvn[q + 6]), "+v"(cvn[q + 7]));
    }
    asm volatile("" : "+v"(cln));
  };
  if constexpr (KFULL) {
    request_indices(iters > 0 && ridx(0) < n_rows, p1_c, p2_c - p1_c, 0);
    settle_indices();   // (once per wave: the first pair pays the round trip)
  }

  for (int it = 0; it < iters; ++it) {
    const bool have = ridx(it) < n_rows;
    const int row = have ? row_c : 0, p1 = have ? p1_c : 0, p2 = have ? p2_c : 0;
    {
      int p1_n = 0, p2_n = 0, row_nn = 0;
      if (it + 1 < iters && ridx(it + 1) < n_rows) {
        p1_n = a.col_ptrs[row_n];
        p2_n = a.col_ptrs[row_n + 1];
      }
      if (it + 2 < iters && ridx(it + 2) < n_rows) row_nn = rows[ridx(it + 2)];
      row_c = row_n;
      p1_c = p1_n;
      p2_c = p2_n;
      row_n = row_nn;
    }
    const int cnt = p2 - p1;   // 0..2 NQ (launcher)
    float* yrow = a.Y + (size_t)row * k;
    const bool live = have && (GB || cnt > 0);
    if (have && !live) {  // empty column -> zeros (wrmf_implicit.hpp:281); the 32 lanes of the half write it
      if constexpr (QUAD) {   // (the group's 16 lanes, as they store a solution)
#pragma unroll
        for (int b = 0; b < NV; b++) *reinterpret_cast<float4*>(yrow + b * 16 * VW + i * VW) = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        for (int e = lane & 31; e < k; e += 32) yrow[e] = 0.f;
      }
    }
    // the longer of the wave's two rows (wave-uniform): block b of four quads (slots 8 b .. 8 b + 7) is touched only when it
    // reaches the block; the first block always is
    // (QUAD: the longest of the four; block b is slots 4 b .. 4 b + 3 of every group)
    int wcnt = max(__builtin_amdgcn_readlane(cnt, 0), __builtin_amdgcn_readlane(cnt, 32));
    if constexpr (QUAD) wcnt = max(wcnt, max(__builtin_amdgcn_readlane(cnt, 16), __builtin_amdgcn_readlane(cnt, 48)));
    auto blk_on = [&](const int q) { return q < 4 || wcnt > SS * (q & ~3); };

    float x[RPN], r[RPN], p[RPN], ap[RPN];
    auto load_warm_start = [&]() {
#pragma unroll
      for (int b = 0; b < NV; b++) {
        const int off = b * 16 * VW + i * VW;
        float4 pc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (have && off < k) pc = *reinterpret_cast<const float4*>(yrow + off);  // warm start
        const float* pf = reinterpret_cast<const float*>(&pc);
#pragma unroll
        for (int c = 0; c < VW; c++) x[b * VW + c] = pf[c];
      }
    };
    if constexpr (KFULL) load_warm_start();
    // ---- gather: all index loads, then all vector loads; slots beyond the row read the zero row and carry c = 0 ----
    float xt[NQ][RPN], cv[GREG ? NQ : 1];
    const float* nx = sNx + (it & 1) * 128 + (QUAD ? 16 * g : 32 * H);   // NQ = 16: this row's indices (nx[s]) / confidences (nx[64 + s])
    {
      // (the loads WITHOUT a per-lane predicate: `in ? load : 0` compiles to a branch per slot with the address arithmetic of
      //  the vector load -- and its wait for the index -- inside: up to eight index round trips one after the other per pair of
      //  rows, found in the listing in round 5.  A slot outside its row reads entry 0 of the matrix and drops the result.)
      int id[NQ];
#pragma unroll
      for (int q = 0; q < NQ; q++) {
        if constexpr (!GREG) {
          id[q] = __float_as_int(QUAD ? nx[q] : nx[2 * q + g2]);
        } else if constexpr (KFULL) {
          id[q] = idn[q];
          cv[q] = cvn[q];
        } else {
          const int s = 2 * q + g2;
          const int j = s < cnt ? p1 + s : 0;
          id[q] = 0;
          cv[q] = 0.f;
          if (blk_on(q)) {   // wave-uniform
            id[q] = a.row_idx[j];
            cv[q] = a.vals[j];
          }
        }
      }
#pragma unroll
      for (int q = 0; q < NQ; q++) {
        const bool in = SS * q + gs < cnt;
        id[q] = in ? id[q] : 0;
        if constexpr (GREG) cv[q] = in ? cv[q] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < NQ; q++) {
        const bool in = SS * q + gs < cnt;
        const float* src = in ? a.X + (size_t)id[q] * k : a.zero_row;
#pragma unroll
        for (int b = 0; b < NV; b++) {
          const int off = b * 16 * VW + i * VW;
          if constexpr (KFULL) {
            // the first block without a branch; the second only when one of the wave's two rows reaches it (half of the rows of
            // this launch have at most 8 non-zeros: gathering the zero row for them cost 0.4 ms of the launch's 5.7)
            float4 pc = make_float4(0.f, 0.f, 0.f, 0.f);
            if (blk_on(q)) pc = *reinterpret_cast<const float4*>(src + off);
            const float* pf = reinterpret_cast<const float*>(&pc);
#pragma unroll
            for (int c = 0; c < VW; c++) xt[q][b * VW + c] = pf[c];
          } else {
            float4 pc = make_float4(0.f, 0.f, 0.f, 0.f);
            if (blk_on(q)) pc = *reinterpret_cast<const float4*>(src + min(off, k - VW));
            const float* pf = reinterpret_cast<const float*>(&pc);
#pragma unroll
            for (int c = 0; c < VW; c++) xt[q][b * VW + c] = off < k ? pf[c] : 0.f;
          }
        }
      }
    }
    // confidence of non-zero lslot of the half's row (loss)
    float cl;
    if constexpr (!GREG) cl = nx[64 + lslot];   // (0 beyond the row)
    else if constexpr (KFULL) cl = (lgrp && lslot < cnt) ? cln : 0.f;
    else cl = (lgrp && lslot < cnt) ? a.vals[p1 + lslot] : 0.f;

    if constexpr (!KFULL) load_warm_start();

    // mode 0: out = X_nnz (c - c1 % (X_nnz^T v + g)) - G v (+ base); mode 1: out = X_nnz (c1 % X_nnz^T v) + G v; mode 2: loss;
    // mode 3: loss_out = v . (mode 1's out) = v . G v + sum_j (c_j - 1) t_j^2 from the dots alone -- t is recorded as in mode 1, no
    // vector is formed (the last CG step: als_cgq_kernel's mode 3)
    auto sweep = [&](const float(&v)[RPN], const int mode, float(&out)[RPN], float& loss_out) {
      float acc[RPN];
#pragma unroll
      for (int rr = 0; rr < RPN; rr++) acc[rr] = 0.f;
      float vinv = 0.f;
      // QUAD: the sweep's per-lane LDS addresses are formed here from an opaque copy of the lane number -- left to the compiler
      // they are formed once per launch and sit in a dozen registers across the row loop, which the kernel does not have
      const int ln = opaque_lane<QUAD>(lane), li = ln & 15, lg = ln >> 4;
      const int lcol = QUAD ? RW * wv + lg : col;
      if (mode != 2) {
        // (1) publish v as two fp16 terms of v * 2^ve: group g2 publishes piece g2 (elements [64 g2 + 4 i, + 4))
        float vmax = 0.f;
#pragma unroll
        for (int rr = 0; rr < RPN; rr++) vmax = fmaxf(vmax, fabsf(v[rr]));
        vmax = row16_max(vmax);
        const int ve = fp16_scale_exp(vmax);
        const float vs = __uint_as_float((unsigned)ve << 23);
        vinv = __uint_as_float((unsigned)(254 - ve) << 23) * (mode == 0 ? -1.f : 1.f);
        if constexpr (QUAD) {
          // the group publishes both pieces of its row's vector.  The column's bytes held its G v until this group folded it
          // (below): same lanes, LDS in order -- the fence only keeps the compiler from moving the stores up
          wave_sync();
#pragma unroll
          for (int b = 0; b < NV; b++) {
            unsigned h0, l0, h1, l1;
            split_f16(v[b * VW] * vs, v[b * VW + 1] * vs, h0, l0);
            split_f16(v[b * VW + 2] * vs, v[b * VW + 3] * vs, h1, l1);
            const int off = lcol * SM::pcs + b * 16 * VW + li * VW;
            *reinterpret_cast<uint2*>(sPh + off) = make_uint2(h0, h1);
            *reinterpret_cast<uint2*>(sPl + off) = make_uint2(l0, l1);
          }
        } else {
          float w4[VW];
#pragma unroll
          for (int c = 0; c < VW; c++) w4[c] = (g2 == 0 ? v[c] : v[VW + c]) * vs;
          unsigned h0, l0, h1, l1;
          split_f16(w4[0], w4[1], h0, l0);
          split_f16(w4[2], w4[3], h1, l1);
          const int off = col * SM::ps + g2 * 16 * VW + i * VW;
          *reinterpret_cast<uint2*>(sPh + off) = make_uint2(h0, h1);
          *reinterpret_cast<uint2*>(sPl + off) = make_uint2(l0, l1);
        }
        __syncthreads();
        // (2) this wave's 32 rows of G against the eight vectors (columns 8..15 of the tile repeat them; QUAD: against sixteen)
        f32x4 d0[2], d1[2];
#pragma unroll
        for (int t = 0; t < 2; t++) d0[t] = d1[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int nb = QUAD ? li * SM::pcs + 8 * lg : (lane & 7) * SM::ps + 8 * (lane >> 4);
        // QUAD: every wave takes all its B operands first (the waves are still aligned from the barrier above); behind the second
        // barrier the columns' bytes take the products
        f16x8 bhs[QUAD ? 4 : 1], bls[QUAD ? 4 : 1];
        if constexpr (QUAD) {
#pragma unroll
          for (int ks = 0; ks < 4; ks++) {
            bhs[ks] = *reinterpret_cast<const f16x8*>(sPh + nb + 32 * ks);
            bls[ks] = *reinterpret_cast<const f16x8*>(sPl + nb + 32 * ks);
          }
          __syncthreads();
        }
#pragma unroll
        for (int ks = 0; ks < 4; ks++) {
          f16x8 bh, bl;
          if constexpr (QUAD) {
            bh = bhs[ks];
            bl = bls[ks];
          } else {
            bh = *reinterpret_cast<const f16x8*>(sPh + nb + 32 * ks);
            bl = *reinterpret_cast<const f16x8*>(sPl + nb + 32 * ks);
          }
#pragma unroll
          for (int t = 0; t < 2; t++) {
            f16x8 ah, al;
            if constexpr (GREG) {
              ah = gAh[t][ks];
              al = gAl[t][ks];
            } else {
              ah = *reinterpret_cast<const f16x8*>(sGf + ((t * 4 + ks) * 2 + 0) * 1024 + (QUAD ? ln : lane) * 16);
              al = *reinterpret_cast<const f16x8*>(sGf + ((t * 4 + ks) * 2 + 1) * 1024 + (QUAD ? ln : lane) * 16);
            }
            d0[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, d0[t], 0, 0, 0);
            d1[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, d1[t], 0, 0, 0);
            d1[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, d1[t], 0, 0, 0);
          }
        }
        if (QUAD || (lane & 15) < 8) {   // D: column = lane & 15, rows 4 (lane >> 4) + 0..3 of the tile
#pragma unroll
          for (int t = 0; t < 2; t++) {
            const f32x4 d = (d0[t] + d1[t]) * ginv;
            float* po = QUAD ? sOut + li * SM::os + 32 * wv + 16 * t + 4 * lg : sOut + (lane & 15) * SM::os + 32 * wv + 16 * t + 4 * (lane >> 4);
            *reinterpret_cast<f32x4*>(po) = d;
          }
        }
      }
      float lacc = 0.f;
      if (mode != 2) {
        float* trec = (mode == 0 ? tacc : tcur) + gs;   // slot 2 q + g2 (QUAD: q) <- t (the 16 lanes of the group write the same value)
#pragma unroll
        for (int q0 = 0; q0 < NQ; q0 += 4) {
          if (blk_on(q0)) {   // wave-uniform
            // (the four quads' dot chains and DPP reductions interleaved: see quad_pass in wrmf_cgq.hip)
            float t[4];
            f32x2 s2[4];
#pragma unroll
            for (int u = 0; u < 4; u++) s2[u] = f32x2{0.f, 0.f};
#pragma unroll
            for (int rr = 0; rr < RPN; rr += 2) {
              const f32x2 va = {v[rr], v[rr + 1]};
#pragma unroll
              for (int u = 0; u < 4; u++) {
                const f32x2 xa = {xt[q0 + u][rr], xt[q0 + u][rr + 1]};
                s2[u] = __builtin_elementwise_fma(xa, va, s2[u]);
              }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) t[u] = s2[u].x + s2[u].y;
#pragma unroll
            for (int u = 0; u < 4; u++) t[u] += dpp<0xB1>(t[u]);
#pragma unroll
            for (int u = 0; u < 4; u++) t[u] += dpp<0x4E>(t[u]);
#pragma unroll
            for (int u = 0; u < 4; u++) t[u] += dpp<0x141>(t[u]);
#pragma unroll
            for (int u = 0; u < 4; u++) t[u] += dpp<0x140>(t[u]);
#pragma unroll
            for (int u = 0; u < 4; u++) {
              const int q = q0 + u;
              const float c = GREG ? cv[q] : (QUAD ? nx[64 + q] : nx[64 + 2 * q + g2]);
              trec[SS * q] = t[u];
              const float w = mode == 0 ? c - (c - 1.f) * (GB ? t[u] + gbias : t[u]) : (c - 1.f) * t[u];
              if (mode == 3) {   // (t is uniform in the group: counted once per group; a slot beyond the row has c = 0, t = 0)
                lacc = fmaf(w, t[u], lacc);
                continue;
              }
#pragma unroll
              for (int rr = 0; rr < RPN; rr++) acc[rr] = fmaf(w, xt[q][rr], acc[rr]);
            }
          }
        }
      } else {
        // loss from t_acc = X_nnz^T y built up by the sweeps (the vectors are not touched again)
        wave_sync();
        const float t = tacc[lslot];
        const float dd = ltgt - t;
        const float ls = row16_sum((lgrp && lslot < cnt) ? cl * dd * dd : 0.f);
        lacc = QUAD ? ls : pair_sum(ls);
      }
      if (mode != 2) {
        // (3) the products are complete: fold this row's G v into group 0's partial sums, then reduce the two groups
        // (QUAD: into the group's own sums, and there is nothing to reduce)
        __syncthreads();
        const float f = (QUAD || g2 == 0) ? vinv : 0.f;
        if (mode == 3) {
          // v . G v in place: this lane's eight products, the group's 16 lanes, group 0's share beside the quads' sum
          float dl = 0.f;
#pragma unroll
          for (int b = 0; b < NV; b++) {
            const float* po = QUAD ? sOut + lcol * SM::os + b * 16 * VW + li * VW : sOut + col * SM::os + b * 16 * VW + i * VW;
            const f32x4 o = *reinterpret_cast<const f32x4*>(po);
#pragma unroll
            for (int c = 0; c < VW; c++) dl = fmaf(o[c], v[b * VW + c], dl);
          }
          lacc = fmaf(f, row16_sum(dl), lacc);
          loss_out = QUAD ? lacc : pair_sum(lacc);
          return;
        }
#pragma unroll
        for (int b = 0; b < NV; b++) {
          const float* po = QUAD ? sOut + lcol * SM::os + b * 16 * VW + li * VW : sOut + col * SM::os + b * 16 * VW + i * VW;
          const f32x4 o = *reinterpret_cast<const f32x4*>(po);
#pragma unroll
          for (int c = 0; c < VW; c++) acc[b * VW + c] = fmaf(f, o[c], acc[b * VW + c]);
        }
#pragma unroll
        for (int rr = 0; rr < RPN; rr++) out[rr] = QUAD ? acc[rr] : pair_sum(acc[rr]);
        if constexpr (GB) {
          if (mode == 0) {
#pragma unroll
            for (int b = 0; b < NV; b++) {
              const int off = b * 16 * VW + i * VW;
              const float4 pc = *reinterpret_cast<const float4*>(a.rhs_init + min(off, k - VW));
              const float* pf = reinterpret_cast<const float*>(&pc);
#pragma unroll
              for (int c = 0; c < VW; c++) out[b * VW + c] += off < k ? pf[c] : 0.f;
            }
          }
        }
      } else {
        loss_out = lacc;
      }
    };
    auto dot16 = [&](const float(&u)[RPN], const float(&w)[RPN]) {
      float s = 0.f;
#pragma unroll
      for (int rr = 0; rr < RPN; rr++) s = fmaf(u[rr], w[rr], s);
      return row16_sum(s);
    };

    float dummy = 0.f;
    sweep(x, 0, r, dummy);
    if constexpr (KFULL)   // (p1_c / p2_c are the next pair's since the top of this iteration)
      request_indices(it + 1 < iters && ridx(it + 1) < n_rows, p1_c, p2_c - p1_c, (it + 1) & 1);
#pragma unroll
    for (int rr = 0; rr < RPN; rr++) p[rr] = r[rr];
    float rsold = dot16(r, r);
    bool conv = !live;   // a dead half keeps in step: its vectors are zero, its updates are masked
    // every step but the last, which leaves no r and no p behind (below)
    for (int itc = 0; itc + 1 < a.cg_steps; ++itc) {
      sweep(p, 1, ap, dummy);
      const float pap = dot16(p, ap);
      // rsold / alpha / beta as the reference holds them: double scalars fed by T-valued dot products (wrmf_implicit.hpp:18-27)
      const float alpha = conv ? 0.f : (float)((double)rsold / (double)pap);
      wave_sync();
      if (lgrp) tacc[lslot] = fmaf(alpha, tcur[lslot], tacc[lslot]);   // X_nnz^T x += alpha X_nnz^T p
      wave_sync();
#pragma unroll
      for (int rr = 0; rr < RPN; rr++) {
        x[rr] = fmaf(alpha, p[rr], x[rr]);
        r[rr] = fmaf(-alpha, ap[rr], r[rr]);
      }
      const float rsnew = dot16(r, r);   // (outside the per-half branch: the DPP reductions want whole rows of lanes)
      if (!conv) {
        if (rsnew < kCgTol) {
          conv = true;
        } else {
          const float beta = (float)((double)rsnew / (double)rsold);
#pragma unroll
          for (int rr = 0; rr < RPN; rr++) p[rr] = fmaf(p[rr], beta, r[rr]);
          rsold = rsnew;
        }
      }
    }
    // the last step: p' A p = p' G p + sum_j (c_j - 1) (x_j . p)^2 needs the dots and the dense product, not the vector A p --
    // nothing reads the residual behind it: the loss comes from t_acc, the row from x
    if (a.cg_steps > 0) {
      float pap = 0.f;
      sweep(p, 3, ap, pap);
      const float alpha = conv ? 0.f : (float)((double)rsold / (double)pap);
      wave_sync();
      if (lgrp) tacc[lslot] = fmaf(alpha, tcur[lslot], tacc[lslot]);
      wave_sync();
#pragma unroll
      for (int rr = 0; rr < RPN; rr++) x[rr] = fmaf(alpha, p[rr], x[rr]);
    }
    float rl = 0.f;
    sweep(x, 2, ap, rl);
    if constexpr (KFULL) {
      // settle the prefetched indices / values here (requested four sweeps ago): left to the next pair's first use, the wait would
      // sit behind that pair's warm-start request and behind this pair's store -- the vectors would be requested a round trip late
      settle_indices();
    }
    if (live) {
      const float xx = dot16(x, x);
      wloss += (double)rl + a.lambda_loss * (double)xx;
      if (QUAD || g2 == 0) {
#pragma unroll
        for (int b = 0; b < NV; b++) {
          const int off = b * 16 * VW + i * VW;
          if (off < k) {
            float4 pc;
            float* pf = reinterpret_cast<float*>(&pc);
#pragma unroll
            for (int c = 0; c < VW; c++) pf[c] = x[b * VW + c];
            *reinterpret_cast<float4*>(yrow + off) = pc;
          }
        }
      }
    }
  }
  const double other = __shfl(wloss, 32);
  // (the lane number counted afresh: `lane` would keep the thread id in a register across the row loop for this one test, the
  //  register that the two-row rank-128 kernel does not have)
  const bool first_lane = __lane_id() == 0;
  if constexpr (QUAD) {   // the wave's four groups
    const double wsum = (wloss + __shfl(wloss, 16)) + (other + __shfl(wloss, 48));
    if (first_lane) a.loss_partials[loss_slot0 + (size_t)blockIdx.x * 4 + wv] = wsum;
  } else {
    if (first_lane) a.loss_partials[loss_slot0 + (size_t)blockIdx.x * 4 + wv] = wloss + other;
  }
}

}  // namespace

bool cgp_supported(int k, bool implicit) { return implicit && k > 64 && k <= 128 && k % 4 == 0; }
bool cgp_wide_supported(int k, bool implicit, bool gbias) { return implicit && k == 128 && !gbias; }
bool cgp_quad_supported(int k, bool implicit, bool gbias) { return implicit && k == 128 && !gbias; }

// rows: n_rows row ids, rank 65..128 (multiple of 4), implicit feedback.  form kCgpPair: each with at most 16 non-zeros (empty
// ones included), two per wave; kCgpWide: 17..32 non-zeros, two per wave (cgp_wide_supported); kCgpQuad: at most 16 non-zeros
// (empty ones included), four per wave (cgp_quad_supported);
// loss partials: cgp_loss_slots(n_rows, cgp_rows_per_wave(form)) slots from loss_slot0 on (wrmf_schedule.h)
hipError_t launch_als_cgp(const AlsArgs& a, const int32_t* rows, int n_rows, CgpForm form, size_t loss_slot0, hipStream_t s,
                          hipEvent_t* ev_slot) {
  const int rpw = cgp_rows_per_wave(form);
  const int grid = cgp_grid(n_rows, rpw);
  if (grid <= 0) return hipSuccess;
  const int iters = cgp_visits(n_rows, rpw);
  const bool gb = a.gbias != 0.f;
  const bool full = !gb && a.k == 128;
  const bool wide = form == kCgpWide, quad = form == kCgpQuad;
  if ((wide || quad) && !full) return hipErrorInvalidValue;
  auto k0 = als_cgp_kernel<false, false>;
  auto k0f = als_cgp_kernel<false, true>;
  auto k1 = als_cgp_kernel<true, false>;
  auto kw = als_cgp_kernel<false, true, 16>;
  auto kq = als_cgp_kernel<false, true, 16, true>;
  const void* fn = quad ? reinterpret_cast<const void*>(kq) : wide ? reinterpret_cast<const void*>(kw)
                        : gb ? reinterpret_cast<const void*>(k1) : (full ? reinterpret_cast<const void*>(k0f) : reinterpret_cast<const void*>(k0));
  const size_t lds = quad ? PairSmem<16, true>::bytes : wide ? PairSmem<16>::bytes : PairSmem<8>::bytes;
  hipError_t err = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err != hipSuccess) return err;
  prof_note(ev_slot, fn);   // (names the bucket's segment when this is its first launch)
  if (quad) hipLaunchKernelGGL(kq, dim3(grid), dim3(256), lds, s, a, rows, n_rows, iters, loss_slot0);
  else if (wide) hipLaunchKernelGGL(kw, dim3(grid), dim3(256), lds, s, a, rows, n_rows, iters, loss_slot0);
  else if (gb) hipLaunchKernelGGL(k1, dim3(grid), dim3(256), lds, s, a, rows, n_rows, iters, loss_slot0);
  else if (full) hipLaunchKernelGGL(k0f, dim3(grid), dim3(256), lds, s, a, rows, n_rows, iters, loss_slot0);
  else hipLaunchKernelGGL(k0, dim3(grid), dim3(256), lds, s, a, rows, n_rows, iters, loss_slot0);
  return hipGetLastError();
}

}  // namespace rsparse_hip
