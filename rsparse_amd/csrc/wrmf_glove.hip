// GloVe by deterministic mini-batch SGD, on the device (gfx950).  rsparse_amd/glove.py (glove_slots_reference, glove_step_reference)
// is the definition in numpy, the C header states it for other hosts; DESIGN.md 3.40 has the scheme.  A step takes the stored
// positions p = step, step + n_steps, ... (k numbers them) from a snapshot of (W_i, W_j, b_i, b_j).  The step is two-sided: slot k
// sends cost_k W_j[c_k] to row r_k and cost_k W_i[r_k] to column c_k, both read from the same snapshot, so it is two gather passes
// over the factor rows themselves with one scalar per slot between them:
//
//   index     once per (x, n_steps), both sides.  Row side: no sort -- in the order (step, k) the key (step << bits(n)) | row already
//             ascends, so it is written directly.  Column side: one stable rocprim radix sort of the positions by
//             (step << bits(n)) | column on exactly the key bits in use, payload = the position; stability keeps k ascending inside
//             a (step, column) segment.  For either side: heads by comparison with the left neighbour and one scan give seg_ptr /
//             seg_dst; a bisection per step gives the segment range of the step; a second scan numbers the chunks of the segments
//             longer than RSPARSE_HIP_BPR_CHUNK.  The step ranges are read back once, so every later grid is exact.
//   walk      a 16-lane group per destination: lane l owns the coordinates q = l, l + 16, ..., so one gather instruction of a group
//             reads 64 contiguous bytes of a factor row.  The destination's own row is widened once into registers; the slots are
//             walked in ascending k with three stages in flight: the source row of slot k + 1, the indices and scalars of slot k + 2,
//             the sorted position of slot k + 3.  Totals and chunk sums are double registers.
//   row side  (first) gathers W_j[c_k] and b_j[c_k]; dot by bpr_reduce16, then inner, cost and term; writes cost[k] and term[k] --
//             two doubles per slot are all that passes between the sides.  The Adagrad update of W_i[r] is STAGED (the column side
//             must still gather the snapshot of W_i); b_i[r] and the states are written in place: only row r's own group reads them.
//   col side  reads cost[k], gathers the snapshot W_i[r_k]; updates W_j[c], b_j[c] and their states in place: only column c's
//             segment touches them behind the row side.
//   chunks    either side: a group per chunk of a segment longer than one chunk; the owner adds the chunk sums in order.
//   commit    a streaming kernel scatters the staged rows into W_i.
//   cost      one workgroup: 0.5 osum_k(term_k), added to the trace slot.
// The per-call workspace is O(batch rank): cost, term, the staged rows in the model's type and the long segments' chunk sums;
// never a copy of a factor matrix.  No float atomics, no host synchronisation between the steps or epochs of a call, every loop
// bounded by the data sizes, no transcendental.  The file is built with contraction off: every product, sum, quotient and root is
// its own rounded float64 operation.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <vector>

#include "../../include/rsparse_wrmf_hip.h"
#include "wrmf_internal.h"
#include "wrmf_device.h"
#include "wrmf_bpr_device.h"

#pragma clang fp contract(off)

namespace rsparse_hip {
namespace {

using namespace dev;
using namespace bprdev;

constexpr int kGloveMagic = 0x474c5645;
constexpr int kGloveTile = kBprThreads;   // chunk sums of one round of the cost kernel
constexpr double kGloveClip = 100.0;      // CLIP_VALUE of the modelled-on solver

// ---- the index -------------------------------------------------------------------------------------------------------------------
// the workspace, in int32 units: header (magic, n_steps, nnz, n), then per side step_seg[n_steps + 1] and step_ch[n_steps + 1]
// (row side first), then per side spay[nnz], sk[nnz], seg_dst[nnz], seg_ptr[nnz + 1], choff[nnz + 1] (n_seg <= nnz bounds the last
// three)
struct GloveSide {
  uint32_t* spay;
  int32_t *sk, *seg_dst, *seg_ptr, *choff, *step_seg, *step_ch;
};
struct GloveIndex {
  int32_t* hdr;
  GloveSide side[2];
  size_t head, ints;
};
inline GloveIndex glove_index_of(void* ws, int64_t nnz, int n_steps) {
  GloveIndex ix;
  int32_t* b = static_cast<int32_t*>(ws);
  const size_t n = (size_t)nnz, ns = (size_t)n_steps + 1, per = 5 * n + 2;
  ix.hdr = b;
  ix.head = 4 + 4 * ns;
  const size_t body = (ix.head + 3) / 4 * 4;
  for (int t = 0; t < 2; t++) {
    GloveSide& sd = ix.side[t];
    sd.step_seg = b + 4 + (size_t)t * 2 * ns;
    sd.step_ch = sd.step_seg + ns;
    int32_t* m = b + body + (size_t)t * per;
    sd.spay = reinterpret_cast<uint32_t*>(m);
    sd.sk = m + n; sd.seg_dst = m + 2 * n; sd.seg_ptr = m + 3 * n; sd.choff = m + 4 * n + 1;
  }
  ix.ints = body + 2 * per;
  return ix;
}

__device__ __forceinline__ int glove_id(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }   // (never outside the factors)

// Row side: sorted position i is slot k of step s, the steps one after the other.  With q = nnz / n_steps and rem = nnz % n_steps
// the steps below rem hold q + 1 slots and the others q (n_steps <= nnz, so q >= 1).
__global__ __launch_bounds__(kBprThreads) void glove_row_keys_kernel(const int32_t* __restrict__ rows, int n, int nnz, int n_steps,
                                                                     int bits, u64* __restrict__ skeys, uint32_t* __restrict__ spay) {
  const int64_t i = (int64_t)blockIdx.x * kBprThreads + threadIdx.x;
  if (i >= nnz) return;
  const int q = nnz / n_steps, rem = nnz % n_steps;
  const int64_t big = (int64_t)rem * (q + 1);
  int s, k;
  if (i < big) {
    s = (int)(i / (q + 1)); k = (int)(i % (q + 1));
  } else {
    s = rem + (int)((i - big) / q); k = (int)((i - big) % q);
  }
  const int64_t p = (int64_t)s + (int64_t)k * n_steps;   // < nnz
  skeys[i] = ((u64)(unsigned)s << bits) | (u64)(unsigned)glove_id(rows[p], n);
  spay[i] = (uint32_t)p;
}
__global__ __launch_bounds__(kBprThreads) void glove_col_keys_kernel(const int32_t* __restrict__ cols, int n, int nnz, int n_steps,
                                                                     int bits, u64* __restrict__ keys, uint32_t* __restrict__ pay) {
  const int64_t e = (int64_t)blockIdx.x * kBprThreads + threadIdx.x;
  if (e >= nnz) return;
  keys[e] = ((u64)(unsigned)(e % n_steps) << bits) | (u64)(unsigned)glove_id(cols[e], n);
  pay[e] = (uint32_t)e;
}
__global__ __launch_bounds__(kBprThreads) void glove_heads_kernel(const u64* __restrict__ skeys, int nnz, int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * kBprThreads + threadIdx.x;
  if (i < nnz) flag[i] = (i == 0 || skeys[i] != skeys[i - 1]) ? 1 : 0;
}
// inc: the inclusive scan of the head flags, so a head's segment is inc[i] - 1 and inc[nnz - 1] the number of segments
__global__ __launch_bounds__(kBprThreads) void glove_entries_kernel(int nnz, int n_steps, u64 dst_mask, const u64* __restrict__ skeys,
                                                                    const int32_t* __restrict__ flag, const int32_t* __restrict__ inc,
                                                                    const uint32_t* __restrict__ spay, int32_t* __restrict__ sk,
                                                                    int32_t* __restrict__ seg_ptr, int32_t* __restrict__ seg_dst) {
  const int64_t i = (int64_t)blockIdx.x * kBprThreads + threadIdx.x;
  if (i >= nnz) return;
  sk[i] = (int32_t)(spay[i] / (uint32_t)n_steps);
  if (flag[i]) {
    seg_ptr[inc[i] - 1] = (int32_t)i;
    seg_dst[inc[i] - 1] = (int32_t)(skeys[i] & dst_mask);
  }
  if (i == nnz - 1) seg_ptr[inc[i]] = nnz;
}
// nch[t], t = 0 .. nnz: the chunks of a segment longer than one chunk, else 0 (0 beyond the last segment too)
__global__ __launch_bounds__(kBprThreads) void glove_nch_kernel(const int32_t* __restrict__ seg_ptr, const int32_t* __restrict__ inc,
                                                                int nnz, int32_t* __restrict__ nch) {
  const int64_t t = (int64_t)blockIdx.x * kBprThreads + threadIdx.x;
  if (t > nnz) return;
  const int len = t < inc[nnz - 1] ? seg_ptr[t + 1] - seg_ptr[t] : 0;
  nch[t] = len > kBprChunk ? (len + kBprChunk - 1) / kBprChunk : 0;
}
__global__ __launch_bounds__(kBprThreads) void glove_steps_kernel(const u64* __restrict__ skeys, const int32_t* __restrict__ inc,
                                                                  const int32_t* __restrict__ choff, int nnz, int n_steps, int bits,
                                                                  int32_t* __restrict__ step_seg, int32_t* __restrict__ step_ch) {
  const int s = blockIdx.x * kBprThreads + threadIdx.x;
  if (s > n_steps) return;
  const u64 want = (u64)(unsigned)s << bits;
  int lo = 0, hi = nnz;   // the first sorted position whose key is >= want
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (skeys[mid] < want) lo = mid + 1; else hi = mid;
  }
  const int n_seg = inc[nnz - 1], seg = lo < nnz ? inc[lo] - 1 : n_seg;
  step_seg[s] = seg;
  step_ch[s] = choff[seg];
}
__global__ void glove_header_kernel(int n_steps, int nnz, int n, int32_t* __restrict__ hdr) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    hdr[0] = kGloveMagic; hdr[1] = n_steps; hdr[2] = nnz; hdr[3] = n;
  }
}

inline int glove_bits(int64_t n) {   // bits that hold 0 .. n - 1, at least 1
  int b = 1;
  while (((int64_t)1 << b) < n) b++;
  return b;
}

#define RSP_TRY(e) do { if ((err = (e)) != hipSuccess) return err; } while (0)

struct GloveScratch {   // what both sides of the index build share
  DevBuf flag, inc, nch, tmp;
  size_t inc_bytes = 0, ex_bytes = 0;
};

// the segments, the step ranges and the chunk numbering of one side from its sorted keys (spay is already in place)
hipError_t glove_side_index(const u64* skeys, const GloveSide& sd, size_t n, int n_steps, int bits, GloveScratch& w, hipStream_t s) {
  hipError_t err;
  const dim3 block(kBprThreads), per_e = bpr_grid((int64_t)n, kBprThreads);
  hipLaunchKernelGGL(glove_heads_kernel, per_e, block, 0, s, skeys, (int)n, w.flag.as<int32_t>());
  RSP_TRY(hipGetLastError());
  RSP_TRY(rocprim::inclusive_scan(w.tmp.p, w.inc_bytes, w.flag.as<int32_t>(), w.inc.as<int32_t>(), n, rocprim::plus<int32_t>(), s));
  hipLaunchKernelGGL(glove_entries_kernel, per_e, block, 0, s, (int)n, n_steps, ((u64)1 << bits) - 1, skeys,
                     (const int32_t*)w.flag.as<int32_t>(), (const int32_t*)w.inc.as<int32_t>(), (const uint32_t*)sd.spay, sd.sk,
                     sd.seg_ptr, sd.seg_dst);
  hipLaunchKernelGGL(glove_nch_kernel, bpr_grid((int64_t)n + 1, kBprThreads), block, 0, s, (const int32_t*)sd.seg_ptr,
                     (const int32_t*)w.inc.as<int32_t>(), (int)n, w.nch.as<int32_t>());
  RSP_TRY(hipGetLastError());
  RSP_TRY(rocprim::exclusive_scan(w.tmp.p, w.ex_bytes, w.nch.as<int32_t>(), sd.choff, (int32_t)0, n + 1, rocprim::plus<int32_t>(), s));
  hipLaunchKernelGGL(glove_steps_kernel, bpr_grid((int64_t)n_steps + 1, kBprThreads), block, 0, s, skeys,
                     (const int32_t*)w.inc.as<int32_t>(), (const int32_t*)sd.choff, (int)n, n_steps, bits, sd.step_seg, sd.step_ch);
  return hipGetLastError();
}

// ---- the walk ----------------------------------------------------------------------------------------------------------------------
struct GloveArgs {   // one side of one step
  const uint32_t* spay;
  const int32_t *sk, *seg_ptr, *seg_dst, *choff;
  const int32_t* src_id;   // by stored position: the columns (row side) or the rows (column side)
  int seg0, seg1, ch0, n_ch, rank, n;
};

template <class T, int R16>
__device__ __forceinline__ void glove_row_load(const T* __restrict__ row, int rank, int lane, T (&out)[R16]) {
#pragma unroll
  for (int q = 0; q < R16; q++) {
    const int c = lane + kBprLanes * q;
    out[q] = c < rank ? row[c] : (T)0;
  }
}
template <class T, int R16>
__device__ __forceinline__ void glove_widen(const T* row, int rank, int lane, double (&vd)[R16]) {
#pragma unroll
  for (int q = 0; q < R16; q++) {
    const int c = lane + kBprLanes * q;
    vd[q] = c < rank ? (double)row[c] : 0.0;
  }
}

// The sums of the m <= kBprChunk contributions at the sorted positions i0 .. of one destination, sequentially from +0.0:
// acc[q] = sum cost_k Wsrc[src_k, q], lin = sum cost_k.  SIDE 0 computes cost_k (own, bo: the destination's row, widened, and its
// bias) and writes cost[k] and term[k]; SIDE 1 reads cost[k].  Three stages are in flight: before slot i is multiplied, the source
// row (and bias) of slot i + 1, the source index and the scalars of slot i + 2 and the sorted position of slot i + 3 are requested,
// each from values that an earlier iteration loaded.
template <class T, int R16, int SIDE>
__device__ __forceinline__ void glove_walk(const GloveArgs& a, const T* __restrict__ fx, const T* __restrict__ lx,
                                           const T* __restrict__ Wsrc, const T* __restrict__ bsrc, const double (&own)[R16], double bo,
                                           double* cost, double* term, int i0, int m, int lane, double (&acc)[R16], double& lin) {
#pragma unroll
  for (int q = 0; q < R16; q++) acc[q] = 0.0;
  lin = 0.0;
  if (m <= 0) return;
  T cur[R16], nxt[R16];
  // slot 0 (suffix 1 below: "the next slot"), slot 1 (suffix 2) and the position of slot 2 (suffix 3)
  uint32_t p3 = a.spay[i0];
  int k1 = a.sk[i0], k2 = 0, k3 = 0;
  int s2 = glove_id(a.src_id[p3], a.n);
  T f1 = (T)0, l1 = (T)0, f2 = (T)0, l2 = (T)0, bn = (T)0;
  double c1 = 0.0, c2 = 0.0;
  if (SIDE == 0) {
    f1 = fx[p3]; l1 = lx[p3]; bn = bsrc[s2];
  } else {
    c1 = cost[k1];
  }
  glove_row_load<T, R16>(Wsrc + (size_t)s2 * a.rank, a.rank, lane, nxt);
  if (m > 1) {
    p3 = a.spay[i0 + 1];
    k2 = a.sk[i0 + 1];
    s2 = glove_id(a.src_id[p3], a.n);
    if (SIDE == 0) {
      f2 = fx[p3]; l2 = lx[p3];
    } else {
      c2 = cost[k2];
    }
  }
  if (m > 2) {
    p3 = a.spay[i0 + 2];
    k3 = a.sk[i0 + 2];
  }
  for (int i = 0; i < m; i++) {
    const int k = k1;
    const double f = (double)f1, l = (double)l1, bj = (double)bn, cs = c1;
#pragma unroll
    for (int q = 0; q < R16; q++) cur[q] = nxt[q];
    if (i + 1 < m) {
      glove_row_load<T, R16>(Wsrc + (size_t)s2 * a.rank, a.rank, lane, nxt);
      if (SIDE == 0) bn = bsrc[s2];
      k1 = k2; f1 = f2; l1 = l2; c1 = c2;
      if (i + 2 < m) {
        s2 = glove_id(a.src_id[p3], a.n);
        k2 = k3;
        if (SIDE == 0) {
          f2 = fx[p3]; l2 = lx[p3];
        } else {
          c2 = cost[k3];
        }
        if (i + 3 < m) {
          p3 = a.spay[i0 + i + 3];
          k3 = a.sk[i0 + i + 3];
        }
      }
    }
    double c;
    if (SIDE == 0) {
      double part = 0.0;
#pragma unroll
      for (int q = 0; q < R16; q++) part = part + own[q] * (double)cur[q];
      const double raw = ((bpr_reduce16(part) + bo) + bj) - l;
      const double inner = raw < -kGloveClip ? -kGloveClip : (raw > kGloveClip ? kGloveClip : raw);
      c = f * inner;
      if (lane == 0) {
        cost[k] = c;
        term[k] = c * inner;
      }
    } else {
      c = cs;
    }
#pragma unroll
    for (int q = 0; q < R16; q++) acc[q] = acc[q] + c * (double)cur[q];
    lin = lin + c;
  }
}

// a group per chunk of the step's long segments: csum[g - ch0] = (W coordinates, lin)
template <class T, int R16, int SIDE>
__global__ __launch_bounds__(kBprThreads) void glove_chunks_kernel(GloveArgs a, const T* __restrict__ fx, const T* __restrict__ lx,
                                                                   const T* Wown, const T* bown, const T* __restrict__ Wsrc,
                                                                   const T* __restrict__ bsrc, double* cost, double* term,
                                                                   double* __restrict__ csum) {
  constexpr int W = kBprLanes * R16;
  const int gl = blockIdx.x * kBprGroups + (threadIdx.x >> 4), lane = threadIdx.x & 15;
  if (gl >= a.n_ch) return;
  const int g = a.ch0 + gl;
  int lo = a.seg0, hi = a.seg1;   // choff[lo] <= g < choff[hi]
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (a.choff[mid] <= g) lo = mid; else hi = mid;
  }
  const int start = a.seg_ptr[lo] + (g - a.choff[lo]) * kBprChunk, left = a.seg_ptr[lo + 1] - start;
  double own[R16], acc[R16], lin, bo = 0.0;
  if (SIDE == 0) {
    const int dst = a.seg_dst[lo];
    glove_widen<T, R16>(Wown + (size_t)dst * a.rank, a.rank, lane, own);
    bo = (double)bown[dst];
  } else {
#pragma unroll
    for (int q = 0; q < R16; q++) own[q] = 0.0;
  }
  glove_walk<T, R16, SIDE>(a, fx, lx, Wsrc, bsrc, own, bo, cost, term, start, left < kBprChunk ? left : kBprChunk, lane, acc, lin);
#pragma unroll
  for (int q = 0; q < R16; q++) csum[(size_t)gl * (W + 1) + kBprLanes * q + lane] = acc[q];
  if (lane == 0) csum[(size_t)gl * (W + 1) + W] = lin;
}

// a group per segment of the step: the totals, then the Adagrad update of the destination.  SIDE 0 writes the new row of W_i to
// stage[segment - seg0] (the column side still gathers the snapshot), SIDE 1 writes W_j in place; the bias and the states of the
// destination are read and written by this group alone.
template <class T, int R16, int SIDE>
__global__ __launch_bounds__(kBprThreads) void glove_update_kernel(GloveArgs a, const T* __restrict__ fx, const T* __restrict__ lx,
                                                                   T* Wown, T* bown, const T* __restrict__ Wsrc,
                                                                   const T* __restrict__ bsrc, double* __restrict__ aW,
                                                                   double* __restrict__ ab, double* cost, double* term,
                                                                   const double* __restrict__ csum, double lr, double lambda,
                                                                   T* __restrict__ stage) {
  constexpr int W = kBprLanes * R16;
  const int sg = a.seg0 + blockIdx.x * kBprGroups + (threadIdx.x >> 4), lane = threadIdx.x & 15;
  if (sg >= a.seg1) return;
  const int i0 = a.seg_ptr[sg], len = a.seg_ptr[sg + 1] - i0, dst = a.seg_dst[sg];
  double own[R16], acc[R16], tot[R16], lin, tlin = 0.0;
  glove_widen<T, R16>(Wown + (size_t)dst * a.rank, a.rank, lane, own);
  const double bo = (double)bown[dst];
#pragma unroll
  for (int q = 0; q < R16; q++) tot[q] = 0.0;
  if (len <= kBprChunk) {
    glove_walk<T, R16, SIDE>(a, fx, lx, Wsrc, bsrc, own, bo, cost, term, i0, len, lane, acc, lin);
#pragma unroll
    for (int q = 0; q < R16; q++) tot[q] = tot[q] + acc[q];
    tlin = tlin + lin;
  } else {
    for (int g = a.choff[sg] - a.ch0; g < a.choff[sg + 1] - a.ch0; g++) {
#pragma unroll
      for (int q = 0; q < R16; q++) tot[q] = tot[q] + csum[(size_t)g * (W + 1) + kBprLanes * q + lane];
      tlin = tlin + csum[(size_t)g * (W + 1) + W];
    }
  }
  const double lw = lambda * (double)len, lb = 0.0 * (double)len;
#pragma unroll
  for (int q = 0; q < R16; q++) {
    const int c = lane + kBprLanes * q;
    if (c < a.rank) {
      const size_t at = (size_t)dst * a.rank + c;
      const double g = tot[q] + lw * own[q];
      const double an = aW[at] + g * g;
      const T nw = an != 0.0 ? (T)(own[q] - (lr * g) / sqrt(an)) : (T)own[q];
      if (SIDE == 0) stage[(size_t)(sg - a.seg0) * a.rank + c] = nw;
      else Wown[at] = nw;
      aW[at] = an;
    }
  }
  if (lane == 0) {
    const double g = tlin + lb * bo;
    const double an = ab[dst] + g * g;
    if (an != 0.0) bown[dst] = (T)(bo - (lr * g) / sqrt(an));
    ab[dst] = an;
  }
}

// the staged rows of the step's row segments into W_i
template <class T>
__global__ __launch_bounds__(kBprThreads) void glove_commit_kernel(const int32_t* __restrict__ seg_dst, int seg0, int n_seg, int rank,
                                                                   const T* __restrict__ stage, T* __restrict__ W) {
  const int64_t t = (int64_t)blockIdx.x * kBprThreads + threadIdx.x;
  if (t >= (int64_t)n_seg * rank) return;
  const int sg = (int)(t / rank), c = (int)(t % rank);
  W[(size_t)seg_dst[seg0 + sg] * rank + c] = stage[t];
}

// one workgroup: trace += 0.5 osum_k(term_k).  A thread sums a chunk sequentially; thread 0 adds a tile's chunk sums in order from LDS.
__global__ __launch_bounds__(kBprThreads) void glove_cost_kernel(const double* __restrict__ term, int cnt, double* __restrict__ trace) {
  __shared__ double sh[kGloveTile];
  const int n_chunks = (cnt + kBprChunk - 1) / kBprChunk;
  double tot = 0.0;
  for (int c0 = 0; c0 < n_chunks; c0 += kGloveTile) {
    const int c = c0 + (int)threadIdx.x;
    if (c < n_chunks) {
      const int k0 = c * kBprChunk, m = min(kBprChunk, cnt - k0);
      double t = 0.0;
      for (int i = 0; i < m; i++) t = t + term[k0 + i];
      sh[threadIdx.x] = t;
    }
    __syncthreads();
    const int n = min(kGloveTile, n_chunks - c0);
    if (threadIdx.x == 0)
      for (int i = 0; i < n; i++) tot = tot + sh[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) trace[0] = trace[0] + 0.5 * tot;
}

inline int glove_cnt(int64_t nnz, int step, int n_steps) { return (int)((nnz - step + n_steps - 1) / n_steps); }

template <class T, int R16>
hipError_t glove_run(const GloveData& d, const void* index, double lr, double lambda, int n_epochs, int only_step, T* Wi, T* Wj, T* bi,
                     T* bj, double* aWi, double* aWj, double* abi, double* abj, double* trace, hipStream_t s) {
  constexpr int W = kBprLanes * R16;
  hipError_t err;
  const GloveIndex ix = glove_index_of(const_cast<void*>(index), d.nnz, d.n_steps);
  const size_t ns = (size_t)d.n_steps + 1;
  std::vector<int32_t> head(ix.head);
  RSP_TRY(hipMemcpyAsync(head.data(), ix.hdr, head.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  RSP_TRY(hipStreamSynchronize(s));
  if (head[0] != kGloveMagic || head[1] != d.n_steps || head[2] != (int32_t)d.nnz || head[3] != d.n)
    return hipErrorInvalidValue;   // (another x or n_steps)
  const int32_t* step_seg[2] = {head.data() + 4, head.data() + 4 + 2 * ns};
  const int32_t* step_ch[2] = {step_seg[0] + ns, step_seg[1] + ns};
  const int first = only_step < 0 ? 0 : only_step, last = only_step < 0 ? d.n_steps : only_step + 1;
  int max_ch = 0, max_rows = 0;
  for (int st = first; st < last; st++) {
    for (int t = 0; t < 2; t++) max_ch = std::max(max_ch, step_ch[t][st + 1] - step_ch[t][st]);
    max_rows = std::max(max_rows, step_seg[0][st + 1] - step_seg[0][st]);
  }
  const size_t cm = (size_t)glove_cnt(d.nnz, first, d.n_steps);
  DevBuf cost, term, stage, csum;
  RSP_TRY(cost.alloc(cm * 8));
  RSP_TRY(term.alloc(cm * 8));
  RSP_TRY(stage.alloc((size_t)max_rows * d.rank * sizeof(T)));
  RSP_TRY(csum.alloc((size_t)max_ch * (W + 1) * 8));
  const T *fx = static_cast<const T*>(d.fx), *lx = static_cast<const T*>(d.lx);
  const dim3 block(kBprThreads);
  GloveArgs a[2];
  for (int t = 0; t < 2; t++) {
    const GloveSide& sd = ix.side[t];
    a[t].spay = sd.spay; a[t].sk = sd.sk; a[t].seg_ptr = sd.seg_ptr; a[t].seg_dst = sd.seg_dst; a[t].choff = sd.choff;
    a[t].src_id = t == 0 ? d.cols : d.rows; a[t].rank = d.rank; a[t].n = d.n;
  }
  double *c = cost.as<double>(), *tm = term.as<double>(), *cs = csum.as<double>();
  for (int e = 0; e < n_epochs; e++) {
    for (int st = first; st < last; st++) {
      const int cnt = glove_cnt(d.nnz, st, d.n_steps);
      if (cnt <= 0) continue;
      for (int t = 0; t < 2; t++) {
        a[t].seg0 = step_seg[t][st]; a[t].seg1 = step_seg[t][st + 1]; a[t].ch0 = step_ch[t][st];
        a[t].n_ch = step_ch[t][st + 1] - a[t].ch0;
      }
      if (a[0].n_ch > 0)
        hipLaunchKernelGGL((glove_chunks_kernel<T, R16, 0>), bpr_grid(a[0].n_ch, kBprGroups), block, 0, s, a[0], fx, lx, (const T*)Wi,
                           (const T*)bi, (const T*)Wj, (const T*)bj, c, tm, cs);
      hipLaunchKernelGGL((glove_update_kernel<T, R16, 0>), bpr_grid(a[0].seg1 - a[0].seg0, kBprGroups), block, 0, s, a[0], fx, lx, Wi, bi,
                         (const T*)Wj, (const T*)bj, aWi, abi, c, tm, (const double*)cs, lr, lambda, stage.as<T>());
      if (a[1].n_ch > 0)
        hipLaunchKernelGGL((glove_chunks_kernel<T, R16, 1>), bpr_grid(a[1].n_ch, kBprGroups), block, 0, s, a[1], fx, lx, (const T*)Wj,
                           (const T*)bj, (const T*)Wi, (const T*)bi, c, tm, cs);
      hipLaunchKernelGGL((glove_update_kernel<T, R16, 1>), bpr_grid(a[1].seg1 - a[1].seg0, kBprGroups), block, 0, s, a[1], fx, lx, Wj, bj,
                         (const T*)Wi, (const T*)bi, aWj, abj, c, tm, (const double*)cs, lr, lambda, (T*)nullptr);
      const int n_rows = a[0].seg1 - a[0].seg0;
      hipLaunchKernelGGL((glove_commit_kernel<T>), bpr_grid((int64_t)n_rows * d.rank, kBprThreads), block, 0, s, a[0].seg_dst, a[0].seg0,
                         n_rows, d.rank, (const T*)stage.as<T>(), Wi);
      hipLaunchKernelGGL(glove_cost_kernel, dim3(1), block, 0, s, (const double*)tm, cnt, trace + (only_step < 0 ? e : 0));
      RSP_TRY(hipGetLastError());
    }
  }
  RSP_TRY(hipStreamSynchronize(s));   // the scratch is freed on return
  return hipSuccess;
}

}  // namespace

size_t glove_index_bytes(int64_t nnz, int n_steps) { return glove_index_of(nullptr, nnz, n_steps).ints * sizeof(int32_t); }

hipError_t launch_glove_index(const GloveData& d, void* ws, hipStream_t s) {
  hipError_t err;
  const GloveIndex ix = glove_index_of(ws, d.nnz, d.n_steps);
  const size_t n = (size_t)d.nnz;
  if (n == 0) {   // no stored entry: every step has no segment
    std::vector<int32_t> head(ix.head, 0);
    head[0] = kGloveMagic; head[1] = d.n_steps; head[3] = d.n;
    RSP_TRY(hipMemcpyAsync(ix.hdr, head.data(), head.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    return hipStreamSynchronize(s);
  }
  const int bits = glove_bits(d.n), key_bits = bits + glove_bits(d.n_steps);
  DevBuf keys, skeys, pay;
  GloveScratch w;
  RSP_TRY(keys.alloc(n * 8));
  RSP_TRY(skeys.alloc(n * 8));
  RSP_TRY(pay.alloc(n * 4));
  RSP_TRY(w.flag.alloc(n * 4));
  RSP_TRY(w.inc.alloc(n * 4));
  RSP_TRY(w.nch.alloc((n + 1) * 4));
  size_t sort_bytes = 0;
  RSP_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys.as<u64>(), skeys.as<u64>(), pay.as<uint32_t>(), ix.side[1].spay, n, 0,
                                    key_bits, s));
  RSP_TRY(rocprim::inclusive_scan(nullptr, w.inc_bytes, w.flag.as<int32_t>(), w.inc.as<int32_t>(), n, rocprim::plus<int32_t>(), s));
  RSP_TRY(rocprim::exclusive_scan(nullptr, w.ex_bytes, w.nch.as<int32_t>(), ix.side[0].choff, (int32_t)0, n + 1, rocprim::plus<int32_t>(), s));
  RSP_TRY(w.tmp.alloc(std::max(sort_bytes, std::max(w.inc_bytes, w.ex_bytes))));
  const dim3 block(kBprThreads), per_e = bpr_grid((int64_t)n, kBprThreads);
  // the row side: the keys ascend as they are written
  hipLaunchKernelGGL(glove_row_keys_kernel, per_e, block, 0, s, d.rows, d.n, (int)n, d.n_steps, bits, skeys.as<u64>(), ix.side[0].spay);
  RSP_TRY(hipGetLastError());
  RSP_TRY(glove_side_index(skeys.as<u64>(), ix.side[0], n, d.n_steps, bits, w, s));
  // the column side: one stable sort
  hipLaunchKernelGGL(glove_col_keys_kernel, per_e, block, 0, s, d.cols, d.n, (int)n, d.n_steps, bits, keys.as<u64>(), pay.as<uint32_t>());
  RSP_TRY(hipGetLastError());
  RSP_TRY(rocprim::radix_sort_pairs(w.tmp.p, sort_bytes, keys.as<u64>(), skeys.as<u64>(), pay.as<uint32_t>(), ix.side[1].spay, n, 0,
                                    key_bits, s));
  RSP_TRY(glove_side_index(skeys.as<u64>(), ix.side[1], n, d.n_steps, bits, w, s));
  hipLaunchKernelGGL(glove_header_kernel, dim3(1), dim3(64), 0, s, d.n_steps, (int)n, d.n, ix.hdr);
  RSP_TRY(hipGetLastError());
  return hipStreamSynchronize(s);   // the scratch is freed on return
}

template <class T>
hipError_t launch_glove_run(const GloveData& d, const void* index, double lr, double lambda, int n_epochs, int only_step, T* Wi, T* Wj,
                            T* bi, T* bj, double* aWi, double* aWj, double* abi, double* abj, double* trace, hipStream_t s) {
  const int r16 = (d.rank + kBprLanes - 1) / kBprLanes;
  if (r16 <= 1) return glove_run<T, 1>(d, index, lr, lambda, n_epochs, only_step, Wi, Wj, bi, bj, aWi, aWj, abi, abj, trace, s);
  if (r16 <= 2) return glove_run<T, 2>(d, index, lr, lambda, n_epochs, only_step, Wi, Wj, bi, bj, aWi, aWj, abi, abj, trace, s);
  if (r16 <= 4) return glove_run<T, 4>(d, index, lr, lambda, n_epochs, only_step, Wi, Wj, bi, bj, aWi, aWj, abi, abj, trace, s);
  return glove_run<T, 8>(d, index, lr, lambda, n_epochs, only_step, Wi, Wj, bi, bj, aWi, aWj, abi, abj, trace, s);
}
template hipError_t launch_glove_run<float>(const GloveData&, const void*, double, double, int, int, float*, float*, float*, float*,
                                            double*, double*, double*, double*, double*, hipStream_t);
template hipError_t launch_glove_run<double>(const GloveData&, const void*, double, double, int, int, double*, double*, double*, double*,
                                             double*, double*, double*, double*, double*, hipStream_t);

#undef RSP_TRY

}  // namespace rsparse_hip
