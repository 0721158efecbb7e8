// Second-order factorization machine by deterministic mini-batch SGD, on the device (gfx950).  rsparse_amd/fm.py
// (fm_forward_reference, fm_step_reference) is the definition in numpy, the C header states it for other hosts; DESIGN.md 3.38 has
// the scheme.  A step takes the rows r = step, step + n_steps, ... (k numbers them) from a snapshot of (w0, w, V):
//
//   index     once per (x, n_steps): one stable rocprim radix sort of the stored positions by (step(r) << bits(d)) | column on
//             exactly the key bits in use, payload = the CSR position; stability keeps the rows ascending inside a (step, column)
//             segment.  Heads by comparison with the left neighbour and one scan give seg_ptr / seg_col; a bisection per step
//             gives the segment range of the step; a second scan numbers the chunks of the segments longer than
//             RSPARSE_HIP_BPR_CHUNK.  The step ranges are read back once, so every later grid is exact.
//   forward   a 16-lane group per row: lane l owns the coordinates c = l, l + 16, ..., so one gather instruction of a group reads
//             64 contiguous bytes of a row of V.  The entries are walked in ascending column with the next entry's row of V in
//             flight; s, q and lin are kept in double registers, chunk by chunk.  A row of more than RSPARSE_HIP_FM_LONG_ROW
//             entries is spread over the 16 groups of its workgroup, a chunk each, and the owner adds the chunk sums in order
//             from LDS.  Writes raw[k], delta[k], the row S[k, :] (float64) and the gaussian trace terms; the binomial count is an
//             integer in LDS with one integer atomic per workgroup.  The same kernel without those outputs is `predict`.
//   w0        one workgroup: the ordered sums of delta (the intercept's gradient) and of the gaussian trace terms -- a thread per
//             chunk, the chunk sums added in order from LDS by one thread each.
//   chunks    a group per chunk of a long segment: delta[k], x and S[k, :] per entry with the next one in flight.
//   update    a group per segment: a short segment walked directly, a long one's chunk sums added in order; the Adagrad update
//             of w[j], V[j, :], aw[j], aV[j, :] in place.  Only column j's segment reads or writes row j behind the forward launch.
// No float atomics, no host synchronisation between the steps or epochs of a call, every loop bounded by the data sizes.  The
// file is built with contraction off: every product, sum, quotient and root is its own rounded float64 operation.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <vector>

#include "../../include/rsparse_wrmf_hip.h"
#include "wrmf_internal.h"
#include "wrmf_device.h"
#include "wrmf_bpr_device.h"
#include "wrmf_fm_index.h"

#pragma clang fp contract(off)

namespace rsparse_hip {
namespace {

using namespace dev;
using namespace bprdev;
using namespace fmidx;

constexpr int kFmLongRow = RSPARSE_HIP_FM_LONG_ROW;
constexpr int kFmTile = kBprThreads;   // chunk sums of one round of the w0 kernel

// ---- the backward index (its layout: wrmf_fm_index.h, which wrmf_ftrl.hip reads too) --------------------------------------------
__device__ __forceinline__ int fm_row_of(const int32_t* __restrict__ p, int n_rows, int64_t pos) {
  int lo = 0, hi = n_rows;   // p[lo] <= pos < p[hi]
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((int64_t)p[mid] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kBprThreads) void fm_keys_kernel(const int32_t* __restrict__ p, const int32_t* __restrict__ j, int n_rows,
                                                              int n_feat, int nnz, int n_steps, int col_bits, u64* __restrict__ keys,
                                                              uint32_t* __restrict__ pay) {
  const int e = blockIdx.x * kBprThreads + threadIdx.x;
  if (e >= nnz) return;
  const int r = fm_row_of(p, n_rows, e);
  keys[e] = ((u64)(unsigned)(r % n_steps) << col_bits) | (u64)(unsigned)fm_col(j[e], n_feat);
  pay[e] = (uint32_t)e;
}
__global__ __launch_bounds__(kBprThreads) void fm_heads_kernel(const u64* __restrict__ skeys, int nnz, int32_t* __restrict__ flag) {
  const int i = blockIdx.x * kBprThreads + threadIdx.x;
  if (i < nnz) flag[i] = (i == 0 || skeys[i] != skeys[i - 1]) ? 1 : 0;
}
// inc: the inclusive scan of the head flags, so a head's segment is inc[i] - 1 and inc[nnz - 1] the number of segments
__global__ __launch_bounds__(kBprThreads) void fm_entries_kernel(const int32_t* __restrict__ p, int n_rows, int nnz, int n_steps,
                                                                 u64 col_mask, const u64* __restrict__ skeys,
                                                                 const int32_t* __restrict__ flag, const int32_t* __restrict__ inc,
                                                                 const uint32_t* __restrict__ spay, int32_t* __restrict__ sk,
                                                                 int32_t* __restrict__ seg_ptr, int32_t* __restrict__ seg_col) {
  const int i = blockIdx.x * kBprThreads + threadIdx.x;
  if (i >= nnz) return;
  sk[i] = fm_row_of(p, n_rows, (int64_t)spay[i]) / n_steps;
  if (flag[i]) {
    seg_ptr[inc[i] - 1] = i;
    seg_col[inc[i] - 1] = (int32_t)(skeys[i] & col_mask);
  }
  if (i == nnz - 1) seg_ptr[inc[i]] = nnz;
}
// nch[t], t = 0 .. nnz: the chunks of a segment longer than one chunk, else 0 (0 beyond the last segment too)
__global__ __launch_bounds__(kBprThreads) void fm_nch_kernel(const int32_t* __restrict__ seg_ptr, const int32_t* __restrict__ inc, int nnz,
                                                             int32_t* __restrict__ nch) {
  const int t = blockIdx.x * kBprThreads + threadIdx.x;
  if (t > nnz) return;
  const int len = t < inc[nnz - 1] ? seg_ptr[t + 1] - seg_ptr[t] : 0;
  nch[t] = len > kBprChunk ? (len + kBprChunk - 1) / kBprChunk : 0;
}
__global__ __launch_bounds__(kBprThreads) void fm_steps_kernel(const u64* __restrict__ skeys, const int32_t* __restrict__ inc,
                                                               const int32_t* __restrict__ choff, int nnz, int n_steps, int col_bits,
                                                               int32_t* __restrict__ hdr, int32_t* __restrict__ step_seg,
                                                               int32_t* __restrict__ step_ch) {
  const int s = blockIdx.x * kBprThreads + threadIdx.x;
  if (s > n_steps) return;
  const u64 want = (u64)(unsigned)s << col_bits;
  int lo = 0, hi = nnz;   // the first sorted position whose key is >= want
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (skeys[mid] < want) lo = mid + 1; else hi = mid;
  }
  const int n_seg = inc[nnz - 1], seg = lo < nnz ? inc[lo] - 1 : n_seg;
  step_seg[s] = seg;
  step_ch[s] = choff[seg];
  if (s == 0) {
    hdr[0] = kFmMagic; hdr[1] = n_steps; hdr[2] = nnz; hdr[3] = n_seg;
  }
}

inline int fm_bits(int64_t n) {   // bits that hold 0 .. n - 1, at least 1
  int b = 1;
  while (((int64_t)1 << b) < n) b++;
  return b;
}

#define RSP_TRY(e) do { if ((err = (e)) != hipSuccess) return err; } while (0)

// ---- the forward pass --------------------------------------------------------------------------------------------------------------
template <class T, int R16>
__device__ __forceinline__ void fm_row_load(const T* __restrict__ row, int rank, int lane, T (&out)[R16]) {
#pragma unroll
  for (int q = 0; q < R16; q++) {
    const int c = lane + kBprLanes * q;
    out[q] = c < rank ? row[c] : (T)0;
  }
}

// the sums of the m <= kBprChunk entries from e0 of a row, sequentially from +0.0: cs = sum t, cq = sum t t, cl = sum w x.  The
// column of entry i + 2 and the row of V of entry i + 1 are requested before entry i is multiplied.
template <class T, int R16>
__device__ __forceinline__ void fm_row_chunk(const int32_t* __restrict__ J, const T* __restrict__ X, const T* __restrict__ w,
                                             const T* __restrict__ V, int n_feat, int rank, int e0, int m, int lane, double (&cs)[R16],
                                             double (&cq)[R16], double& cl) {
#pragma unroll
  for (int q = 0; q < R16; q++) cs[q] = cq[q] = 0.0;
  cl = 0.0;
  if (m <= 0) return;
  T cur[R16], nxt[R16];
  int jn = fm_col(J[e0], n_feat), j2 = m > 1 ? fm_col(J[e0 + 1], n_feat) : 0;
  T xn = X[e0], wn = w[jn];
  fm_row_load<T, R16>(V + (size_t)jn * rank, rank, lane, nxt);
  for (int i = 0; i < m; i++) {
    const double xd = (double)xn, wd = (double)wn;
#pragma unroll
    for (int q = 0; q < R16; q++) cur[q] = nxt[q];
    if (i + 1 < m) {
      jn = j2;
      xn = X[e0 + i + 1];
      wn = w[jn];
      fm_row_load<T, R16>(V + (size_t)jn * rank, rank, lane, nxt);
      if (i + 2 < m) j2 = fm_col(J[e0 + i + 2], n_feat);
    }
#pragma unroll
    for (int q = 0; q < R16; q++) {
      const double t = (double)cur[q] * xd;
      cs[q] = cs[q] + t;
      cq[q] = cq[q] + t * t;
    }
    cl = cl + wd * xd;
  }
}

struct FmFwd {
  const int32_t* p;
  const int32_t* j;
  int n_feat, step, n_steps, cnt, rank, family, ld;   // ld: the doubles of a row of S, 16 ceil(rank / 16)
};

template <class T, int R16, bool TRAIN>
__global__ __launch_bounds__(kBprThreads) void fm_forward_kernel(FmFwd a, const T* __restrict__ X, const T* __restrict__ w0,
                                                                 const T* __restrict__ w, const T* __restrict__ V,
                                                                 const double* __restrict__ y, const double* __restrict__ omega,
                                                                 double* __restrict__ raw_out, double* __restrict__ delta,
                                                                 double* __restrict__ S, double* __restrict__ lterm,
                                                                 double* __restrict__ link, unsigned long long* __restrict__ count) {
  constexpr int W = kBprLanes * R16;
  __shared__ double sh[kBprGroups][2 * W + 1];   // a round's chunk sums of a long row: s, q, lin
  __shared__ int s_len[kBprGroups], s_e0[kBprGroups];
  __shared__ unsigned s_cnt;
  const int grp = threadIdx.x >> 4, lane = threadIdx.x & 15;
  const int k = blockIdx.x * kBprGroups + grp;
  const bool has = k < a.cnt;
  int64_t r = 0;
  int e0 = 0, len = 0;
  if (has) {
    r = (int64_t)a.step + (int64_t)k * a.n_steps;
    e0 = a.p[r];
    len = a.p[r + 1] - e0;
  }
  if (lane == 0) {
    s_len[grp] = has ? len : 0;
    s_e0[grp] = e0;
  }
  if (threadIdx.x == 0) s_cnt = 0u;
  double ts[R16], tq[R16], cs[R16], cq[R16], tl = 0.0, cl;
#pragma unroll
  for (int q = 0; q < R16; q++) ts[q] = tq[q] = 0.0;
  if (has && len <= kFmLongRow) {
    for (int c0 = 0; c0 < len; c0 += kBprChunk) {
      fm_row_chunk<T, R16>(a.j, X, w, V, a.n_feat, a.rank, e0 + c0, min(kBprChunk, len - c0), lane, cs, cq, cl);
#pragma unroll
      for (int q = 0; q < R16; q++) {
        ts[q] = ts[q] + cs[q];
        tq[q] = tq[q] + cq[q];
      }
      tl = tl + cl;
    }
  }
  __syncthreads();
  for (int g = 0; g < kBprGroups; g++) {   // the long rows of the workgroup, one after the other (every test is workgroup-uniform)
    const int L = s_len[g];
    if (L <= kFmLongRow) continue;
    const int ge0 = s_e0[g], n_chunks = (L + kBprChunk - 1) / kBprChunk;
    for (int c0 = 0; c0 < n_chunks; c0 += kBprGroups) {
      const int c = c0 + grp;
      if (c < n_chunks) {
        fm_row_chunk<T, R16>(a.j, X, w, V, a.n_feat, a.rank, ge0 + c * kBprChunk, min(kBprChunk, L - c * kBprChunk), lane, cs, cq, cl);
#pragma unroll
        for (int q = 0; q < R16; q++) {
          sh[grp][kBprLanes * q + lane] = cs[q];
          sh[grp][W + kBprLanes * q + lane] = cq[q];
        }
        if (lane == 0) sh[grp][2 * W] = cl;
      }
      __syncthreads();
      if (grp == g) {
        const int n = min(kBprGroups, n_chunks - c0);
        for (int i = 0; i < n; i++) {
#pragma unroll
          for (int q = 0; q < R16; q++) {
            ts[q] = ts[q] + sh[i][kBprLanes * q + lane];
            tq[q] = tq[q] + sh[i][W + kBprLanes * q + lane];
          }
          tl = tl + sh[i][2 * W];
        }
      }
      __syncthreads();
    }
  }
  double part = 0.0;
#pragma unroll
  for (int q = 0; q < R16; q++) part = part + (ts[q] * ts[q] - tq[q]);
  const double pair = bpr_reduce16(part);
  const double raw = ((double)w0[0] + tl) + 0.5 * pair;
  bool correct = false;
  if (has) {
    if (TRAIN) {
      const double yk = y[r], ok = omega[r];
      double dl;
      if (a.family == RSPARSE_HIP_FM_BINOMIAL) {
        const double m = yk * raw;
        dl = (-(ok * yk)) * (1.0 / (1.0 + fm_exp(m)));
        correct = lane == 0 && m > 0.0;
      } else {
        const double diff = raw - yk;
        dl = ok * diff;
        if (lane == 0 && lterm) lterm[k] = ok * (diff * diff);
      }
      if (lane == 0) {
        if (raw_out) raw_out[k] = raw;
        delta[k] = dl;
      }
#pragma unroll
      for (int q = 0; q < R16; q++)
        if (kBprLanes * q < a.ld) S[(size_t)k * a.ld + kBprLanes * q + lane] = ts[q];
    } else if (lane == 0) {
      link[k] = a.family == RSPARSE_HIP_FM_BINOMIAL ? 1.0 / (1.0 + fm_exp(-raw)) : raw;
    }
  }
  if (TRAIN && count) {
    const u64 bc = __ballot(correct);
    if ((threadIdx.x & 63) == 0 && bc) atomicAdd(&s_cnt, (unsigned)__popcll(bc));
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(count, (unsigned long long)s_cnt);
  }
}

// ---- the intercept and the gaussian trace ------------------------------------------------------------------------------------------
// one workgroup: osum_k(delta_k) and osum_k(lterm_k).  A thread sums a chunk sequentially; thread 0 (delta) and thread 64 (the
// trace terms, another wave) add a tile's chunk sums in order from LDS.
template <class T>
__global__ __launch_bounds__(kBprThreads) void fm_w0_kernel(const double* __restrict__ delta, const double* __restrict__ lterm, int cnt,
                                                            int intercept, double lr, T* __restrict__ w0, double* __restrict__ a0,
                                                            double* __restrict__ trace) {
  __shared__ double sd[kFmTile], sl[kFmTile];
  const int n_chunks = (cnt + kBprChunk - 1) / kBprChunk;
  double tot = 0.0;   // (thread 0: of delta; thread 64: of the trace terms)
  for (int c0 = 0; c0 < n_chunks; c0 += kFmTile) {
    const int c = c0 + (int)threadIdx.x;
    if (c < n_chunks) {
      const int k0 = c * kBprChunk, m = min(kBprChunk, cnt - k0);
      double ad = 0.0, al = 0.0;
      if (intercept)
        for (int i = 0; i < m; i++) ad = ad + delta[k0 + i];
      if (lterm)
        for (int i = 0; i < m; i++) al = al + lterm[k0 + i];
      sd[threadIdx.x] = ad;
      sl[threadIdx.x] = al;
    }
    __syncthreads();
    const int n = min(kFmTile, n_chunks - c0);
    if (threadIdx.x == 0)
      for (int i = 0; i < n; i++) tot = tot + sd[i];
    if (threadIdx.x == 64)
      for (int i = 0; i < n; i++) tot = tot + sl[i];
    __syncthreads();
  }
  if (threadIdx.x == 0 && intercept && cnt > 0) {
    const double th = (double)w0[0];
    const double g = tot + (0.0 * (double)cnt) * th;
    const double an = a0[0] + g * g;
    if (an != 0.0) w0[0] = (T)(th - (lr * g) / sqrt(an));
    a0[0] = an;
  }
  if (threadIdx.x == 64 && lterm) trace[0] = trace[0] + tot;
}

// ---- the backward pass -------------------------------------------------------------------------------------------------------------
// the sums of the m <= kBprChunk contributions at the sorted positions i0 .. of column j (vd: its row of V, widened), sequentially
// from +0.0: acc[c] = sum (delta x) (S[k, c] - V[j, c] x), lin = sum delta x.  The index pair of entry i + 2 and the gathered
// delta, x and row of S of entry i + 1 are requested before entry i is multiplied.
template <class T, int R16>
__device__ __forceinline__ void fm_col_walk(const uint32_t* __restrict__ spay, const int32_t* __restrict__ sk, const T* __restrict__ X,
                                            const double* __restrict__ delta, const double* __restrict__ S, const double (&vd)[R16],
                                            int ld, int i0, int m, int lane, double (&acc)[R16], double& lin) {
#pragma unroll
  for (int q = 0; q < R16; q++) acc[q] = 0.0;
  lin = 0.0;
  if (m <= 0) return;
  double cur[R16], nxt[R16];
  int kn = sk[i0], k2 = m > 1 ? sk[i0 + 1] : 0;
  uint32_t pn = spay[i0], p2 = m > 1 ? spay[i0 + 1] : 0u;
  T xn = X[pn];
  double dn = delta[kn];
#pragma unroll
  for (int q = 0; q < R16; q++) nxt[q] = kBprLanes * q < ld ? S[(size_t)kn * ld + kBprLanes * q + lane] : 0.0;
  for (int i = 0; i < m; i++) {
    const double xd = (double)xn, dx = dn * xd;
#pragma unroll
    for (int q = 0; q < R16; q++) cur[q] = nxt[q];
    if (i + 1 < m) {
      kn = k2; pn = p2;
      xn = X[pn];
      dn = delta[kn];
#pragma unroll
      for (int q = 0; q < R16; q++) nxt[q] = kBprLanes * q < ld ? S[(size_t)kn * ld + kBprLanes * q + lane] : 0.0;
      if (i + 2 < m) {
        k2 = sk[i0 + i + 2];
        p2 = spay[i0 + i + 2];
      }
    }
#pragma unroll
    for (int q = 0; q < R16; q++) acc[q] = acc[q] + dx * (cur[q] - vd[q] * xd);
    lin = lin + dx;
  }
}

struct FmBack {
  const uint32_t* spay;
  const int32_t *sk, *seg_ptr, *seg_col, *choff;
  int seg0, seg1, ch0, n_ch, rank, ld;
};

template <class T, int R16>
__device__ __forceinline__ void fm_widen(const T* __restrict__ row, int rank, int lane, double (&vd)[R16]) {
#pragma unroll
  for (int q = 0; q < R16; q++) {
    const int c = lane + kBprLanes * q;
    vd[q] = c < rank ? (double)row[c] : 0.0;
  }
}

// a group per chunk of the step's long segments: csum[g - ch0] = (W coordinates, lin)
template <class T, int R16>
__global__ __launch_bounds__(kBprThreads) void fm_chunks_kernel(FmBack b, const T* __restrict__ X, const double* __restrict__ delta,
                                                                const double* __restrict__ S, const T* __restrict__ V,
                                                                double* __restrict__ csum) {
  constexpr int W = kBprLanes * R16;
  const int gl = blockIdx.x * kBprGroups + (threadIdx.x >> 4), lane = threadIdx.x & 15;
  if (gl >= b.n_ch) return;
  const int g = b.ch0 + gl;
  int lo = b.seg0, hi = b.seg1;   // choff[lo] <= g < choff[hi]
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (b.choff[mid] <= g) lo = mid; else hi = mid;
  }
  const int start = b.seg_ptr[lo] + (g - b.choff[lo]) * kBprChunk, left = b.seg_ptr[lo + 1] - start;
  double vd[R16], acc[R16], lin;
  fm_widen<T, R16>(V + (size_t)b.seg_col[lo] * b.rank, b.rank, lane, vd);
  fm_col_walk<T, R16>(b.spay, b.sk, X, delta, S, vd, b.ld, start, left < kBprChunk ? left : kBprChunk, lane, acc, lin);
#pragma unroll
  for (int q = 0; q < R16; q++) csum[(size_t)gl * (W + 1) + kBprLanes * q + lane] = acc[q];
  if (lane == 0) csum[(size_t)gl * (W + 1) + W] = lin;
}

// a group per segment of the step: the totals, then the update of column j in place
template <class T, int R16>
__global__ __launch_bounds__(kBprThreads) void fm_update_kernel(FmBack b, const T* __restrict__ X, const double* __restrict__ delta,
                                                                const double* __restrict__ S, const double* __restrict__ csum,
                                                                double lr_w, double lr_v, double lambda_w, double lambda_v,
                                                                T* __restrict__ w, T* __restrict__ V, double* __restrict__ aw,
                                                                double* __restrict__ aV) {
  constexpr int W = kBprLanes * R16;
  const int sg = b.seg0 + blockIdx.x * kBprGroups + (threadIdx.x >> 4), lane = threadIdx.x & 15;
  if (sg >= b.seg1) return;
  const int i0 = b.seg_ptr[sg], len = b.seg_ptr[sg + 1] - i0, j = b.seg_col[sg];
  double vd[R16], acc[R16], tot[R16], lin, tlin = 0.0;
  fm_widen<T, R16>(V + (size_t)j * b.rank, b.rank, lane, vd);
#pragma unroll
  for (int q = 0; q < R16; q++) tot[q] = 0.0;
  if (len <= kBprChunk) {
    fm_col_walk<T, R16>(b.spay, b.sk, X, delta, S, vd, b.ld, i0, len, lane, acc, lin);
#pragma unroll
    for (int q = 0; q < R16; q++) tot[q] = tot[q] + acc[q];
    tlin = tlin + lin;
  } else {
    for (int g = b.choff[sg] - b.ch0; g < b.choff[sg + 1] - b.ch0; g++) {
#pragma unroll
      for (int q = 0; q < R16; q++) tot[q] = tot[q] + csum[(size_t)g * (W + 1) + kBprLanes * q + lane];
      tlin = tlin + csum[(size_t)g * (W + 1) + W];
    }
  }
  const double lv = lambda_v * (double)len, lw = lambda_w * (double)len;
#pragma unroll
  for (int q = 0; q < R16; q++) {
    const int c = lane + kBprLanes * q;
    if (c < b.rank) {
      const size_t at = (size_t)j * b.rank + c;
      const double g = tot[q] + lv * vd[q];
      const double an = aV[at] + g * g;
      if (an != 0.0) V[at] = (T)(vd[q] - (lr_v * g) / sqrt(an));
      aV[at] = an;
    }
  }
  if (lane == 0) {
    const double th = (double)w[j];
    const double g = tlin + lw * th;
    const double an = aw[j] + g * g;
    if (an != 0.0) w[j] = (T)(th - (lr_w * g) / sqrt(an));
    aw[j] = an;
  }
}

inline int fm_ld(int rank) { return kBprLanes * ((rank + kBprLanes - 1) / kBprLanes); }
inline int fm_cnt(int n_rows, int step, int n_steps) { return (int)(((int64_t)n_rows - step + n_steps - 1) / n_steps); }

inline FmFwd fm_fwd_of(const FmData& d, int step) {
  FmFwd a;
  a.p = d.p; a.j = d.j; a.n_feat = d.n_feat; a.step = step; a.n_steps = d.n_steps; a.cnt = fm_cnt(d.n_rows, step, d.n_steps);
  a.rank = d.rank; a.family = d.family; a.ld = fm_ld(d.rank);
  return a;
}

template <class T, int R16>
hipError_t fm_forward(const FmData& d, int step, const T* w0, const T* w, const T* V, const double* y, const double* omega, double* raw,
                      double* delta, double* S, double* link, hipStream_t s) {
  const FmFwd a = fm_fwd_of(d, step);
  if (a.cnt <= 0) return hipSuccess;
  const dim3 grid = bpr_grid(a.cnt, kBprGroups), block(kBprThreads);
  const T* X = static_cast<const T*>(d.x);
  if (y)
    hipLaunchKernelGGL((fm_forward_kernel<T, R16, true>), grid, block, 0, s, a, X, w0, w, V, y, omega, raw, delta, S, (double*)nullptr,
                       (double*)nullptr, (unsigned long long*)nullptr);
  else
    hipLaunchKernelGGL((fm_forward_kernel<T, R16, false>), grid, block, 0, s, a, X, w0, w, V, y, omega, raw, delta, S, (double*)nullptr,
                       link, (unsigned long long*)nullptr);
  return hipGetLastError();
}

template <class T, int R16>
hipError_t fm_run(const FmData& d, const void* index, const FmOpt& o, int n_epochs, int only_step, const double* y, const double* omega,
                  T* w0, T* w, T* V, double* a0, double* aw, double* aV, void* trace, hipStream_t s) {
  constexpr int W = kBprLanes * R16;
  hipError_t err;
  const FmIndex ix = fm_index_of(const_cast<void*>(index), d.nnz, d.n_steps);
  const size_t ns = (size_t)d.n_steps + 1;
  std::vector<int32_t> head(4 + 2 * ns);
  RSP_TRY(hipMemcpyAsync(head.data(), ix.hdr, head.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  RSP_TRY(hipStreamSynchronize(s));
  if (head[0] != kFmMagic || head[1] != d.n_steps || head[2] != (int32_t)d.nnz) return hipErrorInvalidValue;   // (another x or n_steps)
  const int32_t *step_seg = head.data() + 4, *step_ch = step_seg + ns;
  const int first = only_step < 0 ? 0 : only_step, last = only_step < 0 ? d.n_steps : only_step + 1;
  int max_ch = 0;
  for (int st = first; st < last; st++) max_ch = std::max(max_ch, step_ch[st + 1] - step_ch[st]);
  const size_t cm = (size_t)fm_cnt(d.n_rows, first, d.n_steps);
  const bool gauss = d.family == RSPARSE_HIP_FM_GAUSSIAN;
  DevBuf delta, lterm, S, csum;
  RSP_TRY(delta.alloc(cm * 8));
  if (gauss) RSP_TRY(lterm.alloc(cm * 8));
  RSP_TRY(S.alloc(cm * (size_t)fm_ld(d.rank) * 8));
  RSP_TRY(csum.alloc((size_t)max_ch * (W + 1) * 8));
  const T* X = static_cast<const T*>(d.x);
  const dim3 block(kBprThreads);
  FmBack b;
  b.spay = ix.spay; b.sk = ix.sk; b.seg_ptr = ix.seg_ptr; b.seg_col = ix.seg_col; b.choff = ix.choff; b.rank = d.rank; b.ld = fm_ld(d.rank);
  for (int e = 0; e < n_epochs; e++) {
    unsigned long long* count = gauss ? nullptr : static_cast<unsigned long long*>(trace) + e;
    double* loss = gauss ? static_cast<double*>(trace) + e : nullptr;
    for (int st = first; st < last; st++) {
      const FmFwd a = fm_fwd_of(d, st);
      if (a.cnt <= 0) continue;
      hipLaunchKernelGGL((fm_forward_kernel<T, R16, true>), bpr_grid(a.cnt, kBprGroups), block, 0, s, a, X, (const T*)w0, (const T*)w,
                         (const T*)V, y, omega, (double*)nullptr, delta.as<double>(), S.as<double>(), lterm.as<double>(),
                         (double*)nullptr, count);
      if (o.intercept || gauss)
        hipLaunchKernelGGL((fm_w0_kernel<T>), dim3(1), block, 0, s, (const double*)delta.as<double>(),
                           (const double*)(gauss ? lterm.as<double>() : nullptr), a.cnt, o.intercept, o.lr_w, w0, a0, loss);
      b.seg0 = step_seg[st]; b.seg1 = step_seg[st + 1]; b.ch0 = step_ch[st]; b.n_ch = step_ch[st + 1] - b.ch0;
      if (b.n_ch > 0)
        hipLaunchKernelGGL((fm_chunks_kernel<T, R16>), bpr_grid(b.n_ch, kBprGroups), block, 0, s, b, X, (const double*)delta.as<double>(),
                           (const double*)S.as<double>(), (const T*)V, csum.as<double>());
      if (b.seg1 > b.seg0)
        hipLaunchKernelGGL((fm_update_kernel<T, R16>), bpr_grid(b.seg1 - b.seg0, kBprGroups), block, 0, s, b, X,
                           (const double*)delta.as<double>(), (const double*)S.as<double>(), (const double*)csum.as<double>(), o.lr_w,
                           o.lr_v, o.lambda_w, o.lambda_v, w, V, aw, aV);
      RSP_TRY(hipGetLastError());
    }
  }
  RSP_TRY(hipStreamSynchronize(s));   // the scratch is freed on return
  return hipSuccess;
}

}  // namespace

size_t fm_index_bytes(int64_t nnz, int n_steps) { return fm_index_of(nullptr, nnz, n_steps).ints * sizeof(int32_t); }

hipError_t launch_fm_index(const FmData& d, void* ws, hipStream_t s) {
  hipError_t err;
  const FmIndex ix = fm_index_of(ws, d.nnz, d.n_steps);
  const size_t n = (size_t)d.nnz, ns = (size_t)d.n_steps + 1;
  if (n == 0) {   // no stored entry: every step has no segment
    std::vector<int32_t> head(4 + 2 * ns, 0);
    head[0] = kFmMagic; head[1] = d.n_steps;
    RSP_TRY(hipMemcpyAsync(ix.hdr, head.data(), head.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    return hipStreamSynchronize(s);
  }
  const int col_bits = fm_bits(d.n_feat), key_bits = col_bits + fm_bits(d.n_steps);
  DevBuf keys, skeys, pay, flag, inc, nch, tmp;
  RSP_TRY(keys.alloc(n * 8));
  RSP_TRY(skeys.alloc(n * 8));
  RSP_TRY(pay.alloc(n * 4));
  RSP_TRY(flag.alloc(n * 4));
  RSP_TRY(inc.alloc(n * 4));
  RSP_TRY(nch.alloc((n + 1) * 4));
  size_t sort_bytes = 0, inc_bytes = 0, ex_bytes = 0;
  RSP_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys.as<u64>(), skeys.as<u64>(), pay.as<uint32_t>(), ix.spay, n, 0, key_bits, s));
  RSP_TRY(rocprim::inclusive_scan(nullptr, inc_bytes, flag.as<int32_t>(), inc.as<int32_t>(), n, rocprim::plus<int32_t>(), s));
  RSP_TRY(rocprim::exclusive_scan(nullptr, ex_bytes, nch.as<int32_t>(), ix.choff, (int32_t)0, n + 1, rocprim::plus<int32_t>(), s));
  size_t tmp_bytes = std::max(sort_bytes, std::max(inc_bytes, ex_bytes));
  RSP_TRY(tmp.alloc(tmp_bytes));
  const dim3 block(kBprThreads), per_e = bpr_grid((int64_t)n, kBprThreads);
  hipLaunchKernelGGL(fm_keys_kernel, per_e, block, 0, s, d.p, d.j, d.n_rows, d.n_feat, (int)n, d.n_steps, col_bits, keys.as<u64>(),
                     pay.as<uint32_t>());
  RSP_TRY(hipGetLastError());
  RSP_TRY(rocprim::radix_sort_pairs(tmp.p, sort_bytes, keys.as<u64>(), skeys.as<u64>(), pay.as<uint32_t>(), ix.spay, n, 0, key_bits, s));
  hipLaunchKernelGGL(fm_heads_kernel, per_e, block, 0, s, (const u64*)skeys.as<u64>(), (int)n, flag.as<int32_t>());
  RSP_TRY(hipGetLastError());
  RSP_TRY(rocprim::inclusive_scan(tmp.p, inc_bytes, flag.as<int32_t>(), inc.as<int32_t>(), n, rocprim::plus<int32_t>(), s));
  hipLaunchKernelGGL(fm_entries_kernel, per_e, block, 0, s, d.p, d.n_rows, (int)n, d.n_steps, ((u64)1 << col_bits) - 1,
                     (const u64*)skeys.as<u64>(), (const int32_t*)flag.as<int32_t>(), (const int32_t*)inc.as<int32_t>(),
                     (const uint32_t*)ix.spay, ix.sk, ix.seg_ptr, ix.seg_col);
  hipLaunchKernelGGL(fm_nch_kernel, bpr_grid((int64_t)n + 1, kBprThreads), block, 0, s, (const int32_t*)ix.seg_ptr,
                     (const int32_t*)inc.as<int32_t>(), (int)n, nch.as<int32_t>());
  RSP_TRY(hipGetLastError());
  RSP_TRY(rocprim::exclusive_scan(tmp.p, ex_bytes, nch.as<int32_t>(), ix.choff, (int32_t)0, n + 1, rocprim::plus<int32_t>(), s));
  hipLaunchKernelGGL(fm_steps_kernel, bpr_grid((int64_t)ns, kBprThreads), block, 0, s, (const u64*)skeys.as<u64>(),
                     (const int32_t*)inc.as<int32_t>(), (const int32_t*)ix.choff, (int)n, d.n_steps, col_bits, ix.hdr, ix.step_seg,
                     ix.step_ch);
  RSP_TRY(hipGetLastError());
  return hipStreamSynchronize(s);   // the scratch is freed on return
}

template <class T>
hipError_t launch_fm_forward(const FmData& d, int step, const T* w0, const T* w, const T* V, const double* y, const double* omega,
                             double* raw, double* delta, double* S, double* link, hipStream_t s) {
  const int r16 = (d.rank + kBprLanes - 1) / kBprLanes;
  if (r16 <= 1) return fm_forward<T, 1>(d, step, w0, w, V, y, omega, raw, delta, S, link, s);
  if (r16 <= 2) return fm_forward<T, 2>(d, step, w0, w, V, y, omega, raw, delta, S, link, s);
  if (r16 <= 4) return fm_forward<T, 4>(d, step, w0, w, V, y, omega, raw, delta, S, link, s);
  return fm_forward<T, 8>(d, step, w0, w, V, y, omega, raw, delta, S, link, s);
}
template hipError_t launch_fm_forward<float>(const FmData&, int, const float*, const float*, const float*, const double*, const double*,
                                             double*, double*, double*, double*, hipStream_t);
template hipError_t launch_fm_forward<double>(const FmData&, int, const double*, const double*, const double*, const double*,
                                              const double*, double*, double*, double*, double*, hipStream_t);

template <class T>
hipError_t launch_fm_run(const FmData& d, const void* index, const FmOpt& o, int n_epochs, int only_step, const double* y,
                         const double* omega, T* w0, T* w, T* V, double* a0, double* aw, double* aV, void* trace, hipStream_t s) {
  const int r16 = (d.rank + kBprLanes - 1) / kBprLanes;
  if (r16 <= 1) return fm_run<T, 1>(d, index, o, n_epochs, only_step, y, omega, w0, w, V, a0, aw, aV, trace, s);
  if (r16 <= 2) return fm_run<T, 2>(d, index, o, n_epochs, only_step, y, omega, w0, w, V, a0, aw, aV, trace, s);
  if (r16 <= 4) return fm_run<T, 4>(d, index, o, n_epochs, only_step, y, omega, w0, w, V, a0, aw, aV, trace, s);
  return fm_run<T, 8>(d, index, o, n_epochs, only_step, y, omega, w0, w, V, a0, aw, aV, trace, s);
}
template hipError_t launch_fm_run<float>(const FmData&, const void*, const FmOpt&, int, int, const double*, const double*, float*, float*,
                                         float*, double*, double*, double*, void*, hipStream_t);
template hipError_t launch_fm_run<double>(const FmData&, const void*, const FmOpt&, int, int, const double*, const double*, double*,
                                          double*, double*, double*, double*, double*, void*, hipStream_t);

#undef RSP_TRY

}  // namespace rsparse_hip
