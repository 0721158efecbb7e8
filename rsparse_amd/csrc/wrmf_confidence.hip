// Confidence weighting of the interaction matrix on the device (gfx950): BM25, TF-IDF, log / linear confidence and p-norm
// scaling of rows or columns -- the reference's `preprocess` hook (R/model_WRMF.R:184-188, 401-404) and its ScaleNormalize
// (R/model_ScaleNormalize.R), on the resident arrays of either orientation.  rsparse_amd/confidence.py (confidence_reference)
// is the definition in numpy; DESIGN.md 3.25 has the scheme and the measurements.
//
// A matrix is (p, i, x): n_seg segments ("rows" of the user-major arrays, "columns" of the item-major ones), p[0] = 0,
// p[n_seg] = nnz, doubles as in dgCMatrix@x.  Every kernel cuts [0, nnz) into SPANS of kConfSpan entries, whatever the
// segments look like: a workgroup takes kConfChunk consecutive spans, finds the segments that touch them by bisection in p (once over all of p, then
// each thread within that range), and in every span a thread owns four
// consecutive entries (two 16-byte loads).  One segment of 10^8 entries and 10^6 segments of one entry stream alike.
//
//   moments   out[r] = sum |x|^power over segment r, and the total.  Inside a span: a segmented scan over the workgroup in a
//             fixed order (four entries in the thread, Hillis-Steele over the wave, the four waves in sequence).  A segment that
//             lies inside the span is written by it; of a segment that crosses a span boundary the span keeps its part in the
//             scratch (head[s]: the segment began before the span; tail[s]: it began in the span and goes on) and a second
//             launch, one workgroup per boundary, adds tail[s0] + head[s0 + 1] + ... in a fixed tree.  The total is the sum of
//             the spans' totals, by the same tree.  No floating-point atomics, so repeat calls agree bit for bit; nothing is
//             read back and nothing waits.
//   table     per segment / per index: idf, K1 L_u, norm^(scale - 1).  log, log1p and pow run here, once per row or column.
//   apply     out[e] = f_kind(x[e], user table, item table): the table of the segments is read once per segment change, the
//             other one gathered by i[e] (plain loads: the table stays in L2 / MALL).  f is ONE device function of the same
//             three scalars in either orientation, compiled without contraction, so a cell gets the same bits in both -- and
//             every kind but "log" equals the numpy expression bit for bit.  double or float (rounded once) output; the output
//             may be the input.
#include "../../include/rsparse_wrmf_hip.h"
#include "wrmf_internal.h"

#pragma clang fp contract(off)

namespace rsparse_hip {
namespace {

constexpr int kConfSpan = 1024;      // entries per span: kConfThreads x kConfPer
constexpr int kConfThreads = 256;
constexpr int kConfPer = 4;
constexpr int kConfNoSeg = 0x7fffffff;
constexpr int kConfChunk = 8;         // consecutive spans a workgroup takes: one bisection over all of p for the chunk
constexpr int kConfGrid = 256 * 16;

// the largest r in [lo, hi) with p[r] <= e, given p[lo] <= e < p[hi] (the segment that holds entry e: empty ones are passed over)
__device__ __forceinline__ int conf_seg_of(const int32_t* __restrict__ p, int lo, int hi, int64_t e) {
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((int64_t)p[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// the segments of the four entries e0 .. e0 + 3 (kConfNoSeg at and beyond `end`), searched within [r_lo, r_hi)
__device__ __forceinline__ void conf_rows(const int32_t* __restrict__ p, int r_lo, int r_hi, int64_t e0, int64_t end, int (&r)[kConfPer]) {
  int cur = kConfNoSeg;
  int64_t next = 0;
#pragma unroll
  for (int q = 0; q < kConfPer; q++) {
    const int64_t e = e0 + q;
    if (e >= end) { r[q] = kConfNoSeg; continue; }
    if (cur == kConfNoSeg || e >= next) {
      cur = conf_seg_of(p, r_lo, r_hi, e);
      next = (int64_t)p[cur + 1];
    }
    r[q] = cur;
  }
}

__device__ __forceinline__ void conf_load4(const double* x, int64_t e0, int64_t end, bool aligned, double (&v)[kConfPer]) {
  if (aligned && e0 + kConfPer <= end) {
    const double2 a = reinterpret_cast<const double2*>(x + e0)[0], b = reinterpret_cast<const double2*>(x + e0)[1];
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
  } else {
#pragma unroll
    for (int q = 0; q < kConfPer; q++) v[q] = e0 + q < end ? x[e0 + q] : 0.0;
  }
}

// the sum of v over the workgroup in a fixed tree (every thread calls; the result is valid in thread 0)
__device__ __forceinline__ double conf_block_sum(double v, double* s_w) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_down(v, d);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// part: head[n_spans] | tail[n_spans] | span total[n_spans]
__global__ __launch_bounds__(kConfThreads) void conf_moments_kernel(const int32_t* __restrict__ p, const double* __restrict__ x, int n_seg,
                                                                    int64_t nnz, int power, int n_spans, double* __restrict__ out,
                                                                    double* __restrict__ part) {
  __shared__ int s_first[kConfThreads], s_last[kConfThreads], s_wf[4];
  __shared__ double s_incl[kConfThreads], s_wv[4], s_wt[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const bool aligned = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const int n_chunks = (n_spans + kConfChunk - 1) / kConfChunk;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
   const int64_t c_start = (int64_t)c * kConfChunk * kConfSpan;
   const int64_t c_end = c_start + kConfChunk * kConfSpan < nnz ? c_start + kConfChunk * kConfSpan : nnz;
   const int r_lo = conf_seg_of(p, 0, n_seg, c_start), r_hi = conf_seg_of(p, 0, n_seg, c_end - 1) + 1;
   const int s_end = (c + 1) * kConfChunk < n_spans ? (c + 1) * kConfChunk : n_spans;
   for (int s = c * kConfChunk; s < s_end; s++) {
    const int64_t start = (int64_t)s * kConfSpan, end = start + kConfSpan < nnz ? start + kConfSpan : nnz;
    const int64_t e0 = start + (int64_t)t * kConfPer;
    double v[kConfPer];
    conf_load4(x, e0, end, aligned, v);
#pragma unroll
    for (int q = 0; q < kConfPer; q++) v[q] = power == 2 ? v[q] * v[q] : fabs(v[q]);
    int r[kConfPer];
    conf_rows(p, r_lo, r_hi, e0, end, r);
    // the thread's own four: `tail` is the sum of its last run, brk says that a segment begins after its first entry
    bool brk = false;
    double tail = v[0];
#pragma unroll
    for (int q = 1; q < kConfPer; q++) {
      if (r[q] != r[q - 1]) { brk = true; tail = v[q]; } else tail = tail + v[q];
    }
    const double mine = (v[0] + v[1]) + (v[2] + v[3]);
    s_first[t] = r[0];
    s_last[t] = r[kConfPer - 1];
    __syncthreads();
    const bool joins = t > 0 && r[0] != kConfNoSeg && s_last[t - 1] == r[0];   // my first run continues the previous thread's last
    int f = (brk || !joins) ? 1 : 0;
    double sv = tail;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {   // inclusive segmented scan over the wave
      const int fo = __shfl_up(f, d);
      const double vo = __shfl_up(sv, d);
      if (lane >= d) {
        if (!f) sv = vo + sv;
        f |= fo;
      }
    }
    if (lane == 63) { s_wv[wave] = sv; s_wf[wave] = f; }
    __syncthreads();
    double cv = 0.0;
    for (int w = 0; w < wave; w++) cv = s_wf[w] ? s_wv[w] : cv + s_wv[w];
    if (!f) sv = cv + sv;
    s_incl[t] = sv;    // the sum of the run that ends with this thread's last entry, as far as it lies in the span
    __syncthreads();
    double run = joins ? s_incl[t - 1] : 0.0;
    const int after = t + 1 < kConfThreads ? s_first[t + 1] : kConfNoSeg;
#pragma unroll
    for (int q = 0; q < kConfPer; q++) {
      if (r[q] == kConfNoSeg) break;
      if (q > 0 && r[q] != r[q - 1]) run = 0.0;
      run = run + v[q];
      const int nxt = q + 1 < kConfPer ? r[q + 1] : after;
      if (nxt != r[q]) {   // the segment's last entry in this span
        const int64_t ps = (int64_t)p[r[q]], pe = (int64_t)p[r[q] + 1];
        if (ps >= start && pe <= end) out[r[q]] = run;
        else if (ps < start) part[s] = run;
        else part[(size_t)n_spans + s] = run;
      }
    }
    const double tot = conf_block_sum(mine, s_wt);
    if (t == 0) part[2 * (size_t)n_spans + s] = tot;
    __syncthreads();
   }
  }
}

// workgroup 0: total = the sum of the spans' totals.  Workgroup b >= 1: the boundary in front of entry b * kConfSpan; if a
// segment crosses it and this is the first boundary it crosses, the segment's sum = tail[b - 1] + head[b] + ... + head[last].
__global__ __launch_bounds__(kConfThreads) void conf_moments_finish_kernel(const int32_t* __restrict__ p, int n_seg, int n_spans,
                                                                           const double* __restrict__ part, double* __restrict__ out,
                                                                           double* __restrict__ total) {
  __shared__ double s_w[4];
  const int b = blockIdx.x;
  const double* src;
  int64_t cnt;
  double first = 0.0;
  double* dst;
  if (b == 0) {
    src = part + 2 * (size_t)n_spans; cnt = n_spans; dst = total;
  } else {
    const int64_t e = (int64_t)b * kConfSpan;
    const int r = conf_seg_of(p, 0, n_seg, e);
    const int64_t ps = (int64_t)p[r], pe = (int64_t)p[r + 1];
    if (ps >= e || ps < e - kConfSpan || pe <= e) return;   // begins at the boundary, or crossed an earlier one first
    const int64_t last = (pe - 1) / kConfSpan < n_spans ? (pe - 1) / kConfSpan : n_spans - 1;   // (p[n_seg] = nnz: never beyond)
    src = part + b; cnt = last - b + 1; dst = out + r;
    first = part[(size_t)n_spans + b - 1];
  }
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int64_t k = threadIdx.x;
  for (; k + 3 * kConfThreads < cnt; k += 4 * kConfThreads) {
    a0 = a0 + src[k]; a1 = a1 + src[k + kConfThreads]; a2 = a2 + src[k + 2 * kConfThreads]; a3 = a3 + src[k + 3 * kConfThreads];
  }
  for (; k < cnt; k += kConfThreads) a0 = a0 + src[k];
  const double tot = conf_block_sum((a0 + a1) + (a2 + a3), s_w);
  if (threadIdx.x == 0) *dst = first + tot;
}

__global__ __launch_bounds__(256) void conf_table_kernel(int table, int n, const int32_t* __restrict__ p, const double* __restrict__ moment,
                                                         const double* __restrict__ total, double a, double b, double c,
                                                         double* __restrict__ out) {
  const int stride = gridDim.x * blockDim.x;
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
    double o;
    if (table == RSPARSE_HIP_CONFIDENCE_TABLE_IDF) {
      o = log(a) - log1p((double)(p[r + 1] - p[r]));
    } else if (table == RSPARSE_HIP_CONFIDENCE_TABLE_BM25) {
      const double mean = total[0] / c;
      const double ratio = mean != 0.0 ? (b * moment[r]) / mean : b;
      o = a * ((1.0 - b) + ratio);
    } else {
      const double m = moment[r];
      const double nv = b == 2.0 ? sqrt(m) : m;
      o = nv != 0.0 ? pow(nv, a - 1.0) : 0.0;
    }
    out[r] = o;
  }
}

// the weighting itself: ONE function of (value, the user's table entry, the item's table entry) for both orientations
__device__ __forceinline__ double conf_f(int kind, double v, double ut, double it, double a, double b) {
  switch (kind) {
    case RSPARSE_HIP_CONFIDENCE_LINEAR: return 1.0 + a * v;
    case RSPARSE_HIP_CONFIDENCE_LOG: return 1.0 + a * log1p(v / b);
    case RSPARSE_HIP_CONFIDENCE_TFIDF: return sqrt(v) * it;
    case RSPARSE_HIP_CONFIDENCE_BM25: return ((v * (a + 1.0)) / (ut + v)) * it;
    default: return v * ut;   // NORMALIZE: the one table that was given arrives as `ut`
  }
}

template <class OutT>
__global__ __launch_bounds__(kConfThreads) void conf_apply_kernel(int kind, const int32_t* __restrict__ p, const int32_t* __restrict__ i,
                                                                  const double* x, int n_seg, int64_t nnz, int n_spans,
                                                                  const double* __restrict__ seg_table, const double* __restrict__ idx_table,
                                                                  int n_idx, int seg_is_item, double a, double b, OutT* out) {
  const int t = threadIdx.x;
  const bool aligned = (reinterpret_cast<uintptr_t>(x) & 15) == 0, aligned_i = (reinterpret_cast<uintptr_t>(i) & 15) == 0,
             aligned_o = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const int n_chunks = (n_spans + kConfChunk - 1) / kConfChunk;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
   const int64_t c_start = (int64_t)c * kConfChunk * kConfSpan;
   const int64_t c_end = c_start + kConfChunk * kConfSpan < nnz ? c_start + kConfChunk * kConfSpan : nnz;
   int r_lo = 0, r_hi = 1;
   if (seg_table) {
     r_lo = conf_seg_of(p, 0, n_seg, c_start);
     r_hi = conf_seg_of(p, 0, n_seg, c_end - 1) + 1;
   }
   const int s_end = (c + 1) * kConfChunk < n_spans ? (c + 1) * kConfChunk : n_spans;
   for (int s = c * kConfChunk; s < s_end; s++) {
    const int64_t start = (int64_t)s * kConfSpan, end = start + kConfSpan < nnz ? start + kConfSpan : nnz;
    const int64_t e0 = start + (int64_t)t * kConfPer;
    if (e0 >= end) continue;
    const bool full = e0 + kConfPer <= end;
    double v[kConfPer];
    conf_load4(x, e0, end, aligned, v);
    int r[kConfPer] = {kConfNoSeg, kConfNoSeg, kConfNoSeg, kConfNoSeg};
    if (seg_table) conf_rows(p, r_lo, r_hi, e0, end, r);
    int4 jj = make_int4(-1, -1, -1, -1);
    if (idx_table) {
      if (full && aligned_i) {
        jj = *reinterpret_cast<const int4*>(i + e0);
      } else {
        jj.x = i[e0];
        if (e0 + 1 < end) jj.y = i[e0 + 1];
        if (e0 + 2 < end) jj.z = i[e0 + 2];
        if (e0 + 3 < end) jj.w = i[e0 + 3];
      }
    }
    const int j[kConfPer] = {jj.x, jj.y, jj.z, jj.w};
    double w[kConfPer];
    double st_prev = 0.0;
#pragma unroll
    for (int q = 0; q < kConfPer; q++) {
      double st = 0.0, xt = 0.0;
      if (r[q] != kConfNoSeg) st = (q > 0 && r[q] == r[q - 1]) ? st_prev : seg_table[r[q]];
      st_prev = st;
      // (an index outside the table reads nothing and gives NaN)
      if (idx_table && e0 + q < end) xt = (unsigned)j[q] < (unsigned)n_idx ? idx_table[j[q]] : __builtin_nan("");
      double ut = seg_is_item ? xt : st;
      const double it = seg_is_item ? st : xt;
      if (kind == RSPARSE_HIP_CONFIDENCE_NORMALIZE) ut = seg_table ? st : xt;
      w[q] = conf_f(kind, v[q], ut, it, a, b);
    }
    if (full && aligned_o) {
      if constexpr (sizeof(OutT) == 8) {
        reinterpret_cast<double2*>(out + e0)[0] = make_double2(w[0], w[1]);
        reinterpret_cast<double2*>(out + e0)[1] = make_double2(w[2], w[3]);
      } else {
        *reinterpret_cast<float4*>(out + e0) = make_float4((float)w[0], (float)w[1], (float)w[2], (float)w[3]);
      }
    } else {
#pragma unroll
      for (int q = 0; q < kConfPer; q++)
        if (e0 + q < end) out[e0 + q] = (OutT)w[q];
    }
   }
  }
}

inline int conf_spans(int64_t nnz) { return (int)((nnz + kConfSpan - 1) / kConfSpan); }

}  // namespace

size_t confidence_ws_doubles(int64_t nnz) { return 3 * (size_t)conf_spans(nnz) + 1; }

hipError_t launch_confidence_moments(const int32_t* p, const double* x, int n_seg, int64_t nnz, int power, double* out, double* total,
                                     double* ws, hipStream_t s) {
  hipError_t e;
  if ((e = hipMemsetAsync(out, 0, (size_t)n_seg * sizeof(double), s)) != hipSuccess) return e;   // the empty segments
  if (nnz <= 0) return hipMemsetAsync(total, 0, sizeof(double), s);
  const int n_spans = conf_spans(nnz);
  const int n_chunks = (n_spans + kConfChunk - 1) / kConfChunk;
  hipLaunchKernelGGL(conf_moments_kernel, dim3(n_chunks < kConfGrid ? n_chunks : kConfGrid), dim3(kConfThreads), 0, s, p, x, n_seg, nnz,
                     power, n_spans, out, ws);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(conf_moments_finish_kernel, dim3(n_spans), dim3(kConfThreads), 0, s, p, n_seg, n_spans, (const double*)ws, out, total);
  return hipGetLastError();
}

hipError_t launch_confidence_table(int table, int n, const int32_t* p, const double* moment, const double* total, double a, double b,
                                   double c, double* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int grid = (n + 255) / 256;
  hipLaunchKernelGGL(conf_table_kernel, dim3(grid < 4096 ? grid : 4096), dim3(256), 0, s, table, n, p, moment, total, a, b, c, out);
  return hipGetLastError();
}

hipError_t launch_confidence_apply(int kind, const int32_t* p, const int32_t* i, const double* x, int n_seg, int64_t nnz,
                                   const double* seg_table, const double* idx_table, int n_idx, int seg_is_item, double a, double b,
                                   void* out, int out_float, hipStream_t s) {
  if (nnz <= 0) return hipSuccess;
  const int n_spans = conf_spans(nnz);
  const int n_chunks = (n_spans + kConfChunk - 1) / kConfChunk;
  const dim3 grid(n_chunks < kConfGrid ? n_chunks : kConfGrid), block(kConfThreads);
  if (out_float)
    hipLaunchKernelGGL(conf_apply_kernel<float>, grid, block, 0, s, kind, p, i, x, n_seg, nnz, n_spans, seg_table, idx_table, n_idx,
                       seg_is_item, a, b, static_cast<float*>(out));
  else
    hipLaunchKernelGGL(conf_apply_kernel<double>, grid, block, 0, s, kind, p, i, x, n_seg, nnz, n_spans, seg_table, idx_table, n_idx,
                       seg_is_item, a, b, static_cast<double*>(out));
  return hipGetLastError();
}

}  // namespace rsparse_hip
