// Negative sampling on the device: for every row of a CSR exclusion pattern, n items drawn uniformly WITHOUT replacement from the
// items outside the row, merged with the row's `keep` items -- the candidate rows of a sampled-metric evaluation (a held-out item
// against 99 / 999 negatives), handed to wrmf_candidates.hip without ever existing on the host.  gfx950, wave64, integers only.
//
// The stream is a FUNCTION of (seed, global row, exclusion list, n_item, n), not a state (rsparse_amd/rng.py is the same
// definition in numpy, include/rsparse_wrmf_hip.h states it for C hosts).  With seen = the row's sorted unique exclusion list,
// M = n_item - |seen| admissible items numbered by RANK 0 .. M - 1 in ascending item order:
//   item(r)   r + #{i : seen[i] - i <= r}                                  (a binary search: seen[i] - i does not decrease)
//   draw t    Philox4x32-10, key (lo32(seed), hi32(seed)), counter (lo32(t >> 1), g, 2, hi32(t >> 1)) -> o0..o3;
//             w = o1 2^32 + o0 (t even), o3 2^32 + o2 (t odd);  rank = (o_hi M + ((o_lo M) >> 32)) >> 32 = floor(w M / 2^64)
//   chosen    n >= M: every rank.  Otherwise d = min(n, M - n), D = the first d DISTINCT values of the draw sequence; the chosen
//             ranks are D when 2 n <= M and every rank but D otherwise
//   row       the ascending merge of keep and the items of the chosen ranks: |keep| + min(n, M) entries
// "The first d distinct values" does not depend on the order in which the draws are evaluated: a team evaluates 2 * BS of them
// at a time.
//
// Row pointers (sample_len_kernel, sample_scan_kernel, sample_offsets_kernel): out_p from seen_p, keep_p, n and n_item by a
// three-step scan in 64 bits; the first step also flags pointers that are negative or decrease, a seen row longer than n_item
// and a keep row longer than its seen row.  The host reads back the total and the flag and refuses before anything is sampled.
//
// sample_kernel<BS>, one team of BS threads per row (BS = 64, one wave, for n <= kSampleShort; 256 beyond), LDS: tr[T] ranks,
// ti[T] first draw indices, T = the power of two at or above 2 (n + 2 BS), at most 16384 (128 KiB; load <= 0.54 at d = 8192):
//   1. draw: a thread makes ONE Philox call per round and takes its two draws, t = base + 2 tid and t + 1 (the whole output of
//      a call is used).  Every rank goes into the open-addressing table (linear probing from rank & (T - 1); ranks are uniform):
//      an atomic compare-and-swap claims or finds the slot, an atomic min keeps the SMALLEST draw index of the rank -- both
//      order-free.  A draw is a first occurrence iff the slot holds its own index afterwards; a prefix sum over the draws in
//      index order counts them.  The round in which the count reaches d is the last: the draw index t_cut of the d-th distinct
//      value is read off the prefix, and the table's entries with a first index <= t_cut are exactly D (everything dropped comes
//      from the last round).  d <= M / 2, so every draw is new with probability >= 1/2: rounds are capped at a number that d
//      successes miss with probability below 2^-300 (a cap, so that no input can make a team spin).
//   2. compact D into the front of ti (a slot is written only after it was read: the target never passes the source), pad to a
//      power of two and sort it ascending (bitonic, LDS).
//   3. write: with D sorted, the j-th chosen rank is D[j] (direct) or j + #{i : D[i] - i <= j} (complement: the same map as
//      item(r)); its item by the binary search over the seen row in global memory (L2; nothing of seen is staged, so its length
//      is unbounded); its place j + #{keep < item}.  A keep item k with s = its index in seen has rank-position q = k - s and goes
//      to its own index + #{chosen ranks < q} = lower_bound(D, q) or q - lower_bound(D, q).  Every place lies in
//      [0, |keep| + min(n, M)) whatever the lists hold: a keep row that is no subset of seen gives a wrong row, never a write
//      outside it.
// No float arithmetic, no atomic whose order matters: a call repeats bit for bit and a row does not depend on the rows around it.
#include <algorithm>

#include "wrmf_internal.h"
#include "wrmf_device.h"
#include "wrmf_sample_team.h"

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kSampleShort = 64;     // n up to this: a wave per row
constexpr int kSampleMaxTable = 16384;
constexpr unsigned kEmpty = 0xffffffffu;

// ---- row pointers ---------------------------------------------------------------------------------------------------------------
// out_p[row + 1] = the row's length for now; bsum[block] = the block's sum; *flag != 0: an input the library refuses
__global__ __launch_bounds__(256) void sample_len_kernel(const int32_t* __restrict__ seen_p, const int32_t* __restrict__ keep_p,
                                                         int n_rows, int n_item, int n, int32_t* __restrict__ out_p,
                                                         long long* __restrict__ bsum, int* __restrict__ flag) {
  __shared__ long long sw[4];
  const int row = blockIdx.x * 256 + threadIdx.x;
  long long len = 0;
  if (row < n_rows) {
    const int s0 = seen_p[row], s1 = seen_p[row + 1];
    bool bad = s0 < 0 || s1 < s0 || s1 - s0 > n_item;
    int K = 0;
    if (keep_p) {
      const int k0 = keep_p[row], k1 = keep_p[row + 1];
      bad = bad || k0 < 0 || k1 < k0 || k1 - k0 > s1 - s0;
      K = k1 - k0;
    }
    if (bad) atomicOr(flag, 1);
    else len = (long long)K + min(n, n_item - (s1 - s0));
    out_p[row + 1] = (int32_t)len;
  }
  long long tot;
  team_scan<256>(len, sw, &tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// boff[b] = the sum of bsum[0, b); *total = the sum of all (one workgroup)
__global__ __launch_bounds__(256) void sample_scan_kernel(const long long* __restrict__ bsum, int nb, long long* __restrict__ boff,
                                                          long long* __restrict__ total) {
  __shared__ long long sw[4];
  long long carry = 0;
  for (int c0 = 0; c0 < nb; c0 += 256) {
    const int b = c0 + threadIdx.x;
    const long long v = b < nb ? bsum[b] : 0;
    long long tot;
    const long long off = team_scan<256>(v, sw, &tot);
    if (b < nb) boff[b] = carry + off;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(256) void sample_offsets_kernel(int n_rows, const long long* __restrict__ boff, int32_t* __restrict__ out_p) {
  __shared__ long long sw[4];
  const int row = blockIdx.x * 256 + threadIdx.x;
  const long long len = row < n_rows ? out_p[row + 1] : 0;
  long long tot;
  const long long off = team_scan<256>(len, sw, &tot);
  if (row < n_rows) out_p[row + 1] = (int32_t)(boff[blockIdx.x] + off + len);   // (a total past int32 is refused by the host)
  if (row == 0) out_p[0] = 0;
}

// ---- the rows ---------------------------------------------------------------------------------------------------------------------
// the rank of draw t (a 32-bit draw index: hi32(t >> 1) = 0) and of draw t + 1, t even, of global row g among M items
__device__ __forceinline__ void draw_pair(unsigned t, unsigned g, unsigned k0, unsigned k1, unsigned M, unsigned& r0, unsigned& r1) {
  unsigned o[4];
  philox4x32_10(t >> 1, g, 2u, 0u, k0, k1, o);
  r0 = (unsigned)(((u64)o[1] * M + (((u64)o[0] * M) >> 32)) >> 32);
  r1 = (unsigned)(((u64)o[3] * M + (((u64)o[2] * M) >> 32)) >> 32);
}

// rank r, drawn as draw t, into the table -> its slot
__device__ __forceinline__ unsigned table_insert(unsigned* tr, unsigned* ti, unsigned mask, unsigned r, unsigned t) {
  unsigned h = r & mask;
  for (;;) {   // (fewer entries than slots: an empty slot exists)
    const unsigned old = atomicCAS(&tr[h], kEmpty, r);
    if (old == kEmpty || old == r) break;
    h = (h + 1) & mask;
  }
  atomicMin(&ti[h], t);
  return h;
}

template <int BS>
__global__ __launch_bounds__(BS) void sample_kernel(unsigned k0, unsigned k1, unsigned g0, int n_item, int n,
                                                    const int32_t* __restrict__ seen_p, const int32_t* __restrict__ seen_j,
                                                    const int32_t* __restrict__ keep_p, const int32_t* __restrict__ keep_j,
                                                    const int32_t* __restrict__ out_p, int32_t* __restrict__ out_j, int T) {
  extern __shared__ __attribute__((aligned(16))) unsigned smem_sample[];
  unsigned* tr = smem_sample;
  unsigned* ti = smem_sample + T;
  int* sw = reinterpret_cast<int*>(ti + T);   // [4] team_scan, [4] t_cut
  const int tid = threadIdx.x;
  const int row = blockIdx.x;
  const int s0 = seen_p[row], S = seen_p[row + 1] - s0;
  const int kb = keep_p ? keep_p[row] : 0, K = keep_p ? keep_p[row + 1] - kb : 0;
  const int32_t* seen = seen_j + s0;
  const int32_t* keep = keep_j + kb;   // (not read when K == 0)
  const int M = max(n_item - S, 0);
  const int cnt = min(n, M);
  const bool direct = 2 * n <= M;
  const int d = direct ? n : max(M - n, 0);   // the distinct ranks to draw: <= n, and <= M / 2
  if (d > 0) {
    // 1. the first d distinct ranks of the draw sequence
    const int Tr = min(T, pow2_at_least(2 * (d + 2 * BS)));   // (a multiple of BS; more slots than d - 1 + 2 BS entries)
    const unsigned mask = (unsigned)Tr - 1u;
    for (int e = tid; e < Tr; e += BS) {
      tr[e] = kEmpty;
      ti[e] = kEmpty;
    }
    __syncthreads();
    const unsigned g = g0 + (unsigned)row;
    const int max_rounds = (64 * d + 1024) / (2 * BS) + 4;
    int have = 0;
    unsigned t_cut = kEmpty;
    for (int round = 0; round < max_rounds; round++) {
      const unsigned t0 = (unsigned)round * (2u * BS) + 2u * (unsigned)tid;
      unsigned r0, r1;
      draw_pair(t0, g, k0, k1, (unsigned)M, r0, r1);
      const unsigned h0 = table_insert(tr, ti, mask, r0, t0);
      const unsigned h1 = table_insert(tr, ti, mask, r1, t0 + 1u);
      __syncthreads();
      const int f0 = ti[h0] == t0 ? 1 : 0, f1 = ti[h1] == t0 + 1u ? 1 : 0;   // first occurrences (in this round: new ranks)
      int tot;
      const int off = team_scan<BS>(f0 + f1, sw, &tot);
      if (have + tot >= d) {   // (uniform) the d-th distinct value is drawn in this round
        const int need = d - have;   // its number among the round's new ranks, from 1
        if (f0 && off + 1 == need) sw[4] = (int)t0;
        if (f1 && off + f0 + 1 == need) sw[4] = (int)(t0 + 1u);
        __syncthreads();
        t_cut = (unsigned)sw[4];
        break;
      }
      have += tot;
    }
    // 2. D = the entries first drawn up to t_cut, compacted into ti[0, d) and sorted
    int dst0 = 0;
    for (int c0 = 0; c0 < Tr; c0 += BS) {
      const int e = c0 + tid;
      const unsigned r = tr[e];
      const bool kept = r != kEmpty && t_cut != kEmpty && ti[e] <= t_cut;
      int tot;
      const int off = team_scan<BS>(kept ? 1 : 0, sw, &tot);   // (its barriers put every read of this chunk before the writes)
      if (kept && dst0 + off < d) ti[dst0 + off] = r;          // (dst0 + off <= e; < d by construction)
      dst0 += tot;
    }
    const int P = pow2_at_least(d);   // <= Tr / 2
    for (int e = min(dst0, d) + tid; e < P; e += BS) ti[e] = kEmpty;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int i = tid; i < P / 2; i += BS) {
          const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
          const unsigned a = ti[lo], b = ti[hi];
          if ((a > b) == ((lo & size) == 0)) {
            ti[lo] = b;
            ti[hi] = a;
          }
        }
        __syncthreads();
      }
  }
  // 3. the row: chosen items and keep items, each to its place in the ascending merge
  const unsigned* D = ti;
  int32_t* out = out_j + out_p[row];
  for (int j = tid; j < cnt; j += BS) {
    const int r = direct ? (int)D[j] : j + count_shifted_le(D, d, j);
    const int item = r + count_shifted_le(seen, S, r);
    out[j + count_less(keep, K, item)] = item;
  }
  for (int k = tid; k < K; k += BS) {
    const int kv = keep[k];
    const int q = kv - count_less(seen, S, kv);   // the admissible items below kv
    const int lb = count_less(D, d, q);
    out[k + min(max(direct ? lb : q - lb, 0), cnt)] = kv;
  }
}

int pow2_host(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

}  // namespace

size_t sample_negatives_ws_bytes(int n_rows) {
  const size_t nb = ((size_t)std::max(n_rows, 0) + 255) / 256;
  return 2 * nb * 8 + sizeof(SampleStatus);
}

hipError_t launch_row_pointer_scan(int n_rows, const long long* bsum, long long* boff, long long* total, int32_t* out_p, hipStream_t s) {
  const int nb = (n_rows + 255) / 256;
  hipLaunchKernelGGL(sample_scan_kernel, dim3(1), dim3(256), 0, s, bsum, nb, boff, total);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(sample_offsets_kernel, dim3((unsigned)nb), dim3(256), 0, s, n_rows, boff, out_p);
  return hipGetLastError();
}

hipError_t launch_sample_row_pointers(int n_rows, int n_item, int n, const int32_t* seen_p, const int32_t* keep_p, int32_t* out_p,
                                      void* ws, SampleStatus** d_status, hipStream_t s) {
  const int nb = (n_rows + 255) / 256;
  long long* bsum = static_cast<long long*>(ws);
  long long* boff = bsum + nb;
  SampleStatus* st = reinterpret_cast<SampleStatus*>(boff + nb);
  long long* total = &st->total;
  int* flag = &st->flag;
  *d_status = st;
  hipError_t err;
  if ((err = hipMemsetAsync(st, 0, sizeof(SampleStatus), s)) != hipSuccess) return err;
  hipLaunchKernelGGL(sample_len_kernel, dim3((unsigned)nb), dim3(256), 0, s, seen_p, keep_p, n_rows, n_item, n, out_p, bsum, flag);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  return launch_row_pointer_scan(n_rows, bsum, boff, total, out_p, s);
}

template <int BS>
static hipError_t launch_sample_rows(unsigned k0, unsigned k1, unsigned g0, int n_rows, int n_item, int n, const int32_t* seen_p,
                                     const int32_t* seen_j, const int32_t* keep_p, const int32_t* keep_j, const int32_t* out_p,
                                     int32_t* out_j, hipStream_t s) {
  const int T = std::min(kSampleMaxTable, pow2_host(2 * (n + 2 * BS)));
  const size_t lds = (size_t)T * 8 + 8 * sizeof(int);
  hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(sample_kernel<BS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(sample_kernel<BS>, dim3((unsigned)n_rows), dim3(BS), lds, s, k0, k1, g0, n_item, n, seen_p, seen_j, keep_p, keep_j,
                     out_p, out_j, T);
  return hipGetLastError();
}

hipError_t launch_sample_negatives(uint64_t seed, int64_t row0, int n_rows, int n_item, int n, const int32_t* seen_p,
                                   const int32_t* seen_j, const int32_t* keep_p, const int32_t* keep_j, const int32_t* out_p,
                                   int32_t* out_j, hipStream_t s) {
  if (n_rows <= 0) return hipSuccess;
  if (n < 1 || n > kSampleMaxNegatives || n_item < 0 || row0 < 0 || row0 + n_rows > (1ll << 32)) return hipErrorInvalidValue;
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), g0 = (unsigned)row0;
  return n <= kSampleShort ? launch_sample_rows<64>(k0, k1, g0, n_rows, n_item, n, seen_p, seen_j, keep_p, keep_j, out_p, out_j, s)
                           : launch_sample_rows<256>(k0, k1, g0, n_rows, n_item, n, seen_p, seen_j, keep_p, keep_j, out_p, out_j, s);
}

}  // namespace rsparse_hip
