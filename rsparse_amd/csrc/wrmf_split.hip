// Train / test split of a CSR interaction matrix on the device: every stored entry of every row goes to exactly one of two output
// matrices, in its order, with its index and (uninterpreted) value.  gfx950, wave64, integers only.
//
// The split is a FUNCTION of (seed, global row g, position t in the row, the mode's parameters), not a state (rsparse_amd/rng.py
// split_flags is the same definition in numpy, include/rsparse_wrmf_hip.h states it for C hosts):
//   proportion   Philox4x32-10, key (lo32(seed), hi32(seed)), counter (t >> 2, g, 3, 0) -> o0..o3; TEST iff o[t & 3] < T in 64
//                bits, T = floor(p 2^32) in [0, 2^32]
//   leave-out    the h = min(n, max(L - min_train, 0)) first entries of the order "w_a > w_b, or w_a = w_b and t_a < t_b" are test
//     random     counter (t >> 1, g, 4, 0); w = o1 2^32 + o0 (t even), o3 2^32 + o2 (t odd)
//     by         w = the order key of the entry's float64 (f64_key: -0.0 just below +0.0); no random word
//
// Three steps, nothing entry-sized in a workspace:
//   1. count (split_count_wave_kernel, split_count_team_kernel): the row's test count into test_p[row + 1] and, in leave-out mode,
//      (w*, q) into a 16-byte record: w* = the h-th key of the order, q = how many entries EQUAL to w* are test (the first q by
//      position); an entry is then test iff w > w*, or w = w* and fewer than q equal keys precede it.  h = 0 is (2^64 - 1, 0) and
//      h = L is (0, L), so that the same rule holds without a select.
//        L <= kSplitWaveRow (256)   a wave per row, four rows per workgroup: a lane holds the keys of four consecutive positions
//                                   (one Philox call serves four flags or two keys) and the wave finds w* bit by bit from the top:
//                                   64 steps of "how many keys are >= prefix | bit" by ballot
//        L <= kSplitLdsRow (4096)   a workgroup per row: the keys are staged once in LDS, then block_kth_largest (wrmf_device.h),
//                                   the 8-bit-digit radix select the top-k kernels use, on 64 bits
//        longer rows                the same select with the keys recomputed (Philox) or re-read (`by`) in each of its 8 passes
//      The workgroups of the team kernel stride over the rows and skip the short ones.
//   2. row pointers: split_len_kernel validates p (negative or decreasing -> flag), derives the train lengths and sums both per
//      256 rows; the scan is wrmf_sample.hip's (launch_row_pointer_scan), once per output.  The host reads totals and flag back
//      and refuses before step 3.
//   3. compaction (split_write_wave_kernel, split_write_team_kernel; the same two row classes): a wave takes 256 positions, makes
//      their flags four per lane, hands them over to the lane order (position = chunk + 64 k + lane: a shuffle per k), and places
//      every entry by ballot + mbcnt prefix counts with the row's running test count as carry: test entry -> test_p[row] + tests
//      before it, train entry -> train_p[row] + position - tests before it.  Loads and stores are coalesced per 64 entries; indices
//      move as int32, values as opaque 4- or 8-byte words.  The four waves of a team take consecutive chunks and exchange their
//      counts through LDS.  A long row is handled by ONE workgroup (its four waves): rows are not split over workgroups.
// No float arithmetic, no atomic on an output position: the layout comes from the scan and a call repeats bit for bit.
#include <algorithm>

#include "wrmf_internal.h"
#include "wrmf_device.h"

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kSplitWaveRow = 256;    // rows up to this: a wave per row (four positions per lane)
constexpr int kSplitLdsRow = 4096;    // leave-out rows up to this stage their keys in LDS (32 KiB)
constexpr int kSplitMaxTeams = 4096;  // workgroups of the team kernels (they stride over the rows)
enum { kProp = 0, kRand = 1, kBy = 2 };

struct SplitArgs {
  unsigned k0, k1, g0;
  int n_rows;
  u64 T;
  int n, min_train;
  const int32_t* p;
  const double* by;
};
struct SplitRow {   // step 1's result of a leave-out row
  u64 wstar;
  int q, pad;
};
struct SplitIO {
  const int32_t* j;
  const void* v;
  int vb;
  const int32_t *train_p, *test_p;
  int32_t *train_j, *test_j;
  void *train_v, *test_v;
  const SplitRow* rows;
};

__device__ __forceinline__ int mbcnt(u64 m) {   // the set bits of m below this lane
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
// bit j set: position t + j lies in the row
__device__ __forceinline__ unsigned valid4(long long t, int L) {
  return t + 3 < L ? 15u : t < L ? (1u << (int)(L - t)) - 1u : 0u;
}
// the row's length, 0 for pointers that split_len_kernel refuses
__device__ __forceinline__ int row_len(int p0, int p1) { return (p0 < 0 || p1 < p0) ? 0 : p1 - p0; }
__device__ __forceinline__ int held_out(const SplitArgs& a, int L) { return min(a.n, max(L - a.min_train, 0)); }

// proportion mode: the test bits of positions t .. t + 3 (t a multiple of 4)
__device__ __forceinline__ unsigned prop_bits(const SplitArgs& a, unsigned g, unsigned t) {
  unsigned o[4];
  philox4x32_10(t >> 2, g, 3u, 0u, a.k0, a.k1, o);
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) m |= ((u64)o[j] < a.T ? 1u : 0u) << j;
  return m;
}
// leave-out mode: the keys of positions t .. t + 3 (t a multiple of 4; vm = valid4: `by` is read inside the row only)
template <int MODE>
__device__ __forceinline__ void keys4(const SplitArgs& a, unsigned g, const double* byrow, long long t, unsigned vm, u64 (&w)[4]) {
  if constexpr (MODE == kRand) {
    unsigned o[4];
    philox4x32_10((unsigned)(t >> 1), g, 4u, 0u, a.k0, a.k1, o);
    w[0] = ((u64)o[1] << 32) | o[0];
    w[1] = ((u64)o[3] << 32) | o[2];
    philox4x32_10((unsigned)(t >> 1) + 1u, g, 4u, 0u, a.k0, a.k1, o);
    w[2] = ((u64)o[1] << 32) | o[0];
    w[3] = ((u64)o[3] << 32) | o[2];
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) w[j] = ((vm >> j) & 1u) ? f64_key(byrow[t + j]) : 0ull;
  }
}
template <int MODE>
__device__ __forceinline__ u64 key1(const SplitArgs& a, unsigned g, const double* byrow, int t) {
  if constexpr (MODE == kRand) {
    unsigned o[4];
    philox4x32_10((unsigned)t >> 1, g, 4u, 0u, a.k0, a.k1, o);
    return (t & 1) ? (((u64)o[3] << 32) | o[2]) : (((u64)o[1] << 32) | o[0]);
  } else {
    return f64_key(byrow[t]);
  }
}

// ---- step 1 -----------------------------------------------------------------------------------------------------------------------
// rows of at most kSplitWaveRow entries, a wave each (no barrier in this kernel: the waves of a workgroup go their own ways)
template <int MODE>
__global__ __launch_bounds__(256) void split_count_wave_kernel(SplitArgs a, int32_t* __restrict__ test_p, SplitRow* __restrict__ rows) {
  const int lane = threadIdx.x & 63;
  const long long row64 = (long long)blockIdx.x * 4 + rfl((int)(threadIdx.x >> 6));
  if (row64 >= a.n_rows) return;
  const int row = (int)row64;
  const int L = row_len(a.p[row], a.p[row + 1]);
  if (L > kSplitWaveRow) return;
  const unsigned g = a.g0 + (unsigned)row;
  const long long t = 4 * lane;
  const unsigned vm = valid4(t, L);
  if constexpr (MODE == kProp) {
    const unsigned m = vm ? (prop_bits(a, g, (unsigned)t) & vm) : 0u;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) cnt += __popcll(__ballot((m >> j) & 1u));
    if (lane == 0) test_p[row + 1] = cnt;
  } else {
    const int h = held_out(a, L);
    u64 wstar = ~0ull;
    int q = 0;
    if (h >= L) {
      wstar = 0ull;
      q = L;
    } else if (h > 0) {
      u64 w[4] = {0ull, 0ull, 0ull, 0ull};
      if (vm) keys4<MODE>(a, g, a.by + a.p[row], t, vm, w);
      u64 prefix = 0ull;
      for (int b = 63; b >= 0; b--) {   // the largest value that at least h keys reach: the h-th largest key
        const u64 cand = prefix | (1ull << b);
        int c = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) c += __popcll(__ballot(((vm >> j) & 1u) && w[j] >= cand));
        if (c >= h) prefix = cand;
      }
      int gt = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) gt += __popcll(__ballot(((vm >> j) & 1u) && w[j] > prefix));
      wstar = prefix;
      q = h - gt;
    }
    if (lane == 0) {
      test_p[row + 1] = h;
      rows[row].wstar = wstar;
      rows[row].q = q;
      rows[row].pad = 0;
    }
  }
}

// longer rows, a workgroup each
template <int MODE>
__global__ __launch_bounds__(256) void split_count_team_kernel(SplitArgs a, int32_t* __restrict__ test_p, SplitRow* __restrict__ rows) {
  __shared__ u64 skeys[MODE == kProp ? 1 : kSplitLdsRow];
  __shared__ unsigned hist[256];
  __shared__ u64 sres;
  __shared__ int srem;
  __shared__ int sw[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (long long row64 = blockIdx.x; row64 < a.n_rows; row64 += gridDim.x) {
    const int row = (int)row64;
    const int p0 = a.p[row];
    const int L = row_len(p0, a.p[row + 1]);
    if (L <= kSplitWaveRow) continue;   // (uniform over the workgroup)
    const unsigned g = a.g0 + (unsigned)row;
    if constexpr (MODE == kProp) {
      int c = 0;
      for (long long t = 4 * tid; t < L; t += 1024) c += __popc(prop_bits(a, g, (unsigned)t) & valid4(t, L));
      c = butterfly_sum(c);
      if (lane == 0) sw[wv] = c;
      __syncthreads();
      if (tid == 0) test_p[row + 1] = sw[0] + sw[1] + sw[2] + sw[3];
      __syncthreads();
    } else {
      const int h = held_out(a, L);
      u64 wstar = ~0ull;
      int q = 0;
      if (h >= L) {
        wstar = 0ull;
        q = L;
      } else if (h > 0) {
        const double* byrow = a.by + p0;
        if (L <= kSplitLdsRow) {
          for (long long t = 4 * tid; t < L; t += 1024) {
            const unsigned vm = valid4(t, L);
            u64 w[4];
            keys4<MODE>(a, g, byrow, t, vm, w);
#pragma unroll
            for (int j = 0; j < 4; j++)
              if ((vm >> j) & 1u) skeys[t + j] = w[j];
          }
          __syncthreads();
          wstar = block_kth_largest(L, h, 64, [&](int e, bool& ok) { ok = true; return skeys[e]; }, hist, &sres, &srem);
        } else {
          wstar = block_kth_largest(L, h, 64, [&](int e, bool& ok) { ok = true; return key1<MODE>(a, g, byrow, e); }, hist, &sres, &srem);
        }
        q = srem;   // what is left of h below the keys above w*: 1 .. the number of keys equal to w*
        __syncthreads();   // (every read of skeys / srem before the next row's writes)
      }
      if (tid == 0) {
        test_p[row + 1] = h;
        rows[row].wstar = wstar;
        rows[row].q = q;
        rows[row].pad = 0;
      }
    }
  }
}

// ---- step 2 -----------------------------------------------------------------------------------------------------------------------
// test_p[row + 1] holds the test count: train_p[row + 1] = the rest of the row; the sums of both over the block's 256 rows;
// *flag != 0: row pointers that are negative or decrease
__global__ __launch_bounds__(256) void split_len_kernel(const int32_t* __restrict__ p, int n_rows, int32_t* __restrict__ train_p,
                                                        int32_t* __restrict__ test_p, long long* __restrict__ bsum_train,
                                                        long long* __restrict__ bsum_test, int* __restrict__ flag) {
  __shared__ long long sw[8];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  long long tr = 0, te = 0;
  if (row < n_rows) {
    const int p0 = p[row], p1 = p[row + 1];
    if (p0 < 0 || p1 < p0) {
      atomicOr(flag, 1);
      test_p[row + 1] = 0;
    } else {
      te = min(max(test_p[row + 1], 0), p1 - p0);
      tr = (long long)(p1 - p0) - te;
    }
    train_p[row + 1] = (int32_t)tr;
  }
  tr = butterfly_sum(tr);
  te = butterfly_sum(te);
  if (lane == 0) {
    sw[wv] = tr;
    sw[4 + wv] = te;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    bsum_train[blockIdx.x] = (sw[0] + sw[1]) + (sw[2] + sw[3]);
    bsum_test[blockIdx.x] = (sw[4] + sw[5]) + (sw[6] + sw[7]);
  }
}

// ---- step 3 -----------------------------------------------------------------------------------------------------------------------
// One row by NW waves (NW = 1: this wave alone, no barrier; NW = 4: the workgroup, every thread calls it).  sx: 4 ints of LDS.
template <int MODE, int NW>
__device__ __forceinline__ void split_write_row(const SplitArgs& a, const SplitIO& io, int row, int p0, int L, int wv, int lane, int* sx) {
  const unsigned g = a.g0 + (unsigned)row;
  const int tr_row = io.train_p[row], te_row = io.test_p[row];
  u64 wstar = 0ull;
  int q = 0;
  if constexpr (MODE != kProp) {
    wstar = io.rows[row].wstar;
    q = io.rows[row].q;
  }
  const double* byrow = MODE == kBy ? a.by + p0 : nullptr;
  int te_rel = 0;   // the row's test entries before this round's positions
  int eqc = 0;      // its keys equal to w* before them
  for (long long base = 0; base < L; base += 256 * NW) {
    const long long t0 = base + 256 * wv;   // this wave's 256 positions (none of them in the row for a late wave of the last round)
    const long long t = t0 + 4 * lane;
    const unsigned vm = valid4(t, L);
    unsigned m = 0;   // bit j: position t + j is test
    if constexpr (MODE == kProp) {
      if (vm) m = prop_bits(a, g, (unsigned)t) & vm;
    } else {
      unsigned eq = 0;
      if (vm) {
        u64 w[4];
        keys4<MODE>(a, g, byrow, t, vm, w);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          m |= (w[j] > wstar ? 1u : 0u) << j;
          eq |= (w[j] == wstar ? 1u : 0u) << j;
        }
        m &= vm;
        eq &= vm;
      }
      int below = 0, tot = 0;   // equal keys in the lanes below, and in the wave
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const u64 b = __ballot((eq >> j) & 1u);
        below += mbcnt(b);
        tot += __popcll(b);
      }
      int woff = 0, all = tot;
      if constexpr (NW > 1) {
        if (lane == 0) sx[wv] = tot;
        __syncthreads();
        all = 0;
        for (int w = 0; w < NW; w++) {
          if (w < wv) woff += sx[w];
          all += sx[w];
        }
        __syncthreads();
      }
      int r = eqc + woff + below;   // the number of equal keys before this lane's first
#pragma unroll
      for (int j = 0; j < 4; j++)
        if ((eq >> j) & 1u) {
          if (r < q) m |= 1u << j;
          r++;
        }
      eqc += all;
    }
    // from four positions per lane to the lane order: position t0 + 64 k + lane is bit (lane & 3) of lane 16 k + lane / 4
    u64 bt[4];
    int cte = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const unsigned mm = (unsigned)__shfl((int)m, 16 * k + (lane >> 2));
      bt[k] = __ballot(((mm >> (lane & 3)) & 1u) != 0u);   // (bits of positions outside the row are clear)
      cte += __popcll(bt[k]);
    }
    int before = te_rel, all_te = cte;
    if constexpr (NW > 1) {
      if (lane == 0) sx[wv] = cte;
      __syncthreads();
      all_te = 0;
      for (int w = 0; w < NW; w++) {
        if (w < wv) before += sx[w];
        all_te += sx[w];
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const long long tp = t0 + 64 * k + lane;
      const int nb = before + mbcnt(bt[k]);   // the row's test entries before position tp
      if (tp < L) {
        const bool f = (bt[k] >> lane) & 1ull;
        const long long src = (long long)p0 + tp;
        const long long dst = f ? (long long)te_row + nb : (long long)tr_row + (tp - nb);
        (f ? io.test_j : io.train_j)[dst] = io.j[src];
        if (io.vb == 4) static_cast<unsigned*>(f ? io.test_v : io.train_v)[dst] = static_cast<const unsigned*>(io.v)[src];
        else if (io.vb == 8) static_cast<u64*>(f ? io.test_v : io.train_v)[dst] = static_cast<const u64*>(io.v)[src];
      }
      before += __popcll(bt[k]);
    }
    te_rel += all_te;
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void split_write_wave_kernel(SplitArgs a, SplitIO io) {
  const int lane = threadIdx.x & 63;
  const long long row64 = (long long)blockIdx.x * 4 + rfl((int)(threadIdx.x >> 6));
  if (row64 >= a.n_rows) return;
  const int row = (int)row64;
  const int p0 = a.p[row];
  const int L = row_len(p0, a.p[row + 1]);
  if (L > kSplitWaveRow) return;
  split_write_row<MODE, 1>(a, io, row, p0, L, 0, lane, nullptr);
}

template <int MODE>
__global__ __launch_bounds__(256) void split_write_team_kernel(SplitArgs a, SplitIO io) {
  __shared__ int sx[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (long long row64 = blockIdx.x; row64 < a.n_rows; row64 += gridDim.x) {
    const int row = (int)row64;
    const int p0 = a.p[row];
    const int L = row_len(p0, a.p[row + 1]);
    if (L <= kSplitWaveRow) continue;   // (uniform over the workgroup)
    split_write_row<MODE, 4>(a, io, row, p0, L, wv, lane, sx);
  }
}

struct SplitWs {
  SplitRow* rows;
  long long *bsum_train, *bsum_test, *boff;
  SplitStatus* st;
};
SplitWs split_ws(void* ws, int n_rows) {
  const size_t nb = ((size_t)n_rows + 255) / 256;
  SplitWs w;
  w.rows = static_cast<SplitRow*>(ws);
  w.bsum_train = reinterpret_cast<long long*>(w.rows + n_rows);
  w.bsum_test = w.bsum_train + nb;
  w.boff = w.bsum_test + nb;
  w.st = reinterpret_cast<SplitStatus*>(w.boff + nb);
  return w;
}

SplitArgs split_args(uint64_t seed, int64_t row0, int n_rows, uint64_t threshold, int leave_out, int min_train, const int32_t* p,
                     const double* by) {
  SplitArgs a;
  a.k0 = (unsigned)seed;
  a.k1 = (unsigned)(seed >> 32);
  a.g0 = (unsigned)row0;
  a.n_rows = n_rows;
  a.T = threshold;
  a.n = leave_out;
  a.min_train = min_train;
  a.p = p;
  a.by = by;
  return a;
}

bool split_args_ok(int64_t row0, int n_rows, int mode, uint64_t threshold, int leave_out, int min_train, const double* by) {
  if (row0 < 0 || row0 + n_rows > (1ll << 32)) return false;
  if (mode == 0) return threshold <= (1ull << 32) && !by;
  return mode == 1 && leave_out >= 1 && min_train >= 0;
}

}  // namespace

size_t split_ws_bytes(int n_rows) {
  const size_t nb = ((size_t)std::max(n_rows, 0) + 255) / 256;
  return (size_t)std::max(n_rows, 0) * sizeof(SplitRow) + 3 * nb * 8 + sizeof(SplitStatus);
}

hipError_t launch_split_count(uint64_t seed, int64_t row0, int n_rows, int mode, uint64_t threshold, int leave_out, int min_train,
                              const int32_t* p, const double* by, int32_t* train_p, int32_t* test_p, void* ws, SplitStatus** d_status,
                              hipStream_t s) {
  if (n_rows <= 0 || !split_args_ok(row0, n_rows, mode, threshold, leave_out, min_train, by)) return hipErrorInvalidValue;
  const SplitWs w = split_ws(ws, n_rows);
  *d_status = w.st;
  const SplitArgs a = split_args(seed, row0, n_rows, threshold, leave_out, min_train, p, by);
  const unsigned wave_grid = (unsigned)(((long long)n_rows + 3) / 4), team_grid = (unsigned)std::min(n_rows, kSplitMaxTeams);
  const int nb = (n_rows + 255) / 256;
  hipError_t err;
  if ((err = hipMemsetAsync(w.st, 0, sizeof(SplitStatus), s)) != hipSuccess) return err;
  auto count = [&](auto wave_k, auto team_k) {
    hipLaunchKernelGGL(wave_k, dim3(wave_grid), dim3(256), 0, s, a, test_p, w.rows);
    hipLaunchKernelGGL(team_k, dim3(team_grid), dim3(256), 0, s, a, test_p, w.rows);
  };
  if (mode == 0) count(split_count_wave_kernel<kProp>, split_count_team_kernel<kProp>);
  else if (by) count(split_count_wave_kernel<kBy>, split_count_team_kernel<kBy>);
  else count(split_count_wave_kernel<kRand>, split_count_team_kernel<kRand>);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  hipLaunchKernelGGL(split_len_kernel, dim3((unsigned)nb), dim3(256), 0, s, p, n_rows, train_p, test_p, w.bsum_train, w.bsum_test, &w.st->flag);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  if ((err = launch_row_pointer_scan(n_rows, w.bsum_train, w.boff, &w.st->total_train, train_p, s)) != hipSuccess) return err;
  return launch_row_pointer_scan(n_rows, w.bsum_test, w.boff, &w.st->total_test, test_p, s);
}

hipError_t launch_split_write(uint64_t seed, int64_t row0, int n_rows, int mode, uint64_t threshold, int leave_out, int min_train,
                              const int32_t* p, const int32_t* j, const void* v, int value_bytes, const double* by,
                              const int32_t* train_p, int32_t* train_j, void* train_v, const int32_t* test_p, int32_t* test_j,
                              void* test_v, void* ws, hipStream_t s) {
  if (n_rows <= 0 || !split_args_ok(row0, n_rows, mode, threshold, leave_out, min_train, by)) return hipErrorInvalidValue;
  if (value_bytes != 0 && value_bytes != 4 && value_bytes != 8) return hipErrorInvalidValue;
  const SplitWs w = split_ws(ws, n_rows);
  const SplitArgs a = split_args(seed, row0, n_rows, threshold, leave_out, min_train, p, by);
  SplitIO io;
  io.j = j;
  io.v = v;
  io.vb = v ? value_bytes : 0;
  io.train_p = train_p;
  io.test_p = test_p;
  io.train_j = train_j;
  io.test_j = test_j;
  io.train_v = train_v;
  io.test_v = test_v;
  io.rows = w.rows;
  const unsigned wave_grid = (unsigned)(((long long)n_rows + 3) / 4), team_grid = (unsigned)std::min(n_rows, kSplitMaxTeams);
  auto write = [&](auto wave_k, auto team_k) {
    hipLaunchKernelGGL(wave_k, dim3(wave_grid), dim3(256), 0, s, a, io);
    hipLaunchKernelGGL(team_k, dim3(team_grid), dim3(256), 0, s, a, io);
  };
  if (mode == 0) write(split_write_wave_kernel<kProp>, split_write_team_kernel<kProp>);
  else if (by) write(split_write_wave_kernel<kBy>, split_write_team_kernel<kBy>);
  else write(split_write_wave_kernel<kRand>, split_write_team_kernel<kRand>);
  return hipGetLastError();
}

}  // namespace rsparse_hip
