// The interaction matrix from an event log, on the device (gfx950): one (user, item[, value][, timestamp]) record per event ->
// the canonical CSR over the CELLS (distinct (user, item) pairs) with an aggregate of every cell's events, their count and their
// latest timestamp.  rsparse_amd/events.py (events_reference) is the definition in numpy, the C header states it for other
// hosts; DESIGN.md 3.26 has the scheme and the measurements.
//
//   1. pack      key = user << bits(n_items) | item, payload = the event's index; ids outside the shape raise a flag and the
//                call ends there.  32-bit keys when bits(n_users) + bits(n_items) <= 32, else 64-bit.
//   2. sort      rocprim::radix_sort_pairs on exactly the key bits in use: stable, so the events of a cell keep their input
//                order.  Values and timestamps do NOT ride through the sort: they are gathered afterwards by event index.
//   3. heads     an entry whose key differs from its predecessor's opens a cell.  The sorted entries are cut into SPANS of
//                kEvSpan entries whatever the rows look like; a launch counts the heads of every span, a scan gives the spans'
//                first cell.
//   4. reduce    per span: a ballot per wave finds the heads, a head's cell index is the span's offset + its rank among the
//                span's heads.  The lane at a head finds the end of its cell (the next head of the ballot, else a galloping
//                search in the sorted keys), writes j, count and the row pointers between its user and the previous head's
//                (every empty row included), and walks a cell of at most 64 events in input order.  A longer cell goes to a
//                work list: one 64-bit integer atomic reserves its list slot and its chunk slots together.
//   5. long      a thread per chunk of 64 events (counted from the cell's first event) walks it left to right; then one wave
//                per listed cell adds the chunk sums left to right and reduces max / latest / last over the chunks' 64-bit keys
//                with the event index as tie-break.  Nothing depends on the order in which cells entered the list: a cell's
//                chunk slots are its own, wherever they lie.
// No floating-point atomics; the sums have the order the definition states, so the result equals the numpy reference bit for
// bit (the decay weights up to exp2) and repeat calls agree bit for bit.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/rsparse_wrmf_hip.h"
#include "wrmf_internal.h"
#include "wrmf_wave.h"

#pragma clang fp contract(off)

namespace rsparse_hip {
namespace {

using dev::f64_key;
using dev::key_f64;
using dev::u64;

constexpr int kEvThreads = 256;
constexpr int kEvPer = 4;
constexpr int kEvSpan = kEvThreads * kEvPer;   // sorted entries per span
constexpr int kEvChunk = 64;                   // events per chunk of the stated summation order; a longer cell is "long"
constexpr int kEvGrid = 256 * 16;
constexpr u64 kEvSlotMask = (1ull << 40) - 1;  // cursor: list entries << 40 | chunk slots

struct EvLong {   // a cell of more than kEvChunk events
  int32_t start, len, cell, chunk0;   // first sorted position, events, cell index, first chunk slot
};

struct EvIn {
  const uint32_t* sidx;   // event index of every sorted position
  const double* values;   // null: every value is 1
  const double* ts;       // null: no timestamps
  int64_t n;
  int aggregate;
  int decay;              // half_life > 0
  double half_life;
  int has_now;
  double now;
  const u64* now_key;     // !has_now: the key of the largest timestamp
};

__device__ __forceinline__ double ev_now(const EvIn& a) { return a.has_now ? a.now : key_f64(*a.now_key); }

// what a run of m <= kEvChunk events at sorted positions e0 .. contributes, walked in input order: the sum of the terms left to
// right, the largest value key, the largest timestamp key and the event that has it (ties: the later event)
__device__ __forceinline__ void ev_walk(const EvIn& a, double now, int64_t e0, int m, double& sum, u64& vmax, u64& tmax, uint32_t& last) {
  sum = 0.0; vmax = 0; tmax = 0; last = 0;
  for (int k = 0; k < m; k++) {
    const uint32_t idx = a.sidx[e0 + k];
    double t = 0.0;
    if (a.ts) {
      t = a.ts[idx];
      const u64 tk = f64_key(t);
      if (tk >= tmax) { tmax = tk; last = idx; }
    }
    if (a.aggregate == RSPARSE_HIP_EVENTS_SUM) {
      double v = a.values ? a.values[idx] : 1.0;
      if (a.decay) v = v * exp2((t - now) / a.half_life);
      sum = k == 0 ? v : sum + v;
    } else if (a.aggregate == RSPARSE_HIP_EVENTS_MAX) {
      const u64 vk = f64_key(a.values ? a.values[idx] : 1.0);
      vmax = vk > vmax ? vk : vmax;
    }
  }
}

__device__ __forceinline__ u64 ev_wave_max(u64 v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const u64 o = __shfl_xor(v, d);
    v = o > v ? o : v;
  }
  return v;
}

template <class K>
__global__ __launch_bounds__(kEvThreads) void events_pack_kernel(const int32_t* __restrict__ users, const int32_t* __restrict__ items,
                                                                 int64_t n, int n_users, int n_items, int ibits, K* __restrict__ keys,
                                                                 uint32_t* __restrict__ idx, int* __restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int local = 0;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const int32_t u = users[e], i = items[e];
    local |= (u < 0 || u >= n_users || i < 0 || i >= n_items) ? 1 : 0;
    keys[e] = (K)(((u64)(uint32_t)u << ibits) | (u64)(uint32_t)i);
    idx[e] = (uint32_t)e;
  }
  if (local) atomicOr(bad, 1);
}

// the key of the largest timestamp (an integer maximum: any order gives the same bits)
__global__ __launch_bounds__(kEvThreads) void events_now_kernel(const double* __restrict__ ts, int64_t n, u64* __restrict__ now_key) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  u64 m = 0;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const u64 k = f64_key(ts[e]);
    m = k > m ? k : m;
  }
  m = ev_wave_max(m);
  if ((threadIdx.x & 63) == 0) atomicMax((unsigned long long*)now_key, (unsigned long long)m);
}

template <class K>
__global__ __launch_bounds__(kEvThreads) void events_heads_kernel(const K* __restrict__ keys, int64_t n, int n_spans,
                                                                  int32_t* __restrict__ span_count) {
  __shared__ int s_w[4];
  const int t = threadIdx.x;
  for (int s = blockIdx.x; s < n_spans; s += gridDim.x) {
    const int64_t start = (int64_t)s * kEvSpan;
    int c = 0;
#pragma unroll
    for (int q = 0; q < kEvPer; q++) {
      const int64_t e = start + q * kEvThreads + t;
      if (e < n) c += (e == 0 || keys[e] != keys[e - 1]) ? 1 : 0;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_down(c, d);
    __syncthreads();
    if ((t & 63) == 0) s_w[t >> 6] = c;
    __syncthreads();
    if (t == 0) span_count[s] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
  }
}

// the first position behind e whose key differs from key (n: none): the keys are sorted, so gallop, then bisect
template <class K>
__device__ __forceinline__ int64_t ev_cell_end(const K* __restrict__ keys, int64_t n, int64_t e, K key) {
  int64_t lo = e, d = 1;
  while (lo + d < n && keys[lo + d] == key) { lo += d; d <<= 1; }
  int64_t hi = lo + d < n ? lo + d : n;   // keys[lo] == key; keys[hi] != key or hi == n
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] == key) lo = mid; else hi = mid;
  }
  return hi;
}

template <class K>
__global__ __launch_bounds__(kEvThreads) void events_reduce_kernel(const K* __restrict__ keys, EvIn a, int ibits, int n_users, int n_spans,
                                                                   const int32_t* __restrict__ span_off, int32_t* __restrict__ p,
                                                                   int32_t* __restrict__ j, double* __restrict__ x,
                                                                   int32_t* __restrict__ count, double* __restrict__ latest,
                                                                   EvLong* __restrict__ list, u64* __restrict__ cursor) {
  __shared__ int s_cnt[kEvPer * 4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t n = a.n;
  const double now = a.decay ? ev_now(a) : 0.0;
  const K imask = (K)((1ull << ibits) - 1);
  const bool want_latest = a.ts && latest;
  const bool walk = a.aggregate != RSPARSE_HIP_EVENTS_COUNT || want_latest;
  for (int s = blockIdx.x; s < n_spans; s += gridDim.x) {
    const int64_t start = (int64_t)s * kEvSpan;
    K key[kEvPer];
    bool head[kEvPer];
    u64 bal[kEvPer];
#pragma unroll
    for (int q = 0; q < kEvPer; q++) {
      const int64_t e = start + q * kEvThreads + t;
      key[q] = 0;
      head[q] = false;
      if (e < n) {
        key[q] = keys[e];
        head[q] = e == 0 || keys[e - 1] != key[q];
      }
      bal[q] = __ballot(head[q]);
      if (lane == 0) s_cnt[q * 4 + wave] = __popcll(bal[q]);
    }
    __syncthreads();
    const int off = span_off[s];
#pragma unroll
    for (int q = 0; q < kEvPer; q++) {
      if (!head[q]) continue;
      const int64_t e = start + q * kEvThreads + t;
      int before = 0;
      for (int w = 0; w < q * 4 + wave; w++) before += s_cnt[w];
      const int r = off + before + __popcll(bal[q] & ((1ull << lane) - 1));
      // the end of the cell: the next head of this wave's 64 entries, else searched for
      const u64 above = lane == 63 ? 0 : (bal[q] >> (lane + 1));
      const int64_t end = above ? e + __ffsll((unsigned long long)above) : ev_cell_end(keys, n, e, key[q]);
      const int m = (int)(end - e);
      const int u = (int)((u64)key[q] >> ibits);
      j[r] = (int32_t)(key[q] & imask);
      if (count) count[r] = m;
      // row pointers: position r opens every row in (the previous head's user, u]; the last head closes the rows behind it
      const int64_t prev = e == 0 ? -1 : (int64_t)((u64)keys[e - 1] >> ibits);
      for (int64_t rr = prev + 1; rr <= u; rr++) p[rr] = r;
      if (end == n)
        for (int64_t rr = (int64_t)u + 1; rr <= n_users; rr++) p[rr] = r + 1;
      if (a.aggregate == RSPARSE_HIP_EVENTS_COUNT) x[r] = (double)m;
      if (!walk) continue;
      if (m <= kEvChunk) {
        double sum;
        u64 vmax, tmax;
        uint32_t last;
        ev_walk(a, now, e, m, sum, vmax, tmax, last);
        if (a.aggregate == RSPARSE_HIP_EVENTS_SUM) x[r] = sum;
        else if (a.aggregate == RSPARSE_HIP_EVENTS_MAX) x[r] = key_f64(vmax);
        else if (a.aggregate == RSPARSE_HIP_EVENTS_LAST) x[r] = a.values ? a.values[last] : 1.0;
        if (want_latest) latest[r] = key_f64(tmax);
      } else {
        const u64 n_chunks = (u64)((m + kEvChunk - 1) / kEvChunk);
        const u64 old = atomicAdd((unsigned long long*)cursor, (unsigned long long)((1ull << 40) | n_chunks));
        EvLong c;
        c.start = (int32_t)e; c.len = m; c.cell = r; c.chunk0 = (int32_t)(old & kEvSlotMask);
        list[old >> 40] = c;
      }
    }
    __syncthreads();
  }
}

// a thread per chunk slot: the slots of list entry li are [chunk0, chunk0 + its chunks), ascending with li (one atomic gave both)
__global__ __launch_bounds__(kEvThreads) void events_long_chunks_kernel(EvIn a, const EvLong* __restrict__ list,
                                                                        const u64* __restrict__ cursor, u64* __restrict__ cA,
                                                                        u64* __restrict__ cB, uint32_t* __restrict__ cC) {
  const u64 cur = *cursor;
  const int n_list = (int)(cur >> 40);
  const int64_t n_slots = (int64_t)(cur & kEvSlotMask);
  const double now = a.decay ? ev_now(a) : 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n_slots; g += stride) {
    int lo = 0, hi = n_list;
    while (hi - lo > 1) {
      const int mid = lo + ((hi - lo) >> 1);
      if ((int64_t)list[mid].chunk0 <= g) lo = mid; else hi = mid;
    }
    const EvLong c = list[lo];
    const int64_t ch = g - c.chunk0;
    const int64_t done = ch * kEvChunk;
    const int m = (int64_t)c.len - done < kEvChunk ? (int)((int64_t)c.len - done) : kEvChunk;
    double sum;
    u64 vmax, tmax;
    uint32_t last;
    ev_walk(a, now, (int64_t)c.start + done, m, sum, vmax, tmax, last);
    cA[g] = a.aggregate == RSPARSE_HIP_EVENTS_SUM ? (u64)__double_as_longlong(sum) : vmax;
    cB[g] = tmax;
    cC[g] = last;
  }
}

// one wave per listed cell: the chunk sums left to right; max / latest / last over the chunks' keys
__global__ __launch_bounds__(kEvThreads) void events_long_finish_kernel(EvIn a, const EvLong* __restrict__ list,
                                                                        const u64* __restrict__ cursor, const u64* __restrict__ cA,
                                                                        const u64* __restrict__ cB, const uint32_t* __restrict__ cC,
                                                                        double* __restrict__ x, double* __restrict__ latest) {
  const int n_list = (int)(*cursor >> 40);
  const int lane = threadIdx.x & 63;
  const int wave = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6);
  const int n_waves = (int)((gridDim.x * (size_t)blockDim.x) >> 6);
  for (int li = wave; li < n_list; li += n_waves) {
    const EvLong c = list[li];
    // (li is the same in every lane: said to the compiler, so that the loops below are scalar ones)
    const int n_chunks = dev::rfl((c.len + kEvChunk - 1) / kEvChunk);
    const int64_t base = dev::rfl(c.chunk0);
    if (a.aggregate == RSPARSE_HIP_EVENTS_SUM) {
      // 64 chunk sums per load, the next 64 in flight while these are added; a sum is read from its lane into scalar registers
      // (v_readlane, k is uniform), so the dependent chain is one v_add_f64 per chunk
      u64 v = lane < n_chunks ? cA[base + lane] : 0;
      u64 next = 64 + lane < n_chunks ? cA[base + 64 + lane] : 0;
      int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
      auto sum_of = [&](int k) {
        const u64 bits = (u64)(uint32_t)__builtin_amdgcn_readlane(lo, k) | ((u64)(uint32_t)__builtin_amdgcn_readlane(hi, k) << 32);
        return __longlong_as_double((long long)bits);
      };
      double acc = sum_of(0);   // the first chunk's sum as it is, then the others added in order
      for (int b = 0; b < n_chunks; b += 64) {
        const int cnt = n_chunks - b < 64 ? n_chunks - b : 64;
        for (int k = b == 0 ? 1 : 0; k < cnt; k++) acc = acc + sum_of(k);
        v = next;
        if (b + 128 + lane < n_chunks) next = cA[base + b + 128 + lane];
        lo = (int)(uint32_t)v; hi = (int)(uint32_t)(v >> 32);
      }
      if (lane == 0) x[c.cell] = acc;
    } else if (a.aggregate == RSPARSE_HIP_EVENTS_MAX) {
      u64 m = 0;
      for (int k = lane; k < n_chunks; k += 64) {
        const u64 o = cA[base + k];
        m = o > m ? o : m;
      }
      m = ev_wave_max(m);
      if (lane == 0) x[c.cell] = key_f64(m);
    }
    if (a.ts) {
      u64 tm = 0;
      uint32_t id = 0;
      for (int k = lane; k < n_chunks; k += 64) {
        const u64 tk = cB[base + k];
        const uint32_t ik = cC[base + k];
        if (tk > tm || (tk == tm && ik >= id)) { tm = tk; id = ik; }
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        const u64 to = __shfl_xor(tm, d);
        const uint32_t io = __shfl_xor(id, d);
        if (to > tm || (to == tm && io > id)) { tm = to; id = io; }
      }
      if (lane == 0) {
        if (latest) latest[c.cell] = key_f64(tm);
        if (a.aggregate == RSPARSE_HIP_EVENTS_LAST) x[c.cell] = a.values ? a.values[id] : 1.0;
      }
    }
  }
}

inline int ev_bits(int n) {   // bits that hold 0 .. n - 1
  int b = 0;
  while (b < 31 && ((int64_t)1 << b) < (int64_t)n) b++;
  return b;
}

template <class K>
hipError_t events_run(int64_t n, int n_users, int n_items, int ibits, int key_bits, const int32_t* users, const int32_t* items, EvIn a,
                      int32_t* p, int32_t* j, double* x, int32_t* count, double* latest, int64_t capacity, int64_t* n_cells,
                      hipStream_t s, int* status) {
  hipError_t err;
  const size_t nn = (size_t)n;
  const int n_spans = (int)((n + kEvSpan - 1) / kEvSpan);
  const size_t list_cap = nn / (kEvChunk + 1) + 1, slot_cap = nn / 32 + 2;
  DevBuf keys, keys_out, idx, idx_out, tmp, scan_tmp, spans, small, list, cA, cB, cC;
#define RSP_TRY(e) do { if ((err = (e)) != hipSuccess) return err; } while (0)
  RSP_TRY(small.alloc(32));   // [0] the id flag, [8] the cursor, [16] the key of the largest timestamp
  RSP_TRY(hipMemsetAsync(small.p, 0, 32, s));
  int* d_bad = small.as<int>();
  u64* d_cursor = small.as<u64>() + 1;
  u64* d_now = small.as<u64>() + 2;
  RSP_TRY(keys.alloc(nn * sizeof(K)));
  RSP_TRY(idx.alloc(nn * 4));
  const int gn = (int)((n + kEvThreads - 1) / kEvThreads);
  const dim3 grid_n(gn < kEvGrid ? gn : kEvGrid), block(kEvThreads);
  hipLaunchKernelGGL(events_pack_kernel<K>, grid_n, block, 0, s, users, items, n, n_users, n_items, ibits, keys.as<K>(),
                     idx.as<uint32_t>(), d_bad);
  RSP_TRY(hipGetLastError());
  int host_bad = 0;
  RSP_TRY(hipMemcpyAsync(&host_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
  RSP_TRY(hipStreamSynchronize(s));
  if (host_bad) {
    *status = 1;
    return hipSuccess;
  }
  const K* skeys = keys.as<K>();
  a.sidx = idx.as<uint32_t>();
  if (key_bits > 0) {   // (one user and one item: every key is 0 and the log is in order already)
    RSP_TRY(keys_out.alloc(nn * sizeof(K)));
    RSP_TRY(idx_out.alloc(nn * 4));
    size_t tmp_bytes = 0;
    RSP_TRY(rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys.as<K>(), keys_out.as<K>(), idx.as<uint32_t>(), idx_out.as<uint32_t>(),
                                      nn, 0, key_bits, s));
    RSP_TRY(tmp.alloc(tmp_bytes));
    RSP_TRY(rocprim::radix_sort_pairs(tmp.p, tmp_bytes, keys.as<K>(), keys_out.as<K>(), idx.as<uint32_t>(), idx_out.as<uint32_t>(), nn,
                                      0, key_bits, s));
    skeys = keys_out.as<K>();
    a.sidx = idx_out.as<uint32_t>();
  }
  // spans: counts [n_spans + 1] (the last one 0) | offsets [n_spans + 1] (the last one = the number of cells)
  const size_t ns1 = (size_t)n_spans + 1;
  RSP_TRY(spans.alloc(2 * ns1 * 4));
  int32_t* span_count = spans.as<int32_t>();
  int32_t* span_off = span_count + ns1;
  RSP_TRY(hipMemsetAsync(span_count + n_spans, 0, 4, s));
  const dim3 grid_s(n_spans < kEvGrid ? n_spans : kEvGrid);
  hipLaunchKernelGGL(events_heads_kernel<K>, grid_s, block, 0, s, skeys, n, n_spans, span_count);
  RSP_TRY(hipGetLastError());
  size_t scan_bytes = 0;
  RSP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, span_count, span_off, (int32_t)0, ns1, rocprim::plus<int32_t>(), s));
  RSP_TRY(scan_tmp.alloc(scan_bytes));
  RSP_TRY(rocprim::exclusive_scan(scan_tmp.p, scan_bytes, span_count, span_off, (int32_t)0, ns1, rocprim::plus<int32_t>(), s));
  int32_t cells = 0;
  RSP_TRY(hipMemcpyAsync(&cells, span_off + n_spans, 4, hipMemcpyDeviceToHost, s));
  RSP_TRY(hipStreamSynchronize(s));
  *n_cells = cells;
  if ((int64_t)cells > capacity) {
    *status = 2;
    return hipSuccess;
  }
  if (a.decay && !a.has_now) {
    hipLaunchKernelGGL(events_now_kernel, grid_n, block, 0, s, a.ts, n, d_now);
    RSP_TRY(hipGetLastError());
  }
  a.now_key = d_now;
  const bool may_list = a.aggregate != RSPARSE_HIP_EVENTS_COUNT || (a.ts && latest);
  if (may_list) {
    RSP_TRY(list.alloc(list_cap * sizeof(EvLong)));
    RSP_TRY(cA.alloc(slot_cap * 8));
    RSP_TRY(cB.alloc(slot_cap * 8));
    RSP_TRY(cC.alloc(slot_cap * 4));
  }
  hipLaunchKernelGGL(events_reduce_kernel<K>, grid_s, block, 0, s, skeys, a, ibits, n_users, n_spans, (const int32_t*)span_off, p, j, x,
                     count, latest, list.as<EvLong>(), d_cursor);
  RSP_TRY(hipGetLastError());
  if (may_list && n > kEvChunk) {
    const int gc = (int)((slot_cap + kEvThreads - 1) / kEvThreads);
    hipLaunchKernelGGL(events_long_chunks_kernel, dim3(gc < kEvGrid ? gc : kEvGrid), block, 0, s, a, (const EvLong*)list.as<EvLong>(),
                       (const u64*)d_cursor, cA.as<u64>(), cB.as<u64>(), cC.as<uint32_t>());
    RSP_TRY(hipGetLastError());
    const int gl = (int)((list_cap + 3) / 4);
    hipLaunchKernelGGL(events_long_finish_kernel, dim3(gl < 1024 ? gl : 1024), block, 0, s, a, (const EvLong*)list.as<EvLong>(),
                       (const u64*)d_cursor, (const u64*)cA.as<u64>(), (const u64*)cB.as<u64>(), (const uint32_t*)cC.as<uint32_t>(), x,
                       latest);
    RSP_TRY(hipGetLastError());
  }
  RSP_TRY(hipStreamSynchronize(s));   // the scratch is freed on return
#undef RSP_TRY
  return hipSuccess;
}

}  // namespace

hipError_t events_to_csr_device(int64_t n, int n_users, int n_items, const int32_t* users, const int32_t* items, const double* values,
                                const double* ts, int aggregate, double half_life, int has_now, double now, int32_t* p, int32_t* j,
                                double* x, int32_t* count, double* latest, int64_t capacity, int64_t* n_cells, hipStream_t s,
                                int* status) {
  *status = 0;
  EvIn a;
  a.sidx = nullptr; a.values = values; a.ts = ts; a.n = n; a.aggregate = aggregate;
  a.decay = half_life > 0.0 ? 1 : 0; a.half_life = half_life; a.has_now = has_now ? 1 : 0; a.now = now; a.now_key = nullptr;
  const int ibits = ev_bits(n_items), ubits = ev_bits(n_users);
  if (ubits + ibits <= 32)
    return events_run<uint32_t>(n, n_users, n_items, ibits, ubits + ibits, users, items, a, p, j, x, count, latest, capacity, n_cells, s,
                                status);
  return events_run<uint64_t>(n, n_users, n_items, ibits, ubits + ibits, users, items, a, p, j, x, count, latest, capacity, n_cells, s,
                              status);
}

}  // namespace rsparse_hip
