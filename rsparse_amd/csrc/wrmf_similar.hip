// Item-to-item cosine similarity (get_similar_items, R/MatrixFactorizationRecommender.R:79-116): the operands of the top-k
// path, not the scoring.  cosine(i, j) = <v_i / |v_i|, v_j / |v_j|>, so once every item vector is normalised the k most similar
// items of a query ARE its top_product against the normalised matrix (wrmf_topk.hip / wrmf_topk_large.hip, unchanged: fp32
// nomination, double re-scoring and ordering).  What is here:
//
//   normalize_items_kernel  V[:, c0:c1) (fp32 or fp64, n_items x ld row-major) -> Vn64 (n_items x r doubles, compact),
//                           Vn32 = (float)Vn64, flags[item] = 1 for a degenerate item (sum of squares zero or not finite:
//                           its row is written as zeros).  The sum of squares is accumulated in double whatever the input
//                           type, so fp32 factors whose squares underflow in fp32 (1e-30) still normalise.
//   gather_queries_kernel   the rows of Vn32 / Vn64 of a vector of query ids -> Q32 / Q64, the self-exclusion slots
//                           nr_p = 0..n_q, nr_j = query id (top_product's not_recommend), and bad[q] = 1 for a query that
//                           is degenerate (all-zero row) or out of range.
//   mask_queries_kernel     after the top-k: the rows of the bad queries become NA_integer_ / NaN.
//
// All three stream: G lanes per item (G = the power of two >= r / 4, 1..64), four consecutive coordinates per lane, 16-byte loads
// and stores when the rows are 16-byte aligned (scalar otherwise: a column window that starts at the bias column, odd ranks),
// the sum of squares by a butterfly of __shfl_xor within the G lanes (every lane ends with the same bits: at each step the two
// partners add the same two numbers).  No LDS, no atomics.  Bytes per item: sizeof(T) r read, 12 r written.
#include <hip/hip_runtime.h>

#include "wrmf_internal.h"

namespace rsparse_hip {

namespace {

constexpr int kSimThreads = 256;
constexpr int kSimMaxGrid = 256 * 8;   // workgroups (grid-stride over the items beyond)

template <typename T> struct Vec16;   // one 16-byte load of T
template <> struct Vec16<float> { using type = float4; static constexpr int n = 4; };
template <> struct Vec16<double> { using type = double2; static constexpr int n = 2; };

// four consecutive elements at p -> double; `valid` of them exist (the others read as zero)
template <typename T, bool VEC>
__device__ __forceinline__ void load4(const T* __restrict__ p, int valid, double x[4]) {
  if (VEC && valid >= 4) {
    if constexpr (sizeof(T) == 4) {
      const float4 v = *reinterpret_cast<const float4*>(p);
      x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
      const double2 a = *reinterpret_cast<const double2*>(p);
      const double2 b = *reinterpret_cast<const double2*>(p + 2);
      x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; e++) x[e] = e < valid ? (double)p[e] : 0.0;
  }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ p32, double* __restrict__ p64, int valid, const double y[4]) {
  if (VEC && valid >= 4) {
    *reinterpret_cast<float4*>(p32) = make_float4((float)y[0], (float)y[1], (float)y[2], (float)y[3]);
    *reinterpret_cast<double2*>(p64) = make_double2(y[0], y[1]);
    *reinterpret_cast<double2*>(p64 + 2) = make_double2(y[2], y[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; e++)
      if (e < valid) {
        p32[e] = (float)y[e];
        p64[e] = y[e];
      }
  }
}

// G lanes per item, two items per group and pass (both loads are issued before either sum).  VIN / VOUT: the rows of V / of the
// outputs are 16-byte aligned.
template <typename T, int G, bool VIN, bool VOUT>
__global__ void __launch_bounds__(kSimThreads)
normalize_items_kernel(const T* __restrict__ V, int n_items, int64_t ld, int c0, int r, float* __restrict__ Vn32,
                       double* __restrict__ Vn64, int32_t* __restrict__ flags) {
  constexpr int GPB = kSimThreads / G;   // groups per workgroup
  const int gl = threadIdx.x % G;
  const int j0 = 4 * gl;
  const int valid = min(4, r - j0);      // <= 0: this lane holds no coordinate of the row
  const int64_t slots = (int64_t)gridDim.x * GPB;
  // every lane of the workgroup makes the same number of passes (the shuffles below run with all lanes present)
  for (int64_t base = (int64_t)blockIdx.x * GPB; base < n_items; base += 2 * slots) {
    double x[2][4];
    int64_t item[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
      item[u] = base + threadIdx.x / G + u * slots;
      if (item[u] < n_items && valid > 0)
        load4<T, VIN>(V + item[u] * ld + c0 + j0, valid, x[u]);
      else
        x[u][0] = x[u][1] = x[u][2] = x[u][3] = 0.0;
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
      double ss = (x[u][0] * x[u][0] + x[u][1] * x[u][1]) + (x[u][2] * x[u][2] + x[u][3] * x[u][3]);
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, G);
      const bool ok = ss > 0.0 && ss < INFINITY;   // (a NaN fails both)
      const double nrm = sqrt(ss);
      double y[4];
#pragma unroll
      for (int e = 0; e < 4; e++) y[e] = ok ? x[u][e] / nrm : 0.0;
      if (item[u] < n_items) {
        if (valid > 0) store4<VOUT>(Vn32 + item[u] * r + j0, Vn64 + item[u] * r + j0, valid, y);
        if (gl == 0) flags[item[u]] = ok ? 0 : 1;
      }
    }
  }
}

template <int G, bool VEC>
__global__ void __launch_bounds__(kSimThreads)
gather_queries_kernel(const float* __restrict__ Vn32, const double* __restrict__ Vn64, int n_items, int r,
                      const int32_t* __restrict__ query, int n_q, float* __restrict__ Q32, double* __restrict__ Q64,
                      int32_t* __restrict__ nr_p, int32_t* __restrict__ nr_j, int32_t* __restrict__ bad) {
  constexpr int GPB = kSimThreads / G;
  const int gl = threadIdx.x % G;
  const int j0 = 4 * gl;
  const int valid = min(4, r - j0);
  const int64_t slots = (int64_t)gridDim.x * GPB;
  if (blockIdx.x == 0 && threadIdx.x == 0) nr_p[n_q] = n_q;
  for (int64_t base = (int64_t)blockIdx.x * GPB; base < n_q; base += slots) {
    const int64_t q = base + threadIdx.x / G;
    int id = -1;
    if (q < n_q) {
      id = query[q];
      if (id < 0 || id >= n_items) id = -1;   // out of range: nothing is read, the row is masked afterwards
    }
    double y[4] = {0.0, 0.0, 0.0, 0.0};
    if (id >= 0 && valid > 0) load4<double, VEC>(Vn64 + (int64_t)id * r + j0, valid, y);
    int nz = (y[0] != 0.0) | (y[1] != 0.0) | (y[2] != 0.0) | (y[3] != 0.0);
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) nz |= __shfl_xor(nz, o, G);
    if (q < n_q) {
      if (valid > 0) {
        // Q32 = (float)Q64 is Vn32's row bit for bit (Vn32 = (float)Vn64), so Vn32 is not read
        store4<VEC>(Q32 + q * r + j0, Q64 + q * r + j0, valid, y);
      }
      if (gl == 0) {
        nr_p[q] = (int32_t)q;
        nr_j[q] = id >= 0 ? id : 0;
        bad[q] = nz ? 0 : 1;
      }
    }
  }
  (void)Vn32;
}

__global__ void __launch_bounds__(kSimThreads)
mask_queries_kernel(const int32_t* __restrict__ bad, int n_q, int k, int32_t* __restrict__ res, double* __restrict__ scores) {
  const int64_t n = (int64_t)n_q * k;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
    if (bad[e / k]) {
      res[e] = INT32_MIN;                                        // NA_integer_
      scores[e] = __longlong_as_double(0x7ff8000000000000ll);    // NA_real_ as the top-k path writes it
    }
}

int sim_grid(int64_t n, int G) {
  const int gpb = kSimThreads / G;
  const int64_t blocks = (n + gpb - 1) / gpb;
  return (int)(blocks < 1 ? 1 : (blocks > kSimMaxGrid ? kSimMaxGrid : blocks));
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <typename T, int G>
hipError_t launch_normalize_g(const T* V, int n_items, int64_t ld, int c0, int r, float* Vn32, double* Vn64, int32_t* flags,
                              hipStream_t s) {
  constexpr int per16 = Vec16<T>::n;
  const bool vin = aligned16(V) && ld % per16 == 0 && c0 % per16 == 0;
  const bool vout = aligned16(Vn32) && aligned16(Vn64) && r % 4 == 0;
  // (two items per group and pass: half the workgroups of one item per group)
  const dim3 grid(sim_grid(((int64_t)n_items + 1) / 2, G)), block(kSimThreads);
  if (vin && vout)
    hipLaunchKernelGGL((normalize_items_kernel<T, G, true, true>), grid, block, 0, s, V, n_items, ld, c0, r, Vn32, Vn64, flags);
  else if (vin)
    hipLaunchKernelGGL((normalize_items_kernel<T, G, true, false>), grid, block, 0, s, V, n_items, ld, c0, r, Vn32, Vn64, flags);
  else if (vout)
    hipLaunchKernelGGL((normalize_items_kernel<T, G, false, true>), grid, block, 0, s, V, n_items, ld, c0, r, Vn32, Vn64, flags);
  else
    hipLaunchKernelGGL((normalize_items_kernel<T, G, false, false>), grid, block, 0, s, V, n_items, ld, c0, r, Vn32, Vn64, flags);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_normalize_t(const T* V, int n_items, int64_t ld, int c0, int r, float* Vn32, double* Vn64, int32_t* flags,
                              hipStream_t s) {
  if (r <= 4) return launch_normalize_g<T, 1>(V, n_items, ld, c0, r, Vn32, Vn64, flags, s);
  if (r <= 8) return launch_normalize_g<T, 2>(V, n_items, ld, c0, r, Vn32, Vn64, flags, s);
  if (r <= 16) return launch_normalize_g<T, 4>(V, n_items, ld, c0, r, Vn32, Vn64, flags, s);
  if (r <= 32) return launch_normalize_g<T, 8>(V, n_items, ld, c0, r, Vn32, Vn64, flags, s);
  if (r <= 64) return launch_normalize_g<T, 16>(V, n_items, ld, c0, r, Vn32, Vn64, flags, s);
  if (r <= 128) return launch_normalize_g<T, 32>(V, n_items, ld, c0, r, Vn32, Vn64, flags, s);
  return launch_normalize_g<T, 64>(V, n_items, ld, c0, r, Vn32, Vn64, flags, s);
}

template <int G>
hipError_t launch_gather_g(const float* Vn32, const double* Vn64, int n_items, int r, const int32_t* query, int n_q, float* Q32,
                           double* Q64, int32_t* nr_p, int32_t* nr_j, int32_t* bad, hipStream_t s) {
  const bool vec = aligned16(Vn64) && aligned16(Q32) && aligned16(Q64) && r % 4 == 0;
  const dim3 grid(sim_grid(n_q, G)), block(kSimThreads);
  if (vec)
    hipLaunchKernelGGL((gather_queries_kernel<G, true>), grid, block, 0, s, Vn32, Vn64, n_items, r, query, n_q, Q32, Q64, nr_p,
                       nr_j, bad);
  else
    hipLaunchKernelGGL((gather_queries_kernel<G, false>), grid, block, 0, s, Vn32, Vn64, n_items, r, query, n_q, Q32, Q64, nr_p,
                       nr_j, bad);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_normalize_items(const void* V, bool f64, int n_items, int64_t ld, int c0, int r, float* Vn32, double* Vn64,
                                  int32_t* flags, hipStream_t s) {
  if (n_items <= 0) return hipSuccess;
  if (r < 1 || r > 256 || c0 < 0 || (int64_t)c0 + r > ld) return hipErrorInvalidValue;
  return f64 ? launch_normalize_t(static_cast<const double*>(V), n_items, ld, c0, r, Vn32, Vn64, flags, s)
             : launch_normalize_t(static_cast<const float*>(V), n_items, ld, c0, r, Vn32, Vn64, flags, s);
}

size_t similar_query_ws_bytes(int n_q, int r) {
  auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t n = (size_t)(n_q > 0 ? n_q : 0);
  return up(n * r * 8) + up(n * r * 4) + up((n + 1) * 4) + 2 * up(n * 4);
}

SimilarQueryWs similar_query_ws(void* ws, int n_q, int r) {
  auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t n = (size_t)(n_q > 0 ? n_q : 0);
  char* p = static_cast<char*>(ws);
  SimilarQueryWs w;
  w.Q64 = reinterpret_cast<double*>(p); p += up(n * r * 8);
  w.Q32 = reinterpret_cast<float*>(p); p += up(n * r * 4);
  w.nr_p = reinterpret_cast<int32_t*>(p); p += up((n + 1) * 4);
  w.nr_j = reinterpret_cast<int32_t*>(p); p += up(n * 4);
  w.bad = reinterpret_cast<int32_t*>(p);
  return w;
}

hipError_t launch_gather_queries(const float* Vn32, const double* Vn64, int n_items, int r, const int32_t* query, int n_q,
                                 const SimilarQueryWs& w, hipStream_t s) {
  if (n_q <= 0) return hipSuccess;
  if (r < 1 || r > 256) return hipErrorInvalidValue;
#define RSPARSE_SIM_GATHER(G) \
  return launch_gather_g<G>(Vn32, Vn64, n_items, r, query, n_q, w.Q32, w.Q64, w.nr_p, w.nr_j, w.bad, s)
  if (r <= 4) RSPARSE_SIM_GATHER(1);
  if (r <= 8) RSPARSE_SIM_GATHER(2);
  if (r <= 16) RSPARSE_SIM_GATHER(4);
  if (r <= 32) RSPARSE_SIM_GATHER(8);
  if (r <= 64) RSPARSE_SIM_GATHER(16);
  if (r <= 128) RSPARSE_SIM_GATHER(32);
  RSPARSE_SIM_GATHER(64);
#undef RSPARSE_SIM_GATHER
}

hipError_t launch_mask_queries(const int32_t* bad, int n_q, int k, int32_t* res, double* scores, hipStream_t s) {
  const int64_t n = (int64_t)n_q * k;
  if (n <= 0) return hipSuccess;
  int64_t blocks = (n + kSimThreads - 1) / kSimThreads;
  if (blocks > kSimMaxGrid) blocks = kSimMaxGrid;
  hipLaunchKernelGGL(mask_queries_kernel, dim3((int)blocks), dim3(kSimThreads), 0, s, bad, n_q, k, res, scores);
  return hipGetLastError();
}

}  // namespace rsparse_hip
