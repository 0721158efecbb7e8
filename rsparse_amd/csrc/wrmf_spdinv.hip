// In-place inverse of a symmetric positive definite float64 matrix by a BLOCKED SYMMETRIC SWEEP -- block Gauss-Jordan on an SPD
// matrix, the "sweep operator" (gfx950, wave64, fp64; rsparse_amd/ease.py: spd_sweep_reference is the definition,
// include/rsparse_wrmf_hip.h repeats it).
//
// For the pivot blocks K = [k0, k0 + nb), k0 = 0, 64, 128, ... (the last one narrower), on the matrix S that starts as A:
//     T = S[:, K];  D = inv(S[K, K]);  W = T D;  S -= W T^T;  S[:, K] = W;  S[K, :] = W^T;  S[K, K] = -D
// and inv(A) = -S after the last block.  n^3 flops, the same work in every step.  Only the entries on and below the diagonal
// (row >= column; element (i, j) at A[i ld + j]) are read and computed; the mirror kernel negates them and writes the others.
//
// The workspace (spdinv_ws_doubles(n) doubles; NP = n rounded up to a multiple of kTile):
//     Tp [64][NP]   the panel T, COLUMN-major (Tp[c NP + i] = T[i][c]): a K-slice of a row slab is contiguous, which is how the update
//                   kernel streams it.  Rows of the pivot block, rows >= n and columns >= nb hold zeros.
//     Wn [64][NP]   -W in the same layout and with the same zeros: the update is S += Wn T^T for EVERY tile, and the zero rows of the
//                   pivot block make it leave the panel's row and column as they are (x + 0 y = x).
//     D  [64][64]   inv of the pivot block, padded with the identity; both triangles written from one sum each: exactly symmetric.
//     flag          one int: a pivot was not positive and finite.  Set once (the later pivot kernels of the call return when they
//                   see it, so do the other kernels) and counted in *fails; cleared by the first pivot kernel of a call.
//
// spdinv_pivot_kernel   one workgroup of 256.  The block's lower triangle into LDS (mirrored; padded with the identity), an unblocked
//     right-looking Cholesky there (column scaling by thread i, the trailing update over all threads), M = L^-1 by forward substitution
//     (thread j column j; the loop runs over all k < i, zeros included, so that L[i][k] is a broadcast), D[i][j] = sum_{k >= i}
//     M[k][i] M[k][j] for i >= j, written to D[i][j] and D[j][i].
// spdinv_panel_kernel   one workgroup of 256 per 64 rows of NP: the row tile lies wholly above, in or below the pivot block (both are
//     aligned to 64).  Below: T[i][c] = S[i][k0 + c] (coalesced in c, transposed into LDS at a row stride of 65 doubles: no bank
//     conflict); above: T[i][c] = S[k0 + c][i] from ROW block K (coalesced in i).  W = T D on v_mfma_f64_16x16x4_f64: a wave takes 16
//     rows x 64 columns, 4 x 16 instructions, D (stride 80 doubles) and T read from LDS; lane l hands over T[16 w + l % 16][kk + l / 16]
//     and D[kk + l / 16][16 b + l % 16] and holds W[16 w + l / 16 + 4 r][16 b + l % 16].  W goes through LDS once more so that the
//     workspace (i fastest) and the matrix (c fastest below, i fastest above) are both written in coalesced rows.  The pivot tile
//     writes zeros to the workspace and -D to the block.
// spdinv_update_kernel  THE n^3.  A workgroup of 256 owns one kTile x kTile (128 x 128) tile of the lower triangle, a wave a 64 x 64
//     quadrant: 16 sub-tiles of 16 x 16, four doubles each per lane = 64 doubles of accumulator, loaded from S (masked: row < n, column
//     <= row -- a diagonal tile computes the full square and stores its lower half), 16 matrix instructions per K-step of 4, stored.
//     Wn_I and T_J are streamed through LDS in kSlices = 4 K-slices of 16 columns: [16][kLdp = 144] doubles per operand and buffer
//     (144 = 128 + 16: the four K-rows a matrix instruction reads start 32 banks apart), two buffers = 73 728 bytes, so two
//     workgroups share a CU's 160 KiB; a thread moves four 16-byte pieces per operand and slice and has the next slice's loads in
//     flight while the matrix instructions of the current one run.  No masks on the operands: the workspace is padded with zeros.
//     The grid is the list of the lower-triangle tiles row by row (tile id = I (I + 1) / 2 + J): workgroups resident together share
//     the row slab Wn_I and read neighbouring T_J.
// spdinv_mirror_kernel  32 x 32 tiles through LDS: S[i][j] = S[j][i] = -S[i][j] for i >= j.
//
// No atomics on doubles; every sum's order is fixed by the geometry: a repeated call returns the same bits.
#include "../../include/rsparse_wrmf_hip.h"
#include "wrmf_internal.h"
#include "wrmf_device.h"

namespace rsparse_hip {
namespace {

using namespace dev;

constexpr int kNb = RSPARSE_HIP_SPDINV_BLOCK;
static_assert(kNb == 64, "the lane maps below are written for a pivot block of 64");
constexpr int kTile = 128;             // the update kernel's output tile
constexpr int kSliceK = 16;            // K-columns of a slice
constexpr int kSlices = kNb / kSliceK;
constexpr int kLdp = kTile + 16;       // doubles between the K-rows of a slice in LDS
constexpr int kLdd = kNb + 16;         // ... of D in the panel kernel
constexpr int kLdt = kNb + 1;          // ... of the transposed tiles of the panel and pivot kernels

typedef double f64x2 __attribute__((ext_vector_type(2)));

__host__ __device__ inline size_t spd_np(int n) { return ((size_t)n + kTile - 1) / kTile * kTile; }

// the tile (I, J), J <= I, of a lower triangle listed row by row: id = I (I + 1) / 2 + J (the float root, then exact steps)
__device__ __forceinline__ void tri_tile(unsigned id, int& I, int& J) {
  I = (int)((sqrtf(8.0f * (float)id + 1.0f) - 1.0f) * 0.5f);
  while ((unsigned)(I + 1) * (unsigned)(I + 2) / 2 <= id) I++;
  while ((unsigned)I * (unsigned)(I + 1) / 2 > id) I--;
  J = (int)(id - (unsigned)I * (unsigned)(I + 1) / 2);
}

struct SpdWs {
  double* Tp;
  double* Wn;
  double* D;
  int* flag;
  size_t np;
};

__global__ __launch_bounds__(256) void spdinv_pivot_kernel(const double* __restrict__ A, int n, size_t ld, int k0, SpdWs ws, int* fails) {
  __shared__ double sa[kNb * kLdt];
  __shared__ double sm[kNb * kLdt];
  const int tid = threadIdx.x;
  if (k0 == 0) {
    if (tid == 0) *ws.flag = 0;
  } else if (*ws.flag) {
    return;
  }
  const int nb = min(kNb, n - k0);
  for (int idx = tid; idx < kNb * kNb; idx += 256) {
    const int i = idx >> 6, j = idx & 63;
    double v = i == j ? 1.0 : 0.0;
    if (i < nb && j < nb) v = A[(size_t)(k0 + max(i, j)) * ld + (size_t)(k0 + min(i, j))];
    sa[i * kLdt + j] = v;
  }
  __syncthreads();
  for (int p = 0; p < kNb; p++) {
    const double d = sa[p * kLdt + p];
    if (!(d > 0.0) || !(d <= 1.79769313486231570e308)) {   // (uniform: every thread reads the same word)
      if (tid == 0) {
        *ws.flag = 1;
        atomicAdd(fails, 1);
      }
      return;
    }
    const double l = sqrt(d);
    __syncthreads();   // (everyone has read the pivot)
    if (tid >= p && tid < kNb) sa[tid * kLdt + p] = tid == p ? l : sa[tid * kLdt + p] / l;
    __syncthreads();
    const int m = kNb - 1 - p;   // trailing rows and columns p + 1 ..
    for (int idx = tid; idx < m * m; idx += 256) {
      const int i = p + 1 + idx / m, j = p + 1 + idx % m;
      if (j <= i) sa[i * kLdt + j] -= sa[i * kLdt + p] * sa[j * kLdt + p];
    }
    __syncthreads();
  }
  // M = L^-1, thread j its column: m_jj = 1 / l_jj, m_ij = -(sum_{k < i} l_ik m_kj) / l_ii
  if (tid < kNb) {
    const int j = tid;
    for (int i = 0; i < kNb; i++) {
      double s = i == j ? 1.0 : 0.0;
      for (int k = 0; k < i; k++) s -= sa[i * kLdt + k] * sm[k * kLdt + j];
      sm[i * kLdt + j] = i < j ? 0.0 : s / sa[i * kLdt + i];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < kNb * kNb; idx += 256) {
    const int i = idx >> 6, j = idx & 63;
    if (j > i) continue;
    double s = 0.0;
    for (int k = i; k < kNb; k++) s += sm[k * kLdt + i] * sm[k * kLdt + j];
    ws.D[i * kNb + j] = s;
    ws.D[j * kNb + i] = s;
  }
}

__global__ __launch_bounds__(256) void spdinv_panel_kernel(double* __restrict__ A, int n, size_t ld, int k0, SpdWs ws) {
  __shared__ double sD[kNb * kLdd];
  __shared__ double sT[kNb * kLdt];   // [c][i]
  __shared__ double sW[kNb * kLdt];   // [c][i]
  if (*ws.flag) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r0 = blockIdx.x * kNb, nb = min(kNb, n - k0);
  const size_t np = ws.np;
  if (r0 == k0) {   // the pivot tile: zeros in the workspace, -D in the block
    for (int idx = tid; idx < kNb * kNb; idx += 256) {
      const int c = idx >> 6, i = idx & 63;
      ws.Tp[(size_t)c * np + r0 + i] = 0.0;
      ws.Wn[(size_t)c * np + r0 + i] = 0.0;
      if (c <= i && i < nb) A[(size_t)(k0 + i) * ld + (size_t)(k0 + c)] = -ws.D[i * kNb + c];
    }
    return;
  }
  const bool below = r0 > k0;
  for (int idx = tid; idx < kNb * kNb; idx += 256) {
    const int hi = idx >> 6, lo = idx & 63;
    sD[hi * kLdd + lo] = ws.D[idx];
    const int i = below ? hi : lo, c = below ? lo : hi;
    double v = 0.0;
    if (r0 + i < n && c < nb) v = below ? A[(size_t)(r0 + i) * ld + (size_t)(k0 + c)] : A[(size_t)(k0 + c) * ld + (size_t)(r0 + i)];
    sT[c * kLdt + i] = v;
  }
  __syncthreads();
  for (int idx = tid; idx < kNb * kNb; idx += 256) {
    const int c = idx >> 6, i = idx & 63;
    ws.Tp[(size_t)c * np + r0 + i] = sT[c * kLdt + i];
  }
  const int r16 = lane & 15, q4 = lane >> 4;
  f64x4 acc[4];
#pragma unroll
  for (int b = 0; b < 4; b++) acc[b] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int kk = 0; kk < kNb; kk += 4) {
    const double a = sT[(kk + q4) * kLdt + 16 * wv + r16];
#pragma unroll
    for (int b = 0; b < 4; b++) acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sD[(kk + q4) * kLdd + 16 * b + r16], acc[b], 0, 0, 0);
  }
#pragma unroll
  for (int b = 0; b < 4; b++)
#pragma unroll
    for (int r = 0; r < 4; r++) sW[(16 * b + r16) * kLdt + 16 * wv + q4 + 4 * r] = acc[b][r];
  __syncthreads();
  for (int idx = tid; idx < kNb * kNb; idx += 256) {
    const int c = idx >> 6, i = idx & 63;
    ws.Wn[(size_t)c * np + r0 + i] = -sW[c * kLdt + i];
    const int hi = idx >> 6, lo = idx & 63;
    const int mi = below ? hi : lo, mc = below ? lo : hi;   // the matrix: its fastest index to the fastest thread index
    if (r0 + mi < n && mc < nb) {
      const double w = sW[mc * kLdt + mi];
      if (below) A[(size_t)(r0 + mi) * ld + (size_t)(k0 + mc)] = w;
      else A[(size_t)(k0 + mc) * ld + (size_t)(r0 + mi)] = w;
    }
  }
}

__global__ __launch_bounds__(256, 2) void spdinv_update_kernel(double* __restrict__ A, int n, size_t ld, SpdWs ws) {
  __shared__ __attribute__((aligned(16))) double sA[2][kSliceK * kLdp];   // Wn_I
  __shared__ __attribute__((aligned(16))) double sB[2][kSliceK * kLdp];   // T_J
  if (*ws.flag) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  int I, J;
  tri_tile(blockIdx.x, I, J);
  const int r16 = lane & 15, q4 = lane >> 4;
  const int row0 = I * kTile + (wv >> 1) * 64, col0 = J * kTile + (wv & 1) * 64;

  // the slices: thread t moves the rows 2 (t % 64), + 1 of the K-columns t / 64 + 4 m
  const size_t np = ws.np;
  const int lr = 2 * (tid & 63), lk = tid >> 6;
  const double* gA = ws.Wn + (size_t)lk * np + (size_t)I * kTile + lr;
  const double* gB = ws.Tp + (size_t)lk * np + (size_t)J * kTile + lr;
  f64x2 ra[4], rb[4];
  auto fetch = [&](int s) {
#pragma unroll
    for (int m = 0; m < 4; m++) {
      ra[m] = *reinterpret_cast<const f64x2*>(gA + (size_t)(s * kSliceK + 4 * m) * np);
      rb[m] = *reinterpret_cast<const f64x2*>(gB + (size_t)(s * kSliceK + 4 * m) * np);
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int m = 0; m < 4; m++) {
      *reinterpret_cast<f64x2*>(&sA[buf][(lk + 4 * m) * kLdp + lr]) = ra[m];
      *reinterpret_cast<f64x2*>(&sB[buf][(lk + 4 * m) * kLdp + lr]) = rb[m];
    }
  };
  fetch(0);

  f64x4 acc[4][4];
#pragma unroll
  for (int x = 0; x < 4; x++)
#pragma unroll
    for (int y = 0; y < 4; y++) {
      const int col = col0 + 16 * y + r16;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = row0 + 16 * x + q4 + 4 * r;
        acc[x][y][r] = (row < n && col <= row) ? A[(size_t)row * ld + col] : 0.0;
      }
    }
  stage(0);
  __syncthreads();
#pragma unroll
  for (int s = 0; s < kSlices; s++) {
    if (s + 1 < kSlices) fetch(s + 1);
    const double* pa = &sA[s & 1][q4 * kLdp + (wv >> 1) * 64 + r16];
    const double* pb = &sB[s & 1][q4 * kLdp + (wv & 1) * 64 + r16];
#pragma unroll
    for (int kk = 0; kk < kSliceK; kk += 4) {
      double a[4], b[4];
#pragma unroll
      for (int x = 0; x < 4; x++) {
        a[x] = pa[kk * kLdp + 16 * x];
        b[x] = pb[kk * kLdp + 16 * x];
      }
#pragma unroll
      for (int x = 0; x < 4; x++)
#pragma unroll
        for (int y = 0; y < 4; y++) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[x], b[y], acc[x][y], 0, 0, 0);
    }
    if (s + 1 < kSlices) {
      stage((s + 1) & 1);   // (the other buffer: its readers passed the barrier that closed slice s - 1)
      __syncthreads();
    }
  }
#pragma unroll
  for (int x = 0; x < 4; x++)
#pragma unroll
    for (int y = 0; y < 4; y++) {
      const int col = col0 + 16 * y + r16;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = row0 + 16 * x + q4 + 4 * r;
        if (row < n && col <= row) A[(size_t)row * ld + col] = acc[x][y][r];
      }
    }
}

__global__ __launch_bounds__(256) void spdinv_mirror_kernel(double* __restrict__ A, int n, size_t ld, SpdWs ws) {
  __shared__ double t[32][33];
  if (*ws.flag) return;
  int I, J;
  tri_tile(blockIdx.x, I, J);
  const int c = threadIdx.x & 31, r8 = threadIdx.x >> 5;
  const int i0 = I * 32, j0 = J * 32;
  for (int r = r8; r < 32; r += 8) {
    const int i = i0 + r, j = j0 + c;
    double v = 0.0;
    if (i < n && j <= i) {
      v = -A[(size_t)i * ld + j];
      A[(size_t)i * ld + j] = v;
    }
    t[r][c] = v;
  }
  __syncthreads();
  for (int r = r8; r < 32; r += 8) {
    const int i = j0 + r, j = i0 + c;   // the mirrored cell (i, j) = the cell (j, i) of the lower triangle
    if (j < n && i < j) A[(size_t)i * ld + j] = t[c][r];
  }
}

}  // namespace

size_t spdinv_ws_doubles(int n) { return 2 * spd_np(n) * kNb + (size_t)kNb * kNb + 2; }

hipError_t launch_spd_inverse_f64(double* A, int n, int ld, double* wsp, int* fails, hipStream_t s) {
  SpdWs ws;
  ws.np = spd_np(n);
  ws.Tp = wsp;
  ws.Wn = wsp + ws.np * kNb;
  ws.D = ws.Wn + ws.np * kNb;
  ws.flag = reinterpret_cast<int*>(ws.D + kNb * kNb);
  const unsigned nt = (unsigned)(ws.np / kTile), n32 = (unsigned)((n + 31) / 32);
  for (int k0 = 0; k0 < n; k0 += kNb) {
    spdinv_pivot_kernel<<<1, 256, 0, s>>>(A, n, (size_t)ld, k0, ws, fails);
    spdinv_panel_kernel<<<(unsigned)(ws.np / kNb), 256, 0, s>>>(A, n, (size_t)ld, k0, ws);
    spdinv_update_kernel<<<nt * (nt + 1) / 2, 256, 0, s>>>(A, n, (size_t)ld, ws);
  }
  spdinv_mirror_kernel<<<n32 * (n32 + 1) / 2, 256, 0, s>>>(A, n, (size_t)ld, ws);
  return hipGetLastError();
}

}  // namespace rsparse_hip
