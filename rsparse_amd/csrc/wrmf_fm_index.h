// What wrmf_fm.hip and wrmf_ftrl.hip share: the layout of the backward index that rsparse_hip_fm_index_device builds (one sort, one
// layout, two readers) and the stated exponential of the definitions (rsparse_amd/bpr.py: bpr_exp).
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace rsparse_hip {
namespace fmidx {

constexpr int kFmMagic = 0x464d4958;

// the workspace, in int32 units: header (magic, n_steps, nnz, n_seg), step_seg[n_steps + 1], step_ch[n_steps + 1], then
// spay[nnz], sk[nnz], seg_col[nnz], seg_ptr[nnz + 1], choff[nnz + 1] (n_seg <= nnz bounds the last three)
struct FmIndex {
  int32_t *hdr, *step_seg, *step_ch, *sk, *seg_col, *seg_ptr, *choff;
  uint32_t* spay;
  size_t ints;
};
inline FmIndex fm_index_of(void* ws, int64_t nnz, int n_steps) {
  FmIndex ix;
  int32_t* b = static_cast<int32_t*>(ws);
  const size_t n = (size_t)nnz, ns = (size_t)n_steps + 1, head = (4 + 2 * ns + 3) / 4 * 4;
  ix.hdr = b; ix.step_seg = b + 4; ix.step_ch = b + 4 + ns;
  ix.spay = reinterpret_cast<uint32_t*>(b + head);
  ix.sk = b + head + n; ix.seg_col = b + head + 2 * n; ix.seg_ptr = b + head + 3 * n; ix.choff = b + head + 4 * n + 1;
  ix.ints = head + 5 * n + 2;
  return ix;
}

__device__ __forceinline__ int fm_col(int j, int n_feat) { return j < 0 ? 0 : (j >= n_feat ? n_feat - 1 : j); }   // (never outside the parameters)

// E(d) of the definition (rsparse_amd/bpr.py: bpr_exp): plain arithmetic, no library exponential
__device__ __forceinline__ double fm_exp(double d) {
  d = d < -40.0 ? -40.0 : (d > 40.0 ? 40.0 : d);
  const double kk = rint(d * 1.4426950408889634);
  const double r = (d - kk * 6.93147180369123816490e-01) - kk * 1.90821492927058770002e-10;
  double q = 1.0 / 6227020800.0;
  q = q * r + 1.0 / 479001600.0;
  q = q * r + 1.0 / 39916800.0;
  q = q * r + 1.0 / 3628800.0;
  q = q * r + 1.0 / 362880.0;
  q = q * r + 1.0 / 40320.0;
  q = q * r + 1.0 / 5040.0;
  q = q * r + 1.0 / 720.0;
  q = q * r + 1.0 / 120.0;
  q = q * r + 1.0 / 24.0;
  q = q * r + 1.0 / 6.0;
  q = q * r + 1.0 / 2.0;
  q = q * r + 1.0;
  q = q * r + 1.0;
  return ldexp(q, (int)kk);
}

}  // namespace fmidx
}  // namespace rsparse_hip
