// The host-only pieces of the multi-GPU context (wrmf_ctx.cpp): who owns which rows, where they are stored, and the check of
// the caller's column pointers.  No HIP in here: tests/ctx_layout_shim.cpp compiles this header with g++ alone and compares it
// with engine.balanced_bounds / engine.Layout (tests/test_ctx_layout.py).
#ifndef RSPARSE_WRMF_CTX_LAYOUT_H
#define RSPARSE_WRMF_CTX_LAYOUT_H

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace rsparse_hip {

// ---- who owns which rows, and where they are stored (engine.Layout) ----
struct Lay {
  int64_t n = 0;
  int ws = 1, n_sub = 1;
  std::vector<int64_t> b0, b1;   // block of rank r = [b0[r], b1[r])
  int64_t Bs = 1, rows = 0;
  void init(int64_t n_, const std::vector<int64_t>& edges, int n_sub_) {
    n = n_; ws = (int)edges.size() - 1; n_sub = std::max(1, n_sub_);
    b0.assign(edges.begin(), edges.end() - 1);
    b1.assign(edges.begin() + 1, edges.end());
    int64_t biggest = 1;
    for (int r = 0; r < ws; r++) biggest = std::max(biggest, b1[r] - b0[r]);
    Bs = (biggest + n_sub - 1) / n_sub;
    rows = (int64_t)ws * n_sub * Bs;
  }
  void sub_rows(int r, int j, int64_t& c0, int64_t& c1) const {   // local rows of sub-block j of rank r
    const int64_t nr = b1[r] - b0[r];
    c0 = std::min(nr, (int64_t)j * Bs);
    c1 = std::min(nr, (int64_t)(j + 1) * Bs);
  }
  int64_t sub_start(int r, int j) const { return (int64_t)j * ws * Bs + (int64_t)r * Bs; }
  int64_t slab_start(int j) const { return (int64_t)j * ws * Bs; }
  int64_t to_storage(int64_t g) const {
    // the LAST block whose start is <= g (empty blocks share their start with the next one)
    const int r = (int)(std::upper_bound(b0.begin(), b0.end(), g) - b0.begin()) - 1;
    const int64_t loc = g - b0[r], j = loc / Bs;
    return j * ((int64_t)ws * Bs) + (int64_t)r * Bs + (loc - j * Bs);
  }
};

// contiguous blocks balanced by non-zeros: rank r starts where the prefix sum of the row lengths first reaches r / ws of the
// total (engine.balanced_bounds)
inline std::vector<int64_t> balanced_edges(const int32_t* p, int64_t n, int ws) {
  std::vector<int64_t> e((size_t)ws + 1, n);
  e[0] = 0;
  if (ws <= 1 || n == 0) return e;
  const int64_t total = (int64_t)p[n] - (int64_t)p[0];
  for (int r = 1; r < ws; r++) {
    if (total > 0) {
      const int64_t target = total * r / ws + (int64_t)p[0];
      // first row i with prefix (p[i + 1]) >= target, + 1
      const int32_t* it = std::lower_bound(p + 1, p + n + 1, target, [](int32_t a, int64_t t) { return (int64_t)a < t; });
      e[(size_t)r] = std::min<int64_t>(n, (int64_t)(it - (p + 1)) + 1);
    } else {
      e[(size_t)r] = n * r / ws;
    }
  }
  for (int r = 1; r <= ws; r++) e[(size_t)r] = std::max(e[(size_t)r], e[(size_t)r - 1]);
  return e;
}

// The n + 1 column pointers of one orientation: from 0 and non-decreasing (the rule of the single-GPU handles; that there are at
// most INT32_MAX entries is the pointers' type).  "" = fine, else what is wrong with the array `name`.  Everything the layout
// and the sub-block copies size from the pointers is safe behind this check.
inline std::string check_col_ptrs(const int32_t* p, int64_t n, const char* name) {
  if (!p) return std::string(name) + " is NULL";
  if (n < 0) return std::string(name) + ": negative number of columns";
  if (p[0] != 0) return std::string(name) + " must start at 0";
  for (int64_t c = 0; c < n; c++)
    if (p[c + 1] < p[c]) return std::string(name) + " decreases at column " + std::to_string(c);
  return "";
}

// both orientations of one matrix: each array by itself, and the same number of non-zeros in the two
inline std::string check_matrix_ptrs(const int32_t* ui_p, int64_t n_item, const int32_t* iu_p, int64_t n_user) {
  std::string e = check_col_ptrs(ui_p, n_item, "ui_p");
  if (e.empty()) e = check_col_ptrs(iu_p, n_user, "iu_p");
  if (e.empty() && ui_p[n_item] != iu_p[n_user]) e = "ui_p and iu_p hold different numbers of non-zeros";
  return e;
}

}  // namespace rsparse_hip
#endif  // RSPARSE_WRMF_CTX_LAYOUT_H
