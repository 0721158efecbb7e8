// Stand-alone walk of rsparse_amd/csrc/wrmf_ctx_layout.h over the lattice of tests/test_ctx_layout.py, meant to be built with
// -fsanitize=address,undefined and run by itself (README.md in this directory has the command and the output):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all layout_walk.cpp -o layout_walk && ./layout_walk
// Every (n, ranks, sub-blocks, count vector) cell: the edges are monotone from 0 to n, to_storage is a bijection onto the rows
// that the sub-blocks own (no padding row is hit), and make_subs' slicing of the pointers stays inside them.
#include <cstdio>
#include <cstdlib>

#include "../../rsparse_amd/csrc/wrmf_ctx_layout.h"

using namespace rsparse_hip;

static std::vector<int64_t> counts_of(int kind, int64_t n, int ws) {
  std::vector<int64_t> c((size_t)n, 3);
  if (kind == 1) std::fill(c.begin(), c.end(), 0);
  if (kind == 2 && n) c[(size_t)(n / 3)] = std::max<int64_t>(3, 3 * (n - 1));
  if (kind == 3 && n) {
    for (int64_t i = 0; i < std::min<int64_t>(2, n); i++) c[(size_t)i] = c[(size_t)(n - 1 - i)] = 0;
    for (int r = 1; r < ws; r++) {
      const int64_t m = n * r / ws;
      for (int64_t i = std::max<int64_t>(0, m - 2); i < std::min(n, m + 3); i++) c[(size_t)i] = 0;
    }
  }
  return c;
}

#define REQUIRE(cond)                                                                                   \
  do {                                                                                                  \
    if (!(cond)) {                                                                                      \
      std::printf("FAILED %s at n=%lld ws=%d n_sub=%d kind=%d\n", #cond, (long long)n, ws, n_sub, kind); \
      return 1;                                                                                         \
    }                                                                                                   \
  } while (0)

int main() {
  const int64_t ns[] = {0, 1, 7, 400};
  const int wss[] = {1, 2, 3, 5, 8}, n_subs[] = {1, 2, 7, 40};
  long cells = 0, ids = 0, empty_ranks = 0, padding = 0;
  for (int64_t n : ns)
    for (int ws : wss)
      for (int n_sub : n_subs)
        for (int kind = 0; kind < 4; kind++) {
          const std::vector<int64_t> c = counts_of(kind, n, ws);
          std::vector<int32_t> p((size_t)n + 1, 0);
          for (int64_t i = 0; i < n; i++) p[(size_t)i + 1] = p[(size_t)i] + (int32_t)c[(size_t)i];
          REQUIRE(check_col_ptrs(p.data(), n, "p").empty());
          const std::vector<int64_t> e = balanced_edges(p.data(), n, ws);
          REQUIRE((int)e.size() == ws + 1 && e[0] == 0 && e[(size_t)ws] == n);
          for (int r = 0; r < ws; r++) {
            REQUIRE(e[(size_t)r] <= e[(size_t)r + 1]);
            empty_ranks += e[(size_t)r] == e[(size_t)r + 1];
          }
          Lay lay;
          lay.init(n, e, n_sub);
          REQUIRE(lay.rows == (int64_t)ws * n_sub * lay.Bs && lay.Bs >= 1);
          std::vector<int> owned((size_t)lay.rows, 0), hit((size_t)lay.rows, 0);
          int64_t n_owned = 0;
          for (int r = 0; r < ws; r++)
            for (int j = 0; j < n_sub; j++) {
              int64_t c0, c1;
              lay.sub_rows(r, j, c0, c1);
              REQUIRE(0 <= c0 && c0 <= c1 && c1 - c0 <= lay.Bs && lay.b0[(size_t)r] + c1 <= lay.b1[(size_t)r]);
              REQUIRE(lay.sub_start(r, j) == lay.slab_start(j) + (int64_t)r * lay.Bs);
              for (int64_t l = c0; l < c1; l++) {
                const int64_t s = lay.sub_start(r, j) + (l - c0);
                REQUIRE(s >= 0 && s < lay.rows);
                owned[(size_t)s]++;
                REQUIRE(lay.to_storage(lay.b0[(size_t)r] + l) == s);
              }
              n_owned += c1 - c0;
              // what make_subs reads of the pointers for this sub-block
              const int64_t lo = p[(size_t)(lay.b0[(size_t)r] + c0)], hi = p[(size_t)(lay.b0[(size_t)r] + c1)];
              REQUIRE(0 <= lo && lo <= hi && hi <= p[(size_t)n]);
            }
          REQUIRE(n_owned == n);
          for (int64_t g = 0; g < n; g++) {
            const int64_t s = lay.to_storage(g);
            REQUIRE(s >= 0 && s < lay.rows);
            hit[(size_t)s]++;
          }
          for (int64_t s = 0; s < lay.rows; s++) {
            REQUIRE(owned[(size_t)s] <= 1 && hit[(size_t)s] == owned[(size_t)s]);
            padding += owned[(size_t)s] == 0;
          }
          cells++;
          ids += n;
        }
  // the refusals of the pointer check
  const int32_t from_one[] = {1, 2, 2}, decreasing[] = {0, 3, 2}, fine[] = {0, 1, 2}, other_total[] = {0, 1, 3}, none[] = {0};
  int bad = 0;
  bad += check_matrix_ptrs(from_one, 2, fine, 2).empty();
  bad += check_matrix_ptrs(fine, 2, decreasing, 2).empty();
  bad += check_matrix_ptrs(fine, 2, other_total, 2).empty();
  bad += !check_matrix_ptrs(fine, 2, fine, 2).empty();
  bad += !check_matrix_ptrs(none, 0, none, 0).empty();
  if (bad) {
    std::printf("FAILED pointer check: %d wrong answers\n", bad);
    return 1;
  }
  std::printf("layout walk ok: %ld cells, %ld ids mapped, %ld ranks without rows, %ld padding rows never hit, pointer check 5 / 5\n",
              cells, ids, empty_ranks, padding);
  return 0;
}
