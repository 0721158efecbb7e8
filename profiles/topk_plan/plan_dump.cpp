// Decision dump of the launch-plan table (rsparse_amd/csrc/wrmf_topk_plan.h) over the grid of profiles/topk_plan/README.md,
// in the spelling of the parent's launch cascade: kernel expression, LDS bytes, users per workgroup, threads, grid.
// Plain host C++:  g++ -std=c++17 -O1 -I rsparse_amd/csrc profiles/topk_plan/plan_dump.cpp -o plan_dump
#include <cstdio>

#include "wrmf_topk_plan.h"

using namespace rsparse_hip;

int main() {
  const int ranks[] = {4, 30, 32, 62, 64, 126, 128, 158, 160, 256};
  const int users[] = {1, 32, 33, 64, 65, 128, 129, 256, 257, 131072, 131073};
  for (int rank : ranks)
    for (int nu : users)
      for (int k = 1; k <= 256; k++)
        for (int sliced = 0; sliced < 2; sliced++)
          for (int flagged = 0; flagged < 2; flagged++)
            for (int scratch = 0; scratch < 2; scratch++) {
              printf("rank=%d users=%d k=%d sliced=%d flagged=%d scratch=%d: ", rank, nu, k, sliced, flagged, scratch);
              TopLaunch l;
              if (!top_plan_launch(&l, 0, nu, rank, k, sliced ? 2 : 1, sliced ? 4096 : 0, flagged != 0, scratch != 0)) {
                printf("invalid\n");
                continue;
              }
              const TopGeo& g = l.geo;
              const char* vec = rank % 4 == 0 ? "true" : "false";
              char kern[96];
              if (g.family == kTopPipe && g.gbuf) snprintf(kern, sizeof kern, "(top_product_pipe_kernel<%d, %d, %s, true>)", g.KP, g.UB, vec);
              else if (g.family == kTopPipe) snprintf(kern, sizeof kern, "(top_product_pipe_kernel<%d, %d, %s>)", g.KP, g.UB, vec);
              else if (g.family == kTopShared) snprintf(kern, sizeof kern, "(top_product_shared_kernel<%d, %d, %s>)", g.KP, g.UB, vec);
              else snprintf(kern, sizeof kern, "(top_product_kernel<%d, %d, %s, %d>)", g.KP, g.UB, vec, g.W);
              printf("%s lds=%zu users=%d threads=%d grid=%dx%d gbuf=%d\n", kern, g.lds, g.users, g.threads, l.grid_x, l.n_slices, (int)g.gbuf);
            }
  // the call level: slices and scratch
  const int items[] = {100, 4095, 4096, 100000, 1000000};
  for (int rank : {32, 128, 160})
    for (int nu : users)
      for (int ni : items)
        for (int k : {1, 10, 100, 256}) {
          const TopPlan p = top_product_plan(nu, ni, rank, k, k, false);
          printf("rank=%d users=%d items=%d k=%d: S=%d slice_items=%d scratch_floats=%zu\n", rank, nu, ni, k, p.n_slices, p.slice_items,
                 p.scratch_floats);
        }
  return 0;
}
