"""Which kernel runs for which call: the parent's launch cascade against the plan table, over a grid.

    python profiles/topk_plan/grid_dump.py PARENT_TREE [--keep DIR]

Parent side: a scratch copy of PARENT_TREE's rsparse_amd/csrc/wrmf_topk.hip in which the two launch macros of
launch_top_product_geo print the kernel expression, LDS bytes, users, threads and grid and return (nothing before them in that
function touches the device), included into a stand-alone host program that walks the grid -- the parent's own code decides, not
a re-derivation.  New side: profiles/topk_plan/plan_dump.cpp on this tree's wrmf_topk_plan.h.  Grid: ranks {4, 30, 32, 62, 64,
126, 128, 158, 160, 256} x users {1, 32, 33, 64, 65, 128, 129, 256, 257, 131072, 131073} x every k in 1..256 x sliced / unsliced x
flagged / not x scratch given / not; then slices and scratch sizes of whole calls.  Pass: the two dumps are identical and none of
the 12 deleted instantiations occurs.  Host programs only: nothing is launched.
"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parents[2]
DEAD = [r"top_product_shared_kernel<\d+, 2, ", r"top_product_kernel<(32|64), 1, \w+, 2>", r"top_product_kernel<256, 1, \w+, 4>"]

GO = r'''#define RSP_TOPK_GO(KERN, LDS, USERS, THREADS)                                                               \
  {                                                                                                          \
    printf("%s lds=%zu users=%d threads=%d grid=%dx%d gbuf=0\n", #KERN, (size_t)(LDS), USERS, THREADS,    \
           (n_users + (USERS) - 1) / (USERS), n_slices);                                                     \
    return hipSuccess;                                                                                       \
  }
#define RSP_TOPK_GO_P(KERN, LDS, USERS, THREADS, GB)                                                         \
  {                                                                                                          \
    printf("%s lds=%zu users=%d threads=%d grid=%dx%d gbuf=%d\n", #KERN, (size_t)(LDS), USERS, THREADS,   \
           std::min((n_users + (USERS) - 1) / (USERS), user_flags ? 512 : 0x7fffffff), n_slices, (GB) != nullptr); \
    return hipSuccess;                                                                                       \
  }
'''

MAIN = r'''
#include <cstdio>
namespace rsparse_hip {
int padded_rank(int k) { return k <= 0 ? 0 : k <= 32 ? 32 : k <= 64 ? 64 : k <= 128 ? 128 : 0; }   // (wrmf_kernels.hip)
}
using namespace rsparse_hip;
int main() {
  const int ranks[] = {4, 30, 32, 62, 64, 126, 128, 158, 160, 256};
  const int users[] = {1, 32, 33, 64, 65, 128, 129, 256, 257, 131072, 131073};
  float* V = reinterpret_cast<float*>(64);   // (16-byte aligned: VEC follows the rank alone; never dereferenced)
  int flags = 0;
  for (int rank : ranks)
    for (int nu : users)
      for (int k = 1; k <= 256; k++)
        for (int sliced = 0; sliced < 2; sliced++)
          for (int flagged = 0; flagged < 2; flagged++)
            for (int scratch = 0; scratch < 2; scratch++) {
              printf("rank=%d users=%d k=%d sliced=%d flagged=%d scratch=%d: ", rank, nu, k, sliced, flagged, scratch);
              if (launch_top_product_geo(V, V, nu, 1 << 20, rank, k, nullptr, nullptr, nullptr, 0, 0.f, nullptr, nullptr, nullptr,
                                         sliced ? 2 : 1, sliced ? 4096 : 0, flagged ? &flags : nullptr, scratch ? V : nullptr) != hipSuccess)
                printf("invalid\n");
            }
  const int items[] = {100, 4095, 4096, 100000, 1000000};
  for (int rank : {32, 128, 160})
    for (int nu : users)
      for (int ni : items)
        for (int k : {1, 10, 100, 256}) {
          int si = 0;
          const int S = top_product_slices(nu, ni, k, &si);
          printf("rank=%d users=%d items=%d k=%d: S=%d slice_items=%d scratch_floats=%zu\n", rank, nu, ni, k, S, si,
                 top_product_scratch_floats(nu, ni, rank, k));
        }
  return 0;
}
'''


def run(cmd, **kw):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, **kw)
    if r.returncode != 0:
        raise SystemExit("%s\n%s" % (" ".join(map(str, cmd)), r.stderr[-4000:]))
    return r.stdout


def main(argv):
    parent = Path(argv[0]).resolve()
    tmp = Path(argv[argv.index("--keep") + 1]) if "--keep" in argv else Path(tempfile.mkdtemp())
    tmp.mkdir(parents=True, exist_ok=True)
    csrc = parent / "rsparse_amd" / "csrc"
    src = (csrc / "wrmf_topk.hip").read_text()
    a, b = src.index("#define RSP_TOPK_GO(KERN"), src.index("  // GBUF: the launcher hands a scratch")
    (tmp / "parent_dump.hip").write_text(src[:a] + GO + src[b:] + MAIN)
    # (-O0: the kernels are compiled because the file holds them, and never loaded)
    run(["hipcc", "--offload-arch=gfx950", "-O0", "-std=c++17", "-I", str(csrc), str(tmp / "parent_dump.hip"), "-o", str(tmp / "parent_dump")])
    run(["g++", "-std=c++17", "-O1", "-I", str(HERE / "rsparse_amd" / "csrc"), str(HERE / "profiles" / "topk_plan" / "plan_dump.cpp"),
         "-o", str(tmp / "plan_dump")])
    old, new = run([str(tmp / "parent_dump")]), run([str(tmp / "plan_dump")])
    (tmp / "parent_dump.txt").write_text(old)
    (tmp / "plan_dump.txt").write_text(new)
    lo, ln = old.splitlines(), new.splitlines()
    diff = [(x, y) for x, y in zip(lo, ln) if x != y]
    dead = [l for l in lo + ln if any(re.search(d, l) for d in DEAD)]
    kinds = sorted(set(re.findall(r"\((top_product\w+<[^>]+>)\)", old)))
    print("parent: %d lines, new: %d lines, %d differ; %d distinct kernels selected; lines naming a deleted instantiation: %d"
          % (len(lo), len(ln), len(diff) + abs(len(lo) - len(ln)), len(kinds), len(dead)))
    for x, y in diff[:10]:
        print("  parent", x, "\n  new   ", y)
    for k in kinds:
        print("   ", k)
    return 0 if not diff and len(lo) == len(ln) and not dead else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
