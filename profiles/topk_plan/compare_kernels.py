"""Compare the gfx950 device listing of wrmf_topk.hip with the parent's, kernel by kernel.

    python profiles/topk_plan/compare_kernels.py PARENT_TREE [--keep DIR] [--table]

Both trees' wrmf_topk.hip are compiled with `-S --cuda-device-only` and the build's flags (profiles/device_helpers/
compare_listings.py does the compiling and masks `__hip_cuid_*`), the listings are split per kernel symbol and every kernel of
this tree is compared byte for byte with the parent's kernel of the same name.  top_product_shared_kernel lost its UB template
parameter (always 1): the parent's symbols `...shared_kernelILi<KP>ELi1ELb<VEC>EE` are renamed to the new spelling before the
comparison, and the ordinal of a kernel within its listing, which numbers its local labels (`.LBB13_2`, `.Lfunc_end13`), is
masked: the kernels are emitted in another order.  Kernels only the parent has are listed as deleted.  --table prints, per kernel of this tree, VGPRs / AGPR offset /
SGPRs / LDS / scratch on both sides.  A compile, not a run: no GPU is needed.  Exit status 0 = every surviving kernel equal.
"""
import re
import sys
import tempfile
import time
from pathlib import Path

HERE = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(HERE / "profiles" / "device_helpers"))
import compare_listings as CL  # noqa: E402

NAME = "wrmf_topk.hip"


def main(argv):
    keep = Path(argv[argv.index("--keep") + 1]) if "--keep" in argv else Path(tempfile.mkdtemp())
    parent = argv[0]
    texts = {}
    for side, tree in (("parent", parent), ("new", HERE)):
        (keep / side).mkdir(parents=True, exist_ok=True)
        out = keep / side / (NAME + ".s")
        if side == "new" or not out.exists():
            t0 = time.time()
            CL.listing(tree, NAME, out)
            print("%-6s compiled in %.1f s" % (side, time.time() - t0))
        t = re.sub(r"\.L(func_begin|func_end|JTI)\d+", r".L\1N", CL.masked(out))
        texts[side] = re.sub(r"[ \t]+;", " ;", re.sub(r"(\.L|\b)BB\d+_(\d+)", r"\1BBN_\2", t))   # (labels, and the comments naming them)
    texts["parent"] = re.sub(r"(top_product_shared_kernelILi\d+E)Li1E", r"\1", texts["parent"])
    ka, kb = CL.kernels(texts["parent"]), CL.kernels(texts["new"])
    differ = [k for k in kb if ka.get(k) != kb[k]]
    print("parent: %d kernels, %d lines; new: %d kernels, %d lines" % (len(ka), texts["parent"].count("\n"), len(kb),
                                                                         texts["new"].count("\n")))
    print("deleted (%d):" % len(set(ka) - set(kb)))
    for k in sorted(set(ka) - set(kb)):
        print("   ", k)
    if "--table" in argv:
        print("kernel | VGPRs | AGPR offset | SGPRs | LDS | scratch   (parent -> new where they differ)")
        for k in sorted(kb):
            a, b = ka.get(k, ("", {}))[1], kb[k][1]
            print(k, "|", " | ".join(b[r] if a.get(r) == b[r] else "%s -> %s" % (a.get(r), b[r])
                                     for r in (CL.RES[0], CL.RES[2], CL.RES[1], CL.RES[3], CL.RES[4])))
    for k in differ:
        print("DIFFERS:", k, ka.get(k, ("", None))[1], kb[k][1])
    print("%d of %d surviving kernels byte-equal to the parent's" % (len(kb) - len(differ), len(kb)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
