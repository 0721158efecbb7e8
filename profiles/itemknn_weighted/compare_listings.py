"""The binary ItemKNN kernels of two `hipcc -S --cuda-device-only` listings of wrmf_itemknn.hip, instruction by instruction:

    python profiles/itemknn_weighted/compare_listings.py parent.s this.s

pairs the parent's `knn_*_kernel<true / false>` with this tree's `<1 / 0>` and prints, per kernel, the instruction counts and
whether the opcode sequences and the full instruction texts agree."""
import difflib
import re
import sys


def kernels(path):
    out = {}
    for m in re.finditer(r"^(_ZN\w+):[^\n]*\n(.*?)\n\s+s_endpgm", open(path).read(), re.S | re.M):
        # (a branch label carries the number of its function within the file: .LBB4_10 -> .LBB_10)
        body = [re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].strip()) for line in m.group(2).splitlines()]
        out[m.group(1)] = [line for line in body if line and not line.startswith(".") and not line.endswith(":")]
    return out


def main():
    par, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    pairs = {"scatter, fit": ("knn_scatter_kernelILb1E", "knn_scatter_kernelILi1E"), "scatter, lists": ("knn_scatter_kernelILb0E", "knn_scatter_kernelILi0E"),
             "select, fit": ("knn_select_kernelILb1E", "knn_select_kernelILi1E"), "select, lists": ("knn_select_kernelILb0E", "knn_select_kernelILi0E"),
             "mask": ("knn_mask_kernel", "knn_mask_kernel")}
    ops = lambda body: [line.split()[0] for line in body]
    for name, (b, a) in pairs.items():
        ib, ia = par[[k for k in par if b in k][0]], new[[k for k in new if a in k][0]]
        diff = [d for d in difflib.unified_diff(ops(ib), ops(ia), lineterm="", n=0) if not d.startswith(("@@", "---", "+++"))]
        print("%-15s parent %5d instructions, this tree %5d; opcode sequence %s; full text %s" % (
            name, len(ib), len(ia), "the same" if not diff else "differs in %d lines: %s" % (len(diff), " ".join(diff[:24])),
            "the same" if ib == ia else "differs"))


if __name__ == "__main__":
    main()
