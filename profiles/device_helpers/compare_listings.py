"""Compare the gfx950 device listings of two trees, source by source.

    python profiles/device_helpers/compare_listings.py PARENT_TREE [wrmf_X.hip ...] [--keep DIR]

Every `.hip` source of `rsparse_amd/build.py` (or the ones named) is compiled with `-S --cuda-device-only` and the build's
flags (`EXTRA_FLAGS` included) in `rsparse_amd/csrc/` of this tree and of PARENT_TREE (a `git worktree` of the parent commit);
`__hip_cuid_<hash>`, which hipcc derives from the source's path, is masked and the two texts are compared byte for byte.
For a listing that differs, the kernels whose text differs are named with their register, LDS and scratch figures on both
sides.  A compile, not a run: no GPU is needed.  --keep DIR keeps the listings (and reuses the parent's on a later call).
"""
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

HERE = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(HERE))
from rsparse_amd.build import EXTRA_FLAGS, FLAGS, SRC  # noqa: E402

RES = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_accum_offset", ".amdhsa_group_segment_fixed_size",
       ".amdhsa_private_segment_fixed_size")


def listing(tree, name, out):
    csrc = Path(tree) / "rsparse_amd" / "csrc"
    extra = [f.replace(str(HERE), str(Path(tree).resolve())) for f in EXTRA_FLAGS.get(name, [])]
    r = subprocess.run(["hipcc", *FLAGS, *extra, "-S", "--cuda-device-only", name, "-o", str(out)], cwd=csrc,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s in %s:\n%s" % (name, tree, r.stderr[-4000:]))


def masked(path):
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", Path(path).read_text())


def kernels(text):
    """name -> (code text, {resource: value}) for every kernel of a listing"""
    out = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n([\s\S]*?)^\s*\.end_amdhsa_kernel", text, re.M):
        body = m.group(2)
        out[m.group(1)] = (body, {k: re.search(re.escape(k) + r" (\d+)", body).group(1) for k in RES if k + " " in body})
    return out


def main(argv):
    keep = Path(argv[argv.index("--keep") + 1]) if "--keep" in argv else None
    args = [a for i, a in enumerate(argv) if a != "--keep" and (i == 0 or argv[i - 1] != "--keep")]
    parent = args[0]
    names = args[1:] or [s.name for s in SRC if s.suffix == ".hip"]
    tmp = keep or Path(tempfile.mkdtemp())
    (tmp / "parent").mkdir(parents=True, exist_ok=True)
    (tmp / "new").mkdir(parents=True, exist_ok=True)

    def one(name):
        a, b = tmp / "parent" / (name + ".s"), tmp / "new" / (name + ".s")
        if not a.exists():
            listing(parent, name, a)
        try:
            listing(HERE, name, b)
        except RuntimeError as e:
            return name, 0, "    does not compile: " + str(e)[-1500:]
        ta, tb = masked(a), masked(b)
        if ta == tb:
            return name, ta.count("\n"), None
        ka, kb = kernels(ta), kernels(tb)
        rep = []
        for k in sorted(set(ka) | set(kb)):
            if ka.get(k) != kb.get(k):
                rep.append("    %s\n      parent %s\n      new    %s" % (k, ka.get(k, ("", None))[1], kb.get(k, ("", None))[1]))
        return name, ta.count("\n"), "\n".join(rep) or "    (differs outside the kernels)"

    with ThreadPoolExecutor(max_workers=8) as ex:
        res = list(ex.map(one, names))
    equal = sum(r[2] is None for r in res)
    for name, n, rep in res:
        print("%-22s %8d lines  %s" % (name, n, "equal" if rep is None else "DIFFERS in\n" + rep))
    print("%d of %d listings equal (%d lines)" % (equal, len(res), sum(r[1] for r in res)))
    return 0 if equal == len(res) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
