"""The top-k product through two builds of the library: results bit for bit, and call times side by side.

    python profiles/topk_plan/topk_ab.py run LIB.so OUT.npz          (one library, one process: every result array of the shapes)
    python profiles/topk_plan/topk_ab.py compare A.npz B.npz
    python profiles/topk_plan/topk_ab.py ab PARENT.so OUTDIR         (run parent, run new -- a child process each --, compare)
    python profiles/topk_plan/topk_ab.py time PARENT.so OUT.json     (both libraries in one process, alternating, on one device)

Bitwise: the geometry cases of tests/test_top_product.py (every kernel the plan can select, with and without 16-byte staging, the
band edges) without and with a not_recommend matrix, exclusions and a global mean, and the integer-valued tie cases at
k = 2 / 7 / 40 / 88 and 70 / 300 / 40 users, through the host entry rsparse_hip_top_product; inputs are seeded.
Timing: one shape per live kernel family through rsparse_hip_top_product_device; a warm-up call, then REPS timed calls per library,
parent and new alternating, each call ended by a device synchronise.  Criterion per shape: the new median does not exceed the
parent's median by more than the parent's own max - min.
"""
import ctypes
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
NEW = ROOT / "rsparse_amd" / "lib" / "librsparse_wrmf_hip.so"

c_int, c_uint, c_dbl, vp_t = ctypes.c_int, ctypes.c_uint, ctypes.c_double, ctypes.c_void_p
# (the parent has no plan entry: only the entries used here are bound)
SIG = {"rsparse_hip_top_product": [vp_t, vp_t, c_int, c_int, c_int, c_uint, c_uint, vp_t, vp_t, vp_t, c_int, c_dbl, vp_t, vp_t],
       "rsparse_hip_top_product_device": [vp_t, vp_t, c_int, c_int, c_int, c_int, vp_t, vp_t, vp_t, c_int, c_dbl, vp_t, vp_t, vp_t]}


def load(path):
    lib = ctypes.CDLL(str(path))
    for name, args in SIG.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = c_int, args
    lib.rsparse_hip_last_error.restype = ctypes.c_char_p
    return lib


def vp(a):
    return None if a is None else a.ctypes.data_as(vp_t)


def host_call(lib, x, y, k, nr=None, exclude=(), glob_mean=0.0):
    import scipy.sparse as sp
    nrow, rank = x.shape
    nc = y.shape[1]
    xf, yf = np.asfortranarray(x, dtype=np.float64), np.asfortranarray(y, dtype=np.float64)
    res = np.zeros((nrow, k), dtype=np.int32, order="F")
    sc = np.zeros((nrow, k), dtype=np.float64, order="F")
    p = j = None
    if nr is not None:
        nr = sp.csr_matrix(nr)
        nr.sort_indices()
        p, j = nr.indptr.astype(np.int32), nr.indices.astype(np.int32)
    ex = np.asarray(list(exclude), dtype=np.int32)
    rc = lib.rsparse_hip_top_product(vp(xf), vp(yf), nrow, nc, rank, k, 1, vp(p), vp(j), vp(ex) if ex.size else None, int(ex.size),
                                     float(glob_mean), vp(res), vp(sc))
    if rc:
        raise RuntimeError(lib.rsparse_hip_last_error().decode())
    return res, sc


def run(libpath, out):
    import scipy.sparse as sp
    import importlib.util
    spec = importlib.util.spec_from_file_location("ttp", ROOT / "tests" / "test_top_product.py")
    # (the shape list lives with the tests; importing the module needs pytest and the oracle, both in the tree's environment)
    ttp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ttp)
    lib = load(libpath)
    res = {}
    for rank, nr, nc, k, geo in ttp._geometry_cases():
        rng = np.random.default_rng(7 * rank + k + nr)
        x, y = rng.standard_normal((nr, rank)), rng.standard_normal((rank, nc))
        notrec = sp.random(nr, nc, density=0.03, random_state=5, format="csr")
        for tag, kw in (("plain", {}), ("lists", dict(nr=notrec, exclude=[2, 9, nc], glob_mean=3.5))):
            i, s = host_call(lib, x, y, k, **kw)
            res["%s (%d,%d,%d,%d)/%s/res" % (geo, rank, nr, nc, k, tag)] = i
            res["%s (%d,%d,%d,%d)/%s/scores" % (geo, rank, nr, nc, k, tag)] = s
    for k in (2, 7, 40, 88):
        rng = np.random.default_rng(100 + k)
        for n_users in (70, 300, 40):
            x = rng.integers(0, 3, (n_users, 4)).astype(np.float64)
            y = rng.integers(0, 3, (4, 1500)).astype(np.float64)
            nr = sp.random(n_users, 1500, density=0.02, format="csr", random_state=np.random.RandomState(k))
            for tag, kw in (("plain", {}), ("lists", {"nr": nr, "exclude": [3, 77, 1400]})):
                i, s = host_call(lib, x, y, k, **kw)
                res["ties k=%d users=%d/%s/res" % (k, n_users, tag)] = i
                res["ties k=%d users=%d/%s/scores" % (k, n_users, tag)] = s
    np.savez(out, **res)
    print("wrote %s: %d arrays from %s" % (out, len(res), libpath))
    return 0


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def compare(a, b):
    da, db = np.load(a), np.load(b)
    diff = [k for k in da.files if k not in db.files or da[k].shape != db[k].shape or not np.array_equal(bits(da[k]), bits(db[k]))]
    diff += [k for k in db.files if k not in da.files]
    print("%d arrays, %d differ%s" % (len(da.files), len(diff), "".join("\n  " + d for d in diff[:20])))
    return 1 if diff else 0


def ab(parent_lib, outdir):
    outdir = Path(outdir)
    outdir.mkdir(parents=True, exist_ok=True)
    for name, lib in (("parent", parent_lib), ("new", NEW)):
        rc = subprocess.call([sys.executable, __file__, "run", str(lib), str(outdir / (name + ".npz"))])
        if rc:   # (nothing more is started on the device after a failed run)
            return rc
    return compare(outdir / "parent.npz", outdir / "new.npz")


# name, users, items, rank, k: GBUF (the shapes of profiles/r06/r6topk_ab3_*), sliced two-tile, sliced tile per wave, shared, KP = 256
SHAPES = [("gbuf k=10", 262144, 1000000, 128, 10), ("gbuf k=100", 262144, 1000000, 128, 100),
          ("sliced pipe", 1000, 1000000, 128, 10), ("sliced tile per wave", 1, 1000000, 128, 10),
          ("shared", 100, 1000000, 128, 90), ("rank 160 (KP 256)", 100000, 200000, 160, 10)]


def timing(parent_lib, out):
    import torch
    libs = (("parent", load(parent_lib)), ("new", load(NEW)))
    dev = torch.device("cuda", 0)
    report, ok = [], True
    for name, nu, ni, rank, k in SHAPES:
        g = torch.Generator(device=dev).manual_seed(nu + ni + k)
        U = torch.randn((nu, rank), generator=g, device=dev, dtype=torch.float32)
        V = torch.randn((ni, rank), generator=g, device=dev, dtype=torch.float32)
        res = torch.zeros((nu, k), dtype=torch.int32, device=dev)
        sc = torch.zeros((nu, k), dtype=torch.float32, device=dev)
        outs = {}

        def call(lib):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = lib.rsparse_hip_top_product_device(U.data_ptr(), V.data_ptr(), nu, ni, rank, k, None, None, None, 0, 0.0, res.data_ptr(),
                                                    sc.data_ptr(), None)
            torch.cuda.synchronize()
            if rc:
                raise RuntimeError(lib.rsparse_hip_last_error().decode())
            return time.perf_counter() - t0

        for lname, lib in libs:   # warm-up, and the results of the timed shape bit for bit
            call(lib)
            outs[lname] = (res.cpu().numpy().copy(), sc.cpu().numpy().copy())
        reps = 5 if call(libs[0][1]) > 0.05 else 9   # (a probe, not recorded)
        times = {"parent": [], "new": []}
        for r in range(reps):
            for lname, lib in libs:
                times[lname].append(call(lib))
        equal = all(np.array_equal(bits(a), bits(b)) for a, b in zip(outs["parent"], outs["new"]))
        pm, nm = float(np.median(times["parent"])), float(np.median(times["new"]))
        spread = max(times["parent"]) - min(times["parent"])
        row = dict(shape=name, users=nu, items=ni, rank=rank, k=k, parent_ms=[round(1e3 * t, 3) for t in times["parent"]],
                   new_ms=[round(1e3 * t, 3) for t in times["new"]], parent_median_ms=round(1e3 * pm, 3), new_median_ms=round(1e3 * nm, 3),
                   parent_spread_ms=round(1e3 * spread, 3), within=bool(nm <= pm + spread), results_bitwise_equal=bool(equal))
        ok = ok and row["within"] and equal
        report.append(row)
        print(json.dumps(row), flush=True)
        del U, V, res, sc
    Path(out).write_text(json.dumps(report, indent=1))
    return 0 if ok else 1


if __name__ == "__main__":
    cmd = sys.argv[1]
    sys.exit(run(sys.argv[2], sys.argv[3]) if cmd == "run" else compare(sys.argv[2], sys.argv[3]) if cmd == "compare"
             else ab(sys.argv[2], sys.argv[3]) if cmd == "ab" else timing(sys.argv[2], sys.argv[3]))
