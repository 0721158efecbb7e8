"""Every C-ABI entry that exists in float and in double, through two builds of the library, compared bit for bit.

    RSPARSE_HIP_LIB=parent.so python profiles/capi_precisions/capi_ab.py run parent.npz
    python profiles/capi_precisions/capi_ab.py run new.npz                       (a fresh process per library)
    python profiles/capi_precisions/capi_ab.py compare parent.npz new.npz
    python profiles/capi_precisions/capi_ab.py ab parent.so OUTDIR               (the three steps; a child process per run)

Inputs are seeded; every output array, scalar and return code is recorded under a name that says which entry and variant
produced it.  Shapes: 300 x 200 with about 3000 non-zeros, one empty column and one empty row, and the same shape with no
non-zero; rank 8 without biases, rank 10 (8 + 2) with; the lengths 0, 1, 1024, 1025 around the 1024 partial slots of the sums.
"""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

N_ROWS, N_COLS = 300, 200
DTYPES = (("f32", np.float32), ("f64", np.float64))


def matrices(rng):
    import scipy.sparse as sp
    m = sp.random(N_ROWS, N_COLS, density=0.05, format="csc", random_state=np.random.RandomState(5),
                  data_rvs=lambda n: rng.integers(1, 6, n).astype(np.float64)).tolil()
    m[:, 17] = 0   # one empty column
    m[41, :] = 0   # one empty row
    m = sp.csc_matrix(m)
    m.eliminate_zeros()
    m.sort_indices()
    return {"A": m, "Z": sp.csc_matrix((N_ROWS, N_COLS), dtype=np.float64)}


def slots(m):
    return m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data.astype(np.float64)


def vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def factors(rng, rank, dt, bias_last=None):
    X = np.asfortranarray(rng.standard_normal((rank, N_ROWS)) * 0.3, dtype=dt)
    Y = np.asfortranarray(rng.standard_normal((rank, N_COLS)) * 0.3, dtype=dt)
    if bias_last is not None:   # the row of ones of each side (R/model_WRMF.R:160-176)
        X[0 if bias_last else rank - 1, :] = 1.0
        Y[rank - 1 if bias_last else 0, :] = 1.0
    return X, Y


def run(out):
    import scipy.sparse as sp
    import torch
    from rsparse_amd import _lib
    from rsparse_amd.engine import HipBackend
    lib = _lib.load()
    be = HipBackend(0)
    rng = np.random.default_rng(2024)
    mats = matrices(rng)
    res = {}

    def put(name, rc, **arrays):
        res[name + "/rc"] = np.array([rc], dtype=np.int64)
        for k, v in arrays.items():
            res[name + "/" + k] = np.atleast_1d(np.array(v))

    # ---- the stateless half-iterations
    for mname, m in mats.items():
        p, i, x = slots(m)
        cnt = np.diff(sp.csr_matrix(m).indptr)
        for tname, dt in DTYPES:
            impl = getattr(lib, "rsparse_hip_als_implicit_" + ("float" if dt == np.float32 else "double"))
            expl = getattr(lib, "rsparse_hip_als_explicit_" + ("float" if dt == np.float32 else "double"))

            def implicit(tag, rank, solver, gb, bias, base=None, init=1):
                X, Y = factors(np.random.default_rng(7), rank, dt, 1 if bias else None)
                XX = X[:-1] if bias else X
                G = np.asfortranarray(XX @ XX.T + np.float32(0.1) * np.eye(XX.shape[0]), dtype=dt)
                loss = ctypes.c_double(0.0)
                rc = impl(N_ROWS, N_COLS, vp(p), vp(i), vp(x), vp(X), vp(Y), vp(G), rank, 0.1, 1, solver, 3, int(bias), 1, gb,
                          vp(base), 0 if base is None else base.size, init, ctypes.addressof(loss))
                put("als_implicit/%s/%s/%s" % (mname, tname, tag), rc, Y=Y, loss=loss.value,
                    base=np.zeros(0, dt) if base is None else base)

            for solver in (0, 1, 2):
                for gb in (0.0, 0.3):
                    implicit("rank8 solver%d gb%g" % (solver, gb), 8, solver, gb, False)
            for blen in (7, 8):            # rank - 1 and rank: where the read / write rule of global_bias_base branches
                for init in (0, 1):
                    base = np.random.default_rng(9).standard_normal(blen).astype(dt)
                    implicit("rank8 solver0 gb0.3 base len%d init%d" % (blen, init), 8, 0, 0.3, False, base, init)
            for solver in (0, 2):
                for gb in (0.0, 0.3):
                    implicit("rank10 biases solver%d gb%g" % (solver, gb), 10, solver, gb, True)

            for dyn in (0, 1):
                for lam in (0.0, 0.1):
                    for bias in (False, True):
                        for last in (0, 1):
                            for solver in (0, 1):
                                rank = 10 if bias else 8
                                X, Y = factors(np.random.default_rng(7), rank, dt, last if bias else None)
                                cnt_t = cnt.astype(dt)
                                loss = ctypes.c_double(0.0)
                                rc = expl(N_ROWS, N_COLS, vp(p), vp(i), vp(x), vp(X), vp(Y), vp(cnt_t), rank, lam, 1,
                                          solver, 3, dyn, int(bias), last, ctypes.addressof(loss))
                                put("als_explicit/%s/%s/dyn%d lambda%g biases%d last%d solver%d"
                                    % (mname, tname, dyn, lam, bias, last, solver), rc, Y=Y, loss=loss.value)

    # ---- the bias initialisation: stateless and resident
    for mname, m in mats.items():
        t = sp.csc_matrix(m.T)
        t.sort_indices()
        p1, i1, x1 = slots(m)
        p2, i2, x2 = slots(t)
        for tname, dt in DTYPES:
            tdt = torch.float32 if dt == np.float32 else torch.float64
            host = getattr(lib, "rsparse_hip_initialize_biases_" + ("float" if dt == np.float32 else "double"))
            for explicit in (1, 0):
                for calc in (0, 1):
                    for nonneg in (0, 1):
                        tag = "%s/%s/explicit%d calc%d nonneg%d" % (mname, tname, explicit, calc, nonneg)
                        ub, ib = np.zeros(N_ROWS, dt), np.zeros(N_COLS, dt)
                        v1, v2 = x1.copy(), x2.copy()
                        gb = ctypes.c_double(0.0)
                        rc = host(N_ROWS, N_COLS, vp(p1), vp(i1), vp(v1), vp(p2), vp(i2), vp(v2), vp(ub), vp(ib), 0.1, 1, nonneg,
                                  calc, explicit, ctypes.byref(gb))
                        put("initialize_biases_host/" + tag, rc, user_bias=ub, item_bias=ib, gb=gb.value, csc_x=v1, csr_x=v2)
                        d1 = (be.to_device(p1, torch.int32), be.to_device(i1, torch.int32), be.to_device(x1, tdt))
                        d2 = (be.to_device(p2, torch.int32), be.to_device(i2, torch.int32), be.to_device(x2, tdt))
                        h1, h2 = be.make_csc(N_ROWS, N_COLS, *d1), be.make_csc(N_COLS, N_ROWS, *d2)
                        dub, dib = torch.zeros(N_ROWS, dtype=tdt, device=be.device), torch.zeros(N_COLS, dtype=tdt, device=be.device)
                        gb = ctypes.c_double(0.0)
                        s = be._stream()
                        if dt == np.float64:
                            rc = lib.rsparse_hip_initialize_biases_f64_device(h1.h, h2.h, dub.data_ptr(), dib.data_ptr(), 0.1, 1,
                                                                              nonneg, calc, explicit, ctypes.byref(gb), s)
                        elif explicit:
                            rc = lib.rsparse_hip_initialize_biases_explicit_device(h1.h, h2.h, dub.data_ptr(), dib.data_ptr(), 0.1,
                                                                                   1, nonneg, calc, ctypes.byref(gb), s)
                        else:
                            rc = lib.rsparse_hip_initialize_biases_implicit_device(h1.h, h2.h, dub.data_ptr(), dib.data_ptr(), 0.1,
                                                                                   nonneg, calc, ctypes.byref(gb), s)
                        torch.cuda.synchronize()
                        put("initialize_biases_device/" + tag, rc, user_bias=dub.cpu().numpy(), item_bias=dib.cpu().numpy(),
                            gb=gb.value, csc_x=d1[2].cpu().numpy(), csr_x=d2[2].cpu().numpy())
            # ---- the three single sweeps (the handle's columns against a seeded vector of the other side)
            d1 = (be.to_device(p1, torch.int32), be.to_device(i1, torch.int32), be.to_device(x1, tdt))
            h1 = be.make_csc(N_ROWS, N_COLS, *d1)
            other = be.to_device(np.random.default_rng(3).standard_normal(N_ROWS), tdt)
            o = torch.zeros(N_COLS, dtype=tdt, device=be.device)
            f64 = "_f64" if dt == np.float64 else ""
            for dyn in (0, 1):
                for nonneg in (0, 1):
                    rc = getattr(lib, "rsparse_hip_bias_sweep_explicit%s_device" % f64)(h1.h, other.data_ptr(), 0.1, dyn, nonneg,
                                                                                       o.data_ptr(), be._stream())
                    torch.cuda.synchronize()
                    put("bias_sweep_explicit/%s/%s/dyn%d nonneg%d" % (mname, tname, dyn, nonneg), rc, out=o.cpu().numpy())
            means = torch.zeros(N_COLS, dtype=torch.float64, device=be.device)
            adj = torch.zeros(N_COLS, dtype=torch.float64, device=be.device)
            rc = getattr(lib, "rsparse_hip_bias_prep_implicit%s_device" % f64)(h1.h, N_ROWS, 0.1, means.data_ptr(), adj.data_ptr(),
                                                                              be._stream())
            torch.cuda.synchronize()
            put("bias_prep_implicit/%s/%s" % (mname, tname), rc, means=means.cpu().numpy(), adj=adj.cpu().numpy())
            osum = other.to(torch.float64).sum().reshape(1)
            for with_sum in (0, 1):
                for nonneg in (0, 1):
                    rc = getattr(lib, "rsparse_hip_bias_sweep_implicit%s_device" % f64)(
                        h1.h, other.data_ptr(), N_ROWS, osum.data_ptr() if with_sum else None, means.data_ptr(), adj.data_ptr(),
                        nonneg, 0.02, o.data_ptr(), be._stream())
                    torch.cuda.synchronize()
                    put("bias_sweep_implicit/%s/%s/sum%d nonneg%d" % (mname, tname, with_sum, nonneg), rc, out=o.cpu().numpy())

    # ---- the sums at the lengths where the 1024 partial slots and the two-stage tail meet
    for tname, dt in DTYPES:
        tdt = torch.float32 if dt == np.float32 else torch.float64
        f64 = "_f64" if dt == np.float64 else ""
        for n in (0, 1, 1024, 1025):
            src = np.random.default_rng(100 + n).standard_normal((max(n, 1), 3))
            for two in (0, 1):
                a, b = be.to_device(src[:, 0], tdt), be.to_device(src[:, 1], tdt)   # (one element at n = 0: a non-NULL pointer)
                mean = ctypes.c_double(-1.0)
                rc = getattr(lib, "rsparse_hip_values_subtract_mean%s_device" % f64)(n, a.data_ptr(), b.data_ptr() if two else None,
                                                                                    ctypes.byref(mean), be._stream())
                torch.cuda.synchronize()
                put("values_subtract_mean/%s/n%d arrays%d" % (tname, n, 1 + two), rc, x=a.cpu().numpy(), other=b.cpu().numpy(),
                    mean=mean.value)
            F, w = be.to_device(src, tdt), be.to_device(np.abs(src[:, 0]) + 1.0, tdt)
            for weights in (0, 1):
                o = torch.full((1,), -1.0, dtype=torch.float64, device=be.device)
                rc = getattr(lib, "rsparse_hip_weighted_sumsq%s_device" % f64)(F.data_ptr(), 3, n, w.data_ptr() if weights else None,
                                                                              o.data_ptr(), be._stream())
                torch.cuda.synchronize()
                put("weighted_sumsq/%s/n%d weights%d" % (tname, n, weights), rc, out=o.cpu().numpy())
        X = np.asfortranarray(np.random.default_rng(8).standard_normal((8, 1025)), dtype=dt)
        G = np.zeros((8, 8), dtype=dt, order="F")
        rc = getattr(lib, "rsparse_hip_gramian_" + ("float" if dt == np.float32 else "double"))(vp(X), 8, 1025, 0.1, vp(G))
        put("gramian_host/%s/1025x8" % tname, rc, XtX=G)

    np.savez(out, **res)
    codes = sorted({int(v[0]) for k, v in res.items() if k.endswith("/rc")})
    print("wrote %s: %d records, return codes seen %s" % (out, len(res), codes))
    return 0


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def compare(a, b):
    da, db = np.load(a), np.load(b)
    bad = 0 if sorted(da.files) == sorted(db.files) else 1
    groups = {}
    for key in da.files:
        same = key in db.files and da[key].shape == db[key].shape and np.array_equal(bits(da[key]), bits(db[key]))
        g = groups.setdefault("/".join(key.split("/")[:-2]), [0, []])   # entry / matrix / precision
        g[0] += 1
        if not same:
            g[1].append(key)
    for name in sorted(groups):
        n, diff = groups[name]
        bad += len(diff)
        print("%-36s %4d outputs  %s" % (name, n, "bitwise equal" if not diff else "DIFFERS: " + ", ".join(diff)))
    return 1 if bad else 0


def ab(parent_lib, outdir):
    outdir = Path(outdir)
    outdir.mkdir(parents=True, exist_ok=True)
    for name, lib in (("parent", parent_lib), ("new", None)):
        env = dict(os.environ)
        env.pop("RSPARSE_HIP_LIB", None)
        if lib:
            env["RSPARSE_HIP_LIB"] = str(lib)
        rc = subprocess.call([sys.executable, __file__, "run", str(outdir / (name + ".npz"))], env=env)
        if rc:   # (nothing more is started on the device after a failed run)
            return rc
    return compare(outdir / "parent.npz", outdir / "new.npz")


if __name__ == "__main__":
    cmd = sys.argv[1]
    sys.exit(run(sys.argv[2]) if cmd == "run" else compare(sys.argv[2], sys.argv[3]) if cmd == "compare" else ab(sys.argv[2], sys.argv[3]))
