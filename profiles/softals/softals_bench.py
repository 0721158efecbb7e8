"""The soft-ALS half-iteration kernel (wrmf_softals.hip) and the soft_svd / soft_impute drivers at the bench matrix's scale on one
GPU: 1M x 100k, 5e7 entries from rsparse_amd/synth.py.  One JSON line per measurement, appended to softals_bench.jsonl.

    python profiles/softals/softals_bench.py                      every step, each a process of its own under `timeout -k 10`;
                                                                  stops at the first step that fails
    python profiles/softals/softals_bench.py --step kernel --rank 128 --dtype float      one step, in this process

Steps: kernel (the fused pass in its three modes and both orientations, beside score_pairs on the same pattern and the
composition score_pairs + subtract + torch.sparse.mm + scale), skew (a tenth of all entries in one row), fit (one iteration and a
20-iteration fit, with the kernel, Gramian, torch and host parts itemised), bench (the default bench.py run).
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
OUT = HERE / "softals_bench.jsonl"


def say(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    with open(say.out, "a") as f:
        f.write(line + "\n")


say.out = OUT


def timed(fn, reps, torch):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
        del res
    return {"ms": round(statistics.median(out), 3), "min": round(min(out), 3), "max": round(max(out), 3)}


def dataset(a, torch, tdt):
    from rsparse_amd import synth
    d = synth.make_dataset(a.users, a.items, mean_deg=a.nnz / a.users, device="cuda")
    (pu, ju, xu), (pi, ji, xi) = d["c_iu"], d["c_ui"]      # CSR of x (rows = users) and of t(x) (rows = items)
    i32 = lambda t: t.to(torch.int32).contiguous()
    return int(d["nnz"]), (i32(pu), i32(ju), xu.to(tdt)), (i32(pi), i32(ji), xi.to(tdt))


def step_kernel(a, skew=False):
    import numpy as np
    import torch
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    tdt = torch.float32 if a.dtype == "float" else torch.float64
    size = 4 if a.dtype == "float" else 8
    nnz, users, items = dataset(a, torch, tdt)
    r = a.rank
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    U = torch.randn((a.users, r), device="cuda", dtype=tdt, generator=g) * 0.1
    V = torch.randn((a.items, r), device="cuda", dtype=tdt, generator=g) * 0.1
    d = np.linspace(2.0, 1.0, r)
    s = d / (d + 0.5)
    sides = [("users", users, V, U), ("items", items, U, V)]
    if skew:   # a tenth of all entries in ONE row: the first nnz / 10 stored positions of the user orientation become row 0
        p, j, x = users
        cut = int(torch.searchsorted(p.to(torch.int64), torch.tensor([nnz // 10], device="cuda"))[0])
        p2 = torch.cat([p[:1], p[cut:]]).contiguous()
        sides = [("users, row 0 holds %d entries" % int(p2[1]), (p2, j, x), V, U[cut - 1:].contiguous())]
    for side, (p, j, x), M, W in sides:
        n = int(p.numel()) - 1
        gb = nnz * r * size / 1e9
        base = dict(step="skew" if skew else "kernel", side=side, rank=r, dtype=a.dtype, nnz=nnz, rows=n, table_mb=round(M.numel() * size / 1e6, 1))
        for mode, kw in (("plain", {}), ("svd half", dict(s=s)), ("soft_impute half", dict(W=W, w=d, s=s, t=s * d, want_sumsq=True))):
            t = timed(lambda: be.softals_half(p, j, x, M, **kw), a.reps, torch)
            say(what="softals_half " + mode, gather_gb_s=round(gb / t["ms"] * 1e3, 1), **t, **base)
        if skew:
            continue
        t = timed(lambda: be.score_pairs(W, M, p, j), a.reps, torch)
        say(what="score_pairs", gather_gb_s=round(gb / t["ms"] * 1e3, 1), **t, **base)
        ts, tw = torch.as_tensor(s, dtype=tdt, device="cuda"), torch.as_tensor(d, dtype=tdt, device="cuda")

        def composed():
            sc, _, _ = be.score_pairs(W * tw, M, p, j)
            res = x - sc.to(tdt)
            csr = torch.sparse_csr_tensor(p.to(torch.int64), j.to(torch.int64), res, size=(n, M.shape[0]))
            return torch.sparse.mm(csr, M) * ts + W * (ts * tw)
        try:
            t = timed(composed, a.reps, torch)
            say(what="composition: score_pairs, subtract, torch.sparse.mm, scale", **t, **base)
        except Exception as e:   # (reported, not fatal: the composition is the yardstick, not the product)
            say(what="composition", error=str(e)[:200], **base)


def step_fit(a):
    import numpy as np
    import scipy.sparse as sp
    import torch
    from rsparse_amd import soft_impute, soft_svd
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    nnz, (p, j, x), _ = dataset(a, torch, torch.float32)
    m = sp.csr_matrix((x.cpu().numpy().astype(np.float64), j.cpu().numpy(), p.cpu().numpy()), shape=(a.users, a.items))
    del p, j, x
    torch.cuda.empty_cache()
    parts = {}

    def wrap(name):
        fn = getattr(be, name)

        def inner(*args, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*args, **kw)
            torch.cuda.synchronize()
            parts[name] = parts.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
            return out
        setattr(be, name, inner)
    for name in ("softals_half", "gramian", "transpose_csc", "to_device"):
        wrap(name)
    for fn in (soft_svd, soft_impute):
        for iters in (1, 20):
            parts.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn(m, rank=a.rank, lambda_=1.0, n_iter=iters, convergence_tol=-1, precision=a.dtype, rng=1, backend=be)
            torch.cuda.synchronize()
            total = (time.perf_counter() - t0) * 1e3
            rest = total - sum(parts.values())
            say(step="fit", what=fn.__name__, rank=a.rank, dtype=a.dtype, nnz=nnz, n_iter=iters, total_ms=round(total, 1),
                kernel_ms=round(parts.get("softals_half", 0), 1), gramian_ms=round(parts.get("gramian", 0), 1),
                upload_and_transpose_ms=round(parts.get("to_device", 0) + parts.get("transpose_csc", 0), 1),
                torch_and_host_ms=round(rest, 1), final_rank=int(res.d.size), last_delta=res.trace[-1][0])


def step_bench(a):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1"], stdout=subprocess.PIPE, text=True, cwd=str(ROOT))
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    say(step="bench", what="bench.py --gpus 1", rc=r.returncode, result=json.loads(line[-1]) if line else None)
    if r.returncode:
        sys.exit(r.returncode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("kernel", "skew", "fit", "bench"))
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--nnz", type=float, default=5e7)
    ap.add_argument("--rank", type=int, default=128)
    ap.add_argument("--dtype", choices=("float", "double"), default="float")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--out", default=str(OUT), help="the .jsonl the measurements are appended to")
    a = ap.parse_args()
    say.out = a.out
    if a.step:
        {"kernel": step_kernel, "skew": lambda b: step_kernel(b, skew=True), "fit": step_fit, "bench": step_bench}[a.step](a)
        return
    steps = [["--step", "kernel", "--rank", str(r), "--dtype", t] for r in (10, 128) for t in ("float", "double")]
    steps += [["--step", "skew", "--rank", "128", "--dtype", "float"]]
    steps += [["--step", "fit", "--rank", str(r), "--dtype", "float"] for r in (10, 128)]
    steps += [["--step", "bench"]]
    for s in steps:   # every GPU step a process of its own under its own time limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, str(Path(__file__).resolve()), *s,
               "--users", str(a.users), "--items", str(a.items), "--nnz", str(a.nnz), "--reps", str(a.reps), "--out", a.out]
        rc = subprocess.run(cmd).returncode
        if rc:
            say(step=s[1], failed=rc, args=s)
            sys.exit(rc)


if __name__ == "__main__":
    main()
