"""The blocked symmetric sweep (wrmf_spdinv.hip, `HipBackend.spd_inverse`) against the torch route (`ease.spd_inverse`) on one GPU, on
the Gram matrix of the README's EASE shape: 100 000 users x 20 000 items with about 100 items each plus one user of every item,
lambda = 500.  One JSON line per measurement, appended to spd_inverse_bench.jsonl.

    python profiles/spd_inverse/spd_inverse_bench.py --step inverse     both routes on the leading n x n block of the Gram matrix
                                                                        (the Gram matrix of the first n items), n from --sizes,
                                                                        alternating, medians of --reps runs behind a warm-up; then
                                                                        the residual and the difference of the two inverses
    python profiles/spd_inverse/spd_inverse_bench.py --step fit         EASE.fit end to end with inverse="torch" and "sweep"

The sweep's time includes the copy of the input into its buffer (it works in place); TFLOP/s is n^3 over the call's time for
the sweep and for the torch route alike (the torch route executes about 2.3 n^3).
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(HERE.parent / "ease"))
OUT = HERE / "spd_inverse_bench.jsonl"


def say(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def gram(a, torch, be):
    from ease_bench import dataset
    nnz, up, uj = dataset(a, torch)
    n_users, n = a.users + 1, a.items
    ip, iu, _ = be.transpose_csc(n, n_users, up, uj, torch.ones(nnz, dtype=torch.float32, device=uj.device))
    return be.item_gram(ip, iu, up, uj, n_users, n, 500.0), up, uj


def step_inverse(a):
    import torch
    from rsparse_amd.ease import spd_inverse
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    G, _, _ = gram(a, torch, be)
    for n in a.sizes:
        A = G[:n, :n].contiguous()
        buf = torch.empty_like(A)

        def sweep():
            buf.copy_(A)
            return be.spd_inverse(buf)
        times = {"sweep": [], "torch": []}
        routes = {"sweep": sweep, "torch": lambda: spd_inverse(A)}
        for rep in range(a.reps + 1):   # (the first round is the warm-up)
            for name, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = fn()
                torch.cuda.synchronize()
                if rep:
                    times[name].append((time.perf_counter() - t0) * 1e3)
                if name == "torch":
                    P_torch = res
                del res
        eye = torch.eye(n, dtype=torch.float64, device=A.device)
        P = sweep()
        ref_max = float(P_torch.abs().max())
        for name, Q in (("sweep", P), ("torch", P_torch)):
            ms = statistics.median(times[name])
            say(step="inverse", route=name, n=n, ms=round(ms, 3), min=round(min(times[name]), 3), max=round(max(times[name]), 3),
                tflops_on_n3=round(n ** 3 / ms / 1e9, 2), residual=float((Q @ A - eye).abs().max()),
                symmetric=bool(torch.equal(Q, Q.T)), on_host=bool(spd_inverse.on_host) if name == "torch" else False)
        say(step="inverse", what="max |P_sweep - P_torch| / max |P_torch|", n=n, value=float((P - P_torch).abs().max()) / ref_max,
            sweep_over_torch=round(statistics.median(times["sweep"]) / statistics.median(times["torch"]), 3))
        del A, buf, P, P_torch, eye


def step_fit(a):
    import numpy as np
    import scipy.sparse as sp
    import torch
    from ease_bench import dataset
    from rsparse_amd import EASE
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    nnz, up, uj = dataset(a, torch)
    x = sp.csr_matrix((np.ones(nnz, dtype=np.float32), uj.cpu().numpy(), up.cpu().numpy()), shape=(a.users + 1, a.items))
    times = {"torch": [], "sweep": []}
    for rep in range(a.reps + 1):
        for name in times:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = EASE(500.0, backend=be, inverse=name).fit(x)
            torch.cuda.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t0) * 1e3)
            del m
    for name, t in times.items():
        say(step="fit", what="EASE.fit end to end (host canonicalisation of x included)", inverse=name, users=a.users + 1, items=a.items,
            nnz=nnz, ms=round(statistics.median(t), 1), min=round(min(t), 1), max=round(max(t), 1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True, choices=("inverse", "fit"))
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--items", type=int, default=20_000)
    ap.add_argument("--nnz", type=float, default=1e7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[8192, 20_000])
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    {"inverse": step_inverse, "fit": step_fit}[a.step](a)
