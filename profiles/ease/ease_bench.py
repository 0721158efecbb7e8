"""EASE (wrmf_ease.hip) on one GPU at a shape from rsparse_amd/synth.py: 100 000 users x 20 000 items with about 100 items each, and
one more user who holds EVERY item (20 000 entries: the longest row a binary matrix has; a tenth of all entries would be 50 times
the catalogue).  One JSON line per measurement, appended to ease_bench.jsonl; medians of --reps runs behind a warm-up.

    python profiles/ease/ease_bench.py --step fit        the Gram rows, the factorisation, the inverse, the step from P to B
    python profiles/ease/ease_bench.py --step predict    the lists of every user at k = 10, float and double weights (random
                                                         weights: the time does not depend on their values)
    python profiles/ease/ease_bench.py --step torch      the same algebra through torch.sparse.mm + topk on the same GPU

The kernels' own times come from a profiler run of `--step predict --reps 1` (README.md).
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
OUT = HERE / "ease_bench.jsonl"
TOPK = 10


def say(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


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


def dataset(a, torch):
    """the CSR rows of the synthetic pattern plus the user of every item, int32 on the device -> (nnz, up, uj)"""
    from rsparse_amd import synth
    d = synth.make_dataset(a.users, a.items, mean_deg=a.nnz / a.users, device="cuda")
    up, uj, _ = d["c_iu"]
    up = torch.cat([up.to(torch.int64), up[-1:].to(torch.int64) + a.items]).to(torch.int32)
    uj = torch.cat([uj.to(torch.int32), torch.arange(a.items, dtype=torch.int32, device=uj.device)]).contiguous()
    return int(uj.numel()), up.contiguous(), uj


def step_fit(a):
    import torch
    from rsparse_amd.ease import INVERSE_BLOCK, cholesky_inverse_blocked, spd_inverse, weights_from_inverse
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    nnz, up, uj = dataset(a, torch)
    n_users, n = a.users + 1, a.items
    ip, iu, _ = be.transpose_csc(n, n_users, up, uj, torch.ones(nnz, dtype=torch.float32, device=uj.device))
    lens = (up[1:] - up[:-1]).to(torch.int64)
    base = dict(step="fit", users=n_users, items=n, nnz=nnz, longest_row=int(lens.max()))
    A = torch.empty((n, n), dtype=torch.float64, device=be.device)
    say(what="gram rows", scatter_atomics=int((lens * (lens - 1)).sum()), out_gb=round(8 * n * n / 1e9, 2),
        **timed(lambda: be.item_gram(ip, iu, up, uj, n_users, n, 500.0, out=A), a.reps, torch), **base)
    reps = min(a.reps, 3)
    say(what="torch.linalg.cholesky_ex", flops=round(n ** 3 / 3), **timed(lambda: torch.linalg.cholesky_ex(A), reps, torch), **base)
    L = torch.linalg.cholesky_ex(A)[0]
    say(what="cholesky_inverse_blocked (torch.cholesky_solve, %d identity columns at a time)" % INVERSE_BLOCK, flops=round(2 * n ** 3),
        **timed(lambda: cholesky_inverse_blocked(L), reps, torch), **base)
    del L
    P = spd_inverse(A)
    say(what="spd_inverse ran on the", where="host" if spd_inverse.on_host else "device", **base)
    for dtype in (torch.float32, torch.float64):
        ld = (n * dtype.itemsize + 255) // 256 * 256 // dtype.itemsize
        say(what="P -> B", dtype=str(dtype), **timed(lambda: weights_from_inverse(P, dtype, ld), a.reps, torch), **base)


def step_predict(a):
    import torch
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    nnz, up, uj = dataset(a, torch)
    n_users, n = a.users + 1, a.items
    for dtype in (torch.float32, torch.float64):
        ld = (n * dtype.itemsize + 255) // 256 * 256 // dtype.itemsize
        B = torch.randn((n, ld), dtype=dtype, device=be.device)
        B[:, :n].fill_diagonal_(0.0)
        for nr in (True, False):
            t = timed(lambda: be.ease_recommend(up, uj, B, n, TOPK, up if nr else None, uj if nr else None), a.reps, torch)
            say(step="predict", users=n_users, items=n, nnz=nnz, k=TOPK, dtype=str(dtype), not_recommend=nr,
                gathered_gb=round(nnz * n * dtype.itemsize / 1e9, 1), B_gb=round(n * ld * dtype.itemsize / 1e9, 2),
                dense_rows_gb=round(8 * n * n_users / 1e9, 1), rows_per_batch=min(n_users, (1 << 30) // (8 * n)), **t)
        del B


def step_torch(a):
    import torch
    nnz, up, uj = dataset(a, torch)
    n_users, n = a.users + 1, a.items
    x = torch.sparse_csr_tensor(up.to(torch.int64), uj.to(torch.int64), torch.ones(nnz, dtype=torch.float32, device=uj.device),
                                size=(n_users, n))
    B = torch.randn((n, n), dtype=torch.float32, device=uj.device)

    def route():
        s = torch.sparse.mm(x, B)
        s[torch.repeat_interleave(torch.arange(n_users, device=uj.device), (up[1:] - up[:-1]).to(torch.int64)), uj.to(torch.int64)] = -torch.inf
        return torch.topk(s, TOPK, dim=1)
    try:
        say(step="torch", what="torch.sparse.mm(x, B) float32, mask by index, topk per row", users=n_users, items=n, nnz=nnz,
            **timed(route, a.reps, torch))
    except Exception as e:   # (reported, not fatal: the route is the yardstick, not the product)
        say(step="torch", what="torch.sparse route", error=str(e)[:300])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True, choices=("fit", "predict", "torch"))
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--items", type=int, default=20_000)
    ap.add_argument("--nnz", type=float, default=1e7)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    {"fit": step_fit, "predict": step_predict, "torch": step_torch}[a.step](a)
