"""SLIM (wrmf_slim.hip) on one GPU at the shape of profiles/ease/ease_bench.py: 100 000 users x 20 000 items with about 100 items
each, and one more user who holds EVERY item -- so every column's support is the whole catalogue and every column takes the
workspace route.  One JSON line per measurement, appended to --out (default slim_bench.jsonl here); medians of --reps runs behind a
warm-up.

    python profiles/slim/slim_bench.py --step fit      the Gram rows at lambda = 0 and the coordinate-descent launch, with the
                                                       distributions of support sizes and sweeps (--cols N: the first N columns
                                                       of the class's order only)
    python profiles/slim/slim_bench.py --step ease     EASE(500).fit on the same matrix
    python profiles/slim/slim_bench.py --step numpy    the numpy definition on --sample columns, with their updates per column,
                                                       and its time extrapolated to the catalogue (labelled as such)
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
sys.path.insert(0, str(ROOT / "profiles" / "ease"))
from ease_bench import dataset, timed  # noqa: E402

OUT = HERE / "slim_bench.jsonl"


def say(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def quantiles(t, torch):
    q = torch.quantile(t.to(torch.float64), torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0], dtype=torch.float64, device=t.device))
    return [int(v) for v in q.tolist()]


def gram(a, torch):
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    nnz, up, uj = dataset(a, torch)
    n_users, n = a.users + 1, a.items
    ip, iu, _ = be.transpose_csc(n, n_users, up, uj, torch.ones(nnz, dtype=torch.float32, device=uj.device))
    G = torch.empty((n, n), dtype=torch.float64, device=be.device)
    run = lambda: be.item_gram(ip, iu, up, uj, n_users, n, 0.0, out=G)
    return be, run, G, dict(users=n_users, items=n, nnz=nnz, l1=a.l1, l2=a.l2, max_iter=a.max_iter, tol=a.tol), (up, uj)


def step_fit(a):
    import torch
    from rsparse_amd import _lib
    be, run_gram, G, base, _ = gram(a, torch)
    n = a.items
    say(step="fit", what="gram rows at lambda 0", **timed(run_gram, a.reps, torch), **base)
    support = (G > 0).sum(dim=1) - (G.diagonal() > 0).to(torch.int64)
    order = torch.argsort(support, descending=True, stable=True).to(torch.int32)
    if a.cols:
        order = order[:a.cols].contiguous()
    say(step="fit", what="support sizes (min, quartiles, max)", support=quantiles(support, torch),
        share_on_the_workspace_route=round(float((support > _lib.SLIM_LDS_SUPPORT).double().mean()), 4), **base)
    for dtype in [{"float": torch.float32, "double": torch.float64}[name] for name in a.dtypes.split(",")]:
        ld = (n * dtype.itemsize + 255) // 256 * 256 // dtype.itemsize
        W = torch.zeros((n, ld), dtype=dtype, device=be.device)
        sweeps = []
        t = timed(lambda: sweeps.append(be.slim_columns(G, order, a.l1, a.l2, a.max_iter, a.tol, W)), a.reps, torch)
        say(step="fit", what="coordinate-descent launch", dtype=str(dtype), columns=int(order.numel()), sweeps=quantiles(sweeps[-1], torch),
            columns_at_the_cap=int((sweeps[-1] == a.max_iter).sum()), nonzeros_per_column=round(float((W > 0).sum()) / int(order.numel()), 1),
            **t, **base)
        del W


def step_ease(a):
    import numpy as np
    import scipy.sparse as sp
    import torch
    from rsparse_amd import EASE
    be, _, _, base, (up, uj) = gram(a, torch)
    x = sp.csr_matrix((np.ones(int(uj.numel()), np.float32), uj.cpu().numpy(), up.cpu().numpy()), shape=(a.users + 1, a.items))
    say(step="ease", what="EASE(500).fit, host canonicalisation and upload included", **timed(lambda: EASE(500.0, backend=be).fit(x), min(a.reps, 2), torch),
        **{k: v for k, v in base.items() if k in ("users", "items", "nnz")})


def step_numpy(a):
    import numpy as np
    import torch
    from rsparse_amd.slim import slim_columns_reference
    be, run_gram, G, base, _ = gram(a, torch)
    run_gram()
    order = torch.argsort(G.diagonal(), descending=True).cpu().numpy()
    cols = order[np.linspace(0, a.items - 1, a.sample).astype(np.int64)]      # the most popular item, the least, and between
    G = G.cpu().numpy()
    updates, t0 = [], time.perf_counter()
    W, sweeps = slim_columns_reference(G, cols, a.l1, a.l2, a.max_iter, a.tol, updates=updates)
    dt = time.perf_counter() - t0
    dev_W = torch.zeros((a.items, a.items), dtype=torch.float64, device=be.device)
    dev_s = be.slim_columns(be.to_device(G, torch.float64), be.to_device(cols.astype(np.int32), torch.int32), a.l1, a.l2, a.max_iter, a.tol, dev_W)
    say(step="numpy", what="the numpy definition on a sample of columns", columns=cols.tolist(), seconds=round(dt, 2),
        sweeps=sweeps.tolist(), updates=updates, support=[int((G[j] > 0).sum() - (G[j, j] > 0)) for j in cols],
        device_equals_numpy=bool(np.array_equal(dev_W.cpu().numpy()[:, cols], W[:, cols]) and np.array_equal(dev_s.cpu().numpy(), sweeps)),
        EXTRAPOLATED_seconds_for_every_column=round(dt / len(cols) * a.items), **base)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True, choices=("fit", "ease", "numpy"))
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--items", type=int, default=20_000)
    ap.add_argument("--nnz", type=float, default=1e7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--l1", type=float, default=1.0)
    ap.add_argument("--l2", type=float, default=50.0)
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--cols", type=int, default=0)
    ap.add_argument("--sample", type=int, default=3)
    ap.add_argument("--dtypes", default="float,double")
    ap.add_argument("--out", default=str(OUT))
    a = ap.parse_args()
    OUT = Path(a.out)
    {"fit": step_fit, "ease": step_ease, "numpy": step_numpy}[a.step](a)
