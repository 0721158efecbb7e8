#!/usr/bin/env python3
"""`WRMF.evaluate` at scale: the top-k lists of the rescoring `$predict` entry (rsparse_hip_top_product_f64_device, what
`WRMF.predict` runs) scored on the device by ap@k + ndcg@k (rsparse_hip_ranking_metrics_device, wrmf_metrics.hip).  Prints one
JSON line: the metrics call's time, users/s and algorithmic bytes / time against 8 TB/s of HBM
(bytes = 4 n k lists + 4 (n + 1) row pointers + 12 nnz held-out slots + 16 n outputs), and the `predict` call at the same
shape, whose lists the metrics score.

  python tools/gpu_evaluate.py [--users 1000000] [--items 1000000] [--rank 128] [--topk 10] [--held 10]
                               [--long-frac 0.01 --long-len 5000] [--values ratings|ones] [--reps 3]

--long-frac gives that fraction of the users --long-len held-out items each (rows beyond the kernel's LDS cap: their idcg takes
the long-row launch).
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from rsparse_amd.engine import HipBackend  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=1_000_000)
ap.add_argument("--items", type=int, default=1_000_000)
ap.add_argument("--rank", type=int, default=128)
ap.add_argument("--topk", type=int, default=10)
ap.add_argument("--held", type=int, default=10, help="held-out items per user")
ap.add_argument("--long-frac", type=float, default=0.0, help="fraction of users with --long-len held-out items instead")
ap.add_argument("--long-len", type=int, default=5000)
ap.add_argument("--values", choices=("ratings", "ones"), default="ratings", help="relevances: integers 1..5 or all ones")
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()

be = HipBackend(0)
dev = be.device
g = torch.Generator(device=dev).manual_seed(1)
n, n_item = a.users, a.items
U = torch.randn(n, a.rank, generator=g, device=dev) * 0.1
V = torch.randn(n_item, a.rank, generator=g, device=dev) * 0.1


def rows_of(m, d):
    """m rows of d distinct sorted item ids"""
    j = torch.sort(torch.randint(0, n_item - d + 1, (m, d), generator=g, device=dev), dim=1).values
    return (j + torch.arange(d, device=dev)).to(torch.int32)


is_long = torch.zeros(n, dtype=torch.bool, device=dev)
n_long = int(round(n * a.long_frac))
if n_long:
    is_long[torch.linspace(0, n - 1, n_long, device=dev).long()] = True
    n_long = int(is_long.sum())
lens = torch.where(is_long, a.long_len, a.held).to(torch.int64)
p64 = torch.zeros(n + 1, dtype=torch.int64, device=dev)
p64[1:] = torch.cumsum(lens, 0)
nnz = int(p64[-1])
assert nnz < 2 ** 31
j = torch.empty(nnz, dtype=torch.int32, device=dev)
for sel, d in ((~is_long, a.held), (is_long, a.long_len)):
    users = torch.nonzero(sel).view(-1)
    for u0 in range(0, users.numel(), 1 << 16):
        us = users[u0:u0 + (1 << 16)]
        j[(p64[us][:, None] + torch.arange(d, device=dev)).view(-1)] = rows_of(us.numel(), d).view(-1)
x = (torch.randint(1, 6, (nnz,), generator=g, device=dev).to(torch.float64) if a.values == "ratings"
     else torch.ones(nnz, dtype=torch.float64, device=dev))
p = p64.to(torch.int32)

# the lists: `predict`'s device call (fp32 nomination, double re-scoring), timed at the same shape
res, _ = be.top_product(U[:4096], V, a.topk, None, None, None, 0.0)   # warm-up
torch.cuda.synchronize()
t0 = time.perf_counter()
res, _ = be.top_product(U, V, a.topk, None, None, None, 0.0)
torch.cuda.synchronize()
t_predict = time.perf_counter() - t0

apv, ndv = be.ranking_metrics(res, p, j, x)   # warm-up (and the workspace)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(a.reps):
    ap2, nd2 = be.ranking_metrics(res, p, j, x)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / a.reps
same = bool(torch.equal(apv.view(torch.int64), ap2.view(torch.int64)) and torch.equal(ndv.view(torch.int64), nd2.view(torch.int64)))
t0 = time.perf_counter()
for _ in range(a.reps):
    be.ranking_metrics(res, p, j, x, True, False)
torch.cuda.synchronize()
dt_ap = (time.perf_counter() - t0) / a.reps

nbytes = 4 * n * a.topk + 4 * (n + 1) + 12 * nnz + 16 * n
apn = apv.cpu().numpy()
print(json.dumps({"what": "ranking_metrics (ap@k + ndcg@k) of the $predict lists", "users": n, "items": n_item, "rank": a.rank,
                  "topk": a.topk, "held_per_user": a.held, "long_users": n_long, "long_len": a.long_len if n_long else 0,
                  "values": a.values, "nnz_held": nnz, "metrics_seconds": dt, "metrics_ap_only_seconds": dt_ap,
                  "users_per_sec": n / dt, "algorithmic_bytes": nbytes, "gb_per_sec": nbytes / dt / 1e9,
                  "frac_of_8tbs_hbm": nbytes / dt / 8e12, "predict_seconds": t_predict,
                  "metrics_over_predict": dt / t_predict, "repeat_bit_identical": same,
                  "mean_ap": float(np.nanmean(apn)), "mean_ndcg": float(ndv.mean())}))
