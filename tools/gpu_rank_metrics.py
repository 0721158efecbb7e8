#!/usr/bin/env python3
"""Full-ranking metrics at scale: rsparse_hip_held_out_ranks_device + rsparse_hip_rank_summary_device (wrmf_ranks.hip; what
`WRMF.evaluate_ranks` runs) on random factors, against the large-k `$predict` call at k = 257 on the same shape -- both compute
and mask the same key matrix; the top-k path then reads it four times, the rank count once.  Prints one JSON line.

  python tools/gpu_rank_metrics.py [--users 262144] [--items 1000000] [--rank 128] [--held 10]
                                   [--long-frac 0.01 --long-len 5000] [--reps 2] [--what ranks|top257|both]

--what top257 times only the top-k call (rsparse_hip_top_product_device, fp32 scores, k = 257) and binds that one symbol: run it
with RSPARSE_HIP_LIB pointing at another build of the library -- an older one too -- to time that build; interleave such runs
with --what ranks runs of this build for a paired comparison (profiles/rank_metrics/README.md).  The split between the kernels comes from a kernel trace of a --what ranks
run (rocprofv3 --kernel-trace --stats), not from this script.
"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from rsparse_amd import _lib  # noqa: E402
from rsparse_amd.engine import HipBackend  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=262144)
ap.add_argument("--items", type=int, default=1_000_000)
ap.add_argument("--rank", type=int, default=128)
ap.add_argument("--held", type=int, default=10, help="held-out items per user")
ap.add_argument("--long-frac", type=float, default=0.0, help="fraction of users with --long-len held-out items instead")
ap.add_argument("--long-len", type=int, default=5000)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--what", choices=("ranks", "top257", "both"), default="both")
a = ap.parse_args()

torch.cuda.is_available()   # (torch looks at the GPU before the library initialises the runtime: _lib.load)
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
g = torch.Generator(device=dev).manual_seed(1)
n, n_item = a.users, a.items
U = torch.randn(n, a.rank, generator=g, device=dev) * 0.1
V = torch.randn(n_item, a.rank, generator=g, device=dev) * 0.1
out = {"what": a.what, "users": n, "items": n_item, "rank": a.rank, "lib": str(_lib.LIB_PATH)}


def timed(fn):
    fn(4096)   # warm-up (and the workspace)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = fn(n)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts, r


if a.what in ("top257", "both"):
    k = 257
    res = torch.empty((n, k), dtype=torch.int32, device=dev)
    sc = torch.empty((n, k), dtype=torch.float32, device=dev)

    fn = ctypes.CDLL(str(_lib.LIB_PATH)).rsparse_hip_top_product_device
    fn.restype, fn.argtypes = _lib.SIGNATURES["rsparse_hip_top_product_device"]

    def top(m):
        rc = fn(U.data_ptr(), V.data_ptr(), m, n_item, a.rank, k, None, None, None, 0, 0.0, res.data_ptr(), sc.data_ptr(),
                ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert rc == 0, rc
    ts, _ = timed(top)
    out.update(top257_seconds=ts, top257_users_per_sec=n / min(ts))
    del res, sc

if a.what in ("ranks", "both"):
    be = HipBackend(0)

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
        for u0 in range(0, users.numel(), 1 << 14):
            us = users[u0:u0 + (1 << 14)]
            j[(p64[us][:, None] + torch.arange(d, device=dev)).view(-1)] = rows_of(us.numel(), d).view(-1)
    x = torch.randint(1, 6, (nnz,), generator=g, device=dev).to(torch.float64)
    p = p64.to(torch.int32)

    def ranks(m):
        return be.held_out_ranks(U[:m], V, None, None, None, p[:m + 1], j)
    ts, (above, tied, n_adm) = timed(ranks)
    t0 = time.perf_counter()
    mpr, auc, mrr, sums = be.rank_summary(p, x, above, tied, n_adm)
    torch.cuda.synchronize()
    t_sum = time.perf_counter() - t0
    a2, t2, n2 = ranks(n)
    torch.cuda.synchronize()
    same = bool(torch.equal(a2, above) and torch.equal(t2, tied) and torch.equal(n2, n_adm))
    tot_w, tot = float(sums[:, 0].sum()), float(sums[:, 1].sum())
    out.update(held_per_user=a.held, long_users=n_long, long_len=a.long_len if n_long else 0, nnz_held=nnz, ranks_seconds=ts,
               ranks_users_per_sec=n / min(ts), summary_seconds=t_sum, repeat_bit_identical=same, mpr=tot / tot_w,
               mean_auc=float(auc.nanmean()), mean_mrr=float(mrr.nanmean()))
    if "top257_seconds" in out:
        out["ranks_over_top257"] = min(ts) / min(out["top257_seconds"])
print(json.dumps(out))
