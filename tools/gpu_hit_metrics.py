#!/usr/bin/env python
"""Hit-based metrics at several cutoffs (rsparse_hip_hit_metrics_device, wrmf_hits.hip) at scale.  (a) Lists of --users x --k
random items with a planted hit in three rows of ten, about ten held-out items per row (one per stratum of the catalogue):
`hit_metrics` at --cutoffs with every output, without and with first_seen, against `ranking_metrics` (ap only) on the same lists
in the same session -- both read the same lists and make the same lookups.  Host clock around calls that end in a device
synchronise, one warm-up call, then the median of --reps with the minimum and maximum.  (b) On --eval-users users of a model
fitted for one iteration (the shape of tools/gpu_sample_negatives.py), `evaluate(k=(5, 10, 20), negatives=99, metrics=("hit",
"ndcg"))` against three `evaluate(k=c, negatives=99, metrics=("ndcg",))` calls, which take the single-cutoff path unchanged.

    python tools/gpu_hit_metrics.py [--users 262144] [--k 2000] [--items 1000000] [--eval-users 10000] [--out FILE.jsonl]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import scipy.sparse as sp
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from rsparse_amd import WRMF  # noqa: E402
from rsparse_amd.engine import HipBackend  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=262144)
ap.add_argument("--k", type=int, default=2000)
ap.add_argument("--items", type=int, default=1_000_000)
ap.add_argument("--cutoffs", default="10,20,50,100,500,1000,2000")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--eval-users", type=int, default=10_000)
ap.add_argument("--eval-items", type=int, default=1_000_000)
ap.add_argument("--rank", type=int, default=128)
ap.add_argument("--out", default=None)
a = ap.parse_args()

be = HipBackend(0)
dev = be.device
g = torch.Generator(device=dev).manual_seed(1)
lines = []


def timed(fn):
    fn()   # warm-up (code objects, the workspace)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return [sorted(ts)[len(ts) // 2] * 1e3, min(ts) * 1e3, max(ts) * 1e3]


def emit(line):
    print(json.dumps(line), flush=True)
    lines.append(line)


if a.users > 0:
    n, k, n_item = a.users, a.k, a.items
    cutoffs = tuple(int(t) for t in a.cutoffs.split(","))
    width = n_item // 10
    held = (torch.arange(10, device=dev, dtype=torch.int64)[None, :] * width + torch.randint(0, width, (n, 10), generator=g, device=dev))
    lens = torch.randint(5, 11, (n,), generator=g, device=dev)
    mask = torch.arange(10, device=dev)[None, :] < lens[:, None]
    p = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)]).to(torch.int32)
    j = held[mask].to(torch.int32)
    res = torch.randint(1, n_item + 1, (n, k), generator=g, device=dev, dtype=torch.int32)
    rows = torch.nonzero(torch.rand(n, generator=g, device=dev) < 0.3).flatten()
    at = torch.randint(0, k, (rows.numel(),), generator=g, device=dev)
    res[rows, at] = (held[rows, 0] + 1).to(torch.int32)
    names = ("hits", "first", "precision", "recall", "hit", "mrr")
    seen = torch.full((n_item,), 2 ** 31 - 1, dtype=torch.int32, device=dev)

    def with_coverage():
        seen.fill_(2 ** 31 - 1)   # (a slot that is already low takes no atomic: every timed call starts from nothing)
        be.hit_metrics(res, p, j, cutoffs, names, seen)

    first = be.hit_metrics(res, p, j, cutoffs, names)
    again = be.hit_metrics(res, p, j, cutoffs, names)
    t_hit = timed(lambda: be.hit_metrics(res, p, j, cutoffs, names))
    t_one = timed(lambda: be.hit_metrics(res, p, j, cutoffs, ("recall",)))
    t_fill = timed(lambda: seen.fill_(2 ** 31 - 1))
    t_cov = timed(with_coverage)   # (leaves first_seen complete for the coverage figure below)
    t_ap = timed(lambda: be.ranking_metrics(res, p, j, None, True, False))
    hit_last = first["hit"][:, -1]
    emit({"what": "hit_metrics (every output) without / with first_seen against ranking_metrics (ap only) on the same lists",
          "users": n, "k": k, "items": n_item, "cutoffs": list(cutoffs), "held_out_per_user": float(j.numel()) / n, "reps": a.reps,
          "list_bytes": n * k * 4, "hit_metrics_ms": t_hit, "hit_metrics_recall_only_ms": t_one,
          "hit_metrics_with_first_seen_ms": t_cov, "of_which_first_seen_fill_ms": t_fill, "ranking_metrics_ap_ms": t_ap,
          "hit_over_ap": t_hit[0] / t_ap[0], "coverage_adds_ms": t_cov[0] - t_fill[0] - t_hit[0],
          "lists_gb_per_s_hit_metrics": n * k * 4 / t_hit[0] / 1e6,
          "hit_rate_at_last_cutoff": float(hit_last.mean()), "coverage_at_last_cutoff": float((seen <= cutoffs[-1]).sum()) / n_item,
          "repeat_bit_identical": bool(all(torch.equal(first[m].view(torch.int32), again[m].view(torch.int32)) for m in names))})
    del res, held, p, j, seen, first, again

if a.eval_users > 0:
    ne, n_item, r = a.eval_users, a.eval_items, a.rank
    width = n_item // 150
    m = (torch.arange(150, device=dev, dtype=torch.int64)[None, :] * width + torch.randint(0, width, (ne, 150), generator=g, device=dev))
    lens = torch.randint(50, 151, (ne,), generator=g, device=dev)
    mask = torch.arange(150, device=dev)[None, :] < lens[:, None]
    e_p = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)]).cpu().numpy()
    e_j, h_j = m[mask].cpu().numpy(), m[:, 0].cpu().numpy()
    full = sp.csr_matrix((np.ones(e_j.size), e_j, e_p), shape=(ne, n_item))
    held = sp.csr_matrix((np.ones(ne), h_j, np.arange(ne + 1)), shape=(ne, n_item))
    seen = (full - held).tocsr()
    seen.eliminate_zeros()
    model = WRMF(rank=r, lambda_=0.1, feedback="implicit", solver="conjugate_gradient", precision="float", rng=1, factor_init="device")
    model.fit_transform(full, n_iter=1, convergence_tol=-1)
    K = (5, 10, 20)
    model.evaluate(seen, held, K, negatives=10, seed=1, metrics=("hit", "ndcg"))   # warm-up: the transform, the metrics, the sampler
    model.evaluate(seen, held, 10, negatives=10, seed=1, metrics=("ndcg",))

    def wall(fn):
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return out, [sorted(ts)[len(ts) // 2] * 1e3, min(ts) * 1e3, max(ts) * 1e3]

    many, t_many = wall(lambda: model.evaluate(seen, held, K, negatives=99, seed=7, metrics=("hit", "ndcg")))
    three, t_three = wall(lambda: [model.evaluate(seen, held, c, negatives=99, seed=7, metrics=("ndcg",)) for c in K])
    emit({"what": "evaluate(k=(5, 10, 20), negatives=99, metrics=(hit, ndcg)) against three evaluate(k=c, negatives=99, metrics=(ndcg,))",
          "users": ne, "items": n_item, "rank": r, "reps": a.reps, "one_call_ms": t_many, "three_calls_ms": t_three,
          "three_over_one": t_three[0] / t_many[0], "hit_rate": [float(np.nanmean(many["hit"][:, t])) for t in range(3)],
          "ndcg_columns_equal_the_single_calls": [bool(np.array_equal(many["ndcg"][:, t], three[t]["ndcg"], equal_nan=True)) for t in range(3)]})

if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("".join(json.dumps(line) + "\n" for line in lines))
