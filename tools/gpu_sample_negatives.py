#!/usr/bin/env python3
"""Negative sampling at scale (rsparse_hip_sample_negatives_device, wrmf_sample.hip) and the evaluation it feeds.  Users with
50 .. 150 seen items each (ascending, unique, one per stratum of the catalogue), one of them held out (`keep`).  Prints one JSON
line per n with, each the median of --reps calls after a warm-up, with min / max (host clock around calls that end in a device
synchronise):

  (a) sample_ms   the whole `HipBackend.sample_negatives` call: the row-pointer scan, its read-back, the sampling launch;
  (b) top_ms      `HipBackend.top_candidates` (k = 10, fp32 factors of --rank) on the rows (a) made, in the same session;

whether (a) repeats bit for bit, and the draws of row 0 checked against the numpy specification.  Then, on --eval-users users of
a model fitted for one iteration, the wall time of `evaluate(negatives=n)` against the same evaluation with the candidate matrix
built on the host by the numpy specification and passed as `candidates=` (both after a warm-up evaluation), and whether the two
agree.  Kernel times come from a profiler run of this tool, not from it.

  python tools/gpu_sample_negatives.py [--users 100000] [--items 1000000] [--rank 128] [--n 99,999] [--reps 5]
                                       [--eval-users 10000] [--out profiles/sample_negatives/sample_negatives.jsonl]
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
from rsparse_amd import WRMF, rng as R  # noqa: E402
from rsparse_amd.engine import HipBackend  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=100_000)
ap.add_argument("--items", type=int, default=1_000_000)
ap.add_argument("--rank", type=int, default=128)
ap.add_argument("--n", default="99,999")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--eval-users", type=int, default=10_000)
ap.add_argument("--out", default=None)
a = ap.parse_args()

be = HipBackend(0)
dev = be.device
g = torch.Generator(device=dev).manual_seed(1)
n_u, n_item, r = a.users, a.items, a.rank


def seen_rows(n_rows):
    """(seen_p, seen_j, keep_p, keep_j) on the device: 50 .. 150 items per row, one per stratum; keep = the row's first item"""
    width = n_item // 150
    m = (torch.arange(150, device=dev, dtype=torch.int64)[None, :] * width + torch.randint(0, width, (n_rows, 150), generator=g, device=dev))
    lens = torch.randint(50, 151, (n_rows,), generator=g, device=dev)
    mask = torch.arange(150, device=dev)[None, :] < lens[:, None]
    s_p = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)]).to(torch.int32)
    return s_p, m[mask].to(torch.int32), torch.arange(n_rows + 1, dtype=torch.int32, device=dev), m[:, 0].to(torch.int32).contiguous()


def timed(fn):
    fn()   # warm-up (code objects, the workspace)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2] * 1e3, min(ts) * 1e3, max(ts) * 1e3


U = torch.randn(n_u, r, generator=g, device=dev) * 0.1
V = torch.randn(n_item, r, generator=g, device=dev) * 0.1
s_p, s_j, k_p, k_j = seen_rows(n_u)
lines = []
for n in (int(t) for t in a.n.split(",")):
    c_p, c_j = be.sample_negatives(7, 0, s_p, s_j, k_p, k_j, n_item, n)
    c_p2, c_j2 = be.sample_negatives(7, 0, s_p, s_j, k_p, k_j, n_item, n)
    a_ms = timed(lambda: be.sample_negatives(7, 0, s_p, s_j, k_p, k_j, n_item, n))
    b_ms = timed(lambda: be.top_candidates(U, V, 10, c_p, c_j, None, None, None, 0.5))
    e0 = int(s_p[1])
    want = R.sample_negatives(7, 0, s_p[:2].cpu().numpy(), s_j[:e0].cpu().numpy(), k_p[:2].cpu().numpy(), k_j[:1].cpu().numpy(), n_item, n)
    line = {"what": "sample_negatives, then top_candidates (k = 10, fp32 factors) on its rows", "users": n_u, "items": n_item, "rank": r,
            "n": n, "seen_per_user": float(s_j.numel()) / n_u, "candidates": int(c_j.numel()), "reps": a.reps,
            "sample_ms": a_ms[0], "sample_ms_min_max": list(a_ms[1:]), "top_ms": b_ms[0], "top_ms_min_max": list(b_ms[1:]),
            "sample_over_top": a_ms[0] / b_ms[0],
            "repeat_bit_identical": bool(torch.equal(c_p, c_p2) and torch.equal(c_j, c_j2)),
            "row0_equals_specification": bool(np.array_equal(c_j[:int(c_p[1])].cpu().numpy(), want[1]))}
    print(json.dumps(line), flush=True)
    lines.append(line)
    del c_p, c_j, c_p2, c_j2
del U, V, s_p, s_j, k_p, k_j

# ---- end to end: evaluate(negatives=) against the host-built candidate matrix --------------------------------------------------
if a.eval_users > 0:
    ne = a.eval_users
    e_p, e_j, _, h_j = (t.cpu().numpy() for t in seen_rows(ne))
    full = sp.csr_matrix((np.ones(e_j.size), e_j, e_p), shape=(ne, n_item))
    held = sp.csr_matrix((np.ones(ne), h_j, np.arange(ne + 1)), shape=(ne, n_item))
    seen = (full - held).tocsr()
    seen.eliminate_zeros()
    model = WRMF(rank=r, lambda_=0.1, feedback="implicit", solver="conjugate_gradient", precision="float", rng=1, factor_init="device")
    model.fit_transform(full, n_iter=1, convergence_tol=-1)
    model.evaluate(seen, held, 10, negatives=10, seed=1)   # warm-up: the transform, the metrics, the sampler
    for n in (int(t) for t in a.n.split(",")):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev_ev = model.evaluate(seen, held, 10, negatives=n, seed=7)
        torch.cuda.synchronize()
        t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        lists = model._negatives_lists(seen, n_item, held, seen, np.zeros(0, np.int64))
        t_join = time.perf_counter() - t0
        o_p, o_j = R.sample_negatives(7, 0, lists[0].indptr, lists[0].indices, lists[1].indptr, lists[1].indices, n_item, n)
        cand = sp.csr_matrix((np.ones(o_j.size), o_j, o_p), shape=(ne, n_item))
        t_build = time.perf_counter() - t0
        host_ev = model.evaluate(seen, held, 10, candidates=cand)
        torch.cuda.synchronize()
        t_host = time.perf_counter() - t0
        line = {"what": "evaluate(negatives=n) against evaluate(candidates=<built on the host by the numpy specification>)",
                "users": ne, "items": n_item, "rank": r, "n": n, "k": 10, "evaluate_negatives_s": t_dev,
                "host_route_s": t_host, "of_which_host_build_s": t_build, "of_which_joining_the_lists_s": t_join,
                "host_over_device": t_host / t_dev,
                "equal": bool(all(np.array_equal(dev_ev[m], host_ev[m], equal_nan=True) for m in ("ap", "ndcg"))),
                "mean_ndcg": float(np.nanmean(dev_ev["ndcg"]))}
        print(json.dumps(line), flush=True)
        lines.append(line)
if a.out:
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(l) + "\n" for l in lines))
