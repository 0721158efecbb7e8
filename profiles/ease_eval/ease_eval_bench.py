"""EASE under candidates=, sampled negatives, score and the full-ranking metrics on one GPU, at the shape of profiles/ease:
100 000 users x 20 000 items with about 100 items each (rsparse_amd/synth.py), random weights (the times do not depend on their
values), k = 10, not_recommend = x.  One JSON line per measurement, appended to ease_eval_bench.jsonl; medians of --reps calls
behind a warm-up call, host clock around a device synchronise.

    --step full         `ease_recommend` over the whole catalogue: what a user had before.  With RSPARSE_HIP_LIB naming the
                        parent's library this is the parent's call.
    --step candidates   `ease_top_candidates` at --m candidates per user (several: --m 100 320 ...), drawn one per equal stratum
                        of the catalogue (distinct, ascending).  --ratio names the RSPARSE_HIP_EASE_CELLS_RATIO the loaded library
                        was built with (a label: the route of a row is the library's decision).
    --step score        `ease_score_pairs` at --m cells per user
    --step ranks        `ease_held_out_ranks`, one held-out item per user
    --step evaluate     `EASE.evaluate(negatives=99, seed=7)` against `EASE.evaluate` over the catalogue and `evaluate_ranks`, on the
                        first 10 000 users, host work included

The kernels' own times come from a profiler run of `--step candidates --m 100 1000 --reps 1` (README.md).
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
OUT = HERE / "ease_eval_bench.jsonl"
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
    """the CSR rows of the synthetic pattern, int32 on the device -> (nnz, up, uj)"""
    from rsparse_amd import synth
    d = synth.make_dataset(a.users, a.items, mean_deg=a.nnz / a.users, device="cuda")
    up, uj, _ = d["c_iu"]
    return int(uj.numel()), up.to(torch.int32).contiguous(), uj.to(torch.int32).contiguous()


def weights(a, dtype, torch, be):
    n = a.items
    ld = (n * dtype.itemsize + 255) // 256 * 256 // dtype.itemsize
    B = torch.randn((n, ld), dtype=dtype, device=be.device)
    B[:, :n].fill_diagonal_(0.0)
    return B


def strata(n_rows, n_items, m, torch, seed=1):
    """m columns per row, one from each of m equal strata of the catalogue: distinct and ascending -> (p, j) int32 on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    width = n_items // m
    j = torch.arange(m, device="cuda", dtype=torch.int64)[None, :] * width + torch.randint(0, width, (n_rows, m), device="cuda", generator=g)
    p = torch.arange(n_rows + 1, device="cuda", dtype=torch.int64) * m
    return p.to(torch.int32), j.reshape(-1).to(torch.int32).contiguous()


def base(a, nnz, **kw):
    return dict(users=a.users, items=a.items, nnz=nnz, k=TOPK, lib=os.environ.get("RSPARSE_HIP_LIB", "this tree's"), **kw)


def run(a):
    import torch
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    nnz, up, uj = dataset(a, torch)
    n = a.items
    for dtype in [torch.float32] + ([torch.float64] if a.double else []):
        B = weights(a, dtype, torch, be)
        tag = base(a, nnz, dtype=str(dtype))
        if a.step == "full":
            say(step="full", **tag, **timed(lambda: be.ease_recommend(up, uj, B, n, TOPK, up, uj), a.reps, torch))
        elif a.step == "candidates":
            for m in a.m:
                cp, cj = strata(a.users, n, m, torch)
                route = "cells" if m <= 4096 and m * a.ratio <= n else "dense"
                say(step="candidates", m=m, ratio=a.ratio, route=route, cell_lines_gb=round(nnz * m * 128 / 1e9, 1), **tag,
                    **timed(lambda: be.ease_top_candidates(up, uj, B, n, TOPK, cp, cj, up, uj), a.reps, torch))
                del cp, cj
        elif a.step == "score":
            for m in a.m:
                pp, pj = strata(a.users, n, m, torch, seed=2)
                say(step="score", m=m, ratio=a.ratio, **tag, **timed(lambda: be.ease_score_pairs(up, uj, B, n, pp, pj), a.reps, torch))
        elif a.step == "ranks":
            ap, aj = strata(a.users, n, 1, torch, seed=3)
            say(step="ranks", held_out_per_user=1, **tag, **timed(lambda: be.ease_held_out_ranks(up, uj, B, n, ap, aj, up, uj), a.reps, torch))
        del B


def step_evaluate(a):
    import numpy as np
    import scipy.sparse as sp
    import torch
    from rsparse_amd import EASE
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    nnz, up, uj = dataset(a, torch)
    n, rows = a.items, 10_000
    p = up[:rows + 1].cpu().numpy().astype(np.int64)
    x = sp.csr_matrix((np.ones(p[-1]), uj[:p[-1]].cpu().numpy(), p), shape=(rows, n))
    x.sort_indices()
    rng = np.random.default_rng(4)
    free = np.ones((rows, n), dtype=bool)
    free[x.nonzero()] = False
    held_j = np.array([rng.choice(np.flatnonzero(free[u])) for u in range(rows)])
    held = sp.csr_matrix((np.ones(rows), held_j, np.arange(rows + 1)), shape=(rows, n))
    m = EASE(backend=be)
    m._B, m._n_items, m.item_count = weights(a, torch.float32, torch, be), n, np.bincount(x.indices, minlength=n)
    tag = base(a, nnz, eval_users=rows, dtype="torch.float32")
    metrics = ("ndcg", "hit")
    say(step="evaluate", what="evaluate(negatives=99, seed=7)", **tag,
        **timed(lambda: m.evaluate(x, held, TOPK, metrics=metrics, negatives=99, seed=7), a.reps, torch))
    cand = m.sample_negatives(x, 99, actual=held, seed=7)
    say(step="evaluate", what="evaluate(candidates=the same 100 per user, sampled before)", **tag,
        **timed(lambda: m.evaluate(x, held, TOPK, metrics=metrics, candidates=cand), a.reps, torch))
    say(step="evaluate", what="evaluate over the catalogue", **tag, **timed(lambda: m.evaluate(x, held, TOPK, metrics=metrics), a.reps, torch))
    say(step="evaluate", what="evaluate_ranks", **tag, **timed(lambda: m.evaluate_ranks(x, held), a.reps, torch))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True, choices=("full", "candidates", "score", "ranks", "evaluate"))
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--items", type=int, default=20_000)
    ap.add_argument("--nnz", type=float, default=1e7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--m", type=int, nargs="+", default=[100])
    ap.add_argument("--ratio", type=int, default=None)
    ap.add_argument("--double", action="store_true")
    a = ap.parse_args()
    if a.ratio is None:
        from rsparse_amd import _lib
        a.ratio = _lib.EASE_CELLS_RATIO
    step_evaluate(a) if a.step == "evaluate" else run(a)
