#!/usr/bin/env python3
"""`WRMF.predict(..., candidates=)` at scale: the top-k within per-user candidate lists (rsparse_hip_top_candidates_device,
wrmf_candidates.hip) on fp32 factors, every user with the same number of candidates (ascending, unique, one per stratum of the
catalogue).  Prints one JSON line per shape with three times, each the median of --reps calls after a warm-up, with min / max:

  (a) score_ms   the scoring launch alone (`HipBackend.score_pairs` on the candidate pattern);
  (b) call_ms    the whole `HipBackend.top_candidates` call (scores, keys and admissibility bits, plan, select and order);
  (c) torch_ms   the same lists through what a user can write today on the same GPU: `score_pairs`, then a segmented sort in torch
                 -- two stable `torch.sort` calls, by score (descending) and then by row -- and a gather of the first k;

and b_over_c, a_over_b, whether (b) and (c) return the same lists (normal factors: no ties), and whether (b) repeats bit for bit.

  python tools/gpu_candidates.py [--users 100000] [--items 1000000] [--rank 128] [--shapes 10:100,10:1000,100:1000] [--reps 5]
                                 [--out profiles/candidates/candidates.jsonl]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from rsparse_amd.engine import HipBackend  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=100_000)
ap.add_argument("--items", type=int, default=1_000_000)
ap.add_argument("--rank", type=int, default=128)
ap.add_argument("--shapes", default="10:100,10:1000,100:1000", help="k:candidates per user, comma separated")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()

be = HipBackend(0)
dev = be.device
g = torch.Generator(device=dev).manual_seed(1)
n, n_item, r = a.users, a.items, a.rank
U = torch.randn(n, r, generator=g, device=dev) * 0.1
V = torch.randn(n_item, r, generator=g, device=dev) * 0.1


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


def torch_route(p, j, k, c):
    sc, _, _ = be.score_pairs(U, V, p, j, 0.5)
    rows = torch.repeat_interleave(torch.arange(n, device=dev), c)
    o1 = torch.sort(sc, descending=True, stable=True).indices
    o2 = torch.sort(rows[o1], stable=True).indices
    perm = o1[o2].view(n, c)[:, :k]          # (every row has c candidates: its first k of the segmented order)
    return j[perm], sc[perm]


lines = []
for shape in a.shapes.split(","):
    k, c = (int(t) for t in shape.split(":"))
    assert n * c < 2 ** 31 and c <= n_item
    width = n_item // c
    j = (torch.arange(c, device=dev, dtype=torch.int64)[None, :] * width
         + torch.randint(0, width, (n, c), generator=g, device=dev)).to(torch.int32).reshape(-1)
    p = torch.arange(0, n * c + 1, c, device=dev, dtype=torch.int32)
    res, sc = be.top_candidates(U, V, k, p, j, None, None, None, 0.5)
    a_ms = timed(lambda: be.score_pairs(U, V, p, j, 0.5))
    b_ms = timed(lambda: be.top_candidates(U, V, k, p, j, None, None, None, 0.5))
    c_ms = timed(lambda: torch_route(p, j, k, c))
    res2, sc2 = be.top_candidates(U, V, k, p, j, None, None, None, 0.5)
    t_idx, t_sc = torch_route(p, j, k, c)
    line = {"what": "top_candidates (fp32 factors, double scores)", "users": n, "items": n_item, "rank": r, "k": k,
            "candidates_per_user": c, "candidates": n * c, "reps": a.reps,
            "score_ms": a_ms[0], "score_ms_min_max": list(a_ms[1:]), "call_ms": b_ms[0], "call_ms_min_max": list(b_ms[1:]),
            "torch_ms": c_ms[0], "torch_ms_min_max": list(c_ms[1:]), "b_over_c": b_ms[0] / c_ms[0], "a_over_b": a_ms[0] / b_ms[0],
            "rows_equal_to_torch": float(((res - 1) == t_idx).all(dim=1).float().mean()),
            "scores_equal_to_torch": bool(torch.equal(sc, t_sc)),
            "repeat_bit_identical": bool(torch.equal(res, res2) and torch.equal(sc.view(torch.int64), sc2.view(torch.int64)))}
    print(json.dumps(line), flush=True)
    lines.append(line)
    del j, p, res, sc, res2, sc2, t_idx, t_sc
if a.out:
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(l) + "\n" for l in lines))
