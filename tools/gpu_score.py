#!/usr/bin/env python3
"""`WRMF.score` / `evaluate_values` at scale: the pointwise-prediction kernel (rsparse_hip_score_pairs_device, wrmf_score.hip) on
fp32 factors at the stored positions of a users x items pattern.  Prints one JSON line per (rank, pattern): the call's time,
pairs/s and algorithmic bytes / time against 8 TB/s of HBM
(bytes = nnz (4 r gathered + 4 column index + 8 score) + 4 (n + 1) row pointers + n 4 r user vectors; the sums-only call reads
8 nnz of values and writes 16 n instead of the scores -- its scores go through the workspace: + 16 nnz), and the expression a
user writes today, `(U[rows].double() * V[cols].double()).sum(1)`, on the same tensors in the same session.  That expression
materialises 24 r bytes per pair, so it is timed over --torch-pairs positions and scaled to the whole count.

  python tools/gpu_score.py [--users 1000000] [--items 1000000] [--ranks 128,64] [--pairs 100000000] [--reps 5]
                            [--torch-pairs 10000000] [--out profiles/score_values/score_pairs.jsonl]

Two patterns per rank, the same number of pairs each: the row-length law of rsparse_amd.synth (log-normal, sigma = 1), and 1 %
of the rows holding half the pairs.  Columns are uniform.
"""
import argparse
import json
import math
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from rsparse_amd import synth  # noqa: E402
from rsparse_amd.engine import HipBackend  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=1_000_000)
ap.add_argument("--items", type=int, default=1_000_000)
ap.add_argument("--ranks", default="128,64")
ap.add_argument("--pairs", type=int, default=100_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--torch-pairs", type=int, default=10_000_000)
ap.add_argument("--out", default=None)
a = ap.parse_args()

be = HipBackend(0)
dev = be.device
g = torch.Generator(device=dev).manual_seed(1)
n, n_item = a.users, a.items


def scaled(w, total):
    """integer row lengths proportional to w that add up to `total`"""
    lens = torch.floor(w * (total / float(w.sum()))).to(torch.int64)
    lens[: total - int(lens.sum())] += 1
    return lens


def pattern(kind):
    users = torch.arange(n, dtype=torch.int64, device=dev)
    if kind == "synth":   # the law of synth.degrees, rescaled to the pair count
        w = synth.degrees(users, 20250222, a.pairs / n, 1 << 30, 1 << 30).to(torch.float64)
        lens = scaled(w, a.pairs)
    else:                 # 1 % of the rows hold half the pairs
        heavy = torch.zeros(n, dtype=torch.bool, device=dev)
        heavy[torch.linspace(0, n - 1, max(1, n // 100), device=dev).long()] = True
        nh = int(heavy.sum())
        lens = torch.empty(n, dtype=torch.int64, device=dev)
        lens[heavy] = scaled(torch.ones(nh, dtype=torch.float64, device=dev), a.pairs // 2)
        lens[~heavy] = scaled(torch.ones(n - nh, dtype=torch.float64, device=dev), a.pairs - a.pairs // 2)
    p64 = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    p64[1:] = torch.cumsum(lens, 0)
    assert int(p64[-1]) == a.pairs < 2 ** 31
    j = torch.randint(0, n_item, (a.pairs,), generator=g, device=dev, dtype=torch.int32)
    return p64.to(torch.int32), j, int(lens.max())


def timed(fn):
    fn()   # warm-up (code objects, the workspace)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


lines = []
for r in [int(t) for t in a.ranks.split(",")]:
    U = torch.randn(n, r, generator=g, device=dev) * 0.1
    V = torch.randn(n_item, r, generator=g, device=dev) * 0.1
    for kind in ("synth", "skewed"):
        p, j, longest = pattern(kind)
        nnz = a.pairs
        act = torch.randint(1, 6, (nnz,), generator=g, device=dev).to(torch.float64)
        first = be.score_pairs(U, V, p, j, 0.5, act)
        med, lo, hi = timed(lambda: be.score_pairs(U, V, p, j, 0.5))
        med_s, lo_s, hi_s = timed(lambda: be.score_pairs(U, V, p, j, 0.5, act, want_scores=False))
        again = be.score_pairs(U, V, p, j, 0.5, act)
        same = all(bool(torch.equal(x.view(torch.int64), y.view(torch.int64))) for x, y in zip(first, again))
        # the torch expression over a slice of the positions
        m = min(a.torch_pairs, nnz)
        rows = torch.repeat_interleave(torch.arange(n, device=dev), torch.diff(p.to(torch.int64)))[:m]
        cols = j[:m].to(torch.int64)
        med_t, lo_t, hi_t = timed(lambda: (U[rows].double() * V[cols].double()).sum(1) + 0.5)
        ref = (U[rows].double() * V[cols].double()).sum(1) + 0.5
        err = float((first[0][:m] - ref).abs().max())
        del rows, cols, ref
        nbytes = nnz * (4 * r + 4 + 8) + 4 * (n + 1) + n * 4 * r
        nbytes_s = nnz * (4 * r + 4 + 8 + 16) + 4 * (n + 1) + n * 4 * r + 4 * (n + 1) + 16 * n
        line = {"what": "score_pairs (fp32 factors, double accumulation)", "users": n, "items": n_item, "rank": r, "pattern": kind,
                "pairs": nnz, "longest_row": longest, "reps": a.reps,
                "scores_ms": med * 1e3, "scores_ms_min_max": [lo * 1e3, hi * 1e3], "pairs_per_sec": nnz / med,
                "algorithmic_bytes": nbytes, "gb_per_sec": nbytes / med / 1e9, "algorithmic_frac_of_8tbs_hbm": nbytes / med / 8e12,
                "sums_only_ms": med_s * 1e3, "sums_only_ms_min_max": [lo_s * 1e3, hi_s * 1e3],
                "sums_only_algorithmic_bytes": nbytes_s, "sums_only_frac_of_8tbs_hbm": nbytes_s / med_s / 8e12,
                "torch_pairs_timed": m, "torch_ms_for_those": med_t * 1e3, "torch_ms_scaled_to_all_pairs": med_t * 1e3 * nnz / m,
                "torch_over_kernel": (med_t * nnz / m) / med, "max_abs_diff_to_torch": err, "repeat_bit_identical": same,
                "rmse": math.sqrt(float(first[1].sum()) / nnz)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del p, j, act, first, again
    del U, V
if a.out:
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(l) + "\n" for l in lines))
