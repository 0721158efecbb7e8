#!/usr/bin/env python
"""MMR re-ranking (wrmf_mmr.hip) at scale.  (a) Pools of --users x N items drawn uniformly without regard to the user (the rows a
re-ranking gathers are as scattered as a retrieval stage's) out of --items at rank --rank fp32, normal scores sorted descending,
re-ranked to k for every (N, k) of --shapes: `mmr_rerank` against `list_diversity` on the same n x N lists (one pass over exactly
the pool's rows: the HBM floor of the re-ranking), against the same algebra in torch on --torch-users of the lists (a gather of
the pool's rows, then k batched matrix-vector steps; the figure for all lists is an extrapolation from that chunk), and against
`top_product` at N, the ranking that feeds it.  --parent-lib lib.so: the parent commit's library, whose `list_diversity` and
`top_product` are timed in the same process.  (b) On --eval-users users of a model fitted for one iteration,
`evaluate(k=(5, 10, 20), negatives=99)` with and without `diversify=0.5`, and `predict(k=10)` with `diversify=None`, 0.5 and, with
--parent-lib, on the parent's library.  Host clock around calls that end in a device synchronise, one warm-up call, then the median
of --reps with the minimum and maximum; the calls of one group alternate within every repetition.

    python tools/gpu_mmr.py [--users 262144] [--shapes 100:10,1000:100] [--items 1000000] [--eval-users 10000] [--out FILE.jsonl]
"""
import argparse
import copy
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np
import scipy.sparse as sp
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from rsparse_amd import WRMF, _lib  # noqa: E402
from rsparse_amd.engine import HipBackend  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=262144)
ap.add_argument("--shapes", default="100:10,1000:100")
ap.add_argument("--items", type=int, default=1_000_000)
ap.add_argument("--rank", type=int, default=128)
ap.add_argument("--theta", type=float, default=0.5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--torch-users", type=int, default=16384)
ap.add_argument("--eval-users", type=int, default=10_000)
ap.add_argument("--eval-items", type=int, default=1_000_000)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()

be = HipBackend(0)
dev = be.device
g = torch.Generator(device=dev).manual_seed(1)
lines = []


def other_library(path):
    lib = ctypes.CDLL(str(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):   # (the parent's library lacks the entries this change adds)
            f = getattr(lib, name)
            f.restype, f.argtypes = res, args
    b = HipBackend(0)
    b.lib = lib
    return b


parent = other_library(a.parent_lib) if a.parent_lib else None


def stats(ts):
    return [sorted(ts)[len(ts) // 2] * 1e3, min(ts) * 1e3, max(ts) * 1e3]


def timed(fns):
    """{name: fn} -> {name: [median, min, max] ms}: one warm-up each, then --reps rounds that alternate the functions"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(a.reps):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[name].append(time.perf_counter() - t0)
    return {name: stats(v) for name, v in ts.items()}


def emit(line):
    print(json.dumps(line), flush=True)
    lines.append(line)


if a.users > 0:
    n, n_item, r, theta = a.users, a.items, a.rank, a.theta
    V = (torch.randn((n_item, r), generator=g, device=dev, dtype=torch.float32) * 0.1).contiguous()
    U = torch.randn((n, r), generator=g, device=dev, dtype=torch.float32)
    for shape in a.shapes.split(","):
        N, k = (int(t) for t in shape.split(":"))
        res = torch.randint(1, n_item + 1, (n, N), generator=g, device=dev, dtype=torch.int32)
        sc = torch.randn((n, N), generator=g, device=dev, dtype=torch.float64).sort(dim=1, descending=True).values.contiguous()
        want = ("scores", "objective")
        out = be.mmr_rerank(res, sc, V, 0, r, k, theta, want)
        again = be.mmr_rerank(res, sc, V, 0, r, k, theta, want)
        t = timed({"mmr_rerank": lambda: be.mmr_rerank(res, sc, V, 0, r, k, theta, want)})
        fns = {"list_diversity": lambda: be.list_diversity(res, (N,), V, 0, r, ("diversity",)),
               "top_product": lambda: be.top_product(U, V, N, None, None, None, 0.0)}
        if parent is not None:
            fns["list_diversity_parent"] = lambda: parent.list_diversity(res, (N,), V, 0, r, ("diversity",))
            fns["top_product_parent"] = lambda: parent.top_product(U, V, N, None, None, None, 0.0)
        t.update(timed(fns))
        nt = min(a.torch_users, n)
        inv = be.item_inv_norms(V, 0, r)

        def torch_route():
            it = (res[:nt] - 1).to(torch.int64)
            rows = V[it].to(torch.float64) * inv[it][:, :, None]                     # the gather: nt x N x r unit rows
            lo, hi = sc[:nt].min(dim=1, keepdim=True).values, sc[:nt].max(dim=1, keepdim=True).values
            lead = (1.0 - theta) * (sc[:nt] - lo) / (hi - lo)
            sim = torch.zeros((nt, N), dtype=torch.float64, device=dev)
            free = torch.ones((nt, N), dtype=torch.bool, device=dev)
            picks = torch.empty((nt, k), dtype=torch.int64, device=dev)
            ar = torch.arange(nt, device=dev)
            for step in range(k):
                obj = torch.where(free, lead - theta * sim, -torch.inf)
                i = obj.argmax(dim=1)
                picks[:, step] = i
                free[ar, i] = False
                dots = torch.bmm(rows, rows[ar, i][:, :, None])[:, :, 0]             # k batched matrix-vector steps
                sim = dots if step == 0 else torch.maximum(sim, dots)
            return picks
        tp = torch_route()
        t.update(timed({"torch": torch_route}))
        items_t = torch.gather(res[:nt], 1, tp.to(torch.int64))
        emit({"what": "mmr_rerank against list_diversity on the same lists, top_product at "
                      "the pool's width and the same algebra in torch on the first torch_users lists (extrapolated to all lists: x users / torch_users)",
              "users": n, "pool": N, "k": k, "items": n_item, "rank": r, "theta": theta, "reps": a.reps, "ms": t,
              "torch_users": nt, "torch_scaled_ms": t["torch"][0] * n / nt,
              "torch_scaled_over_kernel": t["torch"][0] * n / nt / t["mmr_rerank"][0],
              "kernel_over_list_diversity": t["mmr_rerank"][0] / t["list_diversity"][0],
              "kernel_over_top_product": t["mmr_rerank"][0] / t["top_product"][0],
              "share_of_lists_equal_to_torch": float((items_t == out["items"][:nt]).all(dim=1).double().mean()),
              "repeat_bit_identical": bool(all(torch.equal(again[m].view(torch.int32), out[m].view(torch.int32)) for m in again))})
        del res, sc, out, again, tp
    del V, U

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
    names = ("hit", "ndcg", "diversity")
    fns = {"evaluate": lambda: model.evaluate(seen, held, K, negatives=99, seed=7, metrics=names),
           "evaluate_diversify": lambda: model.evaluate(seen, held, K, negatives=99, seed=7, metrics=names, diversify=0.5),
           "predict": lambda: model.predict(seen, 10),
           "predict_diversify": lambda: model.predict(seen, 10, diversify=0.5)}
    if parent is not None:
        old = copy.copy(model)
        old._be = parent
        fns["predict_parent"] = lambda: old.predict(seen, 10)
        fns["evaluate_parent"] = lambda: old.evaluate(seen, held, K, negatives=99, seed=7, metrics=names)
    t = timed(fns)
    plain, div = fns["evaluate"](), fns["evaluate_diversify"]()
    line = {"what": "evaluate(k=(5, 10, 20), negatives=99; hit, ndcg, diversity) without and with diversify=0.5 (the pool: all 100 "
                    "candidates), predict(k=10) without and with diversify=0.5 (the pool: the top 100 of the catalogue), and the "
                    "undiversified calls on the parent's library",
            "users": ne, "items": n_item, "rank": r, "reps": a.reps, "ms": t,
            "means": {w: {m_: [float(x) for x in np.nanmean(ev[m_], axis=0)] for m_ in names} for w, ev in (("plain", plain), ("diversify", div))}}
    if parent is not None:
        p0, p1 = fns["predict"](), fns["predict_parent"]()
        line["predict_equal_to_parent"] = bool(np.array_equal(np.asarray(p0), np.asarray(p1)) and np.array_equal(p0.scores, p1.scores, equal_nan=True))
    emit(line)

if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("".join(json.dumps(line) + "\n" for line in lines))
