#!/usr/bin/env python
"""Beyond-accuracy metrics of the lists (wrmf_lists.hip, wrmf_diversity.hip) at scale.  (a) Lists of --users x --k items drawn
with Zipf popularity (item = floor(n_item ^ u), u uniform: P(item) ~ 1 / item, the hottest item takes ln 2 / ln n_item of all
positions) out of --items, at --cutoffs: `list_metrics` with the five per-row outputs without and with the exposure histogram,
against `hit_metrics` on the same lists, and the exposure histogram on UNIFORM lists of the same shape (what the same-address
atomics on the hottest items cost).  (b) `list_diversity` at rank --rank fp32 on the same lists against `score_pairs` on a pattern
with the same row gathers, and against the same algebra in torch (index gather of n x k x r, cumulative sum, norms) on
--torch-users of the lists.  (c) On --eval-users users of a model fitted for one iteration, `evaluate(k=(5, 10, 20), negatives=99)`
with every new metric against the accuracy metrics alone, and against the host route: lists and factors copied back, the numpy
definitions.  Host clock around calls that end in a device synchronise, one warm-up call, then the median of --reps with the
minimum and maximum.

    python tools/gpu_list_metrics.py [--users 262144] [--k 2000] [--items 1000000] [--eval-users 10000] [--out FILE.jsonl]
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
from rsparse_amd import metrics as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=262144)
ap.add_argument("--k", type=int, default=2000)
ap.add_argument("--items", type=int, default=1_000_000)
ap.add_argument("--cutoffs", default="10,20,50,100,500,1000,2000")
ap.add_argument("--rank", type=int, default=128)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--torch-users", type=int, default=4096)
ap.add_argument("--eval-users", type=int, default=10_000)
ap.add_argument("--eval-items", type=int, default=1_000_000)
ap.add_argument("--out", default=None)
a = ap.parse_args()

be = HipBackend(0)
dev = be.device
g = torch.Generator(device=dev).manual_seed(1)
lines = []


def timed(fn, before=None):
    if before:
        before()
    fn()   # warm-up (code objects)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        if before:
            before()
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return [sorted(ts)[len(ts) // 2] * 1e3, min(ts) * 1e3, max(ts) * 1e3]


def emit(line):
    print(json.dumps(line), flush=True)
    lines.append(line)


if a.users > 0:
    n, k, n_item, r = a.users, a.k, a.items, a.rank
    cutoffs = tuple(int(t) for t in a.cutoffs.split(",") if int(t) <= k)
    T = len(cutoffs)
    u = torch.rand((n, k), generator=g, device=dev, dtype=torch.float64)
    res = torch.clamp(torch.floor(torch.exp(u * np.log(n_item))), 1, n_item).to(torch.int32)   # Zipf, 1-based
    del u
    uni = torch.randint(1, n_item + 1, (n, k), generator=g, device=dev, dtype=torch.int32)
    cnt = torch.clamp((n_item / torch.arange(1, n_item + 1, device=dev, dtype=torch.float64)), max=2 ** 31 - 1).to(torch.int32)
    info = be.to_device(M.self_information(cnt.cpu().numpy()), torch.int64)
    p = (torch.arange(n + 1, device=dev, dtype=torch.int64) * 8).to(torch.int32)
    j = torch.randint(0, n_item, (n * 8,), generator=g, device=dev, dtype=torch.int32).view(n, 8).sort(dim=1).values.flatten()
    rows = ("valid", "count_sum", "info_sum", "popularity", "novelty")
    expo = torch.zeros((T, n_item), dtype=torch.int32, device=dev)
    first = be.list_metrics(res, cutoffs, n_item, rows, cnt, info)
    again = be.list_metrics(res, cutoffs, n_item, rows, cnt, info)
    t_rows = timed(lambda: be.list_metrics(res, cutoffs, n_item, rows, cnt, info))
    t_valid = timed(lambda: be.list_metrics(res, cutoffs, n_item, ("valid",)))
    t_zero = timed(lambda: expo.zero_())
    t_exp = timed(lambda: be.list_metrics(res, cutoffs, n_item, rows, cnt, info, expo), before=lambda: expo.zero_())
    t_exp_only = timed(lambda: be.list_metrics(res, cutoffs, n_item, (), exposure=expo), before=lambda: expo.zero_())
    hottest = int(expo.sum(dim=0).max())
    t_exp_uni = timed(lambda: be.list_metrics(uni, cutoffs, n_item, (), exposure=expo), before=lambda: expo.zero_())
    t_hit = timed(lambda: be.hit_metrics(res, p, j, cutoffs, ("hits", "first", "precision", "recall", "hit", "mrr")))
    t_copy = timed(lambda: res.clone())
    emit({"what": "list_metrics (five per-row outputs) without / with exposure, exposure alone on Zipf and on uniform lists, "
                  "hit_metrics (six outputs, 8 held-out items per row) and a device copy of the lists",
          "users": n, "k": k, "items": n_item, "cutoffs": list(cutoffs), "reps": a.reps, "list_bytes": n * k * 4,
          "list_metrics_ms": t_rows, "list_metrics_valid_only_ms": t_valid, "list_metrics_with_exposure_ms": t_exp,
          "exposure_zero_ms": t_zero, "exposure_only_zipf_ms": t_exp_only, "exposure_only_uniform_ms": t_exp_uni,
          "hit_metrics_ms": t_hit, "lists_clone_ms": t_copy, "lists_gb_per_s_list_metrics": n * k * 4 / t_rows[0] / 1e6,
          "atomics": n * cutoffs[-1], "atomics_per_ns_zipf": n * cutoffs[-1] / t_exp_only[0] / 1e6,
          "atomics_per_ns_uniform": n * cutoffs[-1] / t_exp_uni[0] / 1e6, "hottest_item_count": hottest,
          "repeat_bit_identical": bool(all(torch.equal(first[m].view(torch.int32), again[m].view(torch.int32)) for m in rows))})
    del uni, first, again, expo

    V = (torch.randn((n_item, r), generator=g, device=dev, dtype=torch.float32) * 0.1).contiguous()
    U = torch.randn((n, r), generator=g, device=dev, dtype=torch.float32)
    c_last = cutoffs[-1]
    t_inv = timed(lambda: be.item_inv_norms(V, 0, r), before=be.drop_v32)
    d0 = be.list_diversity(res, cutoffs, V, 0, r)
    d1 = be.list_diversity(res, cutoffs, V, 0, r)
    t_div = timed(lambda: be.list_diversity(res, cutoffs, V, 0, r))
    head = (res[:, :c_last] - 1).contiguous().flatten()
    pp = (torch.arange(n + 1, device=dev, dtype=torch.int64) * c_last).to(torch.int32)
    t_score = timed(lambda: be.score_pairs(U, V, pp, head))
    nt = min(a.torch_users, n)
    inv = be.item_inv_norms(V, 0, r)
    cut_t = torch.tensor(cutoffs, device=dev) - 1

    def torch_route():
        it = (res[:nt, :c_last] - 1).to(torch.int64)
        rows_ = V[it].to(torch.float64) * inv[it][:, :, None]
        S = torch.cumsum(rows_, dim=1)[:, cut_t, :]
        m_ = (cut_t + 1).to(torch.float64)[None, :]
        return 1.0 - ((S * S).sum(dim=2) - m_) / (m_ * (m_ - 1.0))
    tt = torch_route()
    t_torch = timed(torch_route)
    dd = d0["diversity"][:nt]
    ok = ~torch.isnan(dd)
    gathered = n * c_last * (r * 4 + 8 + 4)
    emit({"what": "list_diversity (fp32 factors) against score_pairs on a pattern with the same row gathers and the same algebra in "
                  "torch on the first torch_users lists (scaled to all lists: x users / torch_users)",
          "users": n, "k": k, "items": n_item, "rank": r, "cutoffs": list(cutoffs), "reps": a.reps, "item_inv_norms_ms": t_inv,
          "list_diversity_ms": t_div, "score_pairs_ms": t_score, "diversity_over_score_pairs": t_div[0] / t_score[0],
          "torch_users": nt, "torch_ms": t_torch, "torch_scaled_ms": t_torch[0] * n / nt, "torch_scaled_over_kernel": t_torch[0] * n / nt / t_div[0],
          "algorithmic_bytes": gathered, "tb_per_s": gathered / t_div[0] / 1e9, "fraction_of_8_tb_per_s": gathered / t_div[0] / 1e9 / 8.0,
          "max_abs_diff_to_torch": float((dd[ok] - tt[ok]).abs().max()), "mean_diversity_last_cutoff": float(d0["diversity"][:, -1].mean()),
          "repeat_bit_identical": bool(torch.equal(d0["diversity"].view(torch.int64), d1["diversity"].view(torch.int64)))})
    del res, V, U, head, pp, d0, d1, tt

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
    pop = np.asarray((seen != 0).sum(axis=0)).ravel().astype(np.int64)
    model = WRMF(rank=r, lambda_=0.1, feedback="implicit", solver="conjugate_gradient", precision="float", rng=1, factor_init="device")
    model.fit_transform(full, n_iter=1, convergence_tol=-1)
    K = (5, 10, 20)
    new = ("popularity", "novelty", "diversity", "gini", "entropy")
    acc = ("hit", "ndcg", "coverage")
    model.evaluate(seen, held, K, negatives=10, seed=1, metrics=acc + new, item_popularity=pop)   # warm-up

    def wall(fn):
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return out, [sorted(ts)[len(ts) // 2] * 1e3, min(ts) * 1e3, max(ts) * 1e3]

    _, t_acc = wall(lambda: model.evaluate(seen, held, K, negatives=99, seed=7, metrics=acc))
    ev, t_all = wall(lambda: model.evaluate(seen, held, K, negatives=99, seed=7, metrics=acc + new, item_popularity=pop))
    # the host route: the lists and the factors copied back, the numpy definitions
    res_d, _, _ = model._predict_device(seen, 20, "x", (), None,
                                        (99, 7, M.canonical_actual(held, ne), None))
    info = M.self_information(pop)

    def host_route():
        top = res_d.cpu().numpy().astype(np.int64) - 1
        Vh = model._V.cpu().numpy()
        ref = M.list_metrics_reference(top, K, n_item, pop, info)
        div = M.list_diversity_reference(top, K, Vh, 0, Vh.shape[1])
        return ref, div, M.exposure_summary(ref["exposure"])
    (ref, div, summ), t_host = wall(host_route)
    emit({"what": "evaluate(k=(5, 10, 20), negatives=99) with the accuracy metrics (hit, ndcg, coverage) alone, with the five new "
                  "metrics beside them, and the host route for the five (lists and factors copied back, the numpy definitions)",
          "users": ne, "items": n_item, "rank": r, "reps": a.reps, "accuracy_only_ms": t_acc, "with_new_metrics_ms": t_all,
          "new_metrics_add_ms": t_all[0] - t_acc[0], "host_route_ms": t_host, "host_over_added": t_host[0] / max(t_all[0] - t_acc[0], 1e-9),
          "popularity_equal": bool(np.array_equal(ev["popularity"], ref["popularity"], equal_nan=True)),
          "novelty_equal": bool(np.array_equal(ev["novelty"], ref["novelty"], equal_nan=True)),
          "gini_equal": bool(np.array_equal(ev["gini"], summ["gini"])),
          "diversity_max_abs_diff": float(np.nanmax(np.abs(ev["diversity"] - div["diversity"]))),
          "means": {k_: [float(x) for x in np.atleast_1d(v)] for k_, v in M.summarize({n_: ev[n_] for n_ in new}).items()}})

if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("".join(json.dumps(line) + "\n" for line in lines))
