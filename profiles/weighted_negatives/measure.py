#!/usr/bin/env python3
"""Popularity-weighted negative sampling at scale (rsparse_hip_sample_negatives_weighted_device, wrmf_sample_weighted.hip) next to
the uniform sampler on the same rows.  Items have Zipf interaction counts (count of the item of popularity rank k = 1e7 / k, the
ranks shuffled over the ids); every user has about 100 seen items drawn in proportion to those counts (so the popular items are
in the histories), one of them held out (`keep`).  Weights = quantize_weights((count + 1) ** power).  Prints one JSON line per
(power, n) with, each the median of --reps calls after a warm-up with min / max (host clock around calls that end in a device
synchronise; the variants of one repetition are timed one after the other, so a drift of the machine hits all of them):

  weighted_ms   the whole `rsparse_hip_sample_negatives_weighted_device` call: the row-pointer scan, its read-back, the launch;
  uniform_ms    `rsparse_hip_sample_negatives_device` on the same rows;
  prefix_ms     `rsparse_hip_weights_prefix_device` (once per evaluation, not per batch);
  <label>:...   the same entries of every library named by --also LABEL=PATH (another build of the library, e.g. the parent
                commit's: entries it lacks are skipped), interleaved with this one's;

the filled rows, whether the call repeats bit for bit, and row 0 checked against the numpy specification.  Then, on --eval-users
users of a model fitted for one iteration, the wall time of `evaluate(negatives=n, negative_weights=w)` against the same evaluation
with the candidate matrix built on the host by the numpy specification and passed as `candidates=`, and whether the two agree.

  python profiles/weighted_negatives/measure.py [--users 100000] [--items 1000000] [--powers 0.75,1.0] [--n 99,999] [--reps 7]
                                                [--eval-users 10000] [--also parent=PATH] [--out FILE.jsonl]
"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np
import scipy.sparse as sp
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from rsparse_amd import WRMF, _lib, rng as R  # noqa: E402
from rsparse_amd.engine import HipBackend  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=100_000)
ap.add_argument("--items", type=int, default=1_000_000)
ap.add_argument("--rank", type=int, default=128)
ap.add_argument("--powers", default="0.75,1.0")
ap.add_argument("--n", default="99,999")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--eval-users", type=int, default=10_000)
ap.add_argument("--also", action="append", default=[])
ap.add_argument("--out", default=None)
a = ap.parse_args()

be = HipBackend(0)
dev = be.device
n_u, n_item = a.users, a.items
counts = np.random.default_rng(1).permutation(1e7 / np.arange(1, n_item + 1, dtype=np.float64))


def seen_rows(n_rows, seed):
    """(seen_p, seen_j, keep_p, keep_j) on the device: 100 draws per row in proportion to the counts, duplicates removed (about 90
    distinct items, the popular ones among them); keep = the row's first item"""
    g = torch.Generator(device=dev).manual_seed(seed)
    prob = torch.from_numpy(counts).to(dev, torch.float32)
    items = torch.multinomial(prob, n_rows * 100, replacement=True, generator=g)
    keys = torch.unique(torch.arange(n_rows, device=dev).repeat_interleave(100) * n_item + items)      # sorted: by row, then item
    rows, s_j = keys // n_item, (keys % n_item).to(torch.int32)
    s_p = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(torch.bincount(rows, minlength=n_rows), 0)]).to(torch.int32)
    return s_p, s_j.contiguous(), torch.arange(n_rows + 1, dtype=torch.int32, device=dev), s_j[s_p[:-1].long()].contiguous()


libs = {"": _lib.load()}
for spec in a.also:
    label, path = spec.split("=", 1)
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    libs[label + ":"] = lib


def med(ts):
    return {"ms": sorted(ts)[len(ts) // 2] * 1e3, "min_max": [min(ts) * 1e3, max(ts) * 1e3]}


def interleaved(calls):
    """{name: fn} -> {name: median / min / max of --reps timings}, one warm-up each, then the variants in turn per repetition"""
    ts = {k: [] for k in calls}
    for rep in range(a.reps + 1):
        for k, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                ts[k].append(time.perf_counter() - t0)
    return {k: med(v) for k, v in ts.items()}


s_p, s_j, k_p, k_j = seen_rows(n_u, 1)
lines = []
for power in (float(t) for t in a.powers.split(",")):
    w = R.quantize_weights((counts + 1.0) ** power)
    d_w = torch.from_numpy(w.view(np.int32)).to(dev)
    cum = be.weights_prefix(d_w)
    seen_share = float(torch.from_numpy(w.astype(np.float64)).to(dev)[s_j.long()].sum() / n_u / float(w.astype(np.float64).sum()))
    for n in (int(t) for t in a.n.split(",")):
        c_p, c_j, filled = be.sample_negatives_weighted(7, 0, s_p, s_j, k_p, k_j, n_item, n, cum)
        c_p2, c_j2, _ = be.sample_negatives_weighted(7, 0, s_p, s_j, k_p, k_j, n_item, n, cum)
        cap = int(c_j.numel())
        out_p, out_j = torch.empty_like(c_p), torch.empty_like(c_j)
        cum2, fl = torch.empty_like(cum), torch.zeros(1, dtype=torch.int32, device=dev)
        calls = {}
        for label, lib in libs.items():
            if hasattr(lib, "rsparse_hip_sample_negatives_weighted_device"):
                calls[label + "weighted"] = lambda lib=lib: _lib.check(lib.rsparse_hip_sample_negatives_weighted_device(
                    7, 0, n_u, n_item, n, s_p.data_ptr(), s_j.data_ptr(), k_p.data_ptr(), k_j.data_ptr(), cum.data_ptr(), out_p.data_ptr(),
                    out_j.data_ptr(), cap, fl.data_ptr(), None))
                calls[label + "prefix"] = lambda lib=lib: _lib.check(lib.rsparse_hip_weights_prefix_device(d_w.data_ptr(), n_item, cum2.data_ptr(), None))
            calls[label + "uniform"] = lambda lib=lib: _lib.check(lib.rsparse_hip_sample_negatives_device(
                7, 0, n_u, n_item, n, s_p.data_ptr(), s_j.data_ptr(), k_p.data_ptr(), k_j.data_ptr(), out_p.data_ptr(), out_j.data_ptr(), cap, None))
        t = interleaved(calls)
        e0 = int(s_p[1])
        want = R.sample_negatives_weighted(7, 0, s_p[:2].cpu().numpy(), s_j[:e0].cpu().numpy(), k_p[:2].cpu().numpy(), k_j[:1].cpu().numpy(),
                                           n_item, n, w)
        line = {"what": "sample_negatives_weighted next to sample_negatives on the same rows", "users": n_u, "items": n_item, "power": power,
                "n": n, "seen_per_user": float(s_j.numel()) / n_u, "weight_share_of_a_seen_row": seen_share, "candidates": cap,
                "reps": a.reps, "filled_rows": filled}
        for k, v in t.items():
            line[k + "_ms"], line[k + "_ms_min_max"] = v["ms"], v["min_max"]
        for label, lib in libs.items():   # another build's rows are this build's
            if label and label + "weighted" in calls:
                out_j.fill_(-1)
                calls[label + "weighted"]()
                torch.cuda.synchronize()
                line[label + "equals_this_build"] = bool(torch.equal(out_p, c_p) and torch.equal(out_j, c_j))
        line["weighted_over_uniform"] = t["weighted"]["ms"] / t["uniform"]["ms"]
        line["repeat_bit_identical"] = bool(torch.equal(c_p, c_p2) and torch.equal(c_j, c_j2))
        line["row0_equals_specification"] = bool(np.array_equal(c_j[:int(c_p[1])].cpu().numpy(), want[1]))
        print(json.dumps(line), flush=True)
        lines.append(line)
        del c_p, c_j, c_p2, c_j2, out_p, out_j
del s_p, s_j, k_p, k_j

# ---- end to end: evaluate(negatives=, negative_weights=) against the host-built candidate matrix -------------------------------
if a.eval_users > 0:
    ne, r = a.eval_users, a.rank
    e_p, e_j, _, h_j = (t.cpu().numpy() for t in seen_rows(ne, 2))
    full = sp.csr_matrix((np.ones(e_j.size), e_j, e_p), shape=(ne, n_item))
    held = sp.csr_matrix((np.ones(ne), h_j, np.arange(ne + 1)), shape=(ne, n_item))
    seen = (full - held).tocsr()
    seen.eliminate_zeros()
    w = R.quantize_weights((counts + 1.0) ** 0.75)
    model = WRMF(rank=r, lambda_=0.1, feedback="implicit", solver="conjugate_gradient", precision="float", rng=1, factor_init="device")
    model.fit_transform(full, n_iter=1, convergence_tol=-1)
    model.evaluate(seen, held, 10, negatives=10, seed=1, negative_weights=w)   # warm-up: the transform, the metrics, the sampler
    for n in (int(t) for t in a.n.split(",")):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev_ev = model.evaluate(seen, held, 10, negatives=n, seed=7, negative_weights=w)
        torch.cuda.synchronize()
        t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        lists = model._negatives_lists(seen, n_item, held, seen, np.zeros(0, np.int64))
        o_p, o_j, _ = R.sample_negatives_weighted(7, 0, lists[0].indptr, lists[0].indices, lists[1].indptr, lists[1].indices, n_item, n, w)
        cand = sp.csr_matrix((np.ones(o_j.size), o_j, o_p), shape=(ne, n_item))
        t_build = time.perf_counter() - t0
        host_ev = model.evaluate(seen, held, 10, candidates=cand)
        torch.cuda.synchronize()
        t_host = time.perf_counter() - t0
        line = {"what": "evaluate(negatives=n, negative_weights=w) against evaluate(candidates=<built on the host by the numpy specification>)",
                "users": ne, "items": n_item, "rank": r, "power": 0.75, "n": n, "k": 10, "evaluate_negatives_s": t_dev, "host_route_s": t_host,
                "of_which_host_build_s": t_build, "host_over_device": t_host / t_dev,
                "equal": bool(all(np.array_equal(dev_ev[m], host_ev[m], equal_nan=True) for m in ("ap", "ndcg"))),
                "mean_ndcg": float(np.nanmean(dev_ev["ndcg"]))}
        print(json.dumps(line), flush=True)
        lines.append(line)
if a.out:
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(l) + "\n" for l in lines))
