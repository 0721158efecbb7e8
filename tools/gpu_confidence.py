#!/usr/bin/env python3
"""The confidence weighting at scale (wrmf_confidence.hip through HipBackend.confidence_{moments,table,apply}) on the synthetic
users x items matrix of bench.py (rsparse_amd.synth.make_dataset), values as doubles, both orientations resident.  One JSON line
per measurement, each the median of --reps calls after a warm-up, timed with HIP events:

  moments / apply   per kind and per orientation; `clone_ms` is torch.clone of the tensors the call must read and write (x for
                    the moments; x, the gathered index array where a table is gathered, and the output for apply), `over_clone`
                    the ratio, `GBps` those bytes over the call's time;
  skew              the same entries with ONE segment holding half of them, and the ratio to the balanced case;
  torch             the same algebra in torch on the same tensors: repeat_interleave row ids, index_add_ for the sums, gathers
                    and element-wise ops for bm25 (with and without the row ids precomputed);
  end to end        (--e2e-users x --e2e-items, rank 128 float, ten iterations) WRMF(preprocess=Confidence("bm25")).fit_transform
                    and predict of --e2e-new users, against the same model with a host callable that computes the numpy reference.

  python tools/gpu_confidence.py [--users 10000000] [--items 1000000] [--reps 5] [--e2e-users 1000000] [--e2e-items 100000]
                                 [--e2e-new 100000] [--out profiles/confidence/confidence.jsonl]
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
from rsparse_amd import WRMF, Confidence, synth  # noqa: E402
from rsparse_amd.confidence import confidence_reference  # noqa: E402
from rsparse_amd.engine import HipBackend  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=10_000_000)
ap.add_argument("--items", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--e2e-users", type=int, default=1_000_000)
ap.add_argument("--e2e-items", type=int, default=100_000)
ap.add_argument("--e2e-new", type=int, default=100_000)
ap.add_argument("--out", default=None)
a = ap.parse_args()

be = HipBackend(0)
dev = be.device
lines = []


def emit(line):
    print(json.dumps(line), flush=True)
    lines.append(line)


def timed(fn):
    fn()   # warm-up (code objects, the workspace, the caching allocator)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


def nbytes(ts):
    return sum(t.numel() * t.element_size() for t in ts)


if a.users > 0:
    d = synth.make_dataset(a.users, a.items, device=str(dev), feedback="implicit")
    sides = {"user-major": tuple(t.to(dev).contiguous() for t in d["c_iu"]), "item-major": tuple(t.to(dev).contiguous() for t in d["c_ui"])}
    del d
    sides = {k: (p, i, x.to(torch.float64)) for k, (p, i, x) in sides.items()}
    n_user, n_item, nnz = a.users, a.items, int(sides["user-major"][2].numel())
    shape = {"users": n_user, "items": n_item, "nnz": nnz, "reps": a.reps}
    um, im = sides["user-major"], sides["item-major"]
    out64 = torch.empty_like(um[2])

    # ---- moments ----
    base = {}
    for side, (p, i, x) in sides.items():
        c_ms = timed(lambda: x.clone())
        for power in (1, 2):
            one, t1 = be.confidence_moments(p, x, power)
            two, t2 = be.confidence_moments(p, x, power)
            ms = timed(lambda: be.confidence_moments(p, x, power))
            base[(side, power)] = ms
            emit(dict(shape, what="moments", side=side, power=power, ms=ms, clone_ms=c_ms, over_clone=ms / c_ms,
                      GBps=nbytes([x]) / ms / 1e6, repeat_bit_identical=bool(torch.equal(one, two) and torch.equal(t1, t2))))

    # ---- apply, per kind and orientation ----
    kinds = [("linear", {"alpha": 40.0}), ("log", {"alpha": 40.0, "eps": 1.0}), ("tfidf", {}), ("bm25", {}),
             ("normalize", {"target": "rows"}), ("normalize", {"target": "columns"})]
    apply_ms = {}
    for kind, par in kinds:
        c = Confidence(kind, **par)
        mom = c.device_fit(be, n_user, n_item, um, im)
        ut = c.device_user_table(be, um, mom)
        for side, arrays, item_major in (("user-major", um, False), ("item-major", im, True)):
            seg, idx = (c._state["item_table"], ut) if item_major else (ut, c._state["item_table"])
            moved = [arrays[2], out64] + ([arrays[1]] if idx is not None else [])
            c_ms = timed(lambda: [t.clone() for t in moved])
            w = c.device_apply(be, arrays, ut, item_major=item_major)
            ms = timed(lambda: c.device_apply(be, arrays, ut, item_major=item_major))
            ms32 = timed(lambda: c.device_apply(be, arrays, ut, item_major=item_major, out=torch.float32))
            apply_ms[(kind, par.get("target"), side)] = ms
            emit(dict(shape, what="apply", kind=kind, params=par, side=side, ms=ms, float_out_ms=ms32, clone_ms=c_ms, over_clone=ms / c_ms,
                      GBps=nbytes(moved) / ms / 1e6, finite=bool(torch.isfinite(w).all())))
            del w
        fit_ms = timed(lambda: c.device_user_table(be, um, c.device_fit(be, n_user, n_item, um, im)))
        emit(dict(shape, what="fit (moments + tables, with the value check's read-back)", kind=kind, params=par, ms=fit_ms))

    # ---- the same algebra in torch (bm25) ----
    p, j, x = um
    K1, B = 100.0, 0.8
    lens = torch.diff(p.to(torch.int64))
    rows = torch.repeat_interleave(torch.arange(n_user, device=dev), lens)
    idf = Confidence("bm25")
    idf.device_fit(be, n_user, n_item, um, im)
    idf_t = idf._state["item_table"]
    j64 = j.to(torch.int64)

    def torch_moments(r):
        return torch.zeros(n_user, dtype=torch.float64, device=dev).index_add_(0, r, x)

    def torch_bm25(r):
        s_u = torch_moments(r)
        KL = K1 * ((1.0 - B) + (B * s_u) / (s_u.sum() / n_user))
        return ((x * (K1 + 1.0)) / (KL[r] + x)) * idf_t[j64]

    t_rows = timed(lambda: torch.repeat_interleave(torch.arange(n_user, device=dev), lens))
    t_mom = timed(lambda: torch_moments(rows))
    t_all = timed(lambda: torch_bm25(rows))
    hip_all = base[("user-major", 1)] + apply_ms[("bm25", None, "user-major")]
    emit(dict(shape, what="torch: bm25 on the user-major arrays", row_ids_ms=t_rows, index_add_ms=t_mom, moments_and_apply_ms=t_all,
              with_row_ids_ms=t_all + t_rows, hip_moments_ms=base[("user-major", 1)], hip_moments_and_apply_ms=hip_all,
              torch_over_hip=t_all / hip_all, torch_with_row_ids_over_hip=(t_all + t_rows) / hip_all))
    del rows, j64, lens

    # ---- skew: one segment holds half of all entries ----
    n_seg = n_user
    rest = nnz - nnz // 2
    cuts = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), nnz // 2, dtype=torch.int64, device=dev),
                      nnz // 2 + (torch.arange(1, n_seg, dtype=torch.int64, device=dev) * rest) // (n_seg - 1)])
    p_skew = cuts.to(torch.int32)
    table = torch.rand(n_seg, dtype=torch.float64, device=dev) + 100.0
    ms_m = timed(lambda: be.confidence_moments(p_skew, x, 1))
    ms_a = timed(lambda: be.confidence_apply("bm25", p_skew, j, x, seg_table=table, idx_table=idf_t, a=K1))
    emit(dict(shape, what="skew: one segment of nnz / 2 entries", moments_ms=ms_m, moments_over_balanced=ms_m / base[("user-major", 1)],
              apply_bm25_ms=ms_a, apply_over_balanced=ms_a / apply_ms[("bm25", None, "user-major")]))
    del sides, um, im, out64, p, j, x, table, p_skew, cuts, idf, idf_t
    torch.cuda.empty_cache()

# ---- end to end ----
if a.e2e_users > 0:
    d = synth.make_dataset(a.e2e_users + a.e2e_new, a.e2e_items, device=str(dev), feedback="implicit")
    p, j, v = (t.cpu().numpy() for t in d["c_iu"])
    del d
    full = sp.csr_matrix((v.astype(np.float64), j, p), shape=(a.e2e_users + a.e2e_new, a.e2e_items))
    full.has_canonical_format = True
    train, new = full[:a.e2e_users], full[a.e2e_users:]
    state = {}

    def host_bm25(m):
        """the callable route: numpy on the host, on whatever block and orientation the hook is handed"""
        r = sp.csr_matrix(m)
        if "st" not in state:
            from rsparse_amd.confidence import confidence_fit_reference
            state["st"] = confidence_fit_reference(r, "bm25")
            return sp.csc_matrix(confidence_reference(r, "bm25", state["st"]))
        return sp.csc_matrix(confidence_reference(r, "bm25"))      # (at inference the hook sees the transposed block)

    for name, pre in (("Confidence('bm25')", Confidence("bm25")), ("host callable (numpy reference)", host_bm25)):
        res = {}
        for rep in range(2):    # (the first run loads code objects and sizes the workspaces)
            state.clear()
            m = WRMF(rank=128, lambda_=0.1, precision="float", preprocess=pre, rng=1, factor_init="device")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.fit_transform(train, n_iter=10, convergence_tol=-1)
            torch.cuda.synchronize()
            res["fit_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            m.predict(new, 10)
            torch.cuda.synchronize()
            res["predict_s"] = time.perf_counter() - t0
        emit(dict(what="end to end: fit_transform (10 iterations, rank 128 float) and predict of new users, k = 10", preprocess=name,
                  users=a.e2e_users, items=a.e2e_items, nnz=int(train.nnz), new_users=a.e2e_new, new_nnz=int(new.nnz), **res))
    t0 = time.perf_counter()
    m = WRMF(rank=128, lambda_=0.1, precision="float", rng=1, factor_init="device")
    m.fit_transform(train, n_iter=10, convergence_tol=-1)
    torch.cuda.synchronize()
    emit(dict(what="end to end: the same fit without a preprocess", fit_s=time.perf_counter() - t0))

if a.out:
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(l) + "\n" for l in lines))
