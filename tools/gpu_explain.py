#!/usr/bin/env python3
"""`WRMF.explain` at scale: the contribution kernel (rsparse_hip_explain_device, wrmf_explain.hip) on fp32 factors for the
top-10 pairs of the users of a synthetic implicit-feedback matrix (rsparse_amd.synth), next to what a user has today on the same
tensors in the same session: `transform` of the same rows (the existing exact half-iteration: one k x k solve per user, no
explanation) and `WRMF._explain_host` run on the GPU (torch's batched linalg.cholesky_ex / cholesky_solve over padded rows).
Prints one JSON line per rank; kernel times are HIP events around the call, median and [min, max] over --reps after a warm-up.

  python tools/gpu_explain.py [--users 100000] [--items 100000] [--ranks 128,64] [--targets 10] [--reps 5]
                              [--torch-users 20000] [--out profiles/explain/explain.jsonl]

The phases are separated by differences of whole calls (the kernel has no timers): with 1 target per user instead of --targets the
per-target part (solve + contributions) is the slope; with every row cut to its first entry the assembly is a single term and what
is left of the 1-target call is the factorisation, the launch and one solve.
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from rsparse_amd import synth  # noqa: E402
from rsparse_amd.engine import HipBackend  # noqa: E402
from rsparse_amd.wrmf import WRMF  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=100_000)
ap.add_argument("--items", type=int, default=100_000)
ap.add_argument("--ranks", default="128,64")
ap.add_argument("--targets", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--torch-users", type=int, default=20_000)
ap.add_argument("--out", default=None)
a = ap.parse_args()

be = HipBackend(0)
dev = be.device
g = torch.Generator(device=dev).manual_seed(1)
n, n_item, lam = a.users, a.items, 0.1
d = synth.make_dataset(n, n_item, device=dev)
x_p, x_j, c = d["c_iu"]                       # columns = users: the CSR rows of the users x items matrix
del d
lens = torch.diff(x_p.to(torch.int64))


def timed(fn):
    fn()   # warm-up (code objects, torch's allocator)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)[len(ms) // 2], [min(ms), max(ms)]


def targets(per_user):
    t_p = torch.arange(0, (n + 1) * per_user, per_user, dtype=torch.int32, device=dev)
    t_j = torch.randint(0, n_item, (n * per_user,), generator=g, device=dev, dtype=torch.int32)
    return t_p, t_j


lines = []
for r in [int(t) for t in a.ranks.split(",")]:
    V = torch.randn(n_item, r, generator=g, device=dev) * 0.1
    G = (V.double().T @ V.double() + lam * torch.eye(r, device=dev, dtype=torch.float64)).float()
    wa, wb = c - 1.0, c
    t_p, t_j = targets(a.targets)
    t1_p, t1_j = targets(1)
    first_p = torch.arange(n + 1, dtype=torch.int32, device=dev)          # every row cut to its first entry
    first = x_p[:-1].to(torch.int64)
    run = lambda tp, tj: be.explain_pairs(V, G, 0.0, 0.0, x_p, x_j, wa, wb, tp, tj)
    out = run(t_p, t_j)
    assert int(out[2].sum()) == 0
    ms_all, mm_all = timed(lambda: run(t_p, t_j))
    ms_one, mm_one = timed(lambda: run(t1_p, t1_j))
    ms_cut, mm_cut = timed(lambda: be.explain_pairs(V, G, 0.0, 0.0, first_p, x_j[first], wa[first], wb[first], t1_p, t1_j))
    again = run(t_p, t_j)
    same = all(bool(torch.equal(p.view(torch.uint8), q.view(torch.uint8))) for p, q in zip(out[:3], again[:3]))
    # the wrapper's own share (segment layout, output allocation): the same call without the kernel's work
    none_p = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    ms_wrap, _ = timed(lambda: be.explain_pairs(V, G, 0.0, 0.0, x_p, x_j, wa, wb, none_p, t_j[:0]))
    # transform of the same rows: the exact half-iteration from zeros
    csc = be.make_csc(n_item, n, x_p, x_j, c)
    emb = torch.zeros((n, r), dtype=torch.float32, device=dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    ms_tr, mm_tr = timed(lambda: be.half_iteration(csc, True, V, emb, G, lam, 0, 3, True, loss, None))
    be.check_numeric()
    sc, _, _ = be.score_pairs(emb, V, t_p, t_j)
    diff = float((out[1] - sc).abs().max())
    # the torch fallback on the GPU, over the first --torch-users users
    m = min(a.torch_users, n)
    sub = lambda p: p[:m + 1].contiguous()
    ms_t, mm_t = timed(lambda: WRMF._explain_host(V, G, 0.0, 0.0, sub(x_p), x_j, wa, wb, sub(t_p), t_j[:int(t_p[m])]))
    ref = WRMF._explain_host(V, G, 0.0, 0.0, sub(x_p), x_j, wa, wb, sub(t_p), t_j[:int(t_p[m])])
    err = float((out[1][:int(t_p[m])] - ref[1]).abs().max())
    per_target = (ms_all - ms_one) / max(a.targets - 1, 1)
    nnz, pairs = int(lens.sum()), n * a.targets
    line = {"what": "explain_pairs (fp32 factors)", "users": n, "items": n_item, "rank": r, "nnz": nnz, "longest_row": int(lens.max()),
            "targets_per_user": a.targets, "pairs": pairs, "contributions": int(out[0].numel()), "reps": a.reps,
            "explain_ms": ms_all, "explain_ms_min_max": mm_all, "users_per_sec": n / ms_all * 1e3, "pairs_per_sec": pairs / ms_all * 1e3,
            "explain_1_target_ms": ms_one, "explain_1_target_ms_min_max": mm_one,
            "explain_rows_cut_to_1_entry_1_target_ms": ms_cut, "explain_rows_cut_ms_min_max": mm_cut,
            "wrapper_only_ms": ms_wrap,
            "per_target_solve_and_contributions_ms": per_target,
            "assemble_ms_estimate": ms_one - ms_cut, "factor_and_one_solve_ms_estimate": ms_cut - ms_wrap,
            "transform_same_rows_ms": ms_tr, "transform_ms_min_max": mm_tr, "explain_over_transform": ms_all / ms_tr,
            "max_abs_total_minus_transform_score": diff,
            "torch_users_timed": m, "torch_ms_for_those": ms_t, "torch_ms_min_max": mm_t, "torch_ms_scaled_to_all_users": ms_t * n / m,
            "torch_over_kernel": (ms_t * n / m) / ms_all, "max_abs_total_diff_to_torch": err, "repeat_bit_identical": same}
    print(json.dumps(line), flush=True)
    lines.append(line)
    del V, G, out, again, emb, csc, ref
if a.out:
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(l) + "\n" for l in lines))
