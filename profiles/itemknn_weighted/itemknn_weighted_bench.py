"""ItemKNN on weighted values (wrmf_itemknn.hip, the uint64 forms) on one GPU, at the two shapes of profiles/itemknn: the bench
matrix (1M x 100k, 5e7 entries) and 163840 x 16384.  One JSON line per measurement, appended to itemknn_weighted_bench.jsonl.

    python profiles/itemknn_weighted/itemknn_weighted_bench.py            every step, each a process of its own under `timeout -k 10`;
                                                                          stops at the first step that fails
    python profiles/itemknn_weighted/itemknn_weighted_bench.py --step model --users 163840 --items 16384 --nnz 8.192e6

Steps: model (the cosine fit on BM25 weights at K = 50 and, in the same process, the binary cosine fit on the same pattern; then
the lists of 100 000 users at k = 10 with and without the rows' weights), skew (both fits after item 0 joined every user; weighted
by "log", since BM25's idf of a column that every user holds is negative), torch_sparse (W^T W through torch.sparse.mm, to_dense,
topk on the same GPU), bench (bench.py, alternating with another built checkout when --parent-tree names one; profiles/itemknn's
step).  The kernels' own times come from a profiler run of `--step model --reps 1` (README.md)."""
import argparse
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "profiles" / "itemknn")]
import itemknn_bench as base   # noqa: E402

OUT = HERE / "itemknn_weighted_bench.jsonl"
K, TOPK, PREDICT_USERS = base.K, base.TOPK, base.PREDICT_USERS
say, timed = base.say, base.timed


def weighted(be, kind, n_users, n_items, up, uj, torch):
    """the pattern with drawn counts 1 .. 5, weighted by `kind` on the device and quantised to 16 bits there (one multiplication
    and rint: the bits of the numpy rule) -> (ip, iu, il, ur, a, b): the operands and tables of the weighted cosine"""
    from rsparse_amd import Confidence
    g = torch.Generator(device="cuda").manual_seed(1)
    v = torch.randint(1, 6, (int(uj.numel()),), generator=g, device="cuda").to(torch.float64)
    um = (up, uj, v)
    conf = Confidence(kind)
    im = be.transpose_csc(n_items, n_users, *um) if conf.needs_items() else None
    mom = conf.device_fit(be, n_users, n_items, um, im)
    w = conf.device_apply(be, um, conf.device_user_table(be, um, mom))
    assert bool((w > 0).all())
    scale = 65535.0 / float(w.max())
    q = torch.clamp(torch.round(w * scale), min=1.0, max=65535.0)
    S = torch.zeros(n_items, dtype=torch.float64, device="cuda").index_add_(0, uj.to(torch.int64), q * q)
    a = torch.sqrt(torch.where(S > 0, S, torch.ones_like(S)))
    ip, iu, il = be.transpose_csc(n_items, n_users, up, uj, q)
    longest = int((ip[1:] - ip[:-1]).max())
    assert 65535 * 65535 * longest < 2 ** 53
    return ip, iu, il, q, a, a.clone()


def fits(be, a, ip, iu, il, up, uj, ur, ta, tb, what, torch, **extra):
    from rsparse_amd import _lib
    work = base.work(ip, up, a.items, torch)
    t = timed(lambda: be.cooc_neighbors_weighted(ip, iu, il, up, uj, ur, a.users, a.items, ta, tb, 0.0, K), a.reps, torch)
    say(what=what + ", weighted cosine", **t, **{**work, "dense_bytes_per_row": 8 * a.items}, **extra)
    t2 = timed(lambda: be.cooc_neighbors(ip, iu, up, uj, a.users, a.items, _lib.KNN_COSINE, K), a.reps, torch)
    say(what=what + ", binary cosine on the same pattern", **t2, **work, **extra)
    say(what=what + ": weighted / binary", ratio=round(t["ms"] / t2["ms"], 3), **extra)


def step_model(a):
    import numpy as np
    import torch
    from rsparse_amd.engine import HipBackend
    from rsparse_amd.itemknn import weighted_similarity_values, weighted_weight_table
    be = HipBackend()
    nnz, _, (up, uj) = base.dataset(a, torch)
    ip, iu, il, ur, ta, tb = weighted(be, "bm25", a.users, a.items, up, uj, torch)
    extra = dict(step="model", users=a.users, items=a.items, nnz=nnz, K=K, weights="bm25")
    fits(be, a, ip, iu, il, up, uj, ur, ta, tb, "fit", torch, **extra)
    nb, sums = be.cooc_neighbors_weighted(ip, iu, il, up, uj, ur, a.users, a.items, ta, tb, 0.0, K)
    sim = weighted_similarity_values(nb.cpu().numpy(), sums.cpu().numpy().view(np.uint64), ta.cpu().numpy(), tb.cpu().numpy(), 0.0)
    q = be.to_device(weighted_weight_table(sim)[0], torch.int64)
    n = min(PREDICT_USERS, a.users)
    xp = up[:n + 1].contiguous()
    for xv in (ur, None):
        t = timed(lambda: be.knn_recommend(xp, uj, nb, q, TOPK, xp, uj, xv=xv), a.reps, torch)
        say(what="predict", k=TOPK, rows=n, not_recommend=True, row_weights=xv is not None, dense_bytes_per_row=8 * a.items, **t, **extra)


def step_skew(a):
    import torch
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    nnz, _, (up, uj) = base.dataset(a, torch)
    dev = uj.device
    lens = (up[1:] - up[:-1]).to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(a.users, device=dev), lens)
    keep = uj != 0
    add = torch.arange(0, a.users, device=dev)                             # item 0 joins the row of every user
    r2 = torch.cat([rows[keep], add])
    c2 = torch.cat([uj[keep].to(torch.int64), torch.zeros_like(add)])
    order = torch.argsort(r2 * a.items + c2)
    r2, c2 = r2[order], c2[order]
    p2 = torch.zeros(a.users + 1, dtype=torch.int64, device=dev)
    p2[1:] = torch.cumsum(torch.bincount(r2, minlength=a.users), 0)
    p2, j2 = p2.to(torch.int32), c2.to(torch.int32).contiguous()
    ip, iu, il, ur, ta, tb = weighted(be, "log", a.users, a.items, p2, j2, torch)
    fits(be, a, ip, iu, il, p2, j2, ur, ta, tb, "fit, item 0 held by every user", torch, step="skew", users=a.users, items=a.items,
         nnz=int(j2.numel()), K=K, weights="log")


def step_torch_sparse(a):
    import torch
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    nnz, _, (up, uj) = base.dataset(a, torch)
    _, _, _, q, _, _ = weighted(be, "bm25", a.users, a.items, up, uj, torch)
    x = torch.sparse_csr_tensor(up.to(torch.int64), uj.to(torch.int64), q, size=(a.users, a.items))
    extra = dict(step="torch_sparse", users=a.users, items=a.items, nnz=nnz, K=K)

    def route():
        xt = x.to_sparse_coo().t().coalesce()
        c = torch.sparse.mm(xt, x.to_sparse_coo()).to_dense()
        c.fill_diagonal_(0)
        return torch.topk(c, K, dim=1)
    try:
        say(what="W^T W through torch.sparse.mm (float64), to_dense, topk per row (dot products only: no cosine)", **timed(route, a.reps, torch), **extra)
    except Exception as e:   # (reported, not fatal: the route is the yardstick, not the product)
        say(what="torch.sparse route", error=str(e)[:300], **extra)


STEPS = {"model": step_model, "skew": step_skew, "torch_sparse": step_torch_sparse, "bench": base.step_bench}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=tuple(STEPS))
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--nnz", type=float, default=5e7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--parent-tree", default=None, help="another built checkout, for the bench step to alternate with")
    ap.add_argument("--out", default=str(OUT), help="the .jsonl the measurements are appended to")
    a = ap.parse_args()
    say.out = a.out
    if a.step:
        STEPS[a.step](a)
        return
    big, one_batch = ["--users", "1000000", "--items", "100000", "--nnz", "5e7"], ["--users", "163840", "--items", "16384", "--nnz", "8.192e6"]
    steps = [["--step", "model", *one_batch], ["--step", "model", *big], ["--step", "skew", *one_batch], ["--step", "skew", *big],
             ["--step", "bench"] + (["--parent-tree", a.parent_tree] if a.parent_tree else []),
             ["--step", "torch_sparse", *one_batch, "--reps", "2"]]   # (last: the one step whose work is not this project's)
    for s in steps:   # every GPU step a process of its own under its own time limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, str(Path(__file__).resolve()), "--reps", str(a.reps), *s, "--out", a.out]
        rc = subprocess.run(cmd).returncode
        if rc:
            say(step=s[1], failed=rc, args=s)
            sys.exit(rc)


if __name__ == "__main__":
    main()
