"""ItemKNN (wrmf_itemknn.hip) on one GPU at two shapes from rsparse_amd/synth.py: the bench matrix (1M x 100k, 5e7 entries) and the
largest catalogue whose dense rows the default workspace holds in one batch (16384 items; 163840 users).  One JSON line per
measurement, appended to itemknn_bench.jsonl.

    python profiles/itemknn/itemknn_bench.py                      every step, each a process of its own under `timeout -k 10`;
                                                                  stops at the first step that fails
    python profiles/itemknn/itemknn_bench.py --step model --users 1000000 --items 100000 --nnz 5e7      one step, in this process

Steps: model (the fit at K = 50, then the lists of 100 000 users at k = 10 from its table), skew (the fit after ONE item was added
to a tenth of the users, and to all of them), torch_sparse (the same algebra through torch.sparse on the same GPU: X^T X, then
topk per row), scipy (the host route, x.T @ x and argpartition per row, on fewer users), bench (bench.py, alternating with
the bench.py of another built checkout when --parent-tree names one).  The kernels' own times come from a profiler run of `--step model
--reps 1` (README.md).
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
OUT = HERE / "itemknn_bench.jsonl"
K, TOPK, PREDICT_USERS = 50, 10, 100_000


def say(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    with open(say.out, "a") as f:
        f.write(line + "\n")


say.out = OUT


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
    """both orientations of the synthetic pattern on the device: (ip, iu) item -> users, (up, uj) user -> items"""
    from rsparse_amd import synth
    d = synth.make_dataset(a.users, a.items, mean_deg=a.nnz / a.users, device="cuda")
    (up, uj, _), (ip, iu, _) = d["c_iu"], d["c_ui"]
    i32 = lambda t: t.to(torch.int32).contiguous()
    return int(d["nnz"]), (i32(ip), i32(iu)), (i32(up), i32(uj))


def work(ip, up, n_items, torch):
    """what a fit does, counted from the shapes: the scatter's atomics, the bytes of dense rows the select scans"""
    lens = (up[1:] - up[:-1]).to(torch.int64)
    return dict(scatter_atomics=int((lens * (lens - 1)).sum()), dense_bytes_per_row=4 * n_items, dense_gb=round(4 * n_items * n_items / 1e9, 2),
                longest_row=int(lens.max()), longest_column=int((ip[1:] - ip[:-1]).max()))


def step_model(a):
    import numpy as np
    import torch
    from rsparse_amd import _lib
    from rsparse_amd.engine import HipBackend
    from rsparse_amd.itemknn import weight_table
    be = HipBackend()
    nnz, (ip, iu), (up, uj) = dataset(a, torch)
    base = dict(step="model", users=a.users, items=a.items, nnz=nnz, K=K)
    for sim in ("cosine", "count"):
        code = {"cosine": _lib.KNN_COSINE, "count": _lib.KNN_COUNT}[sim]
        t = timed(lambda: be.cooc_neighbors(ip, iu, up, uj, a.users, a.items, code, K), a.reps, torch)
        say(what="fit", similarity=sim, **t, **work(ip, up, a.items, torch), **base)
    nb, ct = be.cooc_neighbors(ip, iu, up, uj, a.users, a.items, _lib.KNN_COSINE, K)
    cnt = (ip[1:] - ip[:-1]).cpu().numpy().astype(np.int64)
    q = be.to_device(weight_table(nb.cpu().numpy(), ct.cpu().numpy(), cnt, "cosine"), torch.int64)
    n = min(PREDICT_USERS, a.users)
    xp = up[:n + 1].contiguous()
    lens = (xp[1:] - xp[:-1]).to(torch.int64)
    for nr in (True, False):
        t = timed(lambda: be.knn_recommend(xp, uj, nb, q, TOPK, xp if nr else None, uj if nr else None), a.reps, torch)
        say(what="predict", k=TOPK, rows=n, not_recommend=nr, scatter_atomics_at_most=int(lens.sum()) * K, dense_bytes_per_row=8 * a.items,
            rows_per_batch=min(n, (1 << 30) // (8 * a.items)), **t, **base)


def step_skew(a):
    import torch
    from rsparse_amd import _lib
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    nnz, (ip, iu), (up, uj) = dataset(a, torch)
    dev = uj.device
    for every in (10, 1):   # item 0 joins the rows of every tenth user / of every user
        lens = (up[1:] - up[:-1]).to(torch.int64)
        rows = torch.repeat_interleave(torch.arange(a.users, device=dev), lens)
        keep = uj != 0
        add = torch.arange(0, a.users, every, device=dev)
        r2 = torch.cat([rows[keep], add])
        c2 = torch.cat([uj[keep].to(torch.int64), torch.zeros_like(add)])
        order = torch.argsort(r2 * a.items + c2)
        r2, c2 = r2[order], c2[order]
        p2 = torch.zeros(a.users + 1, dtype=torch.int64, device=dev)
        p2[1:] = torch.cumsum(torch.bincount(r2, minlength=a.users), 0)
        p2, j2 = p2.to(torch.int32), c2.to(torch.int32).contiguous()
        ones = torch.ones(int(j2.numel()), dtype=torch.float32, device=dev)
        ip2, iu2, _ = be.transpose_csc(a.items, a.users, p2, j2, ones)
        t = timed(lambda: be.cooc_neighbors(ip2, iu2, p2, j2, a.users, a.items, _lib.KNN_COSINE, K), a.reps, torch)
        say(step="skew", what="fit, item 0 held by every %s user" % ("tenth" if every == 10 else "single"), users=a.users, items=a.items,
            nnz=int(j2.numel()), K=K, **t, **work(ip2, p2, a.items, torch))


def step_torch_sparse(a):
    import torch
    nnz, _, (up, uj) = dataset(a, torch)
    vals = torch.ones(nnz, dtype=torch.float32, device=uj.device)
    x = torch.sparse_csr_tensor(up.to(torch.int64), uj.to(torch.int64), vals, size=(a.users, a.items))
    base = dict(step="torch_sparse", users=a.users, items=a.items, nnz=nnz, K=K)

    def route():
        xt = x.to_sparse_coo().t().coalesce()
        c = torch.sparse.mm(xt, x.to_sparse_coo()).to_dense()
        c.fill_diagonal_(0)
        return torch.topk(c, K, dim=1)
    try:
        say(what="X^T X through torch.sparse.mm, to_dense, topk per row (counts only: no cosine)", **timed(route, a.reps, torch), **base)
    except Exception as e:   # (reported, not fatal: the route is the yardstick, not the product)
        say(what="torch.sparse route", error=str(e)[:300], **base)


def step_scipy(a):
    import numpy as np
    import scipy.sparse as sp
    import torch
    nnz, _, (up, uj) = dataset(a, torch)
    x = sp.csr_matrix((np.ones(nnz), uj.cpu().numpy(), up.cpu().numpy()), shape=(a.users, a.items))
    del up, uj
    out = []
    for _ in range(max(1, a.reps)):
        t0 = time.perf_counter()
        c = (x.T @ x).tocsr()
        t1 = time.perf_counter()
        top = np.full((a.items, K), -1, dtype=np.int64)
        for i in range(a.items):
            j, v = c.indices[c.indptr[i]:c.indptr[i + 1]], c.data[c.indptr[i]:c.indptr[i + 1]]
            first = np.argpartition(-v, K - 1)[:K] if v.size > K else np.arange(v.size)
            top[i, :first.size] = j[first]
        out.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, c.nnz))
    say(step="scipy", what="host route: x.T @ x, argpartition per row (counts only: no cosine, no order among the K)", users=a.users,
        items=a.items, nnz=nnz, K=K, product_ms=round(statistics.median(o[0] for o in out), 1),
        argpartition_ms=round(statistics.median(o[1] for o in out), 1), product_nnz=int(out[0][2]))


def step_bench(a):
    """bench.py of this tree, alternating with the bench.py of another checkout (--parent-tree: built, with its own library)"""
    trees = [("this", ROOT)] + ([("parent", Path(a.parent_tree).resolve())] if a.parent_tree else [])
    for rep in range(2 if a.parent_tree else 1):
        for name, tree in trees[::-1]:
            r = subprocess.run([sys.executable, str(tree / "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2"], stdout=subprocess.PIPE,
                               text=True, cwd=str(tree))
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            say(step="bench", what="bench.py --gpus 1 --steps 5 --warmup 2", tree=name, rep=rep, rc=r.returncode,
                result=json.loads(line[-1]) if line else None)
            if r.returncode:
                sys.exit(r.returncode)


STEPS = {"model": step_model, "skew": step_skew, "torch_sparse": step_torch_sparse, "scipy": step_scipy, "bench": step_bench}


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
    steps = [["--step", "model", *big], ["--step", "model", *one_batch], ["--step", "skew", *big], ["--step", "skew", *one_batch],
             ["--step", "scipy", "--users", "20000", "--items", "16384", "--nnz", "1e6", "--reps", "1"],
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
