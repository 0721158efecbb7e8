"""The evaluation entries of ItemKNN (wrmf_itemknn.hip: score gather, candidate select, rank count) on one GPU at the shape of
profiles/itemknn: 1M x 100k, 5e7 entries, K = 50, 100 000 users at k = 10.  One JSON line per measurement, appended to
itemknn_eval_bench.jsonl.

    python profiles/itemknn_eval/itemknn_eval_bench.py [--parent-tree DIR]      every step, each a process of its own under
                                                                                 `timeout -k 10`; stops at the first that fails
    python profiles/itemknn_eval/itemknn_eval_bench.py --step calls              one step, in this process

Steps: calls (the new calls beside the unchanged `knn_recommend` on the same rows, and `ItemKNN.evaluate(negatives=99)` on 10 000
users), base (the fit and `knn_recommend` alone -- with --root DIR from the library of another built checkout, so that the driver
can alternate this tree with the parent's), bench (bench.py, alternating in the same way).  The kernels' own times come from a
profiler run of `--step calls --reps 1` (README.md).
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
OUT = HERE / "itemknn_eval_bench.jsonl"
K, TOPK, ROWS, EVAL_ROWS = 50, 10, 100_000, 10_000


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


def model(a, torch):
    """the synthetic pattern on the device, the cosine table fitted on it, and the first ROWS users' rows"""
    import numpy as np
    from rsparse_amd import _lib, synth
    from rsparse_amd.engine import HipBackend
    from rsparse_amd.itemknn import weight_table
    be = HipBackend()
    d = synth.make_dataset(a.users, a.items, mean_deg=a.nnz / a.users, device="cuda")
    (up, uj, _), (ip, iu, _) = d["c_iu"], d["c_ui"]
    i32 = lambda t: t.to(torch.int32).contiguous()
    ip, iu, up, uj = i32(ip), i32(iu), i32(up), i32(uj)
    fit = lambda: be.cooc_neighbors(ip, iu, up, uj, a.users, a.items, _lib.KNN_COSINE, K)
    nb, ct = fit()
    cnt = (ip[1:] - ip[:-1]).cpu().numpy().astype(np.int64)
    q = be.to_device(weight_table(nb.cpu().numpy(), ct.cpu().numpy(), cnt, "cosine"), torch.int64)
    n = min(ROWS, a.users)
    return be, fit, (up[:n + 1].contiguous(), uj, nb, q), cnt, int(d["nnz"])


def stratified(n, n_items, c, torch, gen):
    """c distinct ascending columns per row, one from each of c equal strata: (p, j) int32 on the device"""
    stride = n_items // c
    j = torch.arange(c, device="cuda")[None, :] * stride + torch.randint(0, stride, (n, c), device="cuda", generator=gen)
    return (torch.arange(n + 1, device="cuda") * c).to(torch.int32), j.reshape(-1).to(torch.int32).contiguous()


def step_base(a):
    import torch
    be, fit, (xp, uj, nb, q), _, nnz = model(a, torch)
    base = dict(step="base", tree=a.tree, users=a.users, items=a.items, nnz=nnz, K=K)
    say(what="fit", **timed(fit, a.reps, torch), **base)
    say(what="knn_recommend", k=TOPK, rows=int(xp.numel()) - 1, **timed(lambda: be.knn_recommend(xp, uj, nb, q, TOPK, xp, uj), a.reps, torch),
        **base)


def step_calls(a):
    import numpy as np
    import scipy.sparse as sp
    import torch
    from rsparse_amd import ItemKNN
    be, _, rows, cnt, nnz = model(a, torch)
    xp, uj, nb, q = rows
    n = int(xp.numel()) - 1
    gen = torch.Generator(device="cuda").manual_seed(5)
    base = dict(step="calls", users=a.users, items=a.items, nnz=nnz, K=K, k=TOPK, rows=n)
    say(what="knn_recommend", **timed(lambda: be.knn_recommend(*rows, TOPK, xp, uj), a.reps, torch), **base)
    for c in (100, 1000, 8192):
        cp, cj = stratified(n, a.items, c, torch, gen)
        say(what="knn_top_candidates", candidates_per_row=c,
            **timed(lambda: be.knn_top_candidates(*rows, TOPK, cp, cj, nr_p=xp, nr_j=uj), a.reps, torch), **base)
        if c == 100:
            say(what="knn_score_pairs", pairs_per_row=c, **timed(lambda: be.knn_score_pairs(*rows, cp, cj), a.reps, torch), **base)
    ap, aj = stratified(n, a.items, 1, torch, gen)
    say(what="knn_held_out_ranks", held_out_per_row=1, **timed(lambda: be.knn_held_out_ranks(*rows, ap, aj, nr_p=xp, nr_j=uj), a.reps, torch),
        **base)
    # the class: evaluate(negatives=99) on EVAL_ROWS users, host work included (the tables are set, not fitted again)
    m = ItemKNN(k_neighbors=K, similarity="cosine", backend=be)
    m.neighbors, m.item_count, m._d_tables = nb.cpu().numpy(), cnt, (nb, q)
    e = min(EVAL_ROWS, n)
    hp, hj = xp[:e + 1].cpu().numpy(), uj[:int(xp[e])].cpu().numpy()
    x = sp.csr_matrix((np.ones(hj.size), hj, hp), shape=(e, a.items))
    held = sp.csr_matrix((np.ones(e), aj[:e].cpu().numpy(), np.arange(e + 1)), shape=(e, a.items))
    for what, fn in (("evaluate(negatives=99)", lambda: m.evaluate(x, held, TOPK, metrics=("ndcg", "hit"), negatives=99, seed=7)),
                     ("evaluate()", lambda: m.evaluate(x, held, TOPK, metrics=("ndcg", "hit"))),
                     ("evaluate_ranks()", lambda: m.evaluate_ranks(x, held))):
        say(what=what, eval_rows=e, **timed(fn, max(2, a.reps // 2), torch), **{**base, "rows": e})


def step_bench(a):
    root = Path(a.root).resolve()
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2"], stdout=subprocess.PIPE, text=True,
                       cwd=str(root))
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    say(step="bench", what="bench.py --gpus 1 --steps 5 --warmup 2", tree=a.tree, rc=r.returncode, result=json.loads(line[-1]) if line else None)
    sys.exit(r.returncode)


STEPS = {"calls": step_calls, "base": step_base, "bench": step_bench}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=tuple(STEPS))
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--nnz", type=float, default=5e7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--root", default=str(HERE.parents[1]), help="the built checkout whose library and bench.py a step uses")
    ap.add_argument("--tree", default="this", help="the name of --root in the output")
    ap.add_argument("--parent-tree", default=None, help="another built checkout, for the base and bench steps to alternate with")
    ap.add_argument("--out", default=str(OUT), help="the .jsonl the measurements are appended to")
    a = ap.parse_args()
    say.out = a.out
    sys.path.insert(0, str(Path(a.root).resolve()))
    if a.step:
        STEPS[a.step](a)
        return
    trees = [("this", a.root)] + ([("parent", a.parent_tree)] if a.parent_tree else [])
    steps = [["--step", "calls"]]
    for step in ("base", "bench"):
        for rep in range(2 if a.parent_tree else 1):
            steps += [["--step", step, "--root", root, "--tree", name] for name, root in trees[::-1]]
    for s in steps:   # every GPU step a process of its own under its own time limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, str(Path(__file__).resolve()), "--reps", str(a.reps), "--users", str(a.users),
               "--items", str(a.items), "--nnz", str(a.nnz), *s, "--out", a.out]
        rc = subprocess.run(cmd).returncode
        if rc:
            say(step=s[1], failed=rc, args=s)
            sys.exit(rc)


if __name__ == "__main__":
    main()
