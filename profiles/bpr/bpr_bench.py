"""BPR (wrmf_bpr.hip) on one GPU at the shape of profiles/itemknn/: 1 000 000 users x 100 000 items, 5e7 entries with Zipf item
popularity (rsparse_amd.synth).  One JSON line per measurement, appended to --out (default bpr_bench.jsonl here); medians of
--reps runs behind a warm-up, each timed by two events around the call with the device idle before it.

    python profiles/bpr/bpr_bench.py --step epoch     one epoch at --ranks x --batches, fp32; the factor-row bytes the three gathers
                                                      of a step touch per second
    python profiles/bpr/bpr_bench.py --step uniform   the same with uniform item popularity (the same row lengths)
    python profiles/bpr/bpr_bench.py --step torch     one step written with torch (gathers, sigmoid, two index_add_: atomics)
    python profiles/bpr/bpr_bench.py --step fit       ten epochs from the device-drawn factors, and the fold-in of 100 000 users
The split of an epoch between the kernels is taken from a kernel trace of `--step epoch --reps 1` (the README says how).
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
OUT = HERE / "bpr_bench.jsonl"


def say(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def timed(fn, reps, torch):
    """device time between two events around the call, behind a warm-up call"""
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return {"ms": round(statistics.median(out), 3), "min": round(min(out), 3), "max": round(max(out), 3)}


def dataset(a, torch, uniform=False):
    """the canonical CSR rows on the device, int32 -> (nnz, p, j)"""
    from rsparse_amd import synth
    d = synth.make_dataset(a.users, a.items, mean_deg=a.nnz / a.users, device="cuda")
    p, j, _ = d["c_iu"]
    p, j = p.to(torch.int64), j.to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(a.users, device=p.device), p[1:] - p[:-1])
    if uniform:
        j = torch.randint(0, a.items, (int(j.numel()),), device=p.device, generator=torch.Generator(device=p.device).manual_seed(1))
    keys = torch.unique(rows * a.items + j)                                   # sorted and unique: canonical
    rows, j = keys // a.items, keys % a.items
    p = torch.zeros(a.users + 1, dtype=torch.int64, device=p.device)
    p[1:] = torch.cumsum(torch.bincount(rows, minlength=a.users), 0)
    return int(j.numel()), p.to(torch.int32).contiguous(), j.to(torch.int32).contiguous()


def factors(be, a, rank, torch, n_users=None):
    n_users = a.users if n_users is None else n_users
    U, V = be.init_factors(7, 0, n_users, rank, torch.float32), be.init_factors(7, 1, a.items, rank, torch.float32)
    aU, aV = (torch.zeros(n, dtype=torch.float64, device=be.device) for n in (n_users, a.items))
    return U, V, aU, aV


def step_epoch(a, uniform=False):
    import torch
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    nnz, p, j = dataset(a, torch, uniform)
    counts = torch.bincount(j.to(torch.int64), minlength=a.items)
    base = dict(users=a.users, items=a.items, nnz=nnz, popularity="uniform" if uniform else "zipf", hottest_item=int(counts.max()))
    for rank in a.ranks:
        for batch in a.batches:
            U, V, aU, aV = factors(be, a, rank, torch)
            res = []
            t = timed(lambda: res.append(be.bpr_epochs(p, j, a.items, nnz, 0, 11, 0, 0, 1, batch, U, V, aU, aV, 0.05, 0.01)), a.reps, torch)
            nv, nc = (int(v) for v in res[-1][0].tolist())
            # a step gathers U[u], V[i], V[j] for the score, V[i], V[j] again for the user rows and U[u] twice for the item rows
            gathered = 7 * nv * rank * 4
            say(step="uniform" if uniform else "epoch", rank=rank, batch=batch, steps=-(-nnz // batch), n_valid=nv, auc=round(nc / nv, 4),
                gathered_gb=round(gathered / 1e9, 2), gathered_tb_per_s=round(gathered / 1e12 / (t["ms"] / 1e3), 3), **t, **base)
            del U, V, aU, aV


def step_torch(a):
    """one step of batch triples with torch: the triples are the device sampler's, the update is plain SGD with index_add_"""
    import torch
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    nnz, p, j = dataset(a, torch)
    for rank in a.ranks:
        for batch in a.batches:
            n_steps = -(-nnz // batch)
            U, V, aU, aV = factors(be, a, rank, torch)
            u, i, n = (t.to(torch.int64) for t in be.bpr_triples(p, j, a.items, nnz, 0, 11, 0, 0, 0, n_steps))
            keep = n >= 0
            u, i, n = u[keep], i[keep], n[keep]

            def torch_step():
                Uu, D = U[u], V[i] - V[n]
                z = torch.sigmoid(-(Uu * D).sum(1, keepdim=True))
                gu, gv = z * D, z * Uu
                U.index_add_(0, u, 0.05 * gu)
                V.index_add_(0, i, 0.05 * gv)
                V.index_add_(0, n, -0.05 * gv)

            ours = lambda: be.bpr_step(p, j, a.items, nnz, 0, 11, 0, 0, 0, n_steps, U, V, aU, aV, 0.05, 0.01)
            say(step="torch", what="one step, torch gathers + sigmoid + index_add_ (atomics, not reproducible)", rank=rank, batch=batch,
                triples=int(u.numel()), **timed(torch_step, a.reps, torch))
            say(step="torch", what="one step, rsparse_hip_bpr_step_device (its scratch allocation included)", rank=rank, batch=batch,
                triples=int(u.numel()), **timed(ours, a.reps, torch))
            del U, V, aU, aV


def step_fit(a):
    import torch
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    nnz, p, j = dataset(a, torch)
    rank, batch = a.ranks[0], a.batches[-1]

    def fit():
        U, V, aU, aV = factors(be, a, rank, torch)
        return be.bpr_epochs(p, j, a.items, nnz, 0, 11, 0, 0, 10, batch, U, V, aU, aV, 0.05, 0.01), V, aV

    trace = []
    t = timed(lambda: trace.append(fit()), min(a.reps, 2), torch)
    counts, V, aV = trace[-1]
    say(step="fit", what="ten epochs, initial factors drawn on the device", rank=rank, batch=batch, nnz=nnz,
        auc_per_epoch=[round(int(c) / int(v), 4) for v, c in counts.tolist()], **t)
    n_new = 100_000
    pn = p[:n_new + 1].contiguous()
    jn = j[:int(pn[-1])].contiguous()

    def fold():
        U = torch.zeros((n_new, rank), dtype=torch.float32, device=be.device)
        aU = torch.zeros(n_new, dtype=torch.float64, device=be.device)
        return be.bpr_epochs(pn, jn, a.items, int(pn[-1]), 0, 11, 1, 0, a.transform_iter, 1, U, V, aU, aV, 0.05, 0.01, False)

    say(step="fit", what="fold-in of 100 000 users, the items frozen", rank=rank, epochs=a.transform_iter, nnz=int(pn[-1]),
        **timed(fold, min(a.reps, 2), torch))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True, choices=("epoch", "uniform", "torch", "fit"))
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--nnz", type=float, default=5e7)
    ap.add_argument("--ranks", type=lambda s: [int(v) for v in s.split(",")], default=[64, 128])
    ap.add_argument("--batches", type=lambda s: [int(v) for v in s.split(",")], default=[1 << 16, 1 << 18, 1 << 20])
    ap.add_argument("--transform-iter", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(OUT))
    a = ap.parse_args()
    OUT = Path(a.out)
    {"epoch": step_epoch, "uniform": lambda a: step_epoch(a, True), "torch": step_torch, "fit": step_fit}[a.step](a)
