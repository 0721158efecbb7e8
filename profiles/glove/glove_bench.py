"""GloVe (wrmf_glove.hip) on one GPU: a synthetic symmetric co-occurrence matrix of --n items and about --entries stored entries
(both indices cubic-skewed, so a few items are in very many pairs; the cell counts are the values), fp32.  One JSON line per
measurement, appended to --out (default glove_bench.jsonl here); medians of --reps runs behind a warm-up, each timed by two events
around the call with the device idle before it.

    python profiles/glove/glove_bench.py --step epoch       the index build, one epoch and one step at --ranks x --batches; the bytes
                                                            of factor rows gathered per second (both sides together)
    python profiles/glove/glove_bench.py --step torch       one step against the same step written with torch index_add_ (float
                                                            atomics, plain SGD, not reproducible), in alternating pairs
    python profiles/glove/glove_bench.py --step heavy       one epoch on a matrix whose row 0 (and column 0) holds a tenth of the
                                                            entries against a balanced matrix of the same size (--entries 10 n)
    python profiles/glove/glove_bench.py --step movielens   cost_history after 10 epochs on the MovieLens-100k item co-occurrence
                                                            at batch 2^10, 2^14 and 2^18
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
OUT = HERE / "glove_bench.jsonl"
X_MAX, ALPHA = 10.0, 0.75


def say(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def event_ms(fn, torch):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(fn, reps, torch):
    """device time between two events around the call, behind a warm-up call"""
    fn()
    out = [event_ms(fn, torch) for _ in range(reps)]
    return {"ms": round(statistics.median(out), 3), "min": round(min(out), 3), "max": round(max(out), 3)}


def dataset(n, entries, torch, heavy=False, skew=3):
    """the stored positions of a symmetric n x n count matrix on the device, in CSR order -> (rows, cols, fx, lx); heavy: row 0 and
    column 0 are full"""
    g = torch.Generator(device="cuda").manual_seed(1)
    m = entries // 2
    r = lambda: (torch.rand(m, device="cuda", generator=g) ** skew * n).long()
    i, j = r(), r()
    if heavy:
        i[:n], j[:n] = 0, torch.arange(n, device="cuda")
    key, cnt = torch.unique(torch.cat([i * n + j, j * n + i]), return_counts=True)          # sorted: the CSR order
    x = cnt.double()
    fx = torch.where(x < X_MAX, (x / X_MAX) ** ALPHA, torch.ones_like(x)).float()
    return (key // n).int().contiguous(), (key % n).int().contiguous(), fx, x.log().float()


def parameters(be, n, rank, torch):
    W = [be.init_factors(7, s, n, rank, torch.float32, scale=0.1) for s in (0, 1)]
    b = [torch.zeros(n, dtype=torch.float32, device=be.device) for _ in range(2)]
    return (*W, *b, *(torch.ones(s, dtype=torch.float64, device=be.device) for s in ((n, rank), (n, rank), n, n)))


def epochs_of(a, pos, tag, be, torch):
    nnz = int(pos[0].numel())
    for batch in a.batches:
        n_steps = -(-nnz // batch)
        index = None

        def build():
            nonlocal index
            index = be.glove_index(pos[0], pos[1], a.n, n_steps)

        ms = event_ms(build, torch)                                       # (once: its first call, scratch allocation included)
        say(step="index", matrix=tag, batch=batch, steps=n_steps, nnz=nnz, index_gb=round(index[0].numel() / 1e9, 2), ms=round(ms, 3))
        for rank in a.ranks:
            st = parameters(be, a.n, rank, torch)
            t = timed(lambda: be.glove_epochs(*pos, index, 1, *st, 0.05, 0.0), a.reps, torch)
            gathered = 2 * nnz * rank * 4                                 # a row of W_j per slot on the row side, of W_i on the column side
            say(step="epoch", matrix=tag, rank=rank, batch=batch, steps=n_steps, n=a.n, nnz=nnz, gathered_gb=round(gathered / 1e9, 1),
                gathered_tb_per_s=round(gathered / 1e12 / (t["ms"] / 1e3), 3), **t)
            one = timed(lambda: be.glove_step(*pos, index, 0, *st, 0.05, 0.0), a.reps, torch)
            say(step="one_step", what="step 0, scratch allocation and the read-back of the step ranges included", matrix=tag, rank=rank,
                batch=batch, slots=-(-nnz // n_steps), **one)
            del st
        del index


def step_epoch(a):
    import torch
    from rsparse_amd.engine import HipBackend
    epochs_of(a, dataset(a.n, a.entries, torch), "skewed", HipBackend(), torch)


def step_heavy(a):
    import torch
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    for tag, heavy in (("balanced", False), ("heavy_row", True)):
        pos = dataset(a.n, a.entries, torch, heavy, skew=1)
        say(step="matrix", matrix=tag, nnz=int(pos[0].numel()), row0=int((pos[0] == 0).sum()))
        epochs_of(a, pos, tag, be, torch)


def step_torch(a):
    import torch
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    pos = dataset(a.n, a.entries, torch)
    rows, cols, fx, lx = pos
    nnz = int(rows.numel())
    for batch in a.batches:
        n_steps = -(-nnz // batch)
        slots = torch.arange(0, nnz, n_steps, device="cuda")
        r, c, f, l = rows[slots].long(), cols[slots].long(), fx[slots], lx[slots]
        index = be.glove_index(rows, cols, a.n, n_steps)
        for rank in a.ranks:
            st = parameters(be, a.n, rank, torch)
            Wi, Wj, bi, bj = (t.clone() for t in st[:4])

            def torch_step():
                wi, wj = Wi[r], Wj[c]
                inner = ((wi * wj).sum(1) + bi[r] + bj[c] - l).clamp(-100.0, 100.0)
                cost = f * inner
                Wi.index_add_(0, r, -0.05 * cost[:, None] * wj)
                Wj.index_add_(0, c, -0.05 * cost[:, None] * wi)
                bi.index_add_(0, r, -0.05 * cost)
                bj.index_add_(0, c, -0.05 * cost)

            ours = lambda: be.glove_step(*pos, index, 0, *st, 0.05, 0.0)
            torch_step(), ours()
            pairs = [(event_ms(torch_step, torch), event_ms(ours, torch)) for _ in range(a.reps)]
            t_torch, t_ours = (statistics.median(p[i] for p in pairs) for i in (0, 1))
            say(step="torch", what="one step: gathers + index_add_ (atomics, not reproducible, plain SGD) against rsparse_hip_glove_step_device "
                "(scratch allocation included, Adagrad), alternating", rank=rank, batch=batch, slots=int(slots.numel()),
                torch_ms=round(t_torch, 3), ours_ms=round(t_ours, 3), torch_over_ours=round(t_torch / t_ours, 2))
            del st, Wi, Wj, bi, bj
        del index


def step_movielens(a):
    import numpy as np
    import scipy.sparse as sp
    from rsparse_amd import GloVe
    d = np.load(ROOT / "tests" / "golden" / "movielens100k_csc.npz")
    x = sp.csc_matrix((d["x"].astype(np.float64), d["i"], d["p"]), shape=tuple(int(v) for v in d["Dim"]))
    co = (x.T @ x).tocsr()
    for batch in (1 << 10, 1 << 14, 1 << 18):
        m = GloVe(rank=8, x_max=X_MAX, learning_rate=0.15, batch=batch, rng=1)
        m.fit_transform(co, n_iter=10)
        say(step="movielens", n=co.shape[0], nnz=int(co.nnz), rank=8, batch=batch, cost_history=[round(c, 6) for c in m.cost_history])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True, choices=("epoch", "torch", "heavy", "movielens"))
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--entries", type=lambda s: int(float(s)), default=130_000_000)   # (drawn; about 1e8 stay after the duplicates merge)
    ap.add_argument("--ranks", type=lambda s: [int(v) for v in s.split(",")], default=[64, 128])
    ap.add_argument("--batches", type=lambda s: [int(v) for v in s.split(",")], default=[1 << 16, 1 << 18, 1 << 20])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(OUT))
    a = ap.parse_args()
    OUT = Path(a.out)
    {"epoch": step_epoch, "torch": step_torch, "heavy": step_heavy, "movielens": step_movielens}[a.step](a)
