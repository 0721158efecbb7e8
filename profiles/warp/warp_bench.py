"""WARP (warp_search_kernel of wrmf_bpr.hip) on one GPU at the shape of profiles/bpr/: 1 000 000 users x 100 000 items, 5e7 entries
with Zipf item popularity, fp32, batch 2^20, max_trials 50, margin 0.1.  One JSON line per measurement, appended to --out (default
warp_bench.jsonl here); medians of --reps runs, each from a fresh copy of the same state, behind a warm-up, timed by two events.

    python profiles/warp/warp_bench.py --step epoch     per rank: a BPR epoch and a WARP epoch at the initial factors (searches of
                                                        about one trial), then ten WARP epochs, then the eleventh timed (long searches)
    python profiles/warp/warp_bench.py --step search    the search launch alone (rsparse_hip_warp_triples_device) on one step's
                                                        slots at both states, per scored candidate; BPR's sampler alone beside it
"""
import argparse
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "bpr"))
import bpr_bench  # noqa: E402  (sets sys.path for the package; `say` appends to bpr_bench.OUT)
from bpr_bench import dataset, factors, say, timed  # noqa: E402

T, MARGIN, LR, LAM, SEED = 50, 0.1, 0.05, 0.01, 11


def fresh(state, torch):
    return [t.clone() for t in state]


def trained(be, a, p, j, nnz, rank, w, torch):
    """-> (the initial state, the state after ten WARP epochs, their counts)"""
    init = list(factors(be, a, rank, torch))
    state = fresh(init, torch)
    counts = be.warp_epochs(p, j, a.items, nnz, 0, SEED, 0, 0, 10, a.batch, T, MARGIN, w, *state, LR, LAM)
    return init, state, counts.tolist()


def step_epoch(a):
    import torch
    from rsparse_amd.engine import HipBackend
    from rsparse_amd.warp import rank_weights
    be = HipBackend()
    nnz, p, j = dataset(a, torch)
    w = rank_weights(a.items, T)
    for rank in a.ranks:
        init, late, ten = trained(be, a, p, j, nnz, rank, w, torch)
        base = dict(rank=rank, batch=a.batch, nnz=nnz, steps=-(-nnz // a.batch), max_trials=T)
        res = []
        t = timed(lambda: res.append(be.bpr_epochs(p, j, a.items, nnz, 0, SEED, 0, 0, 1, a.batch, *fresh(init, torch), LR, LAM)), a.reps, torch)
        say(step="epoch", what="BPR epoch at the initial factors (the same kernels as before WARP)", n_valid=int(res[-1][0][0]), **t, **base)
        for name, state, epoch in (("WARP epoch at the initial factors", init, 0), ("WARP epoch after ten epochs", late, 10)):
            res = []
            t = timed(lambda: res.append(be.warp_epochs(p, j, a.items, nnz, 0, SEED, 0, epoch, 1, a.batch, T, MARGIN, w, *fresh(state, torch),
                                                        LR, LAM)), a.reps, torch)
            nv, nl, nc, ns = (int(v) for v in res[-1][0].tolist())
            say(step="epoch", what=name, n_valid=nv, n_looked=nl, auc=round(nc / nl, 4), n_scored=ns, scored_per_slot=round(ns / nnz, 3), **t,
                **base)
        say(step="epoch", what="the ten epochs between", rank=rank, scored_per_slot=[round(c[3] / nnz, 3) for c in ten],
            valid_share=[round(c[0] / nnz, 3) for c in ten])


def step_search(a):
    import torch
    from rsparse_amd.engine import HipBackend
    from rsparse_amd.warp import rank_weights
    be = HipBackend()
    nnz, p, j = dataset(a, torch)
    w, n_steps = rank_weights(a.items, T), -(-nnz // a.batch)
    for rank in a.ranks:
        init, late, _ = trained(be, a, p, j, nnz, rank, w, torch)
        t = timed(lambda: be.bpr_triples(p, j, a.items, nnz, 0, SEED, 0, 0, 0, n_steps), a.reps, torch)
        say(step="search", what="bpr_sample_kernel alone, one step", rank=rank, slots=-(-nnz // n_steps), **t)
        for name, state, epoch in (("initial factors", init, 0), ("after ten epochs", late, 10)):
            # the counts of exactly this step: one step through the whole pipeline on a copy
            ns = int(be.warp_step(p, j, a.items, nnz, 0, SEED, 0, epoch, 0, n_steps, T, MARGIN, w, *fresh(state, torch), LR, LAM)[3])
            t = timed(lambda: be.warp_triples(p, j, a.items, nnz, 0, SEED, 0, epoch, 0, n_steps, T, MARGIN, w, state[0], state[1]), a.reps, torch)
            say(step="search", what="warp_search_kernel alone, one step, " + name, rank=rank, slots=-(-nnz // n_steps), n_scored=ns,
                ns_per_scored=round(t["ms"] * 1e6 / ns, 3), ns_per_slot=round(t["ms"] * 1e6 / -(-nnz // n_steps), 3), **t)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True, choices=("epoch", "search"))
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--nnz", type=float, default=5e7)
    ap.add_argument("--ranks", type=lambda s: [int(v) for v in s.split(",")], default=[128, 64])
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(HERE / "warp_bench.jsonl"))
    a = ap.parse_args()
    bpr_bench.OUT = Path(a.out)
    {"epoch": step_epoch, "search": step_search}[a.step](a)
