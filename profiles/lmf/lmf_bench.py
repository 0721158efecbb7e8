"""Logistic MF (wrmf_lmf.hip) on one GPU at the shape of profiles/bpr/: 1 000 000 users x 100 000 items, 5e7 entries with Zipf item
popularity (rsparse_amd.synth).  One JSON line per measurement, appended to --out (default lmf_bench.jsonl here); medians of
--reps runs behind a warm-up, each timed by two events around the call with the device idle before it.

    python profiles/lmf/lmf_bench.py --step dense   the dense launch at users x items and items x users, K = 128 and 64, as TFLOP/s of
                                                    4 n_rows n_str K; beside it top_product's scoring rate (2 n_rows n_str K) on the
                                                    same shape and a chunked torch.sigmoid(A @ B.T) @ B on --torch-rows rows
    python profiles/lmf/lmf_bench.py --step step    the step launch against score_pairs on the same pattern
    python profiles/lmf/lmf_bench.py --step fit     one full iteration and a 10-iteration fit at K = --k
    python profiles/lmf/lmf_bench.py --step ml100k  NDCG@10 on the MovieLens-100k fixture of the tests (900 training users)
"""
import argparse
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "profiles" / "bpr"))
OUT = HERE / "lmf_bench.jsonl"


def say(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def factors(n, K, torch, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return 0.1 * torch.randn((n, K), device="cuda", dtype=torch.float32, generator=g)


def dense(a, be, torch, timed):
    for n_rows, n_str in ((a.users, a.items), (a.items, a.users)):
        for K in (128, 64):
            A, B = factors(n_rows, K, torch, 1), factors(n_str, K, torch, 2)
            t = timed(lambda: be.lmf_dense(A, B), a.reps, torch)
            say(step="dense", what="lmf_dense_kernel", n_rows=n_rows, n_str=n_str, K=K, slices=be.lmf_slices(n_rows, n_str)[0],
                tflops=round(4.0 * n_rows * n_str * K / t["ms"] / 1e9, 2), **t)
            t = timed(lambda: be.top_product(A, B, 10, None, None, None, 0.0), a.reps, torch)
            say(step="dense", what="top_product, k = 10", n_rows=n_rows, n_str=n_str, K=K,
                tflops=round(2.0 * n_rows * n_str * K / t["ms"] / 1e9, 2), **t)
            rows = min(n_rows, a.torch_rows)

            def chunked():
                for r0 in range(0, rows, 8192):
                    torch.sigmoid(A[r0:r0 + 8192] @ B.T) @ B
            t = timed(chunked, a.reps, torch)
            say(step="dense", what="torch.sigmoid(A @ B.T) @ B in chunks of 8192 rows", n_rows=rows, n_str=n_str, K=K,
                tflops=round(4.0 * rows * n_str * K / t["ms"] / 1e9, 2), **t)


def csr(a, torch):
    from bpr_bench import dataset
    nnz, p, j = dataset(a, torch)
    return nnz, p, j, torch.ones(nnz, dtype=torch.float32, device="cuda")


def step(a, be, torch, timed):
    nnz, p, j, x = csr(a, torch)
    for K in (128, 64):
        A, B = factors(a.users, K, torch, 1), factors(a.items, K, torch, 2)
        aA, D = torch.zeros(A.shape, dtype=torch.float64, device="cuda"), torch.zeros((1,) + tuple(A.shape), device="cuda")
        t = timed(lambda: be.lmf_step(p, j, x, 1.0, A, aA, B, D, K - 2, K - 1, 0.0, 0.6), a.reps, torch)   # (lr = 0: A stays)
        say(step="step", what="lmf_step_kernel", K=K, nnz=nnz, entries_per_us=round(nnz / t["ms"] / 1e3, 1), **t)
        t = timed(lambda: be.score_pairs(A, B, p, j), a.reps, torch)
        say(step="step", what="score_pairs", K=K, nnz=nnz, entries_per_us=round(nnz / t["ms"] / 1e3, 1), **t)


def fit(a, be, torch, timed):
    nnz, p, j, x = csr(a, torch)
    ip = be.transpose_csc(a.items, a.users, p, j, x)
    K = a.k
    U, V = factors(a.users, K, torch, 1), factors(a.items, K, torch, 2)
    U[:, K - 1] = V[:, K - 2] = 1.0
    aU, aV = (torch.zeros(F.shape, dtype=torch.float64, device="cuda") for F in (U, V))

    def iterations(n):
        for _ in range(n):
            be.lmf_half(p, j, x, 1.0, U, aU, V, K - 2, K - 1, 1.0, 0.6)
            be.lmf_half(*ip, 1.0, V, aV, U, K - 2, K - 2, 1.0, 0.6)
    say(step="fit", what="one iteration (user half, item half)", K=K, nnz=nnz, **timed(lambda: iterations(1), a.reps, torch))
    say(step="fit", what="ten iterations", K=K, nnz=nnz, **timed(lambda: iterations(10), 1, torch))


def ml100k(a):
    import numpy as np
    sys.path.insert(0, str(ROOT / "tests"))
    from test_ease_host import brute_lists, ndcg10, protocol
    from rsparse_amd import LogisticMF
    train, hist, held = protocol()
    pop = np.broadcast_to(np.bincount(train.indices, minlength=train.shape[1]).astype(np.float64), hist.shape)
    say(step="ml100k", what="popularity", ndcg10=round(ndcg10(brute_lists(pop, 10, hist, ())[0], held), 4))
    for rank, alpha, lam, n_iter in ((30, 1.0, 0.6, 30), (16, 5.0, 0.6, 30), (16, 5.0, 2.0, 60)):
        m = LogisticMF(rank=rank, alpha=alpha, lambda_=lam, rng=5)
        m.fit_transform(train, n_iter)
        say(step="ml100k", what="LogisticMF", rank=rank, alpha=alpha, lambda_=lam, n_iter=n_iter,
            ndcg10=round(ndcg10(np.asarray(m.predict(hist, 10)), held), 4))


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True, choices=("dense", "step", "fit", "ml100k"))
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--nnz", type=int, default=50_000_000)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--torch-rows", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(OUT))
    a = ap.parse_args()
    OUT = Path(a.out)
    if a.step == "ml100k":
        return ml100k(a)
    import torch
    from bpr_bench import timed
    from rsparse_amd.engine import HipBackend
    {"dense": dense, "step": step, "fit": fit}[a.step](a, HipBackend(), torch, timed)


if __name__ == "__main__":
    main()
