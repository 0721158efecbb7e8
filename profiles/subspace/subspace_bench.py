"""IALSpp (wrmf_subspace.hip) on one GPU.  One JSON line per measurement, appended to --out (default subspace_bench.jsonl here);
medians of --reps runs behind a warm-up, each timed by two events around the call with the device idle before it.

    python profiles/subspace/subspace_bench.py --step half      1 000 000 x 100 000, 5e7 entries (rsparse_amd.synth): per side, rank
                                                                and b the block launches, torch.matmul, score_pairs and the Gramian
    python profiles/subspace/subspace_bench.py --step long      one row holding a tenth of 2e7 entries against the same matrix without it
    python profiles/subspace/subspace_bench.py --step quality   2000 x 1000: the objective after 1 .. 10 iterations, IALSpp against
                                                                WRMF(solver="cholesky") from the same initial factors
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))
OUT = HERE / "subspace_bench.jsonl"


def say(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def timed(fn, reps, torch):
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
    return round(statistics.median(out), 3)


def half_parts(be, csr, W, H, b, reps, torch):
    """the parts of one half, each timed alone -> dict of ms (block / matmul: summed over the blocks)"""
    p, j, x = csr
    k = W.shape[1]
    G = torch.empty((k, k), dtype=torch.float32, device=W.device)
    t = {"gramian": timed(lambda: be.gramian(H, 0.0, G, None), reps, torch),
         "score_pairs": timed(lambda: be.score_pairs(W, H, p, j)[0].to(torch.float32), reps, torch), "matmul": 0.0, "blocks": 0.0}
    e = be.score_pairs(W, H, p, j)[0].to(torch.float32)
    per_block = []
    for c0 in range(0, k, b):
        w = min(b, k - c0)
        t["matmul"] += timed(lambda: torch.matmul(W, G[:, c0:c0 + w]), reps, torch)
        D = torch.matmul(W, G[:, c0:c0 + w])
        W0, e0 = W.clone(), e.clone()

        def block():   # (from the same state every time: the copies are outside the events' cost only by ~2 n k + nnz floats)
            be.subspace_block(p, j, x, H, c0, w, b, G[c0:c0 + w, c0:c0 + w], D, 0.1, W, e)
        copies = timed(lambda: (W.copy_(W0), e.copy_(e0)), reps, torch)
        per_block.append(round(timed(lambda: (W.copy_(W0), e.copy_(e0), block()), reps, torch) - copies, 3))
        block()
    t["blocks"] = round(sum(per_block), 3)
    t["per_block"] = per_block
    t["half"] = round(t["gramian"] + t["score_pairs"] + t["matmul"] + t["blocks"], 3)
    return t


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("half", "long", "quality"), default="half")
    ap.add_argument("--ranks", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--blocks", type=int, nargs="+", default=[64, 32])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(OUT))
    a = ap.parse_args()
    OUT = Path(a.out)
    import numpy as np
    import torch
    from rsparse_amd import synth
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    gen = torch.Generator(device="cuda").manual_seed(1)
    factors = lambda n, k: 0.05 * torch.randn((n, k), device="cuda", generator=gen)
    if a.step == "half":
        d = synth.make_dataset(1_000_000, 100_000, device="cuda")
        nnz = int(d["nnz"])
        for k in a.ranks:
            U, V = factors(d["n_users"], k), factors(d["n_items"], k)
            for b in a.blocks:
                tu = half_parts(be, d["c_iu"], U, V, b, a.reps, torch)
                ti = half_parts(be, d["c_ui"], V, U, b, a.reps, torch)
                gb = lambda t: round(nnz * 4.0 * k / (t["blocks"] * 1e-3) / 1e9, 1)   # floats of H gathered once per block
                say(step="half", rank=k, b=b, nnz=nnz, user_half=tu, item_half=ti, iteration_ms=round(tu["half"] + ti["half"], 3),
                    gathered_GBps_user=gb(tu), gathered_GBps_item=gb(ti))
    elif a.step == "long":
        n, m, k, b = 200_000, 2_200_000, 128, 64
        H = factors(m, k)
        for long_len in (90, 2_000_000):
            lens = torch.full((n,), 90, dtype=torch.int64, device="cuda")
            lens[n // 2] = long_len
            p = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            p[1:] = torch.cumsum(lens, 0)
            nnz = int(p[-1])
            # ascending distinct columns per row: a random start and a stride of 1
            start = (torch.rand(n, device="cuda", generator=gen) * (m - long_len - 1)).long()
            rows = torch.repeat_interleave(torch.arange(n, device="cuda"), lens)
            j = (start[rows] + torch.arange(nnz, device="cuda") - p[:-1][rows]).to(torch.int32)
            x = 1.0 + 39.0 * torch.rand(nnz, device="cuda", generator=gen)
            W = factors(n, k)
            t = half_parts(be, (p.to(torch.int32), j, x), W, H, b, a.reps, torch)
            say(step="long", longest_row=long_len, nnz=nnz, rank=k, b=b, per_block=t["per_block"], blocks=t["blocks"])
    else:
        import scipy.sparse as sp
        from rsparse_amd import IALSpp, WRMF
        from rsparse_amd.ialspp import ialspp_objective
        rng = np.random.default_rng(0)
        x = sp.csr_matrix((rng.random((2000, 1000)) < 0.02) * rng.uniform(1.0, 40.0, (2000, 1000)))
        k = 128
        U0, V0 = ((0.01 * rng.standard_normal((s, k))).astype(np.float32) for s in x.shape)
        for it in range(1, 11):
            row = {"step": "quality", "iterations": it}
            for name, make in (("ialspp_b64", lambda: IALSpp(rank=k, lambda_=0.1, block=64)), ("ialspp_b32", lambda: IALSpp(rank=k, lambda_=0.1, block=32)),
                               ("wrmf_cholesky", lambda: WRMF(rank=k, lambda_=0.1, dynamic_lambda=False, solver="cholesky", precision="float",
                                                               factor_init="device"))):
                mdl = make()
                mdl._init_user_factors, mdl.components = U0, V0.T.copy()
                kw = {"convergence_tol": -np.inf} if name == "wrmf_cholesky" else {}
                U = mdl.fit_transform(x, it, **kw)
                row[name] = ialspp_objective(x, U, mdl.components.T, 0.1)
            say(**row)


if __name__ == "__main__":
    main()
