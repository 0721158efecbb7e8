"""FactorizationMachine (wrmf_fm.hip) on one GPU at a recommender-like shape: one sample per interaction of the 1 000 000 x 100 000
shape of profiles/bpr/ (5e7 samples), each a row of one-hot user + one-hot item (cubic-skewed popularity) + three skewed tags out of
1000, so d = 1 101 000 and every row holds 5 entries.  One JSON line per measurement, appended to --out (default fm_bench.jsonl
here); medians of --reps runs behind a warm-up, each timed by two events around the call with the device idle before it.

    python profiles/fm/fm_bench.py --step epoch    the index build, one epoch and one step at --ranks x --batches, fp32, binomial; the
                                                   forward launch alone; the bytes of the rows of V and S gathered per second
    python profiles/fm/fm_bench.py --step torch    the same step written with torch.sparse.mm + index_add_ (atomics, plain SGD)
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
OUT = HERE / "fm_bench.jsonl"
TAGS = 1000


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


def dataset(a, torch):
    """the canonical CSR of the samples on the device -> (p, j, x, y, omega, d): five ascending columns per row"""
    g = torch.Generator(device="cuda").manual_seed(1)
    n = a.samples
    r = lambda: torch.rand(n, device="cuda", generator=g)
    cols = [(r() * a.users).long(), a.users + (r() ** 3 * a.items).long()]
    third = TAGS // 3
    cols += [a.users + a.items + t * third + (r() ** 4 * third).long() for t in range(3)]
    j = torch.stack(cols, dim=1).reshape(-1).to(torch.int32).contiguous()
    p = (torch.arange(n + 1, device="cuda", dtype=torch.int64) * 5).to(torch.int32)
    x = torch.ones(5 * n, dtype=torch.float32, device="cuda")
    y = torch.where(r() < 0.5, -1.0, 1.0).to(torch.float64)
    return p, j, x, y, torch.ones(n, dtype=torch.float64, device="cuda"), a.users + a.items + TAGS


def parameters(be, d, rank, torch):
    V = be.init_factors(7, 1, d, rank, torch.float32)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=be.device)
    return z(1, torch.float32), z(d, torch.float32), V, z(1, torch.float64), z(d, torch.float64), z((d, rank), torch.float64)


def step_epoch(a):
    import torch
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    p, j, x, y, om, d = dataset(a, torch)
    n, nnz = a.samples, int(j.numel())
    for batch in a.batches:
        n_steps = -(-n // batch)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        index = be.fm_index(p, j, d, n_steps)                                # (once: its first call, scratch allocation included)
        e1.record()
        e1.synchronize()
        say(step="index", batch=batch, steps=n_steps, nnz=nnz, index_gb=round(index[0].numel() / 1e9, 2), ms=round(e0.elapsed_time(e1), 3))
        for rank in a.ranks:
            st = parameters(be, d, rank, torch)
            ld = 16 * (-(-rank // 16))
            run = lambda: be.fm_epochs(p, j, x, index, 1, "binomial", True, y, om, *st, 0.2, 0.2, 0.0, 0.0)
            t = timed(run, a.reps, torch)
            # the forward gathers a row of V (fp32) per stored entry, the backward a row of S (float64) per stored entry
            gathered = nnz * (rank * 4 + ld * 8)
            say(step="epoch", rank=rank, batch=batch, steps=n_steps, samples=n, nnz=nnz, d=d, gathered_gb=round(gathered / 1e9, 1),
                gathered_tb_per_s=round(gathered / 1e12 / (t["ms"] / 1e3), 3), **t)
            one = timed(lambda: be.fm_step(p, j, x, index, 0, "binomial", True, y, om, *st, 0.2, 0.2, 0.0, 0.0), a.reps, torch)
            fwd = timed(lambda: be.fm_forward(p, j, x, "binomial", 0, n_steps, *st[:3], y, om), a.reps, torch)
            rows = -(-n // n_steps)
            say(step="launches", what="step 0: the whole step (scratch allocation included), and its forward launch alone (outputs allocated)",
                rank=rank, batch=batch, rows=rows, step_ms=one["ms"], forward_ms=fwd["ms"],
                forward_v_tb_per_s=round(rows * 5 * rank * 4 / 1e12 / (fwd["ms"] / 1e3), 3))
            del st
        del index


def step_torch(a):
    """one step of `batch` rows with torch: two sparse products forward, index_add_ backward (float atomics, plain SGD)"""
    import torch
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    p, j, x, y, om, d = dataset(a, torch)
    n = a.samples
    for batch in a.batches:
        n_steps = -(-n // batch)
        rows = torch.arange(0, n, n_steps, device="cuda")
        cols = j.view(n, 5)[rows].long()
        B = int(rows.numel())
        Xb = torch.sparse_csr_tensor(torch.arange(B + 1, device="cuda") * 5, cols.reshape(-1), torch.ones(5 * B, device="cuda"), size=(B, d))
        yb, flat = y[rows].float(), cols.reshape(-1)
        index = be.fm_index(p, j, d, n_steps)
        for rank in a.ranks:
            w0, w, V, a0, aw, aV = parameters(be, d, rank, torch)

            def torch_step():
                S = torch.sparse.mm(Xb, V)
                Q = torch.sparse.mm(Xb, V * V)                                # (x is 0 / 1 here: x^2 = x)
                raw = w0 + torch.sparse.mm(Xb, w[:, None])[:, 0] + 0.5 * (S * S - Q).sum(1)
                delta = -yb * torch.sigmoid(-yb * raw)
                dk = delta.repeat_interleave(5)
                V.index_add_(0, flat, -0.2 * dk[:, None] * (S.repeat_interleave(5, dim=0) - V[flat]))
                w.index_add_(0, flat, -0.2 * dk)
                w0.sub_(0.2 * delta.sum())

            ours = lambda: be.fm_step(p, j, x, index, 0, "binomial", True, y, om, w0, w, V, a0, aw, aV, 0.2, 0.2, 0.0, 0.0)
            t_torch, t_ours = timed(torch_step, a.reps, torch), timed(ours, a.reps, torch)
            say(step="torch", what="one step: torch.sparse.mm + index_add_ (atomics, not reproducible, plain SGD) against "
                "rsparse_hip_fm_step_device (scratch allocation included, Adagrad)", rank=rank, batch=batch, rows=B, torch_ms=t_torch["ms"],
                ours_ms=t_ours["ms"], torch_over_ours=round(t_torch["ms"] / t_ours["ms"], 2))
            del w0, w, V, a0, aw, aV
        del index


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True, choices=("epoch", "torch"))
    ap.add_argument("--samples", type=lambda s: int(float(s)), default=50_000_000)
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--ranks", type=lambda s: [int(v) for v in s.split(",")], default=[64, 128])
    ap.add_argument("--batches", type=lambda s: [int(v) for v in s.split(",")], default=[1 << 18, 1 << 20])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(OUT))
    a = ap.parse_args()
    OUT = Path(a.out)
    {"epoch": step_epoch, "torch": step_torch}[a.step](a)
