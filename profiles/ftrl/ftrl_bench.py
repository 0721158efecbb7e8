"""FTRL on the device: what profiles/ftrl/README.md reports.  Needs a GPU; every time is a host clock around work that ends in a
device synchronise, after one warm-up of the same call.  One JSON line per measurement on stdout and in --out.

    python profiles/ftrl/ftrl_bench.py [--scale 1.0] [--out FILE]      (default: ftrl_bench.jsonl beside this script)

--scale multiplies every row count (1.0: 5e7 samples x 1.1M features, 2.5e8 entries -- the factorization machine's shape)."""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from rsparse_amd import _lib  # noqa: E402
from rsparse_amd.engine import HipBackend  # noqa: E402

GLM = ("binomial", 0.1, 0.5, 1e-6, 0.5)


def design(n, d, per_row, dtype, gen, every=False):
    """n x d CSR on the device, per_row entries per row at random columns (sorted), values 1; every: column 0 in every row too"""
    cols = torch.randint(1 if every else 0, d, (n, per_row), device="cuda", generator=gen, dtype=torch.int32)
    if every:
        cols = torch.cat([torch.zeros((n, 1), dtype=torch.int32, device="cuda"), cols], dim=1)
    cols = cols.sort(dim=1).values.reshape(-1).contiguous()
    width = per_row + int(every)
    p = torch.arange(0, (n + 1) * width, width, dtype=torch.int32, device="cuda")
    return p, cols, torch.ones(cols.numel(), dtype=dtype, device="cuda")


def timed(f, repeat=2):
    f()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeat):
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent / "ftrl_bench.jsonl"))
    a = ap.parse_args()
    be = HipBackend()
    gen = torch.Generator(device="cuda").manual_seed(1)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    sink = open(a.out, "w")

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    n, d = int(5e7 * a.scale), 1_100_000
    y = (torch.rand(n, device="cuda", generator=gen) < 0.3).to(torch.float64)
    om = torch.ones(n, dtype=torch.float64, device="cuda")
    for dtype in (torch.float32, torch.float64):
        csr = design(n, d, 5, dtype, gen)
        nnz, pair = csr[1].numel(), 2 * csr[2].element_size()
        for batch in (1 << 20, 1 << 18):
            n_steps = -(-n // batch)
            t0 = time.perf_counter()
            index = be.fm_index(csr[0], csr[1], d, n_steps)
            torch.cuda.synchronize()
            t_index = time.perf_counter() - t0
            for dropout in (0.0, 0.3):
                zn = torch.zeros((d, 2), dtype=dtype, device="cuda")
                t_epoch = timed(lambda: be.ftrl_epochs(*csr, index, 1, *GLM, dropout, 7, 0, y, om, zn))
                name = "rsparse_hip_ftrl_forward%s_device" % ("_f64" if dtype == torch.float64 else "")
                prob, dk = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(batch, dtype=torch.float64, device="cuda")

                def forwards():   # every step's forward launch alone, into buffers allocated once
                    for s in range(n_steps):
                        _lib.check(getattr(be.lib, name)(csr[0].data_ptr(), csr[1].data_ptr(), csr[2].data_ptr(), n, d, nnz, s, n_steps, 0,
                                                         *GLM[1:], dropout, 7, 0, zn.data_ptr(), y.data_ptr(), om.data_ptr(),
                                                         prob.data_ptr(), dk.data_ptr(), be._stream()))

                t_fwd = timed(forwards)
                emit(what="epoch", dtype=str(dtype), n=n, d=d, nnz=nnz, batch=batch, dropout=dropout, epoch_s=t_epoch, forward_s=t_fwd,
                     update_s=t_epoch - t_fwd, index_s=t_index, zn_gather_GBps=nnz * pair / t_fwd / 1e9)
            if dtype == torch.float32 and batch == 1 << 20:
                zn = torch.zeros((d, 2), dtype=dtype, device="cuda")
                t_step = timed(lambda: be.ftrl_step(*csr, index, 0, *GLM, 0.0, 7, 0, y, om, zn))
                rows = torch.arange(0, n, n_steps, device="cuda")
                at = torch.stack([torch.arange(rows.numel(), device="cuda").repeat_interleave(5), csr[1].view(n, 5)[rows].reshape(-1).long()])
                xs = torch.sparse_coo_tensor(at, torch.ones(at.shape[1], dtype=dtype, device="cuda"), size=(rows.numel(), d)).coalesce()
                w, ys = torch.zeros((d, 1), dtype=dtype, device="cuda"), y[rows].to(dtype)

                def torch_step():   # the same step in eager torch: w from (z, n), X w, the link, X^T d and X^T d^2 by index_add_
                    z_, n_ = zn[:, 0], zn[:, 1]
                    w[:, 0] = torch.where(z_.abs() <= 5e-7, 0.0, -(z_ - z_.sign() * 5e-7) / ((0.5 + n_.sqrt()) / 0.1 + 5e-7))
                    dd = torch.sigmoid(torch.sparse.mm(xs, w)[:, 0]) - ys
                    g = (dd[xs.indices()[0]] * xs.values()).clamp(-1000.0, 1000.0)
                    G = torch.zeros(d, dtype=dtype, device="cuda").index_add_(0, xs.indices()[1], g)
                    Q = torch.zeros(d, dtype=dtype, device="cuda").index_add_(0, xs.indices()[1], g * g)
                    nn = n_ + Q
                    zn[:, 0] = torch.where(Q > 0, z_ + G - (nn.sqrt() - n_.sqrt()) / 0.1 * w[:, 0], z_)
                    zn[:, 1] = nn

                emit(what="one step against torch", dtype=str(dtype), batch=batch, ftrl_step_s=t_step, torch_step_s=timed(torch_step))
                del xs
                st = [torch.zeros(s, dtype=t, device="cuda") for s, t in ((1, dtype), (d, dtype), ((d, 1), dtype), (1, torch.float64),
                                                                        (d, torch.float64), ((d, 1), torch.float64))]
                t_fm = timed(lambda: be.fm_epochs(*csr, index, 1, "binomial", True, 2.0 * y - 1.0, om, *st, 0.2, 0.2, 0.0, 0.0))
                emit(what="FactorizationMachine(rank=1) epoch, same matrix and index", dtype=str(dtype), batch=batch, fm_epoch_s=t_fm)
            del index
        del csr
    # the group-width rule: forward time per stored entry on either side of its edges (mean row length 8 | 9 and 32 | 33)
    for per_row in (3, 8, 9, 32, 33, 40):
        rows_n = int(1e8 * a.scale) // per_row
        csr = design(rows_n, d, per_row, torch.float32, gen)
        zn = torch.rand((d, 2), dtype=torch.float32, device="cuda", generator=gen)
        t = timed(lambda: be.ftrl_predict(*csr, *GLM, zn))
        emit(what="forward by row length", per_row=per_row, width=4 if per_row <= 8 else (16 if per_row <= 32 else 64), n=rows_n,
             forward_s=t, ns_per_entry=t / csr[1].numel() * 1e9)
        del csr
    # skew: a column held by every row against none
    n2, batch = int(2e7 * a.scale), 1 << 20
    for every in (False, True):
        csr = design(n2, d, 5, torch.float32, gen, every)
        index = be.fm_index(csr[0], csr[1], d, -(-n2 // batch))
        zn = torch.zeros((d, 2), dtype=torch.float32, device="cuda")
        emit(what="skew", column_in_every_row=every, n=n2, nnz=csr[1].numel(), batch=batch,
             epoch_s=timed(lambda: be.ftrl_epochs(*csr, index, 1, *GLM, 0.0, 7, 0, y[:n2], om[:n2], zn)))
        del csr, index


if __name__ == "__main__":
    main()
