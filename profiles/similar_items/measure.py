"""Throughput of the item-to-item similarity path on one MI355X (profiles/similar_items/README.md quotes the results).

    python profiles/similar_items/measure.py normalize            # (a) the normalisation launch, 1 M items
    python profiles/similar_items/measure.py similar              # (b) similar_items, 262144 queries against 1 M x 128
    python profiles/similar_items/measure.py top_product          # (b) the same shape through HipBackend.top_product

`top_product` uses nothing that this feature added, so it also runs against a library built from the parent commit
(RSPARSE_HIP_LIB=/path/to/that/librsparse_wrmf_hip.so).  Timing: HIP events on the stream around each call, after warm-up calls of
the same shape; every repetition is printed, and the median, minimum and maximum.  One JSON line per measurement."""
import json
import sys

import numpy as np
import torch

from rsparse_amd import _lib
from rsparse_amd.engine import HipBackend

N_ITEMS, RANK, N_Q = 1_000_000, 128, 262_144


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def report(name, ms, **extra):
    out = dict(name=name, lib=str(_lib.LIB_PATH), ms=[round(v, 4) for v in ms], median_ms=float(np.median(ms)), min_ms=min(ms),
               max_ms=max(ms), **extra)
    print(json.dumps(out), flush=True)
    return out


def factors(dtype, ld=RANK):
    g = torch.Generator(device="cuda").manual_seed(1)
    return torch.randn((N_ITEMS, ld), generator=g, device="cuda", dtype=dtype)


def normalize(be):
    for dtype, ld, c0, c1 in ((torch.float32, RANK, 0, RANK), (torch.float64, RANK, 0, RANK), (torch.float32, RANK + 2, 1, RANK + 1)):
        V = factors(dtype, ld)
        r = c1 - c0
        Vn32 = torch.empty((N_ITEMS, r), dtype=torch.float32, device="cuda")
        Vn64 = torch.empty((N_ITEMS, r), dtype=torch.float64, device="cuda")
        flags = torch.empty(N_ITEMS, dtype=torch.int32, device="cuda")
        fn = be.lib.rsparse_hip_normalize_items_f64_device if dtype == torch.float64 else be.lib.rsparse_hip_normalize_items_device
        ms = timed(lambda: _lib.check(fn(V.data_ptr(), N_ITEMS, ld, c0, c1, Vn32.data_ptr(), Vn64.data_ptr(), flags.data_ptr(),
                                         be._stream())), 5, 30)
        nbytes = N_ITEMS * (r * (V.element_size() + 12) + 4)
        med = float(np.median(ms))
        report("normalize_items %s ld=%d [%d,%d)" % (str(dtype).split(".")[1], ld, c0, c1), ms, bytes=nbytes,
               TB_per_s=nbytes / med / 1e9, fraction_of_8TBps=nbytes / med / 1e9 / 8.0)
        # a plain device copy of the same byte count on the same box, for scale
        src = torch.empty(nbytes // 2 // 4, dtype=torch.float32, device="cuda")
        dst = torch.empty_like(src)
        cms = timed(lambda: dst.copy_(src), 5, 30)
        report("device copy of the same bytes", cms, bytes=nbytes, TB_per_s=nbytes / float(np.median(cms)) / 1e9)
        del V, Vn32, Vn64, flags, src, dst


def queries():
    g = torch.Generator(device="cuda").manual_seed(2)
    return torch.randperm(N_ITEMS, generator=g, device="cuda")[:N_Q].to(torch.int32)


def similar(be):
    V = factors(torch.float32)
    q = queries()
    be.normalized_items(V, 0, RANK)
    for k in (10, 100):
        ms = timed(lambda: be.similar_items(V, 0, RANK, q, k), 1, 4)
        report("similar_items k=%d" % k, ms, queries_per_s=N_Q / float(np.median(ms)) * 1e3,
               TFLOP_per_s=2.0 * N_Q * N_ITEMS * RANK / float(np.median(ms)) / 1e9)


def top_product(be):
    V = factors(torch.float32)
    V = V / V.norm(dim=1, keepdim=True)
    q = queries().to(torch.int64)
    for dtype in (torch.float64, torch.float32):
        Vd = V.to(dtype)
        U = Vd[q].contiguous()
        for k in (10, 100):
            ms = timed(lambda: be.top_product(U, Vd, k, None, None, None, 0.0), 1, 4)
            report("top_product %s operands k=%d" % (str(dtype).split(".")[1], k), ms,
                   queries_per_s=N_Q / float(np.median(ms)) * 1e3,
                   TFLOP_per_s=2.0 * N_Q * N_ITEMS * RANK / float(np.median(ms)) / 1e9)
        del Vd, U


if __name__ == "__main__":
    {"normalize": normalize, "similar": similar, "top_product": top_product}[sys.argv[1]](HipBackend())
