"""the kernel of factor_init="device" alone at (10M, 128), fp32 and fp64, against a device fill of the same bytes: device events, 3 warm-up
calls, 20 alternating repetitions, medians.  python tools/gpu_init_bench.py [out.json]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rsparse_amd.engine import HipBackend

be = HipBackend()
n, k = 10_000_000, 128
res = {}
for dtype, name in ((torch.float32, "fp32"), (torch.float64, "fp64")):
    out = torch.empty((n, k), dtype=dtype, device=be.device)
    other = torch.empty((n, k), dtype=dtype, device=be.device)
    nbytes = out.numel() * out.element_size()
    def run_init(): be.init_factors(12345, 0, n, k, dtype, out=out)
    def run_init_ones(): be.init_factors(12345, 0, n, k, dtype, False, 0, out=out)
    def run_fill(): other.fill_(1.5)
    def run_zero(): other.zero_()
    fns = {"init": run_init, "init_ones_col": run_init_ones, "fill": run_fill, "memset": run_zero}
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {kname: [] for kname in fns}
    for rep in range(20):
        for kname, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); f(); b.record(); b.synchronize()
            times[kname].append(a.elapsed_time(b))
    row = {}
    for kname, t in times.items():
        t = sorted(t)
        med = t[len(t) // 2]
        row[kname] = {"ms_median": med, "ms_min": t[0], "ms_max": t[-1], "GBps_median": nbytes / med / 1e6}
    row["bytes"] = nbytes
    row["init_over_fill_time"] = row["init"]["ms_median"] / row["fill"]["ms_median"]
    row["init_rate_over_fill_rate"] = row["fill"]["ms_median"] / row["init"]["ms_median"]
    res[name] = row
    del out, other
    torch.cuda.empty_cache()
print(json.dumps(res, indent=1))
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
