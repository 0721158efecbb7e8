"""from_events at the bench matrix's scale on one GPU: a synthetic log (uniform users, Zipf(1) item popularity, a share of
repeated events) through HipBackend.events_to_csr, against the host route (scipy COO -> CSR + sum_duplicates), torch's
sparse_coo_tensor(...).coalesce() on the same GPU, and a device copy of the call's input and output bytes.  One JSON line per
measurement.

    python profiles/events/events_bench.py [--events 6.5e8] [--users 10000000] [--items 1000000] [--host-events 1e8]
                                           [--reps 3] [--device-only]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))


def say(**kw):
    print(json.dumps(kw), flush=True)


def make_log(n, n_users, n_items, repeat, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    n0 = int(n / (1.0 + repeat))
    users = torch.randint(0, n_users, (n0,), device=dev, generator=g, dtype=torch.int32)
    # Zipf with exponent 1 over the items: the rank is log-uniform
    r = torch.rand(n0, device=dev, generator=g, dtype=torch.float64)
    items = (torch.exp(r * float(np.log(n_items))).floor().to(torch.int64) - 1).clamp_(0, n_items - 1).to(torch.int32)
    del r
    again = torch.randint(0, n0, (n - n0,), device=dev, generator=g)          # events that repeat an earlier one
    users, items = torch.cat([users, users[again]]), torch.cat([items, items[again]])
    del again
    perm = torch.randperm(n, device=dev, generator=g)
    users, items = users[perm].contiguous(), items[perm].contiguous()
    del perm
    values = torch.rand(n, device=dev, generator=g, dtype=torch.float64) + 0.5
    stamps = torch.rand(n, device=dev, generator=g, dtype=torch.float64) * 1e9
    return users, items, values, stamps


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
        del res
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=float, default=6.5e8)
    ap.add_argument("--users", type=int, default=10_000_000)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=float, default=0.1)
    ap.add_argument("--host-events", type=float, default=1e8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    dev = be.device
    n = int(a.events)
    users, items, values, stamps = make_log(n, a.users, a.items, a.repeat, dev, 1)
    bits = lambda k: max(int(k) - 1, 0).bit_length()
    key_bytes = 4 if bits(a.users) + bits(a.items) <= 32 else 8
    say(what="log", events=n, users=a.users, items=a.items, key_bits=bits(a.users) + bits(a.items),
        workspace_bytes_per_event=2 * key_bytes + 8, long_cell_scratch_bytes_per_event=round(16 / 65 + 20 / 32, 2))

    def call(u, i, v, t, **kw):
        return be.events_to_csr(u, i, v, t, a.users, a.items, **kw)

    for name, v, t, kw in (("sum", values, stamps, {}), ("sum, no timestamps", values, None, {}), ("count, pattern only", None, None, dict(aggregate="count")),
                           ("last", values, stamps, dict(aggregate="last")), ("sum, half_life", values, stamps, dict(half_life=1e8))):
        call(users, items, v, t, **kw)                       # (warm-up: code objects, the allocator)
        med, all_t = timed(lambda: call(users, items, v, t, **kw), a.reps)
        cells = int(call(users, items, v, t, **kw)[1].numel())
        say(what="events_to_csr", case=name, seconds=med, runs=all_t, cells=cells, events_per_cell=n / cells,
            events_per_second=n / med)
    in_bytes = n * 24
    out_bytes = cells * 24 + (a.users + 1) * 4
    src, dst = torch.empty(in_bytes + out_bytes, dtype=torch.uint8, device=dev), torch.empty(in_bytes + out_bytes, dtype=torch.uint8, device=dev)
    med, all_t = timed(lambda: dst.copy_(src), a.reps)
    say(what="device copy of the input and output bytes", bytes=in_bytes + out_bytes, seconds=med, runs=all_t)
    del src, dst
    # one cell with a tenth of all events
    hot = torch.rand(n, device=dev) < 0.1
    u2, i2 = users.clone(), items.clone()
    u2[hot], i2[hot] = 123, 456
    del hot
    call(u2, i2, values, stamps)
    med, all_t = timed(lambda: call(u2, i2, values, stamps), a.reps)
    out = call(u2, i2, values, stamps)
    say(what="events_to_csr", case="sum, one cell with a tenth of the events", seconds=med, runs=all_t, cells=int(out[1].numel()),
        largest_cell=int(out[3].max()))
    del out, u2, i2
    if a.device_only:
        return
    try:
        def coalesce():
            idx = torch.stack([users.to(torch.int64), items.to(torch.int64)])
            return torch.sparse_coo_tensor(idx, values, (a.users, a.items)).coalesce()
        coalesce()
        med, all_t = timed(coalesce, a.reps)
        say(what="torch.sparse_coo_tensor(...).coalesce()", events=n, seconds=med, runs=all_t)
    except Exception as e:   # (out of memory at this size is a result too)
        say(what="torch.sparse_coo_tensor(...).coalesce()", events=n, error=repr(e)[:200])
    torch.cuda.empty_cache()
    import scipy.sparse as sp
    h = min(n, int(a.host_events))
    hu, hi, hv = users[:h].cpu().numpy(), items[:h].cpu().numpy(), values[:h].cpu().numpy()
    t0 = time.perf_counter()
    m = sp.coo_matrix((hv, (hu, hi)), shape=(a.users, a.items)).tocsr()
    t1 = time.perf_counter()
    m.sum_duplicates()
    t2 = time.perf_counter()
    say(what="host route: coo_matrix.tocsr() + sum_duplicates()", events=h, tocsr_seconds=t1 - t0, sum_duplicates_seconds=t2 - t1,
        seconds=t2 - t0, cells=int(m.nnz))
    med, all_t = timed(lambda: call(users[:h], items[:h], values[:h], None), a.reps)
    say(what="events_to_csr", case="sum, no timestamps, the host route's events", events=h, seconds=med, runs=all_t)


if __name__ == "__main__":
    main()
