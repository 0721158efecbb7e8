#!/usr/bin/env python3
"""The train / test split at scale (rsparse_hip_split_rows_device, wrmf_split.hip) on the synthetic users x items matrix of the
README's 1M x 100k lines (rsparse_amd.synth.make_dataset, users as rows, fp32 values).  Three modes: proportion p = 0.2, leave-out
n = 1 with random keys, leave-out n = 1 with `by` (a random float64 per entry).  Prints one JSON line per mode with, each the
median of --reps calls after a warm-up, timed with HIP events on resident inputs:

  split_ms      the whole `HipBackend.split_rows` call (count, scan, the read-back of the totals, compaction);
  clone_ms      `torch.clone` of the bytes the call must read and write (p, j, v in -- and `by` --; j, v out);
  torch_ms      the same split written with torch on the same device: a `torch.rand` mask (proportion) or a composite-key
                `torch.sort` of (row, random key | by) (leave-out), then boolean indexing and a `cumsum` for the row pointers;
  host_s        the host route: a numpy mask + two scipy constructions from (data, indices, indptr); for leave-out a per-row argsort over --host-rows rows,
                scaled to all rows (the scaled figure is marked);
  public_s      `rsparse_amd.train_test_split` on the scipy matrix: canonical check, upload, split, download, two constructions;

the kernel's achieved bytes/s (the clone's bytes over split_ms), whether the call repeats bit for bit, and the first rows checked
against the numpy specification.  Then the same call on ONE row of --long-row entries (a row is handled by one workgroup).

  python tools/gpu_split.py [--users 1000000] [--items 100000] [--reps 5] [--host-rows 100000] [--long-row 1000000] [--out profiles/split/split.jsonl]
"""
import argparse
import json
import math
import sys
import time
from pathlib import Path

import numpy as np
import scipy.sparse as sp
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from rsparse_amd import rng as R, synth, train_test_split  # noqa: E402
from rsparse_amd.engine import HipBackend  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=1_000_000)
ap.add_argument("--items", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--host-rows", type=int, default=100_000)
ap.add_argument("--long-row", type=int, default=1_000_000)
ap.add_argument("--out", default=None)
a = ap.parse_args()

be = HipBackend(0)
dev = be.device
d = synth.make_dataset(a.users, a.items, device=str(dev), feedback="implicit")
p, j, v = (t.to(dev).contiguous() for t in d["c_iu"])
del d
n_rows, nnz = int(p.numel()) - 1, int(j.numel())
g = torch.Generator(device=dev).manual_seed(1)
by = torch.rand(nnz, generator=g, device=dev, dtype=torch.float64) * 1.7e9
lens = torch.diff(p.to(torch.int64))
rows = torch.repeat_interleave(torch.arange(n_rows, device=dev), lens)
SEED, PROB = 7, 0.2
T = int(math.floor(PROB * 2.0 ** 32))


def timed(fn):
    fn()   # warm-up (code objects, the workspace, the caching allocator)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def compact(mask):
    """(train, test) CSR from a test mask, in torch: boolean indexing and a cumsum"""
    cs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(mask, 0)])
    te_p = cs[p.to(torch.int64)]
    return (p - te_p).to(torch.int32), j[~mask], v[~mask], te_p.to(torch.int32), j[mask], v[mask]


def torch_proportion():
    return compact(torch.rand(nnz, generator=g, device=dev) < PROB)


def torch_leave_out(keys):
    """a composite key (row ascending, key descending) sorted in one torch.sort; the first h of every row are test"""
    def run():
        k = keys() if callable(keys) else keys
        order = torch.argsort((rows << 32) | ((1 << 32) - 1 - k), stable=True)   # k: 32 bits
        h = torch.clamp(lens - 1, 0, 1)                                     # n = 1, min_train = 1
        first = (torch.arange(nnz, device=dev) - p.to(torch.int64)[rows[order]]) < h[rows[order]]
        mask = torch.zeros(nnz, dtype=torch.bool, device=dev)
        mask[order] = first
        return compact(mask)
    return run


by32 = torch.argsort(torch.argsort(by)).to(torch.int64) >> max(0, (nnz - 1).bit_length() - 32)   # (the torch route's 32-bit stand-in)
modes = [("proportion p = 0.2", dict(test_threshold=T), None, torch_proportion),
         ("leave-out n = 1, random keys", dict(leave_out=1, min_train=1), None,
          torch_leave_out(lambda: torch.randint(0, 1 << 32, (nnz,), generator=g, device=dev, dtype=torch.int64))),
         ("leave-out n = 1, by", dict(leave_out=1, min_train=1), by, torch_leave_out(by32))]

hp, hj, hv, hby = p.cpu().numpy(), j.cpu().numpy(), v.cpu().numpy(), by.cpu().numpy()
x_host = sp.csr_matrix((hv, hj, hp), shape=(n_rows, a.items))


def host_route(name, by_h):
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    scaled = False
    if name.startswith("proportion"):
        mask = rng.random(nnz) < PROB
    else:
        nr = min(n_rows, a.host_rows)
        mask = np.zeros(nnz, bool)
        key = rng.random(nnz) if by_h is None else by_h
        for u in range(nr):
            e0, e1 = hp[u], hp[u + 1]
            if e1 - e0 > 1:
                mask[e0 + np.argsort(-key[e0:e1], kind="stable")[0]] = True
        scaled = nr < n_rows
    t_mask = time.perf_counter() - t0
    if scaled:
        t_mask *= n_rows / nr
    t0 = time.perf_counter()
    te_p = np.concatenate([[0], np.cumsum(mask)])[hp]      # the caller holds a CSR: row pointers by a cumsum, no COO detour
    out = [sp.csr_matrix((hv[m], hj[m], q), shape=x_host.shape) for m, q in ((~mask, hp - te_p), (mask, te_p))]
    return t_mask + time.perf_counter() - t0, scaled, out[1].nnz


lines = []
for name, kw, by_t, torch_fn in modes:
    one = be.split_rows(SEED, 0, p, j, v, by=by_t, **kw)
    two = be.split_rows(SEED, 0, p, j, v, by=by_t, **kw)
    n_tr, n_te = int(one[1].numel()), int(one[4].numel())
    s_ms = timed(lambda: be.split_rows(SEED, 0, p, j, v, by=by_t, **kw))
    moved = [p, j, v, one[1], one[2], one[4], one[5]] + ([by_t] if by_t is not None else [])
    c_ms = timed(lambda: [t.clone() for t in moved])
    t_ms = timed(torch_fn)
    nbytes = sum(t.numel() * t.element_size() for t in moved)
    k = 2000
    e1 = int(hp[k])
    want = R.split_rows(SEED, 0, hp[:k + 1], hj[:e1], by=None if by_t is None else hby[:e1], **kw)
    ok = all(np.array_equal(one[o][:k + 1].cpu().numpy(), want[o]) and np.array_equal(one[o + 1][:int(want[o][-1])].cpu().numpy(), want[o + 1])
             for o in (0, 3))
    h_s, scaled, h_nte = host_route(name, None if by_t is None else hby)
    by_m = None if by_t is None else sp.csr_matrix((hby, hj, hp), shape=x_host.shape)
    pkw = dict(test_proportion=PROB) if "test_threshold" in kw else dict(leave_out=1, by=by_m)
    t0 = time.perf_counter()
    tr, te = train_test_split(x_host, seed=SEED, backend=be, **pkw)
    pub_s = time.perf_counter() - t0
    line = {"what": "split_rows: " + name, "users": n_rows, "items": a.items, "nnz": nnz, "train": n_tr, "test": n_te, "reps": a.reps,
            "split_ms": s_ms[0], "split_ms_min_max": list(s_ms[1:]), "clone_ms": c_ms[0], "clone_ms_min_max": list(c_ms[1:]),
            "torch_ms": t_ms[0], "torch_ms_min_max": list(t_ms[1:]), "bytes_moved": nbytes, "split_GBps": nbytes / s_ms[0] / 1e6,
            "clone_GBps": nbytes / c_ms[0] / 1e6, "split_over_clone": s_ms[0] / c_ms[0], "torch_over_split": t_ms[0] / s_ms[0],
            "host_s": h_s, "host_s_is_scaled_from_rows": a.host_rows if scaled else None, "host_over_split": h_s * 1e3 / s_ms[0],
            "public_s": pub_s, "public_equals_device": bool(te.nnz == n_te and np.array_equal(te.indices, one[4].cpu().numpy())),
            "repeat_bit_identical": bool(all(torch.equal(x, y) for x, y in zip(one, two))),
            "first_rows_equal_specification": bool(ok)}
    print(json.dumps(line), flush=True)
    lines.append(line)
    del one, two, moved, tr, te
# ---- one long row: a row is handled by ONE workgroup in the count and in the compaction, so this is what such a row costs alone
if a.long_row > 0:
    del p, j, v, by, rows, lens, by32
    L = a.long_row
    lp = torch.tensor([0, L], dtype=torch.int32, device=dev)
    lj = torch.arange(L, dtype=torch.int32, device=dev)
    lv = torch.rand(L, generator=g, device=dev)
    lby = torch.rand(L, generator=g, device=dev, dtype=torch.float64)
    for name, kw, by_t in (("proportion p = 0.2", dict(test_threshold=T), None), ("leave-out n = 1, random keys", dict(leave_out=1), None),
                           ("leave-out n = 1000, random keys", dict(leave_out=1000), None), ("leave-out n = 1, by", dict(leave_out=1), lby)):
        one = be.split_rows(SEED, 0, lp, lj, lv, by=by_t, **kw)
        s_ms = timed(lambda: be.split_rows(SEED, 0, lp, lj, lv, by=by_t, **kw))
        want = R.split_rows(SEED, 0, lp.cpu().numpy(), lj.cpu().numpy(), by=None if by_t is None else by_t.cpu().numpy(), **kw)
        line = {"what": "split_rows on ONE row: " + name, "row_entries": L, "test": int(one[4].numel()), "reps": a.reps,
                "split_ms": s_ms[0], "split_ms_min_max": list(s_ms[1:]), "entries_per_us": L / s_ms[0] / 1e3,
                "equals_specification": bool(np.array_equal(one[4].cpu().numpy(), want[4]) and np.array_equal(one[1].cpu().numpy(), want[1]))}
        print(json.dumps(line), flush=True)
        lines.append(line)
if a.out:
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(l) + "\n" for l in lines))
