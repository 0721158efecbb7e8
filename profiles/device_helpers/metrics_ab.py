"""ndcg@k on rows longer than kMetRowCap (512 stored entries), so that metrics_long_kernel and its radix select run; the one
kernel whose listing moved in the device-helper refactor.

    RSPARSE_HIP_LIB=parent.so python profiles/device_helpers/metrics_ab.py run parent.npz
    python profiles/device_helpers/metrics_ab.py run new.npz                    (a fresh process per library)
    python profiles/device_helpers/metrics_ab.py compare parent.npz new.npz     (bitwise: the select is integer arithmetic)
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))


def run(out):
    import scipy.sparse as sp
    from rsparse_amd import metrics
    rng = np.random.default_rng(11)
    n_users, n_items = 300, 6000
    rows, cols, vals = [], [], []
    for u in range(n_users):
        n_u = int(rng.integers(513, 4000)) if u % 10 else int(rng.integers(1, 513))   # every tenth row stays in launch 1
        c = rng.choice(n_items, n_u, replace=False)
        kind = u % 4
        if kind == 0:
            v = rng.standard_normal(n_u)                                   # both signs
        elif kind == 1:
            v = rng.integers(0, 6, n_u).astype(np.float64)                 # heavy ties, stored zeros
        elif kind == 2:
            v = np.exp(rng.standard_normal(n_u) * 8.0)                     # a wide range of exponents
        else:
            v = np.where(rng.random(n_u) < 0.5, -0.0, rng.integers(0, 3, n_u).astype(np.float64))   # -0.0 against +0.0
        rows.append(np.full(n_u, u)), cols.append(c), vals.append(v)
    actual = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n_users, n_items))
    res = {}
    for k in (1, 10, 100, 600, 3000):
        pred = np.stack([rng.permutation(n_items)[:k] for _ in range(n_users)]).astype(np.int32)
        ap, ndcg = metrics.ranking_metrics(pred, actual)
        res["ap_%d" % k], res["ndcg_%d" % k] = ap, ndcg
    np.savez(out, **res)
    print("wrote", out, {k: float(np.nanmean(v)) for k, v in res.items()})


def compare(a, b):
    da, db = np.load(a), np.load(b)
    bad = 0
    for key in da.files:
        same = np.array_equal(da[key].view(np.uint64), db[key].view(np.uint64))
        bad += not same
        print("%-10s %d rows  %s" % (key, da[key].size, "bitwise equal" if same else "DIFFERS"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(run(sys.argv[2]) if sys.argv[1] == "run" else compare(sys.argv[2], sys.argv[3]))
