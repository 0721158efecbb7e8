"""BPR / WARP through item features (wrmf_bpr_features.hip) on one GPU at the shape of profiles/bpr/: 1 000 000 users x
100 000 items, 5e7 entries with Zipf item popularity, fp32.  One JSON line per measurement, appended to --out (default
bpr_features_bench.jsonl here); medians of --reps runs behind a warm-up, each timed by two events around the call.

    python profiles/bpr_features/bpr_features_bench.py --step epoch     a plain epoch and an epoch through each feature set, side by
                                                                        side in one process, BPR and WARP, at --ranks
    python profiles/bpr_features/bpr_features_bench.py --step compose   the compose launch alone for each feature set
Feature sets (--sets): identity; identity + 1000 Zipf tags (5 per item); the tags alone; --losses bpr,warp.  The split of a step
between the launches comes from a kernel trace of one set and one loss at `--step epoch --reps 1` (the README has the command).
"""
import argparse
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "profiles" / "bpr"))
OUT = HERE / "bpr_features_bench.jsonl"


def say(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def feature_sets(n_items, n_tags=1000, per_item=5):
    """-> {name: scipy CSR, n_items x n_feat}: the tags of an item are `per_item` draws from a Zipf law over the tags"""
    import numpy as np
    import scipy.sparse as sp
    rng = np.random.default_rng(3)
    w = 1.0 / np.arange(1, n_tags + 1)
    tags = rng.choice(n_tags, size=(n_items, per_item), p=w / w.sum())
    T = sp.csr_matrix((np.ones(tags.size), (np.repeat(np.arange(n_items), per_item), tags.reshape(-1))), shape=(n_items, n_tags))
    T.data[:] = 1.0                                                        # (a tag drawn twice counts once)
    eye = sp.identity(n_items, format="csr")
    return {"identity": eye, "identity+tags": sp.hstack([eye, T]).tocsr(), "tags": T}


def main(a):
    import numpy as np
    import torch
    import bpr_bench
    from rsparse_amd.bpr import canonical_features
    from rsparse_amd.engine import HipBackend
    from rsparse_amd.warp import rank_weights
    be = HipBackend()
    sets = {k: canonical_features(F, a.items, np.float32) for k, F in feature_sets(a.items).items() if k in a.sets}
    feats = {k: be.item_features(F, torch.float32) for k, F in sets.items()}
    shape = {k: dict(n_feat=F.shape[1], nnz_f=int(F.nnz), longest_column=int(np.diff(F.tocsc().indptr).max())) for k, F in sets.items()}
    if a.step == "compose":
        for rank in a.ranks:
            for k, feat in feats.items():
                H = be.init_factors(7, 1, feat[6], rank, torch.float32)
                t = bpr_bench.timed(lambda: be.compose_rows(feat, H), a.reps, torch)
                moved = (shape[k]["nnz_f"] + a.items) * rank * 4
                say(step="compose", features=k, rank=rank, moved_gb=round(moved / 1e9, 3), tb_per_s=round(moved / 1e12 / (t["ms"] / 1e3), 3),
                    **t, **shape[k])
        return
    nnz, p, j = bpr_bench.dataset(a, torch)
    w = rank_weights(a.items, 50)
    for rank in a.ranks:
        for loss in a.losses:
            U, V, aU, aV = bpr_bench.factors(be, a, rank, torch)
            if loss == "bpr":
                plain = lambda: be.bpr_epochs(p, j, a.items, nnz, 0, 11, 0, 0, 1, a.batch, U, V, aU, aV, 0.05, 0.01)
            else:
                plain = lambda: be.warp_epochs(p, j, a.items, nnz, 0, 11, 0, 0, 1, a.batch, 50, 0.1, w, U, V, aU, aV, 0.05, 0.01)
            base = bpr_bench.timed(plain, a.reps, torch)
            say(step="epoch", loss=loss, features=None, rank=rank, batch=a.batch, nnz=nnz, **base)
            del V, aV
            for k, feat in feats.items():
                H = be.init_factors(7, 1, feat[6], rank, torch.float32)
                aH = torch.zeros(feat[6], dtype=torch.float64, device=be.device)
                if loss == "bpr":
                    run = lambda: be.bpr_feat_epochs(p, j, nnz, 0, 11, 0, 0, 1, a.batch, feat, U, H, aU, aH, 0.05, 0.01)
                else:
                    run = lambda: be.warp_feat_epochs(p, j, nnz, 0, 11, 0, 0, 1, a.batch, 50, 0.1, w, feat, U, H, aU, aH, 0.05, 0.01)
                t = bpr_bench.timed(run, a.reps, torch)
                say(step="epoch", loss=loss, features=k, rank=rank, batch=a.batch, nnz=nnz, over_plain=round(t["ms"] / base["ms"], 3), **t,
                    **shape[k])
                del H, aH
            del U, aU


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True, choices=("epoch", "compose"))
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--nnz", type=float, default=5e7)
    ap.add_argument("--ranks", type=lambda s: [int(v) for v in s.split(",")], default=[64, 128])
    ap.add_argument("--sets", type=lambda s: s.split(","), default=["identity", "identity+tags", "tags"])
    ap.add_argument("--losses", type=lambda s: s.split(","), default=["bpr", "warp"])
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(OUT))
    a = ap.parse_args()
    OUT = Path(a.out)
    main(a)
