"""Hit-based metrics at several cutoffs on the MI355X: every output of wrmf_hits.hip (hits, first, precision, recall, hit, mrr,
first_seen and the coverage counted from it) against the numpy definition `rsparse_amd.metrics.hit_metrics_reference`, BIT FOR
BIT -- every double is one division of two integers, so there is no tolerance --, at the list widths, cutoff sets, row lengths
and user counts at which the kernel takes another path: the 64-position chunk edge, cutoffs that stop short of k, the LDS cap of
512 entries, a partly filled last workgroup.  The device form, the host form, each output alone, a repeated call, two row batches
sharing one first_seen, and `WRMF.evaluate` with a sequence of cutoffs on the movielens fixture."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from test_metrics_abi import NA

pytestmark = pytest.mark.gpu

N_ITEMS = 20000
NEVER = 2 ** 31 - 1
INTS, DOUBLES = ("hits", "first"), ("precision", "recall", "hit", "mrr")


def _same(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    if got.dtype != ref.dtype or got.shape != ref.shape:
        return False
    if got.dtype == np.float64:
        return np.array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(ref).view(np.uint64))
    return np.array_equal(got, ref)


def _cutoff_sets(k):
    sets = [(1,), (63, 64, 65), (1, 64, 128, 129), (k,), (2, 3), (1, k // 2, k - 1), (60, 100, 127),
            tuple(int(c) for c in np.unique(np.linspace(1, k, 16).astype(int)))]
    return sorted({s for s in sets if s[0] >= 1 and s[-1] <= k and all(b > a for a, b in zip(s, s[1:]))})


def _case(k, n_users, seed):
    """R-style lists (1-based, NA) with 0, n_item + 1, negative and repeated entries mixed in, against rows of 0, 1, k / 2, k,
    k + 3, 512, 513 (the LDS-cap edge), 600 and 2000 held-out items"""
    rng = np.random.default_rng(seed)
    lens = [0, 1, max(1, k // 2), k, k + 3, 512, 513, 600, 2000]
    indptr, cols, pred = [0], [], np.empty((n_users, k), dtype=np.int32)
    for u in range(n_users):
        L = lens[(u + seed) % len(lens)]
        c = np.sort(rng.choice(N_ITEMS, size=L, replace=False))
        cols.append(c)
        indptr.append(indptr[-1] + L)
        pr = rng.integers(1, N_ITEMS + 1, k)
        if L:
            h = rng.random(k) < 0.3
            pr[h] = rng.choice(c, size=int(h.sum())) + 1
        r = rng.random(k)
        pr[r < 0.04] = NA
        pr[(r >= 0.04) & (r < 0.06)] = 0
        pr[(r >= 0.06) & (r < 0.08)] = N_ITEMS + 1
        pr[(r >= 0.08) & (r < 0.10)] = -rng.integers(1, 50)
        if k > 3:
            pr[3] = pr[1]
        pred[u] = pr
    j = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32)
    actual = sp.csr_matrix((np.ones(j.size), j, np.array(indptr, dtype=np.int32)), shape=(n_users, N_ITEMS))
    assert actual.indptr.dtype == np.int32 and actual.indices.dtype == np.int32
    return pred, actual


def _reference(pred1, actual, cutoffs):
    from rsparse_amd.metrics import hit_metrics_reference
    return hit_metrics_reference(pred1.astype(np.int64) - 1, actual, cutoffs, n_item=N_ITEMS)   # (NA and 0 turn negative)


class _Dev:
    def __init__(self, pred1, actual):
        from rsparse_amd.engine import HipBackend
        self.be = HipBackend()
        self.res = self.be.to_device(pred1, torch.int32)                    # row-major, as top_product writes it
        self.p = self.be.to_device(actual.indptr, torch.int32)
        self.j = self.be.to_device(actual.indices, torch.int32)

    def seen(self):
        return torch.full((N_ITEMS,), NEVER, dtype=torch.int32, device=self.res.device)

    def run(self, cutoffs, want, seen=None, rows=None):
        a, b = rows or (0, self.res.shape[0])
        out = self.be.hit_metrics(self.res[a:b], self.p[a:b + 1], self.j, cutoffs, want, seen)
        return {m: v.cpu().numpy() for m, v in out.items()}


def _check(got, ref, names):
    for m in names:
        assert _same(got[m], ref[m]), m


@pytest.mark.parametrize("k,n_users", [(1, 1), (5, 5), (64, 6), (65, 7), (200, 301), (8192, 27)])
def test_every_output_equals_the_definition(k, n_users):
    from rsparse_amd.metrics import coverage_from_first_seen
    pred1, actual = _case(k, n_users, 11 + k)
    dev = _Dev(pred1, actual)
    for cutoffs in _cutoff_sets(k):
        ref = _reference(pred1, actual, cutoffs)
        seen = dev.seen()
        got = dev.run(cutoffs, INTS + DOUBLES, seen)
        _check(got, ref, INTS + DOUBLES)
        fs = seen.cpu().numpy()
        assert _same(fs, ref["first_seen"]) and _same(coverage_from_first_seen(fs, cutoffs), ref["coverage"])
        assert (fs[fs != NEVER] <= cutoffs[-1]).all() and (ref["first"] <= cutoffs[-1]).all()   # nothing beyond c_T counts
        # without coverage (the other instantiation; rows with nothing held out return early)
        _check(dev.run(cutoffs, INTS + DOUBLES), ref, INTS + DOUBLES)
    empty = np.diff(actual.indptr) == 0
    assert np.isnan(got["recall"][empty]).all() and not np.isnan(got["recall"][~empty]).any()


def test_each_output_alone_repeats_and_row_batches():
    k, n = 200, 301
    pred1, actual = _case(k, n, 5)
    assert {512, 513, 0}.issubset(set(np.diff(actual.indptr).tolist()))
    dev = _Dev(pred1, actual)
    cutoffs = (1, 64, 128, 129)
    ref = _reference(pred1, actual, cutoffs)
    for m in INTS + DOUBLES:                                                # every nullable output on its own
        got = dev.run(cutoffs, (m,))
        assert list(got) == [m] and _same(got[m], ref[m]), m
        seen = dev.seen()
        got = dev.run(cutoffs, (m,), seen)
        assert _same(got[m], ref[m]) and _same(seen.cpu().numpy(), ref["first_seen"]), m
    seen = dev.seen()                                                        # coverage alone
    assert dev.run(cutoffs, (), seen) == {} and _same(seen.cpu().numpy(), ref["first_seen"])
    with pytest.raises(ValueError):
        dev.run(cutoffs, ())
    # a repeated call returns the same bits, and leaves a first_seen that is already complete as it is
    again = dev.run(cutoffs, INTS + DOUBLES, seen)
    _check(again, ref, INTS + DOUBLES)
    assert _same(seen.cpu().numpy(), ref["first_seen"])
    # two row batches sharing one first_seen are one call on all rows
    seen = dev.seen()
    h = 150
    lo, hi = dev.run(cutoffs, INTS + DOUBLES, seen, (0, h)), dev.run(cutoffs, INTS + DOUBLES, seen, (h, n))
    for m in INTS + DOUBLES:
        assert _same(np.concatenate([lo[m], hi[m]]), ref[m]), m
    assert _same(seen.cpu().numpy(), ref["first_seen"])


@pytest.mark.parametrize("k,n_users,cutoffs", [(5, 7, (2, 3)), (200, 40, (63, 64, 65)), (8192, 10, (10, 500, 8192))])
def test_host_form_and_python_functions(k, n_users, cutoffs):
    from rsparse_amd import _lib, metrics
    pred1, actual = _case(k, n_users, 3 + k)
    ref = _reference(pred1, actual, cutoffs)
    T = len(cutoffs)
    lib = _lib.load()
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    p1 = np.asfortranarray(pred1)                                            # R's column-major integer matrix
    cut = np.array(cutoffs, dtype=np.int32)
    out = {m: np.empty((n_users, T), dtype=np.int32 if m == "hits" else np.float64, order="F") for m in ("hits",) + DOUBLES}
    out["first"] = np.empty(n_users, np.int32)
    seen = np.zeros(N_ITEMS, np.int32)                                       # (the call initialises it)
    _lib.check(lib.rsparse_hip_hit_metrics(vp(p1), n_users, k, vp(actual.indptr), vp(actual.indices), vp(cut), T, vp(out["hits"]),
                                           vp(out["first"]), vp(out["precision"]), vp(out["recall"]), vp(out["hit"]),
                                           vp(out["mrr"]), vp(seen), N_ITEMS))
    _check(out, ref, INTS + DOUBLES)
    assert _same(seen, ref["first_seen"])
    only = np.empty((n_users, T), order="F")
    _lib.check(lib.rsparse_hip_hit_metrics(vp(p1), n_users, k, vp(actual.indptr), vp(actual.indices), vp(cut), T, None, None, None,
                                           vp(only), None, None, None, 0))
    assert _same(only, ref["recall"])
    # the Python functions take 0-based lists with -1 (anything negative is a miss)
    pred0 = np.where(pred1 == NA, -1, pred1.astype(np.int64) - 1)
    got = metrics.topk_metrics(pred0, actual, cutoffs, metrics=INTS + DOUBLES + ("coverage",))
    _check(got, ref, INTS + DOUBLES + ("first_seen", "coverage"))
    assert _same(metrics.recall_k(pred0, actual, cutoffs), ref["recall"])
    assert _same(metrics.precision_k(pred0, actual, cutoffs[1]), ref["precision"][:, 1])
    assert _same(metrics.hit_rate_k(pred0[:, :cutoffs[0]], actual), ref["hit"][:, 0])
    assert _same(metrics.mrr_k(pred0, actual, cutoffs), ref["mrr"])
    assert _same(metrics.coverage_k(pred0, N_ITEMS, cutoffs), ref["coverage"])
    assert metrics.coverage_k(pred0, N_ITEMS, cutoffs[0]) == ref["coverage"][0]


# ---- WRMF.evaluate end to end ------------------------------------------------------------------------------------------------
def test_evaluate_at_several_cutoffs_on_movielens(ml_train):
    from rsparse_amd import WRMF
    from rsparse_amd.metrics import ap_k, hit_metrics_reference, ndcg_k, summarize
    n_user, n_item, tp, ti, tx = ml_train
    full = sp.csc_matrix((tx, ti, tp), shape=(n_user, n_item)).tocsr()
    rng = np.random.default_rng(21)
    coo = full.tocoo()
    out = rng.random(coo.nnz) < 0.2                                   # a fifth of every user's ratings held out
    train = sp.csr_matrix((coo.data[~out], (coo.row[~out], coo.col[~out])), shape=full.shape)
    held = sp.csr_matrix((coo.data[out], (coo.row[out], coo.col[out])), shape=full.shape)
    m = WRMF(rank=10, lambda_=0.1, feedback="implicit", solver="conjugate_gradient", precision="float", rng=1)
    m.fit_transform(train, n_iter=3, convergence_tol=-1)
    assert hasattr(m._backend(), "hit_metrics")
    K = (1, 5, 10, 20)
    names = ("ap", "ndcg", "precision", "recall", "hit", "mrr", "coverage")
    cand = sp.csr_matrix(rng.random(full.shape) < 0.1, dtype=np.float64)
    ways = {"plain": ({}, {}), "candidates": ({"candidates": cand}, {"candidates": cand}),
            "negatives": ({"negatives": 99, "seed": 7}, {"candidates": m.sample_negatives(train, 99, actual=held, seed=7)})}
    for way, (ev_args, pr_args) in ways.items():
        ev = m.evaluate(train, held, K, metrics=names, **ev_args)
        top = m.predict(train, 20, **pr_args)
        ref = hit_metrics_reference(np.asarray(top), held, K, n_item=n_item)
        for name in ("precision", "recall", "hit", "mrr", "coverage"):
            assert _same(ev[name], ref[name]), (way, name)
        for t, c in enumerate(K):
            assert _same(ev["ap"][:, t], ap_k(np.asarray(top)[:, :c], held)), (way, c)
            assert _same(ev["ndcg"][:, t], ndcg_k(np.asarray(top)[:, :c], held)), (way, c)
        s = summarize(ev)
        assert s["hit"].shape == (4,) and (np.diff(s["hit"]) >= 0).all() and s["hit"][-1] > 0.05, way
        assert (np.diff(ev["coverage"]) >= 0).all() and ev["coverage"][0] < ev["coverage"][-1] <= 1.0
    one = m.evaluate(train, held, 10, metrics=("hit", "coverage", "ndcg"))
    both = m.evaluate(train, held, K, metrics=("hit", "coverage"))
    assert one["hit"].shape == (n_user,) and _same(one["hit"], both["hit"][:, 2]) and one["coverage"] == both["coverage"][2]
    assert _same(one["ndcg"], m.evaluate(train, held, 10)["ndcg"])
