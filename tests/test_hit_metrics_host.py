"""Hit-based metrics at several cutoffs (precision, recall, hit rate, reciprocal rank, coverage) without a device: the numpy
definition `rsparse_amd.metrics.hit_metrics_reference` on hand-worked lists and against a position-by-position restatement, the
identities that hold for any input, `WRMF.evaluate` with a sequence of cutoffs on the CPU stand-in backend (which has no
`hit_metrics` and so gets the definition through the `hasattr` fallback) -- plain, `candidates=`, `negatives=` and on two gloo
ranks --, the argument errors, and the status codes of the two C entry points."""
import ctypes
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import _lib
from test_metrics_abi import NA, _eval_model, ref_metrics, to_r

ROOT = Path(__file__).resolve().parent.parent
NEVER = 2 ** 31 - 1
ALL = ("ap", "ndcg", "precision", "recall", "hit", "mrr", "coverage")


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def restated(pred, actual, cutoffs, n_item):
    """the definition once more, one position at a time in plain Python (canonical CSR `actual`)"""
    n, T = pred.shape[0], len(cutoffs)
    hits, first = np.zeros((n, T), np.int32), np.zeros(n, np.int32)
    dbl = {m: np.zeros((n, T)) for m in ("precision", "recall", "hit", "mrr")}
    seen = np.full(n_item, NEVER, np.int32)
    for u in range(n):
        row = set(actual.indices[actual.indptr[u]:actual.indptr[u + 1]].tolist())
        for i in range(1, cutoffs[-1] + 1):
            c = int(pred[u, i - 1])
            if 0 <= c < n_item:
                seen[c] = min(seen[c], i)
            if c in row:
                if first[u] == 0:
                    first[u] = i
                for t, ct in enumerate(cutoffs):
                    hits[u, t] += i <= ct
        for t, ct in enumerate(cutoffs):
            if not row:
                for m in dbl:
                    dbl[m][u, t] = np.nan
                continue
            dbl["precision"][u, t] = np.float64(hits[u, t]) / np.float64(ct)
            dbl["recall"][u, t] = np.float64(hits[u, t]) / np.float64(len(row))
            dbl["hit"][u, t] = 1.0 if hits[u, t] > 0 else 0.0
            dbl["mrr"][u, t] = np.float64(1.0) / np.float64(first[u]) if 0 < first[u] <= ct else 0.0
    cov = np.array([np.float64(np.count_nonzero(seen <= ct)) / np.float64(n_item) for ct in cutoffs])
    return dict(dbl, hits=hits, first=first, first_seen=seen, coverage=cov)


# ---- hand-worked lists ---------------------------------------------------------------------------------------------------------
def _hand():
    pred = np.array([[2, 7, 4, 1, 0, 4],                  # hits at 1 and 3
                     [0, 1, 2, 3, 9, 5],                  # a hit only at c_T = 5
                     [0, 1, 2, 4, 5, 3],                  # the held-out item at 6 > c_T: no hit
                     [5, 5, 5, -1, -1, -1],               # a repeated index hits every time
                     [-1, -5, 10, 11, 1, 1],              # NA, negative, out of range, then a hit at 5
                     [7, 0, 1, 2, 3, 4],                  # a stored zero is relevant
                     [0, 1, 2, 3, 4, 5],                  # an empty row
                     [0, 1, 2, 3, 4, 5]], dtype=np.int64)  # a row longer than k
    rows = [0, 0, 1, 2, 3, 3, 4, 5] + [7] * 8
    cols = [2, 4, 9, 3, 5, 6, 1, 7] + list(range(8))
    vals = [1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 3.0, 0.0] + [1.0] * 8
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=8))])
    actual = sp.csr_matrix((np.array(vals), np.array(cols), indptr), shape=(8, 10))
    assert actual.nnz == 16 and (actual.data == 0).sum() == 1
    return pred, actual


def test_hand_worked_lists():
    from rsparse_amd.metrics import hit_metrics_reference
    pred, actual = _hand()
    r = hit_metrics_reference(pred, actual, (1, 3, 5), n_item=10)
    assert r["hits"].dtype == np.int32 and r["first"].dtype == np.int32 and r["first_seen"].dtype == np.int32
    assert r["hits"].tolist() == [[1, 2, 2], [0, 0, 1], [0, 0, 0], [1, 3, 3], [0, 0, 1], [1, 1, 1], [0, 0, 0], [1, 3, 5]]
    assert r["first"].tolist() == [1, 5, 0, 1, 5, 1, 0, 1]
    assert _same(r["precision"][0], np.array([1.0, 2 / 3, 2 / 5])) and _same(r["recall"][0], np.array([0.5, 1.0, 1.0]))
    assert _same(r["mrr"][1], np.array([0.0, 0.0, 1 / 5])) and _same(r["hit"][1], np.array([0.0, 0.0, 1.0]))
    assert not r["hit"][2].any() and not r["mrr"][2].any() and not r["recall"][2].any()
    assert _same(r["precision"][3], np.array([1.0, 1.0, 3 / 5])) and _same(r["recall"][3], np.array([0.5, 1.5, 1.5]))
    assert _same(r["recall"][4], np.array([0.0, 0.0, 1.0])) and _same(r["precision"][4], np.array([0.0, 0.0, 1 / 5]))
    assert _same(r["hit"][5], np.ones(3)) and _same(r["mrr"][5], np.ones(3))
    for m in ("precision", "recall", "hit", "mrr"):
        assert np.isnan(r[m][6]).all() and not np.isnan(np.delete(r[m], 6, axis=0)).any()
    assert _same(r["recall"][7], np.array([1 / 8, 3 / 8, 5 / 8])) and _same(r["precision"][7], np.ones(3))
    # coverage counts every row, the empty one included, and nothing beyond c_T = 5
    assert r["first_seen"].tolist() == [1, 2, 1, 4, 3, 1, NEVER, 1, NEVER, 5]
    assert _same(r["coverage"], np.array([4 / 10, 6 / 10, 8 / 10]))
    full = restated(pred, actual, (1, 3, 5), 10)
    for name in full:
        assert _same(r[name], full[name]), name
    # one cutoff at k reads the whole list: row 2's item at position 6 is found
    r6 = hit_metrics_reference(pred, actual, (6,))
    assert r6["first"][2] == 6 and r6["hits"][2, 0] == 1 and "coverage" not in r6


def _random_case(seed, n=60, k=40, n_item=300):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 12, n)
    lens[:8] = [0, 1, 1, 1, 1, 0, 50, 45]
    rows = np.repeat(np.arange(n), lens)
    cols = np.concatenate([np.sort(rng.choice(n_item, size=l, replace=False)) for l in lens])
    actual = sp.csr_matrix((rng.integers(0, 3, rows.size).astype(float), cols, np.concatenate([[0], np.cumsum(lens)])),
                           shape=(n, n_item))
    pred = rng.integers(0, n_item, (n, k))
    for u in range(n):
        if lens[u] == 1:                                   # one held-out item, listed at most once
            item = cols[actual.indptr[u]]
            pred[u][pred[u] == item] = (item + 1) % n_item
            if u % 3:
                pred[u, (7 * u) % k] = item
        elif lens[u]:
            h = rng.random(k) < 0.2
            pred[u, h] = rng.choice(cols[actual.indptr[u]:actual.indptr[u + 1]], size=int(h.sum()))
    r = rng.random((n, k))
    pred[r < 0.05] = -1
    pred[(r >= 0.05) & (r < 0.08)] = n_item + 3
    pred[(r >= 0.08) & (r < 0.1)] = -7
    return pred, actual


@pytest.mark.parametrize("cutoffs", [(1,), (40,), (1, 5, 10, 20), (3, 39), tuple(range(2, 34, 2))])
def test_definition_and_identities_on_random_lists(cutoffs):
    from rsparse_amd.metrics import hit_metrics_reference
    pred, actual = _random_case(5)
    n_item = actual.shape[1]
    r = hit_metrics_reference(pred, actual, cutoffs, n_item=n_item)
    full = restated(pred, actual, cutoffs, n_item)
    for name in full:
        assert _same(r[name], full[name]), name
    cut = np.array(cutoffs)
    ok = np.diff(actual.indptr) > 0
    # (one rounding in the quotient, one in the product: two ulps of a count of at most 40)
    assert np.abs(r["precision"][ok] * cut - r["hits"][ok]).max() <= 4 * 40 * 2.0 ** -53
    assert (np.diff(r["hits"], axis=1) >= 0).all() and (r["hits"] <= cut).all()
    assert _same(r["hit"][ok], (r["hits"][ok] > 0).astype(np.float64))
    assert np.array_equal(r["mrr"][ok] > 0, r["hit"][ok] == 1)
    one = (np.diff(actual.indptr) == 1) & (r["hits"][:, -1] <= 1)                   # one held-out item, not listed twice
    assert one.sum() >= 4
    assert _same(r["recall"][one], r["hit"][one])
    assert (np.diff(r["coverage"]) >= 0).all()
    head = pred[:, :cut[-1]]
    assert r["coverage"][-1] == np.unique(head[(head >= 0) & (head < n_item)]).size / n_item
    # positions beyond c_T play no part
    scr = pred.copy()
    scr[:, cut[-1]:] = 0
    r2 = hit_metrics_reference(scr, actual, cutoffs, n_item=n_item)
    for name in r:
        assert _same(r[name], r2[name]), name


def test_summarize():
    from rsparse_amd.metrics import summarize
    ev = {"hit": np.array([[1.0, 1.0], [np.nan, np.nan], [0.0, 1.0]]), "ap": np.array([0.5, np.nan, 0.25]),
          "coverage": np.array([0.1, 0.2]), "mrr": np.full((2, 2), np.nan)}
    s = summarize(ev)
    assert _same(s["hit"], np.array([0.5, 1.0])) and s["ap"] == 0.375 and s["coverage"] is ev["coverage"]
    assert np.isnan(s["mrr"]).all() and s["mrr"].shape == (2,)


# ---- WRMF.evaluate on the CPU stand-in backend ---------------------------------------------------------------------------------
K = (1, 3, 10)


def _check_against_lists(ev, top, held, n_item, cutoffs=K):
    from rsparse_amd.metrics import hit_metrics_reference
    ref = hit_metrics_reference(np.asarray(top), held, cutoffs, n_item=n_item)
    for name in ("precision", "recall", "hit", "mrr", "coverage"):
        assert _same(ev[name], ref[name]), name
    for t, c in enumerate(cutoffs):
        ap, ndcg = ref_metrics(to_r(np.asarray(top)[:, :c]), sp.csr_matrix(held))
        assert _same(ev["ap"][:, t], ap) and _same(ev["ndcg"][:, t], ndcg)


def test_evaluate_at_several_cutoffs_equals_the_definition_on_predict():
    model, m, held = _eval_model()
    assert not hasattr(model._backend(), "hit_metrics")
    n, n_item = m.shape
    ev = model.evaluate(m, held, K, metrics=ALL)
    assert list(ev) == list(ALL) and ev["coverage"].shape == (3,)
    assert all(ev[name].shape == (n, 3) and ev[name].dtype == np.float64 for name in ALL[:-1])
    _check_against_lists(ev, model.predict(m, 10), held, n_item)
    assert np.nansum(ev["hit"][:, 2]) > 10
    # a scalar k: vectors and a float, equal to the one-cutoff column; ap / ndcg as they always were
    one = model.evaluate(m, held, 10, metrics=ALL)
    old = model.evaluate(m, held, 10)
    assert list(old) == ["ap", "ndcg"] and isinstance(one["coverage"], float) and one["coverage"] == ev["coverage"][2]
    for name in ALL[:-1]:
        assert one[name].shape == (n,) and _same(one[name], ev[name][:, 2])
    assert _same(old["ap"], one["ap"]) and _same(old["ndcg"], one["ndcg"])
    seq1 = model.evaluate(m, held, (10,), metrics=("hit", "ap"))
    assert seq1["hit"].shape == (n, 1) and _same(seq1["hit"][:, 0], one["hit"]) and _same(seq1["ap"][:, 0], one["ap"])
    only = model.evaluate(m, held, [3, 10], metrics=("recall",))
    assert list(only) == ["recall"] and _same(only["recall"], ev["recall"][:, 1:])


def test_evaluate_with_candidates_and_with_negatives():
    model, m, held = _eval_model()
    n, n_item = m.shape
    rng = np.random.default_rng(9)
    cand = sp.csr_matrix(rng.random((n, n_item)) < 0.4, dtype=np.float64)
    ev = model.evaluate(m, held, K, metrics=ALL, candidates=cand)
    _check_against_lists(ev, model.predict(m, 10, candidates=cand), held, n_item)
    ev = model.evaluate(m, held, K, metrics=ALL, negatives=15, seed=7)
    _check_against_lists(ev, model.predict(m, 10, candidates=model.sample_negatives(m, 15, actual=held, seed=7)), held, n_item)
    ok = ~np.isnan(ev["hit"][:, 0])
    assert ok.sum() > 50 and ev["hit"][ok, 2].mean() > ev["hit"][ok, 0].mean()


def _several(model, m, held):
    return {"plain": model.evaluate(m, held, K, metrics=ALL), "neg": model.evaluate(m, held, (2, 5), metrics=ALL, negatives=12, seed=3),
            "scalar": model.evaluate(m, held, 4, metrics=("hit", "coverage", "ndcg"))}


def _worker(rank, ws, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT / "tests"))
    import torch.distributed as dist
    model, m, held = _eval_model()
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        torch.save(_several(model, m, held), os.path.join(out_dir, "h%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_give_the_one_process_result(tmp_path):
    import torch.multiprocessing as mp
    one = _several(*_eval_model())
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        got = torch.load(tmp_path / ("h%d.pt" % r), weights_only=False)
        for key in one:
            assert list(got[key]) == list(one[key])
            for name in one[key]:
                assert _same(np.asarray(got[key][name]), np.asarray(one[key][name])), (r, key, name)


def test_argument_errors():
    model, m, held = _eval_model()
    for bad in ((3, 3), (5, 3), (0, 3), (), (2.5,), 0):
        with pytest.raises(ValueError):
            model.evaluate(m, held, bad, metrics=("hit",))
    with pytest.raises(ValueError):
        model.evaluate(m, held, (5, 3))                      # ... for ap / ndcg alike
    with pytest.raises(_lib.UnsupportedOnDevice):
        model.evaluate(m, held, tuple(range(1, 18)), metrics=("hit",))
    with pytest.raises(ValueError):
        model.evaluate(m, held, 3, metrics=("map",))
    with pytest.raises(ValueError):
        model.evaluate(m, held, (1, 3), metrics=("hit", "map"))
    with pytest.raises(ValueError):
        model.evaluate(m, held[:10], (1, 3), metrics=("hit",))
    from rsparse_amd.metrics import hit_metrics_reference, topk_metrics
    pred, actual = _hand()
    with pytest.raises(ValueError):
        hit_metrics_reference(pred, actual, (1, 7))          # a cutoff beyond k = 6
    with pytest.raises(ValueError):
        hit_metrics_reference(pred, actual[:3], (1,))
    with pytest.raises(ValueError):
        topk_metrics(pred, actual, (1, 3), metrics=("map",))
    with pytest.raises(ValueError):
        topk_metrics(pred, actual, (3, 1))
    with pytest.raises(_lib.UnsupportedOnDevice):
        topk_metrics(np.zeros((2, 20), np.int64), actual[:2], tuple(range(1, 18)))


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_hit_metrics_entry_points():
    lib = _lib.load()
    for name in ("rsparse_hip_hit_metrics", "rsparse_hip_hit_metrics_device"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    header = (ROOT / "include" / "rsparse_wrmf_hip.h").read_text()
    assert "#define RSPARSE_HIP_MAX_CUTOFFS 16" in header and _lib.MAX_CUTOFFS == 16


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _call(lib, form, pred, n, k, p, j, cut, n_cut, outs, seen, n_items):
    hits, first, pr, rc, ht, mr = outs
    args = [_vp(pred), n, k, _vp(p), _vp(j), _vp(cut), n_cut, _vp(hits), _vp(first), _vp(pr), _vp(rc), _vp(ht), _vp(mr), _vp(seen),
            n_items]
    if form == "host":
        return lib.rsparse_hip_hit_metrics(*args)
    # (host pointers: every call here is rejected by the argument checks, or is the n_users = 0 no-op, before device work)
    return lib.rsparse_hip_hit_metrics_device(*args, None)


def test_status_codes_without_device():
    lib = _lib.load()
    pred = np.asfortranarray(np.array([[3, 1], [NA, 2]], dtype=np.int32))   # 2 users x k = 2, column-major
    p, j = np.array([0, 2, 3], dtype=np.int32), np.array([0, 2, 1], dtype=np.int32)
    cut = np.array([1, 2], dtype=np.int32)
    outs = (np.empty((2, 2), np.int32), np.empty(2, np.int32)) + tuple(np.empty((2, 2)) for _ in range(4))
    none = (None,) * 6
    seen = np.empty(5, np.int32)
    asc = lambda *c: np.array(c, dtype=np.int32)
    for form in ("host", "device"):
        call = lambda *a: _call(lib, form, *a)
        assert call(pred, 2, 2, p, j, cut, 2, none, None, 0) == _lib.ERR_INVALID            # every output NULL
        assert call(None, 2, 2, p, j, cut, 2, outs, seen, 5) == _lib.ERR_INVALID
        assert call(pred, 2, 2, None, j, cut, 2, outs, seen, 5) == _lib.ERR_INVALID
        assert call(pred, 2, 2, p, None, cut, 2, outs, seen, 5) == _lib.ERR_INVALID
        assert call(pred, 2, 2, p, j, None, 2, outs, seen, 5) == _lib.ERR_INVALID
        assert call(pred, -1, 2, p, j, cut, 2, outs, seen, 5) == _lib.ERR_INVALID
        assert call(pred, 2, 0, p, j, cut, 2, outs, seen, 5) == _lib.ERR_INVALID
        assert call(pred, 2, 2, p, j, cut, 0, outs, seen, 5) == _lib.ERR_INVALID
        assert call(pred, 2, 2, p, j, asc(2, 1), 2, outs, seen, 5) == _lib.ERR_INVALID      # not ascending
        assert call(pred, 2, 2, p, j, asc(1, 1), 2, outs, seen, 5) == _lib.ERR_INVALID      # ... strictly
        assert call(pred, 2, 2, p, j, asc(0, 1), 2, outs, seen, 5) == _lib.ERR_INVALID      # below 1
        assert call(pred, 2, 2, p, j, asc(1, 3), 2, outs, seen, 5) == _lib.ERR_INVALID      # above k
        assert call(pred, 2, 2, p, j, cut, 2, outs, seen, 0) == _lib.ERR_INVALID            # first_seen without items
        assert call(pred, 2, 2, p, j, cut, 2, none, seen, 0) == _lib.ERR_INVALID
        assert call(pred, 2, 20, p, j, asc(*range(1, 18)), 17, outs, seen, 5) == _lib.ERR_UNSUPPORTED
        assert call(pred, 2, 8193, p, j, cut, 2, outs, seen, 5) == _lib.ERR_UNSUPPORTED
        assert call(pred, 0, 2, p, j, cut, 2, outs, seen, 5) == _lib.OK                      # n_users = 0: a no-op
    assert (seen == NEVER).all()                                                             # ... that the host form initialises
    # the host form checks the dgRMatrix slots
    host = lambda *a: _call(lib, "host", *a)
    assert host(pred, 2, 2, asc(1, 2, 3), j, cut, 2, outs, seen, 5) == _lib.ERR_INVALID     # p[0] != 0
    assert host(pred, 2, 2, asc(0, 2, 1), j, cut, 2, outs, seen, 5) == _lib.ERR_INVALID     # p decreases
    assert host(pred, 2, 2, p, asc(2, 0, 1), cut, 2, outs, seen, 5) == _lib.ERR_INVALID     # j not ascending
    assert host(pred, 2, 2, p, asc(1, 1, 1), cut, 2, outs, seen, 5) == _lib.ERR_INVALID     # ... strictly
    # a valid call gets past every argument check (no device here -> a runtime error), with one output or with all
    assert host(pred, 2, 2, p, j, cut, 2, outs, seen, 5) not in (_lib.ERR_INVALID, _lib.ERR_UNSUPPORTED)
    assert host(pred, 2, 2, p, j, cut, 2, none, seen, 5) not in (_lib.ERR_INVALID, _lib.ERR_UNSUPPORTED)
    assert host(pred, 2, 2, p, j, asc(2), 1, (None, outs[1]) + (None,) * 4, None, 0) not in (_lib.ERR_INVALID, _lib.ERR_UNSUPPORTED)
