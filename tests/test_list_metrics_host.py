"""Beyond-accuracy metrics of the lists (popularity, novelty, exposure, intra-list diversity) without a device: the numpy
definitions `rsparse_amd.metrics.list_metrics_reference` / `list_diversity_reference` on hand-worked lists and against a
position-by-position restatement, the identities that hold for any input, the sum-of-unit-vectors form of the diversity against
the pairwise form, `self_information` and `exposure_summary`, `WRMF.evaluate` with every new metric on the CPU stand-in backend
(which has no `list_metrics` / `list_diversity` and so gets the definitions through the `hasattr` fallback) -- plain,
`candidates=`, `negatives=` and on two gloo ranks --, the argument errors, and the status codes of the new C entry points."""
import ctypes
import math
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import _lib
from test_metrics_abi import NA, _eval_model

ROOT = Path(__file__).resolve().parent.parent
NEW = ("popularity", "novelty", "diversity", "gini", "entropy")
ALL = ("ap", "ndcg", "precision", "recall", "hit", "mrr", "coverage") + NEW
TWO32 = 4294967296.0


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def restated(pred, cutoffs, n_item, item_count, item_info):
    """the integer definition once more, one position at a time in plain Python"""
    n, T = pred.shape[0], len(cutoffs)
    valid = np.zeros((n, T), np.int32)
    cs, isum = np.zeros((n, T), np.int64), np.zeros((n, T), np.int64)
    pop, nov = np.full((n, T), np.nan), np.full((n, T), np.nan)
    expo = np.zeros((T, n_item), np.int32)
    for u in range(n):
        for t, ct in enumerate(cutoffs):
            v = c = s = 0
            for i in range(ct):
                item = int(pred[u, i])
                if 0 <= item < n_item:
                    v += 1
                    c += int(item_count[item])
                    s += int(item_info[item])
                    expo[t, item] += 1
            valid[u, t], cs[u, t], isum[u, t] = v, c, s
            if v:
                pop[u, t] = np.float64(c) / np.float64(v)
                nov[u, t] = np.float64(s) / np.float64(v * 2 ** 32)
    return {"valid": valid, "count_sum": cs, "info_sum": isum, "popularity": pop, "novelty": nov, "exposure": expo}


def restated_diversity(pred, cutoffs, V, c0, c1):
    """the pairwise definition, one pair at a time"""
    n, T = pred.shape[0], len(cutoffs)
    W = V[:, c0:c1].astype(np.float64)
    counted, div = np.zeros((n, T), np.int32), np.full((n, T), np.nan)
    for u in range(n):
        for t, ct in enumerate(cutoffs):
            units = []
            for i in range(ct):
                item = int(pred[u, i])
                if 0 <= item < V.shape[0]:
                    ss = float(np.sum(W[item] * W[item]))
                    if ss > 0 and math.isfinite(ss):
                        units.append(W[item] / np.sqrt(ss))
            m = len(units)
            counted[u, t] = m
            if m >= 2:
                d = [1.0 - float(np.dot(units[i], units[j])) for i in range(m) for j in range(i + 1, m)]
                div[u, t] = float(np.mean(d))
    return counted, div


def s_form(pred, cutoffs, V, c0, c1):
    """what the device computes: 1 - (|S|^2 - m) / (m (m - 1)) with S the sum of the unit vectors"""
    from rsparse_amd.metrics import _unit_rows
    unit, bad, _, _ = _unit_rows(V, c0, c1)
    n, T = pred.shape[0], len(cutoffs)
    div = np.full((n, T), np.nan)
    for u in range(n):
        for t, ct in enumerate(cutoffs):
            it = pred[u, :ct]
            it = it[(it >= 0) & (it < V.shape[0])]
            it = it[~bad[it]]
            m = it.size
            if m >= 2:
                S = unit[it].sum(axis=0)
                div[u, t] = 1.0 - (float(S @ S) - m) / (m * (m - 1.0))
    return div


# ---- hand-worked lists ---------------------------------------------------------------------------------------------------------
def test_hand_worked_lists():
    from rsparse_amd.metrics import exposure_summary, list_metrics_reference
    pred = np.array([[0, 1, 1, -1, 5, 2],                 # a repeat, NA and an item beyond the catalogue
                     [2, 2, 2, 2, 2, 2],                  # one item repeated
                     [9, -7, -1, 4, 3, 3],                # nothing valid
                     [1, 0, 2, 0, 1, 2]], dtype=np.int64)
    cnt = np.array([5, 0, 3], dtype=np.int32)
    info = np.array([1 << 32, 3 << 31, (1 << 40) - 1], dtype=np.int64)      # 1 bit, 1.5 bits, just below 256 bits
    r = list_metrics_reference(pred, (1, 3, 6), 3, cnt, info)
    assert r["valid"].dtype == np.int32 and r["count_sum"].dtype == np.int64 and r["exposure"].dtype == np.int32
    assert r["valid"].tolist() == [[1, 3, 4], [1, 3, 6], [0, 0, 0], [1, 3, 6]]
    assert r["count_sum"].tolist() == [[5, 5, 8], [3, 9, 18], [0, 0, 0], [0, 8, 16]]
    assert r["info_sum"][0].tolist() == [1 << 32, (1 << 32) + (3 << 32), (1 << 32) + (3 << 32) + (1 << 40) - 1]
    assert _same(r["popularity"][0], np.array([5.0, 5 / 3, 2.0])) and _same(r["popularity"][3], np.array([0.0, 8 / 3, 16 / 6]))
    assert _same(r["novelty"][0][:2], np.array([1.0, 4 / 3])) and _same(r["novelty"][1], np.full(3, ((1 << 40) - 1) / TWO32))
    assert np.isnan(r["popularity"][2]).all() and np.isnan(r["novelty"][2]).all()
    assert r["exposure"].tolist() == [[1, 1, 1], [2, 3, 4], [3, 4, 9]]
    full = restated(pred, (1, 3, 6), 3, cnt, info)
    for name in full:
        assert _same(r[name], full[name]), name
    # a table that is not given leaves its outputs out
    assert sorted(list_metrics_reference(pred, (2,), 3)) == ["exposure", "valid"]
    assert sorted(list_metrics_reference(pred, (2,), 3, item_count=cnt)) == ["count_sum", "exposure", "popularity", "valid"]
    s = exposure_summary(r["exposure"])
    assert s["gini"][0] == 0.0 and abs(s["entropy"][0] - np.log2(3.0)) < 1e-15                       # equal exposure
    assert s["gini"][1] == (-2 * 2 + 0 * 3 + 2 * 4) / (3 * 9) and s["gini"][2] == (-2 * 3 + 2 * 9) / (3 * 16)
    z = exposure_summary(np.array([[0, 0, 0], [0, 7, 0]]))
    assert np.isnan(z["gini"][0]) and np.isnan(z["entropy"][0]) and z["gini"][1] == 2 / 3 and z["entropy"][1] == 0.0
    big = exposure_summary(np.full((1, 5), 2 ** 31 - 1, dtype=np.int32))               # (sums beyond int32)
    assert big["gini"][0] == 0.0 and abs(big["entropy"][0] - np.log2(5.0)) < 1e-15


def test_hand_worked_diversity():
    from rsparse_amd.metrics import list_diversity_reference
    V = np.zeros((7, 4), dtype=np.float32)
    V[0, :3] = [1, 0, 0]
    V[1, :3] = [0, 2, 0]
    V[2, :3] = [0, 0, 3]
    V[3, :3] = [5, 0, 0]                                   # the direction of item 0
    V[4, :3] = [1e-30, 0, 0]                               # squares underflow in fp32, not in double: a direction
    V[5, :3] = [np.inf, 0, 0]                              # degenerate; item 6: all zeros, degenerate
    V[:, 3] = 9.0                                          # outside the window
    pred = np.array([[0, 1, 2, -1, 9], [0, 3, 4, 0, 0], [0, 1, 5, 6, -1], [5, 6, -1, 9, 0], [0, 1, 0, 1, 3]])
    r = list_diversity_reference(pred, (2, 3, 5), V, 0, 3)
    assert r["counted"].dtype == np.int32 and r["counted"].tolist() == [[2, 3, 3], [2, 3, 5], [2, 2, 2], [0, 0, 1], [2, 3, 5]]
    assert _same(r["diversity"][0], np.ones(3))                                         # orthogonal items
    assert np.abs(r["diversity"][1]).max() <= 1e-15                                     # one direction
    assert _same(r["diversity"][2], np.ones(3)) and np.isnan(r["diversity"][3]).all()
    # items 0 1 0 1 0-like: of the ten pairs of (a b a b a) six are orthogonal
    assert r["diversity"][4].tolist() == [1.0, 2 / 3, 0.6]
    cnt2, div2 = restated_diversity(pred, (2, 3, 5), V, 0, 3)
    assert _same(r["counted"], cnt2) and np.allclose(r["diversity"], div2, rtol=0, atol=1e-15, equal_nan=True)
    whole = list_diversity_reference(pred, (5,), V)        # the constant column makes every pair similar
    assert (whole["diversity"][0] < 0.6).all() and whole["counted"][3, 0] == 2   # ... and the zero row a direction; inf stays out


def _random_case(seed, n=40, k=30, n_item=50):
    rng = np.random.default_rng(seed)
    pred = rng.integers(0, n_item, (n, k))
    r = rng.random((n, k))
    pred[r < 0.05] = -1
    pred[(r >= 0.05) & (r < 0.08)] = n_item + 3
    pred[(r >= 0.08) & (r < 0.1)] = -7
    pred[3] = -1                                           # an all-invalid row
    pred[4] = 7                                            # one item repeated
    pred[5, 0], pred[5, 1:] = 20, -1                       # a single item
    cnt = rng.integers(0, 1000, n_item).astype(np.int32)
    cnt[:3] = [0, 2 ** 31 - 1, 1]
    return pred, cnt


@pytest.mark.parametrize("cutoffs", [(1,), (30,), (1, 5, 10, 20), (3, 29), tuple(range(2, 34, 2))[:14]])
def test_definition_and_identities_on_random_lists(cutoffs):
    from rsparse_amd.metrics import list_metrics_reference, self_information
    pred, cnt = _random_case(5)
    n_item = cnt.size
    info = self_information(cnt)
    r = list_metrics_reference(pred, cutoffs, n_item, cnt, info)
    full = restated(pred, cutoffs, n_item, cnt, info)
    for name in full:
        assert _same(r[name], full[name]), name
    cut = np.array(cutoffs)
    assert (np.diff(r["valid"], axis=1) >= 0).all() and (r["valid"] <= cut).all()
    assert (np.diff(r["count_sum"], axis=1) >= 0).all() and (np.diff(r["info_sum"], axis=1) >= 0).all()
    assert int(r["exposure"][-1].sum()) == int(r["valid"][:, -1].sum())
    assert np.array_equal(r["exposure"].sum(axis=1), r["valid"].sum(axis=0)) and (np.diff(r["exposure"], axis=0) >= 0).all()
    assert (r["valid"][3] == 0).all() and np.isnan(r["popularity"][3]).all() and np.isnan(r["novelty"][3]).all()
    assert _same(r["popularity"][4], np.full(len(cutoffs), np.float64(cnt[7])))          # one item repeated: its own count
    assert _same(r["novelty"][4], np.full(len(cutoffs), np.float64(info[7]) / TWO32))
    ok = r["valid"] > 0
    assert (r["popularity"][ok] >= cnt.min()).all() and (r["popularity"][ok] <= cnt.max()).all()
    assert (r["novelty"][ok] >= info.min() / TWO32).all() and (r["novelty"][ok] <= info.max() / TWO32).all()
    # positions beyond c_T play no part
    scr = pred.copy()
    scr[:, cut[-1]:] = 0
    r2 = list_metrics_reference(scr, cutoffs, n_item, cnt, info)
    for name in r:
        assert _same(r[name], r2[name]), name


def test_diversity_identities_and_the_sum_form():
    from rsparse_amd.metrics import list_diversity_reference
    rng = np.random.default_rng(8)
    pred, _ = _random_case(6)
    n_item = 50
    cutoffs = (1, 2, 7, 30)
    for dtype, r, c0 in ((np.float32, 10, 0), (np.float64, 3, 1), (np.float32, 64, 1)):
        V = rng.standard_normal((n_item, r + c0 + 1)).astype(dtype)
        V[7] *= 1e-25                                      # tiny factors keep their direction
        V[11] = 0                                          # degenerate
        V[12] = V[13] * (1 + 1e-7)                         # nearly identical items
        got = list_diversity_reference(pred, cutoffs, V, c0, c0 + r)
        cnt2, div2 = restated_diversity(pred, cutoffs, V, c0, c0 + r)
        assert _same(got["counted"], cnt2) and np.array_equal(np.isnan(got["diversity"]), cnt2 < 2)
        assert np.allclose(got["diversity"], div2, rtol=0, atol=1e-14, equal_nan=True)
        assert (np.diff(got["counted"], axis=1) >= 0).all() and (got["counted"] <= np.array(cutoffs)).all()
        assert (got["counted"][3] == 0).all() and (got["counted"][5] == 1).all()
        assert np.isnan(got["diversity"][5]).all() and np.isnan(got["diversity"][:, 0]).all()      # fewer than two items
        assert np.abs(got["diversity"][4, 1:]).max() <= 1e-15                                       # one item repeated
        d = got["diversity"][~np.isnan(got["diversity"])]
        assert (d >= -1e-15).all() and (d <= 2 + 1e-15).all()
        # the form the device uses against the pairwise one: the bound of DESIGN.md 3.23, 2 (2 m + r) 2^-53, is far below this
        s = s_form(pred, cutoffs, V, c0, c0 + r)
        assert np.array_equal(np.isnan(s), np.isnan(got["diversity"]))
        assert np.nanmax(np.abs(s - got["diversity"])) <= 1e-11


def test_sum_form_at_long_lists_of_near_duplicates():
    from rsparse_amd.metrics import list_diversity_reference
    rng = np.random.default_rng(2)
    base = rng.standard_normal(256)
    V = (base[None, :] * (1 + 1e-6 * rng.standard_normal((300, 256)))).astype(np.float32)   # nearly one direction
    V[:50] = rng.standard_normal((50, 256)).astype(np.float32) * 1e-25
    pred = rng.integers(0, 300, (3, 1500))
    pred[1] = pred[1] % 50
    pred[2, ::2] = 17                                      # duplicates
    ref = list_diversity_reference(pred, (2, 700, 1500), V)["diversity"]
    assert np.nanmax(np.abs(s_form(pred, (2, 700, 1500), V, 0, 256) - ref)) <= 1e-11


def test_self_information():
    from rsparse_amd.metrics import INFO_LIMIT, self_information
    cnt = np.array([0, 1, 3, 0], dtype=np.int32)           # shares (c + 1) / 8: 1/8, 2/8, 4/8, 1/8
    assert self_information(cnt).tolist() == [3 << 32, 2 << 32, 1 << 32, 3 << 32]
    assert self_information(cnt).dtype == np.int64
    assert self_information(np.array([5])).tolist() == [0]                               # one item: share 1, no information
    worst = self_information(np.array([0] + [2 ** 31 - 1] * 999, dtype=np.int32))
    assert 0 <= worst.min() and worst.max() < INFO_LIMIT and worst[0] == worst.max() and worst[0] > 40 * 2 ** 32
    z = self_information(np.zeros(1000, dtype=np.int64))
    assert (z == z[0]).all() and abs(z[0] / TWO32 - np.log2(1000.0)) < 1e-9
    for bad in (np.array([1, -1]), np.array([1.0, 2.0]), np.zeros(0, np.int32), np.zeros((2, 2), np.int32)):
        with pytest.raises(ValueError):
            self_information(bad)


def test_summarize_passes_the_exposure_numbers_through():
    from rsparse_amd.metrics import summarize
    ev = {"popularity": np.array([[1.0, 3.0], [np.nan, 5.0]]), "gini": np.array([0.1, 0.2]), "entropy": 3.5, "coverage": 0.5}
    s = summarize(ev)
    assert _same(s["popularity"], np.array([1.0, 4.0])) and s["gini"] is ev["gini"] and s["entropy"] == 3.5 and s["coverage"] == 0.5


# ---- WRMF.evaluate on the CPU stand-in backend ---------------------------------------------------------------------------------
K = (1, 3, 10)


def _popularity(m):
    return np.asarray((sp.csr_matrix(m) != 0).sum(axis=0)).ravel().astype(np.int64)


def _check_against_lists(ev, top, model, pop, cutoffs=K):
    from rsparse_amd.metrics import exposure_summary, list_diversity_reference, list_metrics_reference, self_information
    lists = np.asarray(top)
    n_item = pop.size
    ref = list_metrics_reference(lists, cutoffs, n_item, pop, self_information(pop))
    V = model._V.cpu().numpy()
    div = list_diversity_reference(lists, cutoffs, V, 0, V.shape[1])
    summ = exposure_summary(ref["exposure"])
    assert _same(ev["popularity"], ref["popularity"]) and _same(ev["novelty"], ref["novelty"])
    assert _same(ev["diversity"], div["diversity"])
    assert _same(ev["gini"], summ["gini"]) and _same(ev["entropy"], summ["entropy"])
    return ref


def test_evaluate_every_new_metric_equals_the_definitions_on_predict():
    model, m, held = _eval_model()
    be = model._backend()
    assert not hasattr(be, "list_metrics") and not hasattr(be, "list_diversity")
    n, n_item = m.shape
    pop = _popularity(m)
    ev = model.evaluate(m, held, K, metrics=ALL, item_popularity=pop)
    assert list(ev) == list(ALL)
    assert all(ev[name].shape == (n, 3) and ev[name].dtype == np.float64 for name in ("popularity", "novelty", "diversity"))
    assert ev["gini"].shape == (3,) and ev["entropy"].shape == (3,)
    ref = _check_against_lists(ev, model.predict(m, 10), model, pop)
    assert np.isnan(ev["diversity"][:, 0]).all() and 0 < np.nanmean(ev["diversity"][:, 2]) < 2   # one item has no pair
    assert (ref["valid"][:, 2] > 0).all() and 0 < ev["gini"][2] < 1 and 0 < ev["entropy"][2] <= np.log2(n_item)
    # the old names are what they were without the new ones beside them
    old = model.evaluate(m, held, K, metrics=ALL[:7])
    assert list(old) == list(ALL[:7]) and all(_same(old[name], ev[name]) for name in old)
    # a scalar k: vectors and floats, equal to the one-cutoff column
    one = model.evaluate(m, held, 10, metrics=NEW + ("hit",), item_popularity=pop)
    assert list(one) == ["hit"] + list(NEW) and isinstance(one["gini"], float) and isinstance(one["entropy"], float)
    assert one["gini"] == ev["gini"][2] and one["entropy"] == ev["entropy"][2]
    for name in ("popularity", "novelty", "diversity"):
        assert one[name].shape == (n,) and _same(one[name], ev[name][:, 2])
    only = model.evaluate(m, held, [3, 10], metrics=("diversity",))
    assert list(only) == ["diversity"] and _same(only["diversity"], ev["diversity"][:, 1:])
    only = model.evaluate(m, held, 10, metrics=("entropy",))
    assert list(only) == ["entropy"] and only["entropy"] == ev["entropy"][2]
    only = model.evaluate(m, held, (1, 3, 10), metrics=("novelty",), item_popularity=pop.astype(np.int32))
    assert _same(only["novelty"], ev["novelty"])


def test_evaluate_with_candidates_and_with_negatives():
    model, m, held = _eval_model()
    n, n_item = m.shape
    pop = _popularity(m)
    rng = np.random.default_rng(9)
    cand = sp.csr_matrix(rng.random((n, n_item)) < 0.1, dtype=np.float64)     # some lists come out shorter than 10
    ev = model.evaluate(m, held, K, metrics=ALL, candidates=cand, item_popularity=pop)
    ref = _check_against_lists(ev, model.predict(m, 10, candidates=cand), model, pop)
    assert (ref["valid"][:, 2] < 10).any()
    ev = model.evaluate(m, held, K, metrics=ALL, negatives=15, seed=7, item_popularity=pop)
    _check_against_lists(ev, model.predict(m, 10, candidates=model.sample_negatives(m, 15, actual=held, seed=7)), model, pop)


def _several(model, m, held):
    pop = _popularity(m)
    return {"plain": model.evaluate(m, held, K, metrics=ALL, item_popularity=pop),
            "neg": model.evaluate(m, held, (2, 5), metrics=NEW, negatives=12, seed=3, item_popularity=pop),
            "scalar": model.evaluate(m, held, 4, metrics=("gini", "diversity", "hit"))}


def _worker(rank, ws, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT / "tests"))
    import torch.distributed as dist
    model, m, held = _eval_model()
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        torch.save(_several(model, m, held), os.path.join(out_dir, "l%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_give_the_one_process_result(tmp_path):
    import torch.multiprocessing as mp
    one = _several(*_eval_model())
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        got = torch.load(tmp_path / ("l%d.pt" % r), weights_only=False)
        for key in one:
            assert list(got[key]) == list(one[key])
            for name in one[key]:
                assert _same(np.asarray(got[key][name]), np.asarray(one[key][name])), (r, key, name)


def test_argument_errors():
    from rsparse_amd.metrics import (exposure_summary, list_diversity, list_diversity_reference, list_metrics,
                                     list_metrics_reference)
    model, m, held = _eval_model()
    n_item = m.shape[1]
    pop = _popularity(m)
    for name in ("popularity", "novelty"):
        with pytest.raises(ValueError):
            model.evaluate(m, held, 3, metrics=(name,))                                   # item_popularity is missing
        with pytest.raises(ValueError):
            model.evaluate(m, held, 3, metrics=(name,), item_popularity=pop[:-1])         # ... of the wrong length
        with pytest.raises(ValueError):
            model.evaluate(m, held, 3, metrics=(name,), item_popularity=pop.astype(np.float64))
        with pytest.raises(ValueError):
            model.evaluate(m, held, 3, metrics=(name,), item_popularity=-pop - 1)
    with pytest.raises(ValueError):
        model.evaluate(m, held, (5, 3), metrics=("diversity",))
    with pytest.raises(_lib.UnsupportedOnDevice):
        model.evaluate(m, held, tuple(range(1, 18)), metrics=("gini",))
    with pytest.raises(ValueError):
        model.evaluate(m, held, 3, metrics=("gini", "serendipity"))
    pred = np.array([[0, 1, 2], [2, 1, -1]])
    cnt = np.array([1, 2, 3], dtype=np.int32)
    for fn in (list_metrics_reference, list_metrics):
        with pytest.raises(ValueError):
            fn(pred, (1, 4), 3)                                                           # a cutoff beyond k = 3
        with pytest.raises(ValueError):
            fn(pred, (2, 1), 3)
        with pytest.raises(ValueError):
            fn(pred, (1,), 0)
        with pytest.raises(ValueError):
            fn(pred, (1,), 3, item_count=cnt[:2])
        with pytest.raises(ValueError):
            fn(pred, (1,), 3, item_count=np.array([1, -2, 3]))
        with pytest.raises(ValueError):
            fn(pred, (1,), 3, item_info=np.array([0, 1 << 40, 0], dtype=np.int64))
        with pytest.raises(ValueError):
            fn(pred, (1,), 3, item_info=np.array([0, -1, 0], dtype=np.int64))
        with pytest.raises(TypeError):
            fn(pred.astype(np.float64), (1,), 3)
    with pytest.raises(ValueError):
        list_metrics(pred, (1,), 3, metrics=("popularity",))                              # needs a table that is not given
    with pytest.raises(ValueError):
        list_metrics(pred, (1,), 3, metrics=("hits",))
    V = np.ones((3, 4), dtype=np.float32)
    for fn in (list_diversity_reference, list_diversity):
        with pytest.raises(ValueError):
            fn(pred, (1, 4), V)
        for c0, c1 in ((2, 2), (3, 1), (-1, 2), (0, 5)):
            with pytest.raises(ValueError):
                fn(pred, (1,), V, c0, c1)
        with pytest.raises(ValueError):
            fn(pred, (1,), V.astype(np.float16))
    with pytest.raises(_lib.UnsupportedOnDevice):
        list_diversity(pred, (1,), np.ones((3, 300), dtype=np.float32))
    with pytest.raises(ValueError):
        exposure_summary(np.ones((2, 3)))


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
ENTRIES = ("rsparse_hip_list_metrics", "rsparse_hip_list_metrics_device", "rsparse_hip_item_inv_norms_device",
           "rsparse_hip_item_inv_norms_f64_device", "rsparse_hip_list_diversity_device", "rsparse_hip_list_diversity_f64_device",
           "rsparse_hip_list_diversity", "rsparse_hip_list_diversity_f64")


def test_library_exports_the_new_entry_points():
    lib = _lib.load()
    header = (ROOT / "include" / "rsparse_wrmf_hip.h").read_text()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and ("int %s(" % name) in header


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_status_codes_of_list_metrics_without_device():
    lib = _lib.load()
    pred = np.asfortranarray(np.array([[3, 1], [NA, 2]], dtype=np.int32))   # 2 users x k = 2, column-major
    cut = np.array([1, 2], dtype=np.int32)
    cnt, info = np.array([1, 2, 3], dtype=np.int32), np.array([0, 1 << 32, (1 << 40) - 1], dtype=np.int64)
    outs = (np.empty((2, 2), np.int32), np.empty((2, 2), np.int64), np.empty((2, 2), np.int64), np.empty((2, 2)), np.empty((2, 2)))
    none = (None,) * 5
    expo = np.full((3, 2), 77, dtype=np.int32)
    asc = lambda *c: np.array(c, dtype=np.int32)

    def call(form, pred, n, k, cut, n_cut, cnt, info, n_items, outs, expo):
        args = [_vp(pred), n, k, _vp(cut), n_cut, _vp(cnt), _vp(info), n_items] + [_vp(o) for o in outs] + [_vp(expo)]
        # (host pointers: every device-form call here is rejected by the argument checks, or is the n_users = 0 no-op)
        return lib.rsparse_hip_list_metrics(*args) if form == "host" else lib.rsparse_hip_list_metrics_device(*args, None)
    for form in ("host", "device"):
        c = lambda *a: call(form, *a)
        assert c(pred, 2, 2, cut, 2, cnt, info, 3, none, None) == _lib.ERR_INVALID              # every output NULL
        assert c(None, 2, 2, cut, 2, cnt, info, 3, outs, expo) == _lib.ERR_INVALID
        assert c(pred, 2, 2, None, 2, cnt, info, 3, outs, expo) == _lib.ERR_INVALID
        assert c(pred, 2, 2, cut, 2, None, info, 3, outs, expo) == _lib.ERR_INVALID              # count_sum without its table
        assert c(pred, 2, 2, cut, 2, cnt, None, 3, outs, expo) == _lib.ERR_INVALID               # novelty without its table
        assert c(pred, 2, 2, cut, 2, None, info, 3, (None, None, None, outs[3], None), None) == _lib.ERR_INVALID
        assert c(pred, -1, 2, cut, 2, cnt, info, 3, outs, expo) == _lib.ERR_INVALID
        assert c(pred, 2, 0, cut, 2, cnt, info, 3, outs, expo) == _lib.ERR_INVALID
        assert c(pred, 2, 2, cut, 0, cnt, info, 3, outs, expo) == _lib.ERR_INVALID
        assert c(pred, 2, 2, asc(2, 1), 2, cnt, info, 3, outs, expo) == _lib.ERR_INVALID         # not ascending
        assert c(pred, 2, 2, asc(1, 1), 2, cnt, info, 3, outs, expo) == _lib.ERR_INVALID         # ... strictly
        assert c(pred, 2, 2, asc(0, 1), 2, cnt, info, 3, outs, expo) == _lib.ERR_INVALID         # below 1
        assert c(pred, 2, 2, asc(1, 3), 2, cnt, info, 3, outs, expo) == _lib.ERR_INVALID         # above k
        assert c(pred, 2, 2, cut, 2, cnt, info, 0, outs, expo) == _lib.ERR_INVALID               # no items
        assert c(pred, 2, 20, asc(*range(1, 18)), 17, cnt, info, 3, outs, expo) == _lib.ERR_UNSUPPORTED
        assert c(pred, 2, 8193, cut, 2, cnt, info, 3, outs, expo) == _lib.ERR_UNSUPPORTED
        assert c(pred, 0, 2, cut, 2, cnt, info, 3, outs, expo) == _lib.OK                        # n_users = 0: a no-op
    assert (expo == 0).all()                                                                     # ... that the host form zeroes
    host = lambda *a: call("host", *a)
    # the host form checks the ranges of the tables
    assert host(pred, 2, 2, cut, 2, np.array([1, -1, 3], np.int32), info, 3, outs, expo) == _lib.ERR_INVALID
    assert host(pred, 2, 2, cut, 2, cnt, np.array([0, -1, 0], np.int64), 3, outs, expo) == _lib.ERR_INVALID
    assert host(pred, 2, 2, cut, 2, cnt, np.array([0, 1 << 40, 0], np.int64), 3, outs, expo) == _lib.ERR_INVALID
    # a valid call gets past every argument check (no device here -> a runtime error), with one output or with all
    ok = lambda rc: rc not in (_lib.ERR_INVALID, _lib.ERR_UNSUPPORTED)
    assert ok(host(pred, 2, 2, cut, 2, cnt, info, 3, outs, expo))
    assert ok(host(pred, 2, 2, cut, 2, None, None, 3, none, expo))
    assert ok(host(pred, 2, 2, asc(2), 1, None, None, 3, (outs[0],) + (None,) * 4, None))
    assert ok(host(pred, 2, 2, cut, 2, cnt, None, 3, (None, None, None, outs[3], None), None))


def test_status_codes_of_list_diversity_without_device():
    lib = _lib.load()
    pred = np.asfortranarray(np.array([[3, 1], [NA, 2]], dtype=np.int32))
    cut = np.array([1, 2], dtype=np.int32)
    asc = lambda *c: np.array(c, dtype=np.int32)
    counted, div, inv = np.empty((2, 2), np.int32), np.empty((2, 2)), np.empty(3)
    for sfx, dt in (("", np.float32), ("_f64", np.float64)):
        V = np.ones((3, 300), dtype=dt)
        norms = getattr(lib, "rsparse_hip_item_inv_norms%s_device" % sfx)
        assert norms(_vp(V), 3, 300, 0, 0, _vp(inv), None) == _lib.ERR_INVALID                   # an empty window
        assert norms(_vp(V), 3, 300, 2, 1, _vp(inv), None) == _lib.ERR_INVALID
        assert norms(_vp(V), 3, 300, -1, 4, _vp(inv), None) == _lib.ERR_INVALID
        assert norms(_vp(V), 3, 300, 0, 301, _vp(inv), None) == _lib.ERR_INVALID                 # beyond ld
        assert norms(_vp(V), -1, 300, 0, 4, _vp(inv), None) == _lib.ERR_INVALID
        assert norms(None, 3, 300, 0, 4, _vp(inv), None) == _lib.ERR_INVALID
        assert norms(_vp(V), 3, 300, 0, 4, None, None) == _lib.ERR_INVALID
        assert norms(_vp(V), 3, 300, 0, 257, _vp(inv), None) == _lib.ERR_UNSUPPORTED             # more than 256 coordinates
        assert norms(_vp(V), 0, 300, 0, 4, _vp(inv), None) == _lib.OK                            # no items: a no-op

        def call(form, pred, n, k, cut, n_cut, V, n_items, ld, c0, c1, inv, counted, div):
            head = [_vp(pred), n, k, _vp(cut), n_cut, _vp(V), n_items, ld, c0, c1]
            if form == "host":
                return getattr(lib, "rsparse_hip_list_diversity" + sfx)(*head, _vp(counted), _vp(div))
            return getattr(lib, "rsparse_hip_list_diversity%s_device" % sfx)(*head, _vp(inv), _vp(counted), _vp(div), None)
        for form in ("host", "device"):
            c = lambda *a: call(form, *a)
            assert c(pred, 2, 2, cut, 2, V, 3, 300, 0, 4, inv, None, None) == _lib.ERR_INVALID   # every output NULL
            assert c(None, 2, 2, cut, 2, V, 3, 300, 0, 4, inv, counted, div) == _lib.ERR_INVALID
            assert c(pred, 2, 2, None, 2, V, 3, 300, 0, 4, inv, counted, div) == _lib.ERR_INVALID
            assert c(pred, 2, 2, cut, 2, None, 3, 300, 0, 4, inv, counted, div) == _lib.ERR_INVALID
            assert c(pred, -1, 2, cut, 2, V, 3, 300, 0, 4, inv, counted, div) == _lib.ERR_INVALID
            assert c(pred, 2, 0, cut, 2, V, 3, 300, 0, 4, inv, counted, div) == _lib.ERR_INVALID
            assert c(pred, 2, 2, cut, 0, V, 3, 300, 0, 4, inv, counted, div) == _lib.ERR_INVALID
            assert c(pred, 2, 2, asc(2, 1), 2, V, 3, 300, 0, 4, inv, counted, div) == _lib.ERR_INVALID
            assert c(pred, 2, 2, asc(1, 3), 2, V, 3, 300, 0, 4, inv, counted, div) == _lib.ERR_INVALID
            assert c(pred, 2, 2, cut, 2, V, 0, 300, 0, 4, inv, counted, div) == _lib.ERR_INVALID  # no items
            assert c(pred, 2, 2, cut, 2, V, 3, 300, 4, 4, inv, counted, div) == _lib.ERR_INVALID
            assert c(pred, 2, 2, cut, 2, V, 3, 300, -1, 4, inv, counted, div) == _lib.ERR_INVALID
            assert c(pred, 2, 2, cut, 2, V, 3, 300, 0, 301, inv, counted, div) == _lib.ERR_INVALID
            assert c(pred, 2, 2, cut, 2, V, 3, 300, 0, 257, inv, counted, div) == _lib.ERR_UNSUPPORTED
            assert c(pred, 2, 20, asc(*range(1, 18)), 17, V, 3, 300, 0, 4, inv, counted, div) == _lib.ERR_UNSUPPORTED
            assert c(pred, 2, 8193, cut, 2, V, 3, 300, 0, 4, inv, counted, div) == _lib.ERR_UNSUPPORTED
            assert c(pred, 0, 2, cut, 2, V, 3, 300, 0, 4, inv, counted, div) == _lib.OK          # n_users = 0: a no-op
        assert call("device", pred, 2, 2, cut, 2, V, 3, 300, 0, 4, None, counted, div) == _lib.ERR_INVALID   # no norms
        # a valid host call gets past every argument check (no device here -> a runtime error)
        ok = lambda rc: rc not in (_lib.ERR_INVALID, _lib.ERR_UNSUPPORTED)
        assert ok(call("host", pred, 2, 2, cut, 2, V, 3, 300, 1, 257, inv, counted, div))
        assert ok(call("host", pred, 2, 2, asc(2), 1, V, 3, 300, 0, 4, inv, None, div))
