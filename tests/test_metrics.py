"""Ranking metrics on the MI355X: ap_k / ndcg_k (R/metrics.R:31-127) from wrmf_metrics.hip against the reference's own cases
(tests/testthat/test-metrics.R), against the numpy restatement of tests/test_metrics_abi.py on randomised lists (row lengths
around k and beyond the kernel's LDS cap, NA / repeated / out-of-range predictions, stored zeros, negative relevances, all-equal
rows, ties at the kk-th value), the host form against the device form, and `WRMF.evaluate` against ap_k / ndcg_k of `predict`
on the movielens fixture."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from test_metrics_abi import NA, ref_metrics, to_r

pytestmark = pytest.mark.gpu


def _close(got, ref, tol=1e-12):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == np.float64 and got.shape == ref.shape
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True)
    err = np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))
    assert err.max(initial=0.0) <= tol, (float(err.max()), int(np.flatnonzero(fin)[err.argmax()]))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- the reference's cases ---------------------------------------------------------------------------------------------------
def test_reference_cases():
    """tests/testthat/test-metrics.R:3-44 (its 1-based predictions 5, 7, 9, 2 are 4, 6, 8, 1 here)"""
    from rsparse_amd.metrics import ap_k, ndcg_k
    pred = np.array([[4, 6, 8, 1]])
    actual = sp.csr_matrix(np.array([[0, 0, 0, 0, 1, 0, 1, 0, 1, 0]], dtype=float))
    assert ap_k(pred, actual)[0] == 1.0
    a2 = actual.tolil(); a2[0, 9] = 1
    a3 = actual.tolil(); a3[0, 0] = 1
    ap2, ap3 = ap_k(pred, a2)[0], ap_k(pred, a3)[0]
    assert ap2 < 1 and ap2 == ap3 == 0.9375
    actual = sp.csr_matrix(np.array([[0, 0, 0, 0, 10, 0, 8, 0, 4, 0]], dtype=float))
    assert ndcg_k(pred, actual)[0] == 1.0
    n2 = actual.tolil(); n2[0, 4] = 1
    n3 = actual.tolil(); n3[0, 6] = 1                               # (actual_3 = actual, test-metrics.R:41)
    nd2, nd3 = ndcg_k(pred, n2)[0], ndcg_k(pred, n3)[0]
    assert nd2 < 1 and nd3 > nd2
    _close([nd2, nd3], [ref_metrics(to_r(pred), sp.csr_matrix(a))[1][0] for a in (n2, n3)])


# ---- randomised cases --------------------------------------------------------------------------------------------------------
N_ITEMS = 20000


def _case(k, seed):
    """users with rows of length 0, 1, below k, k, above k, and beyond the kernel's LDS cap of 512; per length, relevances drawn
    four ways: continuous with negatives, small integers (stored zeros, ties at the kk-th value), all equal, all zero"""
    rng = np.random.default_rng(seed)
    lens = sorted({0, 1, max(1, k // 2), k, k + 3, 600, 2000, 9000 if k > 2000 else 700})
    rows, cols, vals, preds = [], [], [], []
    u = 0
    for L in lens:
        for mode in range(4):
            c = np.sort(rng.choice(N_ITEMS, size=L, replace=False))
            if mode == 0:
                v = rng.standard_normal(L)
            elif mode == 1:
                v = rng.integers(-1, 4, L).astype(float)
            elif mode == 2:
                v = np.full(L, 2.5)
            else:
                v = np.zeros(L)
            rows.append(np.full(L, u)); cols.append(c); vals.append(v)
            # predictions: hits from the row, random items, NA, out-of-range, repeats
            pr = rng.integers(0, N_ITEMS, k)
            if L:
                hit = rng.random(k) < 0.5
                pr[hit] = rng.choice(c, size=int(hit.sum()))
            r = rng.random(k)
            pr[r < 0.05] = -1
            pr[(r >= 0.05) & (r < 0.08)] = N_ITEMS + 7
            pr[(r >= 0.08) & (r < 0.10)] = 2 ** 31 - 2
            if k > 3:
                pr[3] = pr[1]
            preds.append(pr)
            u += 1
    return np.stack(preds), _csr(rows, cols, vals, u)


def _csr(rows, cols, vals, n):
    """canonical CSR built from its slots, so that every zero stays a stored entry"""
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    counts = np.bincount(r, minlength=n)
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    order = np.lexsort((c, r))
    return sp.csr_matrix((v[order], c[order].astype(np.int32), indptr), shape=(n, N_ITEMS))


@pytest.mark.parametrize("k", [1, 7, 64, 65, 100, 256, 257, 1000, 8192])
def test_random_lists_match_the_restatement(k):
    from rsparse_amd.metrics import ap_k, ndcg_k, ranking_metrics
    pred, actual = _case(k, 100 + k)
    assert (actual.data == 0).any() and (np.diff(actual.indptr) > 512).any()
    ap_ref, nd_ref = ref_metrics(to_r(pred), actual)
    ap, nd = ranking_metrics(pred, actual)
    _close(ap, ap_ref)
    _close(nd, nd_ref)
    assert np.isnan(ap[np.diff(actual.indptr) == 0]).all() and (nd[np.diff(actual.indptr) == 0] == 0).all()
    # one metric at a time is the same computation; a second call repeats the bits
    assert _same_bits(ap_k(pred, actual), ap) and _same_bits(ndcg_k(pred, actual), nd)
    ap2, nd2 = ranking_metrics(pred, actual)
    assert _same_bits(ap2, ap) and _same_bits(nd2, nd)


@pytest.mark.parametrize("k", [10, 257, 8192])
def test_host_form_equals_device_form(k):
    from rsparse_amd import _lib
    from rsparse_amd.engine import HipBackend
    from rsparse_amd.metrics import ranking_metrics
    pred, actual = _case(k, 7 + k)
    ap_h, nd_h = ranking_metrics(pred, actual)
    be = HipBackend()
    res = be.to_device(to_r(pred), torch.int32)                      # row-major, as top_product writes it
    ap_d, nd_d = be.ranking_metrics(res, be.to_device(actual.indptr, torch.int32), be.to_device(actual.indices, torch.int32),
                                    be.to_device(actual.data, torch.float64))
    assert _same_bits(ap_d.cpu().numpy(), ap_h) and _same_bits(nd_d.cpu().numpy(), nd_h)
    ap_only, none = be.ranking_metrics(res, be.to_device(actual.indptr, torch.int32),
                                       be.to_device(actual.indices, torch.int32), None, True, False)
    assert none is None and _same_bits(ap_only.cpu().numpy(), ap_h)
    # the C host form directly, R's column-major matrix
    lib = _lib.load()
    p1 = np.asfortranarray(to_r(pred))
    ap_c, nd_c = np.empty(pred.shape[0]), np.empty(pred.shape[0])
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _lib.check(lib.rsparse_hip_ranking_metrics(vp(p1), pred.shape[0], k, vp(actual.indptr), vp(actual.indices),
                                               vp(actual.data), vp(ap_c), vp(nd_c)))
    assert _same_bits(ap_c, ap_h) and _same_bits(nd_c, nd_h)


def test_duplicates_and_unsorted_input_are_canonicalised():
    from rsparse_amd.metrics import ranking_metrics
    rows = np.array([0, 0, 0, 1, 1, 2])
    cols = np.array([5, 2, 5, 9, 1, 3])
    vals = np.array([1.0, 0.0, 2.0, -1.0, 4.0, 0.0])                 # (0, 5) twice: summed to 3; stored zeros stay
    actual = sp.coo_matrix((vals, (rows, cols)), shape=(3, 12))
    pred = np.array([[5, 2, 2], [1, 9, -1], [3, NA, 40]])
    canon = sp.csr_matrix((np.array([0.0, 3.0, 4.0, -1.0, 0.0]), np.array([2, 5, 1, 9, 3]), np.array([0, 2, 4, 5])),
                          shape=(3, 12))
    ap_ref, nd_ref = ref_metrics(to_r(pred), canon)
    ap, nd = ranking_metrics(pred, actual)
    _close(ap, ap_ref)
    _close(nd, nd_ref)
    assert ap[2] == 1.0 and np.isnan(nd[2])                          # a hit of relevance 0, idcg 0


# ---- WRMF.evaluate end to end ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["float", "double"])
@pytest.mark.parametrize("k", [10, 1500])
def test_evaluate_equals_metrics_of_predict_on_movielens(ml_train, precision, k):
    from rsparse_amd import WRMF
    from rsparse_amd.metrics import ap_k, ndcg_k
    n_user, n_item, tp, ti, tx = ml_train
    full = sp.csc_matrix((tx, ti, tp), shape=(n_user, n_item)).tocsr()
    rng = np.random.default_rng(21)
    coo = full.tocoo()
    out = rng.random(coo.nnz) < 0.2                                   # a fifth of every user's ratings held out
    train = sp.csr_matrix((coo.data[~out], (coo.row[~out], coo.col[~out])), shape=full.shape)
    held = sp.csr_matrix((coo.data[out], (coo.row[out], coo.col[out])), shape=full.shape)
    m = WRMF(rank=10, lambda_=0.1, feedback="implicit", solver="conjugate_gradient", precision=precision, rng=1)
    m.fit_transform(train, n_iter=3, convergence_tol=-1)
    got = m.evaluate(train, held, k)
    top = m.predict(train, k)
    assert _same_bits(got["ap"], ap_k(top, held)) and _same_bits(got["ndcg"], ndcg_k(top, held))
    ap_ref, nd_ref = ref_metrics(to_r(top), held)
    _close(got["ap"], ap_ref)
    _close(got["ndcg"], nd_ref)
    ok = ~np.isnan(got["ap"])
    assert ok.sum() > 800 and (got["ap"][ok] >= 0).all() and (got["ap"][ok] <= 1).all()
    assert got["ap"][ok].mean() > 0.01                                # the model ranks held-out items above chance
    only = m.evaluate(train, held, k, metrics=("ndcg",))
    assert set(only) == {"ndcg"} and _same_bits(only["ndcg"], got["ndcg"])
