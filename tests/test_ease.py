"""EASE on the device (wrmf_ease.hip behind rsparse_hip_item_gram_device / rsparse_hip_ease_recommend_device) against the numpy
definitions of rsparse_amd/ease.py: the Gram rows and the lists bit for bit, the inverse by its residual."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import load_movielens
from rsparse_amd import EASE, _lib
from rsparse_amd.ease import (cholesky_inverse_blocked, ease_gram_reference, ease_recommend_reference, ease_weights_reference, key_scores,
                              spd_inverse)
from rsparse_amd.itemknn import canonical_pattern

pytestmark = pytest.mark.gpu

SPAN, CAND = _lib.KNN_SPAN, _lib.KNN_LDS_CAND
CHUNK, AHEAD = _lib.EASE_CHUNK, _lib.EASE_AHEAD
TILE = {np.float32: _lib.EASE_TILE_BYTES // 4, np.float64: _lib.EASE_TILE_BYTES // 8}   # columns of a workgroup's tile
NA = -2147483648


@functools.lru_cache(maxsize=None)
def backend():
    from rsparse_amd.engine import HipBackend
    return HipBackend()


# ---- the problems (those of the ItemKNN tests, rebuilt) -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted():
    """160 users x 300 items of rising popularity.  Rows of 1, 63, 64, 65 and 257 items (users 0 .. 4); columns of 0, 1, 64, 65 and
    2 SPAN + 1 users (items 299 .. 295); items 10 and 11 with the same users."""
    rng = np.random.default_rng(7)
    n_users, n_items = 160, 300
    d = rng.random((n_users, n_items)) < np.linspace(0.02, 0.25, n_items)[None, :]
    d[:, 11] = d[:, 10]
    free = np.setdiff1d(np.arange(295), (10, 11))
    d[:5] = False
    for u, length in enumerate((1, 63, 64, 65, 257)):
        d[u, rng.choice(free, size=length, replace=False)] = True
    for item, users in ((299, 0), (298, 1), (297, 64), (296, 65), (295, 2 * SPAN + 1)):
        d[:, item] = False
        d[5 + rng.choice(n_users - 5, size=users, replace=False), item] = True
    assert d[:5].sum(axis=1).tolist() == [1, 63, 64, 65, 257]
    assert d[:, 295:].sum(axis=0).tolist() == [2 * SPAN + 1, 65, 64, 1, 0] and (d[:, 10] == d[:, 11]).all() and d[:, 10].any()
    return sp.csr_matrix(d.astype(np.float64))


@functools.lru_cache(maxsize=None)
def small(n_items):
    rng = np.random.default_rng(100 + n_items)
    d = rng.random((40, n_items)) < np.linspace(0.1, 0.6, n_items)[None, :]
    d[0] = True                                                           # a user of every item
    return sp.csr_matrix(d.astype(np.float64))


@functools.lru_cache(maxsize=None)
def movielens_csr():
    n_user, n_item, p, i, x = load_movielens()
    m = sp.csc_matrix((np.ones_like(x), i, p), shape=(n_user, n_item)).tocsr()
    m.sort_indices()
    return m


# ---- Gram ------------------------------------------------------------------------------------------------------------------------
def device_gram(x, lambda_, item0=0, item1=None, ws_rows=0):
    be = backend()
    m = canonical_pattern(x)
    n_users, n_items = m.shape
    up, uj = be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32)
    ip, iu, _ = be.transpose_csc(n_items, n_users, up, uj, torch.ones(int(uj.numel()), dtype=torch.float32, device=uj.device))
    return be.item_gram(ip, iu, up, uj, n_users, n_items, lambda_, item0=item0, item1=item1, ws_rows=ws_rows)


@pytest.mark.parametrize("lambda_", [0.0, 0.5])
@pytest.mark.parametrize("name", ["planted", "small1", "small2", "small65", "small300"])
def test_gram_rows_equal_the_definition(name, lambda_):
    x = planted() if name == "planted" else small(int(name[5:]))
    ref = ease_gram_reference(x, lambda_)
    assert np.array_equal(device_gram(x, lambda_).cpu().numpy(), ref)


@pytest.mark.parametrize("ws_rows", [1, 2, 3])
def test_gram_batches_ranges_and_repeats(ws_rows):
    x = planted()
    ref = ease_gram_reference(x, 0.5)
    assert np.array_equal(device_gram(x, 0.5, ws_rows=ws_rows).cpu().numpy(), ref)
    assert np.array_equal(device_gram(x, 0.5, 290, 300, ws_rows=ws_rows).cpu().numpy(), ref[290:300])
    assert device_gram(x, 0.5, 7, 7).shape == (0, 300)
    assert np.array_equal(device_gram(small(2), 0.0).cpu().numpy(), ease_gram_reference(small(2), 0.0))   # a small call behind a larger one
    # rows written at a stride: what lies between them is left alone
    be = backend()
    out = torch.full((300, 320), -1.0, dtype=torch.float64, device=be.device)
    m = canonical_pattern(x)
    up, uj = be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32)
    ip, iu, _ = be.transpose_csc(300, 160, up, uj, torch.ones(int(uj.numel()), dtype=torch.float32, device=uj.device))
    be.item_gram(ip, iu, up, uj, 160, 300, 0.5, ws_rows=ws_rows, out=out[:, :300])
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :300], ref) and (got[:, 300:] == -1).all()


# ---- inverse ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture_inverse(lambda_):
    """-> (A, P_ref, r_ref): the Gram matrix of the 900-user split, numpy's inverse and its residual max |P A - I|"""
    A = ease_gram_reference(movielens_csr()[:900], lambda_)
    P = np.linalg.inv(A)
    return A, P, np.abs(P @ A - np.eye(A.shape[0])).max()


@pytest.mark.parametrize("lambda_", [0.5, 500.0])
def test_inverse_residual(lambda_):
    """r_dev <= 32 r_ref: both errors grow as cond n eps; the margin covers the summation order of a blocked factorisation.
    Observed: profiles/ease/README.md."""
    A, _, r_ref = fixture_inverse(lambda_)
    d_A = device_gram(movielens_csr()[:900], lambda_)
    assert np.array_equal(d_A.cpu().numpy(), A)
    P = spd_inverse(d_A).cpu().numpy()
    r_dev = np.abs(P @ A - np.eye(A.shape[0])).max()
    print("lambda %g: r_dev %.3g, r_ref %.3g, ratio %.2f, factorised on the %s" % (lambda_, r_dev, r_ref, r_dev / r_ref,
                                                                                "host" if spd_inverse.on_host else "device"))
    assert r_dev <= 32 * r_ref


def test_inverse_in_blocks_of_right_hand_sides():
    """the path of a catalogue beyond ease.INVERSE_BLOCK items, at a block that cuts the fixture into four uneven pieces: the
    same bound"""
    A, _, r_ref = fixture_inverse(500.0)
    L = torch.linalg.cholesky(backend().to_device(A, torch.float64))
    P = cholesky_inverse_blocked(L, block=512).cpu().numpy()
    r_dev = np.abs(P @ A - np.eye(A.shape[0])).max()
    print("blocked: r_dev %.3g, r_ref %.3g, ratio %.2f" % (r_dev, r_ref, r_dev / r_ref))
    assert r_dev <= 32 * r_ref


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("lambda_", [0.5, 500.0])
def test_fitted_weights(lambda_, precision):
    """|B_dev - B_ref| entry by entry.  With R = P A - I, P - inv(A) = R inv(A), so an entry of either inverse is off by at most
    e = n r max|P| (r its residual: r_ref, and at most 32 r_ref on the device by the test above); B_ij = -P_ij / P_jj then moves by
    (e + |B_ij| e) / P_jj to first order, doubled here for the second-order term of the denominator: tol = 2 (33 n r_ref max|P|)
    (1 + |B_ref|) / P_jj.  precision "float" adds the one rounding of B into float32, 2^-24 (|B_ref| + tol), and 2^-150 where it
    underflows."""
    A, P, r_ref = fixture_inverse(lambda_)
    B_ref = ease_weights_reference(A)
    n = A.shape[0]
    tol = 2 * (33 * n * r_ref * np.abs(P).max()) * (1 + np.abs(B_ref)) / np.diag(P)[None, :]
    m = EASE(lambda_, precision=precision, backend=backend()).fit(movielens_csr()[:900])
    B = m.B
    assert B.dtype == (np.float32 if precision == "float" else np.float64) and B.shape == (n, n)
    assert (np.diag(B) == 0).all() and not np.signbit(np.diag(B)).any()
    assert np.array_equal(m.item_count, np.diag(A) - lambda_)
    if precision == "float":
        tol = tol + 2.0 ** -24 * (np.abs(B_ref) + tol) + 2.0 ** -150
    err = np.abs(B.astype(np.float64) - B_ref)
    print("lambda %g %s: max err %.3g, max err / tol %.3g" % (lambda_, precision, err.max(), (err / tol).max()))
    assert (err <= tol).all()


def test_singular_gram_is_a_numeric_error():
    with pytest.raises(_lib.RsparseHipError) as e:
        EASE(0.0, backend=backend()).fit(planted())                        # items 10 and 11 have the same users, item 299 none
    assert e.value.code == _lib.ERR_NUMERIC and "lambda = 0" in str(e.value)


# ---- lists -----------------------------------------------------------------------------------------------------------------------
def padded(B):
    """B as the (n, ld) device tensor the kernel reads: rows at multiples of 256 bytes, zeros beyond n"""
    n = B.shape[0]
    elems = 256 // B.dtype.itemsize
    t = torch.zeros((n, (n + elems - 1) // elems * elems), dtype=torch.from_numpy(B[:0]).dtype, device=backend().device)
    t[:, :n] = torch.from_numpy(B)
    return t


def device_lists(x, B, k, nr=None, excl=(), ws_rows=0, d_B=None):
    """-> (items (n, k) int64 0-based with -1, scores float64 with 0 in the padding): the layout of ease_recommend_reference"""
    be = backend()
    m = canonical_pattern(x, B.shape[0])
    nr_p = nr_j = None
    if nr is not None and nr.nnz:
        nr = sp.csr_matrix(nr)
        nr_p, nr_j = be.to_device(nr.indptr, torch.int32), be.to_device(nr.indices, torch.int32)
    d_ex = be.to_device(np.asarray(excl), torch.int32) if len(excl) else None
    res, keys = be.ease_recommend(be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32),
                                  padded(B) if d_B is None else d_B, B.shape[0], k, nr_p, nr_j, d_ex, ws_rows=ws_rows)
    res, keys = res.cpu().numpy().astype(np.int64), keys.cpu().numpy()
    assert (keys[res == NA] == 0).all()
    return np.where(res == NA, -1, res - 1), np.where(res == NA, 0.0, key_scores(keys))


def same_lists(got, ref):
    return np.array_equal(got[0], ref[0]) and np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64))


def weights(n_items, dtype, seed=0):
    B = np.random.default_rng(seed + n_items).standard_normal((n_items, n_items)).astype(dtype)
    np.fill_diagonal(B, 0.0)
    return B


def users(n_items, seed=1):
    """rows of 0, 1, AHEAD - 1, AHEAD, AHEAD + 1, 2 AHEAD + 3, CHUNK + 1 and all items (capped at n_items)"""
    rng = np.random.default_rng(seed)
    lens = [min(l, n_items) for l in (0, 1, AHEAD - 1, AHEAD, AHEAD + 1, 2 * AHEAD + 3, CHUNK + 1, n_items)]
    d = np.zeros((len(lens), n_items), dtype=bool)
    for u, l in enumerate(lens):
        d[u, rng.choice(n_items, size=l, replace=False)] = True
    return sp.csr_matrix(d.astype(np.float64))


SHAPES = sorted({1, 3, 4, 5} | {t + d for t in TILE.values() for d in (-1, 0, 1)})


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_items", SHAPES)
def test_lists_equal_the_definition(n_items, dtype):
    B, x = weights(n_items, dtype), users(n_items)
    k = min(10, n_items + 2)                                                # (the smallest shapes: k above the items)
    assert same_lists(device_lists(x, B, k), ease_recommend_reference(x, B, k))
    ref = ease_recommend_reference(x, B, k, x, (0,))
    assert same_lists(device_lists(x, B, k, x, (0,)), ref)
    assert (ref[0][-1] == -1).all()                                         # the user of every item has nothing left


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rows_beyond_the_candidate_buffer(dtype):
    """CAND + 100 items: every unmasked cell of a row is a candidate, so every row takes the select's radix fallback; the user without
    a history is the row of ties (every score +0.0)."""
    rng = np.random.default_rng(9)
    n_items = CAND + 100
    d = np.zeros((4, n_items), dtype=bool)
    d[0] = True
    d[1, rng.choice(n_items, size=2000, replace=False)] = True
    d[2, rng.choice(n_items, size=50, replace=False)] = True
    x, B = sp.csr_matrix(d.astype(np.float64)), weights(n_items, dtype)
    d_B = padded(B)
    for k, nr, excl in ((10, None, ()), (1024, None, (3, 4000)), (10, x, (0, 1, 5))):
        got, ref = device_lists(x, B, k, nr, excl, d_B=d_B), ease_recommend_reference(x, B, k, nr, excl)
        assert same_lists(got, ref)
    assert np.array_equal(got[0][3], [2, 3, 4, 6, 7, 8, 9, 10, 11, 12]) and (got[1][3] == 0).all() and (got[0][0] == -1).all()
    # k above the admissible count: one row keeps 3 items
    nr = sp.csr_matrix(np.r_[np.ones((1, n_items)), np.zeros((3, n_items))])
    nr[0, [7, 100, 4195]] = 0
    nr.eliminate_zeros()
    got = device_lists(x, B, 6, nr, d_B=d_B)
    assert same_lists(got, ease_recommend_reference(x, B, 6, nr)) and sorted(got[0][0][:3]) == [7, 100, 4195] and (got[0][0][3:] == -1).all()


@pytest.mark.parametrize("ws_rows", [1, 2, 3])
def test_batches_repeats_and_a_small_call_behind_a_larger_one(ws_rows):
    n_items = TILE[np.float32] + 1
    B, x = weights(n_items, np.float32), users(n_items)
    d_B = padded(B)
    ref = ease_recommend_reference(x, B, 20, x, (5,))
    first = device_lists(x, B, 20, x, (5,), ws_rows=ws_rows, d_B=d_B)
    assert same_lists(first, ref)
    again = device_lists(x, B, 20, x, (5,), ws_rows=ws_rows, d_B=d_B)
    assert same_lists(again, first) and same_lists(device_lists(x, B, 20, x, (5,), d_B=d_B), first)
    Bs, xs = weights(5, np.float64), users(5)
    assert same_lists(device_lists(xs, Bs, 3, ws_rows=ws_rows), ease_recommend_reference(xs, Bs, 3))   # the workspace came back as zeros


def test_columns_outside_the_items_are_skipped():
    """the device form skips them (the host form refuses them): a row with such entries scores as the row without them"""
    be = backend()
    n_items = 40
    B = weights(n_items, np.float32)
    xp = be.to_device(np.array([0, 3, 3 + AHEAD + 2]), torch.int32)
    cols = np.r_[[2, 99999, 5], [1, -3, 4, 6, n_items, 8, 9, 10, 11, 12]]
    assert cols.size == 3 + AHEAD + 2
    res, keys = be.ease_recommend(xp, be.to_device(cols, torch.int32), padded(B), n_items, 5)
    x = sp.csr_matrix(([1.0] * 10, ([0, 0] + [1] * 8, [2, 5, 1, 4, 6, 8, 9, 10, 11, 12])), shape=(2, n_items))
    ref = ease_recommend_reference(x, B, 5)
    assert np.array_equal(res.cpu().numpy() - 1, ref[0]) and np.array_equal(key_scores(keys.cpu().numpy()), ref[1])


# ---- the class -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fitted(precision):
    return EASE(500.0, precision=precision, backend=backend()).fit(movielens_csr()[:900])


@pytest.mark.parametrize("precision", ["float", "double"])
def test_predict_equals_the_definition_on_the_downloaded_weights(precision):
    m = fitted(precision)
    test = movielens_csr()[900:]
    top = m.predict(test, 10, items_exclude=(49,))
    ref = ease_recommend_reference(test, m.B, 10, test, (49,))
    assert np.array_equal(np.asarray(top), ref[0]) and np.array_equal(top.scores, ref[1]) and top.scores.dtype == np.float64
    sim = m.similar_items([0, 49, 180], k=5)
    one_hot = sp.csr_matrix((np.ones(3), [0, 49, 180], [0, 1, 2, 3]), shape=(3, 1682))
    same = m.predict(one_hot, 5)
    assert np.array_equal(np.asarray(sim), np.asarray(same)) and np.array_equal(sim.scores, same.scores)
    assert np.array_equal(sim.scores, np.stack([m.B[i][np.asarray(sim)[r]] for r, i in enumerate((0, 49, 180))]).astype(np.float64))


def test_evaluate_equals_the_metrics_of_the_reference_lists():
    from rsparse_amd.metrics import hit_metrics_reference, list_metrics_reference, ranking_metrics, self_information
    from test_metrics_abi import ref_metrics, to_r
    m = fitted("float")
    test = movielens_csr()[900:].tocsr()
    held_mask = np.random.default_rng(7).random(test.nnz) < 0.5
    part = lambda keep: sp.csr_matrix((test.data[keep], test.indices[keep], np.concatenate([[0], np.cumsum(keep)])[test.indptr]), shape=test.shape)
    hist, held = part(~held_mask), part(held_mask)
    cut = (5, 10)
    ev = m.evaluate(hist, held, cut, metrics=("ap", "ndcg", "precision", "recall", "hit", "mrr", "coverage", "popularity", "novelty"))
    lists = ease_recommend_reference(hist, m.B, 10, hist)[0]
    for t, c in enumerate(cut):
        ap, ndcg = ranking_metrics(lists[:, :c], held)                      # the package's ap_k / ndcg_k: the same bits
        assert np.array_equal(ev["ap"][:, t], ap, equal_nan=True) and np.array_equal(ev["ndcg"][:, t], ndcg, equal_nan=True)
        # ... and their numpy statement, whose sums run in another order: the bound tests/test_metrics.py holds them to
        for got, ref in zip((ap, ndcg), ref_metrics(to_r(lists[:, :c]), held)):
            assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.nanmax(np.abs(got - ref)) <= 1e-12
    hits = hit_metrics_reference(lists, held, cut, 1682)
    for name in ("precision", "recall", "hit", "mrr", "coverage"):
        assert np.array_equal(ev[name], hits[name], equal_nan=True), name
    lm = list_metrics_reference(lists, cut, 1682, m.item_count.astype(np.int32), self_information(m.item_count))
    for name in ("popularity", "novelty"):
        assert np.array_equal(ev[name], lm[name], equal_nan=True), name
    print("NDCG@10 on the device: %.3f" % float(np.nanmean(ev["ndcg"][:, 1])))
    with pytest.raises(_lib.UnsupportedOnDevice):
        m.evaluate(hist, held, 5, metrics=("diversity",))
