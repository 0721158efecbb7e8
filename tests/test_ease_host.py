"""EASE without a device: the numpy definitions of rsparse_amd/ease.py against what they claim to be, the class on the CPU stand-in
backend, the refusals of the C ABI before any device work, and the ABI table."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_movielens
from oracle_backend import OracleBackend
from rsparse_amd import EASE, _lib
from rsparse_amd.ease import (ease_gram_reference, ease_recommend_reference, ease_scores_reference, ease_weights_reference, key_scores,
                              score_keys)

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("rsparse_hip_item_gram_device", "rsparse_hip_ease_recommend_device", "rsparse_hip_item_gram", "rsparse_hip_ease_recommend")


def movielens_csr():
    n_user, n_item, p, i, x = load_movielens()
    return sp.csc_matrix((np.ones_like(x), i, p), shape=(n_user, n_item)).tocsr()


def protocol():
    """binary; the first 900 users train, the other 43 have about half of their items held out -> (train, history, held_out)"""
    m = movielens_csr()
    m.sort_indices()
    train, test = m[:900], m[900:].tocsr()
    held = np.random.default_rng(7).random(test.nnz) < 0.5
    part = lambda keep: sp.csr_matrix((test.data[keep], test.indices[keep], np.concatenate([[0], np.cumsum(keep)])[test.indptr]), shape=test.shape)
    return train, part(~held), part(held)


@pytest.fixture(scope="module")
def fixture_weights():
    train, hist, held = protocol()
    return train, hist, held, ease_weights_reference(ease_gram_reference(train, 500.0))


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def test_weights_are_the_ridge_regression_of_every_column_on_the_others():
    x = (np.random.default_rng(3).random((60, 12)) < 0.4).astype(np.float64)
    B = ease_weights_reference(ease_gram_reference(sp.csr_matrix(x), 2.0))
    assert B.dtype == np.float64 and (np.diag(B) == 0).all() and not np.signbit(np.diag(B)).any()
    err = 0.0
    for j in range(12):
        rest = np.delete(np.arange(12), j)
        w = np.linalg.solve(x[:, rest].T @ x[:, rest] + 2.0 * np.eye(11), x[:, rest].T @ x[:, j])
        err = max(err, np.abs(B[rest, j] - w).max())
    print("EASE identity: max |B - ridge| = %.3g" % err)
    assert err <= 1e-12


def test_gram_reference_is_counts_and_one_rounding_on_the_diagonal():
    rng = np.random.default_rng(5)
    x = sp.csr_matrix((rng.random((40, 9)) < 0.3) * rng.integers(1, 4, (40, 9)).astype(float))   # values are ignored
    x = sp.csr_matrix((np.r_[x.data, 0.0], np.r_[x.indices, 0], np.r_[x.indptr[:-1], x.indptr[-1] + 1]), shape=x.shape)  # a stored zero
    h = (x.toarray() != 0).astype(np.int64)
    a = ease_gram_reference(x, 0.3)
    g = h.T @ h
    assert a.dtype == np.float64 and np.array_equal(a - np.diag(np.diag(a)), g - np.diag(np.diag(g)))
    assert np.array_equal(np.diag(a), np.diag(g).astype(np.float64) + np.float64(0.3))
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            ease_gram_reference(x, bad)


def test_singular_gram_is_a_numeric_error():
    x = sp.csr_matrix(np.array([[1, 1, 0], [1, 1, 0], [0, 0, 0]], dtype=float))   # two equal columns and an empty one
    with pytest.raises(_lib.RsparseHipError) as e:
        ease_weights_reference(ease_gram_reference(x, 0.0))
    assert e.value.code == _lib.ERR_NUMERIC and "lambda = 0" in str(e.value)
    with pytest.raises(_lib.RsparseHipError) as e:
        ease_weights_reference(-np.eye(3))
    assert e.value.code == _lib.ERR_NUMERIC


def test_keys_order_as_the_doubles_and_invert():
    v = np.array([-np.inf, -1e300, -2.5, -5e-324, 0.0, 5e-324, 1.0, 1.0000000000000002, 1e300, np.inf])
    k = score_keys(v)
    assert k.dtype == np.uint64 and (np.diff(k.astype(object)) > 0).all() and np.array_equal(key_scores(k), v)
    assert k.min() > 0 and k.max() < np.uint64(2 ** 64 - 1) and score_keys(np.zeros(1))[0] == np.uint64(1 << 63)
    assert np.array_equal(key_scores(k.view(np.int64)), v)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_scores_reference_is_the_dense_product_bit_for_bit(fixture_weights, dtype):
    """The dense product is taken with numpy's own loop (einsum without BLAS), which sums over the items in ascending order: the
    definition's order with a +-0.0 added for every item a row does not hold.  `hist.toarray() @ B` through OpenBLAS's dgemm blocks
    the sum over the items and differs from both in the last bit (here: 59 % of the cells, at most 5.6e-16)."""
    train, hist, held, B = fixture_weights
    B = B.astype(dtype)
    got = ease_scores_reference(hist, B)
    dense = np.einsum("ui,ij->uj", hist.toarray(), B.astype(np.float64), optimize=False)
    assert got.dtype == np.float64 and np.array_equal(got, dense)
    assert np.abs(got - hist.toarray() @ B.astype(np.float64)).max() <= 1e-14
    assert not np.signbit(got[got == 0]).any()


def brute_lists(score, k, nr, excl):
    n, n_items = score.shape
    items = np.full((n, k), -1, dtype=np.int64)
    scores = np.zeros((n, k))
    for u in range(n):
        adm = np.ones(n_items, dtype=bool)
        if nr is not None:
            adm[nr[u].indices] = False
        adm[list(excl)] = False
        cand = np.flatnonzero(adm)
        first = cand[np.lexsort((cand, -score[u, cand]))[:k]]
        items[u, :first.size], scores[u, :first.size] = first, score[u, first]
    return items, scores


def test_recommend_reference_is_the_brute_force_order(fixture_weights):
    train, hist, held, B = fixture_weights
    score = np.einsum("ui,ij->uj", hist.toarray(), B, optimize=False)   # (the dense product in the definition's order, see above)
    for k, nr, excl in ((10, hist, ()), (7, None, (0, 49, 180)), (25, hist, (1, 2, 3))):
        it, sc = ease_recommend_reference(hist, B, k, nr, excl)
        ref = brute_lists(score, k, nr, excl)
        assert np.array_equal(it, ref[0]) and np.array_equal(sc, ref[1])
    # ties to the smaller item, an empty row, and k above the admissible count
    tiny = np.array([[0.0, 1.0, 1.0, -2.0], [0.5, 0.0, 0.5, 0.5], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 0.0]])
    x = sp.csr_matrix(np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0]], dtype=float))
    it, sc = ease_recommend_reference(x, tiny, 5, x, (3,))
    assert np.array_equal(it, [[1, 2, -1, -1, -1], [0, 2, -1, -1, -1], [0, 1, 2, -1, -1]])
    assert np.array_equal(sc, [[1, 1, 0, 0, 0], [0.5, 0.5, 0, 0, 0], [0, 0, 0, 0, 0]])


# ---- the class on the CPU stand-in -----------------------------------------------------------------------------------------------
def ndcg10(lists, held):
    from test_metrics_abi import ref_metrics, to_r
    return float(np.nanmean(ref_metrics(to_r(lists), held)[1]))


def test_class_beats_popularity_on_the_fixture(fixture_weights):
    train, hist, held, B = fixture_weights
    m = EASE(500.0, precision="double", backend=OracleBackend()).fit(train)
    assert np.array_equal(m.B, B) and np.array_equal(m.item_count, np.asarray(train.sum(axis=0)).ravel())
    top = m.predict(hist, 10)
    ref = ease_recommend_reference(hist, B, 10, hist)
    assert np.array_equal(np.asarray(top), ref[0]) and np.array_equal(top.scores, ref[1]) and top.scores.dtype == np.float64
    pop = np.broadcast_to(m.item_count.astype(np.float64), hist.shape)
    pop_lists, _ = brute_lists(pop, 10, hist, ())
    ease, popularity = ndcg10(np.asarray(top), held), ndcg10(pop_lists, held)
    print("NDCG@10: EASE %.3f, popularity %.3f, ratio %.2f" % (ease, popularity, ease / popularity))
    assert ease >= 1.3 * popularity


def test_class_conventions_on_the_stand_in():
    from test_metrics_abi import _oracle_metrics_backend, ref_metrics, to_r
    from rsparse_amd.metrics import hit_metrics_reference, list_metrics_reference, self_information
    rng = np.random.default_rng(11)
    b = (rng.random((30, 14)) < 0.3).astype(float)
    b[0] = 0
    x = sp.csr_matrix(b)
    m = EASE(1.5, backend=_oracle_metrics_backend()).fit(x)
    assert m.B.dtype == np.float32 and np.array_equal(m.B, ease_weights_reference(ease_gram_reference(x, 1.5), np.float32))
    top = m.predict(x, 4)
    assert np.array_equal(np.asarray(top)[0], [0, 1, 2, 3]) and (top.scores[0] == 0).all()          # the row of ties
    for u in range(30):
        assert not set(np.asarray(top)[u]) & set(np.flatnonzero(b[u]))
    top = m.predict(x, 14, not_recommend=None, items_exclude=(7,))
    assert (np.asarray(top)[:, :13] >= 0).all() and (np.asarray(top)[:, 13] == -1).all() and np.isnan(top.scores[:, 13]).all()
    sim = m.similar_items([2, 5], k=3)
    one_hot = sp.csr_matrix((np.ones(2), [2, 5], [0, 1, 2]), shape=(2, 14))
    ref = m.predict(one_hot, 3)
    assert np.array_equal(np.asarray(sim), np.asarray(ref)) and np.array_equal(sim.scores, ref.scores)
    assert not (np.asarray(sim) == [[2], [5]]).any() and np.array_equal(sim.scores[0], m.B[2][np.asarray(sim)[0]].astype(np.float64))
    held = sp.csr_matrix((rng.random(b.shape) < 0.3) * (1 - b) * 2.0)
    cut = (2, 5)
    ev = m.evaluate(x, held, cut, metrics=("ap", "ndcg", "precision", "recall", "hit", "mrr", "coverage", "popularity", "novelty"))
    lists = np.asarray(m.predict(x, 5))
    for t, c in enumerate(cut):
        ap, ndcg = ref_metrics(to_r(lists[:, :c]), held)
        assert np.array_equal(ev["ap"][:, t], ap, equal_nan=True) and np.array_equal(ev["ndcg"][:, t], ndcg, equal_nan=True)
    hits = hit_metrics_reference(lists, held, cut, 14)
    for name in ("precision", "recall", "hit", "mrr", "coverage"):
        assert np.array_equal(ev[name], hits[name], equal_nan=True), name
    lm = list_metrics_reference(lists, cut, 14, m.item_count.astype(np.int32), self_information(m.item_count))
    for name in ("popularity", "novelty"):
        assert np.array_equal(ev[name], lm[name], equal_nan=True), name
    for kw in ({"metrics": ("ndcg", "diversity")}, {"diversify": 0.5}):
        with pytest.raises(_lib.UnsupportedOnDevice):
            m.evaluate(x, held, 5, **kw)


def test_argument_errors():
    x = sp.csr_matrix(np.eye(4))
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            EASE(bad)
    with pytest.raises(ValueError):
        EASE(precision="half")
    with pytest.raises(RuntimeError):
        EASE(backend=OracleBackend()).predict(x, 2)
    m = EASE(1.0, backend=OracleBackend()).fit(x)
    for k in (0, True, 2.0):
        with pytest.raises(ValueError):
            m.predict(x, k)
    with pytest.raises(_lib.UnsupportedOnDevice):
        m.predict(x, _lib.KNN_MAX_TOPK + 1)
    with pytest.raises(ValueError):
        m.predict(x, 2, items_exclude=(4,))
    with pytest.raises(ValueError):
        m.predict(sp.csr_matrix(np.eye(5)), 2)
    with pytest.raises(ValueError):
        m.similar_items([4])
    with pytest.raises(_lib.RsparseHipError) as e:
        EASE(0.0, backend=OracleBackend()).fit(sp.csr_matrix(np.ones((3, 2))))
    assert e.value.code == _lib.ERR_NUMERIC
    with pytest.raises(_lib.UnsupportedOnDevice):
        EASE(backend=OracleBackend()).fit(sp.csr_matrix((1, _lib.EASE_MAX_ITEMS + 1)))


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------
def test_library_exports_the_ease_entry_points():
    lib = _lib.load()
    text = (ROOT / "include" / "rsparse_wrmf_hip.h").read_text()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert lib.rsparse_hip_abi_version() == 6                                # additive entries: the version stays
    from rsparse_amd.engine import HipBackend
    assert callable(HipBackend.item_gram) and callable(HipBackend.ease_recommend)


def test_constants_mirror_the_header():
    text = (ROOT / "include" / "rsparse_wrmf_hip.h").read_text()
    for name in ("MAX_ITEMS", "TILE_BYTES", "CHUNK", "AHEAD"):
        assert int(re.search(r"#define RSPARSE_HIP_EASE_%s (\d+)" % name, text).group(1)) == getattr(_lib, "EASE_" + name), name
    assert _lib.EASE_CHUNK % _lib.EASE_AHEAD == 0 and _lib.EASE_MAX_ITEMS ** 2 * 8 == 8 << 30


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _answer(rc, code, text):
    assert rc == code, (rc, _lib.load().rsparse_hip_last_error())
    assert text in _lib.load().rsparse_hip_last_error().decode(), _lib.load().rsparse_hip_last_error()


# 3 users x 4 items: rows {0, 2}, {1}, {0, 1, 3}
P = np.array([0, 2, 3, 6], dtype=np.int32)
J = np.array([0, 2, 1, 0, 1, 3], dtype=np.int32)
IP = np.array([0, 2, 4, 5, 6], dtype=np.int32)
IU = np.array([0, 2, 1, 2, 0, 2], dtype=np.int32)


def test_item_gram_device_status_codes():
    # (host pointers: every call here is rejected by the argument checks, or is the empty item range, before device work)
    fn = _lib.load().rsparse_hip_item_gram_device
    out = np.empty((4, 4))

    def call(ip=IP, iu=IU, up=P, uj=J, n_users=3, n_items=4, item0=0, item1=4, lam=0.5, out=out, ld=4, ws_rows=0):
        return fn(_vp(ip), _vp(iu), _vp(up), _vp(uj), n_users, n_items, item0, item1, lam, _vp(out), ld, ws_rows, None)

    for missing in ("ip", "iu", "up", "uj", "out"):
        _answer(call(**{missing: None}), _lib.ERR_INVALID, "NULL")
    _answer(call(n_users=-1), _lib.ERR_INVALID, "bad dimensions")
    _answer(call(n_items=-1), _lib.ERR_INVALID, "bad dimensions")
    for item0, item1 in ((-1, 4), (3, 2), (0, 5)):
        _answer(call(item0=item0, item1=item1), _lib.ERR_INVALID, "item0 <= item1 <= n_items")
    _answer(call(ws_rows=-1), _lib.ERR_INVALID, "ws_rows < 0")
    _answer(call(ld=3), _lib.ERR_INVALID, "ld_out < n_items")
    for lam in (-0.5, float("nan"), float("inf"), -float("inf")):
        _answer(call(lam=lam), _lib.ERR_INVALID, "lambda is negative or not finite")
    big = _lib.EASE_MAX_ITEMS + 1
    _answer(call(n_items=big, item1=4, ld=big), _lib.ERR_UNSUPPORTED, "n_items > 32768")
    assert call(n_items=big, ld=big, out=None) == _lib.ERR_INVALID          # the pointers are looked at first
    assert call(item0=2, item1=2) == _lib.OK                                 # an empty range: a no-op


def test_ease_recommend_device_status_codes():
    fn = _lib.load().rsparse_hip_ease_recommend_device
    raw = np.zeros(4 * 4 + 8, np.float32)
    B = raw[(-raw.ctypes.data // 4) % 4:][:16]                               # 16-byte aligned
    res, sc = np.empty((3, 2), np.int32), np.empty((3, 2), np.uint64)
    ex = np.array([1], dtype=np.int32)

    def call(xp=P, xj=J, n_rows=3, n_items=4, B=B, ld=4, f64=0, nr_p=None, nr_j=None, ex=None, n_ex=0, k=2, ws_rows=0, res=res, sc=sc):
        return fn(_vp(xp), _vp(xj), n_rows, n_items, _vp(B), ld, f64, _vp(nr_p), _vp(nr_j), _vp(ex), n_ex, k, ws_rows, _vp(res), _vp(sc), None)

    for missing in ("xp", "xj", "B", "res", "sc"):
        _answer(call(**{missing: None}), _lib.ERR_INVALID, "NULL")
    _answer(call(n_rows=-1), _lib.ERR_INVALID, "bad dimensions")
    _answer(call(n_items=-1), _lib.ERR_INVALID, "bad dimensions")
    _answer(call(k=0), _lib.ERR_INVALID, "k < 1")
    _answer(call(ws_rows=-1), _lib.ERR_INVALID, "ws_rows < 0")
    _answer(call(nr_p=P), _lib.ERR_INVALID, "nr_p without nr_j")
    _answer(call(n_ex=-1), _lib.ERR_INVALID, "bad exclude")
    _answer(call(n_ex=1), _lib.ERR_INVALID, "bad exclude")
    _answer(call(ld=3), _lib.ERR_INVALID, "ld_B < n_items")
    _answer(call(ld=6), _lib.ERR_INVALID, "multiple of 16 bytes")
    _answer(call(ld=6, f64=1, n_rows=0), _lib.OK, "")                        # (6 doubles are 48 bytes)
    _answer(call(ld=5, f64=1), _lib.ERR_INVALID, "multiple of 16 bytes")
    _answer(call(B=B[1:]), _lib.ERR_INVALID, "multiple of 16 bytes")
    _answer(call(k=_lib.KNN_MAX_TOPK + 1), _lib.ERR_UNSUPPORTED, "k > 1024")
    big = _lib.EASE_MAX_ITEMS + 1
    _answer(call(n_items=big, ld=big + 3), _lib.ERR_UNSUPPORTED, "n_items > 32768")
    assert call(n_rows=0, ex=ex, n_ex=1) == _lib.OK                          # no row: a no-op


def test_host_forms_check_their_arrays_first():
    lib = _lib.load()
    out = np.empty((4, 4))

    def gram(p=P, j=J, n_users=3, n_items=4, lam=1.0, out=out):
        return lib.rsparse_hip_item_gram(_vp(p), _vp(j), n_users, n_items, lam, _vp(out))

    for missing in ("p", "out"):
        _answer(gram(**{missing: None}), _lib.ERR_INVALID, "NULL")
    _answer(gram(j=None), _lib.ERR_INVALID, "j is NULL")
    _answer(gram(lam=-1.0), _lib.ERR_INVALID, "lambda is negative or not finite")
    _answer(gram(n_items=_lib.EASE_MAX_ITEMS + 1), _lib.ERR_UNSUPPORTED, "n_items > 32768")
    _answer(gram(p=np.array([1, 2, 3, 6], np.int32)), _lib.ERR_INVALID, "p[0] != 0")
    _answer(gram(p=np.array([0, 3, 2, 6], np.int32)), _lib.ERR_INVALID, "p decreases")
    _answer(gram(j=np.array([0, 4, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "a column outside [0, n_items)")
    _answer(gram(j=np.array([2, 0, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "not strictly ascending")
    assert gram(n_items=0, p=np.zeros(4, np.int32)) == _lib.OK               # no item: a no-op

    B = np.zeros((4, 4), np.float64, order="F")
    res, sc = np.empty((3, 2), np.int32, order="F"), np.empty((3, 2), np.float64, order="F")
    ex = np.array([1], dtype=np.int32)

    def rec(xp=P, xj=J, n_rows=3, n_items=4, B=B, f64=1, nr_p=None, nr_j=None, ex=None, n_ex=0, k=2, res=res, sc=sc):
        return lib.rsparse_hip_ease_recommend(_vp(xp), _vp(xj), n_rows, n_items, _vp(B), f64, _vp(nr_p), _vp(nr_j), _vp(ex), n_ex, k,
                                              _vp(res), _vp(sc))

    for missing in ("xp", "B", "res", "sc"):
        _answer(rec(**{missing: None}), _lib.ERR_INVALID, "NULL")
    _answer(rec(xj=None), _lib.ERR_INVALID, "x_j is NULL")
    _answer(rec(k=1025), _lib.ERR_UNSUPPORTED, "k > 1024")
    _answer(rec(k=0), _lib.ERR_INVALID, "k < 1")
    _answer(rec(n_ex=1), _lib.ERR_INVALID, "bad exclude")
    _answer(rec(nr_p=P), _lib.ERR_INVALID, "nr_p without nr_j")
    _answer(rec(xp=np.array([0, 3, 2, 6], np.int32)), _lib.ERR_INVALID, "x_p decreases")
    _answer(rec(xj=np.array([0, 2, 1, 0, 1, 4], np.int32)), _lib.ERR_INVALID, "x_j has a column outside [0, n_items)")
    _answer(rec(nr_p=P, nr_j=np.array([0, 2, 1, 0, 1, 9], np.int32)), _lib.ERR_INVALID, "nr_j has a column outside [0, n_items)")
    bad = B.copy(order="F")
    bad[2, 1] = np.inf
    _answer(rec(B=bad), _lib.ERR_INVALID, "not finite")
    _answer(rec(B=bad.astype(np.float32), f64=0), _lib.ERR_INVALID, "not finite")
    assert rec(n_rows=0, xp=np.zeros(1, np.int32), ex=ex, n_ex=1) == _lib.OK  # no row: a no-op
