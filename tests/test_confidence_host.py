"""rsparse_amd/confidence.py without a GPU: `confidence_reference` (the numpy definition of the device kernels) against
independent scipy / numpy expressions on the movielens fixture, `ScaleNormalize` against the reference's diag(norm_vec^(scale - 1))
products, the reuse of the fitted item tables on unseen rows, and `WRMF(preprocess=Confidence(kind))` through the CPU stand-in
backend: it must equal `WRMF()` run on `Confidence(kind).fit_transform(x)` exactly -- the fit, `transform` and `predict` of new
users -- also for "bm25", which a callable applied to the transposed block (the path a `Confidence` never takes) gets wrong."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_movielens


@pytest.fixture(scope="module")
def ml():
    n_user, n_item, p, i, x = load_movielens()
    m = sp.csc_matrix((x, i, p), shape=(n_user, n_item)).tocsr()
    m.sort_indices()
    return m


def test_reference_against_independent_expressions(ml):
    from rsparse_amd.confidence import confidence_fit_reference, confidence_reference
    n, n_item = ml.shape
    df = np.diff(ml.tocsc().indptr)
    idf = np.log(n) - np.log1p(df)
    assert idf.min() >= 0.479                      # every kind is non-negative on this fixture
    st = confidence_fit_reference(ml, "bm25")
    assert st["n_fit"] == n and np.array_equal(st["item_count"], df)
    np.testing.assert_allclose(st["item_table"], idf, rtol=0, atol=4e-15)
    np.testing.assert_allclose(st["mean_row_sum"], ml.sum() / n, rtol=1e-14)

    dense = ml.toarray()

    def same(w, expect):
        assert np.array_equal(w.indptr, ml.indptr) and np.array_equal(w.indices, ml.indices)
        np.testing.assert_allclose(w.toarray(), expect, rtol=1e-13, atol=0)

    same(confidence_reference(ml, "linear", alpha=40.0), np.where(dense != 0, 1 + 40 * dense, 0))
    same(confidence_reference(ml, "log", alpha=40.0, eps=0.5), np.where(dense != 0, 1 + 40 * np.log(1 + dense / 0.5), 0))
    same(confidence_reference(ml, "tfidf"), np.sqrt(dense) * idf[None, :])
    s_u = dense.sum(axis=1)
    L = 0.2 + 0.8 * s_u / s_u.mean()
    same(confidence_reference(ml, "bm25"), dense * 101.0 / (100.0 * L[:, None] + dense) * idf[None, :])
    L2 = 0.5 + 0.5 * s_u / s_u.mean()
    same(confidence_reference(ml, "bm25", K1=1.2, B=0.5), dense * 2.2 / (1.2 * L2[:, None] + dense) * idf[None, :])
    for norm in (1, 2, 3):
        rn = (np.abs(dense) ** norm).sum(axis=1) ** (1.0 / norm)
        same(confidence_reference(ml, "normalize", norm=norm, scale=0.5, target="rows"), dense * (rn ** -0.5)[:, None])
        cn = (np.abs(dense) ** norm).sum(axis=0) ** (1.0 / norm)
        t = np.where(cn != 0, np.where(cn != 0, cn, 1.0) ** (0.25 - 1.0), 0.0)
        same(confidence_reference(ml, "normalize", norm=norm, scale=0.25, target="columns"), dense * t[None, :])


def test_scale_normalize_equals_the_diagonal_product():
    from rsparse_amd import ScaleNormalize
    rng = np.random.default_rng(3)
    d = rng.random((40, 23)) * (rng.random((40, 23)) < 0.3)
    d[7, :] = 0.0            # a zero-norm row
    d[:, 5] = 0.0            # and a zero-norm column
    d[3, 2] = -1.5
    x = sp.csr_matrix(d)
    for target, axis in (("rows", 1), ("columns", 0)):
        for norm in (1, 2):
            for scale in (0.5, 0.0):
                nv = (np.abs(d) ** norm).sum(axis=axis) ** (1.0 / norm)
                vec = np.where(nv != 0, np.where(nv != 0, nv, 1.0) ** (scale - 1.0), 0.0)
                sn = ScaleNormalize(scale=scale, norm=norm, target=target)
                got = sn.fit_transform(x)
                expect = np.diag(vec) @ d if target == "rows" else d @ np.diag(vec)
                np.testing.assert_allclose(got.toarray(), expect, rtol=1e-14, atol=0)
                np.testing.assert_allclose(sn.scaling, vec, rtol=1e-14, atol=0)
                assert np.array_equal(got.indices, x.indices) and np.array_equal(got.indptr, x.indptr)   # the pattern stays
                # transform multiplies by the STORED vector
                y = sp.csr_matrix(rng.random(d.shape) * (rng.random(d.shape) < 0.2))
                expect_y = np.diag(vec) @ y.toarray() if target == "rows" else y.toarray() @ np.diag(vec)
                np.testing.assert_allclose(sn.transform(y).toarray(), expect_y, rtol=1e-14, atol=0)
    sn = ScaleNormalize(target="rows").fit(x)
    with pytest.raises(ValueError):
        sn.transform(x[:10])                       # another nrow, as in R
    with pytest.raises(RuntimeError):
        ScaleNormalize().transform(x)


def test_fitted_item_tables_are_reused_on_unseen_rows(ml):
    from rsparse_amd import Confidence
    from rsparse_amd.confidence import confidence_reference
    train, new = ml[:800], ml[800:]
    for kind, par in (("bm25", {}), ("tfidf", {}), ("normalize", {"target": "columns"}), ("normalize", {"target": "rows"}), ("log", {"alpha": 3.0})):
        c = Confidence(kind, **par)
        w_train = c.fit_transform(train)
        assert c.n_fit == 800 and np.array_equal(c.item_count, np.diff(train.tocsc().indptr))
        again = c.transform(train)
        assert np.array_equal(again.data, w_train.data)          # transform(x_train) == fit_transform(x_train)
        w_new = c.transform(new)
        assert np.array_equal(w_new.indices, new.indices)
        if kind == "bm25":
            # s_u from the new rows, idf and sbar from the fit
            dense = new.toarray()
            s_u = dense.sum(axis=1)
            L = 0.2 + 0.8 * s_u / (train.sum() / 800)
            idf = np.log(800) - np.log1p(np.diff(train.tocsc().indptr))
            np.testing.assert_allclose(w_new.toarray(), dense * 101.0 / (100.0 * L[:, None] + dense) * idf[None, :], rtol=1e-13)
            assert c.mean_row_sum == pytest.approx(train.sum() / 800, rel=1e-14)
            np.testing.assert_allclose(c.item_table, idf, atol=4e-15, rtol=0)
            # and NOT what a fit on the new rows alone gives
            assert not np.allclose(w_new.data, confidence_reference(new, "bm25").data)


def test_empty_and_all_zero_matrices():
    from rsparse_amd import Confidence
    empty = sp.csr_matrix((5, 7), dtype=np.float64)
    zeros = sp.csr_matrix((np.zeros(3), np.array([0, 2, 1]), np.array([0, 2, 2, 3])), shape=(3, 4))
    with np.errstate(all="raise"):
        for kind in ("linear", "log", "tfidf", "bm25", "normalize"):
            w = Confidence(kind).fit_transform(empty)
            assert w.shape == (5, 7) and w.nnz == 0
            w = Confidence(kind).fit_transform(zeros)       # sbar = 0: the pattern comes back, nothing divides by zero
            assert np.array_equal(w.indices, zeros.indices) and np.isfinite(w.data).all()


@pytest.mark.parametrize("kind,par", [("log", {"alpha": 10.0, "eps": 2.0}), ("bm25", {"K1": 20.0})])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_wrmf_with_a_confidence_equals_wrmf_on_the_weighted_matrix(ml, kind, par, precision):
    from oracle_backend import OracleBackend
    from rsparse_amd import WRMF, Confidence
    train, new = ml[:300, :400], ml[800:830, :400]
    kw = dict(rank=6, lambda_=0.1, precision=precision, solver="cholesky", backend=OracleBackend())
    c = Confidence(kind, **par)
    a = WRMF(preprocess=c, rng=1, **kw)
    emb_a = a.fit_transform(train, n_iter=2, convergence_tol=-1)
    ref_c = Confidence(kind, **par)
    xw = ref_c.fit_transform(train)
    b = WRMF(rng=1, **kw)
    emb_b = b.fit_transform(xw, n_iter=2, convergence_tol=-1)
    assert np.array_equal(emb_a, emb_b) and np.array_equal(a.components, b.components)
    assert c.n_fit == 300 and np.array_equal(c.item_count, ref_c.item_count)
    new_w = ref_c.transform(new)
    assert np.array_equal(a.transform(new), b.transform(new_w))
    pa, pb = a.predict(new, 5), b.predict(new_w, 5)
    assert np.array_equal(np.asarray(pa), np.asarray(pb)) and np.array_equal(pa.scores, pb.scores)
    if kind == "bm25":
        # what the callable path does at inference -- the hook on the transposed block -- is another matrix
        wrong = ref_c.host_transform(sp.csr_matrix(new.T)).T
        assert not np.allclose(wrong.toarray(), new_w.toarray())


def test_errors(ml):
    from rsparse_amd import WRMF, Confidence
    from oracle_backend import OracleBackend
    neg = ml[:50].copy()
    neg.data[3] = -1.0
    for kind in ("tfidf", "bm25"):
        with pytest.raises(ValueError):
            Confidence(kind).fit(neg)
    with pytest.raises(ValueError):
        Confidence("log", eps=0.5).fit(neg)        # v / eps = -2
    Confidence("linear").fit(neg)                  # (no domain)
    with pytest.raises(ValueError):
        Confidence("okapi")
    with pytest.raises(ValueError):
        Confidence("bm25", alpha=1.0)
    with pytest.raises(RuntimeError):
        Confidence("bm25").transform(ml)
    with pytest.raises(RuntimeError, match="model is not fitted"):
        WRMF(rank=4, preprocess=Confidence("bm25"), backend=OracleBackend()).transform(ml)
    with pytest.raises(TypeError):
        WRMF(preprocess=3)
