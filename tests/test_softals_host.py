"""soft_svd / soft_impute and PureSVD without a GPU: the numpy definition (rsparse_amd/softals.py) against numpy.linalg.svd, the
driver on the CPU stand-in against the definition, and PureSVD's inference surface on the stand-in."""
import types

import numpy as np
import pytest
import scipy.sparse as sp

from oracle_backend import OracleBackend
from rsparse_amd import PureSVD, soft_impute, soft_svd
from rsparse_amd.softals import initial_left_factor, soft_als_reference, softals_half_reference


@pytest.fixture(scope="module")
def ml(movielens):
    n_user, n_item, p, i, x = movielens
    return sp.csc_matrix((x, i, p), shape=(n_user, n_item)).tocsr()


@pytest.fixture(scope="module")
def u0(ml):
    return initial_left_factor(ml.shape[0], 8, np.random.default_rng(5))


def test_initial_left_factor_is_orthonormal(u0):
    assert np.abs(u0.T @ u0 - np.eye(8)).max() < 1e-12


def test_half_reference_is_the_three_pass_composition():
    rng = np.random.default_rng(0)
    x = sp.random(40, 30, density=0.2, random_state=1, format="csr")
    M, W = rng.standard_normal((30, 5)), rng.standard_normal((40, 5))
    w, s, t = rng.random(5), rng.random(5), rng.random(5)
    out, sumsq = softals_half_reference(x.indptr, x.indices, x.data, M, W, w, s, t)
    delta = x.copy()
    rows = np.repeat(np.arange(40), np.diff(x.indptr))
    delta.data = x.data - np.einsum("tc,tc->t", W[rows] * w, M[x.indices])          # SDDMM at the pattern, subtract
    assert np.allclose(out, (delta @ M) * s + W * t, rtol=1e-13, atol=1e-13)           # CSR x dense
    assert np.isclose(sumsq, float(delta.data @ delta.data), rtol=1e-13)
    plain, _ = softals_half_reference(x.indptr, x.indices, x.data, M, None, None, np.ones(5), None)
    assert np.allclose(plain, x @ M, rtol=1e-13, atol=1e-13)


def test_definition_finds_the_singular_values(ml, u0):
    _, d, v, trace = soft_als_reference(ml, 8, 0.0, 100, -1.0, "svd", u0)
    sv = np.linalg.svd(ml.toarray(), compute_uv=False)[:8]
    err = np.abs(d - sv).max() / sv.max()
    print("relative error of the singular values: %.3g, trace length %d" % (err, len(trace)))
    assert len(trace) == 100
    assert np.abs(d - sv).max() <= 1e-10 * sv.max()
    assert np.abs(v.T @ v - np.eye(8)).max() < 1e-10


@pytest.mark.parametrize("target,fn", [("svd", soft_svd), ("soft_impute", soft_impute)])
def test_driver_on_the_stand_in_equals_the_definition(ml, u0, target, fn):
    init = types.SimpleNamespace(u=u0, d=np.ones(8), v=np.zeros((ml.shape[1], 8)))
    tol = 1e-4
    got = fn(ml, rank=8, lambda_=5.0, n_iter=30, convergence_tol=tol, init=init, backend=OracleBackend())
    u, d, v, trace = soft_als_reference(ml, 8, 5.0, 30, tol, target, u0)
    assert len(got.trace) == len(trace) < 30                          # stopped by convergence_tol, at the same iteration
    assert trace[-1][0] < tol <= trace[-2][0]
    assert np.allclose(np.array(got.trace), np.array(trace), rtol=1e-12, atol=1e-12, equal_nan=True)
    for a, b in ((got.u, u), (got.d, d), (got.v, v)):
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    if target == "soft_impute":
        losses = [l for _, l in trace]
        assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    else:
        assert all(np.isnan(l) for _, l in trace)


def test_rng_makes_a_fit_reproducible(ml):
    a = soft_svd(ml, rank=4, n_iter=3, rng=3, backend=OracleBackend())
    b = soft_svd(ml, rank=4, n_iter=3, rng=3, backend=OracleBackend())
    assert np.array_equal(a.d, b.d) and np.array_equal(a.v, b.v)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lambda_50_lowers_the_rank(ml, u0, dtype):
    lam = 50.0
    # the singular values of the final m, before the threshold: none may sit at lambda, or the rank would hang on rounding
    u, d, v, _ = soft_als_reference(ml, 8, lam, 20, -1.0, "soft_impute", u0, final_svd=False, dtype=dtype)
    m, _ = softals_half_reference(ml.indptr, ml.indices, ml.data.astype(dtype), v, u, d, np.ones(8), None)
    m = m.astype(dtype) + (u * d.astype(dtype)) @ (v.T @ v)
    sv = np.linalg.svd(m.astype(np.float64), compute_uv=False)
    print("singular values of m:", sv)
    assert np.abs(sv - lam).min() > 1e-3 * lam
    _, d_final, v_final, _ = soft_als_reference(ml, 8, lam, 20, -1.0, "soft_impute", u0, dtype=dtype)
    assert d_final.size == int(np.sum(sv > lam)) < 8 and v_final.shape == (ml.shape[1], d_final.size)
    assert np.allclose(d_final, sv[:d_final.size] - lam, rtol=1e-6)


def test_a_lambda_beyond_the_largest_singular_value_raises(ml, u0):
    with pytest.raises(ValueError, match="all singular vectors are zero"):
        soft_als_reference(ml, 8, 1e4, 5, -1.0, "svd", u0)
    init = types.SimpleNamespace(u=u0, d=np.ones(8), v=np.zeros((ml.shape[1], 8)))
    with pytest.raises(ValueError, match="all singular vectors are zero"):
        soft_svd(ml, rank=8, lambda_=1e4, n_iter=5, init=init, backend=OracleBackend())


def test_argument_checks(ml, u0):
    be = OracleBackend()
    small = types.SimpleNamespace(u=u0[:, :4], d=np.ones(4), v=np.zeros((ml.shape[1], 4)))
    with pytest.raises(NotImplementedError):                          # the reference's pad_svd
        soft_svd(ml, rank=8, init=small, backend=be)
    big = types.SimpleNamespace(u=np.zeros((ml.shape[0], 9)), d=np.ones(9), v=np.zeros((ml.shape[1], 9)))
    with pytest.raises(ValueError, match="bigger rank"):
        soft_svd(ml, rank=8, init=big, backend=be)
    with pytest.raises(ValueError):
        soft_svd(ml, rank=8, precision="half", backend=be)
    with pytest.raises(ValueError):
        PureSVD(method="qr")
    with pytest.raises(TypeError):
        PureSVD(init=np.zeros((3, 3)))


# ---- PureSVD on the stand-in ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted(ml_train):
    n_user, n_item, tp, ti, tx = ml_train
    full = sp.csc_matrix((tx, ti, tp), shape=(n_user, n_item)).tocsr()
    coo = full.tocoo()
    out = np.random.default_rng(21).random(coo.nnz) < 0.2
    train = sp.csr_matrix((coo.data[~out], (coo.row[~out], coo.col[~out])), shape=full.shape)
    held = sp.csr_matrix((coo.data[out], (coo.row[out], coo.col[out])), shape=full.shape)
    from test_metrics_abi import _oracle_metrics_backend             # (the stand-in with `ranking_metrics`)
    m = PureSVD(rank=8, lambda_=0.0, rng=1, backend=_oracle_metrics_backend())
    emb = m.fit_transform(train, n_iter=10, convergence_tol=-1)
    return m, emb, train, held


def test_puresvd_transform_and_components(fitted):
    m, emb, train, _ = fitted
    v, d = m.svd.v, m.svd.d
    assert emb.shape == (900, 8) and np.allclose(emb, train @ v, rtol=1e-12, atol=1e-12)     # x %*% v
    shrunk = PureSVD(rank=8, lambda_=20.0, rng=1, backend=OracleBackend())
    e2 = shrunk.fit_transform(train, n_iter=10, convergence_tol=-1)
    assert np.allclose(e2, train @ shrunk.svd.v, rtol=1e-12, atol=1e-12)                     # ... which is not u o d
    assert not np.allclose(e2, shrunk.svd.u * shrunk.svd.d, rtol=1e-3)
    assert np.allclose(m.components, (v * d).T, rtol=1e-15)
    rows = train[100:140]
    assert np.allclose(m.transform(rows), rows @ v, rtol=1e-12, atol=1e-12)
    log = PureSVD(rank=4, preprocess=lambda a: a.log1p(), rng=1, backend=OracleBackend())
    log.fit_transform(train, n_iter=2, convergence_tol=-1)
    assert np.allclose(log.transform(rows), rows.log1p() @ log.svd.v, rtol=1e-12, atol=1e-12)


def test_puresvd_predict_scores_are_the_dense_product(fitted):
    m, _, train, _ = fitted
    rows = train[:50]
    top = m.predict(rows, 10)
    dense = m.transform(rows) @ m.components
    dense[rows.toarray() != 0] = -np.inf
    want = -np.sort(-dense, axis=1)[:, :10]
    assert np.allclose(top.scores, want, rtol=1e-10, atol=1e-10)
    assert np.allclose(np.take_along_axis(dense, np.asarray(top), axis=1), want, rtol=1e-10, atol=1e-10)


def test_puresvd_evaluate_equals_the_metrics_of_predict(fitted):
    # (rsparse_amd.metrics.ap_k / ndcg_k run on the device: tests/test_puresvd.py compares with them; here their restated
    # reference, tests/test_metrics_abi.ref_metrics)
    from test_metrics_abi import ref_metrics, to_r
    m, _, train, held = fitted
    got = m.evaluate(train, held, 10)
    top = m.predict(train, 10)
    canon = sp.csr_matrix(held)
    canon.sort_indices()
    ap, ndcg = ref_metrics(to_r(top), canon)
    assert np.allclose(got["ap"], ap, equal_nan=True, rtol=1e-12)
    assert np.allclose(got["ndcg"], ndcg, equal_nan=True, rtol=1e-12)
    assert np.nanmean(got["ap"]) > 0.05                               # PureSVD ranks held-out items far above chance


def test_puresvd_similar_items_takes_cosines_over_v(fitted):
    m, _, _, _ = fitted
    q = np.array([0, 10, 49, 257])
    got = m.similar_items(q, k=5)

    def cosines(F):
        with np.errstate(invalid="ignore"):
            n = F / np.linalg.norm(F, axis=1, keepdims=True)
        c = np.nan_to_num(n[q] @ n.T, nan=-np.inf)                   # (items without a direction are never returned)
        c[np.arange(q.size), q] = -np.inf
        return c

    c = cosines(m.svd.v)
    assert np.allclose(got.scores, -np.sort(-c, axis=1)[:, :5], rtol=1e-10, atol=1e-12)
    cd = cosines(m.svd.v * m.svd.d)
    assert not np.allclose(got.scores, -np.sort(-cd, axis=1)[:, :5], rtol=1e-3)


def test_puresvd_explain_is_unsupported(fitted):
    m, _, train, _ = fitted
    with pytest.raises(NotImplementedError):
        m.explain(train[:2], sp.csr_matrix(([1.0], ([0], [1])), shape=(2, train.shape[1])))
