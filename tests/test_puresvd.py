"""soft_svd / soft_impute and PureSVD on the device against the float64 definition (rsparse_amd/softals.py) on MovieLens-100k.
Singular vectors are never compared directly -- signs, and rotations inside clusters of singular values, are free: only d,
products, and the singular values of v^T v_ref are."""
import functools
import types

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_movielens
from rsparse_amd.softals import initial_left_factor, soft_als_reference

pytestmark = pytest.mark.gpu

N_ITER = 20
CASES = [("svd", 8, 0.0), ("svd", 8, 5.0), ("svd", 8, 50.0)] + [("soft_impute", k, lam) for k in (8, 32) for lam in (0.0, 5.0, 50.0)]


@functools.lru_cache(maxsize=None)
def ml():
    n_user, n_item, p, i, x = load_movielens()
    return sp.csc_matrix((x, i, p), shape=(n_user, n_item)).tocsr()


@functools.lru_cache(maxsize=None)
def start(rank):
    return initial_left_factor(ml().shape[0], rank, np.random.default_rng(5))


@functools.lru_cache(maxsize=None)
def definition(target, rank, lam, dtype, tol=-1.0):
    return soft_als_reference(ml(), rank, lam, N_ITER, tol, target, start(rank), dtype=np.dtype(dtype))


def fit(target, rank, lam, precision, tol=-1.0, n_iter=N_ITER):
    from rsparse_amd import soft_impute, soft_svd
    init = types.SimpleNamespace(u=start(rank), d=np.ones(rank), v=np.zeros((ml().shape[1], rank)))
    fn = soft_svd if target == "svd" else soft_impute
    return fn(ml(), rank=rank, lambda_=lam, n_iter=n_iter, convergence_tol=tol, init=init, precision=precision)


def corner(u, d, v):
    return (u[:50].astype(np.float64) * d) @ v[:60].astype(np.float64).T


def errors(got, ref):
    """(relative error of d, error of the 50 x 60 corner of u diag(d) v^T over its maximum, of the loss trace, 1 - the smallest
    singular value of v^T v_ref) of a fit (u, d, v, trace) against the float64 definition's"""
    u, d, v, trace = got
    ur, dr, vr, tr = ref
    assert d.shape == dr.shape and len(trace) == len(tr)
    c, cr = corner(u, d, v), corner(ur, dr, vr)
    loss, loss_r = np.array([l for _, l in trace]), np.array([l for _, l in tr])
    e_loss = 0.0 if np.all(np.isnan(loss_r)) else float(np.abs(loss - loss_r).max() / np.abs(loss_r).max())
    align = np.linalg.svd(v.astype(np.float64).T @ vr, compute_uv=False)
    return (float(np.abs(d - dr).max() / dr.max()), float(np.abs(c - cr).max() / np.abs(cr).max()), e_loss, float(1.0 - align.min()))


@pytest.mark.parametrize("target,rank,lam", CASES)
def test_double_fit_equals_the_definition(target, rank, lam):
    ref = definition(target, rank, lam, "float64")
    got = fit(target, rank, lam, "double")
    assert got.d.size == ref[1].size                                  # the same final rank
    e_d, e_c, e_loss, e_v = errors((got.u, got.d, got.v, got.trace), ref)
    print("%s rank %d lambda %g: final rank %d, errors d %.3g corner %.3g loss %.3g subspace %.3g"
          % (target, rank, lam, got.d.size, e_d, e_c, e_loss, e_v))
    assert e_d <= 1e-9 and e_c <= 1e-9 and e_loss <= 1e-9            # the project's bound for its fp64 layer
    deltas = np.array([f for f, _ in got.trace]), np.array([f for f, _ in ref[3]])
    assert np.allclose(deltas[0], deltas[1], rtol=1e-6, atol=1e-12)
    if lam == 50.0 and target == "soft_impute" and rank == 8:
        assert got.d.size == 6


@pytest.mark.parametrize("target,rank,lam", CASES)
def test_float_fit_is_as_close_as_the_definition_in_float(target, rank, lam):
    ref = definition(target, rank, lam, "float64")
    ref32 = definition(target, rank, lam, "float32")
    got = fit(target, rank, lam, "float")
    assert got.u.dtype == np.float32 and got.d.size == ref[1].size == ref32[1].size
    e = errors((got.u, got.d, got.v, got.trace), ref)
    e32 = errors(ref32, ref)
    print("%s rank %d lambda %g: device float errors (d, corner, loss, subspace) %s; definition in float32 %s"
          % (target, rank, lam, " ".join("%.3g" % a for a in e), " ".join("%.3g" % a for a in e32)))
    for a, b in zip(e[:3], e32[:3]):
        assert a <= max(4.0 * b, 1e-6)


@pytest.mark.parametrize("target", ["svd", "soft_impute"])
def test_stops_at_the_iteration_of_the_definition(target):
    tol = 1e-3                                                        # (the definition's change is 4 % and more away from it)
    ref = definition(target, 8, 5.0, "float64", tol)
    got = fit(target, 8, 5.0, "double", tol)
    assert len(got.trace) == len(ref[3]) < N_ITER
    assert errors((got.u, got.d, got.v, got.trace), ref)[0] <= 1e-9


def test_a_lambda_beyond_the_largest_singular_value_raises():
    with pytest.raises(ValueError, match="all singular vectors are zero"):
        fit("svd", 8, 1e4, "double", n_iter=5)                       # (as tests/test_softals_host.py asks of the definition)


def test_rng_start_and_reproducibility():
    from rsparse_amd import soft_svd
    a = soft_svd(ml(), rank=8, n_iter=30, convergence_tol=-1, rng=3)
    b = soft_svd(ml(), rank=8, n_iter=30, convergence_tol=-1, rng=3)
    assert np.array_equal(a.d, b.d) and np.array_equal(a.v, b.v)      # a repeated fit returns the same bits
    sv = np.linalg.svd(ml().toarray(), compute_uv=False)[:8]
    assert np.abs(a.d[:4] - sv[:4]).max() <= 1e-3 * sv[0]


# ---- PureSVD -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fitted(precision, method):
    from rsparse_amd import PureSVD
    full = ml()[:900]                                                 # the rows of the `ml_train` fixture
    coo = full.tocoo()
    out = np.random.default_rng(21).random(coo.nnz) < 0.2
    train = sp.csr_matrix((coo.data[~out], (coo.row[~out], coo.col[~out])), shape=full.shape)
    held = sp.csr_matrix((coo.data[out], (coo.row[out], coo.col[out])), shape=full.shape)
    m = PureSVD(rank=8, lambda_=5.0, method=method, precision=precision, rng=1)
    emb = m.fit_transform(train, n_iter=10, convergence_tol=-1)
    return m, emb, train, held


@pytest.mark.parametrize("precision,method", [("double", "svd"), ("double", "impute"), ("float", "svd")])
def test_puresvd_on_the_device(precision, method):
    from rsparse_amd.metrics import ap_k, ndcg_k
    m, emb, train, held = fitted(precision, method)
    tol = 1e-10 if precision == "double" else 2e-5
    v, d = m.svd.v.astype(np.float64), m.svd.d
    scale = np.abs(train @ v).max()
    assert np.abs(emb - train @ v).max() <= tol * scale               # x %*% v
    assert np.allclose(m.components, (v * d).T, rtol=1e-6 if precision == "float" else 1e-15)
    rows = train[100:140]
    assert np.abs(m.transform(rows) - rows @ v).max() <= tol * scale
    top = m.predict(train[:50], 10)
    dense = (train[:50] @ v) @ (v * d).T
    dense[train[:50].toarray() != 0] = -np.inf
    want = -np.sort(-dense, axis=1)[:, :10]
    assert np.abs(top.scores - want).max() <= tol * np.abs(want).max()                     # scores, not indices
    got = m.evaluate(train, held, 10)
    full_top = m.predict(train, 10)
    assert np.allclose(got["ap"], ap_k(full_top, held), equal_nan=True, rtol=1e-12)
    assert np.allclose(got["ndcg"], ndcg_k(full_top, held), equal_nan=True, rtol=1e-12)
    assert np.nanmean(got["ap"]) > 0.05
    q = np.array([0, 10, 49, 257])
    sim = m.similar_items(q, k=5)
    with np.errstate(invalid="ignore"):
        n = v / np.linalg.norm(v, axis=1, keepdims=True)
    c = np.nan_to_num(n[q] @ n.T, nan=-np.inf)                       # (items without a direction are never returned)
    c[np.arange(q.size), q] = -np.inf
    assert np.allclose(sim.scores, -np.sort(-c, axis=1)[:, :5], rtol=0, atol=1e-9 if precision == "double" else 1e-5)
    neg = m.evaluate(train, held, 10, negatives=99, seed=7)
    again = m.evaluate(train, held, 10, negatives=99, seed=7)
    assert np.array_equal(neg["ap"], again["ap"], equal_nan=True)
    assert np.nanmean(neg["ap"]) > np.nanmean(got["ap"])              # 99 sampled negatives are an easier field than the catalogue
    with pytest.raises(NotImplementedError):
        m.explain(train[:2], sp.csr_matrix(([1.0], ([0], [1])), shape=(2, train.shape[1])))


def test_puresvd_inherited_surface_runs():
    m, _, train, held = fitted("double", "svd")
    cand = sp.csr_matrix(held[:30] + train[:30])
    top = m.predict(train[:30], 5, not_recommend=None, candidates=cand, items_exclude=[3])
    sc = m.score(train[:30], cand)
    assert top.shape == (30, 5) and not np.any(np.asarray(top) == 3)
    dense = sc.toarray()
    row0 = np.asarray(top)[0]
    assert np.allclose(top.scores[0][row0 >= 0], dense[0][row0[row0 >= 0]], rtol=1e-12)
    div = m.predict(train[:30], 5, diversify=0.5)
    assert div.shape == (30, 5)
    vals = m.evaluate_values(train[:30], held[:30])
    ranks = m.evaluate_ranks(train[:30], held[:30])
    assert np.isfinite(vals["rmse"]) and 0.5 < ranks["auc"] <= 1.0
    wide = m.evaluate(train[:30], held[:30], 10, metrics=("recall", "diversity"))
    assert set(wide) >= {"recall", "diversity"}
