"""Logistic MF on the device (wrmf_lmf.hip) against the float64 definition of rsparse_amd/lmf.py.  The bounds are those derived in
DESIGN.md 3.37 (eps = 2^-24): none is scaled from an observed device error, except FIT_BOUND, which is 8 x the rel_fro measured
on an MI355X against the float64 definition (profiles/lmf/README.md), as the design note explains."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import LogisticMF, _lib
from rsparse_amd.lmf import lmf_dense_reference, lmf_fit_reference, lmf_half_reference, softplus
from test_bpr import backend, bits_equal, planted
from test_ease_host import brute_lists

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
FIT_BOUND = 8 * 1.24e-6   # 8 x the measured rel_fro of the fit below


def dev(a, dtype=torch.float32):
    return backend().to_device(a, dtype)


def dense_bounds(A, B):
    """(the bound of D per element, the bound of a row's softplus sum) for fp32 operands A, B"""
    n_str, K = B.shape
    amax = (np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64).T).max()
    sp_max = max(1.0, softplus(A.astype(np.float64) @ B.astype(np.float64).T).max())
    return (EPS * (K * amax / 4 + 4 + n_str) * np.abs(B).astype(np.float64).sum(axis=0)[None, :],
            EPS * n_str * (K * amax + 4 * sp_max))


def check_dense(A, B, slice_rows, want_softplus):
    D, s = backend().lmf_dense(dev(A), dev(B), slice_rows, want_softplus)
    n_slices = -(-B.shape[0] // slice_rows) if slice_rows else D.shape[0]
    assert D.shape == (n_slices,) + A.shape
    tol_d, tol_s = dense_bounds(A, B)
    got = D.cpu().numpy().astype(np.float64).sum(axis=0)
    err = np.abs(got - lmf_dense_reference(A, B))
    assert np.isfinite(got).all() and (err <= tol_d).all(), (A.shape, B.shape, slice_rows, (err / tol_d).max())
    if want_softplus:
        ref = softplus(A.astype(np.float64) @ B.astype(np.float64).T).sum(axis=1)
        err = np.abs(s.cpu().numpy().sum(axis=0) - ref)   # (a missing padding mask is off by multiples of log 2)
        assert (err <= tol_s).all(), (A.shape, B.shape, slice_rows, err.max() / tol_s)


@pytest.mark.parametrize("slice_rows", (0, 32, 96))
@pytest.mark.parametrize("K", (3, 32, 33, 64, 97, 128))
def test_dense_term_against_the_definition(K, slice_rows):
    rng = np.random.default_rng(K)
    for n_rows in (1, 32, 33, 129):
        for n_str in (1, 31, 33, 65, 200):
            A, B = ((0.3 * rng.standard_normal((n, K))).astype(np.float32) for n in (n_rows, n_str))
            check_dense(A, B, slice_rows, want_softplus=n_rows != 32)   # (n_rows = 32: the instantiation without the sums)


def test_dense_term_saturates_without_nan():
    rng = np.random.default_rng(1)
    A, B = ((0.3 * rng.standard_normal((n, 32))).astype(np.float32) for n in (33, 65))
    s = np.abs(A[:3].astype(np.float64) @ B.T.astype(np.float64)).max(axis=1)
    A[:3] *= (300.0 / s)[:, None].astype(np.float32)   # both tails: |s| reaches 300 in these rows
    assert np.abs(A[:3].astype(np.float64) @ B.T.astype(np.float64)).max() > 290
    check_dense(A, B, 0, True)
    a, b = backend().lmf_dense(dev(A), dev(B)), backend().lmf_dense(dev(A), dev(B))
    assert bits_equal(a[0].cpu().numpy(), b[0].cpu().numpy())


LENGTHS = (0, 1, 15, 16, 17, 64, 65, 2049)   # (the last one holds every column: the workgroup path, > LMF_LONG_ROW)


@pytest.mark.parametrize("n_slices", (1, 3))
@pytest.mark.parametrize("lam", (0.0, 0.6))
@pytest.mark.parametrize("K", (3, 33, 128))
def test_step_against_the_definition(K, lam, n_slices):
    assert LENGTHS[-1] > _lib.LMF_LONG_ROW >= LENGTHS[-2]
    rng = np.random.default_rng(100 + K)
    n_cols, n_rows, rank, alpha, lr = 2049, len(LENGTHS), K - 2, 2.0, 0.7
    cols = [np.sort(rng.choice(n_cols, size=L, replace=False)) for L in LENGTHS]
    ip = np.concatenate([[0], np.cumsum(LENGTHS)])
    idx, x = np.concatenate(cols), (0.5 + 2.5 * rng.random(int(ip[-1]))).astype(np.float32)
    A, B = ((0.3 * rng.standard_normal((n, K))).astype(np.float32) for n in (n_rows, n_cols))
    A[:, K - 1] = 1.0
    aA = rng.random((n_rows, K)) * 0.1
    aA[0] = 0.0
    # D: the definition's, rounded to fp32 and cut into slices that sum to it; the empty row's is zero (g = 0 there at lambda = 0)
    D = lmf_dense_reference(A, B).astype(np.float32)
    D[0] = 0.0
    parts = [(0.1 * rng.standard_normal(D.shape)).astype(np.float32) for _ in range(n_slices - 1)]
    parts[1:1] = [(D - sum(parts)).astype(np.float32)] if parts else [D]
    parts = np.stack(parts)
    parts[:, 0] = 0.0
    Dsum = parts.astype(np.float64).sum(axis=0)
    spl = rng.random((n_slices, n_rows))
    c = alpha * x.astype(np.float64)
    ref_A, ref_a, _ = lmf_half_reference(ip, idx, c, A, aA, B, rank, K - 1, lr, lam, D=Dsum)
    dA, da = dev(A), dev(aA, torch.float64)
    rows = backend().lmf_step(dev(ip, torch.int32), dev(idx, torch.int32), dev(x), alpha, dA, da, dev(B), dev(parts), rank, K - 1, lr, lam,
                              softplus=dev(spl, torch.float64), want_rowsums=lam > 0)   # (lambda = 0: the instantiation without them)
    got_A, got_a = dA.cpu().numpy(), da.cpu().numpy()
    assert bits_equal(got_A[:, K - 1], A[:, K - 1])
    if lam == 0:
        assert bits_equal(got_A[0], A[0]) and bits_equal(got_a[0], aA[0])
    assert (np.abs(got_A.astype(np.float64) - ref_A.astype(np.float64)) <= np.spacing(np.abs(ref_A))).all()
    # a' = a + g^2, |g| <= G = sum |w B| + |D| + lambda |A|: every sum of L + K + 8 double operations
    S = A.astype(np.float64) @ B.astype(np.float64).T
    W = np.zeros_like(S)
    r_of = np.repeat(np.arange(n_rows), LENGTHS)
    W[r_of, idx] = c / (1.0 + np.exp(S[r_of, idx]))
    G = W @ np.abs(B).astype(np.float64) + np.abs(Dsum) + lam * np.abs(A)
    scale = 2.0 ** -50 * (np.asarray(LENGTHS)[:, None] + K + 8)
    assert (np.abs(got_a - ref_a) <= scale * (aA + G * G)).all()
    if lam > 0:
        s = S[r_of, idx]
        terms = c * s - c * softplus(s)
        ref = np.bincount(r_of, weights=terms, minlength=n_rows) - spl.sum(axis=0)
        mag = np.bincount(r_of, weights=np.abs(c * s) + c * softplus(s), minlength=n_rows) + spl.sum(axis=0)
        assert (np.abs(rows.cpu().numpy() - ref) <= scale[:, 0] * mag).all()


def rel_fro(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))


def test_fit_fold_in_and_lists():
    """Measured on an MI355X against the float64 definition: rel_fro = 1.24e-6 (U) and 1.10e-6 (V) after 3 iterations
    (FIT_BOUND is 8 x the larger)."""
    x = planted()
    make = lambda: LogisticMF(rank=16, alpha=2.0, learning_rate=1.0, lambda_=0.6, transform_iter=20, rng=5)
    m, m2 = make(), make()
    U, U2 = m.fit_transform(x, 3, trace=True), m2.fit_transform(x, 3)
    assert bits_equal(U, U2) and bits_equal(m.components, m2.components) and bits_equal(m.item_adagrad, m2.item_adagrad)
    K, be = 18, backend()
    U0, V0 = (np.zeros((n, K), dtype=np.float32) for n in x.shape)
    for F, stream, n, one in ((U0, 0, x.shape[0], K - 1), (V0, 1, x.shape[1], K - 2)):
        F[:, :16] = be.init_factors(m.seed, stream, n, 16, torch.float32).cpu().numpy()
        F[:, one] = 1.0
    c_ui = sp.csr_matrix(x, dtype=np.float64) * 2.0
    rU, rV, raU, raV, rtrace = lmf_fit_reference(c_ui, U0, V0, 3, 16, 1.0, 0.6)
    V = m.components.T
    print("rel_fro of the fit: U %.3g, V %.3g, aU %.3g" % (rel_fro(U, rU), rel_fro(V, rV), rel_fro(m.user_adagrad, raU)))
    assert rel_fro(U, rU) <= FIT_BOUND and rel_fro(V, rV) <= FIT_BOUND
    assert bits_equal(U[:, K - 1], U0[:, K - 1]) and bits_equal(V[:, K - 2], V0[:, K - 2])
    assert bits_equal(m.user_bias, U[:, 16]) and bits_equal(m.item_bias, V[:, 17])
    # the trace: the first entry is taken at the very same factors -- the dense bound per row plus the double sums; a later one
    # at factors that differ by at most FIT_BOUND on either side, which moves a score by at most 2 FIT_BOUND max|u| max|v| and a
    # term of the log-likelihood by (1 + c) times that
    assert len(m.trace) == len(rtrace) == 6 and m2.trace == []
    pairs = x.shape[0] * x.shape[1] + c_ui.sum()
    direct = x.shape[0] * dense_bounds(U0, V0)[1] + 2.0 ** -50 * pairs
    assert abs(m.trace[0] - rtrace[0]) <= direct
    norms = np.linalg.norm(rU, axis=1).max() * np.linalg.norm(rV, axis=1).max()
    for h in range(1, 6):
        assert abs(m.trace[h] - rtrace[h]) <= 2 * direct + 2 * FIT_BOUND * norms * pairs, h
    # the fold-in of 20 rows against the definition's, from the device's items
    new = x[8:28]
    emb = m.transform(new)
    ref = lmf_fit_reference(sp.csr_matrix(new, dtype=np.float64) * 2.0, np.tile(np.eye(1, K, K - 1, dtype=np.float32), (20, 1)), V, 20, 16,
                            1.0, 0.6, update_items=False)[0]
    print("rel_fro of the fold-in: %.3g" % rel_fro(emb, ref))
    assert rel_fro(emb, ref) <= FIT_BOUND and bits_equal(emb[:, K - 1], ref[:, K - 1])
    # the lists: a brute-force ordering of U V' from the device's own factors (the products in double, as `predict` scores)
    top = m.predict(new, 10)
    lists, _ = brute_lists(emb.astype(np.float64) @ V.astype(np.float64).T, 10, new, ())
    assert np.array_equal(np.asarray(top), lists)
    sim = m.similar_items([3, 7], 5)
    Vl = V[:, :16].astype(np.float64) / np.linalg.norm(V[:, :16].astype(np.float64), axis=1, keepdims=True)
    cos = Vl[[3, 7]] @ Vl.T
    cos[[0, 1], [3, 7]] = -np.inf
    assert np.array_equal(np.asarray(sim), np.argsort(-cos, axis=1, kind="stable")[:, :5])
    with pytest.raises(_lib.UnsupportedOnDevice):
        m.explain(new, sp.csr_matrix(new.shape))
