"""`HipBackend.spd_inverse` (wrmf_spdinv.hip, the blocked symmetric sweep) on the device: per element against numpy's inverse, with
the torch route of `ease.spd_inverse` on the same input as the yardstick, and `EASE(inverse="sweep")` against the definition."""
import functools

import numpy as np
import pytest
import torch

from rsparse_amd import EASE, _lib
from rsparse_amd.ease import ease_recommend_reference, spd_inverse
from test_ease import backend, fixture_inverse, movielens_csr, planted

pytestmark = pytest.mark.gpu


def ridge_gram(n, lambda_, seed=0):
    h = (np.random.default_rng(seed + n).random((3 * n + 5, n)) < 0.2).astype(np.float64)
    return h.T @ h + lambda_ * np.eye(n)


def sweep(A, pad=0):
    """the entry on a copy of A with `pad` more columns per row (filled with 7) -> (P, the padding as it came back)"""
    n = A.shape[0]
    buf = torch.full((n, n + pad), 7.0, dtype=torch.float64, device=backend().device)
    buf[:, :n] = torch.from_numpy(A)
    P = backend().spd_inverse(buf[:, :n])
    assert P.data_ptr() == buf.data_ptr()   # (in place)
    return P.cpu().numpy(), buf[:, n:].cpu().numpy()


def yardstick(A):
    """the parent's path on the same input: `ease.spd_inverse` (scipy's Cholesky inverse where torch has no device solver)"""
    P = spd_inverse(backend().to_device(A, torch.float64)).cpu().numpy()
    if spd_inverse.on_host:
        from scipy.linalg import cho_factor, cho_solve
        P = cho_solve(cho_factor(A), np.eye(A.shape[0]))
    return P


@pytest.mark.parametrize("lambda_", [0.01, 500.0])
@pytest.mark.parametrize("n,pad", [(1, 0), (2, 0), (63, 0), (64, 0), (65, 0), (127, 0), (128, 0), (129, 0), (200, 3), (333, 0)])
def test_inverse_per_element_against_the_torch_route(n, pad, lambda_):
    """residual max |P A - I| and error max |P - P_ref| / max |P_ref| (P_ref = np.linalg.inv), each at most 4 x the torch route's on
    the same input: both are backward-stable SPD inverses, their errors differ by a small constant and not by the condition number
    (profiles/spd_inverse/README.md has the measured ratios).  Exactly symmetric; a second call returns the same bits; padding
    columns come back untouched."""
    A = ridge_gram(n, lambda_)
    P_ref, eye = np.linalg.inv(A), np.eye(n)
    P, padding = sweep(A, pad)
    Y = yardstick(A)
    res = lambda Q: np.abs(Q @ A - eye).max()
    err = lambda Q: np.abs(Q - P_ref).max() / np.abs(P_ref).max()
    print("n %d lambda %g: residual %.3g (torch %.3g), error %.3g (torch %.3g)" % (n, lambda_, res(P), res(Y), err(P), err(Y)))
    assert np.isfinite(P).all() and res(P) <= 4 * res(Y) and err(P) <= 4 * err(Y)
    assert np.array_equal(P, P.T) and (padding == 7.0).all()
    assert np.array_equal(sweep(A, pad)[0], P)


@pytest.mark.parametrize("name", ["minus_identity", "zero_column"])
def test_a_matrix_that_is_not_positive_definite_is_a_numeric_error(name):
    A = -np.eye(130)
    if name == "zero_column":
        A = ridge_gram(130, 0.0)
        A[:, 70] = A[70, :] = 0.0   # (an item without users, behind the first pivot block)
    with pytest.raises(_lib.RsparseHipError) as e:
        sweep(A)
    assert e.value.code == _lib.ERR_NUMERIC
    good = ridge_gram(130, 1.0)
    assert np.abs(sweep(good)[0] @ good - np.eye(130)).max() < 1e-12


@functools.lru_cache(maxsize=None)
def fitted_sweep():
    return EASE(500.0, precision="double", backend=backend(), inverse="sweep").fit(movielens_csr()[:900])


def test_fit_with_the_sweep_meets_the_tolerance_of_the_torch_fit():
    """the bound of test_ease.test_fitted_weights, on its problem: tol = 2 (33 n r_ref max|P|) (1 + |B_ref|) / P_jj"""
    from rsparse_amd.ease import ease_weights_reference
    A, P, r_ref = fixture_inverse(500.0)
    B_ref, B = ease_weights_reference(A), fitted_sweep().B
    tol = 2 * (33 * A.shape[0] * r_ref * np.abs(P).max()) * (1 + np.abs(B_ref)) / np.diag(P)[None, :]
    assert B.dtype == np.float64 and (np.diag(B) == 0).all() and (np.abs(B - B_ref) <= tol).all()
    test = movielens_csr()[900:]
    top = fitted_sweep().predict(test, 10)
    ref = ease_recommend_reference(test, B, 10, test)
    assert np.array_equal(np.asarray(top), ref[0]) and np.array_equal(top.scores, ref[1])


def test_singular_gram_is_a_numeric_error_with_the_sweep():
    with pytest.raises(_lib.RsparseHipError) as e:
        EASE(0.0, backend=backend(), inverse="sweep").fit(planted())
    assert e.value.code == _lib.ERR_NUMERIC and "lambda = 0" in str(e.value)
