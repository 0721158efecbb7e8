"""The numpy definition of logistic MF (rsparse_amd/lmf.py) and the refusals of `LogisticMF`; no GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

from rsparse_amd import LogisticMF, _lib
from rsparse_amd.lmf import lmf_half_reference, lmf_loglik_reference

RANK, K, LAM = 3, 5, 0.6


def small():
    rng = np.random.default_rng(0)
    m = sp.csr_matrix(((rng.random((7, 9)) < 0.4) * rng.integers(1, 4, (7, 9))).astype(np.float64))
    A, B = 0.3 * rng.standard_normal((7, K)), 0.3 * rng.standard_normal((9, K))
    A[:, K - 1] = B[:, K - 2] = 1.0
    return m, 2.0 * m.data, A, B


def test_gradient_is_the_finite_difference_of_the_log_likelihood():
    m, c, A, B = small()
    ll = lambda X: lmf_loglik_reference(m.indptr, m.indices, c, X, B, RANK, LAM)
    g = lmf_half_reference(m.indptr, m.indices, c, A, np.zeros(A.shape), B, RANK, -1, 1.0, LAM)[2]
    h, num = 1e-6, np.zeros(A.shape)
    for r, col in np.ndindex(*A.shape):
        d = np.zeros(A.shape)
        d[r, col] = h
        num[r, col] = (ll(A + d) - ll(A - d)) / (2 * h)
    assert np.abs(num - g).max() <= 1e-6 * max(1.0, np.abs(g).max())


def test_frozen_coordinate_and_unregularised_biases():
    m, c, A, B = small()
    a0 = np.full(A.shape, 0.25)
    new, a2, g = lmf_half_reference(m.indptr, m.indices, c, A, a0, B, RANK, K - 1, 0.5, LAM)
    assert (g[:, K - 1] == 0).all() and np.array_equal(new[:, K - 1], A[:, K - 1]) and np.array_equal(a2[:, K - 1], a0[:, K - 1])
    assert np.allclose(new, A + 0.5 * g / np.sqrt(a0 + g * g), rtol=1e-15) and np.array_equal(a2, a0 + g * g)
    g0 = lmf_half_reference(m.indptr, m.indices, c, A, a0, B, RANK, K - 1, 0.5, 0.0)[2]
    assert np.allclose(g0[:, :RANK] - g[:, :RANK], LAM * A[:, :RANK], rtol=1e-12) and np.array_equal(g0[:, RANK:], g[:, RANK:])


def test_refusals():
    with pytest.raises(_lib.UnsupportedOnDevice):
        LogisticMF(rank=8, precision="double")
    with pytest.raises(_lib.UnsupportedOnDevice):
        LogisticMF(rank=127)
    LogisticMF(rank=126)
    for bad in (-1.0, 0.0):
        x = sp.csr_matrix(np.array([[1.0, 0.0], [0.0, 2.0]]))
        x.data[1] = bad
        with pytest.raises(ValueError):
            LogisticMF(rank=4).fit_transform(x, 1)
