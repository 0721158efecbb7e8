"""The numpy definition of iALS++ (rsparse_amd/ialspp.py) and the refusals of `IALSpp`; no GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

from rsparse_amd import IALSpp, _lib
from rsparse_amd.ialspp import ialspp_block_reference, ialspp_half_reference, ialspp_objective

LAM = 0.1


def small(n=40, m=60, seed=0):
    rng = np.random.default_rng(seed)
    x = sp.csr_matrix((rng.random((n, m)) < 0.15) * rng.uniform(0.5, 40.0, (n, m)))   # (some confidences below 1)
    x[3] = 0.0                                                                          # an empty row
    x.eliminate_zeros()
    return x, rng


def test_single_block_half_is_the_exact_solve():
    x, rng = small()
    k = 10
    H, W0 = 0.3 * rng.standard_normal((60, k)), rng.standard_normal((40, k))
    W = ialspp_half_reference(x.indptr, x.indices, x.data, H, W0, k, LAM)
    G = H.T @ H + LAM * np.eye(k)
    for u in range(40):
        Hs, c = H[x[u].indices], x[u].data
        ref = np.linalg.solve(G + (Hs * (c - 1.0)[:, None]).T @ Hs, c @ Hs)
        assert np.abs(W[u] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert np.abs(W[3]).max() <= 1e-12   # (the empty row: the exact solve of a zero right-hand side, w - A^-1 (A w))


def test_objective_never_increases_over_a_block():
    x, rng = small(seed=1)
    k, b = 10, 4
    U, V = 0.1 * rng.standard_normal((40, k)), 0.1 * rng.standard_normal((60, k))
    xt = sp.csr_matrix(x.T)
    xt.sort_indices()
    last, widths = ialspp_objective(x, U, V, LAM), []
    for _ in range(3):
        for side in ("items", "users"):
            m, W, H = (xt, V, U) if side == "items" else (x, U, V)
            G = H.T @ H
            rows = np.repeat(np.arange(W.shape[0]), np.diff(m.indptr))
            e = np.einsum("ij,ij->i", W[rows], H[m.indices])
            for c0 in range(0, k, b):
                W, e = ialspp_block_reference(m.indptr, m.indices, m.data, H, G, c0, min(b, k - c0), LAM, W, e)
                U, V = (U, W) if side == "items" else (W, V)
                now = ialspp_objective(x, U, V, LAM)
                assert now <= last * (1 + 1e-13), (side, c0, now, last)
                last = now
                widths.append(min(b, k - c0))
            assert np.abs(e - np.einsum("ij,ij->i", W[rows], H[m.indices])).max() <= 1e-12   # (the running predictions stay true)
    assert widths[:3] == [4, 4, 2]


def test_refusals():
    for kw in ({"precision": "double"}, {"rank": 257}, {"block": 48}, {"feedback": "explicit"}, {"with_user_item_bias": True},
               {"with_global_bias": True}):
        with pytest.raises(_lib.UnsupportedOnDevice):
            IALSpp(**kw)
    with pytest.raises(ValueError):
        IALSpp(solver="cholesky")
    IALSpp(rank=256, block=32)
    x = sp.csr_matrix(np.array([[1.0, 0.0], [0.0, -2.0]]))
    with pytest.raises(ValueError):
        IALSpp(rank=4).fit_transform(x, 1)
