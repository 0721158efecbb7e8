"""The iALS++ block step on the device (wrmf_subspace.hip) against the float64 definition of rsparse_amd/ialspp.py.

The bounds are multiples of YARDSTICKS measured on an MI355X with the EXISTING exact fp32 path, never with the code under test
(profiles/subspace/README.md has the runs):
  ROW_YARD   the largest relative row error (row_scale below says relative to what) of one Cholesky half of
             `als_implicit(solver = cholesky, precision = "float")` against the float64 normal-equation solve, on the inputs of
             the single-block test below (k = 32 and 64)
  FIT_YARD   the relative Frobenius error of a 3-iteration `WRMF(solver="cholesky", precision="float")` fit against a float64 fit of
             the same length, on the matrix of the fit test below
The block step and the single-block half are held to 4 x ROW_YARD (the step adds the rounding of D and of e to the same assembly and
factorisation), the 3-iteration fit to 8 x FIT_YARD (DESIGN.md 3.37's practice for iterated error)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import IALSpp, _lib
from rsparse_amd.ialspp import ialspp_block_reference, ialspp_fit_reference
from test_bpr import backend, bits_equal
from test_ease_host import brute_lists

pytestmark = pytest.mark.gpu

ROW_YARD = 4.179e-07   # (k = 32, the row of 257 entries; k = 64: 4.171e-07)
FIT_YARD = 8.008e-06   # (U; V: 7.194e-06)
ROW_BOUND, FIT_BOUND = 4 * ROW_YARD, 8 * FIT_YARD

LONG, SEG = _lib.SUBSPACE_LONG_ROW, _lib.SUBSPACE_SEGMENT
# (the last row: three workgroup segments, the third one short)
LENGTHS = (0, 1, 2, 31, 32, 33, 64, 65, LONG - 1, LONG, LONG + 1, 2 * SEG + 5)


@functools.lru_cache(maxsize=None)
def problem(k):
    """the CSR of LENGTHS (confidences in [1, 40], one in 17 below 1), H (m x k) and a random W, all as the device sees them"""
    rng = np.random.default_rng(k)
    m = max(LENGTHS) + 59
    ip = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int32)
    idx = np.concatenate([np.sort(rng.choice(m, size=n, replace=False)) for n in LENGTHS]).astype(np.int32)
    c = rng.uniform(1.0, 40.0, idx.size)
    c[::17] = rng.uniform(0.25, 1.0, c[::17].size)
    H = (0.1 * rng.standard_normal((m, k))).astype(np.float32)
    W = (0.1 * rng.standard_normal((len(LENGTHS), k))).astype(np.float32)
    return ip, idx, c.astype(np.float32), H, W


def exact_rows(ip, idx, c, H, lam):
    """the float64 normal-equation solve of every row"""
    H, c = H.astype(np.float64), c.astype(np.float64)
    G = H.T @ H + lam * np.eye(H.shape[1])
    out = np.zeros((ip.size - 1, H.shape[1]))
    for u in range(ip.size - 1):
        Hs, cu = H[idx[ip[u]:ip[u + 1]]], c[ip[u]:ip[u + 1]]
        out[u] = np.linalg.solve(G + (Hs * (cu - 1.0)[:, None]).T @ Hs, cu @ Hs)
    return out


def row_scale(ref, start):
    """per row: max(|ref row|, |the row the step started from|).  A step w <- w - delta rounds delta at ITS size, which is the
    start's wherever the start is the larger of the two: eps |start| is the floor of any fp32 step, so that is what a row's error
    is relative to -- for the yardstick (an exact solve, which has no start) as for the code under test"""
    return np.maximum(np.linalg.norm(ref, axis=1), np.linalg.norm(start.astype(np.float64), axis=1))


def row_err(got, ref, scale):
    return np.linalg.norm(got.astype(np.float64) - ref, axis=1) / scale


def upload(ip, idx, c):
    be = backend()
    return be.to_device(ip, torch.int32), be.to_device(idx, torch.int32), be.to_device(c, torch.float32)


@pytest.mark.parametrize("lam", (1e-3, 0.1))
@pytest.mark.parametrize("where", ("first", "interior", "last"))
@pytest.mark.parametrize("b", (32, 64))
@pytest.mark.parametrize("k", (64, 96, 130, 256))
def test_block_step_against_the_definition(k, b, where, lam):
    ip, idx, c, H, W = problem(k)
    be = backend()
    nb = -(-k // b)
    c0 = b * {"first": 0, "interior": nb // 2, "last": nb - 1}[where]
    width = min(b, k - c0)
    rows = np.repeat(np.arange(W.shape[0]), np.diff(ip))
    H64, W64 = H.astype(np.float64), W.astype(np.float64)
    G64 = H64.T @ H64
    e64 = np.einsum("ij,ij->i", W64[rows], H64[idx])
    refW, refE = ialspp_block_reference(ip, idx, c, H, G64, c0, width, lam, W, e64.astype(np.float32))
    dH, dW, G = be.to_device(H, torch.float32), be.to_device(W, torch.float32), be.to_device(G64, torch.float32)
    e = be.to_device(e64, torch.float32)
    D = torch.matmul(dW, G[:, c0:c0 + width])
    be.subspace_block(*upload(ip, idx, c), dH, c0, width, b, G[c0:c0 + width, c0:c0 + width], D, lam, dW, e)
    assert be.numeric_counts() == (0, 0)
    got, gotE = dW.cpu().numpy(), e.cpu().numpy().astype(np.float64)
    outside = np.ones(k, dtype=bool)
    outside[c0:c0 + width] = False
    assert bits_equal(got[:, outside], W[:, outside])   # W outside the slice keeps its bits
    scale = row_scale(refW, W)
    err_w = row_err(got[:, c0:c0 + width], refW[:, c0:c0 + width], scale)
    # e against the size of what it is the product of: |w_u| max |h_i|
    err_e = np.abs(gotE - refE) / (scale[rows] * np.linalg.norm(H64, axis=1).max())
    worst_e = np.array([err_e[ip[u]:ip[u + 1]].max(initial=0.0) for u in range(W.shape[0])])
    print("k %d b %d c0 %d width %d lam %g: row errors w %s e %s" % (k, b, c0, width, lam, np.array2string(err_w, precision=2),
                                                                      np.array2string(worst_e, precision=2)))
    assert np.isfinite(got).all() and (err_w <= ROW_BOUND).all(), (LENGTHS[int(err_w.argmax())], err_w.max() / ROW_BOUND)
    assert (worst_e <= ROW_BOUND).all(), (LENGTHS[int(worst_e.argmax())], worst_e.max() / ROW_BOUND)


@pytest.mark.parametrize("k", (32, 64))
def test_single_block_half_is_the_exact_solve(k):
    ip, idx, c, H, W = problem(k)
    be, lam = backend(), 0.1
    ref = exact_rows(ip, idx, c, H, lam)
    model = IALSpp(rank=k, lambda_=lam, block=k)
    dW, dH = be.to_device(W, torch.float32), be.to_device(H, torch.float32)
    model._half(be, upload(ip, idx, c), dW, dH, torch.empty((k, k), dtype=torch.float32, device=dW.device))
    assert be.numeric_counts() == (0, 0)
    err = row_err(dW.cpu().numpy(), ref, row_scale(ref, W))   # (the empty row too: its exact solve is 0)
    print("k %d: row errors of the single-block half %s" % (k, np.array2string(err, precision=2)))
    assert (err <= ROW_BOUND).all(), (LENGTHS[int(err.argmax())], err.max() / ROW_BOUND)


def fit_problem():
    """200 x 300, user 5 holds every item but the all-zero column 17, user 9 is empty; the initial factors"""
    rng = np.random.default_rng(3)
    d = (rng.random((200, 300)) < 0.06) * rng.uniform(1.0, 40.0, (200, 300))
    d[5] = rng.uniform(1.0, 40.0, 300)
    d[9] = 0.0
    d[:, 17] = 0.0
    U0, V0 = ((0.01 * rng.standard_normal((n, 128))).astype(np.float32) for n in d.shape)
    return sp.csr_matrix(d), U0, V0


def rel_fro(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))


def test_fit_lists_and_empty_rows():
    x, U0, V0 = fit_problem()

    def fit():
        m = IALSpp(rank=128, lambda_=0.1, block=64)
        m._init_user_factors, m.components = U0, V0.T.copy()
        return m, m.fit_transform(x, 3)

    (m, U), (m2, U2) = fit(), fit()
    assert bits_equal(U, U2) and bits_equal(m.components, m2.components)
    V = m.components.T
    assert np.isfinite(U).all() and np.isfinite(V).all()
    rU, rV = ialspp_fit_reference(x, U0, V0, 3, 64, 0.1)
    print("rel_fro of the fit: U %.3g, V %.3g" % (rel_fro(U, rU), rel_fro(V, rV)))
    assert rel_fro(U, rU) <= FIT_BOUND and rel_fro(V, rV) <= FIT_BOUND
    new = x[20:40]   # (ordinary users: neither the full row nor the empty one)
    emb = m.transform(new)
    top = m.predict(new, 10)
    lists, _ = brute_lists(emb.astype(np.float64) @ V.astype(np.float64).T, 10, new, ())
    assert np.array_equal(np.asarray(top), lists)
