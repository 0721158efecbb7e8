"""FTRL on the device (wrmf_ftrl.hip behind rsparse_hip_ftrl_*) against the numpy definition of rsparse_amd/ftrl.py, bit for bit in
both precisions: the forward pass at every row-length edge and every group width, one step at every segment-length edge, whole fits
through the public class, the host-array forms, the refusals of the C boundary."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import FTRL, _lib
from rsparse_amd.fm import canonical_design, step_rows
from rsparse_amd.ftrl import (CLIP_GRAD, ftrl_fit_reference, ftrl_forward_reference, ftrl_step_reference, ftrl_weights_reference)
from test_bpr import DTYPES, TORCH, backend, bits_equal
from test_fm import rows_of, step_rows_matrix

pytestmark = pytest.mark.gpu

LONG = _lib.FTRL_LONG_ROW
LENGTHS = (0, 1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 129, LONG, LONG + 1)
D, ZERO0 = LONG + 88, LONG + 24                  # the columns from ZERO0 have |z| <= l1: their weight is +0.0
ALPHA, BETA, LAM, RATIO = 0.1, 0.5, 0.3, 0.5
L1, L2 = LAM * RATIO, LAM * (1.0 - RATIO)
WIDTH_BAND = {0: 64, 100: 16, 600: 4}            # fillers -> the group width the header's rule picks (2 G >= nnz / n_rows)


def targets(n, family, rng):
    y = {"binomial": lambda: (rng.random(n) < 0.5).astype(np.float64), "gaussian": lambda: rng.normal(size=n),
         "poisson": lambda: rng.poisson(2.0, size=n).astype(np.float64)}[family]()
    return y, rng.random(n) + 0.5


def state(d, dt, rng):
    """a random non-trivial (z, n) -> the (d, 2) pairs; the columns from ZERO0 (and some others) have |z| <= l1"""
    z, n = rng.normal(size=d), 4.0 * rng.random(d)
    z[ZERO0:] = 0.1 * rng.random(max(d - ZERO0, 0))
    return np.ascontiguousarray(np.stack([z, n], axis=1).astype(dt))


def device(m, zn, *more):
    be = backend()
    csr = (be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32), be.to_device(m.data, TORCH[m.dtype.type]))
    return csr, be.to_device(zn, TORCH[zn.dtype.type]), [be.to_device(a, torch.float64) for a in more]


@functools.lru_cache(maxsize=None)
def forward_rows(fillers):
    rng = np.random.default_rng(3)
    scale = [1.0] * len(LENGTHS)
    scale[LENGTHS.index(129)] = 1e4                                        # |raw| passes 40 there: the clamp of E
    edge = rows_of(LENGTHS * 2 + (2,) * fillers, ZERO0, rng, scale * 2 + [1.0] * fillers)
    edge.resize(edge.shape[0], D)
    minus = sp.csr_matrix((-1.0 - rng.random(68), np.r_[ZERO0:ZERO0 + 4, ZERO0:ZERO0 + 64], [0, 4, 68]), shape=(2, D))   # terms of -0.0
    return sp.vstack([edge, minus]).tocsr()


@pytest.mark.parametrize("fillers", sorted(WIDTH_BAND))
@pytest.mark.parametrize("dropout", [0.0, 0.3])
@pytest.mark.parametrize("family", ["binomial", "gaussian", "poisson"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_forward_equals_the_definition(precision, family, dropout, fillers):
    dt, rng = DTYPES[precision], np.random.default_rng(fillers + 1)
    m = canonical_design(forward_rows(fillers), dt)
    n = m.shape[0]
    mean = m.nnz / n
    assert {True: 4, False: 16 if mean <= 32 else 64}[mean <= 8] == WIDTH_BAND[fillers]
    zn = state(D, dt, rng)
    y, om = targets(n, family, rng)
    csr, dzn, (dy, dom) = device(m, zn, y, om)
    glm = (family, ALPHA, BETA, LAM, RATIO)
    clamped = False
    for step in range(3):
        rows = step_rows(n, step, 3)
        raw, p, _ = ftrl_forward_reference(m.indptr, m.indices, m.data, rows, zn[:, 0], zn[:, 1], family, ALPHA, BETA, L1, L2, dropout, 11, 5)
        got = [t.cpu().numpy() for t in backend().ftrl_forward(*csr, step, 3, *glm, dropout, 11, 5, dzn, dy, dom)]
        assert bits_equal(got[0], p) and bits_equal(got[1], om[rows] * (p - y[rows]))
        clamped |= bool((np.abs(raw) > 40).any())
    assert clamped
    raw, p, (k_of, j, xs, _) = ftrl_forward_reference(m.indptr, m.indices, m.data, np.arange(n), zn[:, 0], zn[:, 1], family, ALPHA, BETA, L1, L2)
    terms = ftrl_weights_reference(zn[:, 0], zn[:, 1], ALPHA, BETA, L1, L2)[j] * xs
    assert np.signbit(terms[k_of >= n - 2]).all() and not terms[k_of >= n - 2].any() and not np.signbit(raw[n - 2:]).any()
    assert bits_equal(backend().ftrl_predict(*csr, *glm, dzn).cpu().numpy(), p)


@pytest.mark.parametrize("dropout", [0.0, 0.3])
@pytest.mark.parametrize("family", ["binomial", "gaussian", "poisson"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_step_equals_the_definition(precision, family, dropout):
    dt, rng = DTYPES[precision], np.random.default_rng(2)
    m = canonical_design(step_rows_matrix(), dt)
    n, d = m.shape
    rows = step_rows(n, 1, 2)
    stored = np.bincount(m[rows].indices, minlength=d)
    assert stored[:6].tolist() == [4199, 4097, 64, 65, 1, 0] and m[rows[17]].nnz == 0
    m.data[m.indptr[rows[5]]:m.indptr[rows[5] + 1]] *= 1e6                    # the clip at +-1000 acts on this row's entries
    zn = state(d, dt, rng)
    y, om = targets(n, family, rng)
    om[rows[3]] = 0.0
    raw5 = ftrl_forward_reference(m.indptr, m.indices, m.data, rows[5:6], zn[:, 0], zn[:, 1], family, ALPHA, BETA, L1, L2, dropout, 9, 4)[0]
    y[rows[5]] = float(raw5[0] <= 0) if family == "binomial" else y[rows[5]]   # (a saturated p that agrees with y would leave d = 0)
    glm = (family, ALPHA, BETA, LAM, RATIO)
    csr, dzn, (dy, dom) = device(m, zn, y, om)
    index = backend().fm_index(csr[0], csr[1], d, 2)
    z, nn = zn[:, 0], zn[:, 1]
    for step, epoch in ((1, 4), (0, 4)):                                       # (the second step starts from the first one's result)
        srows = step_rows(n, step, 2)
        _, p, (k_of, _, xs, keep) = ftrl_forward_reference(m.indptr, m.indices, m.data, srows, z, nn, family, ALPHA, BETA, L1, L2, dropout, 9, epoch)
        unclipped = (om[srows] * (p - y[srows]))[k_of] * xs
        z2, n2, p2, kept = ftrl_step_reference(m.indptr, m.indices, m.data, srows, y, om, z, nn, family, ALPHA, BETA, L1, L2, dropout, 9, epoch)
        got = backend().ftrl_step(*csr, index, step, *glm, dropout, 9, epoch, dy, dom, dzn).cpu().numpy()
        res = dzn.cpu().numpy()
        assert bits_equal(res[:, 0], z2) and bits_equal(res[:, 1], n2) and bits_equal(got, p2) and bits_equal(p2, p)
        if step == 1:
            assert (np.abs(unclipped[keep]) > CLIP_GRAD).any() and kept[5] == 0 and bits_equal(z2[5], z[5]) and bits_equal(n2[5], nn[5])
            assert not bits_equal(z2[0], z[0]) and ((kept != stored).any() == (dropout > 0))
        z, nn = z2, n2


@pytest.mark.parametrize("batch", [1024, 334])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_fit_equals_the_definition(precision, batch):
    dt, rng = DTYPES[precision], np.random.default_rng(8)
    x = sp.random(1000, 200, density=0.03, random_state=4, format="csr")
    y, om = targets(1000, "binomial", rng)
    kw = dict(lambda_=0.02, l1_ratio=0.5, dropout=0.25, batch=batch, precision=precision, rng=6)
    fits = [FTRL(**kw), FTRL(**kw)]
    ps = [[f.partial_fit(x, y, om) for _ in range(3)][-1] for f in fits]
    m = canonical_design(x, dt)
    z, n, p = ftrl_fit_reference(m.indptr, m.indices, m.data, y, om, np.zeros(200, dt), np.zeros(200, dt), 3, batch, "binomial", 0.1, 0.5,
                                 0.02, 0.5, 0.25, fits[0].seed, 0)
    for got, gp in zip(fits, ps):
        assert bits_equal(got.z, z) and bits_equal(got.n, n) and bits_equal(gp, p) and (got.seed, got.epoch) == (fits[0].seed, 3)
    assert bits_equal(fits[0].coef(), ftrl_weights_reference(z, n, 0.1, 0.5, 0.01, 0.01)) and np.count_nonzero(z)
    assert bits_equal(fits[0].predict(x), ftrl_forward_reference(m.indptr, m.indices, m.data, np.arange(1000), z, n, "binomial", 0.1, 0.5,
                                                                 0.01, 0.01)[1])


@pytest.mark.parametrize("family", ["binomial", "gaussian", "poisson"])
def test_host_array_forms_equal_the_definition(family):
    rng = np.random.default_rng(12)
    m = canonical_design(sp.random(300, 50, density=0.08, random_state=2, format="csr"), np.float64)
    y, om = targets(300, family, rng)
    zn = state(50, np.float64, rng)
    ref = ftrl_fit_reference(m.indptr, m.indices, m.data, y, om, zn[:, 0], zn[:, 1], 2, 64, family, ALPHA, BETA, LAM, RATIO, 0.2, 77, 3)
    z, n, prob, out = zn[:, 0].copy(), zn[:, 1].copy(), np.zeros(300), np.zeros(300)
    ptr = lambda a: a.ctypes.data
    lib, code = _lib.load(), {"binomial": 0, "gaussian": 1, "poisson": 2}[family]
    _lib.check(lib.rsparse_hip_ftrl_fit(ptr(m.indptr), ptr(m.indices), ptr(m.data), 300, 50, ptr(y), ptr(om), 2, 64, code, ALPHA, BETA, LAM,
                                        RATIO, 0.2, 77, 3, ptr(z), ptr(n), ptr(prob)))
    assert all(bits_equal(g, r) for g, r in zip((z, n, prob), ref))
    _lib.check(lib.rsparse_hip_ftrl_predict(ptr(m.indptr), ptr(m.indices), ptr(m.data), 300, 50, code, ALPHA, BETA, LAM, RATIO, ptr(z), ptr(n),
                                            ptr(out)))
    assert bits_equal(out, ftrl_forward_reference(m.indptr, m.indices, m.data, np.arange(300), z, n, family, ALPHA, BETA, L1, L2)[1])


@pytest.mark.parametrize("bad", [dict(family=3), dict(dropout=1.0), dict(dropout=-0.1), dict(ratio=1.5), dict(alpha=0.0), dict(beta=-1.0),
                                 dict(lam=-0.5), dict(lam=float("inf")), dict(batch=0)])
def test_invalid_arguments_are_refused_at_the_c_boundary(bad):
    rng = np.random.default_rng(0)
    m = canonical_design(rows_of((3, 2, 4), 8, rng), np.float32)
    zn = state(8, np.float32, rng)
    csr, dzn, (dy, dom) = device(m, zn, np.ones(3), np.ones(3))
    index = backend().fm_index(csr[0], csr[1], 8, 1)
    a = dict(family=0, alpha=ALPHA, beta=BETA, lam=LAM, ratio=RATIO, dropout=0.1, batch=3)
    a.update(bad)
    prob = torch.zeros(3, dtype=torch.float64, device=dzn.device)
    rc = _lib.load().rsparse_hip_ftrl_epochs_device(csr[0].data_ptr(), csr[1].data_ptr(), csr[2].data_ptr(), 3, 8, m.nnz, index[0].data_ptr(),
                                                    1, a["batch"], a["family"], a["alpha"], a["beta"], a["lam"], a["ratio"], a["dropout"],
                                                    1, 0, dy.data_ptr(), dom.data_ptr(), dzn.data_ptr(), prob.data_ptr(), None)
    assert rc == _lib.ERR_INVALID and bits_equal(dzn.cpu().numpy(), zn)
