"""The factorization machine on the device (wrmf_fm.hip behind rsparse_hip_fm_*_device) against the numpy definition of
rsparse_amd/fm.py, bit for bit in both precisions: the forward pass at every row-length edge, one step at every segment-length edge,
whole fits through the public class."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import FactorizationMachine, _lib
from rsparse_amd import rng as prng
from rsparse_amd.fm import canonical_design, fm_delta, fm_fit_reference, fm_forward_reference, fm_link, fm_step_reference, step_rows
from test_bpr import DTYPES, TORCH, backend, bits_equal

pytestmark = pytest.mark.gpu

LONG = _lib.FM_LONG_ROW
LENGTHS = (0, 1, 2, 63, 64, 65, 129, LONG, LONG + 1)


def rows_of(lengths, d, rng, scale=None):
    """a CSR whose row i holds lengths[i] distinct columns with normal values (row scale[i] times larger)"""
    idx = [np.sort(rng.choice(d, size=n, replace=False)) for n in lengths]
    val = [rng.normal(size=n) * (1.0 if scale is None else scale[i]) for i, n in enumerate(lengths)]
    return sp.csr_matrix((np.concatenate(val), np.concatenate(idx), np.concatenate([[0], np.cumsum(lengths)])), shape=(len(lengths), d))


def params(d, rank, dt, rng, states=False):
    w0, w, V = rng.normal(size=1).astype(dt), rng.normal(size=d).astype(dt), (0.3 * rng.normal(size=(d, rank))).astype(dt)
    return (w0, w, V) + ((rng.random(1), rng.random(d), rng.random((d, rank))) if states else ())


def device(m, arrays):
    be = backend()
    csr = (be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32), be.to_device(m.data, TORCH[m.dtype.type]))
    return csr, [be.to_device(a, TORCH[a.dtype.type]) for a in arrays]


def targets(n, family, rng):
    y = np.where(rng.random(n) < 0.5, -1.0, 1.0) if family == "binomial" else rng.normal(size=n)
    return y, rng.random(n) + 0.5


@functools.lru_cache(maxsize=None)
def forward_rows():
    rng = np.random.default_rng(3)
    scale = [1.0] * len(LENGTHS)
    scale[LENGTHS.index(129)] = 40.0                                         # |y raw| passes 40 there: the clamp of E
    return rows_of(LENGTHS * 2, LONG + 8, rng, scale * 2)


@pytest.mark.parametrize("rank", [1, 16, 17, 128])
@pytest.mark.parametrize("family", ["binomial", "gaussian"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_forward_equals_the_definition(precision, family, rank):
    dt, rng = DTYPES[precision], np.random.default_rng(rank)
    m = canonical_design(forward_rows(), dt)
    n, d = m.shape
    w0, w, V = params(d, rank, dt, rng)
    y, om = targets(n, family, rng)
    csr, (dw0, dw, dV, dy, dom) = device(m, (w0, w, V, y, om))
    clamped = False
    for step in range(3):
        rows = step_rows(n, step, 3)
        raw, s = fm_forward_reference(m.indptr, m.indices, m.data, rows, w0, w, V)
        got = [t.cpu().numpy() for t in backend().fm_forward(*csr, family, step, 3, dw0, dw, dV, dy, dom)]
        assert bits_equal(got[0], raw) and bits_equal(got[1], fm_delta(raw, y[rows], om[rows], family))
        assert bits_equal(got[2][:, :rank], s) and not got[2][:, rank:].any()
        clamped |= bool((np.abs(y[rows] * raw) > 40).any())
    assert clamped
    raw = fm_forward_reference(m.indptr, m.indices, m.data, np.arange(n), w0, w, V)[0]
    assert bits_equal(backend().fm_predict(*csr, family, dw0, dw, dV).cpu().numpy(), fm_link(raw, family))


@functools.lru_cache(maxsize=None)
def step_rows_matrix():
    """8400 x 40: the odd rows are step 1 of 2.  There column 0 is in every row but the empty one, column 1 in 64 * 64 + 1 rows,
    columns 2, 3, 4 in 64, 65 and 1 rows, column 5 in none; the even rows hold column 5 and more"""
    rng = np.random.default_rng(5)
    nb, d = 4200, 40
    dense = (rng.random((2 * nb, d)) < 0.05) * rng.normal(size=(2 * nb, d))
    dense[:, :6] = 0.0
    b = dense[1::2]
    b[17] = 0.0
    full = np.delete(np.arange(nb), 17)
    for col, cnt in ((0, nb - 1), (1, 64 * 64 + 1), (2, 64), (3, 65), (4, 1)):
        b[rng.choice(full, size=cnt, replace=False), col] = rng.normal(size=cnt)
    dense[1::2] = b
    dense[0::2, 5] = 1.0
    return sp.csr_matrix(dense)


@pytest.mark.parametrize("rank", [1, 17, 128])
@pytest.mark.parametrize("family", ["binomial", "gaussian"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_step_equals_the_definition(precision, family, rank):
    dt, rng = DTYPES[precision], np.random.default_rng(rank + 1)
    m = canonical_design(step_rows_matrix(), dt)
    n, d = m.shape
    rows = step_rows(n, 1, 2)
    counts = np.bincount(m[rows].indices, minlength=d)
    assert counts[:6].tolist() == [4199, 4097, 64, 65, 1, 0] and m[rows[17]].nnz == 0
    start = params(d, rank, dt, rng, states=True)
    y, om = targets(n, family, rng)
    om[rows[3]] = 0.0
    index = None
    for intercept, lam in ((True, (0.0, 0.0)), (False, (0.03, 0.07))):
        ref = fm_step_reference(m.indptr, m.indices, m.data, rows, y, om, *start, family, intercept, 0.2, 0.1, *lam)
        csr, dev = device(m, start + (y, om))
        index = index or backend().fm_index(csr[0], csr[1], d, 2)
        term = backend().fm_step(*csr, index, 1, family, intercept, dev[6], dev[7], *dev[:6], 0.2, 0.1, *lam)
        assert all(bits_equal(g.cpu().numpy(), r) for g, r in zip(dev[:6], ref[:6]))
        assert term.cpu().numpy()[0] == ref[6]
        assert bits_equal(ref[2][5], start[2][5]) and bits_equal(ref[5][5], start[5][5]) and not bits_equal(ref[2][4], start[2][4])
        assert bits_equal(ref[0], start[0]) == (not intercept)


@pytest.mark.parametrize("batch", [1024, 334])
@pytest.mark.parametrize("family", ["binomial", "gaussian"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_fit_equals_the_definition(precision, family, batch):
    dt, rng = DTYPES[precision], np.random.default_rng(8)
    x = sp.random(1000, 200, density=0.03, random_state=4, format="csr")
    y, om = targets(1000, family, rng)
    kw = dict(rank=17, family=family, batch=batch, lambda_w=0.01, lambda_v=0.02, precision=precision, rng=6)
    a = FactorizationMachine(**kw).fit(x, y, om, n_iter=3)
    b = FactorizationMachine(**kw).fit(x, y, om, n_iter=3)
    m = canonical_design(x, dt)
    V0 = backend().init_factors(a.seed, prng.STREAM_ITEMS, 200, 17, TORCH[dt]).cpu().numpy()              # (the device's draw, as the model took it)
    ref = fm_fit_reference(m.indptr, m.indices, m.data, y, om, np.zeros(1, dt), np.zeros(200, dt), V0, np.zeros(1), np.zeros(200),
                           np.zeros((200, 17)), 3, batch, family, True, 0.2, 0.2, 0.01, 0.02)
    for got in (a, b):
        fitted = (got.w0, got.w, got.v.T, got.adagrad_w0, got.adagrad_w, got.adagrad_v.T)
        assert all(bits_equal(np.asarray(g).reshape(np.shape(r)), r) for g, r in zip(fitted, ref[:6]))
        assert got.trace == ref[6] and got.seed == a.seed
    raw = fm_forward_reference(m.indptr, m.indices, m.data, np.arange(1000), *ref[:3])[0]
    assert bits_equal(a.predict(x), fm_link(raw, family))


@pytest.mark.parametrize("family", ["binomial", "gaussian"])
def test_host_array_forms_equal_the_definition(family):
    rng = np.random.default_rng(12)
    m = canonical_design(sp.random(300, 50, density=0.08, random_state=2, format="csr"), np.float64)
    y, om = targets(300, family, rng)
    start = params(50, 5, np.float64, rng, states=True)
    ref = fm_fit_reference(m.indptr, m.indices, m.data, y, om, *start, 2, 128, family, True, 0.2, 0.1, 0.01, 0.02)
    got = [np.array(a) for a in start]
    trace = np.zeros(2, dtype=np.int64 if family == "binomial" else np.float64)
    ptr = lambda a: a.ctypes.data
    lib, code = _lib.load(), {"binomial": 0, "gaussian": 1}[family]
    _lib.check(lib.rsparse_hip_fm_fit(ptr(m.indptr), ptr(m.indices), ptr(m.data), 300, 50, ptr(y), ptr(om), 2, 128, 5, code, 1, 0.2, 0.1, 0.01,
                                      0.02, *(ptr(a) for a in got), ptr(trace)))
    assert all(bits_equal(g, r) for g, r in zip(got, ref[:6])) and trace.tolist() == ref[6]
    out = np.zeros(300)
    _lib.check(lib.rsparse_hip_fm_predict(ptr(m.indptr), ptr(m.indices), ptr(m.data), 300, 50, 5, code, *(ptr(a) for a in got[:3]), ptr(out)))
    assert bits_equal(out, fm_link(fm_forward_reference(m.indptr, m.indices, m.data, np.arange(300), *ref[:3])[0], family))


def test_rank_129_is_unsupported():
    with pytest.raises(_lib.UnsupportedOnDevice):
        FactorizationMachine(rank=129)
    rng = np.random.default_rng(0)
    m = canonical_design(rows_of((3, 2), 8, rng), np.float32)
    csr, (dw0, dw, dV) = device(m, params(8, 129, np.float32, rng))
    with pytest.raises(_lib.UnsupportedOnDevice):
        backend().fm_predict(*csr, "binomial", dw0, dw, dV)
