"""C ABI of the confidence weighting (rsparse_hip_confidence_{moments,table,apply}_device, rsparse_hip_confidence): the entries
exist and are additive (the version stays 6), bad calls are answered with ERR_INVALID and a text before a device is touched (those
tests need no device), and -- on a device -- the host-pointer entry returns what the device entries return."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from rsparse_amd import _lib

NAMES = ("rsparse_hip_confidence_moments_device", "rsparse_hip_confidence_table_device", "rsparse_hip_confidence_apply_device",
         "rsparse_hip_confidence")
LINEAR, LOG, TFIDF, BM25, NORMALIZE = range(5)


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


P, J, X = np.array([0, 2, 3], np.int32), np.array([1, 4, 0], np.int32), np.array([1.0, 2.0, 3.0])
T2, T5, OUT = np.ones(2), np.ones(5), np.empty(3)


def _last():
    return _lib.load().rsparse_hip_last_error().decode()


def test_library_exports_the_entry_points():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.rsparse_hip_abi_version() == 6
    import rsparse_amd
    from rsparse_amd.engine import HipBackend
    assert all(callable(getattr(HipBackend, n)) for n in ("confidence_moments", "confidence_table", "confidence_apply"))
    assert callable(rsparse_amd.Confidence) and callable(rsparse_amd.ScaleNormalize)


def test_moments_arguments():
    fn = _lib.load().rsparse_hip_confidence_moments_device

    def call(n_seg=2, nnz=3, p=P, x=X, power=1, out=T2, total=OUT):
        return fn(n_seg, nnz, _vp(p), _vp(x), power, _vp(out), _vp(total), None)
    for bad, text in ((dict(power=0), "power must be 1 or 2"), (dict(power=3), "power must be 1 or 2"), (dict(p=None), "NULL"),
                      (dict(x=None), "NULL"), (dict(out=None), "NULL"), (dict(total=None), "NULL"), (dict(n_seg=-1), "dimensions"),
                      (dict(nnz=-1), "dimensions"), (dict(n_seg=0), "without a segment")):
        assert call(**bad) == _lib.ERR_INVALID, bad
        assert text in _last(), (bad, _last())


def test_table_arguments():
    fn = _lib.load().rsparse_hip_confidence_table_device

    def call(table=0, n=2, p=P, moment=T2, total=OUT, a=1.0, b=1.0, c=1.0, out=T2):
        return fn(table, n, _vp(p), _vp(moment), _vp(total), a, b, c, _vp(out), None)
    for bad, text in ((dict(table=3), "unknown confidence table"), (dict(table=-1), "unknown confidence table"), (dict(n=-1), "negative"),
                      (dict(table=0, p=None), "NULL"), (dict(table=1, moment=None), "NULL"), (dict(table=1, total=None), "NULL"),
                      (dict(table=2, moment=None), "NULL"), (dict(out=None), "NULL"), (dict(table=2, b=3.0), "norm must be 1 or 2"),
                      (dict(table=2, b=0.5), "norm must be 1 or 2")):
        assert call(**bad) == _lib.ERR_INVALID, bad
        assert text in _last(), (bad, _last())
    assert call(n=0, out=None) == _lib.OK


def test_apply_arguments():
    fn = _lib.load().rsparse_hip_confidence_apply_device

    def call(kind=LINEAR, n_seg=2, nnz=3, p=P, i=J, x=X, seg=None, idx=None, n_idx=5, seg_is_item=0, a=1.0, b=1.0, out=OUT, out_float=0):
        return fn(kind, n_seg, nnz, _vp(p), _vp(i), _vp(x), _vp(seg), _vp(idx), n_idx, seg_is_item, a, b, _vp(out), out_float, None)
    for bad, text in ((dict(kind=5), "unknown confidence kind"), (dict(kind=-1), "unknown confidence kind"), (dict(p=None), "NULL"),
                      (dict(x=None), "NULL"), (dict(out=None), "NULL"), (dict(n_seg=-1), "dimensions"), (dict(nnz=-2), "dimensions"),
                      (dict(kind=TFIDF), "table"), (dict(kind=TFIDF, seg=T2), "table"),            # the item table is the index table here
                      (dict(kind=TFIDF, idx=T5, seg_is_item=1), "table"), (dict(kind=BM25, idx=T5), "table"),
                      (dict(kind=BM25, seg=T2), "table"), (dict(kind=NORMALIZE), "table"), (dict(kind=NORMALIZE, seg=T2, idx=T5), "table"),
                      (dict(kind=LINEAR, seg=T2), "table"), (dict(kind=LOG, idx=T5), "table"), (dict(kind=LOG, b=0.0), "eps"),
                      (dict(kind=TFIDF, idx=T5, i=None), "indices"), (dict(out=X, out_float=1), "overlaps")):
        assert call(**bad) == _lib.ERR_INVALID, bad
        assert text in _last(), (bad, _last())
    assert call(nnz=0, p=None, x=None, out=None) == _lib.OK


def test_host_entry_arguments():
    fn = _lib.load().rsparse_hip_confidence

    def call(kind=LINEAR, n_rows=2, n_cols=5, p=P, j=J, x=X, a=1.0, b=1.0, norm=2, by_columns=0, out=OUT):
        return fn(kind, n_rows, n_cols, _vp(p), _vp(j), _vp(x), a, b, norm, by_columns, _vp(out))
    for bad, text in ((dict(kind=7), "unknown confidence kind"), (dict(n_rows=-1), "dimensions"), (dict(p=None), "NULL"), (dict(j=None), "NULL"),
                      (dict(x=None), "NULL"), (dict(out=None), "NULL"), (dict(kind=NORMALIZE, norm=3), "norm must be 1 or 2"),
                      (dict(kind=LOG, b=0.0), "eps"), (dict(p=np.array([1, 2, 3], np.int32)), "p[0]"),
                      (dict(p=np.array([0, 3, 2], np.int32)), "decreases"), (dict(n_cols=4), "column index")):
        assert call(**bad) == _lib.ERR_INVALID, bad
        assert text in _last(), (bad, _last())
    assert call(n_rows=0, p=np.zeros(1, np.int32), j=None, x=None, out=None) == _lib.OK


@pytest.mark.gpu
def test_host_entry_equals_the_device_entries():
    """`rsparse_hip_confidence` on a host CSR == fit + transform by rsparse_amd.Confidence / ScaleNormalize on the device arrays
    (the same kernels on the same values: every bit)."""
    from rsparse_amd import Confidence, ScaleNormalize
    rng = np.random.default_rng(4)
    d = (rng.random((90, 700)) < 0.3) * (0.25 + rng.random((90, 700)) * 4)
    d[11, :] = 0.0
    d[:, 0] = 1.5          # a hot column
    m = sp.csr_matrix(d)
    m.sort_indices()
    fn = _lib.load().rsparse_hip_confidence
    p, j = m.indptr.astype(np.int32), m.indices.astype(np.int32)
    cases = [(LINEAR, Confidence("linear", alpha=3.0), (3.0, 0.0, 0, 0)), (LOG, Confidence("log", alpha=3.0, eps=0.5), (3.0, 0.5, 0, 0)),
             (TFIDF, Confidence("tfidf"), (0.0, 0.0, 0, 0)), (BM25, Confidence("bm25", K1=12.0, B=0.6), (12.0, 0.6, 0, 0))]
    for norm in (1, 2):
        cases.append((NORMALIZE, ScaleNormalize(scale=0.25, norm=norm, target="rows"), (0.25, 0.0, norm, 0)))
        cases.append((NORMALIZE, ScaleNormalize(scale=0.25, norm=norm, target="columns"), (0.25, 0.0, norm, 1)))
    for kind, model, (a, b, norm, by_columns) in cases:
        out = np.empty(m.nnz)
        _lib.check(fn(kind, m.shape[0], m.shape[1], _vp(p), _vp(j), _vp(m.data), a, b, norm, by_columns, _vp(out)))
        ref = model.fit_transform(m)
        assert np.array_equal(out, ref.data), (kind, norm, by_columns, np.abs(out - ref.data).max())
