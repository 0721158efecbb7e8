"""C ABI of the train / test split (rsparse_hip_split_rows_device / rsparse_hip_split_rows): the entry points exist and are additive
(the version stays 6), bad calls are answered with status codes before a device is touched (so these tests need none), the
host-pointer form checks the columns and `by`, and -- on a device -- returns what the device form returns."""
import ctypes

import numpy as np
import pytest

from rsparse_amd import _lib
from rsparse_amd import rng as R

NAMES = ("rsparse_hip_split_rows_device", "rsparse_hip_split_rows")
PROPORTION, LEAVE_OUT = 0, 1


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


P, J = np.array([0, 2, 3], np.int32), np.array([1, 4, 0], np.int32)
V, BY = np.array([1.0, 2.0, 3.0], np.float32), np.array([5.0, 5.0, 1.0])


def test_library_exports_the_entry_points():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.rsparse_hip_abi_version() == 6
    assert (R.STREAM_USERS, R.STREAM_ITEMS, R.STREAM_NEGATIVES, R.STREAM_SPLIT, R.STREAM_LEAVE_OUT) == (0, 1, 2, 3, 4)
    import rsparse_amd
    from rsparse_amd import WRMF
    from rsparse_amd.engine import HipBackend
    assert callable(HipBackend.split_rows) and callable(WRMF.train_test_split) and callable(rsparse_amd.train_test_split)


def _caller(name):
    fn = getattr(_lib.load(), name)
    tail = (None,) if name.endswith("_device") else ()
    outs = [np.empty(3, np.int32), np.empty(8, np.int32), np.empty(8, np.float32), np.empty(3, np.int32), np.empty(8, np.int32),
            np.empty(8, np.float32)]

    def call(seed=1, row0=0, n_rows=2, mode=PROPORTION, T=2 ** 31, n=1, min_train=1, p=P, j=J, v=V, vb=4, by=None, trp=outs[0],
             trj=outs[1], trv=outs[2], tep=outs[3], tej=outs[4], tev=outs[5], cap_tr=8, cap_te=8):
        return fn(seed, row0, n_rows, mode, T, n, min_train, _vp(p), _vp(j), _vp(v), vb, _vp(by), _vp(trp), _vp(trj), _vp(trv), _vp(tep),
                  _vp(tej), _vp(tev), cap_tr, cap_te, *tail)
    return call


@pytest.mark.parametrize("name", NAMES)
def test_status_codes_without_a_launch(name):
    # (host pointers: every call here is rejected by the argument checks, or is the n_rows = 0 no-op, before device work)
    call = _caller(name)
    bad = [dict(p=None), dict(j=None), dict(trp=None), dict(tep=None), dict(n_rows=-1), dict(row0=-1), dict(row0=2 ** 32 - 1),
           dict(T=2 ** 32 + 1), dict(mode=2), dict(mode=-1), dict(by=BY),                       # `by` in proportion mode
           dict(mode=LEAVE_OUT, n=0), dict(mode=LEAVE_OUT, n=-4), dict(mode=LEAVE_OUT, min_train=-1),
           dict(vb=2), dict(vb=16), dict(vb=0), dict(v=None), dict(v=None, vb=8),            # values and value_bytes go together
           dict(trv=None), dict(tev=None), dict(trj=None), dict(tej=None), dict(cap_tr=-1), dict(cap_te=-1)]
    for b in bad:
        assert call(**b) == _lib.ERR_INVALID, b
        assert _lib.load().rsparse_hip_last_error()
    assert call(n_rows=0) == _lib.OK                                       # no row: a no-op
    assert call(n_rows=0, mode=LEAVE_OUT, by=BY, v=None, vb=0, trv=None, tev=None) == _lib.OK
    assert call(n_rows=0, T=2 ** 32) == _lib.OK and call(n_rows=0, T=0) == _lib.OK
    assert call(n_rows=0, row0=2 ** 32) == _lib.OK and call(n_rows=1, row0=2 ** 32) == _lib.ERR_INVALID


def test_host_form_checks_the_columns_and_by():
    # (every call is refused by a check of the host arrays, before device work)
    call = _caller("rsparse_hip_split_rows")
    for bad in (dict(j=np.array([4, 1, 0], np.int32)),                     # not ascending
                dict(j=np.array([1, 1, 0], np.int32)),                     # not unique
                dict(j=np.array([-1, 4, 0], np.int32)),
                dict(p=np.array([1, 2, 3], np.int32)), dict(p=np.array([0, 3, 2], np.int32)),
                dict(mode=LEAVE_OUT, by=np.array([5.0, np.nan, 1.0])), dict(mode=LEAVE_OUT, by=np.array([5.0, 1.0, -np.nan]))):
        assert call(**bad) == _lib.ERR_INVALID, bad
        assert _lib.load().rsparse_hip_last_error()


def _case():
    rng = np.random.default_rng(4)
    lens = np.r_[0, 1, 300, 5000, rng.integers(0, 80, size=40)]
    rows = [np.sort(rng.choice(6000, size=l, replace=False)) for l in lens]
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    j = np.concatenate(rows).astype(np.int32)
    return p, j, rng.random(j.size), np.floor(rng.random(j.size) * 4.0) - 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(test_threshold=int(0.3 * 2 ** 32)), dict(leave_out=3, min_train=1), dict(leave_out=70, min_train=0, by=True)],
                         ids=["proportion", "leave_out", "by"])
def test_host_form_equals_device_form(kw):
    import torch
    from rsparse_amd.engine import HipBackend
    fn = _lib.load().rsparse_hip_split_rows
    p, j, v, by = _case()
    kw = dict(kw)
    by = by if kw.pop("by", False) else None
    n_rows, nnz = p.size - 1, int(p[-1])
    mode, T, n, mt = (PROPORTION, kw["test_threshold"], 0, 1) if "test_threshold" in kw else (LEAVE_OUT, 0, kw["leave_out"], kw["min_train"])
    tr_p, te_p = np.full(n_rows + 1, -1, np.int32), np.full(n_rows + 1, -1, np.int32)
    head = (3, 11, n_rows, mode, T, n, mt, _vp(p), _vp(j))
    # the first call: the sizes only
    _lib.check(fn(*head, _vp(v), 8, _vp(by), _vp(tr_p), None, None, _vp(te_p), None, None, 0, 0))
    n_tr, n_te = int(tr_p[-1]), int(te_p[-1])
    assert tr_p[0] == 0 and te_p[0] == 0 and n_tr + n_te == nnz and np.array_equal(np.diff(tr_p) + np.diff(te_p), np.diff(p))
    tr_j, te_j = np.full(n_tr + 3, -1, np.int32), np.full(n_te + 3, -1, np.int32)
    tr_v, te_v = np.full(n_tr + 3, -1.0), np.full(n_te + 3, -1.0)
    args = lambda c0, c1: head + (_vp(v), 8, _vp(by), _vp(tr_p), _vp(tr_j), _vp(tr_v), _vp(te_p), _vp(te_j), _vp(te_v), c0, c1)
    if n_te:
        assert fn(*args(n_tr, n_te - 1)) == _lib.ERR_INVALID and np.all(te_j == -1) and np.all(tr_j == -1)
    _lib.check(fn(*args(n_tr, n_te)))
    d = lambda a: None if a is None else torch.from_numpy(a).to("cuda:0")
    got = HipBackend().split_rows(3, 11, d(p), d(j), d(v), by=d(by), **kw)
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in got]
    want = R.split_rows(3, 11, p, j, by=by, **kw)
    for host, dev, w_p, w_j, w_pos, n_out in (((tr_p, tr_j, tr_v), got[0:3], want[0], want[1], want[2], n_tr),
                                             ((te_p, te_j, te_v), got[3:6], want[3], want[4], want[5], n_te)):
        assert np.array_equal(host[0], dev[0]) and np.array_equal(host[0], w_p)
        assert np.array_equal(host[1][:n_out], dev[1]) and np.array_equal(dev[1], w_j) and np.all(host[1][n_out:] == -1)
        assert np.array_equal(host[2][:n_out], dev[2]) and np.array_equal(dev[2], v[w_pos]) and np.all(host[2][n_out:] == -1.0)
