"""C ABI of the negative sampler (rsparse_hip_sample_negatives_device / rsparse_hip_sample_negatives): the entry points exist and
are additive (the version stays 6), bad calls are answered with status codes before anything is launched, row pointers that
decrease and a capacity that is too small are refused before the sampling launch, and the host-pointer form returns what the
device form returns and checks the contents of the lists."""
import ctypes

import numpy as np
import pytest
import torch

from rsparse_amd import _lib
from rsparse_amd import rng as R

pytestmark = pytest.mark.gpu

NAMES = ("rsparse_hip_sample_negatives_device", "rsparse_hip_sample_negatives")


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


SP, SJ = np.array([0, 2, 3], np.int32), np.array([1, 4, 0], np.int32)
KP, KJ = np.array([0, 1, 1], np.int32), np.array([4], np.int32)


def test_library_exports_the_entry_points():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.rsparse_hip_abi_version() == 6
    assert _lib.MAX_NEGATIVES == R.MAX_NEGATIVES == 8192
    from rsparse_amd import WRMF
    from rsparse_amd.engine import HipBackend
    assert callable(HipBackend.sample_negatives) and callable(WRMF.sample_negatives) and callable(R.sample_negatives)


@pytest.mark.parametrize("name", NAMES)
def test_status_codes_without_a_launch(name):
    # (host pointers: every call here is rejected by the argument checks, or is the n_rows = 0 no-op, before device work)
    fn = getattr(_lib.load(), name)
    out_p, out_j = np.empty(3, np.int32), np.empty(16, np.int32)
    tail = (None,) if name.endswith("_device") else ()

    def call(seed=1, row0=0, n_rows=2, n_item=6, n=2, sp_=SP, sj=SJ, kp=KP, kj=KJ, op=out_p, oj=out_j, cap=16):
        return fn(seed, row0, n_rows, n_item, n, _vp(sp_), _vp(sj), _vp(kp), _vp(kj), _vp(op), _vp(oj), cap, *tail)

    bad = [dict(sp_=None), dict(sj=None), dict(op=None), dict(kp=None), dict(kj=None), dict(n_rows=-1), dict(n_item=-1), dict(n=0),
           dict(n=-5), dict(row0=-1), dict(cap=-1), dict(row0=2 ** 32 - 1)]
    if name.endswith("_device"):
        bad.append(dict(oj=None))
    for b in bad:
        assert call(**b) == _lib.ERR_INVALID, b
        assert _lib.load().rsparse_hip_last_error()
    assert call(n=8193) == _lib.ERR_UNSUPPORTED
    assert call(n_rows=0) == _lib.OK                                       # no row: a no-op
    assert call(n_rows=0, kp=None, kj=None) == _lib.OK


def _device_call(sp_, sj, kp, kj, n_item, n, cap, seed=3, row0=0):
    lib = _lib.load()
    d = lambda a: None if a is None else torch.from_numpy(a).to("cuda:0")
    n_rows = sp_.size - 1
    t = [d(sp_), d(sj), d(kp), d(kj)]
    out_p = torch.zeros(n_rows + 1, dtype=torch.int32, device="cuda:0")
    out_j = torch.full((max(cap, 1),), -1, dtype=torch.int32, device="cuda:0")
    rc = lib.rsparse_hip_sample_negatives_device(seed, row0, n_rows, n_item, n, t[0].data_ptr(), t[1].data_ptr(),
                                                 None if kp is None else t[2].data_ptr(), None if kj is None else t[3].data_ptr(),
                                                 out_p.data_ptr(), out_j.data_ptr(), cap, None)
    torch.cuda.synchronize()
    return rc, out_p.cpu().numpy(), out_j.cpu().numpy()


def test_row_pointers_that_decrease_and_a_small_capacity_are_refused():
    for sp_ in (np.array([3, 2, 3], np.int32), np.array([-1, 0, 2], np.int32), np.array([0, 3, 2], np.int32)):
        rc, _, oj = _device_call(sp_, SJ, None, None, 6, 2, 16)
        assert rc == _lib.ERR_INVALID and np.all(oj == -1)
    rc, _, oj = _device_call(SP, SJ, np.array([0, 1, 0], np.int32), KJ, 6, 2, 16)          # keep_p decreases
    assert rc == _lib.ERR_INVALID and np.all(oj == -1)
    rc, _, oj = _device_call(SP, SJ, np.array([0, 3, 3], np.int32), np.array([0, 1, 4], np.int32), 6, 2, 16)   # a keep row longer than seen
    assert rc == _lib.ERR_INVALID and np.all(oj == -1)
    rc, _, oj = _device_call(np.array([0, 3, 3], np.int32), SJ, None, None, 2, 2, 16)      # a seen row longer than n_item
    assert rc == _lib.ERR_INVALID and np.all(oj == -1)
    rc, _, oj = _device_call(SP, SJ, KP, KJ, 6, 2, 4)                                     # the rows need 2 + 1 + 2 = 5
    assert rc == _lib.ERR_INVALID and np.all(oj == -1) and b"5" in _lib.load().rsparse_hip_last_error()
    rc, op, oj = _device_call(SP, SJ, KP, KJ, 6, 2, 5)
    assert rc == _lib.OK and np.array_equal(op, [0, 3, 5]) and np.all(oj >= 0)


def _case():
    rng = np.random.default_rng(4)
    n_item = 500
    lens = np.r_[0, 500, 499, 1, rng.integers(0, 480, size=40)]
    seen = [np.sort(rng.choice(n_item, size=l, replace=False)) for l in lens]
    keep = [s[::5] for s in seen]
    csr = lambda rows: (np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32), np.concatenate(rows).astype(np.int32))
    return (n_item,) + csr(seen) + csr(keep)


@pytest.mark.parametrize("n", [7, 300])
def test_host_form_equals_device_form(n):
    fn = _lib.load().rsparse_hip_sample_negatives
    n_item, sp_, sj, kp, kj = _case()
    n_rows = sp_.size - 1
    out_p = np.full(n_rows + 1, -1, np.int32)
    # the first call: the sizes only
    _lib.check(fn(3, 11, n_rows, n_item, n, _vp(sp_), _vp(sj), _vp(kp), _vp(kj), _vp(out_p), None, 0))
    total = int(out_p[-1])
    assert out_p[0] == 0 and np.array_equal(np.diff(out_p), np.diff(kp) + np.minimum(n, n_item - np.diff(sp_)))
    out_j = np.full(total + 3, -1, np.int32)
    assert fn(3, 11, n_rows, n_item, n, _vp(sp_), _vp(sj), _vp(kp), _vp(kj), _vp(out_p), _vp(out_j), total - 1) == _lib.ERR_INVALID
    _lib.check(fn(3, 11, n_rows, n_item, n, _vp(sp_), _vp(sj), _vp(kp), _vp(kj), _vp(out_p), _vp(out_j), total))
    rc, d_p, d_j = _device_call(sp_, sj, kp, kj, n_item, n, total, seed=3, row0=11)
    assert rc == _lib.OK and np.array_equal(out_p, d_p) and np.array_equal(out_j[:total], d_j[:total]) and np.all(out_j[total:] == -1)
    want_p, want_j = R.sample_negatives(3, 11, sp_, sj, kp, kj, n_item, n)
    assert np.array_equal(out_p, want_p) and np.array_equal(out_j[:total], want_j)
    # without keep rows
    _lib.check(fn(3, 11, n_rows, n_item, n, _vp(sp_), _vp(sj), None, None, _vp(out_p), _vp(out_j), total))
    want_p, want_j = R.sample_negatives(3, 11, sp_, sj, None, None, n_item, n)
    assert np.array_equal(out_p, want_p) and np.array_equal(out_j[:want_p[-1]], want_j)


def test_host_form_checks_the_lists():
    fn = _lib.load().rsparse_hip_sample_negatives
    out_p, out_j = np.empty(3, np.int32), np.empty(16, np.int32)

    def call(sp_=SP, sj=SJ, kp=KP, kj=KJ, n_item=6):
        return fn(1, 0, 2, n_item, 2, _vp(sp_), _vp(sj), _vp(kp), _vp(kj), _vp(out_p), _vp(out_j), 16)

    assert call() == _lib.OK
    for bad in (dict(kj=np.array([2], np.int32)),                                        # keep is no subset of seen
                dict(kp=np.array([0, 2, 2], np.int32), kj=np.array([4, 1], np.int32)),   # keep not ascending
                dict(kp=np.array([0, 2, 2], np.int32), kj=np.array([1, 1], np.int32)),   # keep not unique
                dict(sj=np.array([4, 1, 0], np.int32)),                                  # seen not sorted
                dict(sj=np.array([1, 1, 0], np.int32)),                                  # seen not unique
                dict(sj=np.array([1, 6, 0], np.int32)), dict(sj=np.array([-1, 4, 0], np.int32)),   # out of range
                dict(sp_=np.array([1, 2, 3], np.int32)), dict(sp_=np.array([0, 3, 2], np.int32)),
                dict(kp=np.array([1, 1, 1], np.int32))):
        assert call(**bad) == _lib.ERR_INVALID, bad
