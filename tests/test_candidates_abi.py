"""C ABI of the top-k within candidate lists (rsparse_hip_top_candidates_device / _f64_device / rsparse_hip_top_candidates): the
entry points exist and are additive (the version stays 6), bad calls are answered with status codes before anything is
launched, and the host-pointer form returns what the device form returns."""
import ctypes

import numpy as np
import pytest
import torch

from rsparse_amd import _lib

pytestmark = pytest.mark.gpu

NAMES = ("rsparse_hip_top_candidates_device", "rsparse_hip_top_candidates_f64_device", "rsparse_hip_top_candidates")
NA = -2147483648


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_library_exports_the_entry_points():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.rsparse_hip_abi_version() == 6
    from rsparse_amd import WRMF
    from rsparse_amd.engine import HipBackend
    assert callable(HipBackend.top_candidates) and callable(WRMF._top_candidates_host)


@pytest.mark.parametrize("name,dt,max_rank", [(NAMES[0], np.float32, 256), (NAMES[1], np.float64, 128)])
def test_device_forms_status_codes_without_a_launch(name, dt, max_rank):
    # (host pointers: every call here is rejected by the argument checks, or is the n_users = 0 no-op, before device work)
    fn = getattr(_lib.load(), name)
    U, V = np.ones((2, 4), dtype=dt), np.ones((3, 4), dtype=dt)
    p, j = np.array([0, 2, 3], np.int32), np.array([0, 2, 1], np.int32)
    nrp, nrj, ex = np.array([0, 1, 1], np.int32), np.array([2], np.int32), np.array([1], np.int32)
    res, sc = np.empty((2, 2), np.int32), np.empty((2, 2))

    def call(U=U, V=V, n=2, m=3, r=4, k=2, p=p, j=j, nrp=nrp, nrj=nrj, ex=ex, nex=1, res=res, sc=sc):
        return fn(_vp(U), _vp(V), n, m, r, k, _vp(p), _vp(j), _vp(nrp), _vp(nrj), _vp(ex), nex, 0.5, _vp(res), _vp(sc), None)

    for bad in (dict(U=None), dict(V=None), dict(p=None), dict(j=None), dict(res=None), dict(sc=None), dict(nrj=None), dict(ex=None),
                dict(n=-1), dict(m=-1), dict(r=0), dict(k=0), dict(k=-3), dict(nex=-1)):
        assert call(**bad) == _lib.ERR_INVALID, bad
        assert _lib.load().rsparse_hip_last_error()
    assert call(r=max_rank + 1) == _lib.ERR_UNSUPPORTED
    assert call(k=8193) == _lib.ERR_UNSUPPORTED
    assert call(n=0) == _lib.OK                                            # no user: a no-op
    assert call(n=0, nrp=None, nrj=None, ex=None, nex=0) == _lib.OK


def test_row_pointers_that_decrease_are_refused():
    lib = _lib.load()
    d = lambda a: torch.from_numpy(a).to("cuda:0")
    U, V = d(np.ones((2, 4), np.float32)), d(np.ones((3, 4), np.float32))
    j = d(np.array([0, 2, 1], np.int32))
    res, sc = torch.empty((2, 2), dtype=torch.int32, device="cuda:0"), torch.empty((2, 2), dtype=torch.float64, device="cuda:0")
    for p in (np.array([3, 2, 1], np.int32), np.array([-1, 0, 2], np.int32)):
        dp = d(p)
        assert lib.rsparse_hip_top_candidates_device(U.data_ptr(), V.data_ptr(), 2, 3, 4, 2, dp.data_ptr(), j.data_ptr(), None, None,
                                                     None, 0, 0.0, res.data_ptr(), sc.data_ptr(), None) == _lib.ERR_INVALID


def test_host_form_status_codes():
    fn = _lib.load().rsparse_hip_top_candidates
    x, y = np.ones((2, 4), order="F"), np.ones((4, 3), order="F")
    p, j = np.array([0, 2, 3], np.int32), np.array([0, 2, 1], np.int32)
    res, sc = np.empty((2, 2), np.int32, order="F"), np.empty((2, 2), order="F")

    def call(x=x, y=y, n=2, m=3, r=4, k=2, p=p, j=j, ex=None, nex=0, res=res, sc=sc):
        return fn(_vp(x), _vp(y), n, m, r, k, 1, _vp(p), _vp(j), None, None, _vp(ex), nex, 0.0, _vp(res), _vp(sc))

    for bad in (dict(x=None), dict(y=None), dict(p=None), dict(j=None), dict(res=None), dict(sc=None), dict(n=-1), dict(m=-1), dict(r=0),
                dict(k=0), dict(nex=1), dict(nex=-1), dict(p=np.array([1, 2, 3], np.int32)), dict(p=np.array([0, 3, 2], np.int32)),
                dict(j=np.array([2, 0, 1], np.int32)), dict(j=np.array([0, 0, 1], np.int32)), dict(j=np.array([0, 3, 1], np.int32)),
                dict(j=np.array([-1, 2, 1], np.int32))):
        assert call(**bad) == _lib.ERR_INVALID, bad
    assert call(r=129) == _lib.ERR_UNSUPPORTED
    assert call(k=8193) == _lib.ERR_UNSUPPORTED
    assert call() == _lib.OK


@pytest.mark.parametrize("k", [3, 40])
def test_host_form_equals_device_form(k):
    lib = _lib.load()
    rng = np.random.default_rng(2)
    n, m, r = 23, 200, 6
    x = np.asfortranarray(rng.integers(-2, 3, size=(n, r)).astype(np.float64))       # ties are real
    y = np.asfortranarray(rng.integers(-2, 3, size=(r, m)).astype(np.float64))
    lens = rng.integers(0, 90, size=n)
    lens[0], lens[1] = 0, 70
    rows = [np.sort(rng.choice(m, size=l, replace=False)) for l in lens]
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    j = np.concatenate(rows).astype(np.int32)
    nr_rows = [rng.permutation(c[::3]) for c in rows]                                 # unsorted: the host form sorts them
    nrp = np.concatenate([[0], np.cumsum([c.size for c in nr_rows])]).astype(np.int32)
    nrj = np.concatenate(nr_rows).astype(np.int32)
    ex1 = np.array([m, 1, 17, 17, 0, m + 5], np.int32)                                 # 1-based; out of range ones are dropped
    res, sc = np.empty((n, k), np.int32, order="F"), np.empty((n, k), order="F")
    _lib.check(lib.rsparse_hip_top_candidates(_vp(x), _vp(y), n, m, r, k, 1, _vp(p), _vp(j), _vp(nrp), _vp(nrj), _vp(ex1), ex1.size,
                                              0.25, _vp(res), _vp(sc)))
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    nrj_sorted = np.concatenate([np.sort(c) for c in nr_rows]).astype(np.int32)
    dU, dV = d(np.ascontiguousarray(x)), d(np.ascontiguousarray(y.T))
    dres, dsc = torch.empty((n, k), dtype=torch.int32, device="cuda:0"), torch.empty((n, k), dtype=torch.float64, device="cuda:0")
    dp, dj, dnp, dnj, dex = d(p), d(j), d(nrp), d(nrj_sorted), d(np.array([0, 16, m - 1], np.int32))
    _lib.check(lib.rsparse_hip_top_candidates_f64_device(dU.data_ptr(), dV.data_ptr(), n, m, r, k, dp.data_ptr(), dj.data_ptr(),
                                                         dnp.data_ptr(), dnj.data_ptr(), dex.data_ptr(), 3, 0.25, dres.data_ptr(),
                                                         dsc.data_ptr(), None))
    torch.cuda.synchronize()
    assert np.array_equal(res, dres.cpu().numpy())
    assert np.array_equal(sc.view(np.int64), dsc.cpu().numpy().view(np.int64))
    assert (res[0] == NA).all() and np.isnan(sc[0]).all() and (res != NA).any()
    # and the fp32 device form on the same (integer-valued) factors
    dres32, dsc32 = torch.empty_like(dres), torch.empty_like(dsc)
    dU32, dV32 = dU.float(), dV.float()
    _lib.check(lib.rsparse_hip_top_candidates_device(dU32.data_ptr(), dV32.data_ptr(), n, m, r, k, dp.data_ptr(),
                                                     dj.data_ptr(), dnp.data_ptr(), dnj.data_ptr(), dex.data_ptr(), 3, 0.25,
                                                     dres32.data_ptr(), dsc32.data_ptr(), None))
    torch.cuda.synchronize()
    assert torch.equal(dres32, dres) and np.array_equal(dsc32.cpu().numpy().view(np.int64), dsc.cpu().numpy().view(np.int64))
