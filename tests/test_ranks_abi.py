"""The C ABI of the full-ranking metrics on the device: the host-pointer entry rsparse_hip_held_out_ranks against the two device
entries on one small case, outputs left out, and the status codes."""
import ctypes

import numpy as np
import pytest
import torch

from rsparse_amd import _lib

pytestmark = pytest.mark.gpu


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _case():
    rng = np.random.default_rng(3)
    n, m, r = 70, 1500, 12
    x = np.asfortranarray(rng.integers(-3, 4, size=(n, r)).astype(np.float64))     # nr x rank, column-major
    y = np.asfortranarray(rng.integers(-3, 4, size=(r, m)).astype(np.float64))     # rank x nc, column-major
    lens = rng.integers(0, 30, size=n)
    lens[0], lens[5] = 10, 0
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    j = np.concatenate([np.sort(rng.choice(m, size=l, replace=False)) for l in lens]).astype(np.int32)
    w = rng.integers(1, 6, size=j.size).astype(np.float64)
    nlens = rng.integers(0, 50, size=n)
    nlens[0] = 20
    nr_p = np.concatenate([[0], np.cumsum(nlens)]).astype(np.int32)
    nr_j = np.concatenate([np.sort(rng.choice(m, size=l, replace=False)) for l in nlens]).astype(np.int32)
    nr_j[:20] = np.sort(np.concatenate([j[:3], np.setdiff1d(np.arange(m), j[:10])[:17]]))   # three held-out items of user 0 are masked
    excl1 = np.array([2, 1, 2, 900, 0, m + 5], dtype=np.int32)                     # 1-based, unsorted, repeated, out of range
    return n, m, r, x, y, p, j, w, nr_p, nr_j, excl1


def test_host_entry_equals_the_device_entries():
    lib = _lib.load()
    n, m, r, x, y, p, j, w, nr_p, nr_j, excl1 = _case()
    above, tied = np.full(j.size, 7, np.int32), np.full(j.size, 7, np.int32)
    n_adm = np.full(n, 7, np.int32)
    mpr, auc, mrr, sums = np.empty(n), np.empty(n), np.empty(n), np.empty((n, 3))
    _lib.check(lib.rsparse_hip_held_out_ranks(_vp(x), _vp(y), n, m, r, _vp(nr_p), _vp(nr_j), _vp(excl1), excl1.size, _vp(p), _vp(j),
                                              _vp(w), _vp(above), _vp(tied), _vp(n_adm), _vp(mpr), _vp(auc), _vp(mrr), _vp(sums)))
    # the device entries on the same operands: row-major fp32 factors, sorted 0-based exclusions
    U, V = _dev(x.astype(np.float32)), _dev(np.ascontiguousarray(y.T).astype(np.float32))
    ex0 = _dev(np.array([0, 1, 899], dtype=np.int32))
    dp, dj, dw = _dev(p), _dev(j), _dev(w)
    d_above = torch.empty(j.size, dtype=torch.int32, device="cuda:0")
    d_tied, d_nadm = torch.empty_like(d_above), torch.empty(n, dtype=torch.int32, device="cuda:0")
    _lib.check(lib.rsparse_hip_held_out_ranks_device(U.data_ptr(), V.data_ptr(), n, m, r, _dev(nr_p).data_ptr(), _dev(nr_j).data_ptr(),
                                                     ex0.data_ptr(), 3, dp.data_ptr(), dj.data_ptr(), 0, d_above.data_ptr(),
                                                     d_tied.data_ptr(), d_nadm.data_ptr(), None))
    d_out = torch.empty((6, n), dtype=torch.float64, device="cuda:0")
    _lib.check(lib.rsparse_hip_rank_summary_device(n, dp.data_ptr(), dw.data_ptr(), d_above.data_ptr(), d_tied.data_ptr(),
                                                   d_nadm.data_ptr(), d_out[0].data_ptr(), d_out[1].data_ptr(), d_out[2].data_ptr(),
                                                   d_out[3].data_ptr(), None))
    torch.cuda.synchronize()
    assert np.array_equal(above, d_above.cpu().numpy()) and np.array_equal(tied, d_tied.cpu().numpy())
    assert np.array_equal(n_adm, d_nadm.cpu().numpy())
    o = d_out.cpu().numpy()
    bits = lambda v: np.ascontiguousarray(v).view(np.int64)
    assert np.array_equal(bits(mpr), bits(o[0])) and np.array_equal(bits(auc), bits(o[1])) and np.array_equal(bits(mrr), bits(o[2]))
    assert np.array_equal(bits(sums.ravel()), bits(o[3:].ravel()))
    # and both against numpy
    from rsparse_amd.metrics import percentile_ranks, rank_summary
    import scipy.sparse as sp
    act = sp.csr_matrix((w, j, p), shape=(n, m))
    nr = sp.csr_matrix((np.ones(nr_j.size), nr_j, nr_p), shape=(n, m))
    ra, rt, rn = percentile_ranks(x @ y, act, nr, [0, 1, 899])
    assert np.array_equal(above, ra.data) and np.array_equal(tied, rt.data) and np.array_equal(n_adm, rn)
    assert (above == -1).any() and np.isnan(mpr[5]) and np.isnan(auc[5]) and np.isnan(mrr[5])
    ref = rank_summary(ra, rt, rn, act)
    ok = ~np.isnan(ref["mpr"])
    assert np.allclose(mpr[ok], ref["mpr"][ok], rtol=1e-13, atol=0) and np.array_equal(np.isnan(mpr), ~ok)
    # outputs left out: what is asked for comes back unchanged
    a2, m2 = np.full(j.size, 7, np.int32), np.empty(n)
    _lib.check(lib.rsparse_hip_held_out_ranks(_vp(x), _vp(y), n, m, r, _vp(nr_p), _vp(nr_j), _vp(excl1), excl1.size, _vp(p), _vp(j),
                                              None, _vp(a2), None, None, None, None, _vp(m2), None))
    assert np.array_equal(a2, above) and np.array_equal(bits(m2), bits(mrr))
    n2 = np.full(n, 7, np.int32)
    _lib.check(lib.rsparse_hip_held_out_ranks(_vp(x), _vp(y), n, m, r, None, None, None, 0, _vp(p), _vp(j), None, None, None,
                                              _vp(n2), None, None, None, None))
    assert (n2 == m).all()


def test_status_codes_on_the_device():
    lib = _lib.load()
    n, m, r, x, y, p, j, w, nr_p, nr_j, excl1 = _case()
    U, V = _dev(x.astype(np.float32)), _dev(np.ascontiguousarray(y.T).astype(np.float32))
    dp, dj = _dev(p), _dev(j)
    a = torch.empty(j.size, dtype=torch.int32, device="cuda:0")
    t, na = torch.empty_like(a), torch.empty(n, dtype=torch.int32, device="cuda:0")

    def call(U=U.data_ptr(), V=V.data_ptr(), n=n, m=m, r=r, ex=None, n_ex=0, p=dp.data_ptr(), j=dj.data_ptr(), chunk=0,
             a=a.data_ptr(), t=t.data_ptr(), na=na.data_ptr()):
        return lib.rsparse_hip_held_out_ranks_device(U, V, n, m, r, None, None, ex, n_ex, p, j, chunk, a, t, na, None)

    assert call() == _lib.OK
    for bad in (dict(U=None), dict(V=None), dict(p=None), dict(j=None), dict(a=None), dict(t=None), dict(na=None), dict(n=-1),
                dict(m=-1), dict(r=0), dict(chunk=-1), dict(n_ex=2)):
        assert call(**bad) == _lib.ERR_INVALID, bad
        assert lib.rsparse_hip_last_error()
    assert call(r=257) == _lib.ERR_UNSUPPORTED
    assert call(n=0) == _lib.OK
    torch.cuda.synchronize()
    out = torch.empty(n, dtype=torch.float64, device="cuda:0")
    summ = lambda **k: lib.rsparse_hip_rank_summary_device(
        k.get("n", n), dp.data_ptr(), k.get("w", None), a.data_ptr(), t.data_ptr(), na.data_ptr(), k.get("mpr", None),
        k.get("auc", out.data_ptr()), None, None, None)
    assert summ() == _lib.OK                                  # auc alone needs no weights
    assert summ(auc=None) == _lib.ERR_INVALID                 # nothing asked for
    assert summ(mpr=out.data_ptr()) == _lib.ERR_INVALID       # mpr needs the weights
    assert summ(n=-1) == _lib.ERR_INVALID
    torch.cuda.synchronize()
