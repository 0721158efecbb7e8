"""C ABI of the event-log ingest (rsparse_hip_events_to_csr_device / rsparse_hip_events_to_csr): the entry points exist and are
additive (the version stays 6), bad calls are answered with status codes before a device is touched (so these tests need none),
the host-pointer form refuses NaN, and an empty log is answered without a launch."""
import ctypes

import numpy as np
import pytest

from rsparse_amd import _lib

NAMES = ("rsparse_hip_events_to_csr_device", "rsparse_hip_events_to_csr")
SUM, COUNT, MAX, LAST = 0, 1, 2, 3


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


U, I = np.array([0, 1, 1], np.int32), np.array([2, 0, 0], np.int32)
V, T = np.array([1.0, 2.0, 3.0]), np.array([5.0, 5.0, 1.0])


def test_library_exports_the_entry_points():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NAMES[0]][1]) == len(_lib.SIGNATURES[NAMES[1]][1]) + 1     # the stream
    assert lib.rsparse_hip_abi_version() == 6
    import rsparse_amd
    from rsparse_amd.engine import HipBackend
    from rsparse_amd.events import AGGREGATES
    assert callable(HipBackend.events_to_csr) and callable(rsparse_amd.from_events) and callable(rsparse_amd.events_reference)
    assert AGGREGATES == {"sum": SUM, "count": COUNT, "max": MAX, "last": LAST}


def _caller(name):
    fn = getattr(_lib.load(), name)
    tail = (None,) if name.endswith("_device") else ()
    outs = [np.full(3, -1, np.int32), np.full(3, -1, np.int32), np.full(3, -1.0), np.full(3, -1, np.int32), np.full(3, -1.0)]
    cells = ctypes.c_int64(-1)

    def call(n=3, n_users=2, n_items=3, u=U, i=I, v=V, t=T, agg=SUM, half_life=0.0, now=0.0, has_now=0, p=outs[0], j=outs[1], x=outs[2],
             count=outs[3], latest=outs[4], cap=3, n_cells=cells):
        return fn(n, n_users, n_items, _vp(u), _vp(i), _vp(v), _vp(t), agg, half_life, now, has_now, _vp(p), _vp(j), _vp(x), _vp(count),
                  _vp(latest), cap, None if n_cells is None else ctypes.byref(n_cells), *tail)
    return call, outs, cells


@pytest.mark.parametrize("name", NAMES)
def test_status_codes_without_a_launch(name):
    # (host pointers: every call here is rejected by the argument checks before device work)
    call, outs, cells = _caller(name)
    bad = [dict(u=None), dict(i=None), dict(p=None), dict(j=None), dict(x=None), dict(n_cells=None), dict(n=-1), dict(n_users=-1),
           dict(n_items=-1), dict(n=2 ** 31), dict(n=2 ** 40), dict(agg=4), dict(agg=-1), dict(cap=-1),
           dict(agg=LAST, t=None), dict(half_life=2.0, t=None), dict(half_life=2.0, agg=MAX), dict(half_life=2.0, agg=COUNT),
           dict(half_life=2.0, agg=LAST)]
    for b in bad:
        assert call(**b) == _lib.ERR_INVALID, b
        assert _lib.load().rsparse_hip_last_error()
    assert all(np.all(o == -1) for o in outs) and cells.value == -1


def test_host_form_refuses_nan_and_answers_an_empty_log():
    call, outs, cells = _caller("rsparse_hip_events_to_csr")
    for b in (dict(v=np.array([1.0, np.nan, 3.0])), dict(t=np.array([5.0, 1.0, -np.nan])), dict(agg=LAST, t=np.array([np.nan, 1.0, 2.0]))):
        assert call(**b) == _lib.ERR_INVALID, b
    assert all(np.all(o == -1) for o in outs)
    # no event: p is all zeros and n_cells = 0, whatever else is given (or missing)
    assert call(n=0) == _lib.OK and cells.value == 0 and np.array_equal(outs[0], [0, 0, 0])
    outs[0][:] = -1
    assert call(n=0, u=None, i=None, v=None, t=None, j=None, x=None, count=None, latest=None, cap=0, n_users=2) == _lib.OK
    assert np.array_equal(outs[0], [0, 0, 0]) and cells.value == 0
    p1 = np.full(1, -1, np.int32)
    assert call(n=0, n_users=0, n_items=0, p=p1) == _lib.OK and p1[0] == 0
