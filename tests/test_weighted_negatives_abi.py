"""C ABI of the weighted negative sampler (rsparse_hip_weights_prefix_device, rsparse_hip_sample_negatives_weighted_device,
rsparse_hip_sample_negatives_weighted) without a device: the entry points exist and are additive (the version stays 6), the ctypes
signatures are the header's declarations, and every refusal the header lists is answered with its status code before a device is
touched -- every pointer here is host memory, so a call that got as far as a launch would not return a status code at all."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from rsparse_amd import _lib
from rsparse_amd import rng as R

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "rsparse_wrmf_hip.h").read_text()
NAMES = ("rsparse_hip_weights_prefix_device", "rsparse_hip_sample_negatives_weighted_device", "rsparse_hip_sample_negatives_weighted")


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


SP, SJ = np.array([0, 2, 3], np.int32), np.array([1, 4, 0], np.int32)
KP, KJ = np.array([0, 1, 1], np.int32), np.array([4], np.int32)
W = np.array([5, 1, 1, 9, 1, 2], np.uint32)
CUM = np.cumsum(W).astype(np.uint64)


def test_library_exports_the_entry_points():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.rsparse_hip_abi_version() == 6
    from rsparse_amd import WRMF
    from rsparse_amd.engine import HipBackend
    assert callable(HipBackend.weights_prefix) and callable(HipBackend.sample_negatives_weighted)
    assert callable(R.sample_negatives_weighted) and callable(WRMF.sample_negatives)


@pytest.mark.parametrize("name", NAMES)
def test_signatures_are_the_header_s(name):
    m = re.search(r"\bint %s\((.*?)\);" % name, HEADER, re.S)
    assert m, name
    params = [re.sub(r"/\*.*?\*/", "", p, flags=re.S).strip() for p in m.group(1).split(",")]

    def ctype(decl):
        if "*" in decl:
            return ctypes.c_void_p
        return {"uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64, "int": ctypes.c_int}[decl.split()[0]]
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int and argtypes == [ctype(p) for p in params], params
    # the stream is stated where the entries are declared
    for needle in ("counter (lo32(t >> 1), g, 5, hi32(t >> 1))", "B(n) = 64 * n + 4096", "item = #{i : C[i] <= r}"):
        assert needle in HEADER


def test_the_prefix_entry_refuses_without_a_launch():
    fn = _lib.load().rsparse_hip_weights_prefix_device
    cum = np.zeros(6, np.uint64)
    assert fn(None, 6, _vp(cum), None) == _lib.ERR_INVALID and _lib.load().rsparse_hip_last_error()
    assert fn(_vp(W), 6, None, None) == _lib.ERR_INVALID
    assert fn(_vp(W), -1, _vp(cum), None) == _lib.ERR_INVALID
    assert fn(_vp(W), 0, _vp(cum), None) == _lib.OK                       # no item: a no-op
    assert np.all(cum == 0)


@pytest.mark.parametrize("name", NAMES[1:])
def test_the_sampling_entries_refuse_without_a_launch(name):
    fn = getattr(_lib.load(), name)
    device = name.endswith("_device")
    out_p, out_j = np.empty(3, np.int32), np.empty(16, np.int32)
    filled32, filled64 = np.full(1, -3, np.int32), np.full(1, -3, np.int64)

    def call(seed=1, row0=0, n_rows=2, n_item=6, n=2, sp_=SP, sj=SJ, kp=KP, kj=KJ, w=W, cum=CUM, op=out_p, oj=out_j, cap=16):
        if device:
            return fn(seed, row0, n_rows, n_item, n, _vp(sp_), _vp(sj), _vp(kp), _vp(kj), _vp(cum), _vp(op), _vp(oj), cap, _vp(filled32), None)
        return fn(seed, row0, n_rows, n_item, n, _vp(sp_), _vp(sj), _vp(kp), _vp(kj), _vp(w), _vp(op), _vp(oj), cap, _vp(filled64))

    bad = [dict(sp_=None), dict(sj=None), dict(op=None), dict(kp=None), dict(kj=None), dict(n_rows=-1), dict(n_item=-1), dict(n=0),
           dict(n=-5), dict(row0=-1), dict(cap=-1), dict(row0=2 ** 32 - 1), dict(w=None, cum=None)]
    if device:
        bad.append(dict(oj=None))
    else:
        bad += [dict(w=np.array([5, 1, 0, 9, 1, 2], np.uint32)),                       # a zero weight
                dict(kj=np.array([2], np.int32)),                                     # the lists are checked: keep no subset of seen
                dict(sj=np.array([4, 1, 0], np.int32)), dict(sj=np.array([1, 6, 0], np.int32)), dict(sp_=np.array([1, 2, 3], np.int32)),
                dict(cap=4)]                                                          # the rows need 5 entries
    for b in bad:
        assert call(**b) == _lib.ERR_INVALID, b
        assert _lib.load().rsparse_hip_last_error()
    assert call(n=8193) == _lib.ERR_UNSUPPORTED
    assert call(n=8193, w=None, cum=None) == _lib.ERR_UNSUPPORTED          # the checks of the uniform entries come first, in their order
    assert call(n_rows=0) == _lib.OK                                       # no row: a no-op
    assert call(n_rows=0, kp=None, kj=None) == _lib.OK
    if not device:
        # the sizes only (out_j NULL): out_p is written on the host, nothing is launched, the count is zeroed
        assert call(oj=None, cap=0) == _lib.OK and np.array_equal(out_p, [0, 3, 5]) and filled64[0] == 0
