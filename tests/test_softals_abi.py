"""The soft-ALS half-iteration of the C ABI without a device: the entry points exist, and bad calls are answered with status
codes before any device work.

Also home of the helpers tests/test_softals_rows.py checks the kernel with."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from rsparse_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("rsparse_hip_softals_half_device", "rsparse_hip_softals_half_f64_device")


def test_library_exports_the_softals_entry_points():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.rsparse_hip_abi_version() == 6                                # additive entries: the version stays
    from rsparse_amd.engine import HipBackend
    assert callable(HipBackend.softals_half)


def test_edge_constants_mirror_the_header():
    text = (ROOT / "include" / "rsparse_wrmf_hip.h").read_text()
    for name, value in (("CHUNK", _lib.SOFTALS_CHUNK), ("SPLIT", _lib.SOFTALS_SPLIT)):
        assert int(re.search(r"#define RSPARSE_HIP_SOFTALS_%s (\d+)" % name, text).group(1)) == value
    assert int(re.search(r"#define RSPARSE_HIP_MAX_RANK (\d+)", text).group(1)) == _lib.MAX_RANK
    assert (_lib.SOFTALS_SPLIT - 1) % _lib.SOFTALS_CHUNK == 0


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("name,dt", [(NAMES[0], np.float32), (NAMES[1], np.float64)])
def test_status_codes_without_device(name, dt):
    # (host pointers: every call here is rejected by the argument checks, or is the n_rows = 0 no-op, before device work)
    fn = getattr(_lib.load(), name)
    p = np.array([0, 2, 3], dtype=np.int32)
    j = np.array([0, 2, 1], dtype=np.int32)
    x = np.ones(3, dtype=dt)
    M, W, out = np.ones((3, 4), dtype=dt), np.ones((2, 4), dtype=dt), np.empty((2, 4), dtype=dt)
    w, s, t, ss = np.ones(4), np.ones(4), np.ones(4), np.empty(1)

    def call(p=p, j=j, x=x, M=M, W=W, n=2, m=3, r=4, w=w, s=s, t=t, out=out, ss=ss):
        return fn(_vp(p), _vp(j), _vp(x), _vp(M), _vp(W), n, m, r, _vp(w), _vp(s), _vp(t), _vp(out), _vp(ss), None)

    for missing in ("p", "j", "x", "M", "out", "s"):
        assert call(**{missing: None}) == _lib.ERR_INVALID
    assert call(W=None) == _lib.ERR_INVALID                                 # w and t without W
    assert call(W=None, t=None) == _lib.ERR_INVALID                         # w without W
    assert call(W=None, w=None) == _lib.ERR_INVALID                         # t without W
    assert call(n=-1) == _lib.ERR_INVALID
    assert call(m=-1) == _lib.ERR_INVALID
    assert call(r=0) == _lib.ERR_INVALID
    assert call(r=_lib.MAX_RANK + 1) == _lib.ERR_UNSUPPORTED                # for both element types
    assert call(r=_lib.MAX_RANK + 1, out=None) == _lib.ERR_INVALID
    assert call(n=0) == _lib.OK                                             # n_rows = 0: a no-op
    assert call(n=0, W=None, w=None, t=None, ss=None) == _lib.OK


# ---- shared with tests/test_softals_rows.py -------------------------------------------------------------------------------------
def half_bound(ref, mag, length, r, eps_out):
    """|out - ref| <= eps_out |ref| + 4 (L + r) 2^-53 mag.  Both sides add, per coordinate, L terms res_t M[j_t, c] whose factor
    res_t carries the error of an r-term dot product, each in some order, in double: each is within (L + r) 2^-53 of the exact
    value, relative to the same sums over absolute values (`mag`); the factor 4 covers both sides twice over.  The store rounds
    once to the element type (eps_out = 2^-24 or 2^-53)."""
    return eps_out * np.abs(ref) + 4.0 * (length + r) * 2.0 ** -53 * mag
