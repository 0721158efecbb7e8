"""The ItemKNN entries of the C ABI without a device: the four symbols exist, the version stays, and every bad call is answered
with its status code and message before any device work."""
import ctypes
import re
from pathlib import Path

import numpy as np

from rsparse_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("rsparse_hip_cooc_neighbors_device", "rsparse_hip_knn_recommend_device", "rsparse_hip_cooc_neighbors",
         "rsparse_hip_knn_recommend")


def test_library_exports_the_itemknn_entry_points():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.rsparse_hip_abi_version() == 6                                # additive entries: the version stays
    from rsparse_amd.engine import HipBackend
    assert callable(HipBackend.cooc_neighbors) and callable(HipBackend.knn_recommend)


def test_constants_mirror_the_header():
    text = (ROOT / "include" / "rsparse_wrmf_hip.h").read_text()
    value = lambda name: eval(re.search(r"#define RSPARSE_HIP_KNN_%s (.+)" % name, text).group(1).replace("ull", ""))
    for name in ("COUNT", "COSINE", "JACCARD", "MAX_USERS", "MAX_NEIGHBORS", "MAX_TOPK", "WS_BYTES", "SPAN", "LDS_CAND"):
        assert value(name) == getattr(_lib, "KNN_" + name), name
    assert _lib.KNN_MAX_USERS == 2 ** 26 and _lib.KNN_WS_BYTES == 2 ** 30
    assert _lib.KNN_LDS_CAND >= _lib.KNN_MAX_TOPK >= _lib.KNN_MAX_NEIGHBORS


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _answer(rc, code, text):
    assert rc == code, (rc, _lib.load().rsparse_hip_last_error())
    assert text in _lib.load().rsparse_hip_last_error().decode(), _lib.load().rsparse_hip_last_error()


# 3 users x 4 items: rows {0, 2}, {1}, {0, 1, 3}
P = np.array([0, 2, 3, 6], dtype=np.int32)
J = np.array([0, 2, 1, 0, 1, 3], dtype=np.int32)
IP = np.array([0, 2, 4, 5, 6], dtype=np.int32)
IU = np.array([0, 2, 1, 2, 0, 2], dtype=np.int32)


def test_cooc_neighbors_device_status_codes():
    # (host pointers: every call here is rejected by the argument checks, or is the empty item range, before device work)
    fn = _lib.load().rsparse_hip_cooc_neighbors_device
    nb, ct = np.empty((4, 2), np.int32), np.empty((4, 2), np.int32)

    def call(ip=IP, iu=IU, up=P, uj=J, n_users=3, n_items=4, item0=0, item1=4, sim=_lib.KNN_COSINE, K=2, ws_rows=0, nb=nb, ct=ct):
        return fn(_vp(ip), _vp(iu), _vp(up), _vp(uj), n_users, n_items, item0, item1, sim, K, ws_rows, _vp(nb), _vp(ct), None)

    for missing in ("ip", "iu", "up", "uj", "nb", "ct"):
        _answer(call(**{missing: None}), _lib.ERR_INVALID, "NULL")
    _answer(call(n_users=-1), _lib.ERR_INVALID, "bad dimensions")
    _answer(call(n_items=-1), _lib.ERR_INVALID, "bad dimensions")
    for item0, item1 in ((-1, 4), (3, 2), (0, 5)):
        _answer(call(item0=item0, item1=item1), _lib.ERR_INVALID, "item0 <= item1 <= n_items")
    for sim in (-1, 3):
        _answer(call(sim=sim), _lib.ERR_INVALID, "unknown similarity")
    _answer(call(K=0), _lib.ERR_INVALID, "K < 1")
    _answer(call(ws_rows=-1), _lib.ERR_INVALID, "ws_rows < 0")
    _answer(call(K=_lib.KNN_MAX_NEIGHBORS + 1), _lib.ERR_UNSUPPORTED, "K > 256")
    _answer(call(n_users=_lib.KNN_MAX_USERS + 1), _lib.ERR_UNSUPPORTED, "n_users > 2^26")
    assert call(n_users=_lib.KNN_MAX_USERS + 1, nb=None) == _lib.ERR_INVALID   # the pointers are looked at first
    assert call(item0=2, item1=2) == _lib.OK                                 # an empty range: a no-op


def test_knn_recommend_device_status_codes():
    fn = _lib.load().rsparse_hip_knn_recommend_device
    nb, q = np.zeros((4, 2), np.int32), np.ones((4, 2), np.uint32)
    res, sc = np.empty((3, 2), np.int32), np.empty((3, 2), np.int64)
    ex = np.array([1], dtype=np.int32)

    def call(xp=P, xj=J, n_rows=3, n_items=4, nb=nb, q=q, K=2, nr_p=None, nr_j=None, ex=None, n_ex=0, k=2, ws_rows=0, res=res, sc=sc):
        return fn(_vp(xp), _vp(xj), n_rows, n_items, _vp(nb), _vp(q), K, _vp(nr_p), _vp(nr_j), _vp(ex), n_ex, k, ws_rows, _vp(res),
                  _vp(sc), None)

    for missing in ("xp", "xj", "nb", "q", "res", "sc"):
        _answer(call(**{missing: None}), _lib.ERR_INVALID, "NULL")
    _answer(call(n_rows=-1), _lib.ERR_INVALID, "bad dimensions")
    _answer(call(n_items=-1), _lib.ERR_INVALID, "bad dimensions")
    _answer(call(K=0), _lib.ERR_INVALID, "K < 1 or k < 1")
    _answer(call(k=0), _lib.ERR_INVALID, "K < 1 or k < 1")
    _answer(call(ws_rows=-1), _lib.ERR_INVALID, "ws_rows < 0")
    _answer(call(nr_p=P), _lib.ERR_INVALID, "nr_p without nr_j")
    _answer(call(n_ex=-1), _lib.ERR_INVALID, "bad exclude")
    _answer(call(n_ex=1), _lib.ERR_INVALID, "bad exclude")
    _answer(call(K=_lib.KNN_MAX_NEIGHBORS + 1), _lib.ERR_UNSUPPORTED, "K > 256")
    _answer(call(k=_lib.KNN_MAX_TOPK + 1), _lib.ERR_UNSUPPORTED, "k > 1024")
    assert call(n_rows=0, ex=ex, n_ex=1) == _lib.OK                          # no row: a no-op


def test_host_forms_check_their_arrays_first():
    lib = _lib.load()
    nb, ct = np.empty((4, 2), np.int32, order="F"), np.empty((4, 2), np.int32, order="F")

    def fit(p=P, j=J, n_users=3, n_items=4, sim=_lib.KNN_JACCARD, K=2, nb=nb, ct=ct):
        return lib.rsparse_hip_cooc_neighbors(_vp(p), _vp(j), n_users, n_items, sim, K, _vp(nb), _vp(ct))

    for missing in ("p", "nb", "ct"):
        _answer(fit(**{missing: None}), _lib.ERR_INVALID, "NULL")
    _answer(fit(j=None), _lib.ERR_INVALID, "j is NULL")
    _answer(fit(K=257), _lib.ERR_UNSUPPORTED, "K > 256")
    _answer(fit(sim=7), _lib.ERR_INVALID, "unknown similarity")
    _answer(fit(n_users=_lib.KNN_MAX_USERS + 1), _lib.ERR_UNSUPPORTED, "n_users > 2^26")
    _answer(fit(p=np.array([1, 2, 3, 6], np.int32)), _lib.ERR_INVALID, "p[0] != 0")
    _answer(fit(p=np.array([0, 3, 2, 6], np.int32)), _lib.ERR_INVALID, "p decreases")
    _answer(fit(j=np.array([0, 4, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "a column outside [0, n_items)")
    _answer(fit(j=np.array([0, -1, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "a column outside [0, n_items)")
    _answer(fit(j=np.array([2, 0, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "not strictly ascending")
    assert fit(n_items=0, p=np.zeros(4, np.int32)) == _lib.OK               # no item: a no-op

    tb, q = np.ones((4, 2), np.int32, order="F"), np.ones((4, 2), np.uint32, order="F")
    res, sc = np.empty((3, 2), np.int32, order="F"), np.empty((3, 2), np.int64, order="F")
    ex = np.array([1], dtype=np.int32)

    def rec(xp=P, xj=J, n_rows=3, n_items=4, tb=tb, q=q, K=2, nr_p=None, nr_j=None, ex=None, n_ex=0, k=2, res=res, sc=sc):
        return lib.rsparse_hip_knn_recommend(_vp(xp), _vp(xj), n_rows, n_items, _vp(tb), _vp(q), K, _vp(nr_p), _vp(nr_j), _vp(ex), n_ex,
                                             k, _vp(res), _vp(sc))

    for missing in ("xp", "tb", "q", "res", "sc"):
        _answer(rec(**{missing: None}), _lib.ERR_INVALID, "NULL")
    _answer(rec(xj=None), _lib.ERR_INVALID, "x_j is NULL")
    _answer(rec(k=1025), _lib.ERR_UNSUPPORTED, "k > 1024")
    _answer(rec(K=0), _lib.ERR_INVALID, "K < 1 or k < 1")
    _answer(rec(n_ex=1), _lib.ERR_INVALID, "bad exclude")
    _answer(rec(nr_p=P), _lib.ERR_INVALID, "nr_p without nr_j")
    _answer(rec(xp=np.array([0, 3, 2, 6], np.int32)), _lib.ERR_INVALID, "x_p decreases")
    _answer(rec(xj=np.array([0, 2, 1, 0, 1, 4], np.int32)), _lib.ERR_INVALID, "x_j has a column outside [0, n_items)")
    _answer(rec(nr_p=P, nr_j=np.array([0, 2, 1, 0, 1, 9], np.int32)), _lib.ERR_INVALID, "nr_j has a column outside [0, n_items)")
    big = q.copy(order="F")
    big[2, 1] = 2 ** 30 + 1
    _answer(rec(q=big), _lib.ERR_INVALID, "above 2^30")
    assert rec(n_rows=0, xp=np.zeros(1, np.int32), ex=ex, n_ex=1) == _lib.OK  # no row: a no-op
