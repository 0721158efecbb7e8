"""The weighted ItemKNN entries of the C ABI without a device: the four symbols exist, the version stays, and every bad call is
answered with its status code and message before any device work."""
import ctypes

import numpy as np

from rsparse_amd import _lib

NAMES = ("rsparse_hip_cooc_neighbors_weighted_device", "rsparse_hip_knn_recommend_weighted_device", "rsparse_hip_cooc_neighbors_weighted",
         "rsparse_hip_knn_recommend_weighted")


def test_library_exports_the_weighted_entry_points():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.rsparse_hip_abi_version() == 6                                # additive entries: the version stays
    assert len(_lib.SIGNATURES["rsparse_hip_cooc_neighbors_weighted_device"][1]) == 18
    # today's arguments plus d_xv
    assert len(_lib.SIGNATURES["rsparse_hip_knn_recommend_weighted_device"][1]) == len(_lib.SIGNATURES["rsparse_hip_knn_recommend_device"][1]) + 1
    assert len(_lib.SIGNATURES["rsparse_hip_knn_recommend_weighted"][1]) == len(_lib.SIGNATURES["rsparse_hip_knn_recommend"][1]) + 1
    from rsparse_amd.engine import HipBackend
    assert callable(HipBackend.cooc_neighbors_weighted)
    import inspect
    assert inspect.signature(HipBackend.knn_recommend).parameters["xv"].default is None


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _answer(rc, code, text):
    assert rc == code, (rc, _lib.load().rsparse_hip_last_error())
    assert text in _lib.load().rsparse_hip_last_error().decode(), _lib.load().rsparse_hip_last_error()


# 3 users x 4 items: rows {0, 2}, {1}, {0, 1, 3}
P = np.array([0, 2, 3, 6], dtype=np.int32)
J = np.array([0, 2, 1, 0, 1, 3], dtype=np.int32)
V = np.array([1, 2, 3, 4, 5, 6], dtype=np.uint32)
IP = np.array([0, 2, 4, 5, 6], dtype=np.int32)
IU = np.array([0, 2, 1, 2, 0, 2], dtype=np.int32)
IL = np.array([1, 4, 3, 5, 2, 6], dtype=np.uint32)
A = np.ones(4)
H_BAD = (-1.0, np.nan, np.inf, -np.inf, 2.0 ** 401)


def test_cooc_neighbors_weighted_device_status_codes():
    # (host pointers: every call here is rejected by the argument checks, or is the empty item range, before device work)
    fn = _lib.load().rsparse_hip_cooc_neighbors_weighted_device
    nb, sums = np.empty((4, 2), np.int32), np.empty((4, 2), np.uint64)

    def call(ip=IP, iu=IU, il=IL, up=P, uj=J, ur=V, n_users=3, n_items=4, item0=0, item1=4, a=A, b=A, h=0.0, K=2, ws_rows=0, nb=nb,
             sums=sums):
        return fn(_vp(ip), _vp(iu), _vp(il), _vp(up), _vp(uj), _vp(ur), n_users, n_items, item0, item1, _vp(a), _vp(b), h, K, ws_rows,
                  _vp(nb), _vp(sums), None)

    for missing in ("ip", "iu", "il", "up", "uj", "ur", "a", "b", "nb", "sums"):
        _answer(call(**{missing: None}), _lib.ERR_INVALID, "NULL")
    _answer(call(n_users=-1), _lib.ERR_INVALID, "bad dimensions")
    _answer(call(n_items=-1), _lib.ERR_INVALID, "bad dimensions")
    for item0, item1 in ((-1, 4), (3, 2), (0, 5)):
        _answer(call(item0=item0, item1=item1), _lib.ERR_INVALID, "item0 <= item1 <= n_items")
    _answer(call(K=0), _lib.ERR_INVALID, "K < 1")
    _answer(call(ws_rows=-1), _lib.ERR_INVALID, "ws_rows < 0")
    for h in H_BAD:
        _answer(call(h=h), _lib.ERR_INVALID, "h is not finite or outside [0, 2^400]")
    _answer(call(K=_lib.KNN_MAX_NEIGHBORS + 1), _lib.ERR_UNSUPPORTED, "K > 256")
    assert call(K=_lib.KNN_MAX_NEIGHBORS + 1, nb=None) == _lib.ERR_INVALID   # the pointers are looked at first
    # an empty range is a no-op, at the largest h, and beyond the binary entry's n_users limit (the 2^53 bound replaces it)
    assert call(item0=2, item1=2, h=2.0 ** 400) == _lib.OK
    assert call(item0=4, item1=4, n_users=_lib.KNN_MAX_USERS + 1) == _lib.OK


def test_knn_recommend_weighted_device_status_codes():
    fn = _lib.load().rsparse_hip_knn_recommend_weighted_device
    nb, q = np.zeros((4, 2), np.int32), np.ones((4, 2), np.uint32)
    res, sc = np.empty((3, 2), np.int32), np.empty((3, 2), np.int64)
    ex = np.array([1], dtype=np.int32)

    def call(xp=P, xj=J, xv=V, n_rows=3, n_items=4, nb=nb, q=q, K=2, nr_p=None, nr_j=None, ex=None, n_ex=0, k=2, ws_rows=0, res=res, sc=sc):
        return fn(_vp(xp), _vp(xj), _vp(xv), n_rows, n_items, _vp(nb), _vp(q), K, _vp(nr_p), _vp(nr_j), _vp(ex), n_ex, k, ws_rows,
                  _vp(res), _vp(sc), None)

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
    # d_xv = NULL is accepted: with it the same refusals and no-ops as with the weights
    _answer(call(xv=None, k=0), _lib.ERR_INVALID, "K < 1 or k < 1")
    assert call(xv=None, n_rows=0, ex=ex, n_ex=1) == _lib.OK                 # no row: a no-op
    assert call(n_rows=0, ex=ex, n_ex=1) == _lib.OK


def test_host_forms_check_their_arrays_first():
    lib = _lib.load()
    nb, sums = np.empty((4, 2), np.int32, order="F"), np.empty((4, 2), np.uint64, order="F")

    def fit(p=P, j=J, l=V, r=V, n_users=3, n_items=4, a=A, b=A, h=0.0, K=2, nb=nb, sums=sums):
        return lib.rsparse_hip_cooc_neighbors_weighted(_vp(p), _vp(j), _vp(l), _vp(r), n_users, n_items, _vp(a), _vp(b), h, K, _vp(nb),
                                                       _vp(sums))

    for missing in ("p", "a", "b", "nb", "sums"):
        _answer(fit(**{missing: None}), _lib.ERR_INVALID, "NULL")
    _answer(fit(j=None), _lib.ERR_INVALID, "j is NULL")
    _answer(fit(l=None), _lib.ERR_INVALID, "l or r is NULL")
    _answer(fit(r=None), _lib.ERR_INVALID, "l or r is NULL")
    _answer(fit(n_users=-1), _lib.ERR_INVALID, "bad dimensions")
    _answer(fit(K=0), _lib.ERR_INVALID, "K < 1")
    _answer(fit(K=257), _lib.ERR_UNSUPPORTED, "K > 256")
    for h in H_BAD:
        _answer(fit(h=h), _lib.ERR_INVALID, "h is not finite or outside [0, 2^400]")
    _answer(fit(p=np.array([1, 2, 3, 6], np.int32)), _lib.ERR_INVALID, "p[0] != 0")
    _answer(fit(p=np.array([0, 3, 2, 6], np.int32)), _lib.ERR_INVALID, "p decreases")
    _answer(fit(j=np.array([0, 4, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "a column outside [0, n_items)")
    _answer(fit(j=np.array([0, -1, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "a column outside [0, n_items)")
    _answer(fit(j=np.array([2, 0, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "not strictly ascending")
    for bad in (0.0, 2.0 ** -201, 2.0 ** 201, np.nan, np.inf, -1.0):
        t = A.copy()
        t[2] = bad
        _answer(fit(a=t), _lib.ERR_INVALID, "outside [2^-200, 2^200]")
        _answer(fit(b=t), _lib.ERR_INVALID, "outside [2^-200, 2^200]")
    # the 2^53 bound: the largest column has 2 users, so max(l) max(r) must stay below 2^52
    big_l, big_r = V.copy(), V.copy()
    big_l[1], big_r[4] = 2 ** 26, 2 ** 26
    _answer(fit(l=big_l, r=big_r), _lib.ERR_INVALID, ">= 2^53")
    assert fit(n_items=0, p=np.zeros(4, np.int32)) == _lib.OK                # no item: a no-op

    tb, q = np.ones((4, 2), np.int32, order="F"), np.ones((4, 2), np.uint32, order="F")
    res, sc = np.empty((3, 2), np.int32, order="F"), np.empty((3, 2), np.int64, order="F")
    ex = np.array([1], dtype=np.int32)

    def rec(xp=P, xj=J, xv=V, n_rows=3, n_items=4, tb=tb, q=q, K=2, nr_p=None, nr_j=None, ex=None, n_ex=0, k=2, res=res, sc=sc):
        return lib.rsparse_hip_knn_recommend_weighted(_vp(xp), _vp(xj), _vp(xv), n_rows, n_items, _vp(tb), _vp(q), K, _vp(nr_p), _vp(nr_j),
                                                      _vp(ex), n_ex, k, _vp(res), _vp(sc))

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
    heavy = V.copy()
    heavy[3] = 2 ** 16
    _answer(rec(xv=heavy), _lib.ERR_INVALID, "above 2^16 - 1")
    # a row of 2^15 + 1 items at 2^16 - 1 each: (2^15 + 1)(2^16 - 1) >= 2^31
    n_wide = 2 ** 15 + 1
    wide_p = np.array([0, n_wide], dtype=np.int32)
    wide_j = np.arange(n_wide, dtype=np.int32)
    wide_tb, wide_q = np.ones((n_wide, 1), np.int32, order="F"), np.ones((n_wide, 1), np.uint32, order="F")
    one_res, one_sc = np.empty((1, 1), np.int32), np.empty((1, 1), np.int64)
    wide = lambda xv: lib.rsparse_hip_knn_recommend_weighted(_vp(wide_p), _vp(wide_j), _vp(xv), 1, n_wide, _vp(wide_tb), _vp(wide_q), 1, None,
                                                             None, None, 0, 1, _vp(one_res), _vp(one_sc))
    _answer(wide(np.full(n_wide, 2 ** 16 - 1, dtype=np.uint32)), _lib.ERR_INVALID, "sum to 2^31 or more")
    _answer(rec(xv=None, k=1025), _lib.ERR_UNSUPPORTED, "k > 1024")          # x_v = NULL is accepted: the same answers
    assert rec(n_rows=0, xp=np.zeros(1, np.int32), ex=ex, n_ex=1) == _lib.OK  # no row: a no-op
    assert rec(xv=None, n_rows=0, xp=np.zeros(1, np.int32), ex=ex, n_ex=1) == _lib.OK
