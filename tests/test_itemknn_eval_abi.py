"""The evaluation entries of ItemKNN in the C ABI without a device: the five symbols exist, the version stays, and every bad call
is answered with its status code and message before any device work."""
import ctypes

import numpy as np
import pytest

from rsparse_amd import _lib

NAMES = ("rsparse_hip_knn_score_pairs_device", "rsparse_hip_knn_top_candidates_device", "rsparse_hip_knn_held_out_ranks_device",
         "rsparse_hip_knn_top_candidates", "rsparse_hip_knn_held_out_ranks")


def test_library_exports_the_evaluation_entry_points():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.rsparse_hip_abi_version() == 6                                # additive entries: the version stays
    from rsparse_amd.engine import HipBackend
    assert callable(HipBackend.knn_score_pairs) and callable(HipBackend.knn_top_candidates) and callable(HipBackend.knn_held_out_ranks)


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _answer(rc, code, text):
    assert rc == code, (rc, _lib.load().rsparse_hip_last_error())
    assert text in _lib.load().rsparse_hip_last_error().decode(), _lib.load().rsparse_hip_last_error()


# 3 users x 4 items: rows {0, 2}, {1}, {0, 1, 3}; the second pattern of an entry (pairs, candidates, actual) is the same one
P = np.array([0, 2, 3, 6], dtype=np.int32)
J = np.array([0, 2, 1, 0, 1, 3], dtype=np.int32)
NB, Q = np.zeros((4, 2), np.int32), np.ones((4, 2), np.uint32)
EX = np.array([1], dtype=np.int32)


def common_refusals(call, pointers):
    """the refusals every device entry shares; `call` takes keyword overrides (host pointers: nothing here reaches a device)"""
    for missing in pointers:
        _answer(call(**{missing: None}), _lib.ERR_INVALID, "NULL")
    _answer(call(n_rows=-1), _lib.ERR_INVALID, "bad dimensions")
    _answer(call(n_items=-1), _lib.ERR_INVALID, "bad dimensions")
    _answer(call(K=0), _lib.ERR_INVALID, "K < 1")
    _answer(call(ws_rows=-1), _lib.ERR_INVALID, "ws_rows < 0")
    _answer(call(K=_lib.KNN_MAX_NEIGHBORS + 1), _lib.ERR_UNSUPPORTED, "K > 256")
    assert call(K=_lib.KNN_MAX_NEIGHBORS + 1, xp=None) == _lib.ERR_INVALID   # the pointers are looked at first


def filter_refusals(call):
    _answer(call(nr_p=P), _lib.ERR_INVALID, "nr_p without nr_j")
    _answer(call(n_ex=-1), _lib.ERR_INVALID, "bad exclude")
    _answer(call(n_ex=1), _lib.ERR_INVALID, "bad exclude")


def test_score_pairs_device_status_codes():
    fn = _lib.load().rsparse_hip_knn_score_pairs_device
    out = np.empty(6, np.int64)

    def call(xp=P, xj=J, xv=None, n_rows=3, n_items=4, nb=NB, q=Q, K=2, pp=P, pj=J, ws_rows=0, out=out):
        return fn(_vp(xp), _vp(xj), _vp(xv), n_rows, n_items, _vp(nb), _vp(q), K, _vp(pp), _vp(pj), ws_rows, _vp(out), None)

    common_refusals(call, ("xp", "xj", "nb", "q", "pp", "pj", "out"))
    assert call(n_rows=0) == _lib.OK                                         # no row: a no-op, with or without weights
    assert call(n_rows=0, xv=np.ones(6, np.uint32)) == _lib.OK


def test_top_candidates_device_status_codes():
    fn = _lib.load().rsparse_hip_knn_top_candidates_device
    res, sc = np.empty((3, 2), np.int32), np.empty((3, 2), np.int64)

    def call(xp=P, xj=J, xv=None, n_rows=3, n_items=4, nb=NB, q=Q, K=2, cp=P, cj=J, nr_p=None, nr_j=None, ex=None, n_ex=0, k=2, ws_rows=0,
             res=res, sc=sc):
        return fn(_vp(xp), _vp(xj), _vp(xv), n_rows, n_items, _vp(nb), _vp(q), K, _vp(cp), _vp(cj), _vp(nr_p), _vp(nr_j), _vp(ex), n_ex, k,
                  ws_rows, _vp(res), _vp(sc), None)

    common_refusals(call, ("xp", "xj", "nb", "q", "cp", "cj", "res", "sc"))
    filter_refusals(call)
    _answer(call(k=0), _lib.ERR_INVALID, "K < 1 or k < 1")
    _answer(call(k=_lib.KNN_MAX_TOPK + 1), _lib.ERR_UNSUPPORTED, "k > 1024")
    assert call(n_rows=0, ex=EX, n_ex=1) == _lib.OK


def test_held_out_ranks_device_status_codes():
    fn = _lib.load().rsparse_hip_knn_held_out_ranks_device
    above, tied, n_adm = np.empty(6, np.int32), np.empty(6, np.int32), np.empty(3, np.int32)

    def call(xp=P, xj=J, xv=None, n_rows=3, n_items=4, nb=NB, q=Q, K=2, ap=P, aj=J, nr_p=None, nr_j=None, ex=None, n_ex=0, ws_rows=0,
             above=above, tied=tied, n_adm=n_adm):
        return fn(_vp(xp), _vp(xj), _vp(xv), n_rows, n_items, _vp(nb), _vp(q), K, _vp(ap), _vp(aj), _vp(nr_p), _vp(nr_j), _vp(ex), n_ex,
                  ws_rows, _vp(above), _vp(tied), _vp(n_adm), None)

    common_refusals(call, ("xp", "xj", "nb", "q", "ap", "aj", "above", "tied", "n_adm"))
    filter_refusals(call)
    assert call(n_rows=0, ex=EX, n_ex=1) == _lib.OK


TB, QF = np.ones((4, 2), np.int32, order="F"), np.ones((4, 2), np.uint32, order="F")


def host_row_refusals(call):
    """what the host forms check of the arrays they share with rsparse_hip_knn_recommend_weighted"""
    _answer(call(xj=None), _lib.ERR_INVALID, "x_j is NULL")
    _answer(call(K=0), _lib.ERR_INVALID, "K < 1")
    _answer(call(K=257), _lib.ERR_UNSUPPORTED, "K > 256")
    _answer(call(n_rows=-1), _lib.ERR_INVALID, "bad dimensions")
    _answer(call(n_ex=1), _lib.ERR_INVALID, "bad exclude")
    _answer(call(nr_p=P), _lib.ERR_INVALID, "nr_p without nr_j")
    _answer(call(xp=np.array([1, 2, 3, 6], np.int32)), _lib.ERR_INVALID, "x_p[0] != 0")
    _answer(call(xp=np.array([0, 3, 2, 6], np.int32)), _lib.ERR_INVALID, "x_p decreases")
    _answer(call(xj=np.array([0, 2, 1, 0, 1, 4], np.int32)), _lib.ERR_INVALID, "x_j has a column outside [0, n_items)")
    _answer(call(xv=np.array([1, 1, 1, 1, 1, 1 << 16], np.uint32)), _lib.ERR_INVALID, "above 2^16 - 1")
    _answer(call(nr_p=P, nr_j=np.array([0, 2, 1, 0, 1, 9], np.int32)), _lib.ERR_INVALID, "nr_j has a column outside [0, n_items)")
    big = QF.copy(order="F")
    big[2, 1] = 2 ** 30 + 1
    _answer(call(q=big), _lib.ERR_INVALID, "above 2^30")


def test_top_candidates_host_form_checks_its_arrays_first():
    lib = _lib.load()
    res, sc = np.empty((3, 2), np.int32, order="F"), np.empty((3, 2), np.int64, order="F")

    def call(xp=P, xj=J, xv=None, n_rows=3, n_items=4, tb=TB, q=QF, K=2, cp=P, cj=J, nr_p=None, nr_j=None, ex=None, n_ex=0, k=2, res=res,
             sc=sc):
        return lib.rsparse_hip_knn_top_candidates(_vp(xp), _vp(xj), _vp(xv), n_rows, n_items, _vp(tb), _vp(q), K, _vp(cp), _vp(cj),
                                                  _vp(nr_p), _vp(nr_j), _vp(ex), n_ex, k, _vp(res), _vp(sc))

    for missing in ("xp", "tb", "q", "cp", "res", "sc"):
        _answer(call(**{missing: None}), _lib.ERR_INVALID, "NULL")
    host_row_refusals(call)
    _answer(call(k=0), _lib.ERR_INVALID, "K < 1 or k < 1")
    _answer(call(k=1025), _lib.ERR_UNSUPPORTED, "k > 1024")
    _answer(call(cj=None), _lib.ERR_INVALID, "cand_j is NULL")
    _answer(call(cp=np.array([1, 2, 3, 6], np.int32)), _lib.ERR_INVALID, "cand_p[0] != 0")
    _answer(call(cp=np.array([0, 3, 2, 6], np.int32)), _lib.ERR_INVALID, "cand_p decreases")
    _answer(call(cj=np.array([2, 0, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "not strictly ascending")      # an unsorted row
    _answer(call(cj=np.array([0, 0, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "not strictly ascending")      # a repeated column
    _answer(call(cj=np.array([0, 4, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "cand_j has a column outside [0, n_items)")
    _answer(call(cj=np.array([-1, 2, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "cand_j has a column outside [0, n_items)")
    zeros = np.zeros(1, np.int32)
    assert call(n_rows=0, xp=zeros, cp=zeros, ex=EX, n_ex=1) == _lib.OK       # no row: a no-op


def test_held_out_ranks_host_form_checks_its_arrays_first():
    lib = _lib.load()
    above, tied, n_adm = np.empty(6, np.int32), np.empty(6, np.int32), np.empty(3, np.int32)

    def call(xp=P, xj=J, xv=None, n_rows=3, n_items=4, tb=TB, q=QF, K=2, ap=P, aj=J, nr_p=None, nr_j=None, ex=None, n_ex=0, above=above,
             tied=tied, n_adm=n_adm):
        return lib.rsparse_hip_knn_held_out_ranks(_vp(xp), _vp(xj), _vp(xv), n_rows, n_items, _vp(tb), _vp(q), K, _vp(ap), _vp(aj),
                                                  _vp(nr_p), _vp(nr_j), _vp(ex), n_ex, _vp(above), _vp(tied), _vp(n_adm))

    for missing in ("xp", "tb", "q", "ap", "above", "tied", "n_adm"):
        _answer(call(**{missing: None}), _lib.ERR_INVALID, "NULL")
    host_row_refusals(call)
    _answer(call(aj=None), _lib.ERR_INVALID, "actual_j is NULL")
    _answer(call(ap=np.array([1, 2, 3, 6], np.int32)), _lib.ERR_INVALID, "actual_p[0] != 0")
    _answer(call(ap=np.array([0, 3, 2, 6], np.int32)), _lib.ERR_INVALID, "actual_p decreases")
    _answer(call(aj=np.array([2, 0, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "actual_j is not strictly ascending")
    zeros = np.zeros(1, np.int32)
    assert call(n_rows=0, xp=zeros, ap=zeros, ex=EX, n_ex=1) == _lib.OK       # no row: a no-op


@pytest.mark.parametrize("name", NAMES)
def test_signatures_match_the_header(name):
    """the number of arguments of every new entry in _lib.SIGNATURES is the header's"""
    import re
    from pathlib import Path
    text = (Path(__file__).resolve().parent.parent / "include" / "rsparse_wrmf_hip.h").read_text()
    decl = re.search(r"\bint %s\(([^;]*?)\);" % name, text).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1])
