"""BPR / WARP through item features (rsparse_amd/bpr.py, warp.py): with identity features the numpy definition is the plain one bit
for bit, and what the new C entries refuse before a device is touched."""
import numpy as np
import pytest
import scipy.sparse as sp

from rsparse_amd import _lib
from rsparse_amd import rng as prng
from rsparse_amd.bpr import bpr_feat_fit_reference, bpr_fit_reference
from rsparse_amd.warp import rank_weights, warp_feat_fit_reference, warp_fit_reference
from test_bpr import bits_equal
from test_bpr_host import J, P, _answer, _vp


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("loss", ["bpr", "warp"])
def test_identity_features_are_the_plain_fit(loss, dtype):
    x = sp.csr_matrix(np.random.default_rng(3).random((60, 40)) < 0.15)
    x.sort_indices()
    U0, V0 = (prng.init_factors(11, s, 0, n, 20, 0.01, dtype=dtype) for s, n in ((prng.STREAM_USERS, 60), (prng.STREAM_ITEMS, 40)))
    F = sp.identity(40, dtype=dtype, format="csr")
    if loss == "bpr":
        ref = bpr_fit_reference(x.indptr, x.indices, 40, U0, V0, 2, 11, 0.1, 0.01, 64)
        got = bpr_feat_fit_reference(x.indptr, x.indices, F, U0, V0, 2, 11, 0.1, 0.01, 64)
    else:
        w = rank_weights(40, 10)
        ref = warp_fit_reference(x.indptr, x.indices, 40, U0, V0, 2, 11, 10, 0.1, w, 0.1, 0.01, 64)
        got = warp_feat_fit_reference(x.indptr, x.indices, F, U0, V0, 2, 11, 10, 0.1, w, 0.1, 0.01, 64)
    assert all(bits_equal(a, b) for a, b in zip(got[:4], ref[:4])) and got[4] == ref[4] and got[4][0][0] > 0
    assert not bits_equal(got[1], V0) and -(-x.nnz // 64) > 2          # the features moved, over several steps per epoch


# F = the 4 x 4 identity by item and by feature (host pointers: every call below is refused before device work)
FP, FJ, FX = np.arange(5, dtype=np.int32), np.arange(4, dtype=np.int32), np.ones(4)


def _calls(fp=FP, cx=FX, H=np.zeros((4, 2)), aH=np.zeros(4), n_feat=4, nnz_f=4, rank=2, mode=0, max_trials=2, f64=True):
    lib, sfx = _lib.load(), "_f64" if f64 else ""
    U, V, a, cnt = np.zeros((3, 2)), np.zeros((4, 2)), np.zeros(4), np.zeros(8, np.int64)
    head = (_vp(P), _vp(J), 3, 4, 6, 0, 1, mode, 0)
    tail = (_vp(fp), _vp(FJ), _vp(FX), _vp(FP), _vp(FJ), _vp(cx), n_feat, nnz_f, _vp(U), _vp(H), _vp(V), _vp(a), _vp(aH), _vp(cnt), None)
    for name, bc in (("step", (0, 1)), ("epochs", (1, 16))):
        yield getattr(lib, "rsparse_hip_bpr_feat_%s%s_device" % (name, sfx))(*head, *bc, rank, 0.1, 0.01, 1, *tail)
        yield getattr(lib, "rsparse_hip_warp_feat_%s%s_device" % (name, sfx))(*head, *bc, max_trials, 0.1, _vp(np.ones(2)), rank, 0.1, 0.01,
                                                                              1, *tail)
    if mode == 0 and max_trials == 2 and aH is not None and cx is not None:      # (what the compose entry takes of these)
        yield getattr(lib, "rsparse_hip_compose_rows%s_device" % sfx)(_vp(fp), _vp(FJ), _vp(FX), 4, n_feat, nnz_f, rank, _vp(H), _vp(V), None)


@pytest.mark.parametrize("kw,code,text", [
    (dict(fp=None), _lib.ERR_INVALID, "NULL"), (dict(cx=None), _lib.ERR_INVALID, "feature array"),
    (dict(H=None), _lib.ERR_INVALID, "NULL"), (dict(aH=None), _lib.ERR_INVALID, "feature array"),
    (dict(n_feat=0), _lib.ERR_INVALID, "n_feat < 1"), (dict(nnz_f=-1), _lib.ERR_INVALID, "nnz_f"),
    (dict(rank=0), _lib.ERR_INVALID, "rank < 1"), (dict(mode=2), _lib.ERR_INVALID, "mode"),
    (dict(rank=_lib.MAX_RANK_F64 + 1), _lib.ERR_UNSUPPORTED, "rank > 128"),
    (dict(rank=_lib.MAX_RANK + 1, f64=False), _lib.ERR_UNSUPPORTED, "rank > 256")])
def test_feature_entries_refuse_before_a_device(kw, code, text):
    n = 0
    for n, rc in enumerate(_calls(**kw), 1):
        _answer(rc, code, text)
    assert n >= 4
    import rsparse_amd
    assert rsparse_amd.bpr_feat_fit_reference is bpr_feat_fit_reference and rsparse_amd.warp_feat_fit_reference is warp_feat_fit_reference
