"""SLIM without a device: the numpy definition of rsparse_amd/slim.py against the optimality conditions of the problem it states and
against cases worked by hand, the class on the CPU stand-in backend, the refusals of the C ABI before any device work, and the ABI
table."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from rsparse_amd import SLIM, _lib
from rsparse_amd.ease import (ease_gram_reference, ease_ranks_reference, ease_recommend_reference, ease_score_pairs_reference,
                              ease_candidates_reference)
from rsparse_amd.metrics import rank_summary, rank_totals
from rsparse_amd.slim import slim_columns_reference, slim_weights_reference
from test_ease_host import brute_lists, ndcg10, protocol
from test_metrics_abi import _oracle_metrics_backend

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("rsparse_hip_slim_columns_device", "rsparse_hip_slim_fit")


def supports(G, j):
    S = np.flatnonzero(G[j] > 0)
    return S[S != j]


# ---- the definition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l1,l2", [(0.5, 1.0), (0.0, 0.5), (2.0, 0.0)])
@pytest.mark.parametrize("n_users,n_items,density", [(60, 40, 0.5), (300, 120, 0.1), (200, 64, 0.3)])
def test_fixed_point_meets_the_optimality_conditions(n_users, n_items, density, l1, l2):
    """At tol = 1e-14 the sweeps end at a point that satisfies, on S_j, c_ij - (G w)_i - l2 w_i = l1 where w_i > 0 and <= l1 where
    w_i = 0, to 1e-9 (the prototype of the definition measured at most 1.5e-12 on these sizes; the margin covers other seeds)."""
    x = sp.csr_matrix((np.random.default_rng(n_items).random((n_users, n_items)) < density).astype(np.float64))
    G = ease_gram_reference(x, 0.0)
    W, sweeps = slim_weights_reference(x, l1, l2, 20000, 1e-14)
    assert W.dtype == np.float64 and W.shape == (n_items, n_items) and sweeps.dtype == np.int32 and sweeps.max() < 20000
    assert (W >= 0).all() and not np.signbit(W).any() and (np.diag(W) == 0).all()
    worst = 0.0
    for j in range(n_items):
        S = supports(G, j)
        outside = np.setdiff1d(np.arange(n_items), S)
        assert (W[outside, j] == 0).all()
        g = G[j, S] - G[S] @ W[:, j] - l2 * W[S, j]
        pos = W[S, j] > 0
        worst = max(worst, np.abs(g[pos] - l1).max(initial=0.0), (g[~pos] - l1).max(initial=0.0))
    print("%d x %d, l1 %g, l2 %g: optimality to %.3g, at most %d sweeps" % (n_users, n_items, l1, l2, worst, sweeps.max()))
    assert worst <= 1e-9


# 4 users x 3 items: rows {0, 1}, {0, 1, 2}, {0, 2}, {1}: n = (3, 3, 2), c_01 = 2, c_02 = 2, c_12 = 1
TINY = sp.csr_matrix(np.array([[1, 1, 0], [1, 1, 1], [1, 0, 1], [0, 1, 0]], dtype=np.float64))


def test_one_column_worked_by_hand():
    """Column 0 at l1 = 0.5, l2 = 1: S = (1, 2), c = (2, 2), d = (3, 2), den = (4, 3); every number below is a binary fraction.
    Sweep 1: u = 2 - 0.5 = 1.5, w_1 = 0.375, r = 0.375 (3, 1) = (1.125, 0.375); u = (2 - 0.375) - 0.5 = 1.125, w_2 = 0.375,
    r = (1.125, 0.375) + 0.375 (1, 2) = (1.5, 1.125).  Sweep 2: u = (2 - (1.5 - 3 * 0.375)) - 0.5 = 1.125, w_1 = 0.28125, delta =
    -0.09375, r = (1.21875, 1.03125); u = (2 - (1.03125 - 2 * 0.375)) - 0.5 = 1.21875, w_2 = 0.40625."""
    G = ease_gram_reference(TINY, 0.0)
    assert np.array_equal(G, [[3, 2, 2], [2, 3, 1], [2, 1, 2]])
    W, sweeps = slim_columns_reference(G, [0], 0.5, 1.0, 1, 0.0)
    assert np.array_equal(W[:, 0], [0.0, 0.375, 0.375]) and sweeps.tolist() == [1] and (W[:, 1:] == 0).all()
    W, sweeps = slim_columns_reference(G, [0], 0.5, 1.0, 2, 0.0)
    assert np.array_equal(W[:, 0], [0.0, 0.28125, 0.40625]) and sweeps.tolist() == [2]
    # dmax of the second sweep is 0.09375 and wmax 0.40625: tol = 0.25 stops there, tol = 0.2 does not
    assert slim_columns_reference(G, [0], 0.5, 1.0, 9, 0.25)[1].tolist() == [2]
    assert slim_columns_reference(G, [0], 0.5, 1.0, 9, 0.2)[1].tolist() == [3]
    # float: the double weights rounded once
    W32, _ = slim_columns_reference(G, [0, 1, 2], 0.3, 0.7, 5, 0.0, np.float32)
    W64, _ = slim_columns_reference(G, [2, 0, 1, 0], 0.3, 0.7, 5, 0.0)
    assert W32.dtype == np.float32 and np.array_equal(W32, W64.astype(np.float32))


def test_a_penalty_at_the_largest_count_leaves_nothing():
    G = ease_gram_reference(TINY, 0.0)
    W, sweeps = slim_columns_reference(G, [0, 1, 2], 2.0, 1.0, 50, 1e-4)     # l1 = max c_ij
    assert (W == 0).all() and not np.signbit(W).any() and sweeps.tolist() == [1, 1, 1]
    W, _ = slim_columns_reference(G, [0, 1, 2], 1.999, 1.0, 50, 1e-4)
    assert (W > 0).any()


def test_sweep_counts():
    rng = np.random.default_rng(4)
    d = rng.random((50, 12)) < 0.3
    d[:, 3] = False                                                           # an item without users
    d[:, 7] = False
    d[-1] = False
    d[-1, 7] = True                                                           # an item that co-occurs with nothing
    x = sp.csr_matrix(d.astype(np.float64))
    G = ease_gram_reference(x, 0.0)
    full, n_full = slim_weights_reference(x, 0.2, 1.0, 100, 1e-6)
    assert n_full[3] == 0 and n_full[7] == 0 and (full[:, [3, 7]] == 0).all() and (full[[3, 7]] == 0).all()
    assert (np.delete(n_full, [3, 7]) >= 2).all() and n_full.max() < 100
    one, n_one = slim_weights_reference(x, 0.2, 1.0, 1, 1e-6)
    two, n_two = slim_weights_reference(x, 0.2, 1.0, 2, 1e-6)
    live = np.delete(np.arange(12), [3, 7])
    assert (n_one[live] == 1).all() and (n_two[live] == 2).all() and n_one[3] == n_two[7] == 0
    # the first sweep of a column starts from r = 0 up to the updates in front of a coordinate: its first coordinate is the closed form
    for j in live:
        i = supports(G, j)[0]
        assert one[i, j] == max((G[j, i] - 0.0) - 0.2, 0.0) / (G[i, i] + 1.0)
    assert not np.array_equal(one, two) and not np.array_equal(two, full)
    # tol = 0 runs to the cap or to an exact fixed point
    _, n_zero = slim_columns_reference(G, live, 0.2, 1.0, 7, 0.0)
    assert (n_zero == 7).all()
    for bad in ({"l1": -1.0}, {"l2": np.nan}, {"tol": np.inf}, {"max_iter": 0}, {"max_iter": 2.0}, {"max_iter": True}):
        kw = {"l1": 0.1, "l2": 0.1, "max_iter": 3, "tol": 0.1, **bad}
        with pytest.raises(ValueError):
            slim_columns_reference(G, [0], **kw)
    with pytest.raises(ValueError):
        slim_columns_reference(G, [12], 0.1, 0.1, 3, 0.1)


# ---- the class on the CPU stand-in -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model():
    rng = np.random.default_rng(11)
    b = (rng.random((40, 30)) < 0.25).astype(np.float64)
    b[0] = 0
    x = sp.csr_matrix(b)
    held = sp.csr_matrix((rng.random(b.shape) < 0.2) * (1 - b) * 2.0)
    return x, held, SLIM(0.2, 1.0, max_iter=50, tol=1e-6, precision="double", backend=_oracle_metrics_backend()).fit(x)


def test_class_fit_is_the_definition(small_model):
    x, _, m = small_model
    W, sweeps = slim_weights_reference(x, 0.2, 1.0, 50, 1e-6)
    assert np.array_equal(m.W, W) and np.array_equal(m.B, W) and m.W.dtype == np.float64
    assert np.array_equal(m.n_sweeps, sweeps) and m.n_sweeps.dtype == np.int32
    assert np.array_equal(m.item_count, np.asarray(x.sum(axis=0)).ravel())
    f = SLIM(0.2, 1.0, max_iter=50, tol=1e-6, backend=_oracle_metrics_backend()).fit(x)
    assert f.W.dtype == np.float32 and np.array_equal(f.W, W.astype(np.float32)) and np.array_equal(f.n_sweeps, sweeps)


def test_class_inference_is_ease_on_the_weights(small_model):
    x, held, m = small_model
    W = m.W
    top = m.predict(x, 5, items_exclude=(3,))
    ref = ease_recommend_reference(x, W, 5, x, (3,))
    assert np.array_equal(np.asarray(top), ref[0]) and np.array_equal(top.scores, np.where(ref[0] < 0, np.nan, ref[1]), equal_nan=True)
    cand = sp.csr_matrix(np.random.default_rng(5).random(x.shape) < 0.3)
    top = m.predict(x, 4, candidates=cand)
    ref = ease_candidates_reference(x, W, cand, 4, x, ())
    assert np.array_equal(np.asarray(top), ref[0])
    metrics = ("ap", "ndcg", "hit", "mrr")
    sampled = m.sample_negatives(x, 99, actual=held, seed=7)
    a = m.evaluate(x, held, (3, 5), metrics=metrics, negatives=99, seed=7)
    c = m.evaluate(x, held, (3, 5), metrics=metrics, candidates=sampled)
    from test_metrics_abi import ref_metrics, to_r
    lists = ease_candidates_reference(x, W, sampled, 5, x, ())[0]
    for t, cut in enumerate((3, 5)):
        ap, ndcg = ref_metrics(to_r(lists[:, :cut]), held)
        assert np.array_equal(a["ap"][:, t], ap, equal_nan=True) and np.array_equal(a["ndcg"][:, t], ndcg, equal_nan=True)
    for name in metrics:
        assert np.array_equal(a[name], c[name], equal_nan=True), name
    pairs = sp.csr_matrix(np.random.default_rng(6).random(x.shape) < 0.1)
    assert np.array_equal(m.score(x, pairs).data, ease_score_pairs_reference(x, W, pairs))
    ref = ease_ranks_reference(x, W, held, x, (1,))
    above, tied, n_adm = m.held_out_ranks(x, held, items_exclude=(1,))
    assert np.array_equal(above.data, ref[0]) and np.array_equal(tied.data, ref[1]) and np.array_equal(n_adm, ref[2])
    ev = m.evaluate_ranks(x, held, items_exclude=(1,))
    tot = rank_totals(rank_summary(above, tied, n_adm, held))
    assert ev["n"] == tot["n"] and all(np.isclose(ev[name], tot[name], rtol=1e-13, atol=0) for name in ("mpr", "auc", "mrr"))
    sim = m.similar_items([2, 5], k=3)
    assert np.array_equal(sim.scores[0], W[2][np.asarray(sim)[0]])


def test_class_beats_popularity_on_the_fixture():
    """l1 = 1, l2 = 500 on the MovieLens split of tests/test_ease_host.py, three sweeps of the numpy definition (the full fit
    runs on the device: tests/test_slim.py records its number)."""
    train, hist, held = protocol()
    m = SLIM(1.0, 500.0, max_iter=3, precision="double", backend=_oracle_metrics_backend()).fit(train)
    assert (m.n_sweeps <= 3).all() and (m.W >= 0).all() and (np.diag(m.W) == 0).all()
    top = m.predict(hist, 10)
    ref = ease_recommend_reference(hist, m.W, 10, hist)
    assert np.array_equal(np.asarray(top), ref[0]) and np.array_equal(top.scores, ref[1])
    pop_lists, _ = brute_lists(np.broadcast_to(m.item_count.astype(np.float64), hist.shape), 10, hist, ())
    slim, popularity = ndcg10(np.asarray(top), held), ndcg10(pop_lists, held)
    print("NDCG@10: SLIM(l1 = 1, l2 = 500, three sweeps) %.3f, popularity %.3f; %.0f non-zeros per column"
          % (slim, popularity, (m.W > 0).sum() / m.W.shape[0]))
    assert slim > popularity


def test_constructor_refusals(monkeypatch):
    for kw in ({"l1": -1.0}, {"l1": np.nan}, {"l2": -0.5}, {"l2": np.inf}, {"tol": -1e-3}, {"tol": np.nan}, {"max_iter": 0},
               {"max_iter": 1.5}, {"max_iter": True}, {"precision": "half"}):
        with pytest.raises(ValueError):
            SLIM(**kw)
    m = SLIM(backend=_oracle_metrics_backend())
    assert (m._l1, m._l2, m._max_iter, m._tol, m._dtype) == (1.0, 50.0, 100, 1e-4, np.float32)
    x = sp.csr_matrix(np.eye(4))
    with pytest.raises(RuntimeError):
        m.predict(x, 2)
    with pytest.raises(RuntimeError):
        m.W
    with pytest.raises(_lib.UnsupportedOnDevice):
        m.fit(sp.csr_matrix((1, _lib.EASE_MAX_ITEMS + 1)))
    fitted = m.fit(x)                                                         # no co-occurrence at all
    assert (fitted.W == 0).all() and (fitted.n_sweeps == 0).all()
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda: 2)
    with pytest.raises(_lib.UnsupportedOnDevice):
        SLIM(backend=_oracle_metrics_backend()).fit(x)


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------
def test_library_exports_the_slim_entry_points():
    lib = _lib.load()
    text = (ROOT / "include" / "rsparse_wrmf_hip.h").read_text()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert lib.rsparse_hip_abi_version() == 6                                # additive entries: the version stays
    from rsparse_amd.engine import HipBackend
    assert callable(HipBackend.slim_columns)
    import rsparse_amd
    assert rsparse_amd.SLIM is SLIM and rsparse_amd.slim_columns_reference is slim_columns_reference


def test_constants_mirror_the_header():
    text = (ROOT / "include" / "rsparse_wrmf_hip.h").read_text()
    cap = int(re.search(r"#define RSPARSE_HIP_SLIM_LDS_SUPPORT (\d+)", text).group(1))
    assert cap == _lib.SLIM_LDS_SUPPORT and cap % 64 == 0
    assert 2 * (cap * 36 + 1024) <= 160 * 1024                               # two workgroups of the LDS form in a CU's LDS


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _answer(rc, code, text):
    assert rc == code, (rc, _lib.load().rsparse_hip_last_error())
    assert text in _lib.load().rsparse_hip_last_error().decode(), _lib.load().rsparse_hip_last_error()


def test_slim_columns_device_status_codes():
    # (host pointers: every call here is rejected by the argument checks, or has no column, before device work)
    fn = _lib.load().rsparse_hip_slim_columns_device
    G = np.zeros((4, 4))
    raw = np.zeros(4 * 4 + 8, np.float32)
    W = raw[(-raw.ctypes.data // 4) % 4:][:16]                               # 16-byte aligned
    cols, sweeps = np.arange(4, dtype=np.int32), np.zeros(4, np.int32)

    def call(G=G, ld_G=4, n_items=4, cols=cols, n_cols=4, l1=1.0, l2=1.0, max_iter=3, tol=1e-4, W=W, ld_W=4, f64=0, sweeps=sweeps):
        return fn(_vp(G), ld_G, n_items, _vp(cols), n_cols, l1, l2, max_iter, tol, _vp(W), ld_W, f64, _vp(sweeps), None)

    for missing in ("G", "cols", "W", "sweeps"):
        _answer(call(**{missing: None}), _lib.ERR_INVALID, "NULL")
    _answer(call(n_items=-1), _lib.ERR_INVALID, "bad dimensions")
    _answer(call(n_cols=-1), _lib.ERR_INVALID, "bad dimensions")
    for bad in (-0.5, float("nan"), float("inf")):
        _answer(call(l1=bad), _lib.ERR_INVALID, "l1 or l2 is negative or not finite")
        _answer(call(l2=bad), _lib.ERR_INVALID, "l1 or l2 is negative or not finite")
        _answer(call(tol=bad), _lib.ERR_INVALID, "tol is negative or not finite")
    _answer(call(max_iter=0), _lib.ERR_INVALID, "max_iter < 1")
    _answer(call(ld_G=3), _lib.ERR_INVALID, "ld_G < n_items")
    _answer(call(ld_W=3), _lib.ERR_INVALID, "ld_W < n_items")
    _answer(call(ld_W=6), _lib.ERR_INVALID, "multiple of 16 bytes")
    _answer(call(ld_W=5, f64=1), _lib.ERR_INVALID, "multiple of 16 bytes")
    _answer(call(W=W[1:]), _lib.ERR_INVALID, "multiple of 16 bytes")
    big = _lib.EASE_MAX_ITEMS + 1
    _answer(call(n_items=big, ld_G=big, ld_W=big + 3), _lib.ERR_UNSUPPORTED, "n_items > 32768")
    assert call(n_items=big, ld_G=big, ld_W=big + 3, W=None) == _lib.ERR_INVALID   # the pointers are looked at first
    _answer(call(n_cols=0), _lib.OK, "")                                     # no column: a no-op
    _answer(call(n_cols=0, ld_W=6, f64=1), _lib.OK, "")                      # (6 doubles are 48 bytes)
    _answer(call(n_items=0, ld_G=0, ld_W=0), _lib.ERR_INVALID, "a column outside [0, n_items)")


# 3 users x 4 items: rows {0, 2}, {1}, {0, 1, 3}
P = np.array([0, 2, 3, 6], dtype=np.int32)
J = np.array([0, 2, 1, 0, 1, 3], dtype=np.int32)


def test_slim_fit_checks_its_arrays_first():
    lib = _lib.load()
    W, sweeps = np.empty((4, 4), order="F"), np.empty(4, np.int32)

    def fit(p=P, j=J, n_users=3, n_items=4, l1=1.0, l2=1.0, max_iter=3, tol=1e-4, W=W, sweeps=sweeps):
        return lib.rsparse_hip_slim_fit(_vp(p), _vp(j), n_users, n_items, l1, l2, max_iter, tol, _vp(W), _vp(sweeps))

    for missing in ("p", "W", "sweeps"):
        _answer(fit(**{missing: None}), _lib.ERR_INVALID, "NULL")
    _answer(fit(j=None), _lib.ERR_INVALID, "j is NULL")
    _answer(fit(n_users=-1), _lib.ERR_INVALID, "bad dimensions")
    _answer(fit(n_items=-1), _lib.ERR_INVALID, "bad dimensions")
    _answer(fit(l1=-1.0), _lib.ERR_INVALID, "l1 or l2 is negative or not finite")
    _answer(fit(l2=float("nan")), _lib.ERR_INVALID, "l1 or l2 is negative or not finite")
    _answer(fit(tol=float("inf")), _lib.ERR_INVALID, "tol is negative or not finite")
    _answer(fit(max_iter=0), _lib.ERR_INVALID, "max_iter < 1")
    _answer(fit(n_items=_lib.EASE_MAX_ITEMS + 1), _lib.ERR_UNSUPPORTED, "n_items > 32768")
    _answer(fit(p=np.array([1, 2, 3, 6], np.int32)), _lib.ERR_INVALID, "p[0] != 0")
    _answer(fit(p=np.array([0, 3, 2, 6], np.int32)), _lib.ERR_INVALID, "p decreases")
    _answer(fit(j=np.array([0, 4, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "a column outside [0, n_items)")
    _answer(fit(j=np.array([2, 0, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "not strictly ascending")
    assert fit(n_items=0, p=np.zeros(4, np.int32)) == _lib.OK               # no item: a no-op
