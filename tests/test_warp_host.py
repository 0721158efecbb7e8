"""WARP's numpy definition (rsparse_amd/warp.py) against BPR's at the ends of the margin, and what the C entries refuse before a
device is touched."""
import math

import numpy as np
import pytest

from rsparse_amd import WARP, _lib
from rsparse_amd import rng as prng
from rsparse_amd.bpr import bpr_step_reference
from rsparse_amd.warp import rank_weights, warp_step_reference, warp_triples
from test_bpr import bits_equal, dense12, planted, sparse300
from test_bpr_host import J, P, _answer, _vp

CASES = [(dense12(65), 21, 1, 2), (sparse300(), 4, 0, 1)]


def random_factors(m, rank, dtype, seed=1):
    rng = np.random.default_rng(seed)
    U, V = ((0.5 * rng.standard_normal((n, rank))).astype(dtype) for n in m.shape)
    return U, V, rng.random(m.shape[0]) * 0.1, rng.random(m.shape[1]) * 0.1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("update_items", [True, False])
def test_an_infinite_margin_is_bpr_on_the_first_admissible_trial(update_items, dtype):
    for m, seed, step, n_steps in CASES:
        U, V, aU, aV = random_factors(m, 17, dtype)
        u, i, j, t, z, scored, counts = warp_triples(seed, 0, 2, 0, m.indptr, m.indices, m.shape[1], U, V, 50, np.inf, np.ones(50), step, n_steps)
        assert ((scored == 1) == (j >= 0)).all() and (t[j >= 0] >= scored[j >= 0]).all() and (j < 0).any()
        assert (t > 1).any() or m.shape[1] == 300                               # (in-row candidates were skipped on the way)
        ref = bpr_step_reference(U, V, aU, aV, u, i, j, 0.05, 0.02, update_items)
        got = warp_step_reference(U, V, aU, aV, seed, 0, 2, 0, m.indptr, m.indices, 50, np.inf, np.ones(50), 0.05, 0.02, update_items, step, n_steps)
        assert all(bits_equal(a, b) for a, b in zip(got[:4], ref[:4])) and not bits_equal(got[0], U)
        assert got[4:] == (ref[4], ref[4], ref[5], ref[4]) == (int((j >= 0).sum()),) + counts


def test_a_margin_of_minus_infinity_moves_nothing():
    m, seed, step, n_steps = CASES[0]
    U, V, aU, aV = random_factors(m, 8, np.float64)
    got = warp_step_reference(U, V, aU, aV, seed, 0, 0, 0, m.indptr, m.indices, 64, -np.inf, rank_weights(12, 64), 0.05, 0.02, True, step, n_steps)
    assert all(bits_equal(a, b) for a, b in zip(got[:4], (U, V, aU, aV)))
    assert got[4] == 0 and 0 < got[5] < got[7] and got[7] > 30 * got[5]     # every slot scored all its admissible trials


def test_a_row_holding_every_item_is_void_and_scores_nothing():
    m = planted()
    U, V, _, _ = random_factors(m, 4, np.float32)
    u, i, j, t, z, scored, _ = warp_triples(5, 0, 0, 0, m.indptr, m.indices, 300, U, V, 64, 0.1, rank_weights(300, 64))
    full = u == 7
    assert full.sum() == 300 and (j[full] == -1).all() and (t[full] == 0).all() and (z[full] == 0).all() and (scored[full] == 0).all()
    assert (scored[u == 6] <= 64).all() and (t[j >= 0] >= 1).all() and (z[j >= 0] > 0).all()
    assert (m[u[j >= 0], j[j >= 0]] == 0).all() and (m[u, i] == 1).all()


def test_rank_weights_and_arguments():
    w = rank_weights(1682, 50)
    assert w[0] == math.log(2 + 1681.0) / math.log(2 + 1682.0) and (np.diff(w) < 0).all() and w[-1] > 0 and prng.STREAM_WARP == 7
    for bad in (dict(max_trials=0), dict(max_trials=65), dict(max_trials=2.0), dict(margin=np.inf), dict(margin=np.nan), dict(rank=0)):
        with pytest.raises(ValueError):
            WARP(**bad)
    import rsparse_amd
    assert rsparse_amd.WARP is WARP and rsparse_amd.warp_triples is warp_triples and issubclass(WARP, rsparse_amd.BPR)


def test_warp_entries_refuse_a_bad_search_before_a_device():
    lib = _lib.load()
    U, V, a, cnt, out = np.zeros((3, 2)), np.zeros((4, 2)), np.zeros(4), np.zeros(8, np.int64), np.zeros(6, np.int32)

    def calls(max_trials=2, margin=0.1, weights=np.ones(2), rank=2):
        head = (_vp(P), _vp(J), 3, 4, 6, 0, 1, 0, 0)
        search = (max_trials, margin, _vp(weights), rank)
        yield lib.rsparse_hip_warp_triples_f64_device(*head, 0, 1, *search, _vp(U), _vp(V), *(_vp(out),) * 4, _vp(a), None)
        yield lib.rsparse_hip_warp_step_f64_device(*head, 0, 1, *search, 0.1, 0.01, 1, _vp(U), _vp(V), _vp(a), _vp(a), _vp(cnt), None)
        yield lib.rsparse_hip_warp_epochs_f64_device(*head, 1, 16, *search, 0.1, 0.01, 1, _vp(U), _vp(V), _vp(a), _vp(a), _vp(cnt), None)
        yield lib.rsparse_hip_warp_fit(_vp(P), _vp(J), 3, 4, 1, 1, 16, *search, 0.1, 0.01, _vp(U), _vp(V), _vp(a), _vp(a), _vp(cnt))

    for kw, text in ((dict(max_trials=0), "max_trials"), (dict(max_trials=65, weights=np.ones(65)), "max_trials"),
                     (dict(margin=np.inf), "margin"), (dict(margin=np.nan), "margin"), (dict(weights=None), "weights is NULL"),
                     (dict(weights=np.array([1.0, -0.5])), "weights entry"), (dict(weights=np.array([np.nan, 1.0])), "weights entry"),
                     (dict(weights=np.array([1.0, np.inf])), "weights entry"), (dict(rank=0), "rank < 1")):
        for rc in calls(**kw):
            _answer(rc, _lib.ERR_INVALID, text)
