"""WARP on the device (warp_search_kernel of wrmf_bpr.hip behind rsparse_hip_warp_*) against the numpy definition of
rsparse_amd/warp.py: the search alone, one step, a whole fit with its fold-in, and the host-array entry -- bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from rsparse_amd import WARP, _lib
from rsparse_amd.warp import rank_weights, warp_fit_reference, warp_step_reference, warp_triples
from test_bpr import DTYPES, TARGETS, TORCH, backend, bits_equal, dense12, planted, sparse300, upload
from test_ease_host import brute_lists, protocol

pytestmark = pytest.mark.gpu

# ---- the search alone --------------------------------------------------------------------------------------------------------------
# Every user has the same factor a (|a| = 1), so a user's score of an item is a per-item constant; the items of HANDFUL score 8
# above the rest, whose scores are noise of size 0.1.  With margin = -4 a candidate violates iff it is one of HANDFUL and the
# positive is not: about one trial in fifty, whatever the rank and the precision -- the searches are long and many exhaust T.
HANDFUL = [3, 77, 150, 211, 260, 299]
SEEDS = {(0, 0): 1, (0, 2 ** 31 - 80): 1, (1, 0): 9, (1, 2 ** 31 - 80): 8}   # chosen on the definition: the asserts on `ref` below


@pytest.mark.parametrize("precision", ["float", "double"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("row0", [0, 2 ** 31 - 80])
@pytest.mark.parametrize("T,rank", [(1, 1), (16, 16), (17, 17), (50, 128), (64, "max")])
def test_search_equals_the_definition(T, rank, row0, mode, precision):
    dtype = DTYPES[precision]
    if rank == "max":
        rank = _lib.MAX_RANK if precision == "float" else _lib.MAX_RANK_F64
    m, rng, seed = planted(), np.random.default_rng(rank), SEEDS[mode, row0]
    a = rng.standard_normal(rank)
    a /= np.sqrt((a * a).sum())
    V = 0.1 * rng.standard_normal((300, rank))
    V[HANDFUL] += 8.0 * a
    U, V, w = np.tile(a, (160, 1)).astype(dtype), V.astype(dtype), rank_weights(300, T)
    ref = warp_triples(seed, mode, 3, row0, m.indptr, m.indices, 300, U, V, T, -4.0, w)
    u, t, scored = ref[0], ref[3], ref[5]
    # conditions on the inputs: the round boundaries, exhausted searches, skipped in-row trials, the full row, and a wave whose
    # four groups stop in four different rounds
    assert {x for x in (1, 16, 17, 33, T) if x <= T} | {0} <= set(t.tolist())
    assert ((t > scored) & (t > 0)).any() or T == 1
    assert (t[u == 7] == 0).all() and (scored[u == 7] == 0).all() and (u == 7).sum() == 300 and (scored[u != 7] > 0).any()
    rounds = np.where(t > 0, (t - 1) // 16, 3)[:t.size // 4 * 4].reshape(-1, 4)
    assert (np.sort(rounds, axis=1) == np.arange(4)).all(axis=1).any() or T < 49
    be = backend()
    got = be.warp_triples(*upload(m), 300, m.nnz, row0, seed, mode, 3, 0, 1, T, -4.0, w, be.to_device(U, TORCH[dtype]),
                          be.to_device(V, TORCH[dtype]))
    assert all(g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), r) for g, r in zip(got[:4], ref[:4]))
    assert bits_equal(got[4].cpu().numpy(), ref[4]) and (ref[4][t > 0] > 0).all()


# ---- one step ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["float", "double"])
@pytest.mark.parametrize("update_items", [True, False])
@pytest.mark.parametrize("rank", [10, 16, 17, 64])
def test_one_step_equals_the_definition(rank, update_items, precision):
    dtype, be, rng = DTYPES[precision], backend(), np.random.default_rng(rank)
    for m, seed, step, n_steps in [(dense12(t), 21, 1, 2) for t in TARGETS] + [(sparse300(), 4, 0, 1)]:
        n_users, n_items = m.shape
        U, V = ((0.5 * rng.standard_normal((n, rank))).astype(dtype) for n in (n_users, n_items))
        aU, aV = rng.random(n_users) * 0.1, rng.random(n_items) * 0.1
        w = rank_weights(n_items, 4)
        ref = warp_step_reference(U, V, aU, aV, seed, 0, 0, 0, m.indptr, m.indices, 4, 0.1, w, 0.05, 0.02, update_items, step, n_steps)
        tk = warp_triples(seed, 0, 0, 0, m.indptr, m.indices, n_items, U, V, 4, 0.1, w, step, n_steps)[3]
        assert 0 < ref[4] < ref[5] and (tk > 1).any()                        # voids among the slots that looked; searches past trial 1
        dev = [be.to_device(x, tdt) for x, tdt in ((U, TORCH[dtype]), (V, TORCH[dtype]), (aU, torch.float64), (aV, torch.float64))]
        counts = be.warp_step(*upload(m), n_items, m.nnz, 0, seed, 0, 0, step, n_steps, 4, 0.1, w, *dev, 0.05, 0.02, update_items)
        got = [x.cpu().numpy() for x in dev]
        assert all(bits_equal(a, b) for a, b in zip(got, ref[:4])) and tuple(counts.cpu().tolist()) == ref[4:], (rank, m.shape)
        assert not bits_equal(got[0], U) and (update_items or bits_equal(got[1], V) and bits_equal(got[3], aV))


# ---- a fit -------------------------------------------------------------------------------------------------------------------------
ARGS = dict(rank=16, learning_rate=0.1, lambda_=0.01, batch=4096, max_trials=50, margin=0.1, transform_iter=50)


@functools.lru_cache(maxsize=None)
def fitted(precision):
    """the 900-user fixture, rank 16, 3 epochs, batch 4096, T = 50 -> (model, U, the definition from the device-drawn factors)"""
    train, _, _ = protocol()
    be, tdt = backend(), TORCH[DTYPES[precision]]
    m = WARP(precision=precision, rng=5, **ARGS)
    U = m.fit_transform(train, 3)
    U0, V0 = (be.init_factors(m.seed, s, n, 16, tdt).cpu().numpy() for s, n in ((0, train.shape[0]), (1, train.shape[1])))
    ref = warp_fit_reference(train.indptr, train.indices, train.shape[1], U0, V0, 3, m.seed, 50, 0.1, rank_weights(train.shape[1], 50),
                             0.1, 0.01, 4096)
    return m, U, ref


@pytest.mark.parametrize("precision", ["float", "double"])
def test_fit_equals_the_definition(precision):
    m, U, ref = fitted(precision)
    assert bits_equal(U, ref[0]) and bits_equal(m.components.T, ref[1]) and U.dtype == DTYPES[precision]
    assert bits_equal(m.user_adagrad, ref[2]) and bits_equal(m.item_adagrad, ref[3])
    assert m.trace == ref[4] and len(m.trace) == 3 and all(len(e) == 4 and e[0] <= e[1] <= e[3] for e in m.trace)
    assert m.trace[2][3] > m.trace[0][3] and bits_equal(m.rank_weights, rank_weights(protocol()[0].shape[1], 50))   # the searches grow longer
    again = WARP(precision=precision, rng=5, **ARGS)
    U2 = again.fit_transform(protocol()[0], 3)
    assert again.seed == m.seed and bits_equal(U2, U) and bits_equal(again.components, m.components) and again.trace == m.trace
    assert bits_equal(again.item_adagrad, m.item_adagrad)


def test_fold_in_and_lists_on_the_fitted_model():
    m, _, ref = fitted("double")
    _, hist, _ = protocol()
    V = ref[1]
    emb = m.transform(hist)
    fold = warp_fit_reference(hist.indptr, hist.indices, hist.shape[1], np.zeros((hist.shape[0], 16)), V, 50, m.seed, 50, 0.1,
                              m.rank_weights, 0.1, 0.01, 4096, mode=1, update_items=False, aV=ref[3])
    assert bits_equal(emb, fold[0]) and bits_equal(m.components.T, V)       # the fold-in is the definition; the items are frozen
    assert bits_equal(m.transform(hist[5:20]), emb[5:20]) and len(m.trace) == 3
    lists, _ = brute_lists(emb @ V.T, 10, hist, ())
    assert np.array_equal(np.asarray(m.predict(hist, 10)), lists)


# ---- the host-array entry ----------------------------------------------------------------------------------------------------------
def test_host_entry_is_the_device_route():
    import scipy.sparse as sp
    be, lib = backend(), _lib.load()
    x = sp.csr_matrix((np.random.default_rng(3).random((30, 14)) < 0.35).astype(np.float64))
    x.sort_indices()
    p, j, w = x.indptr.astype(np.int32), x.indices.astype(np.int32), rank_weights(14, 20)
    U, V, aU, aV, cnt = np.empty((30, 6)), np.empty((14, 6)), np.empty(30), np.empty(14), np.empty(16, np.int64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _lib.check(lib.rsparse_hip_warp_fit(vp(p), vp(j), 30, 14, 99, 4, 16, 20, 0.1, vp(w), 6, 0.1, 0.01, vp(U), vp(V), vp(aU), vp(aV), vp(cnt)))
    dU, dV = be.init_factors(99, 0, 30, 6, torch.float64), be.init_factors(99, 1, 14, 6, torch.float64)
    U0, V0 = dU.cpu().numpy(), dV.cpu().numpy()
    daU, daV = (torch.zeros(n, dtype=torch.float64, device=be.device) for n in (30, 14))
    counts = be.warp_epochs(be.to_device(p, torch.int32), be.to_device(j, torch.int32), 14, x.nnz, 0, 99, 0, 0, 4, 16, 20, 0.1, w, dU, dV,
                            daU, daV, 0.1, 0.01)
    for host, dev in ((U, dU), (V, dV), (aU, daU), (aV, daV), (cnt, counts.reshape(-1))):
        assert bits_equal(host, dev.cpu().numpy())
    ref = warp_fit_reference(p, j, 14, U0, V0, 4, 99, 20, 0.1, w, 0.1, 0.01, 16)
    assert bits_equal(U, ref[0]) and bits_equal(V, ref[1]) and [tuple(r) for r in cnt.reshape(4, 4).tolist()] == ref[4]
