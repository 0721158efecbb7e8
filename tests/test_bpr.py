"""BPR on the device (wrmf_bpr.hip behind rsparse_hip_bpr_*_device / rsparse_hip_bpr_fit) against the numpy definition of
rsparse_amd/bpr.py: the triples, one step's factors and Adagrad states, a whole fit and the fold-in, bit for bit in both
precisions; the inference surface on the fitted model."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import BPR, _lib
from rsparse_amd.bpr import CHUNK, bpr_fit_reference, bpr_step_reference, bpr_triples
from test_ease_host import brute_lists, ndcg10, protocol
from test_metrics_abi import _oracle_metrics_backend

pytestmark = pytest.mark.gpu

DTYPES = {"float": np.float32, "double": np.float64}
TORCH = {np.float32: torch.float32, np.float64: torch.float64}


@functools.lru_cache(maxsize=None)
def backend():
    from rsparse_amd.engine import HipBackend
    return HipBackend()


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def upload(m):
    be = backend()
    return be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32)


def device_step(m, U, V, aU, aV, seed, mode, epoch, step, n_steps, lr, lam, update_items, row0=0):
    """-> (U', V', aU', aV', n_valid, n_correct) as numpy: the layout of bpr_step_reference"""
    be = backend()
    p, j = upload(m)
    dU, dV = be.to_device(U, TORCH[U.dtype.type]), be.to_device(V, TORCH[V.dtype.type])
    daU, daV = be.to_device(aU, torch.float64), be.to_device(aV, torch.float64)
    cnt = be.bpr_step(p, j, m.shape[1], m.nnz, row0, seed, mode, epoch, step, n_steps, dU, dV, daU, daV, lr, lam, update_items)
    cnt = cnt.cpu().numpy()
    return dU.cpu().numpy(), dV.cpu().numpy(), daU.cpu().numpy(), daV.cpu().numpy(), int(cnt[0]), int(cnt[1])


def same_step(got, ref):
    return all(bits_equal(a, b) for a, b in zip(got[:4], ref[:4])) and tuple(got[4:]) == tuple(ref[4:])


# ---- the triples -------------------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 63, 64, 65, 257, 299, 300)


@functools.lru_cache(maxsize=None)
def planted():
    """160 users x 300 items of rising popularity; users 0 .. 7 hold 0, 1, 63, 64, 65, 257, 299 and 300 items"""
    rng = np.random.default_rng(7)
    d = rng.random((160, 300)) < np.linspace(0.02, 0.25, 300)[None, :]
    d[:len(LENGTHS)] = False
    for u, length in enumerate(LENGTHS):
        d[u, rng.choice(300, size=length, replace=False)] = True
    assert d[:len(LENGTHS)].sum(axis=1).tolist() == list(LENGTHS)
    return sp.csr_matrix(d.astype(np.float64))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("row0", [0, 2 ** 31 - 80])
@pytest.mark.parametrize("n_steps", [1, 3, 7])
def test_triples_equal_the_definition(n_steps, row0, mode):
    m = planted()
    p, j = upload(m)
    voids = 0
    for step in range(n_steps):
        ref = bpr_triples(12345678901234567, mode, 3, row0, m.indptr, m.indices, 300, step, n_steps)
        got = backend().bpr_triples(p, j, 300, m.nnz, row0, 12345678901234567, mode, 3, step, n_steps)
        assert all(g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), r) for g, r in zip(got, ref))
        voids += int((ref[2] < 0).sum())
    assert voids >= 300                                                      # (the full row, at least)


# ---- one step ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense12(target, seed=21, n_steps=2, step=1):
    """40 users x 12 items, item 0 in every row, one user holding every item (all void); then users holding item 0 alone -- each
    gives item 0 one positive contribution in the step its slot falls in -- until item 0 has exactly `target` contributions
    in step `step`.  With 12 items the negatives collide: the other items receive both roles."""
    rng = np.random.default_rng(5)
    d = rng.random((40, 12)) < 0.4
    d[:, 0] = True
    d[7] = True
    rows = [np.flatnonzero(r) for r in d]

    def build():
        return sp.csr_matrix((np.ones(sum(r.size for r in rows)), np.concatenate(rows), np.concatenate([[0], np.cumsum([r.size for r in rows])])),
                             shape=(len(rows), 12))

    def count(m):
        _, i, j = bpr_triples(seed, 0, 0, 0, m.indptr, m.indices, 12, step, n_steps)
        return int(((i == 0) & (j >= 0)).sum())

    m = build()
    assert count(m) < target
    while count(m) < target:
        rows.append(np.array([0]))
        m = build()
    assert count(m) == target
    t = bpr_triples(seed, 0, 0, 0, m.indptr, m.indices, 12, step, n_steps)
    u = t[0]
    both = np.intersect1d(t[1][t[2] >= 0], t[2][t[2] >= 0])
    assert both.size >= 5                                                    # items that are positives and negatives in this step
    lens = np.diff(m.indptr)
    assert ((np.bincount(u, minlength=len(rows)) < lens) & (np.bincount(u, minlength=len(rows)) > 0)).any()   # rows cut by the step
    assert (t[2][u == 7] < 0).all() and (u == 7).any()
    return m


@functools.lru_cache(maxsize=None)
def sparse300():
    """60 users x 300 items with one or two items each: most items receive nothing in a step; user 3 holds every item"""
    rng = np.random.default_rng(9)
    d = np.zeros((60, 300), dtype=bool)
    for u in range(60):
        d[u, rng.choice(300, size=1 + u % 2, replace=False)] = True
    d[3] = True
    return sp.csr_matrix(d.astype(np.float64))


TARGETS = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)


@pytest.mark.parametrize("precision", ["float", "double"])
@pytest.mark.parametrize("rank", [1, 10, 16, 17, 64, 128, "max"])
def test_one_step_equals_the_definition(rank, precision):
    dtype = DTYPES[precision]
    if rank == "max":
        rank = _lib.MAX_RANK if precision == "float" else _lib.MAX_RANK_F64
    rng = np.random.default_rng(rank)
    cases = [(dense12(t), 21, 1, 2) for t in TARGETS] + [(sparse300(), 4, 0, 1)]
    for m, seed, step, n_steps in cases:
        n_users, n_items = m.shape
        U, V = ((0.5 * rng.standard_normal((n, rank))).astype(dtype) for n in (n_users, n_items))
        aU, aV = rng.random(n_users) * 0.1, rng.random(n_items) * 0.1
        aU[0] = aV[1] = 0.0
        t = bpr_triples(seed, 0, 0, 0, m.indptr, m.indices, n_items, step, n_steps)
        ref = bpr_step_reference(U, V, aU, aV, *t, 0.05, 0.02, True)
        got = device_step(m, U, V, aU, aV, seed, 0, 0, step, n_steps, 0.05, 0.02, True)
        assert same_step(got, ref), (rank, precision, m.shape)
        z_moves = 0 < ref[5] < ref[4]                                        # (scores on both sides of 0: z is not a constant)
        assert z_moves or rank == 1
        if n_items == 300:
            idle = np.setdiff1d(np.arange(300), np.concatenate([t[1][t[2] >= 0], t[2][t[2] >= 0]]))
            assert idle.size > 100 and bits_equal(got[1][idle], V[idle]) and bits_equal(got[3][idle], aV[idle])
            assert (t[2][t[0] == 3] < 0).all() and bits_equal(got[0][3], U[3]) and got[2][3] == aU[3]
        else:
            assert bits_equal(got[0][7], U[7]) and got[2][7] == aU[7]        # the user whose triples are all void


@pytest.mark.parametrize("precision", ["float", "double"])
def test_frozen_items(precision):
    dtype = DTYPES[precision]
    m = dense12(CHUNK + 1)
    rng = np.random.default_rng(2)
    n_users = m.shape[0]
    U, V = ((0.5 * rng.standard_normal((n, 24))).astype(dtype) for n in (n_users, 12))
    aU, aV = rng.random(n_users) * 0.1, rng.random(12) * 0.1
    for mode, n_steps, step in ((1, 1, 0), (0, 2, 1)):
        t = bpr_triples(8, mode, 2, 0, m.indptr, m.indices, 12, step, n_steps)
        ref = bpr_step_reference(U, V, aU, aV, *t, 0.05, 0.02, False)
        got = device_step(m, U, V, aU, aV, 8, mode, 2, step, n_steps, 0.05, 0.02, False)
        assert same_step(got, ref) and bits_equal(got[1], V) and bits_equal(got[3], aV) and not bits_equal(got[0], U)


# ---- a fit -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fitted(precision):
    """the 900-user fixture, rank 16, 3 epochs, batch 4096 -> (model, U, the definition from the device-drawn initial factors)"""
    train, _, _ = protocol()
    be, tdt = backend(), TORCH[DTYPES[precision]]
    m = BPR(rank=16, learning_rate=0.1, lambda_=0.01, batch=4096, transform_iter=50, precision=precision, rng=5)
    U = m.fit_transform(train, 3)
    U0, V0 = (be.init_factors(m.seed, s, n, 16, tdt).cpu().numpy() for s, n in ((0, train.shape[0]), (1, train.shape[1])))
    ref = bpr_fit_reference(train.indptr, train.indices, train.shape[1], U0, V0, 3, m.seed, 0.1, 0.01, 4096)
    return m, U, ref


@pytest.mark.parametrize("precision", ["float", "double"])
def test_fit_equals_the_definition(precision):
    m, U, ref = fitted(precision)
    assert bits_equal(U, ref[0]) and bits_equal(m.components.T, ref[1]) and U.dtype == DTYPES[precision]
    assert bits_equal(m.user_adagrad, ref[2]) and bits_equal(m.item_adagrad, ref[3])
    assert m.trace == ref[4] and len(m.trace) == 3 and m.trace[2][1] > m.trace[0][1]
    train, _, _ = protocol()
    again = BPR(rank=16, learning_rate=0.1, lambda_=0.01, batch=4096, precision=precision, rng=5)
    U2 = again.fit_transform(train, 3)
    assert again.seed == m.seed and bits_equal(U2, U) and bits_equal(again.components, m.components) and again.trace == m.trace
    assert bits_equal(again.item_adagrad, m.item_adagrad)


def test_surface_on_the_fitted_model():
    m, _, ref = fitted("double")
    _, hist, held = protocol()
    V = ref[1]
    emb = m.transform(hist)
    fold = bpr_fit_reference(hist.indptr, hist.indices, hist.shape[1], np.zeros((hist.shape[0], 16)), V, 50, m.seed, 0.1, 0.01, 4096,
                             mode=1, update_items=False, aV=ref[3])
    assert bits_equal(emb, fold[0]) and bits_equal(m.components.T, V)       # the fold-in is the definition; the items are frozen
    assert bits_equal(m.transform(hist[5:20]), emb[5:20])
    # the same calls on the stand-in holding the definition's factors
    cpu = BPR(rank=16, learning_rate=0.1, lambda_=0.01, batch=4096, transform_iter=50, precision="double",
              backend=_oracle_metrics_backend())
    cpu.seed, cpu._V, cpu._aV = m.seed, torch.from_numpy(V.copy()), torch.from_numpy(ref[3].copy())
    top, top_cpu = m.predict(hist, 10), cpu.predict(hist, 10)
    assert np.array_equal(np.asarray(top), np.asarray(top_cpu)) and np.allclose(top.scores, top_cpu.scores, rtol=1e-12, atol=0)
    lists, _ = brute_lists(emb @ V.T, 10, hist, ())
    assert np.array_equal(np.asarray(top), lists)
    a = m.evaluate(hist, held, (5, 10), negatives=99, seed=7)
    b = cpu.evaluate(hist, held, (5, 10), negatives=99, seed=7)
    # Exact on both sides: the lists, the counts n, the fold-in embeddings (bit for bit above).  Not exact, and held to 1e-12
    # relative as the other surface tests of the package do: the scores of the lists, of `score` and the metric values -- the
    # scoring kernels add a row's rank products, and the metric kernels a list's at most ten terms, in another order than the
    # stand-in's numpy sums, so they differ by a few ulp of a double (2.2e-16 each) with nothing wrong on either side.
    for name in a:
        assert np.allclose(a[name], b[name], rtol=1e-12, atol=0, equal_nan=True), name
    pairs = sp.csr_matrix(np.random.default_rng(6).random(hist.shape) < 0.02)
    assert np.allclose(m.score(hist, pairs).data, cpu.score(hist, pairs).data, rtol=1e-12, atol=1e-300)
    ra, rb = m.evaluate_ranks(hist, held), cpu.evaluate_ranks(hist, held)
    assert ra["n"] == rb["n"] and all(np.isclose(ra[k], rb[k], rtol=1e-12, atol=0) for k in ("mpr", "auc", "mrr"))
    pop = np.broadcast_to(np.bincount(protocol()[0].indices, minlength=hist.shape[1]).astype(np.float64), hist.shape)
    print("NDCG@10 of the device fit (rank 16, 3 epochs): %.3f; popularity %.3f"
          % (ndcg10(np.asarray(top), held), ndcg10(brute_lists(pop, 10, hist, ())[0], held)))
    with pytest.raises(_lib.UnsupportedOnDevice):
        m.explain(hist, pairs)


# ---- the host-array entry ----------------------------------------------------------------------------------------------------------
def test_host_entry_is_the_device_route():
    be, lib = backend(), _lib.load()
    x = sp.csr_matrix((np.random.default_rng(3).random((30, 14)) < 0.35).astype(np.float64))
    x.sort_indices()
    p, j = x.indptr.astype(np.int32), x.indices.astype(np.int32)
    U, V, aU, aV, cnt = np.empty((30, 6)), np.empty((14, 6)), np.empty(30), np.empty(14), np.empty(8, np.int64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _lib.check(lib.rsparse_hip_bpr_fit(vp(p), vp(j), 30, 14, 99, 4, 16, 6, 0.1, 0.01, vp(U), vp(V), vp(aU), vp(aV), vp(cnt)))
    dU, dV = be.init_factors(99, 0, 30, 6, torch.float64), be.init_factors(99, 1, 14, 6, torch.float64)
    U0, V0 = dU.cpu().numpy(), dV.cpu().numpy()
    daU, daV = (torch.zeros(n, dtype=torch.float64, device=be.device) for n in (30, 14))
    counts = be.bpr_epochs(be.to_device(p, torch.int32), be.to_device(j, torch.int32), 14, x.nnz, 0, 99, 0, 0, 4, 16, dU, dV, daU, daV,
                           0.1, 0.01)
    for host, dev in ((U, dU), (V, dV), (aU, daU), (aV, daV), (cnt, counts.reshape(-1))):
        assert bits_equal(host, dev.cpu().numpy())
    ref = bpr_fit_reference(p, j, 14, U0, V0, 4, 99, 0.1, 0.01, 16)
    assert bits_equal(U, ref[0]) and bits_equal(V, ref[1]) and [tuple(r) for r in cnt.reshape(4, 2).tolist()] == ref[4]
