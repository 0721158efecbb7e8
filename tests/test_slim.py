"""SLIM on the device (wrmf_slim.hip behind rsparse_hip_slim_columns_device / rsparse_hip_slim_fit) against the numpy definition of
rsparse_amd/slim.py: the weights and the sweep counts bit for bit, in both precisions."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import load_movielens
from rsparse_amd import SLIM, _lib
from rsparse_amd.ease import (ease_candidates_reference, ease_gram_reference, ease_ranks_reference, ease_recommend_reference,
                              ease_score_pairs_reference)
from rsparse_amd.slim import slim_columns_reference

pytestmark = pytest.mark.gpu

CAP = _lib.SLIM_LDS_SUPPORT
DTYPES = {"float": np.float32, "double": np.float64}


@functools.lru_cache(maxsize=None)
def backend():
    from rsparse_amd.engine import HipBackend
    return HipBackend()


def device_columns(G, cols, l1, l2, max_iter, tol, dtype, d_G=None):
    """-> (W (n_items, n_items) of dtype, sweeps int32 per element of cols): the layout of slim_columns_reference"""
    be = backend()
    n = G.shape[0]
    elems = 256 // np.dtype(dtype).itemsize
    W = torch.zeros((n, (n + elems - 1) // elems * elems), dtype=torch.float32 if dtype == np.float32 else torch.float64, device=be.device)
    d_G = be.to_device(G, torch.float64) if d_G is None else d_G
    sweeps = be.slim_columns(d_G, be.to_device(np.asarray(cols, dtype=np.int32), torch.int32), l1, l2, max_iter, tol, W)
    got = W.cpu().numpy()
    assert (got[:, n:] == 0).all()                                           # the padding of a row is left alone
    return got[:, :n].copy(), sweeps.cpu().numpy()


def same(got, ref):
    bits = np.uint32 if ref[0].dtype == np.float32 else np.uint64
    return (got[0].dtype == ref[0].dtype and np.array_equal(got[0].view(bits), ref[0].view(bits)) and got[1].dtype == np.int32
            and np.array_equal(got[1], ref[1]))


def support_sizes(G):
    return (G > 0).sum(axis=1) - (np.diag(G) > 0)


def from_users(users, n_items):
    rows = np.repeat(np.arange(len(users)), [len(u) for u in users])
    cols = np.concatenate([np.asarray(u, dtype=np.int64) for u in users])
    return sp.csr_matrix((np.ones(cols.size), (rows, cols)), shape=(len(users), n_items))


# ---- support sizes -----------------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def sized():
    """300 items.  Item t < 9 (a target) is held by two users only, whose other items are two overlapping stretches of a set of
    SIZES[t] background items: its support is exactly SIZES[t], with counts of 1 and 2.  The background items 9 .. 299 are
    also held by 30 sparse users.  -> (G, the reference at l1 = 0.3, l2 = 0.5, 8 sweeps, tol = 1e-4, in both precisions)"""
    rng = np.random.default_rng(3)
    n_items, users = 300, []
    for t, s in enumerate(SIZES):
        chosen = np.sort(rng.choice(np.arange(9, n_items), size=s, replace=False))
        users += [np.r_[t, chosen[:(2 * s + 2) // 3]], np.r_[t, chosen[s // 3:]]]
    users += [9 + np.flatnonzero(rng.random(n_items - 9) < 0.05) for _ in range(30)]
    G = ease_gram_reference(from_users(users, n_items), 0.0)
    assert support_sizes(G)[:9].tolist() == list(SIZES) and set(G[:9].ravel()) == {0.0, 1.0, 2.0}
    cols = np.arange(n_items)
    return G, {name: slim_columns_reference(G, cols, 0.3, 0.5, 8, 1e-4, dt) for name, dt in DTYPES.items()}


@pytest.mark.parametrize("precision", ["double", "float"])
def test_support_sizes_around_the_window(precision):
    G, ref = sized()
    got = device_columns(G, np.arange(300), 0.3, 0.5, 8, 1e-4, DTYPES[precision])
    assert same(got, ref[precision])
    assert ref[precision][1][0] == 0 and (ref[precision][1][1:9] >= 1).all() and (ref["double"][0][:, 1:9] > 0).any(axis=0).all()
    assert np.array_equal(ref["float"][0], ref["double"][0].astype(np.float32))     # the float weights: the double ones rounded once


def test_column_lists_repeats_and_a_small_call_behind_a_larger_one():
    G, ref = sized()
    W, sweeps = ref["double"]
    d_G = backend().to_device(G, torch.float64)
    first = device_columns(G, np.arange(300), 0.3, 0.5, 8, 1e-4, np.float64, d_G)
    assert same(first, ref["double"]) and same(device_columns(G, np.arange(300), 0.3, 0.5, 8, 1e-4, np.float64, d_G), first)
    for cols in ([7], [8, 3], [299, 0, 150, 8, 8, 5, 150], np.random.default_rng(1).permutation(300)):
        cols = np.asarray(cols)
        only = np.zeros_like(W)
        only[:, cols] = W[:, cols]
        assert same(device_columns(G, cols, 0.3, 0.5, 8, 1e-4, np.float64, d_G), (only, sweeps[cols])), cols
    got = device_columns(G, np.zeros(0, np.int32), 0.3, 0.5, 8, 1e-4, np.float64, d_G)
    assert (got[0] == 0).all() and got[1].size == 0
    for bad in (-1, 300):
        with pytest.raises(_lib.RsparseHipError) as e:
            device_columns(G, [3, bad], 0.3, 0.5, 8, 1e-4, np.float64, d_G)
        assert e.value.code == _lib.ERR_INVALID and "a column outside" in str(e.value)


# ---- the LDS bound -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def around_the_bound(case):
    """CAP + 2 items.  "mixed": one user holds every item but item 0, another one item 0 and items 1 .. 10 -- item 0 has a support
    of 10, items 1 .. 10 of CAP + 1 (the workspace route), the others of CAP (the last size in LDS).  "below": one user holds the
    items below CAP, another one the items 0 .. 4, CAP and CAP + 1 -- supports of CAP - 1, but CAP + 1 for items 0 .. 4 and 6 for
    the last two.  A few sparse users inside the big user's items vary the counts and leave the supports alone.
    -> (G, cols, their support sizes)"""
    rng = np.random.default_rng(17)
    n_items = CAP + 2
    if case == "mixed":
        users = [np.arange(1, n_items), np.arange(0, 11)]
        inside, cols = np.arange(11, n_items), [5, 0, n_items - 1, 1000, 10]
    else:
        users = [np.arange(0, CAP), np.r_[np.arange(0, 5), CAP, CAP + 1]]
        inside, cols = np.arange(5, CAP), [CAP, 2, CAP - 1, 700]
    users += [inside[rng.random(inside.size) < 0.02] for _ in range(6)]
    G = ease_gram_reference(from_users(users, n_items), 0.0)
    return G, np.asarray(cols), support_sizes(G)[cols]


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("case", ["mixed", "below"])
def test_supports_around_the_lds_bound(case, precision):
    G, cols, sizes = around_the_bound(case)
    assert sizes.tolist() == ([CAP + 1, 10, CAP, CAP, CAP + 1] if case == "mixed" else [6, CAP + 1, CAP - 1, CAP - 1])
    ref = slim_columns_reference(G, cols, 0.1, 0.5, 2, 1e-4, DTYPES[precision])
    assert (ref[1] == 2).all()
    assert same(device_columns(G, cols, 0.1, 0.5, 2, 1e-4, DTYPES[precision]), ref)


# ---- where the first change sits ---------------------------------------------------------------------------------------------------
def planted(strong, where, m=200):
    """A target whose support is m items of count 1 (one user holds the target and all of them) except the support positions
    `strong`, of count 5 (four more users hold the target and that item).  where: the target's index is below, inside or above
    its support.  -> (G, the target, its support)"""
    j = {"below": 0, "inside": m // 2, "above": m}[where]
    S = np.delete(np.arange(m + 1), j)
    users = [np.arange(m + 1)] + [np.array([j, S[p]]) for p in strong for _ in range(4)]
    G = ease_gram_reference(from_users(users, m + 1), 0.0)
    assert np.array_equal(np.flatnonzero(G[j, S] == 5), strong) and (np.delete(G[j, S], strong) == 1).all()
    return G, j, S


@pytest.mark.parametrize("where", ["below", "inside", "above"])
@pytest.mark.parametrize("strong", [(0,), (63,), (64,), (130,), (10, 20), (63, 64, 199)])
def test_the_first_change_of_a_window(strong, where):
    """l1 = 2 lets only the strong coordinates move: the first change of a window sits at lane 0, 63 or, for position 64, at lane 0
    of the second window; every other window has none; (10, 20): two changes in one window."""
    G, j, S = planted(list(strong), where)
    ref = slim_columns_reference(G, [j], 2.0, 0.5, 20, 0.0)
    assert np.array_equal(np.flatnonzero(ref[0][S, j]), strong) and ref[1][0] >= 2
    for dtype in DTYPES.values():
        assert same(device_columns(G, [j], 2.0, 0.5, 20, 0.0, dtype), slim_columns_reference(G, [j], 2.0, 0.5, 20, 0.0, dtype))
    # nothing passes the penalty: one sweep of windows without a change
    none = device_columns(G, [j], 5.0, 0.5, 20, 0.0, np.float64)
    assert (none[0] == 0).all() and none[1].tolist() == [1]


def test_a_coordinate_that_goes_back_to_zero():
    """Item 1 has the target's five users and no other, item 0 three of them: item 0 comes first, takes a weight in the first
    sweep and loses it again once item 1 has taken its own."""
    users = [[0, 1, 2], [0, 1, 2], [0, 1, 2], [1, 2], [1, 2], [0, 1, 2, 3, 4, 5], [3, 4], [5, 0]]
    G = ease_gram_reference(from_users(users, 6), 0.0)
    seen = [slim_columns_reference(G, [2], 0.5, 0.1, n, 0.0)[0][0, 2] for n in range(1, 40)]
    assert seen[0] > 0 and seen[-1] == 0                                     # the reference does take the step back to +0.0
    for n in (1, 2, 5, 39):
        for dtype in DTYPES.values():
            assert same(device_columns(G, [2], 0.5, 0.1, n, 0.0, dtype), slim_columns_reference(G, [2], 0.5, 0.1, n, 0.0, dtype)), n


# ---- penalties, tolerance, tiny catalogues -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_gram(n_users=60, n_items=40, density=0.3):
    x = sp.csr_matrix((np.random.default_rng(n_items).random((n_users, n_items)) < density).astype(np.float64))
    return x, ease_gram_reference(x, 0.0)


@pytest.mark.parametrize("l1,l2,max_iter,tol", [(0.0, 0.5, 30, 1e-4), (0.5, 0.0, 30, 1e-4), (0.0, 0.0, 12, 1e-3), (0.5, 1.0, 25, 0.0),
                                               (0.5, 1.0, 1, 1e-4), (0.5, 1.0, 2, 1e-4), (0.5, 1.0, 2000, 1e-14), (100.0, 1.0, 5, 1e-4)])
def test_penalties_and_tolerances(l1, l2, max_iter, tol):
    _, G = random_gram()
    cols = np.arange(40)
    for dtype in DTYPES.values():
        ref = slim_columns_reference(G, cols, l1, l2, max_iter, tol, dtype)
        assert same(device_columns(G, cols, l1, l2, max_iter, tol, dtype), ref)
    if tol == 0.0:
        assert (ref[1] == max_iter).all()                                    # (no column of this matrix reaches an exact fixed point)


@pytest.mark.parametrize("n_items", [1, 2])
def test_catalogues_of_one_and_two_items(n_items):
    x = sp.csr_matrix(np.ones((3, n_items)))
    G = ease_gram_reference(x, 0.0)
    for dtype in DTYPES.values():
        ref = slim_columns_reference(G, np.arange(n_items), 0.5, 1.0, 10, 1e-4, dtype)
        assert same(device_columns(G, np.arange(n_items), 0.5, 1.0, 10, 1e-4, dtype), ref)
    assert ref[1].tolist() == ([0] if n_items == 1 else [2, 2]) and (n_items == 1 or ref[0][0, 1] == 2.5 / 4)


def test_host_array_entry():
    x, G = random_gram()
    n = 40
    W, sweeps = np.full((n, n), -1.0, order="F"), np.full(n, -1, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _lib.check(_lib.load().rsparse_hip_slim_fit(vp(x.indptr.astype(np.int32)), vp(x.indices.astype(np.int32)), 60, n, 0.5, 1.0, 25, 1e-4,
                                                vp(W), vp(sweeps)))
    assert same((np.ascontiguousarray(W), sweeps), slim_columns_reference(G, np.arange(n), 0.5, 1.0, 25, 1e-4))
    assert same((np.ascontiguousarray(W), sweeps), device_columns(G, np.arange(n), 0.5, 1.0, 25, 1e-4, np.float64))


# ---- the class -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def movielens_csr():
    n_user, n_item, p, i, x = load_movielens()
    m = sp.csc_matrix((np.ones_like(x), i, p), shape=(n_user, n_item)).tocsr()
    m.sort_indices()
    return m


@functools.lru_cache(maxsize=None)
def fitted(precision):
    return SLIM(1.0, 500.0, precision=precision, backend=backend()).fit(movielens_csr()[:900])


SUBSET = (0, 49, 180, 299, 500, 900, 1300, 1681)


@pytest.mark.parametrize("precision", ["float", "double"])
def test_fit_equals_the_definition_on_a_subset_of_columns(precision):
    """the full fit (l1 = 1, l2 = 500, 100 sweeps, tol = 1e-4) of the 900 training users against the numpy definition on the columns
    SUBSET; the class orders the columns by support, the definition does not care"""
    m = fitted(precision)
    train = movielens_csr()[:900]
    G = ease_gram_reference(train, 0.0)
    W, sweeps = slim_columns_reference(G, SUBSET, 1.0, 500.0, 100, 1e-4, DTYPES[precision])
    got = m.W
    assert got.dtype == DTYPES[precision] and got.shape == (1682, 1682) and np.array_equal(got[:, SUBSET], W[:, SUBSET])
    assert m.n_sweeps.dtype == np.int32 and np.array_equal(m.n_sweeps[list(SUBSET)], sweeps)
    assert (got >= 0).all() and (np.diag(got) == 0).all() and np.array_equal(m.item_count, np.diag(G))
    assert (m.n_sweeps[np.diag(G) == 0] == 0).all() and m.n_sweeps.max() <= 100
    print("%s: %.0f non-zeros per column, sweeps: median %d, max %d, %d columns at the cap"
          % (precision, (got > 0).sum() / 1682, np.median(m.n_sweeps), m.n_sweeps.max(), (m.n_sweeps == 100).sum()))


def held_out_split():
    test = movielens_csr()[900:].tocsr()
    held_mask = np.random.default_rng(7).random(test.nnz) < 0.5
    part = lambda keep: sp.csr_matrix((test.data[keep], test.indices[keep], np.concatenate([[0], np.cumsum(keep)])[test.indptr]), shape=test.shape)
    return part(~held_mask), part(held_mask)


@pytest.mark.parametrize("precision", ["float", "double"])
def test_inference_is_ease_on_the_downloaded_weights(precision):
    m = fitted(precision)
    W = m.W
    hist, held = held_out_split()
    top = m.predict(hist, 10, items_exclude=(49,))
    ref = ease_recommend_reference(hist, W, 10, hist, (49,))
    assert np.array_equal(np.asarray(top), ref[0]) and np.array_equal(top.scores, ref[1])
    cand = m.sample_negatives(hist, 99, actual=held, seed=7)
    lists = ease_candidates_reference(hist, W, cand, 10, hist, ())[0]
    a = m.evaluate(hist, held, 10, metrics=("ndcg", "hit"), negatives=99, seed=7)
    c = m.evaluate(hist, held, 10, metrics=("ndcg", "hit"), candidates=cand)
    assert np.array_equal(np.asarray(m.predict(hist, 10, candidates=cand)), lists)
    assert all(np.array_equal(a[name], c[name], equal_nan=True) for name in ("ndcg", "hit"))
    pairs = sp.csr_matrix(np.random.default_rng(6).random(hist.shape) < 0.03)
    assert np.array_equal(m.score(hist, pairs).data, ease_score_pairs_reference(hist, W, pairs))
    ref = ease_ranks_reference(hist, W, held, hist, (1,))
    above, tied, n_adm = m.held_out_ranks(hist, held, items_exclude=(1,))
    assert np.array_equal(above.data, ref[0]) and np.array_equal(tied.data, ref[1]) and np.array_equal(n_adm, ref[2])


def test_full_fit_beats_popularity():
    from test_ease_host import brute_lists, ndcg10
    m = fitted("float")
    hist, held = held_out_split()
    top = m.predict(hist, 10)
    pop_lists, _ = brute_lists(np.broadcast_to(m.item_count.astype(np.float64), hist.shape), 10, hist, ())
    slim, popularity = ndcg10(np.asarray(top), held), ndcg10(pop_lists, held)
    print("NDCG@10: SLIM(l1 = 1, l2 = 500) %.3f, popularity %.3f" % (slim, popularity))
    assert slim > popularity
