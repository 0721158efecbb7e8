"""The candidate select and the score gather of wrmf_itemknn.hip against the numpy definitions of rsparse_amd/itemknn.py
(knn_candidates_reference, knn_score_pairs_reference), through HipBackend: every comparison is np.array_equal.  The candidate rows
sit where the kernel changes course -- the wave, the LDS buffer of RSPARSE_HIP_KNN_LDS_CAND entries and the restricted dense row
beyond it --, on a planted matrix with tied items and on a catalogue larger than the buffer, for binary rows and for rows with
integer weights, in batches of one, two and three dense rows."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import _lib
from rsparse_amd.itemknn import (canonical_pattern, cooccurrence_reference, knn_candidates_reference, knn_recommend_reference,
                                 knn_score_pairs_reference, weight_table)

pytestmark = pytest.mark.gpu

CAND, SPAN = _lib.KNN_LDS_CAND, _lib.KNN_SPAN
N_BIG = CAND + 100
KINDS = ("binary", "weighted")


@functools.lru_cache(maxsize=None)
def backend():
    from rsparse_amd.engine import HipBackend
    return HipBackend()


# ---- the problems: (x, neighbors, q, xv) ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted():
    """160 users x 300 items of rising popularity, rows of 1, 63, 64, 65 and 257 items (users 0 .. 4), an empty history (user 5),
    items 10 and 11 with the same users (and so the same score wherever neither is in the row); the cosine table at K = 50"""
    rng = np.random.default_rng(7)
    n_users, n_items = 160, 300
    d = rng.random((n_users, n_items)) < np.linspace(0.02, 0.25, n_items)[None, :]
    free = np.setdiff1d(np.arange(n_items), (10, 11))
    d[:6] = False
    for u, length in enumerate((1, 63, 64, 65, 257)):
        d[u, rng.choice(free, size=length, replace=False)] = True
    d[:, 11] = d[:, 10]
    assert d[:6].sum(axis=1).tolist() == [1, 63, 64, 65, 257, 0] and d[:, 10].any()
    x = sp.csr_matrix(d.astype(np.float64))
    nb, ct, cnt = cooccurrence_reference(x, 50, "cosine")
    return x, nb, weight_table(nb, ct, cnt, "cosine")


@functools.lru_cache(maxsize=None)
def big():
    """12 users x (CAND + 100) items under a made-up table of K = 8 (some slots empty, weights up to 2^30): user 0 has an empty
    history, the others 30 items each"""
    rng = np.random.default_rng(11)
    d = np.zeros((12, N_BIG), dtype=bool)
    for u in range(1, 12):
        d[u, rng.choice(N_BIG, size=30, replace=False)] = True
    nb = rng.integers(0, N_BIG, size=(N_BIG, 8)).astype(np.int32)
    nb[rng.random(nb.shape) < 0.1] = -1
    q = rng.integers(1, (1 << 30) + 1, size=nb.shape).astype(np.int64)
    q[:, 0] = 1 << 30
    q[nb < 0] = 0
    return sp.csr_matrix(d.astype(np.float64)), nb, q


PROBLEMS = {"planted": planted, "big": big}


@functools.lru_cache(maxsize=None)
def row_weights(name):
    """an integer weight in 1 .. 2^16 - 1 for every stored entry of the problem's rows"""
    x = canonical_pattern(PROBLEMS[name]()[0])
    xv = np.random.default_rng(3).integers(1, 1 << 16, size=x.nnz).astype(np.int64)
    xv[:2] = (1 << 16) - 1
    return xv


def problem(name, kind):
    x, nb, q = PROBLEMS[name]()
    return x, nb, q, (row_weights(name) if kind == "weighted" else None)


def rows_pattern(rows, n_items):
    """a CSR pattern from a list of index arrays"""
    lens = [len(r) for r in rows]
    idx = np.concatenate([np.sort(np.asarray(r, dtype=np.int64)) for r in rows]) if sum(lens) else np.zeros(0, np.int64)
    return sp.csr_matrix((np.ones(idx.size), idx, np.concatenate([[0], np.cumsum(lens)])), shape=(len(rows), n_items))


@functools.lru_cache(maxsize=None)
def big_case(kind):
    """the candidate rows of the large catalogue with their filters -> (cand, nr, excl): rows of 0, 1, 63, 64, 65, CAND and
    CAND + 1 entries, the whole catalogue, candidates that are all masked, three admissible candidates (fewer than any k > 3), 20
    candidates of score 0, and -- row 0, the user without a history -- 200 candidates that all score 0"""
    x, nb, q, xv = problem("big", kind)
    rng = np.random.default_rng(5)
    excl = (7, 64, N_BIG - 1)
    nr = x.tolil(copy=True)
    nr[8, :50] = 1                                                          # the row whose candidates are all masked
    nr = sp.csr_matrix(nr)
    score = knn_score_pairs_reference(x, nb, q, sp.csr_matrix(np.ones(x.shape)), xv).reshape(x.shape)
    pick = lambda n: rng.choice(N_BIG, size=n, replace=False)
    adm9 = np.setdiff1d(np.arange(N_BIG), np.concatenate([nr[9].indices, excl]))
    zero10 = np.setdiff1d(np.flatnonzero(score[10] == 0), np.concatenate([nr[10].indices, excl]))
    rows = [pick(200), pick(0), pick(1), pick(63), pick(64), pick(65), pick(CAND), pick(CAND + 1), np.arange(50),
            np.concatenate([adm9[:3], nr[9].indices[:5], excl]), zero10[:20], np.arange(N_BIG)]
    assert (score[0] == 0).all() and (score[10][rows[10]] == 0).all() and len(rows[10]) == 20
    return rows_pattern(rows, N_BIG), nr, excl


def device_operands(x, nb, q, xv):
    be = backend()
    m = canonical_pattern(x)
    dev = lambda a, t=torch.int32: be.to_device(np.ascontiguousarray(a), t)
    kw = {} if xv is None else {"xv": dev(xv, torch.int64)}
    return (dev(m.indptr), dev(m.indices), dev(nb), dev(q, torch.int64)), kw


def device_filters(nr, excl):
    be = backend()
    out = {}
    if nr is not None:
        nr = sp.csr_matrix(nr)
        nr.sort_indices()
        out.update(nr_p=be.to_device(nr.indptr, torch.int32), nr_j=be.to_device(nr.indices, torch.int32))
    if len(excl):
        out["exclude0"] = be.to_device(np.asarray(excl, dtype=np.int32), torch.int32)
    return out


def zero_based(res, sc):
    torch.cuda.synchronize()
    res, sc = res.cpu().numpy().astype(np.int64), sc.cpu().numpy()
    return np.where(res == -2147483648, -1, res - 1), sc


def device_candidates(name, kind, cand, k, nr=None, excl=(), ws_rows=0):
    be = backend()
    x, nb, q, xv = problem(name, kind)
    rows, kw = device_operands(x, nb, q, xv)
    c = canonical_pattern(cand)
    res, sc = be.knn_top_candidates(*rows, k, be.to_device(c.indptr, torch.int32), be.to_device(c.indices, torch.int32), ws_rows=ws_rows,
                                    **device_filters(nr, excl), **kw)
    assert res.dtype == torch.int32 and sc.dtype == torch.int64 and tuple(res.shape) == (x.shape[0], k)
    return zero_based(res, sc)


def device_lists(name, kind, k, nr=None, excl=(), ws_rows=0):
    x, nb, q, xv = problem(name, kind)
    rows, kw = device_operands(x, nb, q, xv)
    f = device_filters(nr, excl)
    return zero_based(*backend().knn_recommend(*rows, k, f.get("nr_p"), f.get("nr_j"), f.get("exclude0"), ws_rows=ws_rows, **kw))


def device_scores(name, kind, pairs, ws_rows=0):
    be = backend()
    x, nb, q, xv = problem(name, kind)
    rows, kw = device_operands(x, nb, q, xv)
    p = canonical_pattern(pairs)
    out = be.knn_score_pairs(*rows, be.to_device(p.indptr, torch.int32), be.to_device(p.indices, torch.int32), ws_rows=ws_rows, **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.int64
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def plain_reference(name, kind, k):
    x, nb, q, xv = problem(name, kind)
    return knn_recommend_reference(x, nb, q, k, None, (), xv=xv)


def check_workspace_is_clean(name, kind):
    """a plain, unfiltered knn_recommend behind the call: a cell left with a score, a mask or a mark would change a list"""
    k = 50
    got, ref = device_lists(name, kind, k), plain_reference(name, kind, k)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


@functools.lru_cache(maxsize=None)
def big_reference(kind, k):
    x, nb, q, xv = problem("big", kind)
    cand, nr, excl = big_case(kind)
    return knn_candidates_reference(x, nb, q, cand, k, nr, excl, xv=xv)


# ---- the candidate select -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 10, 1024))
@pytest.mark.parametrize("kind", KINDS)
def test_candidate_rows_at_every_edge_of_the_kernel(kind, k):
    cand, nr, excl = big_case(kind)
    items, scores = device_candidates("big", kind, cand, k, nr, excl)
    ref = big_reference(kind, k)
    assert np.array_equal(items, ref[0]) and np.array_equal(scores, ref[1])
    n_adm = (ref[0] >= 0).sum(axis=1)
    assert n_adm[1] == 0 and n_adm[8] == 0 and n_adm[9] == min(3, k)        # no candidate, all masked, fewer than k admissible
    # candidates that all score 0 are listed in ascending order (the user without a history, and the planted zeros of row 10)
    for u in (0, 10):
        adm = np.setdiff1d(cand[u].indices, np.concatenate([nr[u].indices, excl]))
        assert np.array_equal(items[u, :n_adm[u]], adm[:k]) and (scores[u] == 0).all()
    if k == 1024:
        assert n_adm[6] == 1024 and n_adm[7] == 1024 and n_adm[11] == 1024  # CAND, CAND + 1 and all items: full lists
        assert (scores[11, :100] > 0).all()
    check_workspace_is_clean("big", kind)


@pytest.mark.parametrize("ws_rows", (1, 2, 3))
@pytest.mark.parametrize("kind", KINDS)
def test_candidates_in_batches_of_rows(kind, ws_rows):
    cand, nr, excl = big_case(kind)
    items, scores = device_candidates("big", kind, cand, 10, nr, excl, ws_rows=ws_rows)
    ref = big_reference(kind, 10)
    assert np.array_equal(items, ref[0]) and np.array_equal(scores, ref[1])
    check_workspace_is_clean("big", kind)


@pytest.mark.parametrize("kind", KINDS)
def test_candidates_on_the_planted_matrix_with_ties(kind):
    x, nb, q, xv = problem("planted", kind)
    rng = np.random.default_rng(21)
    d = rng.random(x.shape) < 0.4
    d[:, 10:12] = True                                                     # the two identical items are candidates of every row
    cand = sp.csr_matrix(d.astype(np.float64))
    excl = (0, 5, 64)
    for k, nr in ((10, x), (1, None), (300, x)):
        items, scores = device_candidates("planted", kind, cand, k, nr, excl)
        ref = knn_candidates_reference(x, nb, q, cand, k, nr, excl, xv=xv)
        assert np.array_equal(items, ref[0]) and np.array_equal(scores, ref[1])
    # the tie rule is exercised: some list holds items 10 and 11 next to each other with one score, the smaller item first
    at = np.argwhere(items[:, :-1] == 10)
    tied = [(u, t) for u, t in at if items[u, t + 1] == 11 and scores[u, t] == scores[u, t + 1] > 0]
    assert tied
    assert (items[5, :3] == np.setdiff1d(np.flatnonzero(d[5]), excl)[:3]).all() and (scores[5] == 0).all()   # the empty history
    check_workspace_is_clean("planted", kind)


@pytest.mark.parametrize("name,k", (("planted", 10), ("planted", 300), ("big", 10), ("big", 1024)))
@pytest.mark.parametrize("kind", KINDS)
def test_every_item_as_candidate_reproduces_knn_recommend(name, kind, k):
    x, nb, q, xv = problem(name, kind)
    every = sp.csr_matrix(np.ones(x.shape))
    excl = (3, 11)
    lists = device_lists(name, kind, k, x, excl)
    ref = knn_recommend_reference(x, nb, q, k, x, excl, xv=xv)
    assert np.array_equal(lists[0], ref[0]) and np.array_equal(lists[1], ref[1])
    cref = knn_candidates_reference(x, nb, q, every, k, x, excl, xv=xv)
    assert np.array_equal(cref[0], ref[0]) and np.array_equal(cref[1], ref[1])           # in the definitions
    got = device_candidates(name, kind, every, k, x, excl, ws_rows=5)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])             # on the device
    check_workspace_is_clean(name, kind)


# ---- the score gather ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws_rows", (0, 1, 3))
@pytest.mark.parametrize("kind", KINDS)
def test_score_pairs_against_the_definition(kind, ws_rows):
    """pairs rows of 0, 1, SPAN - 1, SPAN, SPAN + 1 and many entries: spans of the flat positions that start and end inside rows"""
    x, nb, q, xv = problem("planted", kind)
    rng = np.random.default_rng(31)
    rows = [rng.choice(300, size=n, replace=False) for n in (0, 1, SPAN - 1, SPAN, SPAN + 1, 300)]
    rows += [rng.choice(300, size=int(n), replace=False) for n in rng.integers(0, 40, size=x.shape[0] - len(rows))]
    pairs = rows_pattern(rows, 300)
    got = device_scores("planted", kind, pairs, ws_rows)
    ref = knn_score_pairs_reference(x, nb, q, pairs, xv)
    assert got.shape == ref.shape and np.array_equal(got, ref) and (ref > 0).any() and (ref == 0).any()
    check_workspace_is_clean("planted", kind)


@pytest.mark.parametrize("name", ("planted", "big"))
@pytest.mark.parametrize("kind", KINDS)
def test_score_pairs_at_the_positions_of_a_list_are_the_lists_scores(name, kind):
    x, nb, q, xv = problem(name, kind)
    if name == "big":
        cand, nr, excl = big_case(kind)
    else:
        cand, nr, excl = sp.csr_matrix((np.random.default_rng(2).random(x.shape) < 0.3).astype(np.float64)), x, (1,)
    items, scores = device_candidates(name, kind, cand, 10, nr, excl)
    listed = rows_pattern([row[row >= 0] for row in items], x.shape[1])
    got = device_scores(name, kind, listed)
    for u in range(x.shape[0]):
        row = items[u][items[u] >= 0]
        order = np.argsort(row)                                             # the pattern holds the list's items in ascending order
        assert np.array_equal(got[listed.indptr[u]:listed.indptr[u + 1]], scores[u, :row.size][order])
    assert (got > 0).any()


# ---- repeated calls -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_repeated_calls_return_the_same_bits(kind):
    cand, nr, excl = big_case(kind)
    first = device_candidates("big", kind, cand, 10, nr, excl, ws_rows=2)
    second = device_candidates("big", kind, cand, 10, nr, excl, ws_rows=2)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    s1, s2 = device_scores("big", kind, cand), device_scores("big", kind, cand)
    assert np.array_equal(s1, s2)
    check_workspace_is_clean("big", kind)
