"""The weighted forms of the ItemKNN kernels (wrmf_itemknn.hip) against the numpy definitions of rsparse_amd/itemknn.py: every
comparison is np.array_equal -- integer operands, 64-bit integer atomics and a key of three stated roundings, there is no
tolerance.  The shapes sit where the kernels change course, as in test_itemknn.py: the span a wave takes of the stored entries, the
lane group's share of an inner list, the LDS candidate buffer of the select (and the radix fallback and tie pass beyond it),
batches of one, two and three dense rows -- and where the weighted forms can go wrong on their own: sums beyond 32 bits and up to
2^53, l != r, a key whose order a fused multiply-add would change, rows of weights at both ends of their range."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import Confidence, ItemKNN, _lib
from rsparse_amd.itemknn import XQ_MAX, canonical_pattern, knn_recommend_reference, weighted_cooccurrence_reference

pytestmark = pytest.mark.gpu

SPAN, CAND = _lib.KNN_SPAN, _lib.KNN_LDS_CAND
TOP16 = 2 ** 16 - 1


@functools.lru_cache(maxsize=None)
def backend():
    from rsparse_amd.engine import HipBackend
    return HipBackend()


# ---- the problems: (pattern m, l, r by stored position, a, b, h) ---------------------------------------------------------------------
def operands(d, seed, top=TOP16, h=0.0, same=()):
    """random l != r in 1 .. top on the pattern of the boolean matrix d, random tables; `same`: pairs of columns (of equal users)
    that get equal operands and equal table entries"""
    rng = np.random.default_rng(seed)
    m = canonical_pattern(sp.csr_matrix(d.astype(np.float64)))
    L, R = rng.integers(1, top + 1, d.shape), rng.integers(1, top + 1, d.shape)
    a, b = rng.uniform(0.5, 2.0, d.shape[1]), rng.uniform(0.5, 2.0, d.shape[1])
    for i, j in same:
        L[:, j], R[:, j], a[j], b[j] = L[:, i], R[:, i], a[i], b[i]
    rows = np.repeat(np.arange(d.shape[0]), np.diff(m.indptr))
    return m, L[rows, m.indices], R[rows, m.indices], a, b, h


def planted_pattern():
    """160 users x 300 items of rising popularity.  Rows of 1, 63, 64, 65 and 257 items (users 0 .. 4); columns of 0, 1, 64, 65 and
    2 SPAN + 1 users (items 299 .. 295); items 10, 11 and items 12, 13 with the same users."""
    rng = np.random.default_rng(7)
    n_users, n_items = 160, 300
    d = rng.random((n_users, n_items)) < np.linspace(0.02, 0.25, n_items)[None, :]
    d[:, 11] = d[:, 10]
    d[:, 13] = d[:, 12]
    free = np.setdiff1d(np.arange(295), (10, 11, 12, 13))
    d[:5] = False
    for u, length in enumerate((1, 63, 64, 65, 257)):
        d[u, rng.choice(free, size=length, replace=False)] = True
    for item, users in ((299, 0), (298, 1), (297, 64), (296, 65), (295, 2 * SPAN + 1)):
        d[:, item] = False
        d[5 + rng.choice(n_users - 5, size=users, replace=False), item] = True
    assert d[:5].sum(axis=1).tolist() == [1, 63, 64, 65, 257]
    assert d[:, 295:].sum(axis=0).tolist() == [2 * SPAN + 1, 65, 64, 1, 0]
    assert (d[:, 10] == d[:, 11]).all() and d[:, 10].any() and (d[:, 12] == d[:, 13]).all() and d[:, 12].sum() > 1
    return d


def planted(h=0.0):
    # items 10 and 11: identical users AND identical weights; items 12 and 13: identical users, different weights
    return operands(planted_pattern(), 11, h=h, same=((10, 11),))


def small(n_items):
    rng = np.random.default_rng(100 + n_items)
    d = rng.random((40, n_items)) < np.linspace(0.1, 0.6, n_items)[None, :]
    d[0] = True                                                           # a user of every item: each item has n_items - 1 neighbours
    return operands(d, 200 + n_items)


def dense_pattern():
    rng = np.random.default_rng(9)
    n_items = CAND + 100
    d = np.zeros((3, n_items), dtype=bool)
    d[0] = True                                                           # one user holds all CAND + 100 items
    d[1, rng.choice(n_items, size=2000, replace=False)] = True
    d[2, rng.choice(n_items, size=50, replace=False)] = True
    return d


def dense_varied():
    return operands(dense_pattern(), 12)


def dense_equal():
    """all weights and table entries equal: rows of more than CAND cells of ONE key, the radix select resolves all eight bytes and
    the tie pass picks the first K by index"""
    m, l, r, a, b, h = operands(dense_pattern(), 13)
    return m, np.ones_like(l), np.ones_like(r), np.full_like(a, 1.5), np.full_like(b, 0.75), 0.125


def wide_sums():
    """31 users of 5 items with l, r at and just below 2^24: sums beyond 2^32 and up to 2^48 31, the largest below 2^53 that 31
    users admit; item 4 has one user"""
    rng = np.random.default_rng(14)
    d = np.ones((31, 5), dtype=bool)
    d[1:, 4] = False
    m, l, r, a, b, h = operands(d, 15)
    top = 2 ** 24
    l, r = top - rng.integers(0, 3, l.size), top - rng.integers(0, 3, r.size)
    rows = np.repeat(np.arange(31), np.diff(m.indptr))
    keep = (m.indices == 0) | (m.indices == 1)
    l[keep], r[keep] = top, top                                           # c_01 = 2^48 31
    assert top * top * 31 < 2 ** 53 <= top * top * 32 and rows.size == l.size
    return m, l, r, a, b, h


def fma_sensitive():
    """one user of items 0, 1, 2, all operands 1: c_01 = c_02 = 1.  a_0 = 3, b_1 = 1 + 3 u, b_2 = 1 + 2 u, h = u (u = 2^-52): with
    the definition's two roundings a_0 b_1 + h == a_0 b_2 + h, the keys tie and item 1 comes first; ONE rounding of the exact a_0 b_1
    + h (a fused multiply-add) is larger, and item 2 would come first"""
    u = 2.0 ** -52
    a, b, h = np.array([3.0, 1.0, 1.0]), np.array([1.0, 1 + 3 * u, 1 + 2 * u]), u
    assert a[0] * b[1] + h == a[0] * b[2] + h
    fused = [float(Fraction(a[0]) * Fraction(b[j]) + Fraction(h)) for j in (1, 2)]
    assert fused[0] > fused[1] == a[0] * b[2] + h
    m = canonical_pattern(sp.csr_matrix(np.ones((1, 3))))
    return m, np.ones(3, dtype=np.int64), np.ones(3, dtype=np.int64), a, b, h


PROBLEMS = {"planted": planted, "planted_h": lambda: planted(h=3.0), "one": lambda: small(1), "two": lambda: small(2), "seven": lambda: small(7),
            "sixty_five": lambda: small(65), "dense_varied": dense_varied, "dense_equal": dense_equal, "wide": wide_sums, "fma": fma_sensitive}


@functools.lru_cache(maxsize=None)
def problem(name):
    return PROBLEMS[name]()


@functools.lru_cache(maxsize=None)
def full_reference(name):
    m, l, r, a, b, h = problem(name)
    return weighted_cooccurrence_reference(m.indptr, m.indices, l, r, m.shape[1], a, b, h, _lib.KNN_MAX_NEIGHBORS)


def reference(name, K):
    """computed once per problem, at the largest K: a list of K neighbours is the head of a longer one"""
    nb, sums = full_reference(name)
    return np.ascontiguousarray(nb[:, :K]), np.ascontiguousarray(sums[:, :K])


@functools.lru_cache(maxsize=None)
def on_device(name):
    be = backend()
    m, l, r, a, b, h = problem(name)
    rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
    order = np.argsort(m.indices, kind="stable")                           # item-major: users ascending within an item
    ip = np.concatenate([[0], np.cumsum(np.bincount(m.indices, minlength=m.shape[1]))])
    dev = lambda t, dt=torch.int32: be.to_device(t, dt)
    return (dev(ip), dev(rows[order]), dev(l[order], torch.int64), dev(m.indptr), dev(m.indices), dev(r, torch.int64), m.shape[0], m.shape[1],
            dev(a, torch.float64), dev(b, torch.float64), h)


def device_fit(name, K, **kw):
    ip, iu, il, up, uj, ur, n_users, n_items, a, b, h = on_device(name)
    nb, sums = backend().cooc_neighbors_weighted(ip, iu, il, up, uj, ur, n_users, n_items, a, b, h, K, **kw)
    torch.cuda.synchronize()
    return nb.cpu().numpy(), sums.cpu().numpy().view(np.uint64)


def check_fit(name, K, **kw):
    nb, sums = device_fit(name, K, **kw)
    ref = reference(name, K)
    assert nb.dtype == np.int32 and sums.dtype == np.uint64
    assert np.array_equal(nb, ref[0]) and np.array_equal(sums, ref[1])
    return nb, sums


# ---- fit -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (1, 50, 256))
def test_fit_planted(K):
    nb, sums = check_fit("planted", K)
    assert (nb[299] == -1).all() and (sums[299] == 0).all()               # a column without users
    assert sums.max() > 2 ** 32                                            # a 32-bit cell would have wrapped
    if K == 256:
        assert ((nb >= 0).sum(axis=1) == 256).any()                        # K = 256 where a row has more
        m, l, r, a, b, h = problem("planted")
        # identical users and weights: equal keys towards a third item, the smaller index first
        both = [row.tolist() for row in nb if 10 in row and 11 in row]
        assert len(both) > 50 and all(row.index(11) == row.index(10) + 1 for row in both)
        # identical users, different weights: ordered by key, either way round somewhere
        ahead = [row.tolist().index(12) < row.tolist().index(13) for row in nb if 12 in row and 13 in row]
        assert any(ahead) and not all(ahead)


def test_the_operands_are_not_interchangeable():
    m, l, r, a, b, h = problem("planted")
    swapped = weighted_cooccurrence_reference(m.indptr, m.indices, r, l, 300, a, b, h, 50)
    assert (swapped[0] != reference("planted", 50)[0]).any(axis=1).sum() > 10 and (l != r).any()


@pytest.mark.parametrize("name,K", [("one", 1), ("one", 3), ("two", 1), ("two", 2), ("two", 5), ("sixty_five", 1), ("sixty_five", 64),
                                    ("sixty_five", 70), ("sixty_five", 256)])
def test_fit_small_shapes(name, K):
    nb, _ = check_fit(name, K)
    n_items = nb.shape[0]
    assert ((nb >= 0).sum(axis=1) == min(K, n_items - 1)).all()           # (user 0 holds every item) the rest is padding


def test_fit_h_enters_the_key():
    free, shrunk = reference("planted", 50), reference("planted_h", 50)
    assert (free[0] != shrunk[0]).any(axis=1).sum() > 10                   # the two orders differ
    check_fit("planted_h", 50)
    check_fit("planted", 50)


def test_fit_key_takes_the_three_roundings_of_the_definition():
    nb, sums = check_fit("fma", 2)
    assert nb[0].tolist() == [1, 2] and sums[0].tolist() == [1, 1]         # a contracted a b + h would give [2, 1]


def test_fit_sums_up_to_2_53():
    nb, sums = check_fit("wide", 4)
    assert int(sums.max()) == 2 ** 48 * 31 and (sums[:4, :3] > 2 ** 32).all()
    assert any(int(c) % 2 for c in sums.ravel() if c > 2 ** 52)            # odd integers above 2^52: no bit to spare


def test_fit_dense_rows_take_the_fallback_select():
    nb, sums = check_fit("dense_varied", 256)
    assert (nb >= 0).all() and len(np.unique(sums)) > 1000
    check_fit("dense_varied", 3)


def test_fit_dense_rows_of_one_key_take_the_tie_pass():
    nb, sums = check_fit("dense_equal", 256)
    lone = np.flatnonzero((sums == 1).all(axis=1))                         # items of user 0 alone: every cell 1, every key equal
    assert lone.size > 1000
    for i in lone[:5]:
        assert nb[i].tolist() == [j for j in range(258) if j != i][:256]
    check_fit("dense_equal", 7)


@pytest.mark.parametrize("ws_rows", (1, 2, 3))
def test_fit_in_batches_of_rows(ws_rows):
    check_fit("seven", 4, ws_rows=ws_rows)                                # 7 rows: a partial last batch, rows reused across batches
    if ws_rows == 3:
        check_fit("planted", 50, ws_rows=64)


def test_fit_of_an_item_range_is_the_slice():
    ref = reference("planted", 50)
    nb, sums = device_fit("planted", 50, item0=20, item1=47, ws_rows=5)
    assert np.array_equal(nb, ref[0][20:47]) and np.array_equal(sums, ref[1][20:47])
    nb, sums = device_fit("planted", 50, item0=295, item1=300)
    assert np.array_equal(nb, ref[0][295:]) and np.array_equal(sums, ref[1][295:])
    assert device_fit("planted", 50, item0=33, item1=33)[0].shape == (0, 50)


def test_fit_repeats_its_bits_and_reads_no_stale_workspace():
    a = device_fit("planted", 256)
    b = device_fit("planted", 256)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    check_fit("seven", 4)                                                  # a small call after a larger one: its own result
    check_fit("two", 2)


# ---- predict -------------------------------------------------------------------------------------------------------------------------
def device_lists(x, nb, q, k, nr=None, excl=(), ws_rows=0, xv=None):
    be = backend()
    m = canonical_pattern(x)
    dev = lambda a, t=torch.int32: be.to_device(a, t)
    nr_p = nr_j = None
    if nr is not None:
        nr = sp.csr_matrix(nr)
        nr.sort_indices()
        nr_p, nr_j = dev(nr.indptr), dev(nr.indices)
    d_ex = dev(np.asarray(excl, dtype=np.int32)) if len(excl) else None
    res, sc = be.knn_recommend(dev(m.indptr), dev(m.indices), dev(nb), dev(q, torch.int64), k, nr_p, nr_j, d_ex, ws_rows=ws_rows,
                               xv=None if xv is None else dev(xv, torch.int64))
    torch.cuda.synchronize()
    res = res.cpu().numpy().astype(np.int64)
    return np.where(res == -2147483648, -1, res - 1), sc.cpu().numpy()


def check_lists(x, nb, q, k, nr=None, excl=(), ws_rows=0, xv=None):
    got = device_lists(x, nb, q, k, nr, excl, ws_rows, xv)
    ref = knn_recommend_reference(x, nb, q, k, nr, excl, xv=xv)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    return got


@functools.lru_cache(maxsize=None)
def tables(K=8):
    """a table over 65 items with shared neighbours, ties among the weights and -1 slots"""
    rng = np.random.default_rng(21)
    nb = np.stack([rng.permutation(65)[:K] for _ in range(65)]).astype(np.int32)
    nb[6] = nb[4][::-1]                                                    # items 4 and 6 share every neighbour
    nb[9, 5:] = -1
    q = rng.integers(1, 2 ** 30 + 1, (65, K))
    q[:, 1] = q[:, 0]
    q[nb < 0] = 0
    q[3, 0] = 2 ** 30
    return nb, q


def users():
    """40 histories over 65 items: user 0 holds every item, user 1 none, user 2 the items 4 and 6, user 3 the items 3 and 9; weights
    of 1 and of 2^16 - 1 within one row"""
    rng = np.random.default_rng(22)
    d = rng.random((40, 65)) < 0.3
    d[0], d[1], d[2], d[3] = True, False, False, False
    d[2, [4, 6]] = True
    d[3, [3, 9]] = True
    x = canonical_pattern(sp.csr_matrix(d.astype(np.float64)))
    xv = rng.choice(np.array([1, 2, 77, TOP16 - 1, TOP16]), size=x.nnz)
    xv[x.indptr[2]:x.indptr[3]] = (1, TOP16)
    xv[x.indptr[3]:x.indptr[4]] = (TOP16, TOP16)
    return x, xv


@pytest.mark.parametrize("ws_rows", (0, 1, 2, 3))
def test_predict_weighted_lists(ws_rows):
    nb, q = tables()
    x, xv = users()
    items, scores = check_lists(x, nb, q, 10, x, (), ws_rows, xv)
    assert (items[0] == -1).all()                                          # every item is the user's own: nothing admissible
    assert np.array_equal(items[1], np.arange(10)) and (scores[1] == 0).all()   # no history: the first k items, score 0
    check_lists(x, nb, q, 10, None, (0, 5, 64), ws_rows, xv)
    check_lists(x, nb, q, 70, x, (2,), ws_rows, xv)                       # k above the admissible items
    check_lists(x, nb, q, 1, None, (), ws_rows, xv)


def test_predict_multiplies_by_the_row_weights():
    nb, q = tables()
    x, xv = users()
    items, scores = check_lists(x, nb, q, 65, None, (), 0, xv)
    j = nb[4][0]                                                           # a neighbour items 4 and 6 share: 1 q + (2^16 - 1) q'
    assert scores[2][items[2] == j][0] == 1 * q[4][nb[4] == j][0] + TOP16 * q[6][nb[6] == j][0]
    assert scores[3].max() >= TOP16 * 2 ** 30                              # the largest weight times the largest q
    assert any(len(np.unique(s[s > 0])) < (s > 0).sum() for s in scores)   # tied scores among the ranked
    ones = device_lists(x, nb, q, 10, x, (), 0, np.ones(x.nnz, dtype=np.int64))
    plain = device_lists(x, nb, q, 10, x)                                  # xv = None: the unweighted entry
    assert np.array_equal(ones[0], plain[0]) and np.array_equal(ones[1], plain[1])
    assert (check_lists(x, nb, q, 10, x, (), 0, xv)[1] != plain[1]).any()


def test_predict_a_weighted_row_beyond_the_candidate_buffer():
    rng = np.random.default_rng(3)
    n_items, K = CAND + 100, 4
    nb = ((np.arange(n_items)[:, None] + 1 + np.arange(K)[None, :]) % n_items).astype(np.int32)
    nb[5, 2] = -1
    q = rng.integers(1, 2 ** 30 + 1, size=(n_items, K))
    q[:, 3] = q[:, 0]                                                      # ties
    d = np.zeros((3, n_items))
    d[0] = 1                                                               # every item scored: more than the buffer holds
    d[1, :10] = 1
    x = canonical_pattern(sp.csr_matrix(d))
    xv = rng.integers(1, TOP16 + 1, x.nnz)
    xv[:200] = TOP16
    assert xv.sum() < 2 ** 31
    for k in (10, 1024):
        items, scores = check_lists(x, nb, q, k, xv=xv)
        assert (items >= 0).all() and scores.max() > 2 ** 46
    check_lists(x, nb, q, 100, x, tuple(range(0, n_items, 3)), xv=xv)


def test_predict_repeats_its_bits_and_shares_the_workspace_with_the_fits():
    nb, q = tables()
    x, xv = users()
    a = device_lists(x, nb, q, 10, x, xv=xv)
    check_fit("sixty_five", 64)                                            # a weighted fit in between: cells of the same width
    b = device_lists(x, nb, q, 10, x, xv=xv)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def interactions():
    rng = np.random.default_rng(31)
    d = planted_pattern() * rng.integers(1, 6, (160, 300))
    return sp.csr_matrix(d.astype(np.float64))


def test_binary_model_is_the_same_before_and_after_a_weighted_one():
    x = interactions()
    be = backend()

    def binary():
        m = ItemKNN(k_neighbors=20, similarity="jaccard", backend=be).fit(x, ws_rows=7)
        top = m.predict(x, 10, ws_rows=3)
        return m.neighbors, m.counts, np.asarray(top), top.scores

    before = binary()
    w = ItemKNN(k_neighbors=20, similarity="rp3beta", weighting="values", alpha=0.8, beta=0.3, backend=be).fit(x, ws_rows=5)
    w.predict(x, 10, ws_rows=2)
    after = binary()
    for s, t in zip(before, after):
        assert np.array_equal(s, t, equal_nan=True)
    from rsparse_amd.itemknn import cooccurrence_reference
    ref = cooccurrence_reference(x, 20, "jaccard")
    assert np.array_equal(after[0], ref[0]) and np.array_equal(after[1], ref[1])


@pytest.mark.parametrize("sim,kw", [("dot", {"weighting": "values"}), ("cosine", {"weighting": "values", "shrinkage": 5.0}),
                                    ("asymmetric", {"weighting": "values", "alpha": 0.3}), ("rp3beta", {"weighting": "values", "alpha": 0.7, "beta": 0.4}),
                                    ("rp3beta", {})])
def test_model_equals_the_cpu_stand_in(sim, kw):
    from oracle_backend import OracleBackend
    x = interactions()
    m = ItemKNN(k_neighbors=20, similarity=sim, backend=backend(), **kw).fit(x)
    host = ItemKNN(k_neighbors=20, similarity=sim, backend=OracleBackend(), **kw).fit(x)
    assert np.array_equal(m.neighbors, host.neighbors) and np.array_equal(m.sums, host.sums) and m.sums.dtype == np.uint64
    assert np.array_equal(m.similarities, host.similarities, equal_nan=True) and np.array_equal(m.item_count, host.item_count)
    top, ref = m.predict(x, 10, items_exclude=(7, 8)), host.predict(x, 10, items_exclude=(7, 8))
    assert np.array_equal(np.asarray(top), np.asarray(ref)) and np.array_equal(top.scores, ref.scores, equal_nan=True)
    alone = m.predict(x[4], 10, items_exclude=(7, 8))                      # a list depends neither on the batch nor on the other rows
    assert np.array_equal(np.asarray(alone)[0], np.asarray(top)[4]) and np.array_equal(alone.scores[0], top.scores[4], equal_nan=True)


def test_bm25_cosine_end_to_end_equals_the_cpu_stand_in():
    """fit, predict and evaluate with device-side BM25 weights against the same model on the CPU stand-in.  Everything that is this
    model's is compared exactly: the table, the lists, and the metrics that are ratios of integers.  The weights themselves come
    from two implementations of BM25 (device log / log1p against numpy's, tests/test_confidence.py: rtol 8 u), so the float64
    `.scores`, which divide by the scale 65535 / max(w), agree to that rounding; ap and ndcg are float sums that the metric kernel
    and the stand-in's numpy reference add in different orders (tests/test_metrics.py compares them at 1e-12), so they are compared
    exactly with the metric kernel on the stand-in's lists, and at 1e-12 with the stand-in's own figures."""
    from rsparse_amd.metrics import ranking_metrics
    from test_metrics_abi import _oracle_metrics_backend
    x = interactions()
    rng = np.random.default_rng(5)
    held = sp.csr_matrix((rng.random(x.shape) < 0.05) * (x.toarray() == 0) * rng.integers(1, 4, x.shape).astype(np.float64))
    exact = ("precision", "recall", "hit", "mrr", "coverage", "popularity")
    cut = (3, 10)
    out = []
    for be in (backend(), _oracle_metrics_backend()):
        m = ItemKNN(k_neighbors=20, similarity="cosine", weighting=Confidence("bm25"), backend=be).fit(x)
        out.append((m, m.evaluate(x, held, cut, metrics=("ap", "ndcg") + exact), m.predict(x, 10)))
    (m, ev, top), (host, ref, top_ref) = out
    assert np.array_equal(m.neighbors, host.neighbors) and np.array_equal(m.sums, host.sums)
    assert np.array_equal(np.asarray(top), np.asarray(top_ref))
    live = np.asarray(top) >= 0
    print("scores: largest relative difference %.3e" % np.abs(top.scores[live] / top_ref.scores[live] - 1).max())
    np.testing.assert_allclose(top.scores[live], top_ref.scores[live], rtol=1e-13, atol=0)
    for name in exact:
        assert np.array_equal(ev[name], ref[name], equal_nan=True), name
    for t, c in enumerate(cut):
        ap, ndcg = ranking_metrics(np.asarray(top_ref)[:, :c], held)
        assert np.array_equal(ev["ap"][:, t], ap, equal_nan=True) and np.array_equal(ev["ndcg"][:, t], ndcg, equal_nan=True)
    for name in ("ap", "ndcg"):
        fin = np.isfinite(ref[name])
        assert np.array_equal(np.isnan(ev[name]), np.isnan(ref[name]))
        err = np.abs(ev[name][fin] - ref[name][fin])
        print("%s: largest difference from the stand-in %.3e" % (name, err.max()))
        assert err.max() <= 1e-12
    assert np.nanmax(ev["ndcg"]) > 0
