"""The ItemKNN kernels (wrmf_itemknn.hip) against the numpy definitions of rsparse_amd/itemknn.py: every comparison is
np.array_equal -- the feature is integer from end to end, there is no tolerance.  The shapes sit where the kernels change course:
the span a wave takes of the stored entries, the lane group's share of an inner list, the LDS candidate buffer of the select (and
the radix fallback beyond it), batches of one, two and three dense rows."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import ItemKNN, _lib
from rsparse_amd.itemknn import SIMILARITIES, canonical_pattern, cooccurrence_reference, knn_recommend_reference, weight_table

pytestmark = pytest.mark.gpu

SIMS = ("cosine", "jaccard", "count")
SPAN, CAND = _lib.KNN_SPAN, _lib.KNN_LDS_CAND


@functools.lru_cache(maxsize=None)
def backend():
    from rsparse_amd.engine import HipBackend
    return HipBackend()


# ---- the problems ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted():
    """160 users x 300 items of rising popularity.  Rows of 1, 63, 64, 65 and 257 items (users 0 .. 4); columns of 0, 1, 64, 65 and
    2 SPAN + 1 users (items 299 .. 295); items 10 and 11 with the same users."""
    rng = np.random.default_rng(7)
    n_users, n_items = 160, 300
    d = rng.random((n_users, n_items)) < np.linspace(0.02, 0.25, n_items)[None, :]
    d[:, 11] = d[:, 10]
    free = np.setdiff1d(np.arange(295), (10, 11))
    d[:5] = False
    for u, length in enumerate((1, 63, 64, 65, 257)):
        d[u, rng.choice(free, size=length, replace=False)] = True
    for item, users in ((299, 0), (298, 1), (297, 64), (296, 65), (295, 2 * SPAN + 1)):
        d[:, item] = False
        d[5 + rng.choice(n_users - 5, size=users, replace=False), item] = True
    assert d[:5].sum(axis=1).tolist() == [1, 63, 64, 65, 257]
    assert d[:, 295:].sum(axis=0).tolist() == [2 * SPAN + 1, 65, 64, 1, 0] and (d[:, 10] == d[:, 11]).all() and d[:, 10].any()
    return sp.csr_matrix(d.astype(np.float64))


@functools.lru_cache(maxsize=None)
def small(n_items):
    rng = np.random.default_rng(100 + n_items)
    d = rng.random((40, n_items)) < np.linspace(0.1, 0.6, n_items)[None, :]
    d[0] = True                                                           # a user of every item: each item has n_items - 1 neighbours
    return sp.csr_matrix(d.astype(np.float64))


@functools.lru_cache(maxsize=None)
def dense_rows():
    """one user holds all CAND + 100 items: every dense row has more cells than the candidate buffer; two more users vary the keys"""
    rng = np.random.default_rng(9)
    n_items = CAND + 100
    d = np.zeros((3, n_items), dtype=bool)
    d[0] = True
    d[1, rng.choice(n_items, size=2000, replace=False)] = True
    d[2, rng.choice(n_items, size=50, replace=False)] = True
    return sp.csr_matrix(d.astype(np.float64))


@functools.lru_cache(maxsize=None)
def dense_varied():
    """the same with a dozen users of half the catalogue each: rows beyond the buffer whose keys take many values, so that the
    radix select can stop before its last byte"""
    rng = np.random.default_rng(10)
    n_items = CAND + 100
    d = rng.random((7, n_items)) < 0.5
    d[0] = True
    return sp.csr_matrix(d.astype(np.float64))


PROBLEMS = {"planted": planted, "dense_varied": dense_varied, "one": lambda: small(1), "two": lambda: small(2), "seven": lambda: small(7), "sixty_five": lambda: small(65),
            "dense": dense_rows}


@functools.lru_cache(maxsize=None)
def reference(name, K, sim):
    return cooccurrence_reference(PROBLEMS[name](), K, sim)


@functools.lru_cache(maxsize=None)
def on_device(name):
    """both orientations of a problem on the device: (ip, iu, up, uj, n_users, n_items)"""
    be = backend()
    m = canonical_pattern(PROBLEMS[name]())
    t = m.tocsc()
    t.sort_indices()
    dev = lambda a: be.to_device(a, torch.int32)
    return dev(t.indptr), dev(t.indices), dev(m.indptr), dev(m.indices), m.shape[0], m.shape[1]


def device_fit(name, K, sim, **kw):
    ip, iu, up, uj, n_users, n_items = on_device(name)
    nb, ct = backend().cooc_neighbors(ip, iu, up, uj, n_users, n_items, SIMILARITIES[sim], K, **kw)
    torch.cuda.synchronize()
    return nb.cpu().numpy(), ct.cpu().numpy()


def check_fit(name, K, sim, **kw):
    nb, ct = device_fit(name, K, sim, **kw)
    ref = reference(name, K, sim)
    assert nb.dtype == np.int32 and ct.dtype == np.int32
    assert np.array_equal(nb, ref[0]) and np.array_equal(ct, ref[1])
    return nb, ct


# ---- fit -----------------------------------------------------------------------------------------------------------------------------
def test_the_three_orders_differ_on_the_planted_matrix():
    tables = [reference("planted", 50, sim)[0] for sim in SIMS]
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert (tables[a] != tables[b]).any(axis=1).sum() > 10
    full = reference("planted", 256, "cosine")[0]
    assert ((full >= 0).sum(axis=1) == 256).any()                          # K = 256 with more than 256 co-occurring items ...
    m = canonical_pattern(planted())
    c = (m.T @ m).toarray()
    np.fill_diagonal(c, 0)
    assert ((c > 0).sum(axis=1) > 256).any()                               # ... in some row


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("K", (1, 50, 256))
def test_fit_planted(K, sim):
    nb, ct = check_fit("planted", K, sim)
    assert (nb[299] == -1).all() and (ct[299] == 0).all()                 # a column without users
    if K >= 50:
        assert nb[10, 0] == 11 and nb[11, 0] == 10 or sim == "count"      # identical columns: each other's best by cosine / Jaccard


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("name,K", [("one", 1), ("one", 3), ("two", 1), ("two", 2), ("two", 5), ("sixty_five", 1), ("sixty_five", 64),
                                    ("sixty_five", 70), ("sixty_five", 256)])
def test_fit_small_shapes(name, K, sim):
    nb, _ = check_fit(name, K, sim)
    n_items = nb.shape[0]
    assert ((nb >= 0).sum(axis=1) == min(K, n_items - 1)).all()           # (user 0 holds every item) the rest is padding


def test_fit_ties_go_to_the_smaller_index():
    # identical columns everywhere: 5 users hold all of 9 items, every key is the same
    x = sp.csr_matrix(np.ones((5, 9)))
    be = backend()
    m = ItemKNN(k_neighbors=4, similarity="cosine", backend=be).fit(x)
    want = np.array([[j for j in range(9) if j != i][:4] for i in range(9)])
    assert np.array_equal(m.neighbors, want) and (m.counts == 5).all() and (m.similarities == 1.0).all()


def test_fit_dense_rows_take_the_fallback_select():
    nb, ct = check_fit("dense", 256, "cosine")
    assert (nb >= 0).all() and len(np.unique(ct)) > 1
    check_fit("dense", 3, "count")
    for sim, K in (("cosine", 256), ("jaccard", 50)):
        nb, ct = check_fit("dense_varied", K, sim)
        assert (nb >= 0).all()
    assert len(np.unique(reference("dense_varied", 256, "cosine")[1])) > 4


@pytest.mark.parametrize("ws_rows", (1, 2, 3))
def test_fit_in_batches_of_rows(ws_rows):
    for sim in SIMS:
        check_fit("seven", 4, sim, ws_rows=ws_rows)                       # 7 rows: a partial last batch, rows reused across batches
    check_fit("planted", 50, "jaccard", ws_rows=64)


def test_fit_of_an_item_range_is_the_slice():
    for sim in SIMS:
        nb, ct = device_fit("planted", 50, sim, item0=20, item1=47, ws_rows=5)
        ref = reference("planted", 50, sim)
        assert np.array_equal(nb, ref[0][20:47]) and np.array_equal(ct, ref[1][20:47])
    nb, ct = device_fit("planted", 50, "cosine", item0=295, item1=300)
    assert np.array_equal(nb, reference("planted", 50, "cosine")[0][295:])
    assert device_fit("planted", 50, "cosine", item0=33, item1=33)[0].shape == (0, 50)


def test_fit_repeats_its_bits_and_reads_no_stale_workspace():
    a = device_fit("planted", 256, "cosine")
    b = device_fit("planted", 256, "cosine")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    check_fit("seven", 4, "cosine")                                        # a small call after a larger one: its own result
    check_fit("two", 2, "count")


def test_model_fit_on_the_device():
    x = planted()
    for sim in SIMS:
        m = ItemKNN(k_neighbors=50, similarity=sim, backend=backend()).fit(x)
        ref = reference("planted", 50, sim)
        assert np.array_equal(m.neighbors, ref[0]) and np.array_equal(m.counts, ref[1]) and np.array_equal(m.item_count, ref[2])


# ---- predict -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables(sim, K=8):
    nb, ct, n = reference("sixty_five", K, sim)
    return nb, weight_table(nb, ct, n, sim)


def device_lists(x, nb, q, k, nr=None, excl=(), ws_rows=0):
    be = backend()
    m = canonical_pattern(x)
    dev = lambda a, t=torch.int32: be.to_device(a, t)
    nr_p = nr_j = None
    if nr is not None:
        nr = sp.csr_matrix(nr)
        nr.sort_indices()
        nr_p, nr_j = dev(nr.indptr), dev(nr.indices)
    d_ex = dev(np.asarray(excl, dtype=np.int32)) if len(excl) else None
    res, sc = be.knn_recommend(dev(m.indptr), dev(m.indices), dev(nb), dev(q, torch.int64), k, nr_p, nr_j, d_ex, ws_rows=ws_rows)
    torch.cuda.synchronize()
    res = res.cpu().numpy().astype(np.int64)
    return np.where(res == -2147483648, -1, res - 1), sc.cpu().numpy()


def check_lists(x, nb, q, k, nr=None, excl=(), ws_rows=0):
    got = device_lists(x, nb, q, k, nr, excl, ws_rows)
    ref = knn_recommend_reference(x, nb, q, k, nr, excl)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    return got


def users():
    """40 histories over 65 items: user 0 holds every item, user 1 none, user 2 the items 4 and 6"""
    x = small(65).tolil()
    x[1] = 0
    x[2] = 0
    x[2, 4] = x[2, 6] = 1
    return x.tocsr()


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("ws_rows", (0, 1, 2))
def test_predict_lists(sim, ws_rows):
    nb, q = tables(sim)
    x = users()
    items, scores = check_lists(x, nb, q, 10, x, (), ws_rows)
    assert (items[0] == -1).all()                                          # every item is the user's own: nothing admissible
    assert np.array_equal(items[1], np.arange(10)) and (scores[1] == 0).all()   # no history: the first k items, score 0
    check_lists(x, nb, q, 10, None, (0, 5, 64), ws_rows)
    check_lists(x, nb, q, 70, x, (2,), ws_rows)                           # k above the admissible items
    check_lists(x, nb, q, 1, None, (), ws_rows)


def test_predict_sums_shared_neighbours_and_breaks_ties_by_index():
    nb, q = tables("count", 8)
    shared = np.intersect1d(nb[4][nb[4] >= 0], nb[6][nb[6] >= 0])
    assert shared.size                                                     # items 4 and 6 share a neighbour: the sum is exercised
    x = users()
    items, scores = check_lists(x, nb, q, 20, x)
    j = shared[0]
    assert scores[2][items[2] == j][0] == q[4][nb[4] == j][0] + q[6][nb[6] == j][0]
    assert any(len(np.unique(s[s > 0])) < (s > 0).sum() for s in scores)   # tied scores among the ranked
    # a table with empty slots: K above n_items - 1
    nb65, ct65, n65 = reference("sixty_five", 70, "cosine")
    assert (nb65 < 0).any()
    check_lists(x, nb65, weight_table(nb65, ct65, n65, "cosine"), 12, x)


def test_predict_a_row_beyond_the_candidate_buffer():
    rng = np.random.default_rng(3)
    n_items, K = CAND + 100, 4
    nb = ((np.arange(n_items)[:, None] + 1 + np.arange(K)[None, :]) % n_items).astype(np.int32)
    nb[5, 2] = -1
    q = rng.integers(1, 2 ** 30 + 1, size=(n_items, K))
    q[:, 3] = q[:, 0]                                                      # ties
    d = np.zeros((3, n_items))
    d[0] = 1                                                               # every item scored: more than the buffer holds
    d[1, :10] = 1
    x = sp.csr_matrix(d)
    for k in (10, 1024):
        items, _ = check_lists(x, nb, q, k)
        assert (items >= 0).all()
    check_lists(x, nb, q, 100, x, tuple(range(0, n_items, 3)))


def test_predict_repeats_its_bits_and_reads_no_stale_workspace():
    nb, q = tables("cosine")
    x = users()
    a = device_lists(x, nb, q, 10, x)
    test_predict_a_row_beyond_the_candidate_buffer()                       # a larger call in between
    b = device_lists(x, nb, q, 10, x)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    check_fit("seven", 4, "cosine")                                        # the two entries share the workspace
    check_lists(x[:3], nb, q, 5, x[:3])


def test_model_predict_and_evaluate_on_the_device():
    from rsparse_amd.metrics import ranking_metrics, topk_metrics
    from oracle_backend import OracleBackend
    x = planted()
    rng = np.random.default_rng(5)
    held = sp.csr_matrix((rng.random(x.shape) < 0.05) * (1.0 - x.toarray()) * rng.integers(1, 4, x.shape))
    for sim in SIMS:
        m = ItemKNN(k_neighbors=20, similarity=sim, backend=backend()).fit(x)
        host = ItemKNN(k_neighbors=20, similarity=sim, backend=OracleBackend()).fit(x)
        top, ref = m.predict(x, 10, items_exclude=(7, 8)), host.predict(x, 10, items_exclude=(7, 8))
        assert np.array_equal(np.asarray(top), np.asarray(ref)) and np.array_equal(top.scores, ref.scores, equal_nan=True)
    cut = (3, 10)
    ev = m.evaluate(x, held, cut, metrics=("ap", "ndcg", "precision", "recall", "hit", "mrr", "coverage", "popularity"))
    top = np.asarray(m.predict(x, 10))
    hits = topk_metrics(top, held, cut, metrics=("precision", "recall", "hit", "mrr", "coverage"), n_item=x.shape[1])
    for name in ("precision", "recall", "hit", "mrr", "coverage"):
        assert np.array_equal(ev[name], hits[name], equal_nan=True), name
    for t, c in enumerate(cut):
        ap, ndcg = ranking_metrics(top[:, :c], held)
        assert np.array_equal(ev["ap"][:, t], ap, equal_nan=True) and np.array_equal(ev["ndcg"][:, t], ndcg, equal_nan=True)
    assert ev["popularity"].shape == (x.shape[0], 2)
