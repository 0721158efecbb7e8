"""ItemKNN without a GPU: the two numpy definitions (rsparse_amd/itemknn.py) against brute-force dense numpy on a tiny matrix,
and the class on the CPU stand-in, where it runs those definitions.

Also home of the problems tests/test_itemknn.py checks the kernels with."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle_backend import OracleBackend
from rsparse_amd import ItemKNN, _lib
from rsparse_amd.itemknn import (Q_ONE, cooccurrence_reference, knn_recommend_reference, similarity_values, weight_table)

SIMS = ("cosine", "jaccard", "count")


def tiny():
    """12 users x 9 items of rising popularity (the three orders differ): item 8 has no user, items 2 and 3 the same users, a
    duplicate and an explicit zero among the entries"""
    rng = np.random.default_rng(4)
    d = (rng.random((12, 9)) < np.linspace(0.2, 0.9, 9)[None, :]).astype(float)
    d[:, 8] = 0
    d[:, 3] = d[:, 2]
    d[0, :] = 0          # an empty history row
    m = sp.coo_matrix(d)
    rows, cols, vals = list(m.row), list(m.col), list(m.data)
    rows += [1, 5]       # (1, 7) twice: summed; (5, 8) an explicit zero: eliminated
    cols += [7, 8]
    vals += [1.0, 0.0]
    d[1, 7] = 1
    return sp.csr_matrix(sp.coo_matrix((vals, (rows, cols)), shape=d.shape)), (d != 0).astype(np.int64)


def brute_fit(b, K, sim):
    """the definition through the dense items x items product"""
    n_items = b.shape[1]
    c = b.T @ b
    n = np.diag(c).copy()
    nb = np.full((n_items, K), -1, dtype=np.int32)
    ct = np.zeros((n_items, K), dtype=np.int32)
    for i in range(n_items):
        cand = []
        for j in range(n_items):
            if j == i or c[i, j] == 0:
                continue
            cij = int(c[i, j])
            num, den = {"count": (cij, 1), "cosine": (cij * cij, int(n[i]) * int(n[j])), "jaccard": (cij, int(n[i]) + int(n[j]) - cij)}[sim]
            cand.append((-(np.float64(num) / np.float64(den)), j, cij))
        cand.sort()
        for s, (_, j, cij) in enumerate(cand[:K]):
            nb[i, s], ct[i, s] = j, cij
    return nb, ct, n


def brute_predict(b, nb, q, k, nr, excl):
    n_users, n_items = b.shape
    items = np.full((n_users, k), -1, dtype=np.int64)
    scores = np.zeros((n_users, k), dtype=np.int64)
    for u in range(n_users):
        score = [0] * n_items
        for i in np.flatnonzero(b[u]):
            for s in range(nb.shape[1]):
                if nb[i, s] >= 0:
                    score[nb[i, s]] += int(q[i, s])
        cand = sorted((-score[j], j) for j in range(n_items) if j not in excl and (nr is None or not nr[u, j]))
        for t, (neg, j) in enumerate(cand[:k]):
            items[u, t], scores[u, t] = j, -neg
    return items, scores


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("K", (1, 3, 8, 12))
def test_fit_reference_is_the_dense_definition(sim, K):
    x, b = tiny()
    nb, ct, n = cooccurrence_reference(x, K, sim)
    rb, rc, rn = brute_fit(b, K, sim)
    assert nb.dtype == np.int32 and ct.dtype == np.int32
    assert np.array_equal(nb, rb) and np.array_equal(ct, rc) and np.array_equal(n, rn)
    assert (nb[8] == -1).all() and (ct[8] == 0).all()                   # no user: no neighbour
    if K >= 3:
        assert nb[2, 0] == 3 and nb[3, 0] == 2                             # identical columns are each other's best


def test_the_three_orders_differ_on_the_tiny_matrix():
    x, _ = tiny()
    tables = [cooccurrence_reference(x, 8, sim)[0] for sim in SIMS]
    assert not np.array_equal(tables[0], tables[1]) and not np.array_equal(tables[0], tables[2])
    assert not np.array_equal(tables[1], tables[2])


@pytest.mark.parametrize("sim", SIMS)
def test_predict_reference_is_the_dense_definition(sim):
    x, b = tiny()
    nb, ct, n = cooccurrence_reference(x, 3, sim)
    q = weight_table(nb, ct, n, sim)
    assert q.max() <= Q_ONE or sim == "count"
    for k, nr, excl in ((4, b, ()), (9, None, ()), (12, b, (1, 4)), (2, None, (0,))):
        got = knn_recommend_reference(x, nb, q, k, None if nr is None else sp.csr_matrix(nr), excl)
        ref = brute_predict(b, nb, q, k, nr, set(excl))
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_similarity_values_and_weights():
    x, _ = tiny()
    nb, ct, n = cooccurrence_reference(x, 8, "cosine")
    sim = similarity_values(nb, ct, n, "cosine")
    pad = nb < 0
    assert np.isnan(sim[pad]).all() and (sim[~pad] > 0).all() and (sim[~pad] <= 1).all()
    assert sim[2, 0] == 1.0                                                # identical columns
    i, s = np.argwhere(~pad)[5]
    assert sim[i, s] == np.sqrt(np.float64(int(ct[i, s]) ** 2) / np.float64(int(n[i]) * int(n[nb[i, s]])))
    q = weight_table(nb, ct, n, "cosine")
    assert q.dtype == np.int64 and (q[pad] == 0).all() and np.array_equal(q[~pad], np.rint(sim[~pad] * 2.0 ** 30).astype(np.int64))
    assert np.array_equal(weight_table(nb, ct, n, "count"), ct)


# ---- the class on the CPU stand-in -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    x, b = tiny()
    return {sim: ItemKNN(k_neighbors=4, similarity=sim, backend=OracleBackend()).fit(x) for sim in SIMS}, x, b


@pytest.mark.parametrize("sim", SIMS)
def test_fit_sets_the_tables(fitted, sim):
    models, x, b = fitted
    m = models[sim]
    nb, ct, n = cooccurrence_reference(x, 4, sim)
    assert np.array_equal(m.neighbors, nb) and np.array_equal(m.counts, ct) and np.array_equal(m.item_count, b.sum(axis=0))
    assert m.similarities.dtype == np.float64 and np.array_equal(np.isnan(m.similarities), nb < 0)   # padding
    top = m.similar_items([2, 8], k=3)
    assert np.array_equal(np.asarray(top), nb[[2, 8], :3]) and (np.asarray(top)[1] == -1).all()
    assert np.array_equal(top.scores, m.similarities[[2, 8], :3], equal_nan=True)
    assert m.similar_items(k=4).shape == (9, 4)


@pytest.mark.parametrize("sim", SIMS)
def test_predict_conventions(fitted, sim):
    models, x, b = fitted
    m = models[sim]
    q = weight_table(m.neighbors, m.counts, m.item_count, sim)
    unit = 1.0 if sim == "count" else 2.0 ** 30
    top = m.predict(x, 4)                                                  # not_recommend = x
    ref = knn_recommend_reference(x, m.neighbors, q, 4, x)
    assert np.array_equal(np.asarray(top), ref[0])
    assert np.array_equal(top.scores, np.where(ref[0] < 0, np.nan, ref[1] / unit), equal_nan=True)
    for u in range(12):
        assert not set(np.asarray(top)[u]) & set(np.flatnonzero(b[u]))
    # an empty history row: the first k admissible items in ascending order, all of score 0
    assert np.array_equal(np.asarray(top)[0], [0, 1, 2, 3]) and (top.scores[0] == 0).all()
    top = m.predict(x, 4, items_exclude=(0, 2))
    assert np.array_equal(np.asarray(top)[0], [1, 3, 4, 5]) and not np.isin(np.asarray(top), (0, 2)).any()
    # k above the admissible items: -1 / NaN behind them
    top = m.predict(x, 12, not_recommend=None, items_exclude=(7,))
    assert (np.asarray(top)[:, :8] >= 0).all() and (np.asarray(top)[:, 8:] == -1).all()
    assert np.isnan(top.scores[:, 8:]).all() and not np.isnan(top.scores[:, :8]).any()
    ref = knn_recommend_reference(x, m.neighbors, q, 12, None, (7,))
    assert np.array_equal(np.asarray(top), ref[0])
    top = m.predict(x, 9)
    assert np.array_equal((np.asarray(top) >= 0).sum(axis=1), 9 - b.sum(axis=1))


def test_evaluate_equals_the_metrics_of_predict(fitted):
    from rsparse_amd.metrics import hit_metrics_reference, list_metrics_reference, self_information
    from test_metrics_abi import _oracle_metrics_backend, ref_metrics
    models, x, b = fitted
    m = ItemKNN(k_neighbors=4, similarity="cosine", backend=_oracle_metrics_backend()).fit(x)
    held = sp.csr_matrix((np.random.default_rng(2).random(b.shape) < 0.3) * (1 - b) * 2.0)
    cut = (2, 5)
    ev = m.evaluate(x, held, cut, metrics=("ap", "ndcg", "precision", "recall", "hit", "mrr", "coverage", "popularity", "novelty"))
    top = np.asarray(m.predict(x, 5))
    one = np.where(top < 0, -2147483648, top + 1).astype(np.int32)
    for t, c in enumerate(cut):
        ap, ndcg = ref_metrics(one[:, :c], held)
        assert np.array_equal(ev["ap"][:, t], ap, equal_nan=True) and np.array_equal(ev["ndcg"][:, t], ndcg, equal_nan=True)
    hits = hit_metrics_reference(top, held, cut, 9)
    for name in ("precision", "recall", "hit", "mrr", "coverage"):
        assert np.array_equal(ev[name], hits[name], equal_nan=True), name
    lists = list_metrics_reference(top, cut, 9, m.item_count.astype(np.int32), self_information(m.item_count))
    for name in ("popularity", "novelty"):
        assert np.array_equal(ev[name], lists[name], equal_nan=True), name
    one_k = m.evaluate(x, held, 5, metrics=("ap", "coverage"))
    assert np.array_equal(one_k["ap"], ev["ap"][:, 1], equal_nan=True) and one_k["coverage"] == ev["coverage"][1]


def test_argument_errors():
    x, _ = tiny()
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            ItemKNN(k_neighbors=bad)
    with pytest.raises(_lib.UnsupportedOnDevice):
        ItemKNN(k_neighbors=257)
    with pytest.raises(ValueError):
        ItemKNN(similarity="pearson")
    m = ItemKNN(k_neighbors=3, backend=OracleBackend())
    with pytest.raises(RuntimeError):
        m.predict(x, 3)
    with pytest.raises(RuntimeError):
        m.similar_items()
    with pytest.raises(TypeError):
        m.fit(x.toarray())
    m.fit(x)
    with pytest.raises(ValueError):
        m.predict(x[:, :5], 3)                                             # another number of items
    with pytest.raises(ValueError):
        m.predict(x, 0)
    with pytest.raises(_lib.UnsupportedOnDevice):
        m.predict(x, 1025)
    with pytest.raises(ValueError):
        m.predict(x, 3, items_exclude=(9,))
    with pytest.raises(TypeError):
        m.predict(x, 3, not_recommend=x.toarray())
    with pytest.raises(ValueError):
        m.predict(x, 3, not_recommend=x[:5])
    with pytest.raises(ValueError):
        m.similar_items(k=4)
    with pytest.raises(ValueError):
        m.similar_items([9])
    with pytest.raises(ValueError):
        m.evaluate(x, x, 3, metrics=("auc",))
    with pytest.raises(ValueError):
        m.evaluate(x, x[:5], 3)
