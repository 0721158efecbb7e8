"""ItemKNN under the evaluation protocols without a GPU: the three numpy definitions (knn_score_pairs_reference,
knn_candidates_reference, knn_ranks_reference) against brute force on the tiny matrix of tests/test_itemknn_host.py, and the class
on the CPU stand-in, where it runs those definitions: candidates=, negatives=, score, held_out_ranks, evaluate_ranks."""
import numpy as np
import pytest
import scipy.sparse as sp

from rsparse_amd import Confidence, ItemKNN, WRMF
from rsparse_amd.itemknn import (Q_ONE, canonical_pattern, cooccurrence_reference, knn_candidates_reference, knn_ranks_reference,
                                 knn_recommend_reference, knn_score_pairs_reference, weight_table)
from rsparse_amd.metrics import rank_summary, rank_totals
from test_itemknn_host import brute_predict, tiny
from test_metrics_abi import _oracle_metrics_backend

METRICS = ("ap", "ndcg", "precision", "recall", "hit", "mrr", "coverage", "popularity", "novelty")


def tables(sim="cosine", K=4):
    x, b = tiny()
    nb, ct, n = cooccurrence_reference(x, K, sim)
    return x, b, nb, weight_table(nb, ct, n, sim)


def seen(b):
    """not_recommend for the brute-force comparisons: the pattern itself (x also stores a zero, which a filter would count)"""
    return sp.csr_matrix(b.astype(np.float64))


def dense_scores(b, nb, q, xv=None):
    """score_u[j] by its definition, in Python integers"""
    n_users, n_items = b.shape
    s = np.zeros((n_users, n_items), dtype=np.int64)
    e = 0
    for u in range(n_users):
        for i in np.flatnonzero(b[u]):
            w = 1 if xv is None else int(xv[e])
            e += 1
            for t in range(nb.shape[1]):
                if nb[i, t] >= 0:
                    s[u, nb[i, t]] += w * int(q[i, t])
    return s


# ---- the definitions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", (False, True))
def test_score_pairs_reference_is_the_dense_definition(weights):
    x, b, nb, q = tables()
    xv = np.arange(1, canonical_pattern(x).nnz + 1) if weights else None
    s = dense_scores(b, nb, q, xv)
    pairs = sp.csr_matrix(np.random.default_rng(1).random(b.shape) < 0.4)
    got = knn_score_pairs_reference(x, nb, q, pairs, xv)
    pat = canonical_pattern(pairs)
    assert got.dtype == np.int64 and np.array_equal(got, s[pat.nonzero()])
    assert (s[b != 0] > 0).any() and np.array_equal(knn_score_pairs_reference(x, nb, q, sp.csr_matrix(b), xv), s[b != 0])   # nothing is masked
    with pytest.raises(ValueError):
        knn_score_pairs_reference(x, nb, q, pairs[:5], xv)


@pytest.mark.parametrize("sim", ("cosine", "count"))
def test_candidates_reference_is_the_dense_definition(sim):
    x, b, nb, q = tables(sim)
    s = dense_scores(b, nb, q)
    d = np.random.default_rng(2).random(b.shape) < 0.6
    d[3] = False                                                            # a row without candidates
    d[4, :] = b[4] != 0                                                     # candidates that are all masked by not_recommend = x
    cand, excl = sp.csr_matrix(d), (1,)
    for k in (1, 3, 9):
        items, scores = knn_candidates_reference(x, nb, q, cand, k, seen(b), excl)
        for u in range(b.shape[0]):
            adm = [j for j in np.flatnonzero(d[u]) if not b[u, j] and j not in excl]
            want = sorted(adm, key=lambda j: (-s[u, j], j))[:k]
            assert items[u, :len(want)].tolist() == want and (items[u, len(want):] == -1).all()
            assert scores[u, :len(want)].tolist() == [s[u, j] for j in want] and (scores[u, len(want):] == 0).all()
        assert (items[3] == -1).all() and (items[4] == -1).all()
    # the user without a history: its candidates in ascending order, all of score 0
    items, scores = knn_candidates_reference(x, nb, q, cand, 9, seen(b), excl)
    adm0 = np.setdiff1d(np.flatnonzero(d[0]), excl)
    assert np.array_equal(items[0, :adm0.size], adm0) and (scores[0] == 0).all()


@pytest.mark.parametrize("sim", ("cosine", "jaccard", "count"))
def test_every_item_as_candidate_is_knn_recommend(sim):
    x, b, nb, q = tables(sim)
    every = sp.csr_matrix(np.ones(b.shape))
    for k, nr, excl in ((4, seen(b), ()), (9, None, (0, 2)), (12, seen(b), (7,))):
        a, c = knn_recommend_reference(x, nb, q, min(k, 9), nr, excl), knn_candidates_reference(x, nb, q, every, min(k, 9), nr, excl)
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
        ref = brute_predict(b, nb, q, min(k, 9), None if nr is None else b, excl)
        assert np.array_equal(c[0], ref[0]) and np.array_equal(c[1], ref[1])


def test_score_pairs_at_a_list_are_the_lists_scores():
    x, b, nb, q = tables()
    cand = sp.csr_matrix(np.random.default_rng(3).random(b.shape) < 0.7)
    items, scores = knn_candidates_reference(x, nb, q, cand, 5, x)
    for u in range(b.shape[0]):
        row = items[u][items[u] >= 0]
        listed = sp.csr_matrix((np.ones(row.size), (np.full(row.size, u), row)), shape=b.shape)
        got = knn_score_pairs_reference(x, nb, q, listed)
        assert np.array_equal(got, scores[u, :row.size][np.argsort(row)])


def test_ranks_reference_is_the_dense_definition():
    x, b, nb, q = tables()
    s = dense_scores(b, nb, q)
    rng = np.random.default_rng(4)
    d = rng.random((12, 11)) < 0.4                                          # two columns beyond the items: out of range
    d[:, 2:4] = True                                                        # the identical items 2 and 3, held out together
    d[7] = False
    actual, excl = sp.csr_matrix(d.astype(float)), (5,)
    above, tied, n_adm = knn_ranks_reference(x, nb, q, actual, seen(b), excl)
    assert above.dtype == tied.dtype == n_adm.dtype == np.int32 and above.shape == (actual.nnz,)
    e = 0
    tied_pair = 0
    for u in range(12):
        adm = [j for j in range(9) if not b[u, j] and j not in excl]
        assert n_adm[u] == len(adm)
        for h in np.flatnonzero(d[u]):
            if h in adm:
                assert above[e] == sum(s[u, j] > s[u, h] for j in adm) and tied[e] == sum(s[u, j] == s[u, h] for j in adm if j != h)
            else:
                assert above[e] == -1 and tied[e] == -1
            e += 1
        if 2 in adm and 3 in adm and s[u, 2] == s[u, 3] > 0:
            tied_pair += 1
    assert e == actual.nnz and tied_pair > 0
    # everything masked: n_adm = 0 and every entry inadmissible
    above, tied, n_adm = knn_ranks_reference(x, nb, q, actual, sp.csr_matrix(np.ones(b.shape)))
    assert (n_adm == 0).all() and (above == -1).all() and (tied == -1).all()


# ---- the class on the CPU stand-in -----------------------------------------------------------------------------------------------
def fitted(sim="cosine", **kw):
    x, b = tiny()
    return ItemKNN(k_neighbors=4, similarity=sim, backend=_oracle_metrics_backend(), **kw).fit(x), x, b


def held_out(b, seed=2):
    return sp.csr_matrix((np.random.default_rng(seed).random(b.shape) < 0.3) * (1 - b) * 2.0)


@pytest.mark.parametrize("sim", ("cosine", "count"))
def test_predict_with_candidates(sim):
    m, x, b = fitted(sim)
    q = weight_table(m.neighbors, m.counts, m.item_count, sim)
    unit = 1.0 if sim == "count" else float(Q_ONE)
    cand = sp.csr_matrix(np.random.default_rng(5).random(b.shape) < 0.5)
    top = m.predict(x, 4, items_exclude=(1,), candidates=cand.tocsc())     # any sparse format
    ref = knn_candidates_reference(x, m.neighbors, q, cand, 4, canonical_pattern(x), (1,))
    assert np.array_equal(np.asarray(top), ref[0])
    assert np.array_equal(top.scores, np.where(ref[0] < 0, np.nan, ref[1] / unit), equal_nan=True)
    every = sp.csr_matrix(np.ones(b.shape))
    a, c = m.predict(x, 9), m.predict(x, 9, candidates=every)
    assert np.array_equal(np.asarray(a), np.asarray(c)) and np.array_equal(a.scores, c.scores, equal_nan=True)


def test_evaluate_on_every_item_equals_evaluate():
    m, x, b = fitted()
    held = held_out(b)
    every = sp.csr_matrix(np.ones(b.shape))
    for k in (3, (2, 5)):
        plain, cand = m.evaluate(x, held, k, metrics=METRICS), m.evaluate(x, held, k, metrics=METRICS, candidates=every)
        assert set(plain) == set(cand) == set(METRICS)
        for name in METRICS:
            assert np.array_equal(plain[name], cand[name], equal_nan=True), name


@pytest.mark.parametrize("weights", (False, True))
def test_evaluate_with_negatives_is_evaluate_on_the_sampled_candidates(weights):
    """the tiny matrix has 9 items, so the MovieLens-sized call of the protocol, negatives=99, takes every admissible item; 3
    negatives leave a choice"""
    m, x, b = fitted()
    held = held_out(b)
    w = np.arange(1, 10, dtype=np.float64) if weights else None
    for n in (99, 3):
        cand = WRMF(backend=_oracle_metrics_backend()).sample_negatives(x, n, actual=held, seed=7, weights=w)
        mine = m.sample_negatives(x, n, actual=held, seed=7, weights=w)
        assert np.array_equal(cand.indptr, mine.indptr) and np.array_equal(cand.indices, mine.indices)
        a = m.evaluate(x, held, 3, metrics=METRICS, negatives=n, seed=7, negative_weights=w)
        c = m.evaluate(x, held, 3, metrics=METRICS, candidates=cand)
        for name in METRICS:
            assert np.array_equal(a[name], c[name], equal_nan=True), name
        assert (cand.multiply(held) != 0).nnz == held.nnz                   # the held-out items are kept
        assert cand.multiply(sp.csr_matrix(b)).nnz == 0                    # and nothing of not_recommend = x is drawn
    other = m.evaluate(x, held, 3, negatives=3, seed=8)
    assert set(other) == {"ap", "ndcg"}


def test_argument_refusals():
    m, x, b = fitted()
    held = held_out(b)
    every = sp.csr_matrix(np.ones(b.shape))
    with pytest.raises(ValueError, match="shape"):
        m.predict(x, 3, candidates=every[:5])
    with pytest.raises(ValueError, match="shape"):
        m.predict(x, 3, candidates=every[:, :5])
    with pytest.raises(TypeError):
        m.predict(x, 3, candidates=every.toarray())
    with pytest.raises(ValueError, match="seed"):
        m.evaluate(x, held, 3, negatives=3)
    with pytest.raises(ValueError, match="exclude each other"):
        m.evaluate(x, held, 3, negatives=3, seed=1, candidates=every)
    with pytest.raises(ValueError, match="negative_weights needs negatives"):
        m.evaluate(x, held, 3, negative_weights=np.ones(9))
    with pytest.raises(ValueError, match="seed"):
        m.sample_negatives(x, 3)
    with pytest.raises(ValueError):
        m.evaluate(x, held, 3, negatives=0, seed=1)
    with pytest.raises(ValueError, match="shape"):
        m.score(x, every[:, :5])
    with pytest.raises(TypeError):
        m.score(x, every.toarray())
    with pytest.raises(ValueError, match="shape"):
        m.held_out_ranks(x, held[:, :5])
    with pytest.raises(TypeError):
        m.evaluate_ranks(x, held.toarray())
    with pytest.raises(ValueError):
        m.held_out_ranks(x, held, items_exclude=(9,))
    unfitted = ItemKNN(backend=_oracle_metrics_backend())
    for call in (lambda: unfitted.score(x, every), lambda: unfitted.held_out_ranks(x, held), lambda: unfitted.predict(x, 3, candidates=every)):
        with pytest.raises(RuntimeError):
            call()


def test_score_is_scaled_as_the_lists_scores():
    """ "count": the raw sum; binary cosine: sum / 2^30; a weighted kind: sum / (s_l 2^30 / max(sim)) -- what `.scores` reports"""
    x, b = tiny()
    every = sp.csr_matrix(np.ones(b.shape))
    for kw in (dict(similarity="count"), dict(similarity="cosine"), dict(similarity="cosine", weighting="values"), dict(similarity="rp3beta")):
        m = ItemKNN(k_neighbors=4, backend=_oracle_metrics_backend(), **kw).fit(x)
        be = m._backend()
        pat = canonical_pattern(x)
        xq = m._row_weights(pat, be)
        raw = knn_score_pairs_reference(x, m.neighbors, m._weights(), every, xv=xq).astype(np.float64)
        if kw["similarity"] == "count":
            want = raw
        elif "weighting" in kw or kw["similarity"] == "rp3beta":
            want = raw / (np.float64(m._ops.scale_l) * np.float64(m._q[1]))
        else:
            want = raw / np.float64(Q_ONE)
        got = m.score(x, every)
        assert got.dtype == np.float64 and got.shape == b.shape and np.array_equal(got.data, want) and (want > 0).any()
        # the list's scores are the scores at the list's cells
        top = m.predict(x, 3, not_recommend=None)
        dense = got.toarray()
        for u in range(b.shape[0]):
            assert np.array_equal(top.scores[u], dense[u, np.asarray(top)[u]])
        # stored zeros of `pairs` are positions too, duplicates merge
        odd = sp.csr_matrix((np.array([0.0, 1.0, 1.0]), (np.array([1, 1, 1]), np.array([4, 2, 2]))), shape=b.shape)
        assert m.score(x, odd).indices.tolist() == [2, 4] and np.array_equal(m.score(x, odd).data, dense[1, [2, 4]])


def test_ranks_on_the_stand_in():
    m, x, b = fitted()
    held = held_out(b)
    q = weight_table(m.neighbors, m.counts, m.item_count, "cosine")
    ref = knn_ranks_reference(x, m.neighbors, q, held, canonical_pattern(x), (1,))   # (not_recommend="x" is the pattern the model sees)
    above, tied, n_adm = m.held_out_ranks(x, held, items_exclude=(1,))
    assert np.array_equal(above.data, ref[0]) and np.array_equal(tied.data, ref[1]) and np.array_equal(n_adm, ref[2])
    assert above.dtype == np.int32 and np.array_equal(above.indptr, held.indptr) and n_adm.dtype == np.int32
    ev = m.evaluate_ranks(x, held, items_exclude=(1,), per_user=True)
    summ = rank_summary(above, tied, n_adm, held)
    tot = rank_totals(summ)
    assert set(ev) == {"mpr", "auc", "mrr", "n", "mpr_per_user", "auc_per_user", "mrr_per_user", "n_adm_per_user"}
    assert ev["n"] == tot["n"] == int((ref[0] >= 0).sum())
    for name in ("mpr", "auc", "mrr"):
        assert np.allclose(ev[name + "_per_user"], summ[name], rtol=1e-13, atol=0, equal_nan=True), name
        assert np.isclose(ev[name], tot[name], rtol=1e-13, atol=0), name
    assert set(m.evaluate_ranks(x, held)) == {"mpr", "auc", "mrr", "n"}
    none = m.evaluate_ranks(x, sp.csr_matrix(b.shape))
    assert none["n"] == 0 and np.isnan(none["mpr"])


def test_a_weighted_model_fitted_with_a_confidence():
    """BM25 cosine: the rows' weights (`_row_weights`) go into every new path"""
    x, b = tiny()
    x = x.copy()
    x.data = np.random.default_rng(6).integers(1, 5, size=x.nnz).astype(np.float64)
    m = ItemKNN(k_neighbors=4, similarity="cosine", weighting=Confidence("bm25"), backend=_oracle_metrics_backend()).fit(x)
    be = m._backend()
    xq = m._row_weights(canonical_pattern(x), be)
    assert xq is not None and len(set(xq.tolist())) > 2
    every = sp.csr_matrix(np.ones(b.shape))
    held = held_out(b)
    a, c = m.predict(x, 5), m.predict(x, 5, candidates=every)
    assert np.array_equal(np.asarray(a), np.asarray(c)) and np.array_equal(a.scores, c.scores, equal_nan=True)
    cand = sp.csr_matrix(np.random.default_rng(8).random(b.shape) < 0.5)
    ref = knn_candidates_reference(x, m.neighbors, m._weights(), cand, 4, canonical_pattern(x), (), xv=xq)
    unweighted = knn_candidates_reference(x, m.neighbors, m._weights(), cand, 4, canonical_pattern(x), ())
    top = m.predict(x, 4, candidates=cand)
    assert np.array_equal(np.asarray(top), ref[0]) and not np.array_equal(ref[1], unweighted[1])
    assert np.array_equal(m.score(x, every).data, m._scale(knn_score_pairs_reference(x, m.neighbors, m._weights(), every, xv=xq)))
    rr = knn_ranks_reference(x, m.neighbors, m._weights(), held, canonical_pattern(x), (), xv=xq)
    above, tied, n_adm = m.held_out_ranks(x, held)
    assert np.array_equal(above.data, rr[0]) and np.array_equal(tied.data, rr[1]) and np.array_equal(n_adm, rr[2])
    one, two = m.evaluate(x, held, 3, negatives=4, seed=3), m.evaluate(x, held, 3, candidates=m.sample_negatives(x, 4, actual=held, seed=3))
    assert all(np.array_equal(one[name], two[name], equal_nan=True) for name in one)
