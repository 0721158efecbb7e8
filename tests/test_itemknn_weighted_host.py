"""ItemKNN on weighted values, without a device: the two numpy definitions of rsparse_amd/itemknn.py (the weighted fit, the
weighted lists) against brute-force dense numpy, the quantisation rule, every recipe's operands against its formula, and the model
on the CPU stand-in backend.  Integer fixtures (weights whose maximum is 2^bits - 1: the scale is 1 and quantisation the identity)
are compared exactly; real-valued weights against the float64 dense value within the bound the test derives from the quantisation
step."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle_backend import OracleBackend
from rsparse_amd import Confidence, ItemKNN, _lib
from rsparse_amd.itemknn import (Q_ONE, XQ_MAX, canonical_pattern, check_exact_bound, check_tables, cooccurrence_reference,
                                 knn_recommend_reference, operand_bits, quantize_values, weight_table, weighted_cooccurrence_reference,
                                 weighted_key, weighted_operands, weighted_similarity_values, weighted_weight_table)


# ---- the problems ------------------------------------------------------------------------------------------------------------------
def integer_matrix(bits=4, n_users=30, n_items=12, seed=1):
    """integer weights in 1 .. 2^bits - 1 with the maximum present; items 3 and 4 identical (users and weights), items 5 and 6 with
    the same users and other weights; item 11 without users"""
    rng = np.random.default_rng(seed)
    top = 2 ** bits - 1
    d = (rng.random((n_users, n_items)) < 0.35) * rng.integers(1, top + 1, (n_users, n_items))
    d[:, 4] = d[:, 3]
    d[:, 6] = np.where(d[:, 5] > 0, top + 1 - d[:, 5], 0)
    d[:, 11] = 0
    d[0, 0] = top
    return sp.csr_matrix(d.astype(np.float64))


def real_matrix(seed=2, n_users=50, n_items=20):
    rng = np.random.default_rng(seed)
    d = (rng.random((n_users, n_items)) < 0.3) * rng.integers(1, 9, (n_users, n_items))
    return sp.csr_matrix(d.astype(np.float64))


def dense_fit(L, R, a, b, h, K):
    """the definition on dense arrays: C = L^T R without its diagonal, every row ordered by (key descending, j ascending)"""
    n_items = L.shape[1]
    C = L.astype(np.int64).T @ R.astype(np.int64)
    np.fill_diagonal(C, 0)
    nb = np.full((n_items, K), -1, dtype=np.int32)
    sums = np.zeros((n_items, K), dtype=np.uint64)
    for i in range(n_items):
        j = np.flatnonzero(C[i])
        key = C[i, j].astype(np.float64) / (a[i] * b[j] + h)
        first = j[np.lexsort((j, -key))[:K]]
        nb[i, :first.size] = first
        sums[i, :first.size] = C[i, first]
    return nb, sums, C


def operands_dense(m, ops):
    L, R = np.zeros(m.shape, dtype=np.int64), np.zeros(m.shape, dtype=np.int64)
    rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
    L[rows, m.indices], R[rows, m.indices] = ops.l, ops.r
    return L, R


# ---- quantisation ------------------------------------------------------------------------------------------------------------------
def test_quantize_values_rule():
    w = np.array([0.0, 1e-9, 0.2, 0.5, 1.0, 2.0])
    q, s = quantize_values(w, 8)
    assert s == 255.0 / 2.0 and q.dtype == np.int64
    assert np.array_equal(q, [0, 1, 26, 64, 128, 255])                     # 0 stays 0, a positive weight is at least 1, rint to even
    assert np.array_equal(q[2:], np.rint(w[2:] * s))
    q16, s16 = quantize_values(w)                                          # 16 bits by default
    assert s16 == 65535.0 / 2.0 and q16.max() == 65535
    ints = np.array([3.0, 15.0, 1.0, 7.0])
    q, s = quantize_values(ints, 4)
    assert s == 1.0 and np.array_equal(q, ints)                            # the maximum is 2^bits - 1: the identity
    # the fit's scale at predict, clipped to 2^16 - 1
    q, s = quantize_values(np.array([0.0, 1e-9, 1.0, 1e9]), scale=100.0, top=XQ_MAX)
    assert s == 100.0 and np.array_equal(q, [0, 1, 100, XQ_MAX])
    assert quantize_values(np.zeros(0))[0].shape == (0,) and np.array_equal(quantize_values(np.zeros(3))[0], [0, 0, 0])


def test_a_constant_operand_quantises_to_one():
    q, s = quantize_values(np.full(7, 2.5), 16)
    assert np.array_equal(q, np.ones(7)) and s == 1.0 / 2.5
    x = real_matrix()
    ops = weighted_operands(ItemKNN(similarity="dot")._weigh(canonical_pattern(x), None, True), "dot")
    assert (ops.l == 1).all() and (ops.r == 1).all() and ops.scale_l == 1.0 and (ops.a == 1.0).all() and ops.h == 0.0


def test_negative_and_non_finite_weights_are_refused():
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            quantize_values(np.array([1.0, bad]))
    x = real_matrix().tolil()
    x[3, 2] = -2.0
    with pytest.raises(ValueError):
        ItemKNN(similarity="dot", weighting="values", backend=OracleBackend()).fit(x.tocsr())
    with pytest.raises(ValueError):
        ItemKNN(similarity="rp3beta", weighting="values", backend=OracleBackend()).fit(x.tocsr())


def test_bits_rule_and_the_exactness_bound():
    assert [operand_bits(b, n) for b, n in ((16, 1), (24, 1), (16, 2 ** 10), (24, 2 ** 10), (24, 2 ** 10 + 1), (16, 2 ** 21),
                                            (24, 2 ** 21), (24, 2 ** 21 + 1))] == [16, 24, 16, 21, 21, 16, 16, 15]
    rng = np.random.default_rng(4)
    for n_users, asked, want in ((1, 24, 24), (2 ** 10, 24, 21), (2 ** 10, 16, 16), (2 ** 21, 24, 16)):
        col = sp.csr_matrix((rng.random(n_users) + 0.5, (np.arange(n_users), np.zeros(n_users, dtype=np.int64))), shape=(n_users, 2))
        ops = weighted_operands(col, "dot", bits=asked)
        assert ops.bits == want and ops.item_count.max() == n_users
        if n_users > 1:
            assert ops.l.max() == 2 ** want - 1 and ops.l.max() ** 2 * n_users < 2 ** 53
    check_exact_bound([2 ** 24], [2 ** 24], 31)
    with pytest.raises(ValueError):
        check_exact_bound([2 ** 24], [2 ** 24], 32)                        # 2^53 exactly
    with pytest.raises(ValueError):
        weighted_cooccurrence_reference(np.arange(34), np.zeros(33, dtype=np.int64), np.full(33, 2 ** 24), np.full(33, 2 ** 24), 1,
                                        [1.0], [1.0], 0.0, 1)                 # 33 users of one item
    for bad in (0, 25, 2.5, True):
        with pytest.raises(ValueError):
            quantize_values(np.ones(2), bad)
    check_tables([2.0 ** -200, 2.0 ** 200], [1.0, 1.0], 2.0 ** 400)
    for a, h in (([0.0], 0.0), ([2.0 ** 201], 0.0), ([np.nan], 0.0), ([np.inf], 0.0), ([1.0], -1.0), ([1.0], np.inf), ([1.0], 2.0 ** 401),
                 ([1.0], np.nan)):
        with pytest.raises(ValueError):
            check_tables(a, [1.0], h)
        if h == 0.0:
            with pytest.raises(ValueError):
                check_tables([1.0], a, h)


# ---- the fit against brute force -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (1, 4, 11, 15))
def test_dot_on_integer_weights_is_the_dense_product(K):
    x = integer_matrix()
    m = canonical_pattern(x)
    ops = weighted_operands(m, "dot", bits=4)
    assert ops.scale_l == 1.0 and np.array_equal(ops.l, m.data) and np.array_equal(ops.r, m.data)
    nb, sums = weighted_cooccurrence_reference(m.indptr, m.indices, ops.l, ops.r, 12, ops.a, ops.b, ops.h, K)
    W = x.toarray().astype(np.int64)
    want_nb, want_sums, C = dense_fit(W, W, ops.a, ops.b, ops.h, K)
    assert np.array_equal(C + np.diag(np.diag(W.T @ W)), W.T @ W)
    assert nb.dtype == np.int32 and sums.dtype == np.uint64
    assert np.array_equal(nb, want_nb) and np.array_equal(sums, want_sums)
    live = nb >= 0
    assert np.array_equal(sums[live], (W.T @ W)[np.nonzero(live)[0], nb[live]])          # the sums ARE W^T W
    assert (nb[11] == -1).all() and (sums[11] == 0).all() and not (nb == 11).any()        # the item without users
    assert np.array_equal(weighted_similarity_values(nb, sums, ops.a, ops.b, ops.h)[live], sums[live].astype(np.float64))


@pytest.mark.parametrize("sim,kw", [("cosine", {}), ("cosine", {"shrinkage": 40.0}), ("asymmetric", {"alpha": 0.3, "shrinkage": 3.0}),
                                    ("rp3beta", {"alpha": 0.7, "beta": 0.5}), ("rp3beta", {"alpha": 1.0})])
def test_every_kind_equals_the_dense_definition_with_its_ties(sim, kw):
    x = integer_matrix()
    m = canonical_pattern(x)
    ops = weighted_operands(m, sim, bits=4, **kw)
    nb, sums = weighted_cooccurrence_reference(m.indptr, m.indices, ops.l, ops.r, 12, ops.a, ops.b, ops.h, 11)
    L, R = operands_dense(m, ops)
    want_nb, want_sums, _ = dense_fit(L, R, ops.a, ops.b, ops.h, 11)
    assert np.array_equal(nb, want_nb) and np.array_equal(sums, want_sums)
    if sim == "cosine" and not kw:
        # items 3 and 4 are one column twice: equal keys towards every third item, the tie goes to 3; each other's best, at 1
        sims = weighted_similarity_values(nb, sums, ops.a, ops.b, ops.h)
        assert nb[3, 0] == 4 and nb[4, 0] == 3 and abs(sims[3, 0] - 1.0) < 1e-15
        for i in (0, 1, 2, 7):
            row = nb[i].tolist()
            if 3 in row:
                assert row.index(4) == row.index(3) + 1 and sims[i, row.index(3)] == sims[i, row.index(4)]
        # items 5 and 6 share their users, not their weights: their keys towards a third item differ
        assert any(sims[i, nb[i].tolist().index(5)] != sims[i, nb[i].tolist().index(6)] for i in range(5) if 5 in nb[i] and 6 in nb[i])


def test_shrinkage_changes_the_order():
    x = integer_matrix()
    m = canonical_pattern(x)
    tables = []
    for shrinkage in (0.0, 40.0):
        ops = weighted_operands(m, "cosine", shrinkage=shrinkage, bits=4)
        tables.append(weighted_cooccurrence_reference(m.indptr, m.indices, ops.l, ops.r, 12, ops.a, ops.b, ops.h, 11)[0])
    assert (tables[0] != tables[1]).any()


# ---- the recipes ---------------------------------------------------------------------------------------------------------------------
def test_recipes_follow_their_formulas():
    x = real_matrix()
    w = Confidence("tfidf").fit_transform(x, backend=OracleBackend())
    v, j = w.data, w.indices
    n = np.bincount(j, minlength=20)
    rows = np.repeat(np.arange(50), np.diff(w.indptr))
    q, s = quantize_values(v, 16)
    S = np.bincount(j, weights=(q * q).astype(np.float64), minlength=20)
    assert s == 65535.0 / v.max() and (S == np.array([(q[j == i] ** 2).sum() for i in range(20)])).all()

    ops = weighted_operands(w, "dot")
    assert np.array_equal(ops.l, q) and np.array_equal(ops.r, q) and (ops.a == s).all() and (ops.b == s).all() and ops.h == 0.0
    assert ops.scale_l == s and ops.scale_r == s and ops.bits == 16 and np.array_equal(ops.item_count, n)

    ops = weighted_operands(w, "cosine", shrinkage=2.5)
    assert np.array_equal(ops.l, q) and np.array_equal(ops.r, q)
    assert np.array_equal(ops.a, np.sqrt(S)) and np.array_equal(ops.b, np.sqrt(S)) and ops.h == 2.5 * s * s

    ops = weighted_operands(w, "asymmetric", alpha=0.3, shrinkage=1.5)
    assert np.array_equal(ops.l, q) and np.array_equal(ops.a, S ** 0.3) and np.array_equal(ops.b, S ** (1.0 - 0.3)) and ops.h == 1.5 * s * s
    half = weighted_operands(w, "asymmetric")                              # alpha = 0.5 by default: the cosine's tables
    assert np.array_equal(half.a, S ** 0.5) and np.array_equal(half.b, S ** 0.5)

    alpha, beta = 0.8, 0.4
    d = np.bincount(rows, weights=v, minlength=50)
    ql, sl = quantize_values(v ** alpha, 16)
    qr, sr = quantize_values((v / d[rows]) ** alpha, 16)
    ops = weighted_operands(w, "rp3beta", alpha=alpha, beta=beta)
    assert np.array_equal(ops.l, ql) and np.array_equal(ops.r, qr) and (ops.l != ops.r).any() and ops.h == 0.0
    assert np.array_equal(ops.a, sl * np.bincount(j, weights=v, minlength=20) ** alpha) and np.array_equal(ops.b, sr * n.astype(np.float64) ** beta)
    # beta = 0 is P3alpha: no popularity term, so every row is ordered by its sums alone
    p3 = weighted_operands(w, "rp3beta", alpha=alpha, beta=0.0)
    assert np.array_equal(p3.l, ql) and np.array_equal(p3.r, qr) and (p3.b == sr).all() and np.array_equal(p3.a, ops.a)
    m = ItemKNN(k_neighbors=19, similarity="rp3beta", weighting=Confidence("tfidf"), alpha=alpha, backend=OracleBackend()).fit(x)
    for i in range(20):
        live = m.neighbors[i] >= 0
        c, jj = m.sums[i][live].astype(np.int64), m.neighbors[i][live]
        assert np.array_equal(np.lexsort((jj, -c)), np.arange(c.size))
    L, R = np.zeros((50, 20)), np.zeros((50, 20))
    L[rows, j], R[rows, j] = v ** alpha, (v / d[rows]) ** alpha
    col = (np.bincount(j, weights=v, minlength=20) ** alpha)[:, None]
    dense = (L.T @ R) / col                                                # P3alpha in float64
    # an operand is off by at most 0.5 / scale (1 / scale where the clip to >= 1 acts); the denominator is not quantised
    dL, dR = (np.where(t > 0, np.where(t * sc < 0.5, 1.0, 0.5) / sc, 0.0) for t, sc in ((L, sl), (R, sr)))
    bound = (L.T @ dR + dL.T @ R + dL.T @ dR) / col + 1e-13 * dense
    live = m.neighbors >= 0
    at = (np.nonzero(live)[0], m.neighbors[live])
    assert (np.abs(m.similarities[live] - dense[at]) <= bound[at]).all() and (bound[at] < 1e-3 * dense[at]).all()


def test_reported_cosine_of_bm25_weights_is_within_the_quantisation_bound():
    x = real_matrix()
    be = OracleBackend()
    model = ItemKNN(k_neighbors=19, similarity="cosine", weighting=Confidence("bm25"), backend=be).fit(x)
    w = Confidence("bm25").fit_transform(x, backend=be)
    assert w.data.min() > 0
    s = model._ops.scale_l
    W = w.toarray()
    # every weight is off by at most 0.5 / scale, 1 / scale where the clip to >= 1 acts
    delta = np.where(W > 0, np.where(W * s < 0.5, 1.0, 0.5) / s, 0.0)
    N = W.T @ W
    EN = W.T @ delta + delta.T @ W + delta.T @ delta                       # |sum w'w' - sum ww|
    norm, enorm = np.sqrt((W * W).sum(axis=0)), np.sqrt((delta * delta).sum(axis=0))
    D = np.outer(norm, norm)
    ED = np.outer(norm, enorm) + np.outer(enorm, norm) + np.outer(enorm, enorm)        # |the product of the norms' error|
    live = model.neighbors >= 0
    i, j = np.nonzero(live)[0], model.neighbors[live]
    assert (D[i, j] > 2 * ED[i, j]).all()
    exact = N[i, j] / D[i, j]
    bound = EN[i, j] / (D[i, j] - ED[i, j]) + N[i, j] * ED[i, j] / (D[i, j] * (D[i, j] - ED[i, j])) + 1e-13 * exact
    err = np.abs(model.similarities[live] - exact)
    print("largest error %.3e, its bound %.3e, largest bound %.3e" % (err.max(), bound[err.argmax()], bound.max()))
    assert (err <= bound).all() and bound.max() < 1e-3
    assert live.sum() == (N[~np.eye(20, dtype=bool)] > 0).sum()            # K = n_items - 1: every co-occurring pair is a slot


# ---- the lists -----------------------------------------------------------------------------------------------------------------------
def test_weighted_lists_against_dense_numpy():
    rng = np.random.default_rng(6)
    n_items, K = 12, 5
    nb = np.stack([rng.permutation(n_items)[:K] for _ in range(n_items)]).astype(np.int32)
    nb[2, 3:] = -1
    q = rng.integers(0, Q_ONE + 1, (n_items, K))
    q[nb < 0] = 0
    x = integer_matrix(bits=16, n_items=n_items, seed=8)
    m = canonical_pattern(x)
    xv = m.data.astype(np.int64)
    assert xv.max() == XQ_MAX and xv.min() >= 1
    Qd = np.zeros((n_items, n_items), dtype=np.int64)
    for i in range(n_items):
        for s_ in range(K):
            if nb[i, s_] >= 0:
                Qd[i, nb[i, s_]] += q[i, s_]
    score = x.toarray().astype(np.int64) @ Qd
    for nr, excl in ((None, ()), (x, (1, 7))):
        items, scores = knn_recommend_reference(x, nb, q, 6, nr, excl, xv=xv)
        for u in range(x.shape[0]):
            adm = np.ones(n_items, dtype=bool)
            if nr is not None:
                adm[m.indices[m.indptr[u]:m.indptr[u + 1]]] = False
            adm[list(excl)] = False
            cand = np.flatnonzero(adm)
            first = cand[np.lexsort((cand, -score[u, cand]))[:6]]
            assert np.array_equal(items[u, :first.size], first) and (items[u, first.size:] == -1).all()
            assert np.array_equal(scores[u, :first.size], score[u, first])
    ones = knn_recommend_reference(x, nb, q, 6, None, (), xv=np.ones(m.nnz, dtype=np.int64))
    plain = knn_recommend_reference(x, nb, q, 6, None, ())
    assert np.array_equal(ones[0], plain[0]) and np.array_equal(ones[1], plain[1])
    with pytest.raises(ValueError):
        knn_recommend_reference(x, nb, q, 6, None, (), xv=xv[:-1])


def test_weight_table_of_the_weighted_kinds():
    sim = np.array([[0.5, 0.25, np.nan], [2.0, 1e-12, 0.3]])
    q, scale = weighted_weight_table(sim)
    assert scale == 2.0 ** 30 / 2.0 and np.array_equal(q, [[2 ** 28, 2 ** 27, 0], [2 ** 30, 0, np.rint(0.3 * scale)]])
    q, scale = weighted_weight_table(np.full((2, 2), np.nan))
    assert scale == 1.0 and (q == 0).all()


# ---- the model on the CPU stand-in -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bm25_model():
    x = real_matrix()
    return ItemKNN(k_neighbors=6, similarity="cosine", weighting=Confidence("bm25"), shrinkage=1.0, backend=OracleBackend()).fit(x), x


def test_model_attributes_of_a_weighted_fit(bm25_model):
    m, x = bm25_model
    assert m.counts is None and m.sums.dtype == np.uint64 and m.sums.shape == m.neighbors.shape == (20, 6)
    assert np.array_equal(m.item_count, np.diff(x.tocsc().indptr))
    live = m.neighbors >= 0
    i, j = np.nonzero(live)[0], m.neighbors[live]
    assert np.array_equal(m.similarities[live], weighted_key(m.sums[live], m._ops.a[i], m._ops.b[j], m._ops.h))
    assert np.isnan(m.similarities[~live]).all() and (m.sums[~live] == 0).all()
    top = m.similar_items([0, 3], k=4)
    assert np.array_equal(np.asarray(top), m.neighbors[[0, 3], :4]) and np.array_equal(top.scores, m.similarities[[0, 3], :4])


def test_a_list_does_not_depend_on_the_batch(bm25_model):
    m, x = bm25_model
    whole = m.predict(x, 7, items_exclude=(2,))
    for u in (0, 5, 17, 49):
        alone = m.predict(x[u], 7, items_exclude=(2,))
        assert np.array_equal(np.asarray(alone)[0], np.asarray(whole)[u]) and np.array_equal(alone.scores[0], whole.scores[u], equal_nan=True)
    part = m.predict(x[10:20], 7, items_exclude=(2,))
    assert np.array_equal(np.asarray(part), np.asarray(whole)[10:20]) and np.array_equal(part.scores, whole.scores[10:20], equal_nan=True)


def test_model_predict_is_the_definition_on_the_fit_scale(bm25_model):
    m, x = bm25_model
    pat = canonical_pattern(x)
    w_new = m._weighting.transform(pat, backend=OracleBackend())
    xq, _ = quantize_values(w_new.data, scale=m._ops.scale_l, top=XQ_MAX)
    q, q_scale = weighted_weight_table(m.similarities)
    assert q.max() == Q_ONE and q_scale == 2.0 ** 30 / np.nanmax(m.similarities)
    items, scores = knn_recommend_reference(x, m.neighbors, q, 5, x, (), xv=xq)
    top = m.predict(x, 5)
    assert np.array_equal(np.asarray(top), items)
    assert np.array_equal(top.scores, np.where(items < 0, np.nan, scores / (m._ops.scale_l * q_scale)), equal_nan=True)
    # the scores approximate sum_i w_ui sim_ij
    S = np.zeros((20, 20))
    live = m.neighbors >= 0
    S[np.nonzero(live)[0], m.neighbors[live]] = m.similarities[live]
    approx = w_new.toarray() @ S
    u, c = np.nonzero(np.asarray(top) >= 0)
    np.testing.assert_allclose(top.scores[u, c], approx[u, np.asarray(top)[u, c]], rtol=1e-3, atol=1e-6)


def test_no_weighting_scores_with_ones():
    x = real_matrix()
    m = ItemKNN(k_neighbors=6, similarity="rp3beta", beta=0.3, backend=OracleBackend()).fit(x)
    assert m._row_weights(canonical_pattern(x), OracleBackend()) is None
    q, _ = weighted_weight_table(m.similarities)
    ref = knn_recommend_reference(x, m.neighbors, q, 5, x)
    assert np.array_equal(np.asarray(m.predict(x, 5)), ref[0])


def test_parameter_errors():
    x = real_matrix()
    for sim in ("jaccard", "count"):
        for weighting in ("values", Confidence("bm25")):
            with pytest.raises(ValueError):
                ItemKNN(similarity=sim, weighting=weighting)
    for kw in ({"similarity": "pearson"}, {"similarity": "pearson", "weighting": "values"}, {"weighting": "bm25"}, {"weighting": 3},
               {"bits": 0}, {"bits": 25}, {"bits": 2.5}, {"similarity": "dot", "shrinkage": -1.0}, {"similarity": "dot", "shrinkage": np.nan},
               {"similarity": "asymmetric", "alpha": 1.5}, {"similarity": "asymmetric", "alpha": -0.1}, {"similarity": "rp3beta", "alpha": np.inf},
               {"similarity": "rp3beta", "beta": -0.5}, {"similarity": "cosine", "weighting": "values", "shrinkage": -2}):
        with pytest.raises(ValueError):
            ItemKNN(**kw)
    with pytest.raises(_lib.UnsupportedOnDevice):
        ItemKNN(similarity="dot", k_neighbors=257)
    m = ItemKNN(similarity="dot", weighting="values", backend=OracleBackend())
    with pytest.raises(RuntimeError):
        m.predict(x, 3)
    m.fit(x)
    with pytest.raises(ValueError):
        m.predict(x[:, :5], 3)
    with pytest.raises(_lib.UnsupportedOnDevice):
        m.predict(x, 1025)
    neg = x.copy()
    neg.data[0] = -1.0
    with pytest.raises(ValueError):
        m.predict(neg, 3)


def test_a_row_whose_weights_sum_to_2_31_is_refused():
    n_items = 2 ** 15 + 2
    x = sp.csr_matrix(np.vstack([np.ones(n_items), np.r_[1.0, np.zeros(n_items - 1)]]))
    x.data[:] = 1.0
    fit = sp.csr_matrix(([1.0, 1e-6], ([0, 1], [0, 1])), shape=(2, n_items))  # the fit's scale: 65535 per unit of weight
    m = ItemKNN(k_neighbors=1, similarity="dot", weighting="values", backend=OracleBackend()).fit(fit)
    assert m._ops.scale_l == 65535.0
    assert np.asarray(m.predict(x[1], 1, not_recommend=None)).shape == (1, 1)
    with pytest.raises(_lib.UnsupportedOnDevice):
        m.predict(x, 1)                                                    # (2^15 + 2) (2^16 - 1) >= 2^31


@pytest.mark.parametrize("sim", ("cosine", "jaccard", "count"))
def test_the_pattern_kinds_are_unchanged(sim):
    x = real_matrix()
    old = ItemKNN(k_neighbors=5, similarity=sim, backend=OracleBackend()).fit(x)
    explicit = ItemKNN(k_neighbors=5, similarity=sim, weighting=None, shrinkage=0.0, bits=16, backend=OracleBackend()).fit(x)
    nb, ct, n = cooccurrence_reference(x, 5, sim)
    for m in (old, explicit):
        assert not m._weighted and m.sums is None
        assert np.array_equal(m.neighbors, nb) and np.array_equal(m.counts, ct) and m.counts.dtype == np.int32 and np.array_equal(m.item_count, n)
        q = weight_table(nb, ct, n, sim)
        ref = knn_recommend_reference(x, nb, q, 4, x)
        top = m.predict(x, 4)
        assert np.array_equal(np.asarray(top), ref[0])
        assert np.array_equal(top.scores, np.where(ref[0] < 0, np.nan, ref[1] / (1.0 if sim == "count" else 2.0 ** 30)), equal_nan=True)
