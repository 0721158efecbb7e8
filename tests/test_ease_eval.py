"""EASE under the evaluation protocols on the device (wrmf_ease.hip behind rsparse_hip_ease_score_pairs_device /
_top_candidates_device / _held_out_ranks_device) against the numpy definitions of rsparse_amd/ease.py: items by np.array_equal,
scores by their BITS, for both precisions of B.  B is handed to the entries directly: one fitted on `planted()`, and integer-valued
ones with entries in {-2, ..., 2}, whose sums tie often.  A row is scored at its cells while it asks for at most
n_items // EASE_CELLS_RATIO of them (and at most KNN_LDS_CAND), through its dense row otherwise: the problems put rows of both
routes into one call."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import EASE, WRMF, _lib
from rsparse_amd.ease import (ease_candidates_reference, ease_gram_reference, ease_ranks_reference, ease_recommend_reference,
                              ease_score_pairs_reference, ease_scores_reference, ease_weights_reference, key_scores, score_keys)
from rsparse_amd.itemknn import canonical_pattern
from rsparse_amd.metrics import rank_totals
from test_ease import backend, fitted, movielens_csr, padded, planted, same_lists

pytestmark = pytest.mark.gpu

CAND, RATIO = _lib.KNN_LDS_CAND, _lib.EASE_CELLS_RATIO
N_BIG = CAND + 100   # the dense route's select takes the radix fallback; more candidates than the LDS buffer holds are possible
NA = -2147483648
DTYPES = [np.float32, np.float64]
HISTORIES = (0, 1, 7, 8, 9, 63, 64, 65, 257, None)   # the look-ahead and chunk edges of the scorers; None: every item
PROBLEMS = [("fitted", 300), ("integer", 300), ("integer", 1), ("integer", 3), ("integer", N_BIG)]


def threshold(n_items):
    """the largest number of cells of a row that still takes the cell route"""
    return min(n_items // RATIO, CAND)


def counts(n_items):
    """candidates per row: the edges of a wave's 64 cells and of a workgroup's stride, both sides of the routing threshold, both
    sides of the LDS buffer, every item"""
    return sorted({min(c, n_items) for c in (0, 1, 63, 64, 65, 128, 129, threshold(n_items), threshold(n_items) + 1, CAND, CAND + 1, n_items)})


@functools.lru_cache(maxsize=None)
def weights(kind, n_items, dtype):
    """-> (B as numpy, B as the device tensor the kernels read)"""
    if kind == "fitted":
        assert n_items == planted().shape[1]
        B = ease_weights_reference(ease_gram_reference(planted(), 0.5), dtype)
    else:
        B = np.random.default_rng(n_items).integers(-2, 3, size=(n_items, n_items)).astype(dtype)
        np.fill_diagonal(B, 0.0)
    d_B = padded(B)
    B.setflags(write=False)
    return B, d_B


@functools.lru_cache(maxsize=None)
def problem(n_items):
    """-> (x, candidates): at least two rows for every candidate count of `counts`, their histories cycling through HISTORIES (whole
    cycles: the first row has no history, the last one every item), the candidates drawn from all items (so some lie in the row's
    own history)"""
    rng = np.random.default_rng(1000 + n_items)
    cs = counts(n_items)
    n_rows = -(-2 * len(cs) // len(HISTORIES)) * len(HISTORIES)
    x = np.zeros((n_rows, n_items), dtype=bool)
    c = np.zeros_like(x)
    for r in range(n_rows):
        h = HISTORIES[r % len(HISTORIES)]
        x[r, rng.choice(n_items, size=n_items if h is None else min(h, n_items), replace=False)] = True
        c[r, rng.choice(n_items, size=cs[(r // 2) % len(cs)], replace=False)] = True
    return sp.csr_matrix(x.astype(np.float64)), sp.csr_matrix(c.astype(np.float64))


def on_device(m):
    be = backend()
    return be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32)


def filters(nr, excl):
    be = backend()
    nr_p = nr_j = None
    if nr is not None and nr.nnz:
        nr_p, nr_j = on_device(sp.csr_matrix(nr))
    return {"nr_p": nr_p, "nr_j": nr_j, "exclude0": be.to_device(np.asarray(excl), torch.int32) if len(excl) else None}


def device_candidates(x, B, d_B, cand, k, nr=None, excl=(), ws_rows=0):
    """-> (items (n, k) int64 0-based with -1, scores float64 with 0 in the padding): the layout of ease_candidates_reference"""
    xp, xj = on_device(canonical_pattern(x, B.shape[0]))
    cp, cj = on_device(canonical_pattern(cand))
    res, keys = backend().ease_top_candidates(xp, xj, d_B, B.shape[0], k, cp, cj, ws_rows=ws_rows, **filters(nr, excl))
    res, keys = res.cpu().numpy().astype(np.int64), keys.cpu().numpy()
    assert (keys[res == NA] == 0).all()
    return np.where(res == NA, -1, res - 1), np.where(res == NA, 0.0, key_scores(keys))


# ---- the lists within candidates -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,n_items", PROBLEMS)
def test_candidate_lists_equal_the_definition(kind, n_items, dtype):
    (B, d_B), (x, cand) = weights(kind, n_items, dtype), problem(n_items)
    lens = np.diff(cand.indptr)
    if n_items >= 300:                                                      # rows of both routes in one call
        assert (lens <= threshold(n_items)).sum() >= 4 and (lens > threshold(n_items)).sum() >= 4
    k = min(10, n_items + 2)                                                # (the smallest shapes: k above the items)
    assert same_lists(device_candidates(x, B, d_B, cand, k), ease_candidates_reference(x, B, cand, k))
    excl = (0, n_items // 2)
    ref = ease_candidates_reference(x, B, cand, k, x, excl)
    got = device_candidates(x, B, d_B, cand, k, x, excl)
    assert same_lists(got, ref)
    assert (ref[0][-1] == -1).all() and (ref[0][:2] == -1).all()            # the user of every item; the rows without candidates
    if kind == "integer" and n_items >= 300:                                # the tie rule was at work: equal neighbours in a list
        assert ((ref[1][:, 1:] == ref[1][:, :-1]) & (ref[0][:, 1:] >= 0)).any()
    if n_items == N_BIG:                                                    # k above the admissible count of a long row, on both routes
        for r in (np.flatnonzero(lens == 129)[0], np.flatnonzero(lens == CAND + 1)[0]):
            row = cand[r].indices
            nr = sp.csr_matrix((np.ones(row.size - 3), (np.zeros(row.size - 3, dtype=int), row[3:])), shape=(1, n_items))
            got = device_candidates(x[r], B, d_B, cand[r], 6, nr)
            assert same_lists(got, ease_candidates_reference(x[r], B, cand[r], 6, nr))
            assert sorted(got[0][0][:3]) == row[:3].tolist() and (got[0][0][3:] == -1).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,n_items", [("fitted", 300), ("integer", N_BIG)])
def test_candidates_holding_every_item_are_the_full_lists(kind, n_items, dtype):
    (B, d_B), (x, _) = weights(kind, n_items, dtype), problem(n_items)
    x = x[:12]
    every = sp.csr_matrix(np.ones(x.shape))
    for k, nr, excl in ((10, x, ()), (1024 if n_items == N_BIG else 300, None, (3, n_items - 1))):
        assert same_lists(device_candidates(x, B, d_B, every, k, nr, excl), ease_recommend_reference(x, B, k, nr, excl))


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_routes_return_the_same_bits(dtype):
    """the same rows and candidates twice: at 100 candidates a row is scored at its cells; with a threshold's worth of excluded
    items added to the candidates it takes the dense route, and the additions are masked"""
    n_items = N_BIG
    (B, d_B), (x, _) = weights("integer", n_items, dtype), problem(n_items)
    assert 100 <= threshold(n_items) < n_items // 2
    rng = np.random.default_rng(3)
    pad = np.sort(rng.choice(n_items, size=threshold(n_items), replace=False))
    free = np.setdiff1d(np.arange(n_items), pad)
    few = np.zeros(x.shape, dtype=bool)
    for r in range(x.shape[0]):
        few[r, rng.choice(free, size=100, replace=False)] = True
    many = few.copy()
    many[:, pad] = True
    for nr in (None, x):
        a = device_candidates(x, B, d_B, sp.csr_matrix(few), 20, nr, tuple(pad))
        b = device_candidates(x, B, d_B, sp.csr_matrix(many), 20, nr, tuple(pad))
        assert same_lists(a, b) and same_lists(a, ease_candidates_reference(x, B, sp.csr_matrix(few), 20, nr, tuple(pad)))
    assert (a[0][0] >= 0).all() and (a[0][-1] == -1).all()


@pytest.mark.parametrize("ws_rows", [1, 2, 3])
def test_batches_repeats_and_a_small_call_behind_a_larger_one(ws_rows):
    (B, d_B), (x, cand) = weights("fitted", 300, np.float32), problem(300)
    ref = ease_candidates_reference(x, B, cand, 20, x, (5,))
    first = device_candidates(x, B, d_B, cand, 20, x, (5,), ws_rows=ws_rows)
    assert same_lists(first, ref)
    assert same_lists(device_candidates(x, B, d_B, cand, 20, x, (5,), ws_rows=ws_rows), first)
    assert same_lists(device_candidates(x, B, d_B, cand, 20, x, (5,)), first)
    (Bs, d_Bs), (xs, cs) = weights("integer", 3, np.float64), problem(3)
    assert same_lists(device_candidates(xs, Bs, d_Bs, cs, 3, ws_rows=ws_rows), ease_candidates_reference(xs, Bs, cs, 3))
    # the workspace came back as zeros: the full lists behind it are right
    res, keys = backend().ease_recommend(*on_device(canonical_pattern(x)), d_B, 300, 10)
    full = ease_recommend_reference(x, B, 10)
    assert np.array_equal(res.cpu().numpy() - 1, full[0]) and np.array_equal(key_scores(keys.cpu().numpy()), full[1])


# ---- the scores at given cells -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,n_items", PROBLEMS)
def test_scores_at_the_candidate_cells(kind, n_items, dtype):
    (B, d_B), (x, cand) = weights(kind, n_items, dtype), problem(n_items)
    pat = canonical_pattern(cand)
    keys = backend().ease_score_pairs(*on_device(canonical_pattern(x)), d_B, n_items, *on_device(pat)).cpu().numpy()
    ref = ease_score_pairs_reference(x, B, cand)
    assert np.array_equal(keys.view(np.uint64), score_keys(ref)) and np.array_equal(key_scores(keys).view(np.uint64), ref.view(np.uint64))
    own = backend().ease_score_pairs(*on_device(canonical_pattern(x)), d_B, n_items, *on_device(canonical_pattern(x))).cpu().numpy()
    assert np.array_equal(key_scores(own).view(np.uint64), ease_score_pairs_reference(x, B, x).view(np.uint64))   # nothing is masked


@pytest.mark.parametrize("ws_rows", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_score_of_unsorted_repeated_and_outside_columns(dtype, ws_rows):
    """through the device entry, which takes any columns: a row of few pairs (its cells), rows of many (their dense rows), a row
    without pairs; a column outside the items gives the key of +0.0 on both routes"""
    n_items = 300
    (B, d_B), (x, _) = weights("fitted", n_items, dtype), problem(n_items)
    x = x[[3, 9, 7, 0, 13]]                                                  # histories of 8, all, 63, 0 and 8 items
    rng = np.random.default_rng(8)
    t = threshold(n_items)
    rows = [np.r_[rng.integers(0, n_items, size=t - 4), [7, 7, -1, n_items]],
            np.r_[rng.integers(0, n_items, size=5 * t), [n_items + 5, 99999, -3, 11, 11]],
            x[2].indices[::-1],
            np.zeros(0, dtype=np.int64),
            np.r_[rng.integers(0, n_items, size=t + 1)]]
    for r in (0, 1, 4):
        rng.shuffle(rows[r])
    pp = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    pj = np.concatenate(rows)
    be = backend()
    keys = be.ease_score_pairs(*on_device(canonical_pattern(x)), d_B, n_items, be.to_device(pp, torch.int32), be.to_device(pj, torch.int32),
                               ws_rows=ws_rows).cpu().numpy().view(np.uint64)
    score = ease_scores_reference(x, B)
    u = np.repeat(np.arange(5), np.diff(pp))
    inside = (pj >= 0) & (pj < n_items)
    want = np.where(inside, score[u, np.where(inside, pj, 0)], 0.0)
    assert np.array_equal(keys, score_keys(want)) and (keys[~inside] == np.uint64(1 << 63)).all() and (~inside).sum() == 5
    again = be.ease_score_pairs(*on_device(canonical_pattern(x)), d_B, n_items, be.to_device(pp, torch.int32), be.to_device(pj, torch.int32),
                                ws_rows=ws_rows).cpu().numpy().view(np.uint64)
    assert np.array_equal(again, keys)


# ---- held-out ranks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws_rows", [0, 1, 3])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["fitted", "integer"])
def test_held_out_ranks_equal_the_definition(kind, dtype, ws_rows):
    n_items = 300
    (B, d_B), (x, _) = weights(kind, n_items, dtype), problem(n_items)
    rng = np.random.default_rng(12)
    d = rng.random((x.shape[0], n_items + 2)) < 0.03
    d[:, n_items:] = rng.random((x.shape[0], 2)) < 0.3                      # entries outside the items
    d[0, :n_items] = rng.random(n_items) < 0.2                              # the user without a history: the whole row is one tie
    d[2, x[2].indices[:3]] = True                                           # entries that not_recommend = x masks
    d[:, 5] = True                                                          # an excluded item, held out in every row
    actual, excl = sp.csr_matrix(d.astype(np.float64)), (5,)
    assert x[0].nnz == 0
    ref = ease_ranks_reference(x, B, actual, x, excl)
    be = backend()
    got = be.ease_held_out_ranks(*on_device(canonical_pattern(x)), d_B, n_items, *on_device(actual), ws_rows=ws_rows, **filters(x, excl))
    above, tied, n_adm = (v.cpu().numpy() for v in got)
    assert np.array_equal(above, ref[0]) and np.array_equal(tied, ref[1]) and np.array_equal(n_adm, ref[2])
    row0 = slice(actual.indptr[0], actual.indptr[1])
    inside0 = (actual.indices[row0] < n_items) & (actual.indices[row0] != 5)
    assert (above[row0][inside0] == 0).all() and (tied[row0][inside0] == n_items - 2).all() and n_adm[0] == n_items - 1
    assert (above[row0][~inside0] == -1).all() and (ref[0] == -1).sum() >= x.shape[0] + 3 and n_adm[-1] == 0
    if kind == "integer":
        assert (tied[above >= 0] > 0).mean() > 0.5                          # exact ties are plentiful
    unfiltered = be.ease_held_out_ranks(*on_device(canonical_pattern(x)), d_B, n_items, *on_device(actual), ws_rows=ws_rows)
    ref = ease_ranks_reference(x, B, actual)
    assert all(np.array_equal(v.cpu().numpy(), r) for v, r in zip(unfiltered, ref)) and (ref[2] == n_items).all()


# ---- the class -------------------------------------------------------------------------------------------------------------------
def split():
    test = movielens_csr()[900:].tocsr()
    held_mask = np.random.default_rng(7).random(test.nnz) < 0.5
    part = lambda keep: sp.csr_matrix((test.data[keep], test.indices[keep], np.concatenate([[0], np.cumsum(keep)])[test.indptr]), shape=test.shape)
    return part(~held_mask), part(held_mask)


@pytest.mark.parametrize("precision", ["float", "double"])
def test_the_class_on_the_device(precision):
    from rsparse_amd.metrics import hit_metrics_reference, ranking_metrics
    m = fitted(precision)
    B = m.B
    hist, held = split()
    n_items = hist.shape[1]
    cand = sp.csr_matrix(np.random.default_rng(5).random(hist.shape) < np.linspace(0.01, 0.2, hist.shape[0])[:, None])
    lens = np.diff(canonical_pattern(cand).indptr)
    assert (lens <= threshold(n_items)).any() and (lens > threshold(n_items)).any()
    top = m.predict(hist, 10, items_exclude=(49,), candidates=cand)
    ref = ease_candidates_reference(hist, B, cand, 10, hist, (49,))
    assert np.array_equal(np.asarray(top), ref[0]) and top.scores.dtype == np.float64
    assert np.array_equal(top.scores.view(np.uint64), np.where(ref[0] < 0, np.nan, ref[1]).view(np.uint64))
    sc = m.score(hist, cand)
    assert np.array_equal(sc.data.view(np.uint64), ease_score_pairs_reference(hist, B, cand).view(np.uint64))
    # the sampled protocol: the negatives are WRMF's for the seed, the metrics those of the definition's lists
    negatives = m.sample_negatives(hist, 99, actual=held, seed=7)
    theirs = WRMF(backend=backend()).sample_negatives(hist, 99, actual=held, seed=7)
    assert np.array_equal(negatives.indptr, theirs.indptr) and np.array_equal(negatives.indices, theirs.indices)
    cut = (5, 10)
    ev = m.evaluate(hist, held, cut, metrics=("hit", "ndcg"), negatives=99, seed=7)
    lists = ease_candidates_reference(hist, B, negatives, 10, hist)[0]
    hits = hit_metrics_reference(lists, held, cut, n_items)
    assert set(ev) == {"hit", "ndcg"} and np.array_equal(ev["hit"], hits["hit"], equal_nan=True)
    for t, c in enumerate(cut):
        assert np.array_equal(ev["ndcg"][:, t], ranking_metrics(lists[:, :c], held)[1], equal_nan=True)
    print("sampled protocol (99 negatives), %s: hit@10 %.3f, NDCG@10 %.3f" % (precision, np.nanmean(ev["hit"][:, 1]), np.nanmean(ev["ndcg"][:, 1])))
    # ranks: one held-out item of weight 1 per user, so every sum of the summary has one term and no order of addition
    one = sp.csr_matrix((np.ones(held.shape[0]), held.indices[held.indptr[:-1]], np.arange(held.shape[0] + 1)), shape=held.shape)
    assert (np.diff(held.indptr) > 0).all()
    rr = ease_ranks_reference(hist, B, one, hist, (49,))
    above, tied, n_adm = m.held_out_ranks(hist, one, items_exclude=(49,))
    assert np.array_equal(above.data, rr[0]) and np.array_equal(tied.data, rr[1]) and np.array_equal(n_adm, rr[2]) and above.dtype == np.int32
    ranks = m.evaluate_ranks(hist, one, items_exclude=(49,), per_user=True)
    t = lambda a, dt: torch.from_numpy(np.asarray(a)).to(dt)
    mpr, auc, mrr, sums = WRMF._rank_summary_host(t(one.indptr, torch.int32), t(one.data, torch.float64), t(rr[0], torch.int32),
                                                  t(rr[1], torch.int32), t(rr[2], torch.int32))
    sums = sums.numpy()
    tot = rank_totals({"sum_w": sums[:, 0], "sum_w_pct": sums[:, 1], "P": sums[:, 2], "auc": auc.numpy(), "mrr": mrr.numpy()})
    for name, v in (("mpr", mpr), ("auc", auc), ("mrr", mrr)):
        assert np.array_equal(ranks[name + "_per_user"], v.numpy(), equal_nan=True), name
        assert ranks[name] == tot[name] or (np.isnan(ranks[name]) and np.isnan(tot[name])), name
    assert ranks["n"] == tot["n"] == int((rr[0] >= 0).sum()) and np.array_equal(ranks["n_adm_per_user"], rr[2])
