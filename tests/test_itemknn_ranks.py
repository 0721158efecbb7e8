"""The rank count of wrmf_itemknn.hip (knn_ranks_kernel) against rsparse_amd.itemknn.knn_ranks_reference, through HipBackend and
through `ItemKNN.held_out_ranks` / `evaluate_ranks`: every comparison is np.array_equal.  Held-out rows at the edges of the
kernel's batches of RSPARSE_HIP_RANKS_BATCH entries on a catalogue larger than a batch, inadmissible entries of every kind, tied
scores, a row with nothing admissible; and, on a catalogue `knn_recommend` can list whole, the counts recomputed from its lists."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import ItemKNN, WRMF, _lib
from rsparse_amd.itemknn import canonical_pattern, knn_ranks_reference, knn_recommend_reference, knn_score_pairs_reference
from rsparse_amd.metrics import canonical_actual, rank_totals
from test_itemknn_candidates import KINDS, N_BIG, backend, device_filters, device_lists, device_operands, problem, rows_pattern

pytestmark = pytest.mark.gpu

BATCH = _lib.RANKS_BATCH


def device_ranks(name, kind, actual, nr=None, excl=(), ws_rows=0):
    """`actual` may have more columns than the model has items: those entries are out of range"""
    be = backend()
    x, nb, q, xv = problem(name, kind)
    rows, kw = device_operands(x, nb, q, xv)
    act = canonical_actual(actual, x.shape[0])
    got = be.knn_held_out_ranks(*rows, be.to_device(act.indptr, torch.int32), be.to_device(act.indices, torch.int32), ws_rows=ws_rows,
                                **device_filters(nr, excl), **kw)
    torch.cuda.synchronize()
    assert all(t.dtype == torch.int32 for t in got)
    return tuple(t.cpu().numpy() for t in got)


@functools.lru_cache(maxsize=None)
def big_case(kind):
    """the held-out rows of the large catalogue (12 users) -> (actual with 10 columns beyond the items, nr, excl): rows of 0, 1, 2,
    BATCH and BATCH + 1 entries; a row whose entries lie in not_recommend, in items_exclude and outside the items beside two
    admissible ones; a row where everything is masked; a row of 2 BATCH + 7 entries; the user without a history"""
    x, nb, q, xv = problem("big", kind)
    rng = np.random.default_rng(17)
    excl = (7, 64, N_BIG - 1)
    nr = x.tolil(copy=True)
    nr[6, :] = 1                                                            # nothing admissible
    nr = sp.csr_matrix(nr)
    pick = lambda n: rng.choice(N_BIG, size=n, replace=False)
    own5 = x[5].indices
    mixed = np.concatenate([own5[:2], excl, [N_BIG, N_BIG + 9], np.setdiff1d(np.arange(100, 110), own5)[:2]])
    rows = [pick(40), pick(0), pick(1), pick(2), pick(BATCH), mixed, pick(3), pick(BATCH + 1), pick(2 * BATCH + 7), pick(5),
            pick(BATCH - 1), pick(64)]
    return rows_pattern(rows, N_BIG + 10), nr, excl


@pytest.mark.parametrize("ws_rows", (0, 1, 3))
@pytest.mark.parametrize("kind", KINDS)
def test_held_out_rows_at_the_batch_edges(kind, ws_rows):
    x, nb, q, xv = problem("big", kind)
    actual, nr, excl = big_case(kind)
    above, tied, n_adm = device_ranks("big", kind, actual, nr, excl, ws_rows)
    ref = knn_ranks_reference(x, nb, q, actual, nr, excl, xv=xv)
    assert np.array_equal(above, ref[0]) and np.array_equal(tied, ref[1]) and np.array_equal(n_adm, ref[2])
    p = actual.indptr
    assert np.diff(p).tolist() == [40, 0, 1, 2, BATCH, 9, 3, BATCH + 1, 2 * BATCH + 7, 5, BATCH - 1, 64]
    # the inadmissible entries of row 5 -- two of its own items, the three excluded, the two outside the items -- and no others
    row5 = slice(p[5], p[6])
    assert (above[row5] == -1).sum() == 7 and np.array_equal(above[row5] == -1, tied[row5] == -1) and (above[row5] >= 0).sum() == 2
    # nothing admissible in row 6
    assert n_adm[6] == 0 and (above[p[6]:p[7]] == -1).all() and (tied[p[6]:p[7]] == -1).all()
    assert n_adm[0] == N_BIG - len(excl) and n_adm[1] == N_BIG - np.union1d(x[1].indices, excl).size
    # held-out items tied with each other: the many of score 0 in a long row, each counted in the other's `tied`
    long_row = slice(p[8], p[9])
    zero = (above[long_row] >= 0) & (tied[long_row] > 1000)
    assert zero.sum() > BATCH and len(set(tied[long_row][zero])) == 1
    # the user without a history: every admissible item ties at 0
    assert (above[p[0]:p[1]][above[p[0]:p[1]] >= 0] == 0).all() and (tied[p[0]:p[1]].max() == n_adm[0] - 1)
    again = device_ranks("big", kind, actual, nr, excl, ws_rows)
    assert all(np.array_equal(a, b) for a, b in zip((above, tied, n_adm), again))        # a repeated call: the same bits
    k = 50
    got, plain = device_lists("big", kind, k), knn_recommend_reference(x, nb, q, k, None, (), xv=xv)
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])        # the workspace was left all zeros


@pytest.mark.parametrize("kind", KINDS)
def test_counts_recomputed_from_the_full_lists(kind):
    """the planted matrix (300 items): `knn_recommend` at k = n_items lists every admissible item with its score, and above / tied
    follow from a list by counting.  Items 10 and 11 have the same users: held out together, they tie at a positive score."""
    x, nb, q, xv = problem("planted", kind)
    n, n_items = x.shape
    rng = np.random.default_rng(23)
    d = (rng.random(x.shape) < 0.05) & (x.toarray() == 0)
    d[:, 10:12] = True
    actual = sp.csr_matrix(d.astype(np.float64))
    excl = (0, 299)
    above, tied, n_adm = device_ranks("planted", kind, actual, x, excl)
    ref = knn_ranks_reference(x, nb, q, actual, x, excl, xv=xv)
    assert np.array_equal(above, ref[0]) and np.array_equal(tied, ref[1]) and np.array_equal(n_adm, ref[2])
    items, scores = device_lists("planted", kind, n_items, x, excl)
    assert np.array_equal((items >= 0).sum(axis=1), n_adm)
    both = 0
    for u in range(n):
        listed, s = items[u, :n_adm[u]], scores[u, :n_adm[u]]
        for e in range(actual.indptr[u], actual.indptr[u + 1]):
            at = np.flatnonzero(listed == actual.indices[e])
            if at.size == 0:
                assert above[e] == -1 and tied[e] == -1
                continue
            assert above[e] == (s > s[at[0]]).sum() and tied[e] == (s == s[at[0]]).sum() - 1
        e10 = actual.indptr[u] + np.searchsorted(actual[u].indices, 10)
        if above[e10] >= 0 and above[e10 + 1] >= 0 and above[e10] == above[e10 + 1] and s[np.flatnonzero(listed == 10)[0]] > 0:
            assert tied[e10] == tied[e10 + 1] >= 1
            both += 1
    assert both > 0


@pytest.mark.parametrize("weighting", (None, "values"))
def test_the_class_on_the_device(weighting):
    """`held_out_ranks` and `evaluate_ranks` of a fitted model against the definitions.  The summary is compared bit for bit with
    `WRMF._rank_summary_host` fed the reference counts on a leave-one-out `actual` of weight 1: with one entry per user every sum
    of the summary has a single term, so its value does not depend on the order in which a backend adds."""
    rng = np.random.default_rng(29)
    x = problem("planted", "binary")[0].copy()
    x.data = rng.integers(1, 6, size=x.nnz).astype(np.float64)
    model = ItemKNN(k_neighbors=20, similarity="cosine", weighting=weighting).fit(x)
    n, n_items = x.shape
    dense = x.toarray() != 0
    held = np.array([rng.choice(np.flatnonzero(~dense[u])) for u in range(n)])
    held[:3] = (10, 0, 11)                                                 # (user 1's is excluded below: no admissible entry)
    actual = sp.csr_matrix((np.ones(n), held, np.arange(n + 1)), shape=x.shape)
    excl = (0,)
    be = model._backend()
    m = canonical_pattern(x)
    xq = model._row_weights(m, be)
    ref = knn_ranks_reference(x, model.neighbors, model._weights(), actual, x, excl, xv=xq)
    above, tied, n_adm = model.held_out_ranks(x, actual, items_exclude=excl)
    assert np.array_equal(above.data, ref[0]) and np.array_equal(tied.data, ref[1]) and np.array_equal(n_adm, ref[2])
    assert np.array_equal(above.indices, actual.indices) and above.dtype == np.int32 and ref[0][1] == -1 and (ref[0] >= 0).sum() > n // 2
    ev = model.evaluate_ranks(x, actual, items_exclude=excl, per_user=True)
    t = lambda a, dt: torch.from_numpy(np.asarray(a)).to(dt)
    mpr, auc, mrr, sums = WRMF._rank_summary_host(t(actual.indptr, torch.int32), t(actual.data, torch.float64), t(ref[0], torch.int32),
                                                  t(ref[1], torch.int32), t(ref[2], torch.int32))
    sums = sums.numpy()
    tot = rank_totals({"sum_w": sums[:, 0], "sum_w_pct": sums[:, 1], "P": sums[:, 2], "auc": auc.numpy(), "mrr": mrr.numpy()})
    assert set(ev) == {"mpr", "auc", "mrr", "n", "mpr_per_user", "auc_per_user", "mrr_per_user", "n_adm_per_user"}
    for name, v in (("mpr", mpr), ("auc", auc), ("mrr", mrr)):
        assert np.array_equal(ev[name + "_per_user"], v.numpy(), equal_nan=True), name
        assert ev[name] == tot[name], name
    assert ev["n"] == tot["n"] == int((ref[0] >= 0).sum()) and np.array_equal(ev["n_adm_per_user"], ref[2])
    # the score at the held-out cells orders them as the counts say
    sc = model.score(x, actual)
    raw = knn_score_pairs_reference(x, model.neighbors, model._weights(), actual, xv=xq)
    assert np.array_equal(sc.data, model._scale(raw)) and np.array_equal(sc.indices, actual.indices)
