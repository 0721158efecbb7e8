"""Full-ranking counts on the device (wrmf_ranks.hip behind rsparse_hip_held_out_ranks_device / rsparse_hip_rank_summary_device;
`WRMF.held_out_ranks`, `WRMF.evaluate_ranks`): exact against numpy on integer-valued factors at every kernel path and batch
boundary, bracketed by the fp32 dot product's error bound on real-valued ones, repeat calls bit for bit, the summary kernel
against rsparse_amd.metrics.rank_summary, and the class on MovieLens -- tied to `predict`'s lists."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

from rsparse_amd._lib import RANKS_BATCH as T

LENS = (0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3)
_cache = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _backend():
    from rsparse_amd.engine import HipBackend
    if "be" not in _cache:
        _cache["be"] = HipBackend(0)
    return _cache["be"]


def _counts(S, adm, p, j):
    """numpy: (above, tied, n_adm) of the entries (p, j) from the scores S and the admissibility mask, by sorting each row"""
    above = np.full(j.size, -1, dtype=np.int64)
    tied = np.full(j.size, -1, dtype=np.int64)
    for u in range(S.shape[0]):
        srt = np.sort(S[u][adm[u]])
        h = j[p[u]:p[u + 1]]
        ok = adm[u, h]
        lo, hi = np.searchsorted(srt, S[u, h], "left"), np.searchsorted(srt, S[u, h], "right")
        above[p[u]:p[u + 1]] = np.where(ok, srt.size - hi, -1)
        tied[p[u]:p[u + 1]] = np.where(ok, hi - lo - 1, -1)
    return above, tied, adm.sum(axis=1)


def _integer_case(rank, n, m):
    """factors from {-3..3}: every score is an integer of magnitude <= 9 rank <= 2304, exact in fp32 whatever the order of the sum.
    user 0 has a zero embedding (every item ties), user 1 has every item in not_recommend (n_adm = 0); the held-out rows cycle
    through the lengths around the wave and the batch boundaries (capped at the items there are); a tenth of every row is in
    not_recommend, held-out items included, and three items are excluded for everybody."""
    key = (rank, n, m)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(1000 * rank + 10 * n + m)
    U = rng.integers(-3, 4, size=(n, rank)).astype(np.float32)
    V = rng.integers(-3, 4, size=(m, rank)).astype(np.float32)
    U[0] = 0.0
    lens = [min(LENS[(u + 3) % len(LENS)] if n > 3 else (2 * T + 3, T, 65)[u], m) for u in range(n)]
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    j = np.concatenate([np.sort(rng.choice(m, size=l, replace=False)) for l in lens]).astype(np.int32)
    nr = rng.random((n, m)) < 0.1
    nr[1] = True
    excl = np.array(sorted({1, 5 % m, m - 1}), dtype=np.int32)
    adm = ~nr
    adm[:, excl] = False
    nr = sp.csr_matrix(nr)
    S = U.astype(np.int64) @ V.astype(np.int64).T
    assert np.abs(S).max() <= 9 * rank
    w = rng.integers(0, 6, size=j.size).astype(np.float64)          # weights with stored zeros
    _cache[key] = dict(U=U, V=V, p=p, j=j, w=w, nr_p=nr.indptr.astype(np.int32), nr_j=nr.indices.astype(np.int32), excl=excl,
                       ref=_counts(S, adm, p, j))
    return _cache[key]


def _call(c, max_chunk_users=0, U=None, V=None):
    be = _backend()
    above, tied, n_adm = be.held_out_ranks(_dev(c["U"] if U is None else U), _dev(c["V"] if V is None else V), _dev(c["nr_p"]),
                                           _dev(c["nr_j"]), _dev(c["excl"]), _dev(c["p"]), _dev(c["j"]), max_chunk_users)
    torch.cuda.synchronize()
    return above, tied, n_adm


@pytest.mark.parametrize("m", [37, 1024, 4099])
@pytest.mark.parametrize("n", [3, 130])
@pytest.mark.parametrize("rank", [8, 50, 128, 160])
def test_exact_against_numpy_integers(rank, n, m):
    c = _integer_case(rank, n, m)
    ra, rt, rn = c["ref"]
    above, tied, n_adm = _call(c)
    a, t, na = above.cpu().numpy(), tied.cpu().numpy(), n_adm.cpu().numpy()
    assert a.dtype == np.int32 and t.dtype == np.int32 and na.dtype == np.int32
    assert np.array_equal(na, rn), np.flatnonzero(na != rn)[:5]
    assert np.array_equal(a, ra), np.flatnonzero(a != ra)[:5]
    assert np.array_equal(t, rt), np.flatnonzero(t != rt)[:5]
    # the cases the construction promises
    p = c["p"]
    if p[1] > p[0]:
        z = slice(p[0], p[1])
        assert np.all((a[z] == 0) & (t[z] == na[0] - 1) | (a[z] == -1))          # the zero embedding ties every item
    assert na[1] == 0 and np.all(a[p[1]:p[2]] == -1) and np.all(t[p[1]:p[2]] == -1)
    assert (a == -1).any() and (a >= 0).any() and np.array_equal(a == -1, t == -1)
    # several chunks of users, and a repeated call: the same bits
    a64, t64, n64 = _call(c, max_chunk_users=64)
    assert torch.equal(a64, above) and torch.equal(t64, tied) and torch.equal(n64, n_adm)
    a2, t2, n2 = _call(c)
    assert torch.equal(a2, above) and torch.equal(t2, tied) and torch.equal(n2, n_adm)


def test_no_exclusions_and_an_empty_pattern():
    c = dict(_integer_case(8, 3, 37))
    be = _backend()
    S = c["U"].astype(np.int64) @ c["V"].astype(np.int64).T
    ra, rt, rn = _counts(S, np.ones(S.shape, bool), c["p"], c["j"])
    above, tied, n_adm = be.held_out_ranks(_dev(c["U"]), _dev(c["V"]), None, None, None, _dev(c["p"]), _dev(c["j"]))
    assert np.array_equal(above.cpu().numpy(), ra) and np.array_equal(tied.cpu().numpy(), rt)
    assert np.array_equal(n_adm.cpu().numpy(), rn) and (rn == 37).all()
    p0 = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    above, tied, n_adm = be.held_out_ranks(_dev(c["U"]), _dev(c["V"]), None, None, None, p0, p0[:0])
    assert above.numel() == 0 and tied.numel() == 0 and n_adm.cpu().tolist() == [37, 37, 37]


@pytest.mark.parametrize("rank,n,m", [(8, 130, 4099), (128, 3, 4099), (50, 130, 37)])
def test_summary_kernel_against_numpy_on_the_device_counts(rank, n, m):
    """mrr, auc and the count are sums of half-integers: exact.  sum w, sum w pct and mpr: a fixed-order double sum of
    non-negative terms against numpy's, within 2 (len + 2) 2^-52 relative (tests/test_score.py::_check_sums)"""
    from rsparse_amd.metrics import rank_summary
    c = _integer_case(rank, n, m)
    above, tied, n_adm = _call(c)
    be = _backend()
    mpr, auc, mrr, sums = (v.cpu().numpy() for v in be.rank_summary(_dev(c["p"]), _dev(c["w"]), above, tied, n_adm))
    act = sp.csr_matrix((c["w"], c["j"], c["p"]), shape=(n, m))
    ref = rank_summary(above.cpu().numpy(), tied.cpu().numpy(), n_adm.cpu().numpy(), act)
    rel = 2.0 * (np.diff(c["p"]) + 2) * 2.0 ** -52
    got = {"mpr": mpr, "auc": auc, "mrr": mrr, "sum_w": sums[:, 0], "sum_w_pct": sums[:, 1], "P": sums[:, 2]}
    for name, v in got.items():
        want = ref[name]
        assert np.array_equal(np.isnan(v), np.isnan(want)), name
        ok = ~np.isnan(want)
        err = np.abs(v[ok] - want[ok])
        print("%s: max err / bound = %.3g" % (name, float(np.max(err / np.maximum(rel[ok] * np.abs(want[ok]), 1e-300), initial=0.0))))
        assert np.all(err <= rel[ok] * np.abs(want[ok])), (name, int(np.argmax(err)))
    assert np.isnan(mpr).any() and np.isnan(auc).any() and (~np.isnan(mpr)).any()
    # any output may be left out, and a repeated call returns the same bits
    from rsparse_amd import _lib
    only = torch.full((n,), -7.0, dtype=torch.float64, device="cuda:0")
    _lib.check(be.lib.rsparse_hip_rank_summary_device(n, _dev(c["p"]).data_ptr(), None, above.data_ptr(), tied.data_ptr(),
                                                      n_adm.data_ptr(), None, only.data_ptr(), None, None, None))
    torch.cuda.synchronize()
    assert np.array_equal(only.cpu().numpy().view(np.int64), auc.view(np.int64))
    again = be.rank_summary(_dev(c["p"]), _dev(c["w"]), above, tied, n_adm)
    for v, w in zip(again, (mpr, auc, mrr, sums)):
        assert np.array_equal(v.cpu().numpy().view(np.int64), w.view(np.int64))


@pytest.mark.parametrize("rank", [64, 128])
def test_real_valued_factors_within_the_fp32_dot_product_bound(rank):
    """standard-normal factors: the fp32 score of item j is within e_j = (rank + 2) 2^-24 sum_k |u_k v_jk| of the double one (the
    standard bound for an fp32 dot product of that length, in any order of summation), so an item counts as above h for certain
    when its double score exceeds h's by more than e_j + e_h and cannot when it falls short by more than that"""
    rng = np.random.default_rng(rank)
    n, m = 40, 3000
    U = rng.standard_normal((n, rank)).astype(np.float32)
    V = rng.standard_normal((m, rank)).astype(np.float32)
    lens = rng.integers(0, 40, size=n)
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    j = np.concatenate([np.sort(rng.choice(m, size=l, replace=False)) for l in lens]).astype(np.int32)
    nr = sp.csr_matrix(rng.random((n, m)) < 0.05)
    excl = np.array([0, 7, 2999], dtype=np.int32)
    adm = ~nr.toarray()
    adm[:, excl] = False
    c = dict(U=U, V=V, p=p, j=j, nr_p=nr.indptr.astype(np.int32), nr_j=nr.indices.astype(np.int32), excl=excl)
    above, tied, n_adm = (v.cpu().numpy() for v in _call(c))
    S = U.astype(np.float64) @ V.astype(np.float64).T
    E = (rank + 2) * 2.0 ** -24 * (np.abs(U).astype(np.float64) @ np.abs(V).astype(np.float64).T)
    assert np.array_equal(n_adm, adm.sum(axis=1))
    worst = 0
    for u in range(n):
        for e in range(p[u], p[u + 1]):
            h = j[e]
            if not adm[u, h]:
                assert above[e] == -1 and tied[e] == -1
                continue
            others = adm[u].copy()
            others[h] = False
            d, tol = (S[u] - S[u, h])[others], (E[u] + E[u, h])[others]
            lo_gt, hi_gt = int(np.sum(d > tol)), int(np.sum(d > -tol))
            lo_ge, hi_ge = int(np.sum(d >= tol)), int(np.sum(d >= -tol))
            assert lo_gt <= above[e] <= hi_gt, (u, e, lo_gt, above[e], hi_gt)
            assert lo_ge <= above[e] + tied[e] <= hi_ge, (u, e, lo_ge, above[e] + tied[e], hi_ge)
            worst = max(worst, hi_gt - lo_gt)
    print("rank %d: widest bracket %d items" % (rank, worst))


# ---- the class, on MovieLens ------------------------------------------------------------------------------------------------
def _ml(ml_train, precision):
    from rsparse_amd import WRMF
    key = ("ml", precision)
    if key not in _cache:
        n_user, n_item, p, i, x = ml_train
        train = sp.csc_matrix((x, i, p), shape=(n_user, n_item)).tocsr()
        model = WRMF(rank=10, lambda_=0.1, feedback="implicit", solver="cholesky", precision=precision, rng=1)
        model.fit_transform(train, n_iter=3, convergence_tol=-1)
        seen, held = train[:200].copy(), train[:200].copy()
        seen.data[1::2] = 0.0
        held.data[0::2] = 0.0
        seen.eliminate_zeros(); held.eliminate_zeros()
        _cache[key] = (model, seen, held)
    return _cache[key]


@pytest.mark.parametrize("precision", ["float", "double"])
def test_class_on_movielens(ml_train, precision):
    from rsparse_amd.metrics import canonical_actual, rank_totals
    model, seen, held = _ml(ml_train, precision)
    be = model._backend()
    excl = [3, 10]
    # some held-out entries are not admissible: every seventh of them joins not_recommend
    extra = held.copy()
    extra.data[:] = 0.0
    extra.data[::7] = 1.0
    extra.eliminate_zeros()
    nr = (seen + extra).tocsr()
    above, tied, n_adm = model.held_out_ranks(seen, held, not_recommend=nr, items_exclude=excl)
    pat = canonical_actual(held, held.shape[0])
    assert np.array_equal(above.indices, pat.indices) and np.array_equal(above.indptr, pat.indptr) and above.dtype == np.int32
    masked = nr.toarray() != 0
    masked[:, excl] = True
    bad = masked[np.repeat(np.arange(held.shape[0]), np.diff(pat.indptr)), pat.indices]
    assert bad.sum() >= extra.nnz and np.array_equal(above.data == -1, bad) and np.array_equal(tied.data == -1, bad)
    assert np.array_equal(n_adm, (~masked).sum(axis=1))
    # the backend call on the embeddings `transform` computes: bit for bit
    emb = model._transform_device(sp.csr_matrix(seen, dtype=np.float64))
    nrs = nr.copy()
    nrs.sort_indices()
    d = lambda a, t: be.to_device(a, t)
    ba, bt, bn = be.held_out_ranks(emb, model._V, d(nrs.indptr, torch.int32), d(nrs.indices, torch.int32),
                                   d(np.array(excl), torch.int32), d(pat.indptr, torch.int32), d(pat.indices, torch.int32))
    assert np.array_equal(ba.cpu().numpy(), above.data) and np.array_equal(bt.cpu().numpy(), tied.data)
    assert np.array_equal(bn.cpu().numpy(), n_adm)
    # evaluate_ranks is the summary of these counts: bit for bit
    mpr, auc, mrr, sums = (v.cpu().numpy() for v in be.rank_summary(d(pat.indptr, torch.int32), d(pat.data, torch.float64), ba, bt, bn))
    ev = model.evaluate_ranks(seen, held, not_recommend=nr, items_exclude=excl, per_user=True)
    bits = lambda v: np.asarray(v, dtype=np.float64).view(np.int64)
    assert np.array_equal(bits(ev["mpr_per_user"]), bits(mpr)) and np.array_equal(bits(ev["auc_per_user"]), bits(auc))
    assert np.array_equal(bits(ev["mrr_per_user"]), bits(mrr)) and np.array_equal(ev["n_adm_per_user"], n_adm)
    tot = rank_totals({"sum_w": sums[:, 0], "sum_w_pct": sums[:, 1], "P": sums[:, 2], "auc": auc, "mrr": mrr})
    plain = model.evaluate_ranks(seen, held, not_recommend=nr, items_exclude=excl)
    for name in ("mpr", "auc", "mrr", "n"):
        assert ev[name] == tot[name] == plain[name], name
    assert ev["n"] == int((~bad).sum())
    print("%s: mpr %.4f auc %.4f mrr %.4f over %d entries" % (precision, ev["mpr"], ev["auc"], ev["mrr"], ev["n"]))
    assert 0.0 < ev["mpr"] < 0.5 < ev["auc"] < 1.0           # a fitted model beats the 0.5 of a random order


@pytest.mark.parametrize("precision", ["float", "double"])
def test_above_is_the_position_in_predicts_list(ml_train, precision):
    """k = every item (1682 <= 8192): the list of `predict` holds the admissible items best first, so a held-out item sits at
    position `above` -- wherever the order of its score among the others is beyond doubt.  `predict` orders by scores
    recomputed in double (from the double factors of a double model), the counts by the fp32 scores of the fp32 factors: both
    place item h alike when no other admissible score is within e_j + e_h of it, e = (rank + 4) 2^-24 sum_k |u_k v_k| (the fp32
    dot product's bound plus one rounding of each factor).  Such entries are compared, the others are counted: e is about 1e-6
    of the score's scale and 1682 scores lie about 1e-3 apart, so all but a few per cent of the entries qualify."""
    model, seen, held = _ml(ml_train, precision)
    n_item = held.shape[1]
    above, tied, n_adm = model.held_out_ranks(seen, held)
    top = np.asarray(model.predict(seen, n_item))
    emb = model.transform(seen).astype(np.float64)
    comp = np.asarray(model.components, dtype=np.float64)
    S = emb @ comp
    E = (comp.shape[0] + 4) * 2.0 ** -24 * (np.abs(emb) @ np.abs(comp))
    adm = np.ones(S.shape, bool)
    adm[seen.nonzero()] = False
    checked = 0
    for u in range(held.shape[0]):
        assert np.array_equal(top[u] >= 0, np.arange(n_item) < n_adm[u])
        pos = np.full(n_item, -1)
        pos[top[u, :n_adm[u]]] = np.arange(n_adm[u])
        for e in range(above.indptr[u], above.indptr[u + 1]):
            h = above.indices[e]
            others = adm[u].copy()
            others[h] = False
            if np.all(np.abs(S[u] - S[u, h])[others] > (E[u] + E[u, h])[others]):
                assert tied.data[e] == 0 and pos[h] == above.data[e], (u, h, pos[h], above.data[e])
                checked += 1
    print("%s: %d of %d entries beyond doubt" % (precision, checked, above.nnz))
    assert checked > above.nnz // 2
