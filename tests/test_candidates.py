"""Top-k within per-user candidate lists on the device (wrmf_candidates.hip behind rsparse_hip_top_candidates_device /
_f64_device; `WRMF.predict(..., candidates=)` / `evaluate(..., candidates=)`): exact lists and scores on integer-valued factors
against a numpy statement of the contract at every row length around the class break (64 / 65 candidates), the workgroup
strides and the LDS staging limit (2048 / 2049), every k from 1 to 8192; generic factors within the derived bound (tests/test_score_abi.py: score_bound); the same
candidates in rows of either class; the scores of `score_pairs`, bit for bit; and the class on MovieLens against `predict` with
the complement as not_recommend."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from test_score_abi import ref_scores, score_bound

pytestmark = pytest.mark.gpu

N_ROWS, N_COLS = 300, 6000
BASE_LENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025)
ZERO_SHORT, ZERO_LONG = 3, 13          # rows of 63 and of 1024 candidates whose user vector is zero (integer case)
KS = (1, 10, 64, 100, 256, 257, 1000, 8192)
CASES = [(8, np.float32), (10, np.float32), (128, np.float32), (130, np.float32), (8, np.float64), (128, np.float64)]
NA = -2147483648
GLOB = 0.5
_cache = {}


def _pattern():
    """300 x 6000: the lengths on both sides of the class break and of the 256-thread strides repeated, rows of 2047, 2048 and
    2049 (the longest row staged in LDS and the first that is not), one row of 5000, one of 6000 (every item), a trailing empty
    row; columns ascending and unique.  A not_recommend pattern that removes about a fifth
    of every row's candidates (and names items that are no candidates), and 30 excluded items.  -> (lens, p, j, nr_p, nr_j,
    excl, ok): ok[t] = position t is admissible"""
    if "pat" not in _cache:
        rng = np.random.default_rng(5)
        lens = np.tile(BASE_LENS, 20)[:N_ROWS].copy()
        lens[N_ROWS - 6:] = (2047, 2048, 2049, 5000, 6000, 0)
        assert lens[ZERO_SHORT] == 63 and lens[ZERO_LONG] == 1024
        p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        rows = [np.sort(rng.choice(N_COLS, size=l, replace=False)) for l in lens]
        j = np.concatenate(rows).astype(np.int32)
        excl = np.sort(rng.choice(N_COLS, size=30, replace=False)).astype(np.int32)
        nr_rows = []
        for c in rows:
            take = c[rng.random(c.size) < 0.2]
            other = rng.choice(N_COLS, size=5, replace=False)
            nr_rows.append(np.union1d(take, other))
        nr_p = np.concatenate([[0], np.cumsum([r.size for r in nr_rows])]).astype(np.int32)
        nr_j = np.concatenate(nr_rows).astype(np.int32)
        ok = np.concatenate([~np.isin(c, excl) & ~np.isin(c, n) for c, n in zip(rows, nr_rows)])
        assert p[-1] % 64 and 0 < ok.sum() < ok.size
        _cache["pat"] = (lens, p, j, nr_p, nr_j, excl, ok)
    return _cache["pat"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _call(U, V, k, p, j, nr_p=None, nr_j=None, excl=None, glob=0.0):
    """one call of the device entry of the factors' type on device tensors: (res, scores) as numpy"""
    from rsparse_amd import _lib
    lib = _lib.load()
    fn = lib.rsparse_hip_top_candidates_f64_device if U.dtype == torch.float64 else lib.rsparse_hip_top_candidates_device
    n, r = U.shape
    res = torch.full((n, k), 7, dtype=torch.int32, device=U.device)
    sc = torch.full((n, k), -7.0, dtype=torch.float64, device=U.device)
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(fn(U.data_ptr(), V.data_ptr(), n, int(V.shape[0]), r, k, p.data_ptr(), j.data_ptr(), ptr(nr_p), ptr(nr_j), ptr(excl),
                  0 if excl is None else int(excl.numel()), float(glob), res.data_ptr(), sc.data_ptr(), None))
    torch.cuda.synchronize()
    return res.cpu().numpy(), sc.cpu().numpy()


def _contract(s, p, j, ok, k):
    """the numpy statement: per row the admissible candidates (ascending items), kk = min(k, their number), v the kk-th best
    score, A those above v and G those equal to it; all of A plus the kk - |A| largest indices among the G items within the first
    kk of A u G in item order; best first, equal scores with the larger index first.  -> (res 1-based with NA, scores with NaN)"""
    n = p.size - 1
    res = np.full((n, k), NA, dtype=np.int32)
    sc = np.full((n, k), np.nan)
    for u in range(n):
        sl = slice(p[u], p[u + 1])
        m = ok[sl]
        it, v = j[sl][m].astype(np.int64), s[sl][m] + 0.0
        kk = min(k, it.size)
        if kk == 0:
            continue
        if kk < it.size:
            vk = np.partition(v, it.size - kk)[it.size - kk]
            ag = np.flatnonzero(v >= vk)[:kk]                    # the first kk of A u G in item order
            t = ag[v[ag] == vk]
            keep = np.concatenate([np.flatnonzero(v > vk), t[t.size - (kk - int((v > vk).sum())):]])
            it, v = it[keep], v[keep]
        o = np.lexsort((-it, -v))
        res[u, :kk], sc[u, :kk] = it[o] + 1, v[o]
    return res, sc


# ---- 1. exact, with ties ----------------------------------------------------------------------------------------------------
def _int_factors(r, dt):
    key = ("int", r, np.dtype(dt).name)
    if key not in _cache:
        rng = np.random.default_rng(200 + r)
        U = rng.integers(-2, 3, size=(N_ROWS, r)).astype(dt)
        V = rng.integers(-2, 3, size=(N_COLS, r)).astype(dt)
        U[ZERO_SHORT] = 0
        U[ZERO_LONG] = 0
        _, p, j, _, _, _, _ = _pattern()
        ref, _ = ref_scores(U, V, p, j, GLOB)                   # integers + 0.5: exact in any order
        _cache[key] = (_dev(U), _dev(V), ref)
    return _cache[key]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("r,dt", CASES)
def test_exact_lists_and_scores_on_integer_factors(r, dt, k):
    lens, p, j, nr_p, nr_j, excl, ok = _pattern()
    dU, dV, ref = _int_factors(r, dt)
    res, sc = _call(dU, dV, k, _dev(p), _dev(j), _dev(nr_p), _dev(nr_j), _dev(excl), GLOB)
    want_r, want_s = _contract(ref, p, j, ok, k)
    assert np.array_equal(res, want_r), np.flatnonzero((res != want_r).any(axis=1))[:10]
    assert np.array_equal(np.isnan(sc), want_r == NA) and np.all(sc[want_r != NA] == want_s[want_r != NA])
    for u in (ZERO_SHORT, ZERO_LONG):   # everything ties: the first kk admissible candidates in item order, largest first
        it = j[p[u]:p[u + 1]][ok[p[u]:p[u + 1]]]
        kk = min(k, it.size)
        assert np.array_equal(res[u, :kk] - 1, it[:kk][::-1]) and np.all(sc[u, :kk] == GLOB)


def test_no_exclusions_at_all():
    lens, p, j, _, _, _, _ = _pattern()
    dU, dV, ref = _int_factors(8, np.float32)
    res, sc = _call(dU, dV, 100, _dev(p), _dev(j), None, None, None, GLOB)
    want_r, want_s = _contract(ref, p, j, np.ones(j.size, bool), 100)
    assert np.array_equal(res, want_r) and np.all(sc[want_r != NA] == want_s[want_r != NA])
    assert np.array_equal((res != NA).sum(axis=1), np.minimum(100, lens))


def test_a_slice_of_the_row_pointers():
    """rows 100 .. 199 of the pattern through their slice of the row pointers (absolute slots, p[0] > 0)"""
    lens, p, j, nr_p, nr_j, excl, ok = _pattern()
    dU, dV, ref = _int_factors(10, np.float32)
    a, b = 100, 200
    res, sc = _call(dU[a:b], dV, 10, _dev(p)[a:], _dev(j), _dev(nr_p)[a:], _dev(nr_j), _dev(excl), GLOB)
    want_r, want_s = _contract(ref, p, j, ok, 10)
    assert p[a] > 0 and np.array_equal(res, want_r[a:b]) and np.all(sc[res != NA] == want_s[a:b][res != NA])


def test_backend_batches_of_rows_give_the_same_lists():
    """HipBackend.top_candidates cuts a pattern beyond its workspace budget into batches of rows (slices of the row pointers)"""
    from rsparse_amd.engine import HipBackend
    lens, p, j, nr_p, nr_j, excl, ok = _pattern()
    dU, dV, _ = _int_factors(8, np.float32)
    args = (dU, dV, 10, _dev(p), _dev(j), _dev(nr_p), _dev(nr_j), _dev(excl), GLOB)
    be = HipBackend(0)
    res, sc = be.top_candidates(*args)
    be.top_candidates_batch = 3000          # (an instance attribute: rows of 5000 and 6000 go alone, the others in groups)
    res_b, sc_b = be.top_candidates(*args)
    assert torch.equal(res, res_b) and torch.equal(sc.view(torch.int64), sc_b.view(torch.int64))
    want_r, _ = _contract(_int_factors(8, np.float32)[2], p, j, ok, 10)
    assert np.array_equal(res.cpu().numpy(), want_r)
    empty = be.top_candidates(dU, dV, 4, torch.zeros(N_ROWS + 1, dtype=torch.int32, device="cuda:0"), _dev(j)[:0], None, None, None, 0.0)
    assert bool((empty[0] == NA).all()) and bool(torch.isnan(empty[1]).all())


# ---- 2. generic factors -----------------------------------------------------------------------------------------------------
def _normal_factors(r, dt):
    key = ("normal", r, np.dtype(dt).name)
    if key not in _cache:
        rng = np.random.default_rng(100 + r)
        U = rng.standard_normal((N_ROWS, r)).astype(dt)
        V = rng.standard_normal((N_COLS, r)).astype(dt)
        _, p, j, _, _, _, _ = _pattern()
        ref, absdot = ref_scores(U, V, p, j, GLOB)
        _cache[key] = (_dev(U), _dev(V), ref, score_bound(absdot, ref, r))
    return _cache[key]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("r,dt", CASES)
def test_generic_factors_within_the_bound(r, dt, k):
    lens, p, j, nr_p, nr_j, excl, ok = _pattern()
    dU, dV, ref, tol = _normal_factors(r, dt)
    res, sc = _call(dU, dV, k, _dev(p), _dev(j), _dev(nr_p), _dev(nr_j), _dev(excl), GLOB)
    worst = 0.0
    for u in range(N_ROWS):
        sl = slice(p[u], p[u + 1])
        it, m = j[sl], ok[sl]
        kk = min(k, int(m.sum()))
        got, gs = res[u, :kk].astype(np.int64) - 1, sc[u, :kk]
        assert np.all(res[u, kk:] == NA) and np.all(np.isnan(sc[u, kk:])) and np.all(res[u, :kk] != NA), u
        if kk == 0:
            continue
        pos = np.searchsorted(it, got)
        assert np.all(pos < it.size) and np.array_equal(it[pos], got) and np.all(m[pos]) and np.unique(got).size == kk, u
        err = np.abs(gs - ref[sl][pos]) / tol[sl][pos]
        worst = max(worst, float(err.max()))
        assert np.all(err <= 1.0), (u, float(err.max()))
        assert np.all((gs[:-1] > gs[1:]) | ((gs[:-1] == gs[1:]) & (got[:-1] > got[1:]))), u
        out = m.copy()
        out[pos] = False                                         # admissible and not returned
        assert np.all(ref[sl][out] <= gs[-1] + tol[sl][out] + tol[sl][pos[-1]]), u
    print("rank %d %s k %d: max |score - ref| / bound = %.3g" % (r, np.dtype(dt).name, k, worst))


# ---- 3. independence of the row class ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 50, 64])
def test_the_same_candidates_in_rows_of_either_class(k):
    """50 admissible candidates alone, among 200 and among 3000 positions whose other entries not_recommend removes: a wave, a
    workgroup on a row staged in LDS, a workgroup on a row read from the workspace in every pass"""
    rng = np.random.default_rng(3)
    r = 8
    u = rng.integers(-2, 3, size=(1, r)).astype(np.float32)
    U = np.repeat(u, 3, axis=0)
    V = rng.integers(-2, 3, size=(N_COLS, r)).astype(np.float32)
    core = np.sort(rng.choice(N_COLS, size=50, replace=False))
    rest = np.setdiff1d(np.arange(N_COLS), core)
    rows, nrs = [core], [np.zeros(0, np.int64)]
    for n in (200, 3000):
        extra = np.sort(rng.choice(rest, size=n - 50, replace=False))
        rows.append(np.union1d(core, extra))
        nrs.append(extra)
    p = np.concatenate([[0], np.cumsum([c.size for c in rows])]).astype(np.int32)
    j = np.concatenate(rows).astype(np.int32)
    nr_p = np.concatenate([[0], np.cumsum([c.size for c in nrs])]).astype(np.int32)
    nr_j = np.concatenate(nrs).astype(np.int32)
    res, sc = _call(_dev(U), _dev(V), k, _dev(p), _dev(j), _dev(nr_p), _dev(nr_j), None, 0.0)
    assert np.array_equal(res[0], res[1]) and np.array_equal(res[0], res[2])
    assert np.array_equal(sc[0].view(np.int64), sc[1].view(np.int64)) and np.array_equal(sc[0].view(np.int64), sc[2].view(np.int64))
    ref, _ = ref_scores(U[:1], V, p[:2], j[:50], 0.0)
    want_r, want_s = _contract(ref, p[:2], j[:50], np.ones(50, bool), k)
    assert np.array_equal(res[0], want_r[0]) and np.all(sc[0][want_r[0] != NA] == want_s[0][want_r[0] != NA])
    assert np.unique(ref).size < 50          # the scores do tie


# ---- 4. consistency with score_pairs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,dt", [(10, np.float32), (128, np.float32), (128, np.float64)])
def test_scores_are_those_of_score_pairs_and_calls_repeat(r, dt):
    from rsparse_amd import _lib
    lib = _lib.load()
    lens, p, j, nr_p, nr_j, excl, ok = _pattern()
    dU, dV, _, _ = _normal_factors(r, dt)
    dp, dj = _dev(p), _dev(j)
    args = (dU, dV, 100, dp, dj, _dev(nr_p), _dev(nr_j), _dev(excl), GLOB)
    res, sc = _call(*args)
    res2, sc2 = _call(*args)
    assert np.array_equal(res, res2) and np.array_equal(sc.view(np.int64), sc2.view(np.int64))
    pairs = torch.empty(j.size, dtype=torch.float64, device="cuda:0")
    fn = lib.rsparse_hip_score_pairs_f64_device if dt == np.float64 else lib.rsparse_hip_score_pairs_device
    _lib.check(fn(dU.data_ptr(), dV.data_ptr(), N_ROWS, N_COLS, r, dp.data_ptr(), dj.data_ptr(), GLOB, None, pairs.data_ptr(), None,
                  None, None))
    torch.cuda.synchronize()
    pairs = pairs.cpu().numpy() + 0.0        # (the lists hold +0 for a score of -0)
    for u in range(N_ROWS):
        got = res[u][res[u] != NA].astype(np.int64) - 1
        pos = p[u] + np.searchsorted(j[p[u]:p[u + 1]], got)
        assert np.array_equal(sc[u, :got.size].view(np.int64), pairs[pos].view(np.int64)), u


# ---- 5. the class, on MovieLens ---------------------------------------------------------------------------------------------
MODELS = {
    "float": dict(rank=10, lambda_=0.1, feedback="explicit", solver="cholesky", with_user_item_bias=True, with_global_bias=True,
                  precision="float"),
    "double": dict(rank=10, lambda_=0.1, feedback="implicit", solver="cholesky", precision="double"),
}


@pytest.mark.parametrize("name", list(MODELS))
def test_class_on_movielens(ml_train, name):
    from rsparse_amd import WRMF
    from rsparse_amd.metrics import ap_k, ndcg_k
    n_user, n_item, cp, ci, cx = ml_train
    train = sp.csc_matrix((cx, ci, cp), shape=(n_user, n_item)).tocsr()
    model = WRMF(rng=1, **MODELS[name])
    model.fit_transform(train, n_iter=3, convergence_tol=-1)
    n = 200
    x = train[:n]
    rng = np.random.default_rng(7)
    # (100 candidates per user among the items with at least 10 ratings: two items with the same ratings by the same users --
    # MovieLens has dozens rated once -- get the same factors, and their scores tie exactly for every user)
    pool = np.flatnonzero(np.diff(train.tocsc().indptr) >= 10)
    cols = np.concatenate([np.sort(rng.choice(pool, size=100, replace=False)) for _ in range(n)])
    cand = sp.csr_matrix((np.zeros(cols.size), cols, np.arange(0, 100 * n + 1, 100)), shape=(n, n_item))
    inx = np.zeros((n, n_item), bool)
    inx[np.repeat(np.arange(n), np.diff(x.indptr)), x.indices] = True
    inc = np.zeros((n, n_item), bool)
    inc[np.repeat(np.arange(n), 100), cols] = True
    # the float64 reference: rows whose neighbouring scores among the best 11 admissible candidates are closer than twice the bound
    emb = model.transform(x).astype(np.float64)
    comp = np.asarray(model.components, dtype=np.float64)
    r = comp.shape[0]
    S = emb @ comp + model.global_bias
    B = score_bound(np.abs(emb) @ np.abs(comp), S, r)
    adm = inc & ~inx
    skip = np.zeros(n, bool)
    for u in range(n):
        it = np.flatnonzero(adm[u])
        o = it[np.argsort(-S[u, it], kind="stable")][:11]
        gaps = S[u, o[:-1]] - S[u, o[1:]]
        skip[u] = bool(np.any(gaps <= 2.0 * np.maximum(B[u, o[:-1]], B[u, o[1:]])))
    assert skip.sum() == 0                       # (CPU side: the seed-fixed candidates leave no near-tie)
    assert skip.mean() <= 0.01
    got = model.predict(x, 10, candidates=cand)
    want = model.predict(x, 10, not_recommend=sp.csr_matrix((inx | ~inc).astype(np.float64)))
    assert np.array_equal(np.asarray(got)[~skip], np.asarray(want)[~skip])
    assert np.array_equal((np.asarray(got) >= 0).sum(axis=1), np.minimum(10, adm.sum(axis=1)))
    # evaluate: the metrics of those lists, bit for bit
    held = train[:n].copy()
    held.data[::3] = 0.0                         # (stored zeros: relevant items of relevance 0)
    ev = model.evaluate(x, held, 10, not_recommend=None, candidates=cand)
    top = model.predict(x, 10, not_recommend=None, candidates=cand)
    assert np.array_equal(ev["ap"], ap_k(top, held), equal_nan=True) and np.array_equal(ev["ndcg"], ndcg_k(top, held), equal_nan=True)
    # an empty pattern: every list is empty, without a launch
    none = model.predict(x, 3, candidates=sp.csr_matrix((n, n_item)))
    assert (np.asarray(none) == -1).all() and np.isnan(none.scores).all()
