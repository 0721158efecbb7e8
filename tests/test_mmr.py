"""MMR re-ranking on the MI355X (wrmf_mmr.hip) against the numpy definition `rsparse_amd.metrics.mmr_reference`.

The acceptance rule is "eps-greedy along its own path": the definition is replayed in numpy with the device's picks as the prefix
(`replay` of tests/test_mmr_host.py); at every step the device's pick must be valid and untaken, its reference objective within
EPS = 1e-12 of the step's maximum, and the returned `objective` within 1e-12 of the reference value (the bound of DESIGN.md 3.24
at r = 256 is about 3e-14).  On top of that the lists must equal the reference's own, item for item, wherever the reference's
smallest winning margin along its path exceeds MARGIN = 1e-9 or is an exact tie (which the tie rule decides: the lower position);
the lists exempt from that equality may be at most 1 % of a test's lists, which the test asserts -- the inputs are chosen so
that there is none.

Shapes: the pools around the 64 lanes of a wave and the batch of the lane groups (fewer positions than groups, one batch, several),
k = 1 and k = N, one user at a pool of 8192 (LDS beyond 64 KiB), every lane-group width (ranks 1 .. 256), the misaligned scalar
path (a window from column 1) and both factor types.  Then lists with NA, 0, n_item + 1, negative and repeated
entries, NaN and infinite scores, degenerate items, an all-invalid row and a row with fewer valid positions than k; duplicated
factor rows; a repeated call; each nullable output alone; the host form; and the class on the movielens fixture."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from test_list_metrics import DEGENERATE, NEAR, TINY, _factors, _lists, _windows
from test_metrics_abi import NA
from test_mmr_host import replay, unit_rows

pytestmark = pytest.mark.gpu

EPS = 1e-12
MARGIN = 1e-9
SHAPES = [(1, 1), (2, 2), (16, 5), (63, 10), (64, 64), (65, 10), (100, 10), (257, 20), (1000, 50)]
RANKS = [1, 3, 4, 5, 8, 16, 17, 32, 33, 64, 100, 128, 129, 256]
WANT = ("scores", "positions", "objective")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref))


def _thetas(rank):
    # rank 1: every cosine is +-1 to within an ulp, so theta = 1 makes every step a near-tie; theta = 0 has no dot product in it
    return (0.3, 0.7) if rank == 1 else (0.0, 0.3, 0.7, 1.0)


def _torch_type(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _run(be, res, sc, V, c0, c1, k, theta, want=WANT):
    return {m: v.cpu().numpy() for m, v in be.mmr_rerank(res, sc, V, c0, c1, k, theta, want).items()}


def _check(got, pred1, sc, Vh, c0, c1, k, theta, case):
    """the acceptance rule of the module's docstring for one call -> the number of lists exempt from the item-for-item equality"""
    from rsparse_amd.metrics import mmr_reference
    n, N = pred1.shape
    pred0 = pred1.astype(np.int64) - 1                                        # (NA and 0 turn negative)
    unit = unit_rows(Vh, c0, c1)
    ref = mmr_reference(pred0, sc, k, theta, Vh, c0, c1)
    assert got["items"].dtype == np.int32 and got["positions"].dtype == np.int32 and got["items"].shape == (n, k), case
    assert got["scores"].dtype == np.float64 and got["objective"].dtype == np.float64, case
    none = got["positions"] == NA
    pos = np.where(none, -1, got["positions"].astype(np.int64) - 1)
    assert ((pos >= -1) & (pos < N)).all(), case
    at = np.where(none, 0, pos)
    assert np.array_equal(got["items"], np.where(none, NA, np.take_along_axis(pred1, at, axis=1))), case
    assert _same(got["scores"], np.where(none, np.nan, np.take_along_axis(sc, at, axis=1))), case
    assert np.array_equal(np.isnan(got["objective"]), none), case
    exempt, worst_gap, worst_obj, low = 0, 0.0, 0.0, np.inf
    for u in range(n):
        steps = replay(pred0[u], sc[u], unit, theta, pos[u])
        for t, (ok, obj, best, _) in enumerate(steps):
            assert ok, (case, u, t)
            if pos[u, t] >= 0:
                worst_gap = max(worst_gap, best - obj)
                worst_obj = max(worst_obj, abs(got["objective"][u, t] - obj))
        margins = [obj - second for ok, obj, _, second in replay(pred0[u], sc[u], unit, theta, ref["positions"][u])
                   if second > -np.inf and not np.isnan(obj)]
        close = [m for m in margins if 0.0 < m <= MARGIN]
        low = min([low] + [m for m in margins if m > 0.0])
        if close:
            exempt += 1
        else:
            assert np.array_equal(pos[u], ref["positions"][u]), (case, u)
    print("%s: max (step maximum - the pick's objective) = %.3g, max |objective - reference| = %.3g, smallest margin %.3g, "
          "%d of %d lists exempt" % (case, worst_gap, worst_obj, low, exempt, n))
    assert worst_gap <= EPS and worst_obj <= EPS, case
    if theta == 0.0:   # no dot product in the objective: the definition's own bits
        assert _same(got["objective"], ref["objective"]), case
    return exempt


def _clean(rng, n, N, n_items):
    """distinct items per list, normal scores sorted descending: the inputs for which the reference has no near-tie"""
    pred1 = np.stack([rng.permutation(n_items)[:N] for _ in range(n)]).astype(np.int32) + 1
    sc = -np.sort(-rng.standard_normal((n, N)), axis=1)
    return pred1, sc


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("rank", RANKS)
def test_every_pick_follows_the_definition(rank, dtype):
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    n_items = 1200
    lists = exempt = 0
    for ld, c0, c1 in _windows(rank):
        rng = np.random.default_rng(2000 * rank + c0)
        Vh = rng.standard_normal((n_items, ld)).astype(dtype)
        V = be.to_device(Vh, _torch_type(dtype))
        for N, k in SHAPES:
            n = 5 if N < 257 else 3                                           # (the definition in numpy is the cost of this test)
            pred1, sc = _clean(rng, n, N, n_items)
            res, dsc = be.to_device(pred1, torch.int32), be.to_device(sc, torch.float64)
            for theta in _thetas(rank):
                case = "rank %d %s window %d:%d of %d, pool %d, k %d, theta %g" % (rank, np.dtype(dtype).name, c0, c1, ld, N, k, theta)
                exempt += _check(_run(be, res, dsc, V, c0, c1, k, theta), pred1, sc, Vh, c0, c1, k, theta, case)
                lists += n
        be.drop_v32()
    assert exempt * 100 <= lists, (exempt, lists)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("rank", RANKS)
def test_one_user_at_the_largest_pool(rank, dtype):
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    n_items, N, k = 9000, 8192, 3
    ld, c0, c1 = _windows(rank)[rank % 2]                                      # the aligned window at even ranks, the scalar path at odd
    rng = np.random.default_rng(77 + rank)
    Vh = rng.standard_normal((n_items, ld)).astype(dtype)
    V = be.to_device(Vh, _torch_type(dtype))
    pred1, sc = _clean(rng, 1, N, n_items)
    res, dsc = be.to_device(pred1, torch.int32), be.to_device(sc, torch.float64)
    exempt = 0
    for theta in _thetas(rank):
        case = "rank %d %s window %d:%d of %d, pool %d, k %d, theta %g" % (rank, np.dtype(dtype).name, c0, c1, ld, N, k, theta)
        exempt += _check(_run(be, res, dsc, V, c0, c1, k, theta), pred1, sc, Vh, c0, c1, k, theta, case)
    assert exempt == 0


def _dirty(N, n, n_items, ld, c0, c1, dtype, seed):
    rng = np.random.default_rng(seed)
    Vh = _factors(n_items, ld, c0, c1, dtype, seed)
    Vh[NEAR[1]] = rng.standard_normal(ld).astype(dtype)                        # (two nearly identical items would BE a near-tie)
    pred1 = _lists(N, n, n_items, seed + 1, special=DEGENERATE + (TINY,))
    sc = -np.sort(-rng.standard_normal((n, N)), axis=1)
    r = rng.random((n, N))
    sc[r < 0.03] = np.nan
    sc[(r >= 0.03) & (r < 0.04)] = np.inf
    sc[(r >= 0.04) & (r < 0.05)] = -np.inf
    if n > 3 and N > 6:
        pred1[3, 6:] = NA                                                      # fewer valid positions than k
    return Vh, pred1, sc


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("rank", [1, 3, 10, 64, 100, 128, 256])
def test_lists_with_invalid_and_repeated_entries(rank, dtype):
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    n_items = 300
    lists = exempt = 0
    for ld, c0, c1 in _windows(rank):
        for N, k, n in [(2, 2, 5), (63, 10, 37), (100, 10, 37), (257, 20, 5), (1000, 50, 5)]:
            Vh, pred1, sc = _dirty(N, n, n_items, ld, c0, c1, dtype, 7 * N + rank + c0)
            V = be.to_device(Vh, _torch_type(dtype))
            res, dsc = be.to_device(pred1, torch.int32), be.to_device(sc, torch.float64)
            for theta in _thetas(rank)[-2:]:
                case = "rank %d %s window %d:%d of %d, pool %d, k %d, %d users, theta %g" % (rank, np.dtype(dtype).name, c0, c1, ld, N,
                                                                                          k, n, theta)
                got = _run(be, res, dsc, V, c0, c1, k, theta)
                exempt += _check(got, pred1, sc, Vh, c0, c1, k, theta, case)
                lists += n
                assert (got["items"][1] == NA).all() and np.isnan(got["objective"][1]).all(), case      # the all-invalid row
                if n > 3 and N > 6:
                    assert (got["items"][3, 6:] == NA).all(), case
            be.drop_v32()
    assert exempt * 100 <= lists, (exempt, lists)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_duplicated_rows_repeats_and_each_output_alone(dtype):
    from rsparse_amd.engine import HipBackend
    from rsparse_amd.metrics import mmr_reference
    be = HipBackend()
    n_items, n = 400, 9
    for rank, N, k in [(10, 100, 10), (128, 100, 20), (128, 300, 20), (33, 65, 30)]:
        for ld, c0, c1 in _windows(rank):
            rng = np.random.default_rng(rank + N + c0)
            Vh = rng.standard_normal((n_items, ld)).astype(dtype)
            a, b = 17, 311
            Vh[b] = Vh[a]                                                      # bit-identical rows
            pred1, sc = _clean(rng, n, N, n_items)
            for u in range(n):                                                 # a and b at positions 2 u + 1 < 3 u + 5 with equal scores
                row = pred1[u][~np.isin(pred1[u], (a + 1, b + 1))]
                pred1[u] = np.concatenate([row, rng.permutation(n_items)[:N] + 1])[:N]     # (b may return: a repeat, harmless)
                pa, pb = 2 * u + 1, 3 * u + 5
                pred1[u, pa], pred1[u, pb] = (a + 1, b + 1) if u % 2 == 0 else (b + 1, a + 1)
                sc[u, pb] = sc[u, pa]
            swapped = pred1.copy()
            swapped[pred1 == a + 1], swapped[pred1 == b + 1] = b + 1, a + 1
            V = be.to_device(Vh, _torch_type(dtype))
            dsc = be.to_device(sc, torch.float64)
            res, res_sw = be.to_device(pred1, torch.int32), be.to_device(swapped, torch.int32)
            for theta in (0.0, 0.5, 1.0):
                case = "rank %d %s window %d:%d, pool %d, k %d, theta %g" % (rank, np.dtype(dtype).name, c0, c1, N, k, theta)
                got = _run(be, res, dsc, V, c0, c1, k, theta)
                assert _check(got, pred1, sc, Vh, c0, c1, k, theta, case) == 0
                ref = mmr_reference(pred1.astype(np.int64) - 1, sc, k, theta, Vh, c0, c1)
                assert np.array_equal(got["items"] - 1, ref["items"]), case    # the items match exactly
                for u in range(n):                                             # the tie goes to the lower position
                    p = (got["positions"][u] - 1).tolist()
                    if 3 * u + 5 in p:
                        assert 2 * u + 1 in p and p.index(2 * u + 1) < p.index(3 * u + 5), (case, u)
                # the duplicated rows are interchangeable bit for bit
                sw = _run(be, res_sw, dsc, V, c0, c1, k, theta)
                assert _same(sw["positions"], got["positions"]) and _same(sw["objective"], got["objective"]), case
                again = _run(be, res, dsc, V, c0, c1, k, theta)                # a repeated call returns the same bits
                assert all(_same(again[m], got[m]) for m in got), case
                for m in WANT:                                                 # every nullable output on its own, and none
                    only = _run(be, res, dsc, V, c0, c1, k, theta, want=(m,))
                    assert sorted(only) == sorted(("items", m)) and _same(only[m], got[m]) and _same(only["items"], got["items"]), case
                only = _run(be, res, dsc, V, c0, c1, k, theta, want=())
                assert list(only) == ["items"] and _same(only["items"], got["items"]), case
            lo, hi = _run(be, res[:4], dsc[:4], V, c0, c1, k, 0.5), _run(be, res[4:], dsc[4:], V, c0, c1, k, 0.5)
            whole = _run(be, res, dsc, V, c0, c1, k, 0.5)
            for m in whole:                                                    # a row's bits do not depend on the batch it is in
                assert _same(np.concatenate([lo[m], hi[m]]), whole[m]), (rank, N, m)
            be.drop_v32()
    with pytest.raises(ValueError):
        be.mmr_rerank(res, dsc, V, c0, c1, k, 0.5, want=("rank",))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_host_form(dtype):
    from rsparse_amd import metrics
    from rsparse_amd.engine import HipBackend
    n_items, n, N, k = 300, 5, 129, 20
    for ld, c0, c1 in _windows(10):
        Vh, pred1, sc = _dirty(N, n, n_items, ld, c0, c1, dtype, 31 + c0)
        pred0 = np.where(pred1 == NA, -1, pred1.astype(np.int64) - 1)          # the Python functions take 0-based lists with -1
        got = metrics.mmr_rerank(pred0, sc, k, 0.5, Vh, c0, c1)
        be = HipBackend()                                                      # the device form gives the same bits
        dev = _run(be, be.to_device(pred1, torch.int32), be.to_device(sc, torch.float64), be.to_device(Vh, _torch_type(dtype)), c0, c1,
                   k, 0.5)
        assert _check(dev, pred1, sc, Vh, c0, c1, k, 0.5, "host form, window %d:%d" % (c0, c1)) == 0
        zero_based = lambda a: np.where(a == NA, -1, a.astype(np.int64) - 1)
        assert _same(got["items"], zero_based(dev["items"])) and _same(got["positions"], zero_based(dev["positions"]))
        assert _same(got["scores"], dev["scores"]) and _same(got["objective"], dev["objective"])


# ---- through the class on the movielens fixture --------------------------------------------------------------------------------
def test_predict_and_evaluate_diversify_on_movielens(ml_train):
    from rsparse_amd import WRMF
    from rsparse_amd.metrics import list_diversity, mmr_reference, mmr_rerank, ndcg_k
    n_user, n_item, tp, ti, tx = ml_train
    full = sp.csc_matrix((tx, ti, tp), shape=(n_user, n_item)).tocsr()
    rng = np.random.default_rng(21)
    coo = full.tocoo()
    out = rng.random(coo.nnz) < 0.2                                   # a fifth of every user's ratings held out
    train = sp.csr_matrix((coo.data[~out], (coo.row[~out], coo.col[~out])), shape=full.shape)
    held = sp.csr_matrix((coo.data[out], (coo.row[out], coo.col[out])), shape=full.shape)
    m = WRMF(rank=10, lambda_=0.1, feedback="implicit", solver="conjugate_gradient", precision="float", rng=1)
    m.fit_transform(train, n_iter=3, convergence_tol=-1)
    assert hasattr(m._backend(), "mmr_rerank")
    Vh = m._V.cpu().numpy()
    res, sc, _ = m._predict_device(train, 50, "x", ())                # the pool with its double scores, as the re-ranking sees it
    pool1, pool_sc = res.cpu().numpy(), sc.cpu().numpy()
    pool0 = np.where(pool1 == NA, -1, pool1.astype(np.int64) - 1)
    got = m.predict(train, 10, diversify=0.5, pool=50)
    alone = mmr_rerank(pool0, pool_sc, 10, 0.5, Vh)                   # the stand-alone device function on predict(m, 50)
    assert _same(np.asarray(got), alone["items"]) and _same(got.objective, alone["objective"])
    assert _same(got.scores, alone["scores"].astype(got.scores.dtype))
    dev = {"items": np.where(alone["items"] < 0, NA, alone["items"] + 1).astype(np.int32), "scores": alone["scores"],
           "positions": np.where(alone["positions"] < 0, NA, alone["positions"] + 1).astype(np.int32), "objective": alone["objective"]}
    exempt = _check(dev, pool1, pool_sc, Vh, 0, Vh.shape[1], 10, 0.5, "movielens, pool 50, k 10, theta 0.5")
    assert exempt * 100 <= n_user
    plain = m.predict(train, 10)
    zero = m.predict(train, 10, diversify=0.0)
    assert _same(np.asarray(zero), np.asarray(plain)) and _same(zero.scores, plain.scores)
    same = m.predict(train, 10, diversify=None)
    assert _same(np.asarray(same), np.asarray(plain)) and _same(same.scores, plain.scores) and same.objective is None
    # evaluate: one re-rank at max(k), every metric on the re-ranked lists
    K = (5, 10, 20)
    ev = m.evaluate(train, held, K, metrics=("ndcg", "diversity"), diversify=0.7)
    top = m.predict(train, 20, diversify=0.7)
    lists = np.asarray(top)
    assert _same(ev["diversity"], list_diversity(lists, K, Vh)["diversity"])
    for t, c in enumerate(K):
        assert _same(ev["ndcg"][:, t], ndcg_k(lists[:, :c], held))
    base = m.evaluate(train, held, K, metrics=("ndcg", "diversity"))
    assert (np.nanmean(ev["diversity"], axis=0) >= np.nanmean(base["diversity"], axis=0)).all()
    # with sampled negatives the pool is the candidates' top-`pool`
    ev = m.evaluate(train, held, K, metrics=("hit", "diversity"), negatives=99, seed=7, diversify=0.5)
    cand = m.sample_negatives(train, 99, actual=held, seed=7)
    lists = np.asarray(m.predict(train, 20, candidates=cand, diversify=0.5))
    assert _same(ev["diversity"], list_diversity(lists, K, Vh)["diversity"])
