"""Beyond-accuracy metrics of the lists on the MI355X.  The integer kernel (wrmf_lists.hip): valid, count_sum, info_sum, the two
integer-ratio doubles popularity and novelty, and the exposure histogram against the numpy definition
`rsparse_amd.metrics.list_metrics_reference`, BIT FOR BIT (the doubles compared as uint64 views) -- there is no tolerance.  The
diversity kernels (wrmf_diversity.hip): `counted` exactly, `diversity` within 1e-11 absolute of the pairwise
`list_diversity_reference` (the bound of DESIGN.md 3.23 at the API's limits, m = 8192 and r = 256, is 3.7e-12), NaN in the same
places, a repeated call bit-identical; the inverse norms within 4 ulp of numpy's and exactly 0.0 for degenerate items.  Shapes:
the list widths around the 64-position chunk, the cutoff sets of test_hit_metrics.py, a partly filled last workgroup, a small
catalogue with heavy exposure collisions and a larger one, every lane-group width of the gather (ranks 1 .. 256), the misaligned
scalar path (a window from column 1) and both factor types.  Then `WRMF.evaluate` with every new name on the movielens fixture."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from test_metrics_abi import NA

pytestmark = pytest.mark.gpu

INT_OUT = ("valid", "count_sum", "info_sum", "popularity", "novelty")
DIV_TOL = 1e-11


def _same(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    if got.dtype != ref.dtype or got.shape != ref.shape:
        return False
    if got.dtype == np.float64:
        return np.array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(ref).view(np.uint64))
    return np.array_equal(got, ref)


def _cutoff_sets(k):
    sets = [(1,), (63, 64, 65), (1, 64, 128, 129), (k,), tuple(int(c) for c in np.unique(np.linspace(1, k, 16).astype(int)))]
    return sorted({s for s in sets if s[0] >= 1 and s[-1] <= k and all(b > a for a, b in zip(s, s[1:]))})


def _lists(k, n_users, n_items, seed, special=()):
    """R-style lists (1-based, NA) with NA, 0, n_item + 1, negative and repeated entries and the `special` items mixed in; row 1
    (where there is one) is all invalid"""
    rng = np.random.default_rng(seed)
    pred = rng.integers(1, n_items + 1, (n_users, k)).astype(np.int64)
    r = rng.random((n_users, k))
    pred[r < 0.04] = NA
    pred[(r >= 0.04) & (r < 0.06)] = 0
    pred[(r >= 0.06) & (r < 0.08)] = n_items + 1
    pred[(r >= 0.08) & (r < 0.10)] = -int(rng.integers(1, 50))
    if special:
        sp_at = (r >= 0.10) & (r < 0.25)
        pred[sp_at] = rng.choice(np.asarray(special) + 1, size=int(sp_at.sum()))
    if k > 3:
        pred[:, 3] = pred[:, 1]
    if n_users > 1:
        pred[1] = np.where(np.arange(k) % 3 == 0, NA, np.where(np.arange(k) % 3 == 1, 0, n_items + 1))
    if n_users > 2:
        pred[2] = pred[2, 0]                                                  # one entry repeated
    return pred.astype(np.int32)


def _zero_based(pred1):
    return pred1.astype(np.int64) - 1                                         # (NA and 0 turn negative)


def _tables(n_items, seed):
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 2 ** 31, n_items).astype(np.int32)
    cnt[:3] = [0, 2 ** 31 - 1, 1]
    info = rng.integers(0, 2 ** 40, n_items).astype(np.int64)
    info[:3] = [2 ** 40 - 1, 0, 1]
    return cnt, info


class _Dev:
    def __init__(self, pred1, n_items, cnt=None, info=None):
        from rsparse_amd.engine import HipBackend
        self.be = HipBackend()
        self.n_items = n_items
        self.res = self.be.to_device(pred1, torch.int32)                      # row-major, as top_product writes it
        self.cnt = None if cnt is None else self.be.to_device(cnt, torch.int32)
        self.info = None if info is None else self.be.to_device(info, torch.int64)

    def exposure(self, T):
        return torch.zeros((T, self.n_items), dtype=torch.int32, device=self.res.device)

    def run(self, cutoffs, want, exposure=None, rows=None, tables=(True, True)):
        a, b = rows or (0, self.res.shape[0])
        out = self.be.list_metrics(self.res[a:b], cutoffs, self.n_items, want, self.cnt if tables[0] else None,
                                   self.info if tables[1] else None, exposure)
        return {m: v.cpu().numpy() for m, v in out.items()}


def _cumulated(exposure):
    return torch.cumsum(exposure.to(torch.int64), dim=0).cpu().numpy().astype(np.int32)


# ---- the integer kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n_users,n_items", [(1, 1, 300), (2, 5, 300), (63, 37, 300), (64, 5, 20000), (65, 37, 20000),
                                               (129, 5, 300), (200, 37, 20000), (200, 37, 300)])
def test_every_integer_output_equals_the_definition(k, n_users, n_items):
    from rsparse_amd.metrics import list_metrics_reference
    pred1 = _lists(k, n_users, n_items, 11 + k)
    cnt, info = _tables(n_items, k)
    dev = _Dev(pred1, n_items, cnt, info)
    for cutoffs in _cutoff_sets(k):
        ref = list_metrics_reference(_zero_based(pred1), cutoffs, n_items, cnt, info)
        expo = dev.exposure(len(cutoffs))
        got = dev.run(cutoffs, INT_OUT, expo)
        for m in INT_OUT:
            assert _same(got[m], ref[m]), (cutoffs, m)
        assert _same(_cumulated(expo), ref["exposure"]), cutoffs
        got = dev.run(cutoffs, INT_OUT)                                       # without exposure: the other instantiation
        for m in INT_OUT:
            assert _same(got[m], ref[m]), (cutoffs, m)
    if n_users > 1:
        assert (got["valid"][1] == 0).all() and np.isnan(got["popularity"][1]).all() and np.isnan(got["novelty"][1]).all()


def test_each_output_alone_repeats_and_row_batches():
    from rsparse_amd.metrics import list_metrics_reference
    k, n, n_items = 200, 37, 300
    pred1 = _lists(k, n, n_items, 5)
    cnt, info = _tables(n_items, 9)
    dev = _Dev(pred1, n_items, cnt, info)
    cutoffs = (1, 64, 128, 129)
    ref = list_metrics_reference(_zero_based(pred1), cutoffs, n_items, cnt, info)
    for m in INT_OUT:                                                         # every nullable output on its own
        tables = (m in ("count_sum", "popularity"), m in ("info_sum", "novelty"))
        got = dev.run(cutoffs, (m,), tables=tables)                           # ... with only the table it needs
        assert list(got) == [m] and _same(got[m], ref[m]), m
        expo = dev.exposure(4)
        got = dev.run(cutoffs, (m,), expo)
        assert _same(got[m], ref[m]) and _same(_cumulated(expo), ref["exposure"]), m
    expo = dev.exposure(4)                                                    # exposure alone, without a table
    assert dev.run(cutoffs, (), expo, tables=(False, False)) == {} and _same(_cumulated(expo), ref["exposure"])
    with pytest.raises(ValueError):
        dev.run(cutoffs, ())
    with pytest.raises(ValueError):
        dev.run(cutoffs, ("popularity",), tables=(False, True))
    # a repeated call returns the same bits
    first, again = dev.run(cutoffs, INT_OUT, dev.exposure(4)), dev.run(cutoffs, INT_OUT, expo)
    for m in INT_OUT:
        assert _same(first[m], ref[m]) and _same(again[m], ref[m]), m
    assert _same(_cumulated(expo), 2 * ref["exposure"])                       # ... and the histogram accumulates
    # two row batches sharing one exposure array are one call on all rows
    expo = dev.exposure(4)
    h = 18
    lo, hi = dev.run(cutoffs, INT_OUT, expo, (0, h)), dev.run(cutoffs, INT_OUT, expo, (h, n))
    for m in INT_OUT:
        assert _same(np.concatenate([lo[m], hi[m]]), ref[m]), m
    assert _same(_cumulated(expo), ref["exposure"])


@pytest.mark.parametrize("k,n_users,n_items,cutoffs", [(5, 7, 300, (2, 3)), (200, 37, 20000, (63, 64, 65)), (129, 5, 300, (1, 129))])
def test_host_form_of_the_integer_metrics(k, n_users, n_items, cutoffs):
    from rsparse_amd import metrics
    pred1 = _lists(k, n_users, n_items, 3 + k)
    cnt, info = _tables(n_items, 4)
    pred0 = np.where(pred1 == NA, -1, _zero_based(pred1))                     # the Python functions take 0-based lists with -1
    ref = metrics.list_metrics_reference(pred0, cutoffs, n_items, cnt, info)
    got = metrics.list_metrics(pred0, cutoffs, n_items, cnt, info)
    assert sorted(got) == sorted(ref)
    for m in ref:
        assert _same(got[m], ref[m]), m
    only = metrics.list_metrics(pred0, cutoffs, n_items, item_info=info, metrics=("novelty", "popularity"))
    assert list(only) == ["novelty"] and _same(only["novelty"], ref["novelty"])
    only = metrics.list_metrics(pred0, cutoffs, n_items, metrics=("exposure",))
    assert list(only) == ["exposure"] and _same(only["exposure"], ref["exposure"])
    s = metrics.exposure_summary(got["exposure"])
    assert s["gini"].shape == (len(cutoffs),) and ((s["gini"] >= 0) & (s["gini"] < 1)).all() and (s["entropy"] > 0).all()


# ---- the diversity kernels -----------------------------------------------------------------------------------------------------
DEGENERATE = (5, 6, 8, 9)     # all-zero, all-zero, an infinite and a NaN coordinate
TINY = 7                      # 1e-30: its squares underflow in fp32, not in the double sum -- a direction like any other
NEAR = (12, 13)               # nearly identical items
LIST_CASES = [(1, 1, (1,)), (2, 5, (1, 2)), (63, 5, (63,)), (64, 37, (1, 64)), (65, 5, (63, 64, 65)),
              (129, 37, (1, 64, 128, 129)), (200, 37, tuple(int(c) for c in np.unique(np.linspace(1, 200, 16).astype(int)))),
              (200, 5, (200,))]


def _factors(n_items, ld, c0, c1, dtype, seed):
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((n_items, ld)).astype(dtype)
    V[DEGENERATE[0]] = 0
    V[DEGENERATE[1], c0:c1] = 0                                               # zero inside the window only
    V[DEGENERATE[2], (c0 + c1) // 2] = np.inf
    V[DEGENERATE[3], (c0 + c1) // 2] = np.nan
    V[TINY] = 1e-30
    V[NEAR[1]] = V[NEAR[0]] * (1 + 1e-6)
    return V


def _windows(rank):
    """(ld, c0, c1): the whole matrix, and the latent columns of a model with biases -- a window from column 1 of rank + 2
    columns, whose rows are not 16-byte aligned"""
    return [(rank, 0, rank), (rank + 2, 1, rank + 1)]


def _ulps(a, b):
    return np.abs(a.view(np.int64) - b.view(np.int64))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("rank", [1, 3, 4, 10, 64, 100, 128, 256])
def test_diversity_and_inverse_norms(rank, dtype):
    from rsparse_amd.engine import HipBackend
    from rsparse_amd.metrics import list_diversity_reference
    be = HipBackend()
    n_items = 300
    for ld, c0, c1 in _windows(rank):
        Vh = _factors(n_items, ld, c0, c1, dtype, rank + c0)
        V = be.to_device(Vh, torch.float64 if dtype == np.float64 else torch.float32)
        W = Vh[:, c0:c1].astype(np.float64)
        with np.errstate(all="ignore"):
            ss = (W * W).sum(axis=1)
            ok = (ss > 0) & np.isfinite(ss)
            inv_ref = np.where(ok, 1.0 / np.sqrt(np.where(ok, ss, 1.0)), 0.0)
        inv = be.item_inv_norms(V, c0, c1).cpu().numpy()
        assert inv.dtype == np.float64 and (inv[~ok] == 0.0).all() and not np.signbit(inv[~ok]).any()
        assert set(DEGENERATE) <= set(np.flatnonzero(~ok).tolist()) and ok[TINY]
        assert _ulps(inv[ok], inv_ref[ok]).max() <= 4
        assert be.item_inv_norms(V, c0, c1) is be.item_inv_norms(V, c0, c1)   # kept until the matrix changes
        for k, n_users, cutoffs in LIST_CASES:
            pred1 = _lists(k, n_users, n_items, 7 * k + rank, special=DEGENERATE + (TINY,) + NEAR)
            ref = list_diversity_reference(_zero_based(pred1), cutoffs, Vh, c0, c1)
            res = be.to_device(pred1, torch.int32)
            got = {m: v.cpu().numpy() for m, v in be.list_diversity(res, cutoffs, V, c0, c1).items()}
            case = (ld, c0, k, n_users, cutoffs)
            assert _same(got["counted"], ref["counted"]), case
            assert np.array_equal(np.isnan(got["diversity"]), np.isnan(ref["diversity"])), case
            assert np.array_equal(np.isnan(got["diversity"]), ref["counted"] < 2), case
            err = np.abs(got["diversity"] - ref["diversity"])
            print("rank %d %s window %d:%d of %d, k %d, %d users, %d cutoffs: max |diversity - reference| = %.3g"
                  % (rank, np.dtype(dtype).name, c0, c1, ld, k, n_users, len(cutoffs), np.nanmax(err) if (~np.isnan(err)).any() else 0.0))
            assert not (err > DIV_TOL).any(), case
            again = {m: v.cpu().numpy() for m, v in be.list_diversity(res, cutoffs, V, c0, c1).items()}
            assert _same(again["counted"], got["counted"]) and _same(again["diversity"], got["diversity"]), case
            only = be.list_diversity(res, cutoffs, V, c0, c1, want=("diversity",))          # each output alone
            assert list(only) == ["diversity"] and _same(only["diversity"].cpu().numpy(), got["diversity"]), case
            only = be.list_diversity(res, cutoffs, V, c0, c1, want=("counted",))
            assert list(only) == ["counted"] and _same(only["counted"].cpu().numpy(), got["counted"]), case
            if n_users > 2:
                assert (got["counted"][1] == 0).all()                                       # the all-invalid row
                rep = got["diversity"][2][got["counted"][2] >= 2]                            # one item repeated
                assert (np.abs(rep) <= DIV_TOL).all()
        be.drop_v32()


def test_diversity_in_a_large_catalogue_and_row_batches():
    from rsparse_amd.engine import HipBackend
    from rsparse_amd.metrics import list_diversity_reference
    be = HipBackend()
    n_items, rank, k, n = 20000, 10, 200, 37
    Vh = _factors(n_items, rank, 0, rank, np.float32, 3)
    V = be.to_device(Vh, torch.float32)
    pred1 = _lists(k, n, n_items, 77, special=DEGENERATE + (TINY,) + NEAR)
    cutoffs = (1, 64, 128, 129)
    ref = list_diversity_reference(_zero_based(pred1), cutoffs, Vh, 0, rank)
    res = be.to_device(pred1, torch.int32)
    got = {m: v.cpu().numpy() for m, v in be.list_diversity(res, cutoffs, V, 0, rank).items()}
    assert _same(got["counted"], ref["counted"]) and not (np.abs(got["diversity"] - ref["diversity"]) > DIV_TOL).any()
    assert np.array_equal(np.isnan(got["diversity"]), np.isnan(ref["diversity"]))
    lo, hi = be.list_diversity(res[:18], cutoffs, V, 0, rank), be.list_diversity(res[18:], cutoffs, V, 0, rank)
    for m in got:                                                             # a row's bits do not depend on the batch it is in
        assert _same(np.concatenate([lo[m].cpu().numpy(), hi[m].cpu().numpy()]), got[m]), m


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_host_form_of_the_diversity(dtype):
    from rsparse_amd import metrics
    from rsparse_amd.engine import HipBackend
    n_items, k, n = 300, 129, 5
    pred1 = _lists(k, n, n_items, 31, special=DEGENERATE + (TINY,) + NEAR)
    pred0 = np.where(pred1 == NA, -1, _zero_based(pred1))
    cutoffs = (1, 64, 128, 129)
    for ld, c0, c1 in _windows(10):
        Vh = _factors(n_items, ld, c0, c1, dtype, 5)
        ref = metrics.list_diversity_reference(pred0, cutoffs, Vh, c0, c1)
        got = metrics.list_diversity(pred0, cutoffs, Vh, c0, c1)
        assert _same(got["counted"], ref["counted"]) and not (np.abs(got["diversity"] - ref["diversity"]) > DIV_TOL).any()
        assert np.array_equal(np.isnan(got["diversity"]), np.isnan(ref["diversity"]))
        be = HipBackend()                                                     # the device form gives the same bits
        dev = be.list_diversity(be.to_device(pred1, torch.int32), cutoffs,
                                be.to_device(Vh, torch.float64 if dtype == np.float64 else torch.float32), c0, c1)
        assert _same(dev["diversity"].cpu().numpy(), got["diversity"]) and _same(dev["counted"].cpu().numpy(), got["counted"])


# ---- WRMF.evaluate end to end ------------------------------------------------------------------------------------------------
def test_evaluate_every_new_metric_on_movielens(ml_train):
    from rsparse_amd import WRMF
    from rsparse_amd.metrics import (exposure_summary, list_diversity, list_diversity_reference, list_metrics_reference,
                                     self_information, summarize)
    n_user, n_item, tp, ti, tx = ml_train
    full = sp.csc_matrix((tx, ti, tp), shape=(n_user, n_item)).tocsr()
    rng = np.random.default_rng(21)
    coo = full.tocoo()
    out = rng.random(coo.nnz) < 0.2                                   # a fifth of every user's ratings held out
    train = sp.csr_matrix((coo.data[~out], (coo.row[~out], coo.col[~out])), shape=full.shape)
    held = sp.csr_matrix((coo.data[out], (coo.row[out], coo.col[out])), shape=full.shape)
    m = WRMF(rank=10, lambda_=0.1, feedback="implicit", solver="conjugate_gradient", precision="float", rng=1)
    m.fit_transform(train, n_iter=3, convergence_tol=-1)
    be = m._backend()
    assert hasattr(be, "list_metrics") and hasattr(be, "list_diversity")
    pop = np.asarray((train != 0).sum(axis=0)).ravel().astype(np.int64)
    info = self_information(pop)
    K = (1, 5, 10, 20)
    new = ("popularity", "novelty", "diversity", "gini", "entropy")
    names = ("ndcg", "hit", "coverage") + new
    V = m._V.cpu().numpy()
    cand = sp.csr_matrix(rng.random(full.shape) < 0.1, dtype=np.float64)
    ways = {"plain": ({}, {}), "candidates": ({"candidates": cand}, {"candidates": cand}),
            "negatives": ({"negatives": 99, "seed": 7}, {"candidates": m.sample_negatives(train, 99, actual=held, seed=7)})}
    for way, (ev_args, pr_args) in ways.items():
        ev = m.evaluate(train, held, K, metrics=names, item_popularity=pop, **ev_args)
        assert list(ev) == list(names), way
        top = np.asarray(m.predict(train, 20, **pr_args))
        ref = list_metrics_reference(top, K, n_item, pop, info)
        assert _same(ev["popularity"], ref["popularity"]) and _same(ev["novelty"], ref["novelty"]), way
        summ = exposure_summary(ref["exposure"])
        assert _same(ev["gini"], summ["gini"]) and _same(ev["entropy"], summ["entropy"]), way
        div = list_diversity_reference(top, K, V, 0, V.shape[1])
        assert np.array_equal(np.isnan(ev["diversity"]), np.isnan(div["diversity"])), way
        assert not (np.abs(ev["diversity"] - div["diversity"]) > DIV_TOL).any(), way
        assert _same(ev["diversity"], list_diversity(top, K, V)["diversity"]), way     # the stand-alone device function
        old = m.evaluate(train, held, K, metrics=("ndcg", "hit", "coverage"), **ev_args)
        assert all(_same(old[name], ev[name]) for name in old), way                     # the old names are what they were
        s = summarize(ev)
        assert s["popularity"].shape == (4,) and s["gini"] is ev["gini"] and 0 < s["diversity"][-1] < 2, way
        assert ((ev["gini"] > 0) & (ev["gini"] < 1)).all(), way
    # a WRMF model gravitates to popular items: its lists are more popular than the sampled negatives' mix
    plain = summarize(m.evaluate(train, held, 10, metrics=("popularity", "novelty"), item_popularity=pop))
    assert plain["popularity"] > pop.mean() and isinstance(plain["novelty"], float)
    one = m.evaluate(train, held, 10, metrics=new, item_popularity=pop)
    both = m.evaluate(train, held, K, metrics=new, item_popularity=pop)
    assert isinstance(one["gini"], float) and one["gini"] == both["gini"][2] and one["entropy"] == both["entropy"][2]
    for name in ("popularity", "novelty"):
        assert one[name].shape == (n_user,) and _same(one[name], both[name][:, 2]), name
    # the order of the diversity's sums follows the cutoffs: the same bits for the same cutoffs, and two orders within the
    # tolerance of the reference each
    same = m.evaluate(train, held, (10,), metrics=("diversity",))["diversity"]
    assert one["diversity"].shape == (n_user,) and _same(one["diversity"], same[:, 0])
    assert not (np.abs(one["diversity"] - both["diversity"][:, 2]) > 2 * DIV_TOL).any()
    with pytest.raises(ValueError):
        m.evaluate(train, held, 10, metrics=("novelty",))
    with pytest.raises(ValueError):
        m.evaluate(train, held, 10, metrics=("popularity",), item_popularity=pop[:-1])
