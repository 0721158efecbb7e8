"""MMR re-ranking of the predicted lists without a device: the numpy definition `rsparse_amd.metrics.mmr_reference` on hand-worked
lists (the picks derived in the comments), the three consequences of the definition (theta = 0 is the valid prefix, the result
for k is the k-prefix of the result for a larger k, an exact tie between duplicated rows goes to the lower position), theta = 1,
equal scores, invalid positions, a degenerate row, short and empty lists; `WRMF.predict(diversify=)` / `WRMF.evaluate(diversify=)`
on the movielens fixture through the CPU stand-in backend (which has no `mmr_rerank` and so gets the definition through the
`hasattr` fallback) -- plain, `candidates=`, `negatives=` and on two gloo ranks --, the argument errors, and the status codes of
the new C entry points.  `replay` -- the definition's objective along a GIVEN path of picks -- is what tests/test_mmr.py holds
the kernel to."""
import ctypes
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import _lib
from conftest import csc_take_rows, load_movielens
from test_metrics_abi import NA, _oracle_metrics_backend

ROOT = Path(__file__).resolve().parent.parent


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def unit_rows(V, c0, c1):
    """u_j = V[j, c0:c1] inv_j in float64, the zero vector for a degenerate item: the statement of the definition"""
    W = np.asarray(V)[:, c0:c1].astype(np.float64)
    with np.errstate(all="ignore"):
        ss = (W * W).sum(axis=1)
        good = (ss > 0) & np.isfinite(ss)
        inv = np.where(good, 1.0 / np.sqrt(np.where(good, ss, 1.0)), 0.0)
        return np.where(good[:, None], W * inv[:, None], 0.0)


def replay(items, scores, unit, theta, positions):
    """One list (0-based items, scores) along the GIVEN path `positions` (-1 = nothing picked): per step (is the pick valid and
    untaken, the definition's objective of the pick, the step's maximum over the open positions, the runner-up's objective or
    -inf).  Stops being meaningful at the first step that is not ok."""
    items, scores = np.asarray(items, dtype=np.int64), np.asarray(scores, dtype=np.float64)
    N = items.size
    ok = (items >= 0) & (items < unit.shape[0]) & np.isfinite(scores)
    U = unit[np.where(ok, items, 0)]
    rel = np.zeros(N)
    if ok.any():
        lo, hi = scores[ok].min(), scores[ok].max()
        if hi != lo:
            with np.errstate(all="ignore"):
                rel = np.where(ok, (scores - lo) / (hi - lo), 0.0)
    lead = (1.0 - theta) * rel
    free, sim, steps = ok.copy(), np.zeros(N), []
    for t, i in enumerate(positions):
        if i < 0:
            steps.append((not free.any(), np.nan, np.nan, -np.inf))     # nothing picked: right only when nothing is open
            continue
        obj = np.where(free, lead - theta * sim, -np.inf)
        rest = np.delete(obj, i)
        steps.append((bool(free[i]), float(obj[i]), float(obj.max()), float(rest.max()) if rest.size else -np.inf))
        free[i] = False
        dots = (U * U[i]).sum(axis=1)                                           # (as the definition: the same order in every row)
        sim = dots if t == 0 else np.maximum(sim, dots)
    return steps


# ---- hand-worked lists ---------------------------------------------------------------------------------------------------------
def test_hand_worked_rank_2():
    from rsparse_amd.metrics import mmr_reference
    V = np.array([[2.0, 0.0], [3.0, 4.0], [0.0, 5.0], [-1.0, 0.0]], dtype=np.float32)     # units (1,0) (.6,.8) (0,1) (-1,0)
    pred, sc = np.array([[0, 1, 2]]), np.array([[3.0, 2.0, 1.0]])                          # rel = 1, 0.5, 0
    # theta = 0.5.  step 0: 0.5 rel = .5, .25, 0 -> position 0 (.5).  step 1: cosines to item 0 are .6 and 0:
    # .25 - .5 * .6 = -.05 against 0 - 0 = 0 -> position 2 (0).  step 2: max(.6, <u1, u2> = .8) -> .25 - .4 = -.15
    r = mmr_reference(pred, sc, 3, 0.5, V)
    assert r["items"].dtype == np.int64 and r["positions"].dtype == np.int64 and r["objective"].dtype == np.float64
    assert r["items"].tolist() == [[0, 2, 1]] and r["positions"].tolist() == [[0, 2, 1]]
    assert np.allclose(r["objective"], [[0.5, 0.0, -0.15]], rtol=0, atol=1e-15)
    # theta = 0.2: step 1 is .8 * .5 - .2 * .6 = .28 against 0 -> the plain order
    r = mmr_reference(pred, sc, 3, 0.2, V)
    assert r["positions"].tolist() == [[0, 1, 2]] and np.allclose(r["objective"], [[0.8, 0.28, -0.16]], rtol=0, atol=1e-15)
    # item 3 points away from item 0: with theta = 1 it is the second pick (cosine -1, objective +1), whatever its score
    pred, sc = np.array([[0, 1, 2, 3]]), np.array([[4.0, 3.0, 2.0, 1.0]])
    # step 0: every objective is 0 -> the lowest position.  step 1: -(.6), -(0), -(-1) -> position 3 (1).  step 2: item 1 has
    # max(.6, -.6) = .6, item 2 max(0, 0) = 0 -> position 2 (0).  step 3: item 1: max(.6, .8) -> -.8
    r = mmr_reference(pred, sc, 4, 1.0, V)
    assert r["positions"].tolist() == [[0, 3, 2, 1]] and np.allclose(r["objective"], [[0.0, 1.0, 0.0, -0.8]], rtol=0, atol=1e-15)
    # a window: column 1 alone makes items 0 and 3 degenerate (zero vectors: cosine 0 to everything) and items 1, 2 identical
    r = mmr_reference(pred, sc, 4, 1.0, V, 1, 2)
    # step 0: position 0.  step 1: all cosines to the zero vector are 0 -> position 1.  step 2: item 2 has cosine 1 to item 1,
    # item 3 (zero vector) 0 -> position 3 (0), then position 2 (-1)
    assert r["positions"].tolist() == [[0, 1, 3, 2]] and np.allclose(r["objective"], [[0.0, 0.0, 0.0, -1.0]], rtol=0, atol=1e-15)


def test_hand_worked_rank_3_with_invalid_positions():
    from rsparse_amd.metrics import mmr_reference
    V = np.array([[1, 0, 0], [0, 2, 0], [0, 0, 3], [1, 1, 0], [0, 0, 0]], dtype=np.float64)       # item 4 is degenerate
    s2 = np.sqrt(0.5)
    # positions 1 (NA), 3 (beyond the catalogue), 4 (negative), 6 (NaN score) and 7 (infinite score) are invalid
    pred = np.array([[3, -1, 0, 5, -7, 1, 2, 2, 4]])
    sc = np.array([[9.0, 8.5, 8.0, 7.5, 7.0, 6.0, np.nan, np.inf, 5.0]])
    # valid: positions 0 (item 3, s 9), 2 (item 0, s 8), 5 (item 1, s 6), 8 (item 4, s 5): rel = 1, .75, .25, 0.  theta = 0.5:
    # step 0: .5, .375, .125, 0 -> position 0.  step 1: cosines to item 3 = (1,1,0)/sqrt 2: item 0 s2, item 1 s2, item 4 0:
    #   .375 - .5 s2 = .0214.., .125 - .5 s2 = -.2285.., 0 -> position 2.  step 2: item 1: max(s2, 0) -> -.2285.., item 4: 0
    #   -> position 8 (0).  step 3: position 5 (-.2285..).  a fifth pick does not exist
    r = mmr_reference(pred, sc, 5, 0.5, V)
    assert r["positions"].tolist() == [[0, 2, 8, 5, -1]] and r["items"].tolist() == [[3, 0, 4, 1, -1]]
    assert np.allclose(r["objective"][0, :4], [0.5, 0.375 - 0.5 * s2, 0.0, 0.125 - 0.5 * s2], rtol=0, atol=1e-15)
    assert np.isnan(r["objective"][0, 4])
    steps = replay(pred[0], sc[0], unit_rows(V, 0, 3), 0.5, r["positions"][0])
    assert all(ok for ok, _, _, _ in steps) and all(o == m for _, o, m, _ in steps[:4])
    # an all-invalid list, and all scores equal (rel = 0 everywhere: the first pick is position 0, then the least similar)
    pred = np.array([[-1, 5, -3, 9], [0, 3, 1, 2]])
    sc = np.array([[1.0, 2.0, 3.0, 4.0], [2.5, 2.5, 2.5, 2.5]])
    r = mmr_reference(pred, sc, 3, 0.5, V)
    assert r["items"][0].tolist() == [-1, -1, -1] and r["positions"][0].tolist() == [-1, -1, -1] and np.isnan(r["objective"][0]).all()
    # row 1: step 0 position 0 (item 0).  step 1: item 3 s2, item 1 0, item 2 0 -> position 2 (0).  step 2: item 3:
    # max(s2, s2), item 2: 0 -> position 3
    assert r["positions"][1].tolist() == [0, 2, 3] and np.allclose(r["objective"][1], 0.0, rtol=0, atol=0)


# ---- the consequences of the definition ----------------------------------------------------------------------------------------
def _random_case(seed, n=12, N=40, n_item=60, rank=5, dtype=np.float32):
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((n_item, rank)).astype(dtype)
    V[7] = 0
    pred = rng.integers(0, n_item, (n, N)).astype(np.int64)
    r = rng.random((n, N))
    pred[r < 0.05] = -1
    pred[(r >= 0.05) & (r < 0.08)] = n_item
    pred[(r >= 0.08) & (r < 0.10)] = -9
    sc = -np.sort(-rng.standard_normal((n, N)), axis=1)
    sc[(r >= 0.10) & (r < 0.13)] = np.nan
    sc[(r >= 0.13) & (r < 0.14)] = -np.inf
    pred[1] = -1                                                                 # nothing valid
    pred[2, 6:] = n_item                                                         # fewer valid positions than k
    return pred, sc, V


def test_theta_zero_is_the_valid_prefix():
    from rsparse_amd.metrics import mmr_reference
    pred, sc, V = _random_case(1)
    r = mmr_reference(pred, sc, 20, 0.0, V)
    for u in range(pred.shape[0]):
        ok = np.flatnonzero((pred[u] >= 0) & (pred[u] < V.shape[0]) & np.isfinite(sc[u]))[:20]
        want = np.full(20, -1)
        want[:ok.size] = ok
        assert r["positions"][u].tolist() == want.tolist()
        assert r["items"][u, :ok.size].tolist() == pred[u, ok].tolist()
    assert (r["positions"][1] == -1).all() and (r["positions"][2] >= 0).sum() <= 6


@pytest.mark.parametrize("theta", [0.3, 0.7, 1.0])
def test_prefix_property_and_greedy_along_its_own_path(theta):
    from rsparse_amd.metrics import mmr_reference
    pred, sc, V = _random_case(2)
    r5, r20 = mmr_reference(pred, sc, 5, theta, V), mmr_reference(pred, sc, 20, theta, V)
    for name in r5:
        assert _same(r5[name], r20[name][:, :5]), name
    unit = unit_rows(V, 0, V.shape[1])
    for u in range(pred.shape[0]):
        steps = replay(pred[u], sc[u], unit, theta, r20["positions"][u])
        assert all(ok for ok, _, _, _ in steps)
        picked = r20["positions"][u] >= 0
        assert all(o == m for (_, o, m, _), p in zip(steps, picked) if p)
        assert _same(np.array([o for _, o, _, _ in steps]), r20["objective"][u])
    both = mmr_reference(pred, sc, 20, theta, V.astype(np.float64))              # the factor type only changes the rows' bits
    assert _same(both["positions"], r20["positions"])


def test_exact_tie_between_duplicated_rows_goes_to_the_lower_position():
    from rsparse_amd.metrics import mmr_reference
    rng = np.random.default_rng(3)
    V = rng.standard_normal((10, 7)).astype(np.float32)
    V[8] = V[4]                                                                  # bit-identical rows
    for a, b in ((4, 8), (8, 4)):
        pred = np.array([[1, a, 6, b, 2]])
        sc = np.array([[5.0, 3.0, 2.0, 3.0, 1.0]])                               # equal scores at positions 1 and 3
        for theta in (0.0, 0.4, 1.0):
            r = mmr_reference(pred, sc, 5, theta, V)
            pos = r["positions"][0].tolist()
            assert pos.index(1) < pos.index(3), (a, theta)
            steps = replay(pred[0], sc[0], unit_rows(V, 0, 7), theta, r["positions"][0])
            t = pos.index(1)
            assert steps[t][1] == steps[t][3]                                    # the runner-up of that step ties exactly


def test_argument_errors_of_the_definition_and_the_device_function():
    from rsparse_amd.metrics import check_trade_off, mmr_reference, mmr_rerank
    V = np.ones((3, 4), dtype=np.float32)
    pred, sc = np.array([[0, 1, 2], [2, 1, -1]]), np.zeros((2, 3))
    for bad in (-0.1, 1.5, np.nan, "0.5", None, True, np.inf):
        with pytest.raises(ValueError):
            check_trade_off(bad)
    assert check_trade_off(0) == 0.0 and check_trade_off(np.float32(1.0)) == 1.0
    for fn in (mmr_reference, mmr_rerank):
        for k in (0, 4, 2.0, True):
            with pytest.raises(ValueError):
                fn(pred, sc, k, 0.5, V)
        with pytest.raises(ValueError):
            fn(pred, sc, 2, 1.5, V)
        with pytest.raises(ValueError):
            fn(pred, sc[:, :2], 2, 0.5, V)
        with pytest.raises(ValueError):
            fn(pred, sc.astype(np.int64), 2, 0.5, V)
        with pytest.raises(TypeError):
            fn(pred.astype(np.float64), sc, 2, 0.5, V)
        for c0, c1 in ((2, 2), (3, 1), (-1, 2), (0, 5)):
            with pytest.raises(ValueError):
                fn(pred, sc, 2, 0.5, V, c0, c1)
        with pytest.raises(ValueError):
            fn(pred, sc, 2, 0.5, V.astype(np.float16))
    with pytest.raises(_lib.UnsupportedOnDevice):
        mmr_rerank(pred, sc, 2, 0.5, np.ones((3, 300), dtype=np.float32))
    with pytest.raises(_lib.UnsupportedOnDevice):
        mmr_rerank(np.zeros((1, 8193), dtype=np.int64), np.zeros((1, 8193)), 2, 0.5, V)


# ---- WRMF.predict / WRMF.evaluate on the CPU stand-in backend ------------------------------------------------------------------
N_USERS = 150
K = (5, 10, 20)


def _ml_model():
    """the first N_USERS users of the movielens fixture, a fifth of their ratings held out, fitted on the CPU stand-in"""
    from rsparse_amd import WRMF
    n_user, n_item, p, i, x = load_movielens()
    tp, ti, tx = csc_take_rows(N_USERS, p, i, x)
    full = sp.csc_matrix((tx, ti, tp), shape=(N_USERS, n_item)).tocoo()
    out = np.random.default_rng(21).random(full.nnz) < 0.2
    train = sp.csr_matrix((full.data[~out], (full.row[~out], full.col[~out])), shape=full.shape)
    held = sp.csr_matrix((full.data[out], (full.row[out], full.col[out])), shape=full.shape)
    rng = np.random.default_rng(3)
    rank = 6
    model = WRMF(rank=rank, lambda_=0.1, feedback="implicit", solver="cholesky", precision="float",
                 backend=_oracle_metrics_backend(), rng=1)
    model._init_user_factors = (rng.standard_normal((N_USERS, rank)) * 0.01).astype(np.float32)
    model.components = (rng.standard_normal((rank, n_item)) * 0.01).astype(np.float32)
    model.fit_transform(train, n_iter=2, convergence_tol=-1)
    return model, train, held


@pytest.fixture(scope="module")
def ml_model():
    return _ml_model()


def _pool(model, x, pool, not_recommend="x", items_exclude=(), candidates=None):
    """the top-`pool` of every row as the re-ranking sees it: 0-based lists (negative = NA) and the scores in double (`predict`
    rounds `.scores` to the model's precision)"""
    res, sc, _ = model._predict_device(x, pool, not_recommend, items_exclude, candidates)
    return res.cpu().numpy().astype(np.int64) - 1, sc.cpu().numpy().astype(np.float64)


def _reference_of(model, pool, k, theta):
    from rsparse_amd.metrics import mmr_reference
    V = model._V.cpu().numpy()
    return mmr_reference(pool[0], pool[1], k, theta, V, 0, V.shape[1])


def test_predict_diversify_equals_the_definition_on_the_pool(ml_model):
    model, train, held = ml_model
    assert not hasattr(model._backend(), "mmr_rerank")
    plain = model.predict(train, 10)
    same = model.predict(train, 10, diversify=None)
    assert _same(np.asarray(plain), np.asarray(same)) and _same(plain.scores, same.scores) and same.objective is None
    pool50 = _pool(model, train, 50)
    for theta in (0.5, 1.0):
        got = model.predict(train, 10, diversify=theta, pool=50)
        ref = _reference_of(model, pool50, 10, theta)
        assert got.shape == (N_USERS, 10) and _same(np.asarray(got), ref["items"]) and _same(got.objective, ref["objective"])
        picked = np.take_along_axis(pool50[1], ref["positions"], axis=1)
        assert _same(got.scores, picked.astype(got.scores.dtype))
    assert not _same(np.asarray(got), np.asarray(plain))                         # theta = 1 does change the lists
    zero = model.predict(train, 10, diversify=0.0, pool=50)
    assert _same(np.asarray(zero), np.asarray(plain)) and _same(zero.scores, plain.scores)
    # the default pool: min(10 k, 8192, n_item)
    got = model.predict(train, 10, diversify=0.5)
    assert _same(np.asarray(got), _reference_of(model, _pool(model, train, 100), 10, 0.5)["items"])
    # exclusions shape the pool
    got = model.predict(train, 5, not_recommend=None, items_exclude=(0, 49, 99), diversify=0.5, pool=30)
    ref = _reference_of(model, _pool(model, train, 30, None, (0, 49, 99)), 5, 0.5)
    assert _same(np.asarray(got), ref["items"]) and not np.isin(np.asarray(got), (0, 49, 99)).any()


def test_predict_diversify_with_candidates(ml_model):
    model, train, held = ml_model
    rng = np.random.default_rng(9)
    cand = sp.csr_matrix(rng.random(train.shape) < 0.02, dtype=np.float64)       # about 34 per row: some pools are short
    got = model.predict(train, 10, candidates=cand, diversify=0.5, pool=40)
    pool = _pool(model, train, 40, candidates=cand)
    ref = _reference_of(model, pool, 10, 0.5)
    assert (pool[0] < 0).any() and _same(np.asarray(got), ref["items"]) and _same(got.objective, ref["objective"])


def _several(model, train, held):
    return {"predict": model.predict(train, 10, diversify=0.7, pool=30),
            "objective": model.predict(train, 10, diversify=0.7, pool=30).objective,
            "evaluate": model.evaluate(train, held, K, metrics=("ndcg", "hit", "diversity", "coverage"), diversify=0.7),
            "negatives": model.evaluate(train, held, (2, 5), metrics=("hit", "diversity"), negatives=30, seed=3, diversify=0.5,
                                        pool=20)}


def test_evaluate_diversify_scores_the_reranked_lists(ml_model):
    from rsparse_amd.metrics import list_diversity_reference
    model, train, held = ml_model
    V = model._V.cpu().numpy()
    names = ("ndcg", "hit", "recall", "diversity", "coverage")
    ev = model.evaluate(train, held, K, metrics=names, diversify=0.7)
    lists = np.asarray(model.predict(train, 20, diversify=0.7))                  # one re-rank at max(k), the default pool of 200
    assert _same(lists, _reference_of(model, _pool(model, train, 200), 20, 0.7)["items"])
    div = list_diversity_reference(lists, K, V, 0, V.shape[1])["diversity"]
    assert _same(ev["diversity"], div)
    plain = model.evaluate(train, held, K, metrics=names)
    assert np.nanmean(ev["diversity"], axis=0)[2] > np.nanmean(plain["diversity"], axis=0)[2]
    assert not _same(ev["hit"], plain["hit"])
    none = model.evaluate(train, held, K, metrics=names, diversify=None)
    assert all(_same(none[m], plain[m]) for m in names)
    zero = model.evaluate(train, held, K, metrics=names, diversify=0.0)
    assert all(_same(zero[m], plain[m]) for m in ("hit", "recall", "diversity", "coverage"))
    # the prefix property: a scalar cutoff is the column of the sequence
    one = model.evaluate(train, held, 10, metrics=("hit", "diversity"), diversify=0.7, pool=200)
    assert _same(one["hit"], ev["hit"][:, 1]) and _same(one["diversity"], ev["diversity"][:, 1])
    # negatives: the pool is the candidates' top-`pool`
    ev = model.evaluate(train, held, (2, 5), metrics=("hit", "diversity"), negatives=30, seed=3, diversify=0.5, pool=20)
    cand = model.sample_negatives(train, 30, actual=held, seed=3)
    lists = np.asarray(model.predict(train, 5, candidates=cand, diversify=0.5, pool=20))
    assert _same(ev["diversity"], list_diversity_reference(lists, (2, 5), V, 0, V.shape[1])["diversity"])


def _worker(rank, ws, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT / "tests"))
    import torch.distributed as dist
    model, train, held = _ml_model()
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        torch.save(_several(model, train, held), os.path.join(out_dir, "mmr%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_give_the_one_process_result(tmp_path, ml_model):
    import torch.multiprocessing as mp
    one = _several(*ml_model)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        got = torch.load(tmp_path / ("mmr%d.pt" % r), weights_only=False)
        assert _same(np.asarray(got["predict"]), np.asarray(one["predict"])) and _same(got["objective"], one["objective"]), r
        for key in ("evaluate", "negatives"):
            assert list(got[key]) == list(one[key])
            for name in one[key]:
                assert _same(np.asarray(got[key][name]), np.asarray(one[key][name])), (r, key, name)


def test_argument_errors_of_predict_and_evaluate(ml_model):
    model, train, held = ml_model
    for bad in (-0.01, 1.01, float("nan"), "0.5", True):
        with pytest.raises(ValueError):
            model.predict(train, 5, diversify=bad)
        with pytest.raises(ValueError):
            model.evaluate(train, held, 5, diversify=bad)
    with pytest.raises(ValueError):
        model.predict(train, 5, pool=50)                                         # pool without diversify
    with pytest.raises(ValueError):
        model.evaluate(train, held, 5, pool=50)
    for pool in (4, 8193, 50.0):
        with pytest.raises(ValueError):
            model.predict(train, 5, diversify=0.5, pool=pool)
    with pytest.raises(ValueError):
        model.evaluate(train, held, (5, 10), diversify=0.5, pool=9)              # below max(k)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
ENTRIES = ("rsparse_hip_mmr_rerank_device", "rsparse_hip_mmr_rerank_f64_device", "rsparse_hip_mmr_rerank", "rsparse_hip_mmr_rerank_f64")


def test_library_exports_the_new_entry_points():
    lib = _lib.load()
    header = (ROOT / "include" / "rsparse_wrmf_hip.h").read_text()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and ("int %s(" % name) in header
    assert lib.rsparse_hip_abi_version() == 6


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_status_codes_without_device():
    lib = _lib.load()
    lists = np.asfortranarray(np.array([[3, 1, 2], [NA, 2, 1]], dtype=np.int32))       # 2 users x a pool of 3
    sc = np.asfortranarray(np.array([[3.0, 2.0, 1.0], [np.nan, 2.0, 1.0]]))
    items, pos = np.empty((2, 2), np.int32), np.empty((2, 2), np.int32)
    picked, obj, inv = np.empty((2, 2)), np.empty((2, 2)), np.empty(3)
    for sfx, dt in (("", np.float32), ("_f64", np.float64)):
        V = np.ones((3, 300), dtype=dt)

        def call(form, lists, sc, n, N, k, theta, V, n_items, ld, c0, c1, inv, items, picked=picked, pos=pos, obj=obj):
            head = [_vp(lists), _vp(sc), n, N, k, theta, _vp(V), n_items, ld, c0, c1]
            if form == "host":
                return getattr(lib, "rsparse_hip_mmr_rerank" + sfx)(*head, _vp(items), _vp(picked), _vp(pos), _vp(obj))
            # (host pointers: every device-form call here is rejected by the argument checks, or is the n_users = 0 no-op)
            return getattr(lib, "rsparse_hip_mmr_rerank%s_device" % sfx)(*head, _vp(inv), _vp(items), _vp(picked), _vp(pos), _vp(obj),
                                                                      None)
        for form in ("host", "device"):
            c = lambda *a, **kw: call(form, *a, **kw)
            assert c(None, sc, 2, 3, 2, 0.5, V, 3, 300, 0, 4, inv, items) == _lib.ERR_INVALID
            assert c(lists, None, 2, 3, 2, 0.5, V, 3, 300, 0, 4, inv, items) == _lib.ERR_INVALID
            assert c(lists, sc, 2, 3, 2, 0.5, None, 3, 300, 0, 4, inv, items) == _lib.ERR_INVALID
            assert c(lists, sc, 2, 3, 2, 0.5, V, 3, 300, 0, 4, inv, None) == _lib.ERR_INVALID        # the items are not nullable
            assert c(lists, sc, -1, 3, 2, 0.5, V, 3, 300, 0, 4, inv, items) == _lib.ERR_INVALID
            assert c(lists, sc, 2, 3, 0, 0.5, V, 3, 300, 0, 4, inv, items) == _lib.ERR_INVALID       # k < 1
            assert c(lists, sc, 2, 3, 4, 0.5, V, 3, 300, 0, 4, inv, items) == _lib.ERR_INVALID       # k > N
            assert c(lists, sc, 2, 0, 0, 0.5, V, 3, 300, 0, 4, inv, items) == _lib.ERR_INVALID
            for theta in (-0.001, 1.001, float("nan"), float("inf"), -float("inf")):
                assert c(lists, sc, 2, 3, 2, theta, V, 3, 300, 0, 4, inv, items) == _lib.ERR_INVALID
            assert c(lists, sc, 2, 3, 2, 0.5, V, 0, 300, 0, 4, inv, items) == _lib.ERR_INVALID       # no items
            assert c(lists, sc, 2, 3, 2, 0.5, V, 3, 300, 4, 4, inv, items) == _lib.ERR_INVALID       # an empty window
            assert c(lists, sc, 2, 3, 2, 0.5, V, 3, 300, -1, 4, inv, items) == _lib.ERR_INVALID
            assert c(lists, sc, 2, 3, 2, 0.5, V, 3, 300, 0, 301, inv, items) == _lib.ERR_INVALID     # beyond ld
            assert c(lists, sc, 2, 3, 2, 0.5, V, 3, 300, 0, 257, inv, items) == _lib.ERR_UNSUPPORTED
            assert c(lists, sc, 2, 8193, 2, 0.5, V, 3, 300, 0, 4, inv, items) == _lib.ERR_UNSUPPORTED
            assert c(lists, sc, 0, 3, 2, 0.5, V, 3, 300, 0, 4, inv, items) == _lib.OK                # n_users = 0: a no-op
            assert c(lists, sc, 0, 3, 2, 0.0, V, 3, 300, 0, 4, inv, items, None, None, None) == _lib.OK
        assert call("device", lists, sc, 2, 3, 2, 0.5, V, 3, 300, 0, 4, None, items) == _lib.ERR_INVALID     # no norms
        # a valid host call gets past every argument check (no device here -> a runtime error), with the items alone too
        ok = lambda rc: rc not in (_lib.ERR_INVALID, _lib.ERR_UNSUPPORTED)
        assert ok(call("host", lists, sc, 2, 3, 2, 1.0, V, 3, 300, 0, 4, inv, items))
        assert ok(call("host", lists, sc, 2, 3, 3, 0.0, V, 3, 300, 1, 257, inv, np.empty((2, 3), np.int32), None, None, None))
