"""Pointwise predictions on the device (wrmf_score.hip behind rsparse_hip_score_pairs_device / _f64_device and
rsparse_hip_sparse_approximation; `WRMF.score`, `WRMF.evaluate_values`): every stored position against numpy float64 within
the derived bound (tests/test_score_abi.py: score_bound), the error sums per row, repeat calls bit for bit, and the class on
MovieLens -- tied to `predict`'s scores."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from test_score_abi import out_rounding, ref_scores, score_bound

pytestmark = pytest.mark.gpu

N_ROWS, N_COLS = 300, 6000
BASE_LENS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
_cache = {}


def _pattern():
    """300 x 6000: the lengths around every lane-group / wave / error-sum boundary repeated, one row of 5000, a trailing empty
    row; 19203 stored positions (not a multiple of 64: the last lane group and the last wave are partial), columns unsorted"""
    if "pat" not in _cache:
        rng = np.random.default_rng(5)
        lens = np.tile(BASE_LENS, 20)[:N_ROWS].copy()
        lens[N_ROWS - 2], lens[N_ROWS - 1] = 5000, 0
        p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        assert p[-1] == 19203 and p[-1] % 64
        j = np.concatenate([rng.choice(N_COLS, size=l, replace=False) for l in lens]).astype(np.int32)
        act = rng.integers(1, 6, size=j.size).astype(np.float64)
        _cache["pat"] = (lens, p, j, act)
    return _cache["pat"]


def _factors(r, dt):
    """factors of rank r and their numpy reference at the pattern, computed once per (rank, type)"""
    key = (r, np.dtype(dt).name)
    if key not in _cache:
        rng = np.random.default_rng(100 + r)
        U = rng.standard_normal((N_ROWS, r)).astype(dt)
        V = rng.standard_normal((N_COLS, r)).astype(dt)
        _, p, j, _ = _pattern()
        _cache[key] = (U, V) + ref_scores(U, V, p, j, 0.0)
    return _cache[key]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _call(U, V, p, j, add=0.0, actual=None, scores=True, sse=False, sae=False):
    """one call of the device entry of the factors' type: (scores, sse, sae) as numpy, None for what was not asked for"""
    from rsparse_amd import _lib
    lib = _lib.load()
    fn = lib.rsparse_hip_score_pairs_f64_device if U.dtype == torch.float64 else lib.rsparse_hip_score_pairs_device
    n, r = U.shape
    d_sc = torch.full((int(j.numel()),), -7.0, dtype=torch.float64, device=U.device) if scores else None
    d_sse = torch.full((n,), -7.0, dtype=torch.float64, device=U.device) if sse else None
    d_sae = torch.full((n,), -7.0, dtype=torch.float64, device=U.device) if sae else None
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(fn(U.data_ptr(), V.data_ptr(), n, int(V.shape[0]), r, p.data_ptr(), j.data_ptr(), float(add), ptr(actual),
                  ptr(d_sc), ptr(d_sse), ptr(d_sae), None))
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (d_sc, d_sse, d_sae))


def _check_sums(sc, act, p, sse, sae):
    """per row against numpy on the device's own scores: every term is non-negative, so any order is within (len + 1) roundings
    of the sum and one of each term: 2 (len + 2) 2^-52 relative; exact zeros for the empty rows"""
    d = sc - act
    for u in range(p.size - 1):
        e = d[p[u]:p[u + 1]]
        rel = 2.0 * (e.size + 2) * 2.0 ** -52
        r2, r1 = float(np.sum(e * e)), float(np.sum(np.abs(e)))
        if sse is not None:
            assert abs(sse[u] - r2) <= rel * r2, (u, e.size, sse[u], r2)
        if sae is not None:
            assert abs(sae[u] - r1) <= rel * r1, (u, e.size, sae[u], r1)


def _device_case(r, dt):
    lens, p, j, act = _pattern()
    U, V, ref, absdot = _factors(r, dt)
    dU, dV, dp, dj, dact = _dev(U), _dev(V), _dev(p), _dev(j), _dev(act)
    tol = score_bound(absdot, ref, r)
    # every output, add = 0
    sc, sse, sae = _call(dU, dV, dp, dj, 0.0, dact, True, True, True)
    err = np.abs(sc - ref)
    print("rank %d %s: max |score - ref| / bound = %.3g" % (r, np.dtype(dt).name, float(np.max(err / tol))))
    assert np.all(err <= tol), (r, int(np.argmax(err / tol)))
    _check_sums(sc, act, p, sse, sae)
    assert np.all(sse[lens == 0] == 0.0) and np.all(sae[lens == 0] == 0.0)
    # scores only, with a global bias
    add = 0.625
    sc_b, none1, none2 = _call(dU, dV, dp, dj, add, None, True, False, False)
    assert none1 is None and none2 is None
    assert np.all(np.abs(sc_b - (ref + add)) <= score_bound(absdot, ref + add, r))
    # the sums only: the scores stay in the library's workspace, and are the same scores
    none0, sse2, sae2 = _call(dU, dV, dp, dj, 0.0, dact, False, True, True)
    assert none0 is None and np.array_equal(sse2, sse) and np.array_equal(sae2, sae)
    _, sse3, none3 = _call(dU, dV, dp, dj, 0.0, dact, False, True, False)
    assert none3 is None and np.array_equal(sse3, sse)
    # a repeated call returns the same bits
    sc2, sse4, sae4 = _call(dU, dV, dp, dj, 0.0, dact, True, True, True)
    assert np.array_equal(sc2.view(np.int64), sc.view(np.int64))
    assert np.array_equal(sse4.view(np.int64), sse.view(np.int64)) and np.array_equal(sae4.view(np.int64), sae.view(np.int64))


@pytest.mark.parametrize("r", [1, 3, 4, 10, 12, 64, 100, 128, 130, 256])
def test_device_entry_fp32(r):
    _device_case(r, np.float32)


@pytest.mark.parametrize("r", [3, 10, 64, 128, 256])
def test_device_entry_fp64(r):
    _device_case(r, np.float64)


def test_unaligned_operands_take_the_element_path():
    """a factor matrix that starts 4 bytes past a 16-byte boundary (a view into a larger buffer) at a rank that is a multiple of 4"""
    _, p, j, _ = _pattern()
    U, V, ref, absdot = _factors(12, np.float32)
    buf = torch.zeros(V.size + 1, dtype=torch.float32, device="cuda:0")
    dV = buf[1:].view(N_COLS, 12)
    dV.copy_(_dev(V))
    assert dV.data_ptr() % 16 == 4
    sc, _, _ = _call(_dev(U), dV, _dev(p), _dev(j))
    assert np.all(np.abs(sc - ref) <= score_bound(absdot, ref, 12))


def test_three_million_pairs_at_rank_8():
    """3 000 001 positions over 1000 x 1000 (columns repeat within rows): more than the resident grid covers in one pass, the
    smallest lane groups, and a last chunk of one position"""
    rng = np.random.default_rng(8)
    n, r, nnz = 1000, 8, 3_000_001
    lens = np.full(n, nnz // n)
    lens[n // 2] += nnz - lens.sum()
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    j = rng.integers(0, n, size=nnz).astype(np.int32)
    act = rng.integers(1, 6, size=nnz).astype(np.float64)
    U = rng.standard_normal((n, r)).astype(np.float32)
    V = rng.standard_normal((n, r)).astype(np.float32)
    ref, absdot = ref_scores(U, V, p, j, 0.25)
    sc, sse, sae = _call(_dev(U), _dev(V), _dev(p), _dev(j), 0.25, _dev(act), True, True, True)
    assert np.all(np.abs(sc - ref) <= score_bound(absdot, ref, r))
    d = sc - act
    rows = np.repeat(np.arange(n), lens)
    r2, r1 = np.bincount(rows, d * d, n), np.bincount(rows, np.abs(d), n)
    rel = 2.0 * (lens + 2) * 2.0 ** -52
    assert np.all(np.abs(sse - r2) <= rel * r2) and np.all(np.abs(sae - r1) <= rel * r1)


def test_all_empty_pattern_and_zero_rows():
    U, V, _, _ = _factors(4, np.float32)
    dU, dV = _dev(U), _dev(V)
    p = torch.zeros(N_ROWS + 1, dtype=torch.int32, device="cuda:0")
    j = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    act = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    _, sse, sae = _call(dU, dV, p, j, 0.0, act, False, True, True)          # the sums alone: zeroed, nothing scored
    assert np.all(sse == 0.0) and np.all(sae == 0.0)
    sc, sse, sae = _call(dU, dV, p, j, 0.0, act, True, True, True)
    assert np.all(sse == 0.0) and np.all(sae == 0.0) and sc[0] == -7.0      # no position is written
    from rsparse_amd.engine import HipBackend
    be = HipBackend(0)
    sc, sse, sae = be.score_pairs(dU, dV, p, j[:0], 0.5, act[:0])
    assert sc.numel() == 0 and float(sse.abs().sum()) == 0.0 and float(sae.abs().sum()) == 0.0


def test_host_entry_csr_and_csc_give_the_same_values():
    from rsparse_amd import als
    rng = np.random.default_rng(11)
    n, m, r = 37, 29, 10
    t = sp.random(n, m, density=0.2, random_state=3, format="csr")
    t.data[:] = 1.0
    X = np.asfortranarray(rng.standard_normal((r, n)))
    Y = np.asfortranarray(rng.standard_normal((r, m)))
    got_r = als.sparse_approximation(t, X, Y)
    tc = t.tocsc()
    got_c = als.sparse_approximation(tc, X, Y)
    ref, absdot = ref_scores(X.T, Y.T, t.indptr, t.indices, 0.0)
    tol = score_bound(absdot, ref, r)
    assert np.all(np.abs(got_r - ref) <= tol)
    # the same cells in CSC order
    as_r = sp.csr_matrix((got_r, t.indices, t.indptr), shape=t.shape).tocsc()
    as_r.sort_indices(); tc.sort_indices()
    assert np.array_equal(as_r.indices, tc.indices)
    refc, absc = ref_scores(Y.T, X.T, tc.indptr, tc.indices, 0.0)
    assert np.all(np.abs(got_c - refc) <= score_bound(absc, refc, r))
    assert np.all(np.abs(got_c - as_r.data) <= 2.0 * score_bound(absc, refc, r))


# ---- the class, on MovieLens ------------------------------------------------------------------------------------------------
def _ml_csr(n_user, n_item, p, i, x):
    return sp.csc_matrix((x, i, p), shape=(n_user, n_item)).tocsr()


MODELS = {
    "explicit_bias_float": dict(rank=10, lambda_=0.1, feedback="explicit", solver="cholesky", with_user_item_bias=True,
                                with_global_bias=True, precision="float"),
    "double": dict(rank=10, lambda_=0.1, feedback="explicit", solver="cholesky", precision="double"),
    "implicit_cg_128": dict(rank=128, lambda_=0.1, feedback="implicit", solver="conjugate_gradient", precision="float"),
}


def _fit(name, train):
    from rsparse_amd import WRMF
    if name not in _cache:
        model = WRMF(rng=1, **MODELS[name])
        model.fit_transform(train, n_iter=3, convergence_tol=-1)
        _cache[name] = model
    return _cache[name]


@pytest.mark.parametrize("name", list(MODELS))
def test_class_score_on_movielens(ml_train, name):
    from rsparse_amd.metrics import canonical_actual
    train = _ml_csr(*ml_train)
    model = _fit(name, train)
    x = train[:200]
    emb = model.transform(x).astype(np.float64)
    comp = np.asarray(model.components, dtype=np.float64)
    r = comp.shape[0]
    # score at the pattern of x itself
    pat = canonical_actual(x, x.shape[0])
    ref, absdot = ref_scores(emb, comp.T, pat.indptr, pat.indices, model.global_bias)
    tol = score_bound(absdot, ref, r)
    got = model.score(x, x)
    assert sp.isspmatrix_csr(got) and got.dtype == model._np_dtype()
    assert np.array_equal(got.indptr, pat.indptr) and np.array_equal(got.indices, pat.indices)
    assert np.all(np.abs(got.data.astype(np.float64) - ref) <= tol + out_rounding(model, ref))
    sc, _, _ = model._score_device(sp.csr_matrix(x, dtype=np.float64), pat, False, True)   # the doubles, before they are stored
    sc = sc.cpu().numpy()
    assert np.all(np.abs(sc - ref) <= tol)
    # the cells `predict` returns: the same scores (both sides are doubles stored in the model's precision)
    top = model.predict(x, 10, not_recommend=None)
    assert (np.asarray(top) >= 0).all()
    rows = np.repeat(np.arange(x.shape[0]), 10)
    cells = sp.csr_matrix((np.ones(rows.size), (rows, np.asarray(top).ravel())), shape=x.shape)
    got_top = model.score(x, cells)
    ptop = np.take_along_axis(np.asarray(top.scores, dtype=np.float64), np.argsort(np.asarray(top), axis=1), axis=1).ravel()
    ref_t, abs_t = ref_scores(emb, comp.T, got_top.indptr, got_top.indices, model.global_bias)
    tol_t = score_bound(abs_t, ref_t, r) + 2.0 * out_rounding(model, ref_t)
    assert np.all(np.abs(got_top.data.astype(np.float64) - ptop) <= tol_t)
    # evaluate_values is the RMSE / MAE of those scores
    ev = model.evaluate_values(x, x, per_user=True)
    d = sc - pat.data
    rel = 2.0 * (pat.nnz + 2) * 2.0 ** -52
    assert ev["n"] == pat.nnz
    assert abs(ev["rmse"] - np.sqrt(np.mean(d * d))) <= rel * ev["rmse"]
    assert abs(ev["mae"] - np.mean(np.abs(d))) <= rel * ev["mae"]
    u = 7
    e = d[pat.indptr[u]:pat.indptr[u + 1]]
    assert abs(ev["rmse_per_user"][u] - np.sqrt(np.mean(e * e))) <= rel * ev["rmse_per_user"][u]
    ev2 = model.evaluate_values(x, x, per_user=True)
    assert ev2["rmse"] == ev["rmse"] and ev2["mae"] == ev["mae"] and np.array_equal(ev2["mae_per_user"], ev["mae_per_user"])


def test_held_out_rmse_beats_the_global_mean(movielens, ml_train):
    """the 43 held-out users: embedded from every second rating of theirs, judged on the others"""
    from conftest import csc_drop_rows
    n_user, n_item, p, i, x = movielens
    train = _ml_csr(*ml_train)
    model = _fit("explicit_bias_float", train)
    cv = _ml_csr(n_user - 900, n_item, *csc_drop_rows(900, p, i, x))
    seen, held = cv.copy(), cv.copy()
    seen.data[1::2] = 0.0
    held.data[0::2] = 0.0
    seen.eliminate_zeros(); held.eliminate_zeros()
    ev = model.evaluate_values(seen, held)
    mean = train.data.mean()
    base = float(np.sqrt(np.mean((held.data - mean) ** 2)))
    print("held-out rmse %.4f, global mean %.4f, n = %d" % (ev["rmse"], base, ev["n"]))
    assert ev["n"] == held.nnz and ev["rmse"] < base
