"""Per-item contributions on the device (wrmf_explain.hip behind rsparse_hip_explain_device / _f64_device; `WRMF.explain`): every
contribution and every total against the numpy float64 oracle of tests/test_explain_host.py at the chunk, wave and rank-class
edges, untouched outputs, repeat calls bit for bit, a singular system, and the class on MovieLens tied to `score` and `predict`.

The bounds, on the error divided by the pair's sum |contribution| (1 for an empty row).  Double: 1e-9, the per-row figure of the
fp64 layer.  Float: 4 x YARDSTICK of the rank class, where the yardstick is the same error of the EXISTING path -- an exact-solver
half-iteration from zeros, then rsparse_hip_score_pairs_device -- against the same oracle scores on the same inputs
(`_yardstick_error` below measures it again on every run and prints it next to explain's; the constants are the maxima recorded in
profiles/explain/README.md).  The factor covers one more pair of triangular solves and another summation order."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from test_explain_host import explain_oracle, model_oracle, top_n_oracle

pytestmark = pytest.mark.gpu

N_USER, N_ITEM = 64, 4000
CH_F32, CH_F64 = 16, 8          # vectors per LDS chunk of the kernel (Ex<T>::CH)
BASE_LENS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257)
TARGETS = (0, 1, 2, 4, 5, 17)   # 5: one more than the workgroup has waves
LONG_USER, OWN_USER = 45, 33
LAMBDA = 0.1
SENTINEL = -7.0
BOUND_F64 = 1e-9
# max over the ranks of a class and both modes of the existing path's scaled error (profiles/explain/README.md)
YARDSTICK = {32: 1.70e-5, 64: 4.64e-6, 128: 3.01e-6}
_cache = {}


def _rank_class(r):
    return 32 if r <= 32 else 64 if r <= 64 else 128


def bound_f32(r):
    return 4.0 * YARDSTICK[_rank_class(r)]


def _rows():
    """the rows of x and the targets, shared by every rank and mode: row lengths around the chunk (8, 16), wave and 256 edges, one
    row of 3000; 0 / 1 / 2 / 4 / 5 / 17 targets per user in a cycle that shifts against the lengths"""
    if "rows" not in _cache:
        rng = np.random.default_rng(12)
        lens = np.array([BASE_LENS[u % len(BASE_LENS)] for u in range(N_USER)])
        lens[LONG_USER] = 3000
        tcnt = np.array([TARGETS[(u + u // len(BASE_LENS)) % len(TARGETS)] for u in range(N_USER)])
        assert CH_F32 - 1 in lens and CH_F32 + 1 in lens and CH_F64 - 1 in lens and CH_F64 + 1 in lens
        assert ((lens == 0) & (tcnt > 0)).any() and ((lens > 0) & (tcnt == 0)).any() and tcnt[LONG_USER] > 0 and tcnt[OWN_USER] > 1
        x_p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        x_j = np.concatenate([np.sort(rng.choice(N_ITEM, size=l, replace=False)) for l in lens]).astype(np.int32)
        c = rng.integers(1, 41, size=x_j.size).astype(np.float64)
        t_p = np.concatenate([[0], np.cumsum(tcnt)]).astype(np.int32)
        t_j = np.concatenate([np.sort(rng.choice(N_ITEM, size=t, replace=False)) for t in tcnt]).astype(np.int32)
        t_j[t_p[OWN_USER]] = x_j[x_p[OWN_USER] + 3]            # a target that is an item of the user's own row
        _cache["rows"] = (lens, tcnt, x_p, x_j, c, t_p, t_j)
    return _cache["rows"]


def _case(r, dt, mode):
    """inputs of one (rank, type, mode) in the element type and their oracle, computed once"""
    key = (r, np.dtype(dt).name, mode)
    if key not in _cache:
        lens, tcnt, x_p, x_j, c, t_p, t_j = _rows()
        V = (0.1 * np.random.default_rng(300 + r).standard_normal((N_ITEM, r))).astype(dt)
        if mode == "implicit":
            V64 = V.astype(np.float64)
            base, diag, per, wa = (V64.T @ V64 + LAMBDA * np.eye(r)).astype(dt), 0.0, 0.0, (c - 1.0).astype(dt)
        else:
            base, diag, per, wa = None, 0.0, LAMBDA, np.ones_like(c).astype(dt)
        wb = c.astype(dt)
        _cache[key] = (V, base, diag, per, wa, wb) + explain_oracle(V, base, diag, per, x_p, x_j, wa, wb, t_p, t_j)
    return _cache[key]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _call(V, base, diag, per, x_p, x_j, wa, wb, t_p, t_j, indptr, tail=64):
    """one call of the device entry of V's type on outputs pre-filled with the sentinel: (contrib with `tail` extra elements, total,
    flags) as numpy"""
    from rsparse_amd import _lib
    lib = _lib.load()
    dV = _dev(V)
    fn = lib.rsparse_hip_explain_f64_device if dV.dtype == torch.float64 else lib.rsparse_hip_explain_device
    d = [_dev(a) for a in (base, x_p, x_j, wa, wb, t_p, t_j, indptr)]
    contrib = torch.full((int(indptr[-1]) + tail,), SENTINEL, dtype=dV.dtype, device="cuda:0")
    total = torch.full((len(t_j),), SENTINEL, dtype=torch.float64, device="cuda:0")
    flags = torch.full((len(x_p) - 1,), int(SENTINEL), dtype=torch.int32, device="cuda:0")
    _lib.check(fn(dV.data_ptr(), int(V.shape[0]), int(V.shape[1]), None if base is None else d[0].data_ptr(), float(diag),
                  float(per), len(x_p) - 1, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(),
                  d[6].data_ptr(), d[7].data_ptr(), contrib.data_ptr(), total.data_ptr(), flags.data_ptr(), None))
    torch.cuda.synchronize()
    return contrib.cpu().numpy(), total.cpu().numpy(), flags.cpu().numpy()


def _yardstick_error(r, mode):
    """the existing path on the same inputs (float): an exact-solver half-iteration from zeros, then the scores at the targets;
    -> its max scaled error against the oracle's totals"""
    from rsparse_amd.engine import HipBackend
    lens, tcnt, x_p, x_j, c, t_p, t_j = _rows()
    V, base, diag, per, wa, wb, _, total, _, scale = _case(r, np.float32, mode)
    be = HipBackend(0)
    dV = _dev(V)
    csc = be.make_csc(N_ITEM, N_USER, _dev(x_p), _dev(x_j), _dev(c.astype(np.float32)))
    emb = torch.zeros((N_USER, r), dtype=torch.float32, device="cuda:0")
    loss = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    be.half_iteration(csc, mode == "implicit", dV, emb, _dev(base), LAMBDA, 0, 3, True, loss, None)
    be.check_numeric()
    sc, _, _ = be.score_pairs(emb, dV, _dev(t_p), _dev(t_j))
    return float(np.max(np.abs(sc.cpu().numpy() - total) / scale))


def _device_case(r, dt, mode):
    lens, tcnt, x_p, x_j, c, t_p, t_j = _rows()
    V, base, diag, per, wa, wb, contrib, total, indptr, scale = _case(r, dt, mode)
    got_c, got_t, got_f = _call(V, base, diag, per, x_p, x_j, wa, wb, t_p, t_j, indptr)
    n_out = int(indptr[-1])
    seg = np.repeat(np.arange(len(t_j)), np.diff(indptr))
    err_c = float(np.max(np.abs(got_c[:n_out].astype(np.float64) - contrib) / scale[seg]))
    err_t = float(np.max(np.abs(got_t - total) / scale))
    if dt == np.float32:
        yard = _yardstick_error(r, mode)
        print("rank %d float %s: explain contrib %.3g total %.3g, yardstick %.3g, ratio %.2f" %
              (r, mode, err_c, err_t, yard, max(err_c, err_t) / yard))
        bound = bound_f32(r)
    else:
        print("rank %d double %s: explain contrib %.3g total %.3g" % (r, mode, err_c, err_t))
        bound = BOUND_F64
    assert err_c <= bound and err_t <= bound, (r, mode, err_c, err_t, bound)
    # an empty row: totals exactly 0 and the flag unset; a user without targets: its flag is not written; nothing past the end
    users = np.repeat(np.arange(N_USER), tcnt)
    assert np.all(got_t[lens[users] == 0] == 0.0) and np.all(got_f[(lens == 0) & (tcnt > 0)] == 0)
    assert np.all(got_f[tcnt == 0] == int(SENTINEL)) and np.all(got_f[tcnt > 0] == 0)
    assert np.all(got_c[n_out:] == SENTINEL) and np.all(np.isfinite(got_c[:n_out])) and not np.any(got_c[:n_out] == SENTINEL)
    # a repeat call: the same bits in every output
    again = _call(V, base, diag, per, x_p, x_j, wa, wb, t_p, t_j, indptr)
    for a, b in zip((got_c, got_t, got_f), again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("mode", ["implicit", "explicit"])
@pytest.mark.parametrize("r", [8, 10, 32, 33, 64, 65, 128])
def test_device_entry_fp32(r, mode):
    _device_case(r, np.float32, mode)


@pytest.mark.parametrize("mode", ["implicit", "explicit"])
@pytest.mark.parametrize("r", [10, 64, 128])
def test_device_entry_fp64(r, mode):
    _device_case(r, np.float64, mode)


def test_users_without_targets_leave_every_output_untouched():
    """no user has a target: the call launches (t_j is given) and writes nothing at all"""
    lens, tcnt, x_p, x_j, c, t_p, t_j = _rows()
    V, base, diag, per, wa, wb = _case(8, np.float32, "implicit")[:6]
    none_p = np.zeros(N_USER + 1, dtype=np.int32)
    got_c, got_t, got_f = _call(V, base, diag, per, x_p, x_j, wa, wb, none_p, np.zeros(1, np.int32), np.zeros(1, np.int64))
    assert np.all(got_c == SENTINEL) and np.all(got_t == SENTINEL) and np.all(got_f == int(SENTINEL))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_a_singular_system_sets_the_flag_and_gives_nan(dt):
    """explicit form with diag = diag_per_nnz = 0 at rank 8: a row of 3 non-zeros makes A_u = sum of 3 outer products, singular by
    construction; rows of 200 non-zeros are well conditioned and stay within the bound"""
    rng = np.random.default_rng(77)
    r, lens = 8, np.array([200, 3, 200, 0, 200])
    x_p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    x_j = np.concatenate([np.sort(rng.choice(N_ITEM, size=l, replace=False)) for l in lens]).astype(np.int32)
    c = rng.integers(1, 41, size=x_j.size).astype(dt)
    tcnt = np.array([2, 3, 1, 2, 5])
    t_p = np.concatenate([[0], np.cumsum(tcnt)]).astype(np.int32)
    t_j = rng.integers(0, N_ITEM, size=t_p[-1]).astype(np.int32)
    V = (0.1 * rng.standard_normal((N_ITEM, r))).astype(dt)
    wa = np.ones_like(c)
    ok = np.repeat(lens != 3, tcnt)
    # (the oracle skips the singular user: np.linalg.solve would answer with noise or raise)
    t_p_ok = np.concatenate([[0], np.cumsum(np.where(lens == 3, 0, tcnt))]).astype(np.int32)
    contrib, total, indptr_ok, scale = explain_oracle(V, None, 0.0, 0.0, x_p, x_j, wa, c, t_p_ok, t_j[ok])
    indptr = np.concatenate([[0], np.cumsum(np.repeat(lens, tcnt))]).astype(np.int64)
    got_c, got_t, got_f = _call(V, None, 0.0, 0.0, x_p, x_j, wa, c, t_p, t_j, indptr)
    assert list(got_f) == [0, 1, 0, 0, 0]
    seg_ok = np.repeat(ok, np.diff(indptr))
    assert np.all(np.isnan(got_t[~ok])) and np.all(np.isnan(got_c[:indptr[-1]][~seg_ok])) and np.all(got_c[indptr[-1]:] == SENTINEL)
    bound = bound_f32(r) if dt == np.float32 else BOUND_F64
    seg = np.repeat(np.arange(int(ok.sum())), np.diff(indptr_ok))
    assert np.all(np.abs(got_t[ok] - total) <= bound * scale)
    assert np.all(np.abs(got_c[:indptr[-1]][seg_ok].astype(np.float64) - contrib) <= bound * scale[seg])


# ---- the class, on MovieLens ------------------------------------------------------------------------------------------------
MODELS = {
    "implicit_cg_float": dict(rank=10, lambda_=0.1, feedback="implicit", solver="conjugate_gradient", precision="float"),
    "explicit_cholesky_double": dict(rank=10, lambda_=0.1, feedback="explicit", solver="cholesky", precision="double"),
}


@pytest.mark.parametrize("name", list(MODELS))
def test_class_explain_on_movielens(ml_train, name):
    from rsparse_amd import WRMF
    from rsparse_amd.metrics import canonical_actual
    n_user, n_item, p, i, v = ml_train
    train = sp.csc_matrix((v, i, p), shape=(n_user, n_item)).tocsr()
    model = WRMF(rng=1, **MODELS[name])
    model.fit_transform(train, n_iter=3, convergence_tol=-1)
    x = train[:200]
    top = model.predict(x, 5)
    assert (np.asarray(top) >= 0).all()
    rows = np.repeat(np.arange(x.shape[0]), 5)
    pairs = sp.csr_matrix((np.ones(rows.size), (rows, np.asarray(top).ravel())), shape=x.shape)
    pat = canonical_actual(pairs, x.shape[0])
    xc = sp.csr_matrix(x, dtype=np.float64)
    contrib, total, indptr, scale = model_oracle(model, xc, pat)
    f32 = model._precision == "float"
    bound = bound_f32(model._rank) if f32 else BOUND_F64
    rnd = (lambda ref: 2.0 ** -24 * np.abs(ref)) if f32 else (lambda ref: 0.0)      # a double stored in the model's precision
    ex = model.explain(x, pairs, n=3)
    seg = np.repeat(np.arange(pat.nnz), np.diff(indptr))
    print("%s: max scaled error, contrib %.3g total %.3g" % (name, float(np.max(np.abs(ex.contrib - contrib) / scale[seg])),
                                                           float(np.max(np.abs(ex.total - total) / scale))))
    assert np.array_equal(ex.indptr, indptr) and np.array_equal(ex.pairs_indices, pat.indices)
    assert np.all(np.abs(ex.contrib.astype(np.float64) - contrib) <= bound * scale[seg])
    assert np.all(np.abs(ex.total - total) <= bound * scale)
    # the decomposition is of the score the model gives: `score` at the pairs and `predict`'s own scores
    sc = model.score(x, pairs)
    assert np.array_equal(sc.indices, pat.indices)
    assert np.all(np.abs(ex.total - sc.data.astype(np.float64)) <= bound * scale + rnd(total))
    ptop = np.take_along_axis(np.asarray(top.scores, dtype=np.float64), np.argsort(np.asarray(top), axis=1), axis=1).ravel()
    assert np.all(np.abs(ex.total - ptop) <= bound * scale + rnd(total))
    # the three largest contributions: the oracle's, wherever its ordering is decided by more than the bound
    items = np.concatenate([xc.indices[xc.indptr[u]:xc.indptr[u + 1]] for u in rows]).astype(np.int64)
    wi, wc = top_n_oracle(contrib, indptr, items, 3)
    assert ex.top_items.shape == (pat.nnz, 3) and ex.top_contrib.dtype == model._np_dtype()
    assert np.all(np.abs(ex.top_contrib.astype(np.float64) - wc) <= bound * scale[:, None])
    checked = 0
    for q in range(pat.nnz):
        srt = np.sort(contrib[indptr[q]:indptr[q + 1]])[::-1]
        gaps = srt[:3] - srt[1:4] if srt.size > 3 else np.zeros(0)
        if gaps.size == 3 and np.all(gaps > 2.0 * bound * scale[q]):          # (both neighbours may move by the bound)
            assert np.array_equal(ex.top_items[q], wi[q]), q
            checked += 1
    assert checked > pat.nnz // 2
