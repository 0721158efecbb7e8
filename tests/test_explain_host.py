"""`WRMF.explain` without a device: the class through the CPU stand-in backend (its torch fallback `_explain_host`) against a numpy
float64 oracle written here -- per user A_u from the inputs in double, np.linalg.solve, then the contributions --, `total` against
`score`, the argument checks, the top-n selection against a numpy argsort, two ranks under gloo, and the C ABI's argument checks,
which touch no device.

Also home of `explain_oracle`, the reference tests/test_explain.py checks the kernel against."""
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

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("rsparse_hip_explain_device", "rsparse_hip_explain_f64_device")


def explain_oracle(V, base, diag, per_nnz, x_p, x_j, wa, wb, t_p, t_j):
    """numpy float64, user by user: -> (contrib: ragged, one segment of len(row) per target in target order; total; indptr;
    scale: sum |contrib| of the target's segment, 1 for an empty row).  Inputs of any float type, converted to double first."""
    V = np.asarray(V, dtype=np.float64)
    k = V.shape[1]
    B = np.zeros((k, k)) if base is None else np.asarray(base, dtype=np.float64)
    wa, wb = np.asarray(wa, dtype=np.float64), np.asarray(wb, dtype=np.float64)
    lens = np.diff(x_p).astype(np.int64)
    indptr = np.concatenate([[0], np.cumsum(np.repeat(lens, np.diff(t_p)))]).astype(np.int64)
    contrib = np.zeros(indptr[-1])
    total, scale = np.zeros(len(t_j)), np.ones(len(t_j))
    for u in range(len(x_p) - 1):
        q0, q1 = t_p[u], t_p[u + 1]
        if q1 == q0 or lens[u] == 0:
            continue
        e = slice(x_p[u], x_p[u + 1])
        Y = V[x_j[e]]
        A = B + (diag + per_nnz * lens[u]) * np.eye(k) + (Y * wa[e][:, None]).T @ Y
        Z = np.linalg.solve(A, V[t_j[q0:q1]].T)               # k x targets
        C = (Y @ Z) * wb[e][:, None]                          # positions x targets
        for q in range(q0, q1):
            contrib[indptr[q]:indptr[q + 1]] = C[:, q - q0]
        total[q0:q1] = C.sum(axis=0)
        scale[q0:q1] = np.abs(C).sum(axis=0)
    return contrib, total, indptr, scale


def top_n_oracle(contrib, indptr, items, n):
    """numpy: the n largest of every segment, descending, equal values with the lower item first, padded with -1 / 0"""
    n_pairs = len(indptr) - 1
    ti, tc = np.full((n_pairs, n), -1, dtype=np.int64), np.zeros((n_pairs, n))
    for q in range(n_pairs):
        c, it = contrib[indptr[q]:indptr[q + 1]], items[indptr[q]:indptr[q + 1]]
        order = np.lexsort((it, -c))[:n]                      # by -c, ties by item
        ti[q, :order.size], tc[q, :order.size] = it[order], c[order]
    return ti, tc


def model_oracle(model, x, pat):
    """the oracle on a fitted (or hand-made) model's own factors: x canonical CSR with the preprocessed values, pat the pattern"""
    c = np.asarray(x.data, dtype=np.float64)
    V = model._V.cpu().numpy()
    if model._feedback == "implicit":
        args = (model._XtX.cpu().numpy(), 0.0, 0.0, c - 1.0)
    else:
        args = (None,) + ((0.0, model._lambda) if model._dynamic_lambda else (model._lambda, 0.0)) + (np.ones_like(c),)
    base, diag, per, wa = args
    return explain_oracle(V, base, diag, per, x.indptr, x.indices, wa, c, pat.indptr, pat.indices)


# ---- the class through the CPU stand-in -------------------------------------------------------------------------------------
def _backend():
    sys.path.insert(0, str(ROOT / "tests"))
    from oracle_backend import OracleBackend
    return OracleBackend()


def _problem():
    """157 x 53, row lengths 0 .. 40 (the problem of tests/test_score_abi.py) and a pattern of pairs with stored zeros"""
    rng = np.random.default_rng(17)
    n_user, n_item = 157, 53
    lens = np.clip(rng.lognormal(1.5, 1.0, n_user).astype(int), 0, 40)
    rows = np.repeat(np.arange(n_user), lens)
    cols = np.concatenate([rng.choice(n_item, size=l, replace=False) for l in lens])
    m = sp.csr_matrix((1.0 + rng.geometric(0.5, size=rows.size), (rows, cols)), shape=(n_user, n_item))
    pairs = sp.csr_matrix((rng.random((n_user, n_item)) < 0.08) * rng.integers(1, 5, (n_user, n_item)).astype(float))
    pairs.data[::7] = 0.0
    assert (lens == 0).any() and (np.diff(pairs.indptr)[lens == 0] > 0).any()   # a user with targets and an empty row
    return m, pairs


CONFIGS = {
    "implicit": dict(feedback="implicit", solver="conjugate_gradient", lambda_=0.1),
    "explicit_dynamic": dict(feedback="explicit", solver="cholesky", lambda_=0.1, dynamic_lambda=True),
    "explicit_fixed": dict(feedback="explicit", solver="cholesky", lambda_=0.5, dynamic_lambda=False),
}
_fits = {}


def _fit(name, data, m):
    from rsparse_amd import WRMF
    if (name, data) not in _fits:
        model = WRMF(rank=8, precision="double", backend=_backend(), rng=1, **CONFIGS[name])
        model.fit_transform(m, n_iter=2, convergence_tol=-1)
        _fits[(name, data)] = model
    return _fits[(name, data)]


def _check_against_oracle(model, x, pairs):
    from rsparse_amd.metrics import canonical_actual
    from rsparse_amd.wrmf import Explanation
    pat = canonical_actual(pairs, x.shape[0])
    xc = sp.csr_matrix(x, dtype=np.float64)
    xc.sum_duplicates()
    contrib, total, indptr, scale = model_oracle(model, xc, pat)
    ex = model.explain(x, pairs)
    assert isinstance(ex, Explanation) and ex.top_items is None and ex.top_contrib is None
    assert np.array_equal(ex.pairs_indptr, pat.indptr) and np.array_equal(ex.pairs_indices, pat.indices)
    assert ex.indptr.dtype == np.int64 and np.array_equal(ex.indptr, indptr)
    assert ex.total.dtype == np.float64 and ex.contrib.dtype == model._np_dtype() and ex.items.dtype == np.int32
    users = np.repeat(np.arange(x.shape[0]), np.diff(pat.indptr))
    want_items = np.concatenate([xc.indices[xc.indptr[u]:xc.indptr[u + 1]] for u in users] + [np.zeros(0, np.int32)])
    assert np.array_equal(ex.items, want_items)
    seg = np.repeat(np.arange(pat.nnz), np.diff(indptr))
    assert np.all(np.abs(ex.contrib - contrib) <= 1e-10 * scale[seg])
    assert np.all(np.abs(ex.total - total) <= 1e-10 * scale)
    # the decomposition is of the score `transform` + `score` give
    sc = model.score(x, pairs)
    assert np.array_equal(sc.indices, pat.indices)
    assert np.all(np.abs(ex.total - sc.data) <= 1e-10 * scale)
    empty = np.diff(xc.indptr)[users] == 0
    assert np.all(ex.total[empty] == 0.0)
    return ex, (contrib, total, indptr, scale)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_explain_equals_the_oracle_on_the_synthetic_problem(name):
    m, pairs = _problem()
    model = _fit(name, "synth", m)
    for p in (pairs, pairs.tocsc(), pairs.tocoo()):
        _check_against_oracle(model, m, p)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_explain_equals_the_oracle_on_movielens(ml_train, name):
    n_user, n_item, p, i, v = ml_train
    train = sp.csc_matrix((v, i, p), shape=(n_user, n_item)).tocsr()
    model = _fit(name, "ml", train)
    x = train[:60]
    top = np.asarray(model.predict(x, 5))
    rows = np.repeat(np.arange(x.shape[0]), 5)
    rows, cols = np.append(rows, 3), np.append(top.ravel(), x[3].indices[0])   # and a target that is an item of the user's own row
    pairs = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=x.shape)
    _check_against_oracle(model, x, pairs)


def test_preprocess_and_duplicates_are_applied_as_in_transform():
    from rsparse_amd import WRMF
    m, pairs = _problem()

    def pre(c):
        c = c.copy()
        c.data = 1.0 + 2.0 * np.log1p(c.data)
        return c
    model = WRMF(rank=6, precision="double", backend=_backend(), rng=2, preprocess=pre, **CONFIGS["implicit"])
    model.fit_transform(m, n_iter=2, convergence_tol=-1)
    from rsparse_amd.metrics import canonical_actual
    pat = canonical_actual(pairs, m.shape[0])
    want = model_oracle(model, sp.csr_matrix(pre(m)), pat)
    ex = model.explain(m, pairs)
    assert np.all(np.abs(ex.total - want[1]) <= 1e-10 * want[3])
    # an entry split into two stored duplicates is the same entry
    coo = m.tocoo()
    dup = sp.coo_matrix((np.concatenate([coo.data[:5] - 0.25, [0.25] * 5, coo.data[5:]]),
                         (np.concatenate([coo.row[:5], coo.row[:5], coo.row[5:]]),
                          np.concatenate([coo.col[:5], coo.col[:5], coo.col[5:]]))), shape=m.shape)
    ex2 = model.explain(dup, pairs)
    assert np.array_equal(ex2.indptr, ex.indptr) and np.all(np.abs(ex2.total - ex.total) <= 1e-10 * want[3])


def test_float_model_returns_float_contributions():
    from rsparse_amd import WRMF
    m, pairs = _problem()
    model = WRMF(rank=6, precision="float", backend=_backend(), rng=3, **CONFIGS["explicit_dynamic"])
    model.fit_transform(m, n_iter=2, convergence_tol=-1)
    from rsparse_amd.metrics import canonical_actual
    pat = canonical_actual(pairs, m.shape[0])
    contrib, total, indptr, scale = model_oracle(model, sp.csr_matrix(m, dtype=np.float64), pat)
    ex = model.explain(m, pairs, n=2)
    assert ex.contrib.dtype == np.float32 and ex.top_contrib.dtype == np.float32 and ex.total.dtype == np.float64
    seg = np.repeat(np.arange(pat.nnz), np.diff(indptr))
    assert np.all(np.abs(ex.contrib - contrib) <= 1e-10 * scale[seg] + 2.0 ** -24 * np.abs(contrib))
    assert np.all(np.abs(ex.total - total) <= 1e-10 * scale)          # (the float32 factors enter both sides alike)


# ---- arguments -----------------------------------------------------------------------------------------------------------
def _hand_made(rank=6, n_item=53, **kw):
    """a model that was never fitted: random item factors and their Gramian set by hand (what explain / transform read)"""
    from rsparse_amd import WRMF
    args = dict(rank=rank, lambda_=0.1, feedback="implicit", solver="conjugate_gradient", precision="double", backend=_backend())
    args.update(kw)
    model = WRMF(**args)
    rng = np.random.default_rng(4)
    k = model._rank
    V = 0.3 * rng.standard_normal((n_item, k))
    model._V = torch.from_numpy(V).to(model._dev_t())
    model._XtX = torch.from_numpy(V.T @ V + 0.1 * np.eye(k)).to(model._dev_t())
    model.components = np.asfortranarray(V.T)
    return model


def test_argument_checks():
    from rsparse_amd import WRMF
    m, pairs = _problem()
    with pytest.raises(RuntimeError):
        WRMF(rank=4, precision="float").explain(m, pairs)                     # not fitted
    model = _hand_made()
    with pytest.raises(ValueError, match="ncol"):
        model.explain(m[:, :50], pairs)
    with pytest.raises(ValueError):
        model.explain(m, pairs[:10])
    with pytest.raises(ValueError):
        model.explain(m, pairs[:, :50])
    with pytest.raises(TypeError):
        model.explain(m, pairs.toarray())
    with pytest.raises(ValueError):
        model.explain(m, pairs, n=0)
    assert model.explain(m, sp.csr_matrix(pairs.shape)).total.size == 0       # no pair at all


def test_unsupported_configurations_name_the_option():
    m, pairs = _problem()
    cases = [(dict(solver="nnls"), {}, "nnls"),
             (dict(feedback="explicit", solver="cholesky", with_user_item_bias=True), {}, "with_user_item_bias"),
             (dict(), dict(global_bias=0.25), "global bias"),
             (dict(rank=129, precision="float"), {}, "rank > 128")]
    for kw, attrs, word in cases:
        model = _hand_made(**kw)
        for name, v in attrs.items():
            setattr(model, name, v)
        with pytest.raises(_lib.UnsupportedOnDevice, match=word):
            model.explain(m, pairs)


# ---- top-n ---------------------------------------------------------------------------------------------------------------
def test_top_n_selection_against_numpy():
    from rsparse_amd.engine import explain_top_n
    rng = np.random.default_rng(9)
    lens = np.array([0, 1, 2, 3, 4, 7, 40, 3, 0, 5])
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    contrib = rng.standard_normal(indptr[-1]).round(1)                        # one decimal: many equal values
    contrib[indptr[7]:indptr[8]] = 0.5                                        # a segment of equal contributions
    items = np.concatenate([np.sort(rng.choice(100, size=l, replace=False)) for l in lens]).astype(np.int32)
    assert np.unique(contrib[indptr[6]:indptr[7]]).size < 40
    for n in (1, 3, 5):
        ti, tc = explain_top_n(torch.from_numpy(contrib), torch.from_numpy(indptr), torch.from_numpy(items), n)
        wi, wc = top_n_oracle(contrib, indptr, items, n)
        assert ti.dtype == torch.int32 and np.array_equal(ti.numpy(), wi) and np.array_equal(tc.numpy(), wc)
    assert np.array_equal(wi[7, :3], items[indptr[7]:indptr[8]])              # equal values: ascending items
    assert np.all(wi[0] == -1) and np.all(wc[0] == 0.0) and wi[1, 1] == -1    # rows shorter than n are padded


def test_explain_with_n_on_a_model_with_tied_items():
    model = _hand_made()
    V = model._V.numpy().copy()
    V[7] = V[5]
    V[30] = V[5]                                                              # items 5, 7, 30: the same factors
    model._V = torch.from_numpy(V)
    model._XtX = torch.from_numpy(V.T @ V + 0.1 * np.eye(V.shape[1]))
    x = sp.csr_matrix((np.array([2.0, 2.0, 3.0, 2.0, 1.5, 4.0]), (np.zeros(6, int), np.array([5, 7, 11, 30, 40, 2]))), shape=(3, 53))
    x = sp.vstack([x[0], sp.csr_matrix(([1.0, 2.0], ([0, 0], [3, 9])), shape=(1, 53)), sp.csr_matrix((1, 53))]).tocsr()
    pairs = sp.csr_matrix((np.ones(5), ([0, 0, 1, 1, 2], [1, 5, 0, 9, 4])), shape=(3, 53))
    from rsparse_amd.metrics import canonical_actual
    pat = canonical_actual(pairs, 3)
    contrib, total, indptr, scale = model_oracle(model, x, pat)
    items = np.concatenate([x[u].indices for u in (0, 0, 1, 1)]).astype(np.int32)
    n = 4
    ex = model.explain(x, pairs, n=n)
    wi, wc = top_n_oracle(ex.contrib, indptr, items, n)                       # the selection, on the values it was made from
    assert np.array_equal(ex.top_items, wi) and np.array_equal(ex.top_contrib, wc)
    assert ex.top_items.shape == (5, n) and ex.top_items.dtype == np.int32
    assert np.all(np.abs(ex.top_contrib - top_n_oracle(contrib, indptr, items, n)[1]) <= 1e-10 * scale[:, None])
    assert np.all(ex.top_items[2:4, 2:] == -1) and np.all(ex.top_contrib[2:4, 2:] == 0.0)   # a row of 2 entries, n = 4
    assert np.all(ex.top_items[4] == -1) and ex.total[4] == 0.0                             # an empty row
    for q in (0, 1):                                                          # the tied items in ascending order, side by side
        at = [int(np.flatnonzero(ex.top_items[q] == it)[0]) for it in (5, 7) if it in ex.top_items[q]]
        assert at == sorted(at)
    assert np.array_equal(ex.indptr, indptr) and np.array_equal(ex.items, items)   # the ragged arrays, copied on demand


# ---- two ranks -----------------------------------------------------------------------------------------------------------
def _worker(rank, ws, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    m, pairs = _problem()
    model = _hand_made()
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        ex = model.explain(m, pairs, n=3)
        refused = False
        try:
            model.explain(m, pairs)
        except _lib.UnsupportedOnDevice:
            refused = True
        torch.save({"total": ex.total, "top_items": ex.top_items, "top_contrib": ex.top_contrib, "items": ex.items,
                    "refused": refused}, os.path.join(out_dir, "e%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_sharded_explain_equals_one_process(tmp_path):
    import torch.multiprocessing as mp
    m, pairs = _problem()
    one = _hand_made().explain(m, pairs, n=3)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        got = torch.load(tmp_path / ("e%d.pt" % r), weights_only=False)
        assert got["refused"] and got["items"] is None
        assert np.array_equal(got["total"], one.total) and np.array_equal(got["top_items"], one.top_items)
        assert np.array_equal(got["top_contrib"], one.top_contrib)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_explain_entry_points():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.rsparse_hip_abi_version() == 6
    from rsparse_amd.engine import HipBackend
    assert callable(HipBackend.explain_pairs)


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("name,dt", [(NAMES[0], np.float32), (NAMES[1], np.float64)])
def test_status_codes_without_device(name, dt):
    # (host pointers: every call here is rejected by the argument checks, or is a no-op, before device work)
    fn = getattr(_lib.load(), name)
    V = np.ones((3, 4), dtype=dt)
    base = np.eye(4, dtype=dt)
    x_p, x_j = np.array([0, 2, 3], dtype=np.int32), np.array([0, 2, 1], dtype=np.int32)
    wa, wb = np.ones(3, dtype=dt), np.ones(3, dtype=dt)
    t_p, t_j = np.array([0, 1, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    out_p = np.array([0, 2], dtype=np.int64)
    contrib, total, flags = np.empty(3, dtype=dt), np.empty(2), np.empty(2, dtype=np.int32)

    def call(V=V, m=3, r=4, base=base, n=2, x_p=x_p, x_j=x_j, wa=wa, wb=wb, t_p=t_p, t_j=t_j, out_p=out_p, contrib=contrib,
             total=total, flags=flags):
        return fn(_vp(V), m, r, _vp(base), 0.1, 0.0, n, _vp(x_p), _vp(x_j), _vp(wa), _vp(wb), _vp(t_p), _vp(t_j), _vp(out_p),
                  _vp(contrib), _vp(total), _vp(flags), None)

    for gone in ("V", "x_p", "t_p", "flags", "x_j", "wa", "wb", "out_p", "contrib", "total"):
        assert call(**{gone: None}) == _lib.ERR_INVALID, gone
    assert call(m=-1) == _lib.ERR_INVALID
    assert call(n=-1) == _lib.ERR_INVALID
    assert call(r=0) == _lib.ERR_INVALID
    assert call(r=129) == _lib.ERR_UNSUPPORTED
    assert call(r=129, V=None) == _lib.ERR_INVALID
    assert call(n=0) == _lib.OK                                            # no user: a no-op
    assert call(n=0, base=None) == _lib.OK
    assert call(t_j=None) == _lib.OK                                       # no target at all: a no-op
    assert call(t_j=None, x_j=None, wa=None, wb=None, out_p=None, contrib=None, total=None) == _lib.OK
