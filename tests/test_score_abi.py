"""Pointwise predictions (cpp_make_sparse_approximation, src/utils.cpp:4-56) without a device: the C ABI's three entry points
exist and answer bad calls with status codes before any device work, `WRMF.score` / `WRMF.evaluate_values` through the CPU
stand-in backend equal the numpy product at the pattern, and under torch.distributed (gloo, two ranks) they return what one
process returns, bit for bit.

Also home of `score_bound`, the tolerance tests/test_score.py checks the kernels against."""
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
NAMES = ("rsparse_hip_score_pairs_device", "rsparse_hip_score_pairs_f64_device", "rsparse_hip_sparse_approximation")


def score_bound(absdot, score, r):
    """Both sides sum r exact (fp32 factors) or once-rounded (fp64) products in some order: each is within gamma_r * sum |u_c v_c|
    of the exact sum, gamma_r ~ r 2^-53 (a rounded product adds one more term of that size: the factor 4 covers both sides
    twice over), and the final `+ add` rounds once more."""
    return 4.0 * r * 2.0 ** -53 * absdot + 2.0 ** -52 * np.abs(score)


def ref_scores(U, V, p, j, add):
    """numpy float64: (scores, sum_c |u_c v_c|) at the CSR pattern (p, j), rows of U (n x r) against rows of V (n_item x r)"""
    rows = np.repeat(np.arange(U.shape[0]), np.diff(p))
    Ur, Vj = U.astype(np.float64)[rows], V.astype(np.float64)[j]
    return np.einsum("tc,tc->t", Ur, Vj) + add, np.einsum("tc,tc->t", np.abs(Ur), np.abs(Vj))


def out_rounding(model, ref):
    """what storing a double in the model's `precision` adds: half an ulp of float32 for precision = "float", nothing else"""
    return 2.0 ** -24 * np.abs(ref) if model._precision == "float" else 0.0


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_score_entry_points():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.rsparse_hip_abi_version() == 6
    from rsparse_amd import als
    from rsparse_amd.engine import HipBackend
    assert callable(als.sparse_approximation) and callable(HipBackend.score_pairs)


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _slots(dt):
    U = np.ones((2, 4), dtype=dt)
    V = np.ones((3, 4), dtype=dt)
    p = np.array([0, 2, 3], dtype=np.int32)
    j = np.array([0, 2, 1], dtype=np.int32)
    act = np.array([1.0, 2.0, 3.0])
    return U, V, p, j, act


@pytest.mark.parametrize("name,dt", [(NAMES[0], np.float32), (NAMES[1], np.float64)])
def test_device_forms_status_codes_without_device(name, dt):
    # (host pointers: every call here is rejected by the argument checks, or is the n_rows = 0 no-op, before device work)
    fn = getattr(_lib.load(), name)
    U, V, p, j, act = _slots(dt)
    sc, sse, sae = np.empty(3), np.empty(2), np.empty(2)

    def call(U=U, V=V, n=2, m=3, r=4, p=p, j=j, act=act, sc=sc, sse=sse, sae=sae):
        return fn(_vp(U), _vp(V), n, m, r, _vp(p), _vp(j), 0.5, _vp(act), _vp(sc), _vp(sse), _vp(sae), None)

    assert call(sc=None, sse=None, sae=None) == _lib.ERR_INVALID          # no output asked for
    assert call(U=None) == _lib.ERR_INVALID
    assert call(V=None) == _lib.ERR_INVALID
    assert call(p=None) == _lib.ERR_INVALID
    assert call(j=None) == _lib.ERR_INVALID
    assert call(act=None) == _lib.ERR_INVALID                              # the sums need the values
    assert call(act=None, sc=None, sae=None) == _lib.ERR_INVALID
    assert call(act=None, sc=None, sse=None) == _lib.ERR_INVALID
    assert call(n=-1) == _lib.ERR_INVALID
    assert call(m=-1) == _lib.ERR_INVALID
    assert call(r=0) == _lib.ERR_INVALID
    assert call(r=257) == _lib.ERR_UNSUPPORTED                             # RSPARSE_HIP_MAX_RANK, for both element types
    assert call(r=257, sc=None, sse=None, sae=None) == _lib.ERR_INVALID
    assert call(n=0) == _lib.OK                                            # n_rows = 0: a no-op
    assert call(n=0, act=None, sse=None, sae=None) == _lib.OK


def test_host_form_status_codes_without_device():
    fn = _lib.load().rsparse_hip_sparse_approximation
    X = np.asfortranarray(np.ones((4, 2)))      # rank x n_rows
    Y = np.asfortranarray(np.ones((4, 3)))      # rank x n_cols
    p = np.array([0, 2, 3], dtype=np.int32)     # CSR slots of a 2 x 3 template
    j = np.array([0, 2, 1], dtype=np.int32)
    pc = np.array([0, 1, 2, 3], dtype=np.int32)  # CSC slots of the same shape
    ic = np.array([0, 1, 0], dtype=np.int32)
    out = np.empty(3)

    def call(n=2, m=3, p=p, idx=j, kind=2, X=X, Y=Y, rank=4, out=out):
        return fn(n, m, _vp(p), _vp(idx), kind, _vp(X), _vp(Y), rank, _vp(out))

    for kind in (0, 3, -1):
        assert call(kind=kind) == _lib.ERR_INVALID                         # CSC = 1 or CSR = 2
    assert call(p=None) == _lib.ERR_INVALID
    assert call(idx=None) == _lib.ERR_INVALID
    assert call(X=None) == _lib.ERR_INVALID
    assert call(Y=None) == _lib.ERR_INVALID
    assert call(out=None) == _lib.ERR_INVALID
    assert call(n=-1) == _lib.ERR_INVALID
    assert call(m=-1) == _lib.ERR_INVALID
    assert call(rank=0) == _lib.ERR_INVALID
    assert call(rank=257) == _lib.ERR_UNSUPPORTED
    # the dgRMatrix / dgCMatrix slots
    assert call(p=np.array([1, 2, 3], np.int32)) == _lib.ERR_INVALID       # p[0] != 0
    assert call(p=np.array([0, 3, 2], np.int32)) == _lib.ERR_INVALID       # p decreases
    assert call(idx=np.array([0, 3, 1], np.int32)) == _lib.ERR_INVALID     # a column outside the matrix
    assert call(idx=np.array([0, -1, 1], np.int32)) == _lib.ERR_INVALID
    assert call(p=pc, idx=np.array([0, 2, 0], np.int32), kind=1) == _lib.ERR_INVALID   # CSC: a row outside the matrix
    # an empty pattern has nothing to compute
    assert call(p=np.zeros(3, np.int32), idx=None, out=None) == _lib.OK
    # a valid call gets past every argument check (no device here -> a runtime error)
    assert call() not in (_lib.ERR_INVALID, _lib.ERR_UNSUPPORTED)
    assert call(p=pc, idx=ic, kind=1) not in (_lib.ERR_INVALID, _lib.ERR_UNSUPPORTED)


def test_wrapper_argument_checks():
    from rsparse_amd import als
    t = sp.csr_matrix(np.eye(2, 3))
    X, Y = np.asfortranarray(np.ones((4, 2))), np.asfortranarray(np.ones((4, 3)))
    with pytest.raises(TypeError):
        als.sparse_approximation(np.eye(2, 3), X, Y)
    with pytest.raises(ValueError):
        als.sparse_approximation(t, X.astype(np.float32), Y)
    with pytest.raises(ValueError):
        als.sparse_approximation(t, X, np.asfortranarray(np.ones((4, 2))))


# ---- WRMF.score / evaluate_values through the CPU stand-in -----------------------------------------------------------------
def _problem():
    """the 157 x 53 problem of tests/test_metrics_abi.py, with ratings as values"""
    rng = np.random.default_rng(17)
    n_user, n_item = 157, 53
    lens = np.clip(rng.lognormal(1.5, 1.0, n_user).astype(int), 0, 40)
    rows = np.repeat(np.arange(n_user), lens)
    cols = np.concatenate([rng.choice(n_item, size=l, replace=False) for l in lens])
    m = sp.csr_matrix((1.0 + rng.geometric(0.5, size=rows.size), (rows, cols)), shape=(n_user, n_item))
    held = sp.csr_matrix((rng.random((n_user, n_item)) < 0.1) * rng.integers(1, 5, (n_user, n_item)).astype(float))
    held.data[::7] = 0.0                                              # stored zeros are positions too
    return m, held


def _model(bias):
    sys.path.insert(0, str(ROOT / "tests"))
    from oracle_backend import OracleBackend
    from rsparse_amd import WRMF
    m, held = _problem()
    model = WRMF(rank=6, lambda_=0.1, feedback="explicit", solver="cholesky", precision="float", with_user_item_bias=bias,
                 with_global_bias=bias, backend=OracleBackend(), rng=1)
    model.fit_transform(m, n_iter=2, convergence_tol=-1)   # (one process: every rank holds the same model)
    return model, m, held


@pytest.mark.parametrize("bias", [False, True])
def test_score_and_evaluate_values_equal_the_numpy_product(bias):
    model, m, held = _model(bias)
    assert (model.global_bias != 0.0) == bias
    emb = model.transform(m).astype(np.float64)
    comp = np.asarray(model.components, dtype=np.float64)            # (rank [+ 2]) x n_item
    assert emb.shape[1] == comp.shape[0] == 6 + 2 * bias
    pat = held.tocsr()
    ref, absdot = ref_scores(emb, comp.T, pat.indptr, pat.indices, model.global_bias)
    dense = emb @ comp + model.global_bias
    rows = np.repeat(np.arange(pat.shape[0]), np.diff(pat.indptr))
    tol = score_bound(absdot, ref, comp.shape[0])
    assert np.all(np.abs(dense[rows, pat.indices] - ref) <= tol)     # (the two ways of writing the reference agree)
    for pairs in (held, held.tocsc(), held.tocoo()):
        got = model.score(m, pairs)
        assert sp.isspmatrix_csr(got) and got.shape == held.shape and got.dtype == np.float32
        assert np.array_equal(got.indptr, pat.indptr) and np.array_equal(got.indices, pat.indices)   # stored zeros kept
        assert np.all(np.abs(got.data.astype(np.float64) - ref) <= tol + out_rounding(model, ref))
    # the doubles behind it, before they are stored as float32: the bound as it stands
    from rsparse_amd.metrics import canonical_actual
    sc, sse, sae = model._score_device(sp.csr_matrix(m, dtype=np.float64), canonical_actual(held, m.shape[0]), True, True)
    sc = sc.numpy()
    assert sc.dtype == np.float64 and np.all(np.abs(sc - ref) <= tol)
    d = sc - pat.data
    rel = 2.0 * (pat.nnz + 2) * 2.0 ** -52        # sums of non-negative terms, in any order, on both sides
    ev = model.evaluate_values(m, held, per_user=True)
    assert ev["n"] == pat.nnz and set(ev) == {"rmse", "mae", "n", "rmse_per_user", "mae_per_user"}
    assert abs(ev["rmse"] - np.sqrt(np.mean(d * d))) <= rel * ev["rmse"]
    assert abs(ev["mae"] - np.mean(np.abs(d))) <= rel * ev["mae"]
    cnt = np.diff(pat.indptr)
    for u in (0, 5, 100, 156):
        e = d[pat.indptr[u]:pat.indptr[u + 1]]
        if cnt[u]:
            assert abs(ev["rmse_per_user"][u] - np.sqrt(np.mean(e * e))) <= rel * ev["rmse_per_user"][u]
            assert abs(ev["mae_per_user"][u] - np.mean(np.abs(e))) <= rel * ev["mae_per_user"][u]
    assert ev["rmse_per_user"].dtype == np.float64 and ev["rmse_per_user"].shape == (m.shape[0],)
    assert np.array_equal(np.isnan(ev["rmse_per_user"]), cnt == 0) and np.array_equal(np.isnan(ev["mae_per_user"]), cnt == 0)
    assert set(model.evaluate_values(m, held)) == {"rmse", "mae", "n"}
    # nothing stored at all
    none = sp.csr_matrix(held.shape)
    assert model.score(m, none).nnz == 0
    ev0 = model.evaluate_values(m, none, per_user=True)
    assert ev0["n"] == 0 and np.isnan(ev0["rmse"]) and np.isnan(ev0["mae"]) and np.isnan(ev0["rmse_per_user"]).all()


def test_shape_errors_are_worded_like_predict():
    model, m, held = _model(False)
    with pytest.raises(ValueError, match="ncol"):
        model.score(m[:, :50], held)
    with pytest.raises(ValueError):
        model.score(m, held[:10])                       # row count
    with pytest.raises(ValueError):
        model.score(m, held[:, :50])                    # column count
    with pytest.raises(ValueError):
        model.evaluate_values(m, held[:10])
    with pytest.raises(ValueError):
        model.evaluate_values(m, held[:, :50])
    with pytest.raises(TypeError):
        model.score(m, held.toarray())
    from rsparse_amd import WRMF
    with pytest.raises(RuntimeError):
        WRMF(rank=4, precision="float").score(m, held)


# ---- two ranks --------------------------------------------------------------------------------------------------------------
def _both(model, m, held):
    return {"score": model.score(m, held), "plain": model.evaluate_values(m, held),
            "per_user": model.evaluate_values(m, held, per_user=True)}


def _worker(rank, ws, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    model, m, held = _model(True)
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        torch.save(_both(model, m, held), os.path.join(out_dir, "s%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_sharded_score_equals_one_process(tmp_path):
    import torch.multiprocessing as mp
    model, m, held = _model(True)
    one = _both(model, m, held)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        got = torch.load(tmp_path / ("s%d.pt" % r), weights_only=False)
        a, b = got["score"], one["score"]
        assert a.shape == b.shape and a.dtype == b.dtype
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data)
        for key in ("plain", "per_user"):
            assert set(got[key]) == set(one[key])
            for name in one[key]:
                assert np.array_equal(got[key][name], one[key][name], equal_nan=True), (r, key, name)
