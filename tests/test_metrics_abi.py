"""Ranking metrics (ap_k / ndcg_k, R/metrics.R:31-127) without a device: the C ABI's two entry points exist and answer bad
calls with status codes before any device work, the Python functions reject a row-count mismatch, and `WRMF.evaluate` under
torch.distributed (gloo, two ranks) returns what one process returns, bit for bit.

Also home of `ref_metrics`, the line-by-line numpy restatement of R/metrics.R:93-127 that tests/test_metrics.py checks the
kernels against."""
import ctypes
import math
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
NA = -2147483648


# ---- the reference, restated ------------------------------------------------------------------------------------------------
def _ap_at_k(predicted, actual, k):                        # :93-98
    k = min(k, len(predicted), len(actual))
    pk_seq = np.isin(predicted[:k], actual)                # predicted[seq_len(k)] %in% actual
    xx = np.cumsum(pk_seq) / np.arange(1, k + 1)           # cumsum(pk_seq) / seq_along(pk_seq)
    return float(np.mean(xx)) if k else math.nan           # mean(numeric(0)) = NaN


def _dcg_at_k(pred, act_ind, act_rel, k):                  # :101-112
    k = min(k, len(pred), len(act_ind))
    pos = {int(c): t for t, c in reversed(list(enumerate(act_ind)))}   # match(): the first position
    dcg = 0.0
    for i in range(1, k + 1):
        j = pos.get(int(pred[i - 1]))
        if j is not None:
            dcg = dcg + act_rel[j] / math.log2(i + 1)
    return dcg


def _idcg_at_k(act_rel, k):                                # :115-123
    k = min(k, len(act_rel))
    if len(act_rel) == 0:
        return 1.0
    res = np.sort(act_rel)[::-1][:k]
    return float(np.sum(res / np.log2(np.arange(1, len(res) + 1) + 1)))


def _ndcg_at_k(pred, act_ind, act_rel, k):                 # :125-127
    k = min(k, len(pred), len(act_ind))
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(_dcg_at_k(pred, act_ind, act_rel, k)) / np.float64(_idcg_at_k(act_rel, k)))


def ref_metrics(pred1, actual):
    """ap_k / ndcg_k (:31-89) of R-style predictions (n x k, 1-based, NA) against a canonical CSR `actual`: (ap, ndcg)."""
    n, k = pred1.shape
    ap, ndcg = np.empty(n), np.empty(n)
    for u in range(n):
        p1, p2 = actual.indptr[u], actual.indptr[u + 1]
        u_ind = actual.indices[p1:p2].astype(np.int64) + 1
        u_x = actual.data[p1:p2]
        ord_ = np.argsort(-u_x, kind="stable")              # order(u_x, decreasing = TRUE)
        pr = pred1[u].astype(np.int64)
        ap[u] = _ap_at_k(pr, u_ind[ord_], k)
        ndcg[u] = _ndcg_at_k(pr, u_ind[ord_], u_x[ord_], k)
    return ap, ndcg


def to_r(pred0):
    """0-based with -1 -> 1-based with NA_integer_ (what rsparse_amd.metrics hands the library)"""
    pred0 = np.asarray(pred0, dtype=np.int64)
    return np.where(pred0 >= 0, pred0 + 1, NA).astype(np.int32)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_metrics_entry_points():
    lib = _lib.load()
    for name in ("rsparse_hip_ranking_metrics", "rsparse_hip_ranking_metrics_device"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.rsparse_hip_abi_version() == 6


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _slots():
    pred = np.asfortranarray(np.array([[3, 1], [NA, 2]], dtype=np.int32))   # 2 users x k = 2, column-major
    p = np.array([0, 2, 3], dtype=np.int32)
    j = np.array([0, 2, 1], dtype=np.int32)
    x = np.array([1.0, 2.0, 3.0])
    return pred, p, j, x


def _host(lib, pred, n, k, p, j, x, ap, nd):
    return lib.rsparse_hip_ranking_metrics(_vp(pred), n, k, _vp(p), _vp(j), _vp(x), _vp(ap), _vp(nd))


def _dev(lib, pred, n, k, p, j, x, ap, nd):
    # (host pointers: every call here is rejected by the argument checks, or is the n_users = 0 no-op, before device work)
    return lib.rsparse_hip_ranking_metrics_device(_vp(pred), n, k, _vp(p), _vp(j), _vp(x), _vp(ap), _vp(nd), None)


def test_status_codes_without_device():
    lib = _lib.load()
    pred, p, j, x = _slots()
    ap, nd = np.empty(2), np.empty(2)
    for call in (_host, _dev):
        assert call(lib, pred, 2, 2, p, j, x, None, None) == _lib.ERR_INVALID          # no output asked for
        assert call(lib, None, 2, 2, p, j, x, ap, nd) == _lib.ERR_INVALID
        assert call(lib, pred, 2, 2, None, j, x, ap, nd) == _lib.ERR_INVALID
        assert call(lib, pred, 2, 2, p, None, x, ap, nd) == _lib.ERR_INVALID
        assert call(lib, pred, 2, 2, p, j, None, None, nd) == _lib.ERR_INVALID          # ndcg needs the relevances
        assert call(lib, pred, -1, 2, p, j, x, ap, nd) == _lib.ERR_INVALID
        assert call(lib, pred, 2, 0, p, j, x, ap, nd) == _lib.ERR_INVALID
        assert call(lib, pred, 2, 8193, p, j, x, ap, nd) == _lib.ERR_UNSUPPORTED
        assert call(lib, pred, 0, 2, p, j, x, ap, nd) == _lib.OK                         # n_users = 0: a no-op
    # the host form checks the dgRMatrix slots
    assert _host(lib, pred, 2, 2, np.array([1, 2, 3], np.int32), j, x, ap, nd) == _lib.ERR_INVALID   # p[0] != 0
    assert _host(lib, pred, 2, 2, np.array([0, 2, 1], np.int32), j, x, ap, nd) == _lib.ERR_INVALID   # p decreases
    assert _host(lib, pred, 2, 2, p, np.array([2, 0, 1], np.int32), x, ap, nd) == _lib.ERR_INVALID   # j not ascending
    assert _host(lib, pred, 2, 2, p, np.array([1, 1, 1], np.int32), x, ap, nd) == _lib.ERR_INVALID   # ... strictly
    # x is read only for ndcg; a valid call gets past every argument check (no device here -> a runtime error)
    rc = _host(lib, pred, 2, 2, p, j, None, ap, None)
    assert rc not in (_lib.ERR_INVALID, _lib.ERR_UNSUPPORTED)
    rc = _host(lib, pred, 2, 2, p, j, x, ap, nd)
    assert rc not in (_lib.ERR_INVALID, _lib.ERR_UNSUPPORTED)


def test_python_metrics_reject_a_row_count_mismatch():
    from rsparse_amd import metrics
    import rsparse_amd
    assert rsparse_amd.metrics is metrics
    pred = np.array([[0, 1], [2, -1]])
    actual = sp.csr_matrix(np.eye(3))
    with pytest.raises(ValueError):
        metrics.ap_k(pred, actual)
    with pytest.raises(ValueError):
        metrics.ndcg_k(pred, actual)
    with pytest.raises(ValueError):
        metrics.ap_k(pred[0], actual[:2])          # not a matrix


def test_restatement_on_the_reference_cases():
    """tests/testthat/test-metrics.R:3-44 on the restatement itself (the GPU file runs them on the kernels)"""
    pred = to_r(np.array([[4, 6, 8, 1]]))
    a1 = sp.csr_matrix(np.array([[0, 0, 0, 0, 1, 0, 1, 0, 1, 0]], dtype=float))
    assert ref_metrics(pred, a1)[0][0] == 1.0
    a2 = a1.tolil(); a2[0, 9] = 1; a2 = a2.tocsr()
    a3 = a1.tolil(); a3[0, 0] = 1; a3 = a3.tocsr()
    assert ref_metrics(pred, a2)[0][0] == ref_metrics(pred, a3)[0][0] == 0.9375
    n1 = sp.csr_matrix(np.array([[0, 0, 0, 0, 10, 0, 8, 0, 4, 0]], dtype=float))
    assert ref_metrics(pred, n1)[1][0] == 1.0


# ---- WRMF.evaluate on two ranks ---------------------------------------------------------------------------------------------
def _oracle_metrics_backend():
    sys.path.insert(0, str(ROOT / "tests"))
    from oracle_backend import OracleBackend

    class MetricsOracleBackend(OracleBackend):
        def ranking_metrics(self, res, p, j, x, want_ap=True, want_ndcg=True):
            n = res.shape[0]
            act = sp.csr_matrix((x.numpy(), j.numpy(), p.numpy()), shape=(n, int(j.max()) + 1 if j.numel() else 1))
            ap, ndcg = ref_metrics(res.numpy(), act)
            return (torch.from_numpy(ap) if want_ap else None), (torch.from_numpy(ndcg) if want_ndcg else None)

    return MetricsOracleBackend()


def _eval_problem():
    rng = np.random.default_rng(17)
    n_user, n_item = 157, 53
    lens = np.clip(rng.lognormal(1.5, 1.0, n_user).astype(int), 0, 40)
    rows = np.repeat(np.arange(n_user), lens)
    cols = np.concatenate([rng.choice(n_item, size=l, replace=False) for l in lens])
    m = sp.csr_matrix((1.0 + rng.geometric(0.5, size=rows.size), (rows, cols)), shape=(n_user, n_item))
    held = sp.csr_matrix((rng.random((n_user, n_item)) < 0.1) * rng.integers(1, 5, (n_user, n_item)).astype(float))
    held.data[::7] = 0.0                                              # stored zeros are relevant items
    return m, held


def _eval_model():
    from rsparse_amd import WRMF
    m, held = _eval_problem()
    rng = np.random.default_rng(3)
    k = 6
    model = WRMF(rank=k, lambda_=0.1, feedback="implicit", solver="cholesky", precision="float",
                 backend=_oracle_metrics_backend(), rng=1)
    model._init_user_factors = (rng.standard_normal((m.shape[0], k)) * 0.01).astype(np.float32)
    model.components = (rng.standard_normal((k, m.shape[1])) * 0.01).astype(np.float32)
    model.fit_transform(m, n_iter=2, convergence_tol=-1)   # (one process: every rank holds the same model)
    return model, m, held


def _worker_eval(rank, ws, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    model, m, held = _eval_model()
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        res = {kk: model.evaluate(m, held, kk) for kk in (3, 10)}
        res["ap_only"] = model.evaluate(m, held, 5, metrics=("ap",))
        torch.save(res, os.path.join(out_dir, "m%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_sharded_evaluate_equals_one_process(tmp_path):
    import torch.multiprocessing as mp
    model, m, held = _eval_model()
    one = {kk: model.evaluate(m, held, kk) for kk in (3, 10)}
    one["ap_only"] = model.evaluate(m, held, 5, metrics=("ap",))
    # the one-process result is the restatement of predict's lists
    top = model.predict(m, 10)
    ap, ndcg = ref_metrics(to_r(top), held.tocsr())
    assert np.array_equal(one[10]["ap"], ap, equal_nan=True) and np.array_equal(one[10]["ndcg"], ndcg, equal_nan=True)
    assert set(one["ap_only"]) == {"ap"}
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker_eval, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        got = torch.load(tmp_path / ("m%d.pt" % r), weights_only=False)
        for key in one:
            assert set(got[key]) == set(one[key])
            for name in one[key]:
                assert got[key][name].dtype == np.float64 and got[key][name].shape == (m.shape[0],)
                assert np.array_equal(got[key][name], one[key][name], equal_nan=True), (r, key, name)
    with pytest.raises(ValueError):
        model.evaluate(m, held[:10], 3)
    with pytest.raises(ValueError):
        model.evaluate(m, held, 3, metrics=("map",))
