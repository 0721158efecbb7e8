"""Top-k within per-user candidate lists (`WRMF.predict(..., candidates=)` / `evaluate(..., candidates=)`) without a device: the
numpy fallback `WRMF._top_candidates_host` against the restatement of the reference's heap (oracle.wrmf_oracle.top_product) with
not_recommend = the given rows plus the complement of the candidates, on integer-valued factors (every sum exact, ties real,
everything compared with ==); the class through the CPU stand-in backend on MovieLens; the argument errors; and two gloo ranks
against one.  `evaluate` scores its lists with the device metrics kernels on every backend, and `metrics.ap_k` / `ndcg_k` run
there too: that one test is marked `gpu`."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import wrmf_oracle as O
from test_score_abi import out_rounding, score_bound

ROOT = Path(__file__).resolve().parent.parent
N_U, N_I, RANK = 40, 300, 4
NA = -2147483648
_cache = {}


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))


def _small_case():
    """40 x 300, factors in {-2 .. 2}.  Row 0: no candidate; row 1: every candidate in not_recommend; row 2: a zero user vector
    over 50 candidates (everything ties); row 3: exactly 17 admissible candidates; the others 1 .. 120 random candidates.  The
    exclusion list hits candidates of most rows."""
    if "small" not in _cache:
        rng = np.random.default_rng(42)
        U = rng.integers(-2, 3, size=(N_U, RANK)).astype(np.float32)
        V = rng.integers(-2, 3, size=(N_I, RANK)).astype(np.float32)
        U[2] = 0.0
        lens = rng.integers(1, 121, size=N_U)
        lens[0], lens[1], lens[2], lens[3] = 0, 30, 50, 17
        excl = np.array([5, 77, 150, 299], dtype=np.int64)
        rows_c, rows_nr = [], []
        for u in range(N_U):
            pool = np.setdiff1d(np.arange(N_I), excl) if u == 3 else np.arange(N_I)
            c = np.sort(rng.choice(pool, size=lens[u], replace=False))
            rows_c.append(c)
            if u == 1:
                nr = np.union1d(c, rng.choice(N_I, size=10, replace=False))      # covers the candidates
            elif u == 3:
                nr = np.setdiff1d(rng.choice(N_I, size=40, replace=False), c)     # misses them: 17 stay admissible
            else:
                nr = np.sort(rng.choice(N_I, size=rng.integers(0, 60), replace=False))
            rows_nr.append(np.sort(nr))
        mk = lambda rows: sp.csr_matrix((np.ones(sum(r.size for r in rows)), np.concatenate(rows).astype(np.int32),
                                         np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)), shape=(N_U, N_I))
        cand, nr = mk(rows_c), mk(rows_nr)
        assert np.any(np.isin(cand.indices, excl)) and cand[1].nnz == 30 and (cand[1].multiply(nr[1])).nnz == 30
        _cache["small"] = (U, V, cand, nr, excl)
    return _cache["small"]


def _union_with_complement(cand, nr):
    """not_recommend rows plus every item that is not a stored position of the row's candidates, as sorted CSR"""
    out = ~_pattern_mask(cand)
    if nr is not None:
        out |= _pattern_mask(nr)
    out = sp.csr_matrix(out.astype(np.float64))
    out.sort_indices()
    return out


def _pattern_mask(m):
    """the stored positions of a sparse matrix as a dense bool array (stored zeros included)"""
    m = sp.csr_matrix(m)
    out = np.zeros(m.shape, dtype=bool)
    out[np.repeat(np.arange(m.shape[0]), np.diff(m.indptr)), m.indices] = True
    return out


@pytest.mark.parametrize("glob_mean", [0.0, 0.5])
@pytest.mark.parametrize("k", [1, 5, 16, 17, 18, 60, 300])
def test_host_fallback_equals_the_reference_heap(k, glob_mean):
    from rsparse_amd import WRMF
    U, V, cand, nr, excl = _small_case()
    res, sc = WRMF._top_candidates_host(torch.from_numpy(U), torch.from_numpy(V), k, _i32(cand.indptr), _i32(cand.indices),
                                        _i32(nr.indptr), _i32(nr.indices), _i32(excl), glob_mean)
    res, sc = res.numpy(), sc.numpy()
    un = _union_with_complement(cand, nr)
    want_r, want_s = O.top_product(U.astype(np.float64), V.astype(np.float64).T, k, un.indptr, un.indices, (excl + 1).tolist(), glob_mean)
    assert res.dtype == np.int32 and sc.dtype == np.float64 and res.shape == (N_U, k)
    assert np.array_equal(res, want_r)
    assert np.array_equal(np.isnan(sc), want_r == NA) and np.all(sc[want_r != NA] == want_s[want_r != NA])
    adm = (_pattern_mask(cand) & ~_pattern_mask(nr))
    adm[:, excl] = False
    n_adm = adm.sum(axis=1)
    assert np.array_equal((res != NA).sum(axis=1), np.minimum(k, n_adm))
    assert n_adm[0] == 0 and n_adm[1] == 0 and n_adm[3] == 17
    if k < 50:   # the zero user: every admissible candidate ties, the heap keeps the first k in item order, largest first
        it = np.flatnonzero(adm[2])
        assert it.size > k and np.array_equal(res[2, :k] - 1, it[:k][::-1]) and np.all(sc[2, :k] == glob_mean)


def test_host_fallback_without_exclusions():
    from rsparse_amd import WRMF
    U, V, cand, _, _ = _small_case()
    res, sc = WRMF._top_candidates_host(torch.from_numpy(U), torch.from_numpy(V), 10, _i32(cand.indptr), _i32(cand.indices), None, None,
                                        None, 0.0)
    un = _union_with_complement(cand, None)
    want_r, want_s = O.top_product(U.astype(np.float64), V.astype(np.float64).T, 10, un.indptr, un.indices, (), 0.0)
    assert np.array_equal(res.numpy(), want_r) and np.all(sc.numpy()[want_r != NA] == want_s[want_r != NA])


# ---- the class through the CPU stand-in, on MovieLens -----------------------------------------------------------------------
N_EVAL = 120


def _ml_model(ml_train):
    if "ml" not in _cache:
        sys.path.insert(0, str(ROOT / "tests"))
        from oracle_backend import OracleBackend
        from rsparse_amd import WRMF
        n_user, n_item, p, i, x = ml_train
        train = sp.csc_matrix((x, i, p), shape=(n_user, n_item)).tocsr()
        model = WRMF(rank=8, lambda_=0.1, feedback="implicit", solver="cholesky", precision="float", backend=OracleBackend(), rng=1)
        model.fit_transform(train[:300], n_iter=2, convergence_tol=-1)
        seen = train[:N_EVAL].copy()
        rng = np.random.default_rng(7)
        cols = np.concatenate([np.sort(rng.choice(n_item, size=100, replace=False)) for _ in range(N_EVAL)])
        cand = sp.csr_matrix((np.zeros(cols.size), cols, np.arange(0, 100 * N_EVAL + 1, 100)), shape=(N_EVAL, n_item))
        _cache["ml"] = (model, seen, cand)
    return _cache["ml"]


def _check_scores(model, seen, top):
    emb = model.transform(seen).astype(np.float64)
    comp = np.asarray(model.components, dtype=np.float64)
    idx = np.asarray(top)
    rows, cols = np.nonzero(idx >= 0)
    it = idx[rows, cols]
    ref = np.einsum("tc,ct->t", emb[rows], comp[:, it]) + model.global_bias
    absdot = np.einsum("tc,ct->t", np.abs(emb[rows]), np.abs(comp[:, it]))
    tol = score_bound(absdot, ref, comp.shape[0]) + out_rounding(model, ref)
    assert np.all(np.abs(np.asarray(top.scores, dtype=np.float64)[rows, cols] - ref) <= tol)


def test_class_equals_predict_with_the_complement_on_movielens(ml_train):
    model, seen, cand = _ml_model(ml_train)
    # stored zeros are positions: the values of `cand` are all zero
    got = model.predict(seen, 10, candidates=cand)
    want = model.predict(seen, 10, not_recommend=_union_with_complement(cand, seen))
    assert np.array_equal(np.asarray(got), np.asarray(want)) and got.scores.dtype == want.scores.dtype
    assert (np.asarray(got) >= 0).sum() > 0.9 * got.size
    adm = _pattern_mask(cand) & ~_pattern_mask(seen)
    assert np.array_equal((np.asarray(got) >= 0).sum(axis=1), np.minimum(10, adm.sum(axis=1)))
    assert all(adm[u, i] for u in range(N_EVAL) for i in np.asarray(got)[u] if i >= 0)
    _check_scores(model, seen, got)
    # nothing else excluded, a global exclusion list, COO input with duplicates
    excl = [int(c) for c in cand.indices[:7]]
    coo = sp.vstack([cand, cand[:0]]).tocoo()
    coo = sp.coo_matrix((np.r_[coo.data, coo.data[:50]], (np.r_[coo.row, coo.row[:50]], np.r_[coo.col, coo.col[:50]])), shape=cand.shape)
    got2 = model.predict(seen, 25, not_recommend=None, items_exclude=excl, candidates=coo)
    want2 = model.predict(seen, 25, not_recommend=_union_with_complement(cand, None), items_exclude=excl)
    assert np.array_equal(np.asarray(got2), np.asarray(want2)) and (np.asarray(got2) >= 0).all()
    _check_scores(model, seen, got2)
    # candidates=None is the call as it was
    assert np.array_equal(np.asarray(model.predict(seen, 5, candidates=None)), np.asarray(model.predict(seen, 5)))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["float", "double"])
def test_evaluate_equals_the_metrics_of_the_lists(ml_train, precision):
    """(on the device: `evaluate` hands the lists to the metrics kernels, and metrics.ap_k / ndcg_k are those kernels too)"""
    from rsparse_amd import WRMF
    from rsparse_amd.metrics import ap_k, ndcg_k
    n_user, n_item, p, i, x = ml_train
    train = sp.csc_matrix((x, i, p), shape=(n_user, n_item)).tocsr()
    model = WRMF(rank=8, lambda_=0.1, feedback="implicit", solver="cholesky", precision=precision, rng=1)
    model.fit_transform(train[:300], n_iter=2, convergence_tol=-1)
    seen, held = train[:N_EVAL].copy(), train[:N_EVAL].copy()
    seen.data[1::2] = 0.0
    held.data[0::2] = 0.0
    seen.eliminate_zeros(); held.eliminate_zeros()
    rng = np.random.default_rng(9)
    neg = sp.csr_matrix((np.ones(99 * N_EVAL), rng.integers(0, n_item, size=99 * N_EVAL), np.arange(0, 99 * N_EVAL + 1, 99)),
                        shape=held.shape)
    cand = (held + neg).tocsr()          # the held-out items against 99 sampled negatives
    ev = model.evaluate(seen, held, 10, candidates=cand)
    top = model.predict(seen, 10, candidates=cand)
    assert np.array_equal(ev["ap"], ap_k(top, held), equal_nan=True) and np.array_equal(ev["ndcg"], ndcg_k(top, held), equal_nan=True)
    assert np.nanmean(ev["ndcg"]) > 0.3   # a fitted model ranks the held-out items above sampled negatives


def test_argument_errors(ml_train):
    from rsparse_amd import _lib
    model, seen, cand = _ml_model(ml_train)
    for fn in (lambda **kw: model.predict(seen, kw.pop("k", 10), **kw), lambda **kw: model.evaluate(seen, seen, kw.pop("k", 10), **kw)):
        with pytest.raises(ValueError):
            fn(candidates=cand[:10])                     # row count
        with pytest.raises(ValueError):
            fn(candidates=cand[:, :50])                  # column count
        with pytest.raises(TypeError):
            fn(candidates=cand.toarray())                # not sparse
        with pytest.raises(ValueError):
            fn(candidates=cand, k=0)
        with pytest.raises(_lib.UnsupportedOnDevice):
            fn(candidates=cand, k=8193)
        with pytest.raises(ValueError):
            fn(candidates=cand, items_exclude=[seen.shape[1]])
        with pytest.raises(ValueError):
            fn(candidates=cand, not_recommend=seen[:10])


# ---- two gloo ranks against one ---------------------------------------------------------------------------------------------
def _lists(model, seen, cand):
    top = model.predict(seen, 10, items_exclude=[3], candidates=cand)
    return {"idx": np.asarray(top).copy(), "scores": np.asarray(top.scores).copy()}


def _worker(rank, ws, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    sys.path.insert(0, str(ROOT / "tests"))
    from conftest import csc_take_rows, load_movielens
    n_user, n_item, p, i, x = load_movielens()
    model, seen, cand = _ml_model((900, n_item) + tuple(csc_take_rows(900, p, i, x)))
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        torch.save(_lists(model, seen, cand), os.path.join(out_dir, "w%d_%d.pt" % (ws, rank)))
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_give_the_one_process_result(ml_train, tmp_path):
    import torch.multiprocessing as mp
    model, seen, cand = _ml_model(ml_train)
    one = _lists(model, seen, cand)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        got = torch.load(tmp_path / ("w2_%d.pt" % r), weights_only=False)
        assert np.array_equal(got["idx"], one["idx"]) and np.array_equal(got["scores"], one["scores"], equal_nan=True)
