"""$predict / top_product for 256 < k <= 8192 (RSPARSE_HIP_MAX_TOPK_LARGE): the large-k device path (wrmf_topk_large.hip)
against the oracle's heap, the closed form of that heap's result the kernels rely on, and the ABI's limits."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import wrmf_oracle as O
from rsparse_amd import _lib


def _host_call(k, nr=2, nc=50, rank=4):
    lib = _lib.load()
    x = np.asfortranarray(np.ones((nr, rank)))
    y = np.asfortranarray(np.ones((rank, nc)))
    res = np.zeros((nr, k), dtype=np.int32, order="F")
    sc = np.zeros((nr, k), dtype=np.float64, order="F")
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.rsparse_hip_top_product(vp(x), vp(y), nr, nc, rank, k, 1, None, None, None, 0, 0.0, vp(res), vp(sc))
    return rc, lib.rsparse_hip_last_error().decode()


@pytest.mark.parametrize("k", [257, 1000, 8192])
def test_large_k_passes_the_argument_checks(k):
    rc, msg = _host_call(k)
    assert rc not in (_lib.ERR_UNSUPPORTED, _lib.ERR_INVALID), msg   # (no device here -> runtime error)


def test_k_above_the_large_limit_is_unsupported():
    rc, msg = _host_call(8193)
    assert rc == _lib.ERR_UNSUPPORTED and "8192" in msg


def _closed_form(x, y, k, nr_p=None, nr_j=None, exclude=(), glob_mean=0.0):
    """The reference heap's result without the heap (the rule wrmf_topk_large.hip implements): v_k the k-th best admissible
    score, A the items above it, G the admissible items at it; t = the G items among the first k of A u G in ascending item
    order; all of A and the k - |A| largest indices of t, best first, equal scores with the larger index first."""
    nrow, nc = x.shape[0], y.shape[1]
    res = np.full((nrow, k), O.NA_INTEGER, dtype=np.int32)
    scores = np.full((nrow, k), np.nan)
    excl = np.asarray(list(exclude), dtype=np.int64) - 1
    for j in range(nrow):
        s = x[j] @ y
        ok = np.ones(nc, dtype=bool)
        if nr_p is not None:
            ok[nr_j[nr_p[j]:nr_p[j + 1]]] = False
        ok[excl[(excl >= 0) & (excl < nc)]] = False
        adm = np.flatnonzero(ok)
        kk = min(k, adm.size)
        if kk == 0:
            continue
        vk = np.sort(s[adm])[::-1][kk - 1]
        A = adm[s[adm] > vk]
        AG = adm[s[adm] >= vk]                       # ascending item order
        t = np.intersect1d(AG[:kk], adm[s[adm] == vk])
        keep = np.concatenate([A, t[len(t) - (kk - len(A)):]])
        order = np.lexsort((-keep, -s[keep]))       # score descending, then index descending
        res[j, :kk] = keep[order] + 1
        scores[j, :kk] = s[keep[order]] + glob_mean
    return res, scores


@pytest.mark.parametrize("seed", range(6))
def test_closed_form_of_the_heap_matches_the_oracle(seed):
    rng = np.random.default_rng(seed)
    nrow, nc, rank = 40, 300, 3
    x = rng.integers(-1, 2, (nrow, rank)).astype(np.float64)
    y = rng.integers(-2, 3, (rank, nc)).astype(np.float64)     # few distinct scores: ties everywhere
    x[::7] = 0.0
    notrec = sp.random(nrow, nc, density=0.3, random_state=seed, format="csr")
    notrec.sort_indices()
    for k in (1, 5, 40, 150, 280, 400):
        for args in (dict(), dict(nr_p=notrec.indptr, nr_j=notrec.indices, exclude=[1, 9, nc], glob_mean=0.25)):
            ref_i, ref_s = O.top_product(x, y, k, **args)
            got_i, got_s = _closed_form(x, y, k, **args)
            assert np.array_equal(got_i, ref_i), (k, args.keys())
            assert np.allclose(got_s, ref_s, equal_nan=True)


# ---- on the device --------------------------------------------------------------------------------------------------------------
def _hip_top_product(x, y, k, nr=None, exclude=(), glob_mean=0.0):
    lib = _lib.load()
    nrow, rank = x.shape
    nc = y.shape[1]
    xf = np.asfortranarray(x, dtype=np.float64)
    yf = np.asfortranarray(y, dtype=np.float64)
    res = np.zeros((nrow, k), dtype=np.int32, order="F")
    sc = np.zeros((nrow, k), dtype=np.float64, order="F")
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    p = j = None
    if nr is not None:
        nr = sp.csr_matrix(nr)
        nr.sort_indices()
        p, j = nr.indptr.astype(np.int32), nr.indices.astype(np.int32)
    ex = np.asarray(list(exclude), dtype=np.int32)
    _lib.check(lib.rsparse_hip_top_product(vp(xf), vp(yf), nrow, nc, rank, k, 1, vp(p), vp(j), vp(ex) if ex.size else None,
                                           int(ex.size), float(glob_mean), vp(res), vp(sc)))
    return res, sc


def _hip_top_product_f32(x, y, k, nr=None, exclude=(), glob_mean=0.0):
    """rsparse_hip_top_product_device: fp32 factors on the device, fp32 scores, no re-scoring"""
    import torch
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    U = torch.tensor(np.ascontiguousarray(x, dtype=np.float32), device=dev)
    V = torch.tensor(np.ascontiguousarray(y.T, dtype=np.float32), device=dev)
    n, rank = U.shape
    res = torch.empty((n, k), dtype=torch.int32, device=dev)
    sc = torch.empty((n, k), dtype=torch.float32, device=dev)
    p = j = None
    if nr is not None:
        nr = sp.csr_matrix(nr)
        nr.sort_indices()
        p = torch.tensor(nr.indptr.astype(np.int32), device=dev)
        j = torch.tensor(nr.indices.astype(np.int32), device=dev)
    ex0 = np.unique(np.asarray(list(exclude), dtype=np.int64) - 1)
    ex0 = ex0[(ex0 >= 0) & (ex0 < V.shape[0])]
    e = torch.tensor(ex0.astype(np.int32), device=dev) if ex0.size else None
    _lib.check(lib.rsparse_hip_top_product_device(U.data_ptr(), V.data_ptr(), n, V.shape[0], rank, k,
                                                  None if p is None else p.data_ptr(), None if j is None else j.data_ptr(),
                                                  None if e is None else e.data_ptr(), int(ex0.size), float(glob_mean),
                                                  res.data_ptr(), sc.data_ptr(), None))
    torch.cuda.synchronize()
    return res.cpu().numpy(), sc.cpu().numpy().astype(np.float64)


def _variants(nrow, nc, seed):
    notrec = sp.random(nrow, nc, density=0.05, random_state=seed, format="csr")
    notrec.sort_indices()
    return notrec, (dict(), dict(nr=notrec), dict(nr=notrec, exclude=[1, 7, nc], glob_mean=0.5))


def _oracle(x, y, k, notrec, args):
    nr = args.get("nr")
    return O.top_product(x, y, k, *(None, None) if nr is None else (notrec.indptr, notrec.indices),
                         exclude=args.get("exclude", ()), glob_mean=args.get("glob_mean", 0.0))


def _assert_f32_matches(got_i, got_s, ref_i1, ref_s1):
    """ref_*1: the oracle's top k + 1 -- the last place is fp32 noise too when the (k+1)-th score is within it"""
    k = got_i.shape[1]
    assert np.allclose(got_s, ref_s1[:, :k], rtol=1e-4, atol=1e-5, equal_nan=True)
    # indices agree wherever the neighbouring scores are separated by more than fp32 noise
    gap_ok = np.ones_like(ref_i1, dtype=bool)
    d = np.abs(np.diff(ref_s1, axis=1))
    tol = 1e-4 * np.maximum(1.0, np.abs(ref_s1[:, :-1]))
    gap_ok[:, :-1] &= ~(d <= tol)
    gap_ok[:, 1:] &= ~(d <= tol)
    gap_ok = gap_ok[:, :k]
    assert np.array_equal(got_i[gap_ok], ref_i1[:, :k][gap_ok])


CASES = [(10, 3, 2000, 257), (30, 129, 3000, 300), (64, 1, 70000, 512), (128, 3, 20000, 1000), (200, 1, 9000, 2048),
         (256, 3, 5000, 4096), (128, 1, 12000, 8192), (64, 129, 600, 1000), (30, 1000, 400, 300), (10, 1000, 1500, 257),
         (128, 129, 2500, 2048)]


@pytest.mark.gpu
@pytest.mark.parametrize("rank,nr,nc,k", CASES)
def test_large_k_double_form_matches_the_oracle(rank, nr, nc, k):
    rng = np.random.default_rng(rank + nr + k)
    x = rng.standard_normal((nr, rank)).astype(np.float32).astype(np.float64)
    y = rng.standard_normal((rank, nc)).astype(np.float32).astype(np.float64)
    notrec, variants = _variants(nr, nc, 3)
    for args in variants:
        ref_i, ref_s = _oracle(x, y, k, notrec, args)
        got_i, got_s = _hip_top_product(x, y, k, **args)
        assert np.array_equal(got_i, ref_i), sorted(args)
        assert np.allclose(got_s, ref_s, rtol=1e-12, atol=1e-12, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("rank,nr,nc,k", CASES)
def test_large_k_fp32_form_matches_the_oracle(rank, nr, nc, k):
    rng = np.random.default_rng(rank + nr + k)
    x = rng.standard_normal((nr, rank)).astype(np.float32).astype(np.float64)
    y = rng.standard_normal((rank, nc)).astype(np.float32).astype(np.float64)
    notrec, variants = _variants(nr, nc, 3)
    for args in variants:
        ref_i1, ref_s1 = _oracle(x, y, k + 1, notrec, args)
        got_i, got_s = _hip_top_product_f32(x, y, k, **args)
        _assert_f32_matches(got_i, got_s, ref_i1, ref_s1)


@pytest.mark.gpu
def test_large_k_zero_users_tie_every_item():
    """Users with an empty row of x get a zero embedding: every item ties, the candidate list overflows and the heap is replayed."""
    rng = np.random.default_rng(5)
    rank, nr, nc, k = 30, 6, 20000, 300
    x = rng.standard_normal((nr, rank))
    x[[0, 3, 5]] = 0.0
    y = rng.standard_normal((rank, nc))
    notrec, variants = _variants(nr, nc, 4)
    for args in variants:
        ref_i, ref_s = _oracle(x, y, k, notrec, args)
        got_i, got_s = _hip_top_product(x, y, k, **args)
        assert np.array_equal(got_i, ref_i), sorted(args)
        assert np.allclose(got_s, ref_s, rtol=1e-12, atol=1e-12, equal_nan=True)
        got_i, got_s = _hip_top_product_f32(x, y, k, **args)
        assert np.array_equal(got_i[[0, 3, 5]], ref_i[[0, 3, 5]])     # exact ties: the heap's order, in fp32 too
        _assert_f32_matches(got_i, got_s, *_oracle(x, y, k + 1, notrec, args))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [300, 1000])
def test_large_k_duplicated_items(k):
    rng = np.random.default_rng(k)
    rank, nr, nc = 16, 20, 3000
    base = rng.standard_normal((rank, 300))
    y = base[:, rng.integers(0, 300, nc)]               # every vector ~10 times
    x = rng.standard_normal((nr, rank))
    notrec, variants = _variants(nr, nc, 5)
    for args in variants:
        ref_i, ref_s = _oracle(x, y, k, notrec, args)
        got_i, got_s = _hip_top_product(x, y, k, **args)
        assert np.array_equal(got_i, ref_i), sorted(args)
        got_i, got_s = _hip_top_product_f32(x, y, k, **args)
        assert np.array_equal(got_i, ref_i), sorted(args)              # equal vectors: equal fp32 scores as well


@pytest.mark.gpu
def test_large_k_near_ties_resolve_in_double():
    rng = np.random.default_rng(3)
    rank, nc, k = 64, 2000, 600
    y = rng.standard_normal((rank, nc))
    for j in range(0, nc, 2):
        y[:, j + 1] = y[:, j] * (1.0 + (1e-9 if (j // 2) % 2 else -1e-9))
    x = rng.standard_normal((30, rank))
    ref_i, ref_s = O.top_product(x, y, k)
    got_i, got_s = _hip_top_product(x, y, k)
    assert np.array_equal(got_i, ref_i)
    assert np.allclose(got_s, ref_s, rtol=1e-13, atol=0)
    f32 = (x.astype(np.float32) @ y.astype(np.float32))
    assert (f32[:, 0::2] == f32[:, 1::2]).mean() > 0.5


@pytest.mark.gpu
def test_large_k_exclusions_leave_fewer_than_k():
    rng = np.random.default_rng(8)
    rank, nr, nc, k = 32, 40, 1000, 800
    x = rng.standard_normal((nr, rank))
    y = rng.standard_normal((rank, nc))
    notrec = sp.random(nr, nc, density=0.3, random_state=2, format="csr")
    notrec.sort_indices()
    excl = list(range(1, 60))
    ref_i, ref_s = O.top_product(x, y, k, notrec.indptr, notrec.indices, exclude=excl, glob_mean=-1.0)
    assert (ref_i == O.NA_INTEGER).any()
    got_i, got_s = _hip_top_product(x, y, k, nr=notrec, exclude=excl, glob_mean=-1.0)
    assert np.array_equal(got_i, ref_i)
    assert np.allclose(got_s, ref_s, rtol=1e-12, atol=1e-12, equal_nan=True)
    got_i, got_s = _hip_top_product_f32(x, y, k, nr=notrec, exclude=excl, glob_mean=-1.0)
    assert np.array_equal(got_i == O.NA_INTEGER, ref_i == O.NA_INTEGER)
    _assert_f32_matches(got_i, got_s, *O.top_product(x, y, k + 1, notrec.indptr, notrec.indices, exclude=excl, glob_mean=-1.0))


@pytest.mark.gpu
def test_large_k_more_users_than_one_chunk():
    """1M items: a chunk is ~512 users (2 GiB of keys); 600 users run in two chunks.  First and last rows against the oracle."""
    rng = np.random.default_rng(11)
    rank, nr, nc, k = 10, 600, 1_000_000, 300
    x = rng.standard_normal((nr, rank))
    y = rng.standard_normal((rank, nc))
    x[nr - 2] = 0.0                                   # a zero user in the second chunk
    got_i, got_s = _hip_top_product(x, y, k)
    rows = [0, 1, 2, nr - 3, nr - 2, nr - 1]
    ref_i, ref_s = O.top_product(x[rows], y, k)
    assert np.array_equal(got_i[rows], ref_i)
    assert np.allclose(got_s[rows], ref_s, rtol=1e-12, atol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [500, 2000])
def test_wrmf_predict_large_k_orders_like_the_reference_on_movielens(movielens, ml_train, k):
    """k = 2000 is above the 1682 items: the rest of every row is NA."""
    from rsparse_amd import WRMF
    n_user, n_item, tp, ti, tx = ml_train
    train = sp.csc_matrix((tx, ti, tp), shape=(n_user, n_item)).tocsr()
    for precision in ("double", "float"):
        m = WRMF(rank=10, lambda_=0.1, feedback="implicit", solver="conjugate_gradient", precision=precision, rng=1)
        emb = m.fit_transform(train, n_iter=3, convergence_tol=-1)
        preds = m.predict(train, k)
        nr = train.copy(); nr.sort_indices()
        ref_i, ref_s = O.top_product(np.asarray(emb, dtype=np.float64), np.asarray(m.components, dtype=np.float64), k,
                                     nr.indptr, nr.indices)
        ref0 = np.where(ref_i == O.NA_INTEGER, -1, ref_i - 1)
        assert np.array_equal(np.asarray(preds), ref0), precision
        assert np.allclose(np.nan_to_num(preds.scores), np.nan_to_num(ref_s), rtol=1e-12 if precision == "double" else 1e-6)
