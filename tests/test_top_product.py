"""$predict / top_product: the reference's own value-level test (tests/testthat/test-top-product.R:3-14:
top-k of one row equals order(decreasing)[1:k]) for the oracle on CPU, and GPU parity of the HIP kernel
against the oracle including exclusions, ties and NA fill."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import wrmf_oracle as O
from rsparse_amd import _lib


def test_oracle_matches_order_decreasing():
    rng = np.random.default_rng(1)
    nr, k, nc = 100, 10, 50                       # test-top-product.R:4-6
    m1 = rng.random((nr, k))
    m2 = rng.random((k, nc))
    m3 = m1 @ m2
    res, scores = O.top_product(m1, m2, k)
    for row in (0, 17, 99):
        expect = np.argsort(-m3[row], kind="stable")[:k] + 1
        assert np.array_equal(res[row], expect)
        assert np.allclose(scores[row], m3[row][expect - 1])


def test_oracle_exclusions_ties_and_na():
    x = np.zeros((2, 3))
    x[1] = [1.0, 0.0, 0.0]
    y = np.arange(18, dtype=np.float64).reshape(3, 6)
    # row 0: all scores 0 -> the heap keeps the first k admissible items, output has the larger index first
    res, sc = O.top_product(x, y, 3)
    assert list(res[0]) == [3, 2, 1] and np.all(sc[0] == 0)
    assert list(res[1]) == [6, 5, 4]
    nr = sp.csr_matrix(np.array([[0, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1]]))
    res, sc = O.top_product(x, y, 3, nr.indptr, nr.indices, exclude=[5])
    assert list(res[0]) == [4, 3, 1] and list(res[1]) == [4, 3, 2]
    res, sc = O.top_product(x, y, 5, exclude=[1, 2, 3])
    assert list(res[0][:3]) == [6, 5, 4] and np.all(res[0][3:] == O.NA_INTEGER) and np.isnan(sc[0][3:]).all()


def test_oracle_tie_eviction_order():
    """src/matrix_top_product.cpp:61-86: a min-heap on (score, index) pairs; a newcomer replaces the top only if its score
    is strictly larger, and the top among tied minima is the smallest index."""
    one = np.ones((1, 1))
    res, _ = O.top_product(one, np.array([[1.0, 1.0, 5.0]]), 2)
    assert list(res[0]) == [3, 2]          # (1, item 0) is evicted by the 5, (1, item 1) stays
    res, _ = O.top_product(one, np.array([[1.0, 5.0, 1.0]]), 2)
    assert list(res[0]) == [2, 1]          # the heap is full with minimum 1 when the second 1 arrives: not admitted


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


def _plan(nr, nc, rank, k, rescore=1, extra=-1):
    """the launches of a call of this shape (rsparse_hip_top_product_plan; rescore = 1, extra = -1: the host form above), one dict
    of strings per launch"""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    _lib.check(lib.rsparse_hip_top_product_plan(nr, nc, rank, k, extra, rescore, buf, len(buf)))
    return [dict(kv.split("=") for kv in line.split()) for line in buf.value.decode().splitlines()]


def _full_geometries(nr, nc, rank, k):
    """"family KP UB W buffers" of every launch of the host form that is not a re-run for flagged users"""
    return {" ".join(l[f] for f in ("family", "KP", "UB", "W", "buffers")) for l in _plan(nr, nc, rank, k) if l["flagged"] == "0"}


def test_plan_entry_describes_the_launches():
    """No device call: the plan is host arithmetic.  The host form of (128, 700, 20000, 100) nominates kc = 125 per user over
    19 item slices on the tile-per-wave kernel, re-runs flagged users of the merge unsliced, and re-runs the users the re-scoring
    flags at k = 100 on the one-tile shared kernel; the device form of more than 131072 users goes in chunks."""
    p = _plan(700, 20000, 128, 100)
    assert [(l["family"], l["k"], l["grid"], l["flagged"]) for l in p] == [("per_wave", "125", "22x19", "0"),
                                                                           ("per_wave", "125", "22x1", "1"),
                                                                           ("shared", "100", "6x1", "1")]
    assert p[0]["scratch_floats"] == str(2 * 19 * 700 * 125 + 700 + 16) and p[0]["slice_items"] == str(32 * 33)
    p = _plan(131072 + 200, 4200, 32, 60, rescore=0)
    assert [(l["user0"], l["n_users"], l["buffers"], l["grid"]) for l in p] == [("0", "131072", "global", "512x1"),
                                                                                ("131072", "200", "global", "1x1")]
    assert p[0]["scratch_floats"] == str(512 * 2 * 256 * 156 + 16) and p[0]["lds"] == str((2 * 32 * 36 + 3 * 256) * 4 + 64 + 4 * 156 * 16)
    lib = _lib.load()
    buf = ctypes.create_string_buffer(8)
    assert lib.rsparse_hip_top_product_plan(10, 10, 8, 300, -1, 1, buf, 8) == _lib.ERR_UNSUPPORTED     # (the large-k path)
    assert lib.rsparse_hip_top_product_plan(10, 10, 8, 3, -1, 1, buf, 8) == _lib.ERR_INVALID           # (buffer too small)


@pytest.mark.gpu
@pytest.mark.parametrize("rank,nr,nc,k", [(10, 100, 50, 10), (16, 70, 3001, 25), (64, 33, 777, 7), (128, 129, 5000, 100),
                                          (20, 5, 40, 12),
                                          # what these reach (the plan entry; kc = k + max(8, k / 4) candidates are nominated, the
                                          # re-run at k is flagged): (128, 300, 5000, 10) the two-tile kernel with 256 users per
                                          # workgroup over 4 item slices; (128, 100, 3000, 100) and (128, 40, 1000, 120) a tile per
                                          # wave with 32 users; (128, 70, 4000, 200) and (128, 33, 2000, 256) the same on two waves;
                                          # (64, 300, 2000, 256) and (30, 140, 900, 5) the candidate buffers in global memory, the
                                          # latter with scalar staging (rank % 4 != 0).  Every geometry: test_hip_every_geometry
                                          (128, 300, 5000, 10), (128, 100, 3000, 100), (128, 70, 4000, 200),
                                          (64, 300, 2000, 256), (128, 33, 2000, 256), (30, 140, 900, 5), (128, 40, 1000, 120),
                                          # few users over many items: the items are split over the workgroups and the slices'
                                          # lists merged (one user over 70000 items: 63 slices; 1000 users over 9000: 8)
                                          (128, 1, 70000, 10), (64, 3, 20000, 100), (128, 1000, 9000, 10), (16, 37, 5000, 256)])
def test_hip_matches_oracle(rank, nr, nc, k):
    rng = np.random.default_rng(rank + nr)
    x = rng.standard_normal((nr, rank)).astype(np.float32).astype(np.float64)
    y = rng.standard_normal((rank, nc)).astype(np.float32).astype(np.float64)
    notrec = sp.random(nr, nc, density=0.05, random_state=3, format="csr")
    excl = [1, 7, nc]                                     # 1-based like R
    for args in (dict(), dict(nr=notrec), dict(nr=notrec, exclude=excl, glob_mean=0.5)):
        ref_i, ref_s = O.top_product(x, y, k, *(None, None) if "nr" not in args else (notrec.indptr, notrec.indices),
                                     exclude=args.get("exclude", ()), glob_mean=args.get("glob_mean", 0.0))
        got_i, got_s = _hip_top_product(x, y, k, **args)
        assert np.allclose(got_s, ref_s, rtol=1e-4, atol=1e-5, equal_nan=True)
        # indices agree wherever the neighbouring scores are separated by more than fp32 noise
        gap_ok = np.ones_like(ref_i, dtype=bool)
        d = np.abs(np.diff(ref_s, axis=1))
        tol = 1e-4 * np.maximum(1.0, np.abs(ref_s[:, :-1]))
        gap_ok[:, :-1] &= d > tol
        gap_ok[:, 1:] &= d > tol
        assert np.array_equal(got_i[gap_ok], ref_i[gap_ok])


@pytest.mark.gpu
def test_hip_ties_and_na_fill():
    x = np.zeros((3, 4))
    x[1] = [1.0, 0, 0, 0]
    y = np.arange(40, dtype=np.float64).reshape(4, 10)
    ref_i, ref_s = O.top_product(x, y, 4)
    got_i, got_s = _hip_top_product(x, y, 4)
    assert np.array_equal(got_i, ref_i) and np.array_equal(got_s, ref_s)       # all-zero rows: ties everywhere
    ref_i, ref_s = O.top_product(x, y, 6, exclude=[1, 2, 3, 4, 5, 6, 7])
    got_i, got_s = _hip_top_product(x, y, 6, exclude=[1, 2, 3, 4, 5, 6, 7])
    assert np.array_equal(got_i, ref_i) and np.array_equal(np.isnan(got_s), np.isnan(ref_s))
    assert (got_i[:, 3:] == O.NA_INTEGER).all()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 7, 40, 88])
def test_hip_tied_scores_follow_the_heap(k):
    """Integer-valued factors: every user has many items tied at its k-th score, interleaved with larger scores; which of
    them survive depends on the arrival order exactly as in the reference's heap (the device replays the arrivals of a
    round through the heap when, and only when, there are more candidates at the k-th score than places).  k = 88 at 70 users
    (110 candidates) is the one-tile shared kernel: its settle and replay code with ties."""
    one = np.ones((1, 1))
    for sc, kk in (([1.0, 1.0, 5.0], 2), ([1.0, 5.0, 1.0], 2)):
        ref_i, ref_s = O.top_product(one, np.array([sc]), kk)
        got_i, got_s = _hip_top_product(one, np.array([sc]), kk)
        assert np.array_equal(got_i, ref_i) and np.array_equal(got_s, ref_s)
    rng = np.random.default_rng(100 + k)
    if k == 88:
        assert _full_geometries(70, 1500, 4, k) == {"shared 32 1 4 lds"}
    for n_users in (70, 300, 40):      # (the tile-sharing kernels with 128 users per workgroup, the global buffers, a tile per wave)
        x = rng.integers(0, 3, (n_users, 4)).astype(np.float64)
        y = rng.integers(0, 3, (4, 1500)).astype(np.float64)          # scores are small integers: ties everywhere
        nr = sp.random(n_users, 1500, density=0.02, format="csr", random_state=np.random.RandomState(k))
        nr.sort_indices()
        for kw in ({}, {"nr": nr, "exclude": [3, 77, 1400]}):
            ref_i, ref_s = O.top_product(x, y, k, *((kw["nr"].indptr, kw["nr"].indices) if kw else (None, None)),
                                         exclude=kw.get("exclude", ()))
            got_i, got_s = _hip_top_product(x, y, k, **kw)
            assert np.array_equal(got_i, ref_i) and np.array_equal(got_s, ref_s)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 40])
def test_hip_split_items_with_ties_falls_back_to_the_heap(k):
    """The split launch (few users, many items) merges per-slice lists; membership at the k-th score is ambiguous when more
    candidates sit there than places -- then the user is recomputed by the unsplit kernel, which follows the reference's heap.
    Integer-valued factors over 6000 items (ties everywhere), with and without exclusion lists; plus k larger than the number of
    admissible items (NA fill through the merge)."""
    rng = np.random.default_rng(7 + k)
    for n_users in (1, 9, 70):
        x = rng.integers(0, 3, (n_users, 4)).astype(np.float64)
        y = rng.integers(0, 3, (4, 6000)).astype(np.float64)
        nr = sp.random(n_users, 6000, density=0.01, format="csr", random_state=np.random.RandomState(k))
        nr.sort_indices()
        for kw in ({}, {"nr": nr, "exclude": [3, 77, 5999]}):
            ref_i, ref_s = O.top_product(x, y, k, *((kw["nr"].indptr, kw["nr"].indices) if kw else (None, None)),
                                         exclude=kw.get("exclude", ()))
            got_i, got_s = _hip_top_product(x, y, k, **kw)
            assert np.array_equal(got_i, ref_i) and np.array_equal(got_s, ref_s)
    # almost everything excluded: fewer admissible items than k
    x = rng.standard_normal((2, 8))
    y = rng.standard_normal((8, 5000))
    excl = list(range(1, 5001 - 2))                      # 1-based: all but the last two items
    ref_i, ref_s = O.top_product(x, y, k, exclude=excl)
    got_i, got_s = _hip_top_product(x, y, k, exclude=excl)
    assert np.array_equal(got_i, ref_i) and np.array_equal(np.isnan(got_s), np.isnan(ref_s))
    assert (got_i[:, 2:] == O.NA_INTEGER).all()


@pytest.mark.gpu
@pytest.mark.parametrize("rank,nr,nc,k", [(128, 300, 6000, 10), (128, 130, 6000, 100), (64, 77, 3000, 10), (10, 500, 1682, 100),
                                          (36, 3, 30000, 10), (128, 40, 2500, 250)])
def test_hip_orders_like_the_double_product(rank, nr, nc, k):
    """find_top_product multiplies in double (R/utils.R:35-36): the device's candidates come from an fp32 pass, but scores and
    ORDER are those of the double product -- indices equal to the oracle's everywhere, not only where fp32 separates the scores."""
    rng = np.random.default_rng(7 * rank + k)
    x = rng.standard_normal((nr, rank))
    y = rng.standard_normal((rank, nc))
    notrec = sp.random(nr, nc, density=0.03, random_state=5, format="csr")
    for args in (dict(), dict(nr=notrec, exclude=[2, 9, nc], glob_mean=3.5)):
        ref_i, ref_s = O.top_product(x, y, k, *(None, None) if "nr" not in args else (notrec.indptr, notrec.indices),
                                     exclude=args.get("exclude", ()), glob_mean=args.get("glob_mean", 0.0))
        got_i, got_s = _hip_top_product(x, y, k, **args)
        assert np.array_equal(got_i, ref_i)
        assert np.allclose(got_s, ref_s, rtol=1e-12, atol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("rank,nr,nc,k", [(128, 700, 20000, 100), (64, 520, 9000, 60), (32, 300, 7000, 200), (128, 700, 4000, 100)])
def test_hip_large_k_many_users_candidates_in_global_memory(rank, nr, nc, k):
    """Many users at a large k.  An unsliced call for more than 128 users -- (128, 700, 4000, 100): fewer than 4096 items -- keeps
    the candidate buffers in a global scratch and settles a user once per batch of arrivals (wrmf_topk.hip GBUF): three workgroups,
    the last one partly filled, 125 tiles, exclusion lists.  The three larger shapes are split over the items since slicing came
    (19 / 8 / 6 slices) and run the LDS geometries a sliced call takes: a tile per wave, the two-tile kernel with 128 users, a tile
    per wave.  Indices equal to the oracle's."""
    assert ("pipe %d 2 4 global" % rank in _full_geometries(nr, nc, rank, k)) == (nc < 4096)
    rng = np.random.default_rng(11 * rank + k)
    x = rng.standard_normal((nr, rank))
    y = rng.standard_normal((rank, nc))
    notrec = sp.random(nr, nc, density=0.01, random_state=9, format="csr")
    for args in (dict(), dict(nr=notrec, exclude=[5, 6, nc - 1], glob_mean=-1.25)):
        ref_i, ref_s = O.top_product(x, y, k, *(None, None) if "nr" not in args else (notrec.indptr, notrec.indices),
                                     exclude=args.get("exclude", ()), glob_mean=args.get("glob_mean", 0.0))
        got_i, got_s = _hip_top_product(x, y, k, **args)
        assert np.array_equal(got_i, ref_i)
        assert np.allclose(got_s, ref_s, rtol=1e-12, atol=1e-12)


# (rank, users, items, k) -> the geometry of the nominating pass, "family KP UB W buffers".  Every instantiation the plan's table can
# select, with 16-byte staging (ranks 32 / 64 / 128 / 160) and with scalar staging (30 / 62 / 126 / 158), at the smallest shape at
# which it exists: one workgroup (two at rank > 128) with a partly filled last user block, 47 item tiles, or 129 tiles in 4 slices.
def _geometry_cases():
    cases = []
    for r in (32, 30, 64, 62, 128, 126, 160, 158):
        kp = 32 if r <= 32 else 64 if r <= 64 else 128 if r <= 128 else 256
        if kp <= 128:
            cases += [(r, 130, 1500, 1, "pipe %d 2 4 global" % kp), (r, 130, 4100, 1, "pipe %d 2 4 lds" % kp),
                      (r, 40, 1500, 1, "per_wave %d 2 4 lds" % kp), (r, 20, 1500, 1, "per_wave %d 1 4 lds" % kp)]
        cases += [(r, 70, 1500, 1, "pipe %d 1 4 lds" % kp), (r, 70, 1500, {32: 88, 64: 81, 128: 68, 256: 43}[kp], "shared %d 1 4 lds" % kp)]
        if kp >= 128:
            cases += [(r, 20, 1500, 152 if kp == 128 else 1, "per_wave %d 1 2 lds" % kp)]
    # k at the upper edge of a band: the largest candidate buffers that fit the LDS next to the tiles (or, global, the longest)
    cases += [(128, 130, 4100, 16, "pipe 128 2 4 lds"), (128, 70, 1500, 67, "pipe 128 1 4 lds"), (128, 70, 1500, 80, "shared 128 1 4 lds"),
              (128, 40, 1500, 28, "per_wave 128 2 4 lds"), (128, 20, 1500, 151, "per_wave 128 1 4 lds"),
              (160, 70, 1500, 42, "pipe 256 1 4 lds"), (160, 70, 1500, 67, "shared 256 1 4 lds"),
              (128, 130, 1500, 256, "pipe 128 2 4 global"), (160, 20, 1500, 205, "per_wave 256 1 2 lds")]
    return cases


def test_geometry_cases_cover_every_instantiation():
    """44 product kernels: per rank class up to 128 the two-tile kernel with 2 (global / LDS) and 1 user blocks per wave, the shared
    kernel, a tile per wave with 2 and 1 blocks; two waves at 128 and 256; at 256 one block per wave only; each with and without
    16-byte staging."""
    assert len({(geo, r % 4 == 0) for r, _, _, _, geo in _geometry_cases()}) == 44


@pytest.mark.gpu
@pytest.mark.parametrize("rank,nr,nc,k,geometry", _geometry_cases())
def test_hip_every_geometry(rank, nr, nc, k, geometry):
    """Every kernel the plan can select runs a full (unflagged) launch -- asserted through the plan entry -- and orders like the
    double product: indices equal to the oracle's everywhere, without and with a not_recommend matrix, exclusions and a global
    mean."""
    assert _full_geometries(nr, nc, rank, k) == {geometry}
    rng = np.random.default_rng(7 * rank + k + nr)
    x = rng.standard_normal((nr, rank))
    y = rng.standard_normal((rank, nc))
    notrec = sp.random(nr, nc, density=0.03, random_state=5, format="csr")
    for args in (dict(), dict(nr=notrec, exclude=[2, 9, nc], glob_mean=3.5)):
        ref_i, ref_s = O.top_product(x, y, k, *(None, None) if "nr" not in args else (notrec.indptr, notrec.indices),
                                     exclude=args.get("exclude", ()), glob_mean=args.get("glob_mean", 0.0))
        got_i, got_s = _hip_top_product(x, y, k, **args)
        assert np.array_equal(got_i, ref_i)
        assert np.allclose(got_s, ref_s, rtol=1e-12, atol=1e-12)


@pytest.mark.gpu
def test_hip_large_k_user_chunks_share_the_scratch():
    """More users than one launch of the global-buffer geometry takes (131072): the chunks run one after the other on the stream and
    reuse the scratch slots; the first and the last users (the second chunk's) against the oracle."""
    rng = np.random.default_rng(5)
    rank, nc, k, nr = 32, 4200, 60, 131072 + 200
    x = rng.standard_normal((nr, rank))
    y = rng.standard_normal((rank, nc))
    got_i, got_s = _hip_top_product(x, y, k, exclude=[10, 11])
    for rows in (slice(0, 64), slice(131072 - 32, 131072 + 200)):
        ref_i, ref_s = O.top_product(x[rows], y, k, exclude=[10, 11])
        assert np.array_equal(got_i[rows], ref_i)
        assert np.allclose(got_s[rows], ref_s, rtol=1e-12, atol=1e-12)


@pytest.mark.gpu
def test_hip_near_ties_resolve_in_double():
    """Pairs of items whose vectors differ by 1e-9 relative: equal scores in fp32 (where the larger index would come first),
    ordered by the double product in the reference."""
    rng = np.random.default_rng(3)
    rank, nc, k = 64, 400, 20
    y = rng.standard_normal((rank, nc))
    for j in range(0, nc, 2):                      # item j + 1 = item j, a hair smaller or larger
        y[:, j + 1] = y[:, j] * (1.0 + (1e-9 if (j // 2) % 2 else -1e-9))
    x = rng.standard_normal((60, rank))
    ref_i, ref_s = O.top_product(x, y, k)
    got_i, got_s = _hip_top_product(x, y, k)
    assert np.array_equal(got_i, ref_i)
    assert np.allclose(got_s, ref_s, rtol=1e-13, atol=0)
    f32 = (x.astype(np.float32) @ y.astype(np.float32))
    assert (f32[:, 0::2] == f32[:, 1::2]).mean() > 0.5          # the case under test: fp32 does not separate the pairs


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 100])
def test_wrmf_predict_orders_like_the_reference_on_movielens(movielens, ml_train, k):
    """every movielens user, k = 10 and 100, precision = "double" -- the indices `predict` returns equal
    the oracle's top_product of the model's own double factors."""
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
        assert np.allclose(preds.scores, np.nan_to_num(ref_s), rtol=1e-12 if precision == "double" else 1e-6)


@pytest.mark.gpu
def test_wrmf_predict(movielens, ml_train):
    """test-wrmf.R:59-61: predict(cv, k = K) has nrow(cv) rows and K columns; never recommends seen items."""
    from conftest import csc_drop_rows
    from rsparse_amd import WRMF
    n_user_all, n_item, p, i, x = movielens
    n_user, _, tp, ti, tx = ml_train
    train = sp.csc_matrix((tx, ti, tp), shape=(n_user, n_item))
    cp, ci, cx = csc_drop_rows(900, p, i, x)
    cv = sp.csc_matrix((cx, ci, cp), shape=(n_user_all - 900, n_item)).tocsr()
    m = WRMF(rank=8, lambda_=0.1, feedback="implicit", solver="conjugate_gradient", precision="float", rng=1)
    m.fit_transform(train, n_iter=3, convergence_tol=-1)
    K = 7
    preds = m.predict(cv, K)
    assert preds.shape == (cv.shape[0], K) and preds.scores.shape == (cv.shape[0], K)
    emb = m.transform(cv)
    dense = emb.astype(np.float64) @ m.components.astype(np.float64)
    for r in range(cv.shape[0]):
        seen = set(cv.indices[cv.indptr[r]:cv.indptr[r + 1]])
        assert not (set(preds[r]) & seen)
        assert np.all(np.diff(preds.scores[r]) <= 1e-6)
        assert np.allclose(preds.scores[r], dense[r, preds[r]], rtol=1e-4, atol=1e-5)
    none = m.predict(cv, K, not_recommend=None, items_exclude=[0, 1, 2])
    assert not (set(none.ravel()) & {0, 1, 2})
