"""Popularity-weighted negative sampling on the device (wrmf_sample_weighted.hip behind `HipBackend.weights_prefix` /
`HipBackend.sample_negatives_weighted`) against its numpy specification (`rsparse_amd.rng.sample_negatives_weighted`): out_p,
out_j and the filled count are compared with ==, there is no tolerance -- the feature is integer-only.  The pattern is the one of
tests/test_sample_negatives.py (300 rows over 6000 items; seen lengths that give n >= M rows, M = 0 / 1 and n = M - 1; the wave /
workgroup class break at n = 64 | 65); on top of it: weights that need the high half of the 64 x 64 product, a full table, a seen
row that holds the heavy items (most draws rejected), rows whose budget ends and that are filled (both team classes), heavy
items at the multiples of the table size (what the multiplicative hash is for), a seen row of 40 000 items among 60 000 and global rows around
2^31."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import _lib
from rsparse_amd import rng as R

pytestmark = pytest.mark.gpu

N_ITEM, N_ROWS, SEED = 6000, 300, 20241
LENS = (0, 1, 63, 64, 65, 1023, 1025, 5000, 5990, 5999, 6000)
ROW_KEEP_ALL, ROW_KEEP_NONE = 13, 16      # seen lengths 63 and 1023
_cache = {}


def _csr(rows):
    p = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    j = (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)
    return p, j


def _zipf(n_item, power=1.0, seed=1):
    """Zipf counts over the items in a shuffled order, as integer weights"""
    c = 1e6 / np.arange(1, n_item + 1, dtype=np.float64) ** power
    return R.quantize_weights(np.random.default_rng(seed).permutation(c))


def _pattern():
    """300 rows over 6000 items, seen lengths tiled from LENS; keep = every third seen item, one row keeps its whole seen row,
    one keeps nothing"""
    if "pat" not in _cache:
        rng = np.random.default_rng(3)
        seen = [np.sort(rng.choice(N_ITEM, size=LENS[u % len(LENS)], replace=False)) for u in range(N_ROWS)]
        keep = [s[::3] for s in seen]
        keep[ROW_KEEP_ALL] = seen[ROW_KEEP_ALL].copy()
        keep[ROW_KEEP_NONE] = seen[ROW_KEEP_NONE][:0]
        assert keep[ROW_KEEP_ALL].size == 63 and seen[ROW_KEEP_NONE].size == 1023
        _cache["pat"] = _csr(seen) + _csr(keep)
    return _cache["pat"]


def _weights(kind):
    if ("w", kind) not in _cache:
        _cache["w", kind] = {"zipf": lambda: _zipf(N_ITEM), "ones": lambda: np.ones(N_ITEM, np.uint32),
                             "max": lambda: np.full(N_ITEM, 2 ** 32 - 1, dtype=np.uint32)}[kind]()
    return _cache["w", kind]


def _want(n, kind="zipf", row0=0):
    """the specification's rows of the pattern, computed once per (n, weights, row0) and shared"""
    if ("want", n, kind, row0) not in _cache:
        sp_, sj, kp, kj = _pattern()
        _cache["want", n, kind, row0] = R.sample_negatives_weighted(SEED, row0, sp_, sj, kp, kj, N_ITEM, n, _weights(kind))
    return _cache["want", n, kind, row0]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _device(seed, row0, sp_, sj, kp, kj, n_item, n, w):
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    cum = be.weights_prefix(_dev(np.asarray(w, dtype=np.uint32).view(np.int32)))
    assert cum.dtype == torch.int64 and np.array_equal(cum.cpu().numpy().view(np.uint64), R.weights_prefix(w))
    op, oj, filled = be.sample_negatives_weighted(seed, row0, _dev(sp_), _dev(sj), None if kp is None else _dev(kp),
                                                  None if kj is None else _dev(kj), n_item, n, cum)
    torch.cuda.synchronize()
    assert op.dtype == torch.int32 and oj.dtype == torch.int32 and isinstance(filled, int)
    return op.cpu().numpy(), oj.cpu().numpy(), filled


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert got[2] == want[2]


@pytest.mark.parametrize("n", [1, 10, 63, 64, 65, 99, 256, 999])
def test_kernel_equals_the_specification(n):
    sp_, sj, kp, kj = _pattern()
    want = _want(n)
    got = _device(SEED, 0, sp_, sj, kp, kj, N_ITEM, n, _weights("zipf"))
    _same(got, want)
    got_p, got_j, _ = got
    # what the rows are, whatever the stream: |keep| + min(n, M) entries, ascending and unique, keep inside, no other seen item
    M = N_ITEM - np.diff(sp_)
    assert np.array_equal(np.diff(got_p), np.diff(kp) + np.minimum(n, M))
    for u in (0, 7, 8, 9, 10, ROW_KEEP_ALL, ROW_KEEP_NONE, 299):
        row, seen, keep = got_j[got_p[u]:got_p[u + 1]], sj[sp_[u]:sp_[u + 1]], kj[kp[u]:kp[u + 1]]
        assert np.all(np.diff(row) > 0) and np.all(np.isin(keep, row)) and not np.any(np.isin(np.setdiff1d(row, keep), seen))
        assert row.size == 0 or (row[0] >= 0 and row[-1] < N_ITEM)


@pytest.mark.parametrize("kind", ["ones", "max"])
@pytest.mark.parametrize("n", [1, 10, 63, 64, 65, 99, 256, 999])
def test_uniform_and_the_largest_weights(n, kind):
    """w = 1 everywhere (W = 6000: the product's low half only) and w = 2^32 - 1 everywhere (W = 2.6e13: its high half)"""
    sp_, sj, kp, kj = _pattern()
    _same(_device(SEED, 0, sp_, sj, kp, kj, N_ITEM, n, _weights(kind)), _want(n, kind))


def test_without_keep_rows():
    sp_, sj, _, _ = _pattern()
    w = _weights("zipf")
    _same(_device(SEED, 0, sp_, sj, None, None, N_ITEM, 65, w), R.sample_negatives_weighted(SEED, 0, sp_, sj, None, None, N_ITEM, 65, w))


def test_the_largest_n_fills_the_table():
    n, n_item, S = 8192, 20000, 100
    rng = np.random.default_rng(8)
    seen = [np.sort(rng.choice(n_item, size=S, replace=False)) for _ in range(3)]
    sp_, sj = _csr(seen)
    kp, kj = _csr([s[::10] for s in seen])
    w = _zipf(n_item, power=0.75)
    want = R.sample_negatives_weighted(9, 5, sp_, sj, kp, kj, n_item, n, w)
    got = _device(9, 5, sp_, sj, kp, kj, n_item, n, w)
    _same(got, want)
    assert np.array_equal(np.diff(got[0]), np.full(3, 10 + n))


def test_a_history_that_holds_the_heavy_items():
    """the seen row is the 3000 heaviest of 6000 items: more than 90 % of the draws are dropped, their indices still count"""
    w = _weights("zipf")
    heavy = np.sort(np.argsort(w, kind="stable")[-3000:])
    assert w[heavy].sum() > 0.9 * w.sum()
    sp_, sj = _csr([heavy, heavy[::2], heavy])
    kp, kj = _csr([heavy[::100], heavy[:0], heavy[:5]])
    for n in (10, 99):
        want = R.sample_negatives_weighted(12, 0, sp_, sj, kp, kj, N_ITEM, n, w)
        assert want[2] == 0
        _same(_device(12, 0, sp_, sj, kp, kj, N_ITEM, n, w), want)


@pytest.mark.parametrize("n,n_item", [(8, 64), (100, 400)])
def test_rows_whose_budget_ends_are_filled(n, n_item):
    """w = [2^31, 1, ..., 1]: a wave-class and a team-class call; rows that see item 0 draw nothing that counts, rows that do not
    draw item 0 and at most a few others; a row with n >= M is no fill"""
    w = np.ones(n_item, np.uint32)
    w[0] = 2 ** 31
    rng = np.random.default_rng(n)
    seen = [np.array([5]), np.array([0, 5]), np.zeros(0, np.int64), np.arange(n_item - n), np.arange(1, n_item - n - 1)]
    seen += [np.sort(rng.choice(n_item, size=l, replace=False)) for l in (3, n_item // 2, n_item - n - 1, n_item - n - 2)]
    sp_, sj = _csr(seen)
    kp, kj = _csr([s[::2] for s in seen])
    want = R.sample_negatives_weighted(7, 0, sp_, sj, kp, kj, n_item, n, w)
    assert 0 < want[2] < len(seen)
    if n == 8:
        assert np.array_equal(want[1][want[0][0]:want[0][1]], [0, 1, 2, 3, 4, 5, 6, 7, 8])      # keep = {5}
    _same(_device(7, 0, sp_, sj, kp, kj, n_item, n, w), want)


@pytest.mark.parametrize("n", [8, 48])
def test_heavy_items_at_the_multiples_of_the_table_size(n):
    """n_item = 32768, the heavy items at the ids that are multiples of 512 (the table size at n = 8): `item & (T - 1)` would
    send every one of them to slot 0"""
    n_item = 32768
    w = np.ones(n_item, np.uint32)
    w[::512] = 2 ** 12
    rng = np.random.default_rng(1)
    seen = [np.sort(rng.choice(n_item, size=l, replace=False)) for l in (0, 50, 50, 3000)] + [np.arange(0, n_item, 1024)]
    sp_, sj = _csr(seen)
    kp, kj = _csr([s[::7] for s in seen])
    want = R.sample_negatives_weighted(3, 0, sp_, sj, kp, kj, n_item, n, w)
    assert want[2] == 0 and np.sum(want[1] % 512 == 0) >= 5 * n // 2       # (8 heavy items in 9 draws: they collide in the table)
    _same(_device(3, 0, sp_, sj, kp, kj, n_item, n, w), want)


@pytest.mark.parametrize("n", [99, 999])
def test_a_seen_row_of_40000_items(n):
    n_item = 60000
    rng = np.random.default_rng(11)
    seen = [np.sort(rng.choice(n_item, size=l, replace=False)) for l in (40000, 0, 70, 59000, 40000)]
    sp_, sj = _csr(seen)
    kp, kj = _csr([s[::1000] for s in seen])
    w = _zipf(n_item, power=0.75)
    want = R.sample_negatives_weighted(1 << 40, 0, sp_, sj, kp, kj, n_item, n, w)
    got = _device(1 << 40, 0, sp_, sj, kp, kj, n_item, n, w)
    _same(got, want)


def test_global_rows_around_2_to_the_31():
    sp_, sj, kp, kj = _pattern()
    w = _weights("zipf")
    row0 = 2 ** 31 - 2
    want = R.sample_negatives_weighted(SEED, row0, sp_[:5], sj, kp[:5], kj, N_ITEM, 99, w)
    _same(_device(SEED, row0, sp_[:5], sj, kp[:5], kj, N_ITEM, 99, w), want)
    first = _want(99)
    assert not np.array_equal(want[1], first[1][:first[0][4]])           # the row index is part of the stream


def test_a_repeat_and_a_split_of_the_rows_are_identical():
    sp_, sj, kp, kj = _pattern()
    w = _weights("zipf")
    want = _want(99)
    for _ in range(2):
        _same(_device(SEED, 0, sp_, sj, kp, kj, N_ITEM, 99, w), want)
    # the row pointers of a part are a slice of the whole's: absolute positions into seen_j / keep_j
    a_p, a_j, a_f = _device(SEED, 0, sp_[:138], sj, kp[:138], kj, N_ITEM, 99, w)
    b_p, b_j, b_f = _device(SEED, 137, sp_[137:], sj, kp[137:], kj, N_ITEM, 99, w)
    assert np.array_equal(np.concatenate([a_p, a_p[-1] + b_p[1:]]), want[0])
    assert np.array_equal(np.concatenate([a_j, b_j]), want[1]) and a_f + b_f == want[2]
    other = _device(SEED + 1, 0, sp_, sj, kp, kj, N_ITEM, 99, w)
    assert np.array_equal(other[0], want[0]) and not np.array_equal(other[1], want[1])


def test_nothing_is_written_past_the_last_row_and_a_zero_weight_is_refused():
    lib = _lib.load()
    sp_, sj, kp, kj = _pattern()
    want_p, want_j, _ = _want(99)
    total = int(want_p[-1])
    d_sp, d_sj, d_kp, d_kj = _dev(sp_), _dev(sj), _dev(kp), _dev(kj)
    d_w = _dev(_weights("zipf").view(np.int32))
    cum = torch.zeros(N_ITEM, dtype=torch.int64, device="cuda:0")
    _lib.check(lib.rsparse_hip_weights_prefix_device(d_w.data_ptr(), N_ITEM, cum.data_ptr(), None))
    out_p = torch.full((N_ROWS + 1,), -7, dtype=torch.int32, device="cuda:0")
    out_j = torch.full((total + 5000,), -7, dtype=torch.int32, device="cuda:0")
    filled = torch.full((1,), -7, dtype=torch.int32, device="cuda:0")

    def call(cap, f):
        return lib.rsparse_hip_sample_negatives_weighted_device(SEED, 0, N_ROWS, N_ITEM, 99, d_sp.data_ptr(), d_sj.data_ptr(), d_kp.data_ptr(),
                                                                d_kj.data_ptr(), cum.data_ptr(), out_p.data_ptr(), out_j.data_ptr(), cap,
                                                                f, None)
    assert call(total - 1, filled.data_ptr()) == _lib.ERR_INVALID     # refused before the sampling launch: nothing of out_j is written
    torch.cuda.synchronize()
    assert bool((out_j == -7).all())
    _lib.check(call(total, None))                                     # exactly enough; the count is optional
    _lib.check(call(total, filled.data_ptr()))
    torch.cuda.synchronize()
    got = out_j.cpu().numpy()
    assert np.array_equal(out_p.cpu().numpy(), want_p) and np.array_equal(got[:total], want_j) and np.all(got[total:] == -7)
    assert int(filled[0]) == 0                                        # zeroed, then counted
    # a zero weight, in the last block of the prefix
    w0 = _weights("zipf").copy()
    w0[5999] = 0
    assert lib.rsparse_hip_weights_prefix_device(_dev(w0.view(np.int32)).data_ptr(), N_ITEM, cum.data_ptr(), None) == _lib.ERR_INVALID


def test_host_form_equals_the_specification():
    import ctypes
    fn = _lib.load().rsparse_hip_sample_negatives_weighted
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    sp_, sj, kp, kj = _pattern()
    w = _weights("zipf")
    want_p, want_j, _ = R.sample_negatives_weighted(SEED, 11, sp_[:40], sj, kp[:40], kj, N_ITEM, 99, w)
    n_rows = 39
    out_p = np.full(n_rows + 1, -1, np.int32)
    filled = np.full(1, -1, np.int64)
    sj39, kj39 = np.ascontiguousarray(sj[:sp_[39]]), np.ascontiguousarray(kj[:kp[39]])
    _lib.check(fn(SEED, 11, n_rows, N_ITEM, 99, vp(sp_), vp(sj39), vp(kp), vp(kj39), vp(w), vp(out_p), None, 0, None))
    assert np.array_equal(out_p, want_p)
    out_j = np.full(int(out_p[-1]) + 3, -1, np.int32)
    _lib.check(fn(SEED, 11, n_rows, N_ITEM, 99, vp(sp_), vp(sj39), vp(kp), vp(kj39), vp(w), vp(out_p), vp(out_j), int(out_p[-1]), vp(filled)))
    assert np.array_equal(out_p, want_p) and np.array_equal(out_j[:-3], want_j) and np.all(out_j[-3:] == -1) and filled[0] == 0


def test_evaluate_with_weighted_negatives_equals_the_candidates_route(ml_train):
    from rsparse_amd import WRMF
    n_user, n_item, p, i, x = ml_train
    train = sp.csc_matrix((x, i, p), shape=(n_user, n_item)).tocsr()
    model = WRMF(rank=8, lambda_=0.1, feedback="implicit", solver="cholesky", precision="float", rng=1)
    model.fit_transform(train[:300], n_iter=2, convergence_tol=-1)
    seen, held = train[:200].copy(), train[:200].copy()
    seen.data[1::2] = 0.0
    held.data[0::2] = 0.0
    seen.eliminate_zeros(); held.eliminate_zeros()
    w = R.popularity_weights(train, power=1.0)
    spec = model._negatives_lists(seen, n_item, sp.csr_matrix(held), seen, np.zeros(0, np.int64))
    want_p, want_j, filled = R.sample_negatives_weighted(7, 0, spec[0].indptr, spec[0].indices, spec[1].indptr, spec[1].indices, n_item, 99, w)
    assert filled == 0
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                 # nothing is filled: no warning
        cand = model.sample_negatives(seen, 99, actual=held, seed=7, weights=w)
        assert np.array_equal(cand.indptr, want_p) and np.array_equal(cand.indices, want_j) and np.all(cand.data == 1.0)
        direct = model.evaluate(seen, held, 10, negatives=99, seed=7, negative_weights=w)
        model.negatives_batch = 5000                                   # several sampling calls: the batching cannot change a row
        batched = model.evaluate(seen, held, 10, negatives=99, seed=7, negative_weights=w)
        model.negatives_batch = None
    routed = model.evaluate(seen, held, 10, candidates=sp.csr_matrix((np.ones(want_j.size), want_j, want_p), shape=seen.shape))
    for name in ("ap", "ndcg"):
        assert np.array_equal(direct[name], routed[name], equal_nan=True) and np.array_equal(batched[name], routed[name], equal_nan=True)
    uniform = model.evaluate(seen, held, 10, negatives=99, seed=7)
    assert not np.array_equal(uniform["ndcg"], direct["ndcg"], equal_nan=True)
    # rows that are filled: one warning with the specification's count
    wf = np.ones(n_item, np.int64)
    wf[int(np.argmax(np.diff(train[:200].tocsc().indptr)))] = 2 ** 31
    f_want = R.sample_negatives_weighted(7, 0, spec[0].indptr, spec[0].indices, spec[1].indptr, spec[1].indices, n_item, 99, wf)
    assert f_want[2] > 0
    with pytest.warns(RuntimeWarning, match=r"%d row\(s\)" % f_want[2]):
        f_cand = model.sample_negatives(seen, 99, actual=held, seed=7, weights=wf)
    assert np.array_equal(f_cand.indices, f_want[1])
