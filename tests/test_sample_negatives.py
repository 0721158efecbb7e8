"""Negative sampling on the device (wrmf_sample.hip behind `HipBackend.sample_negatives`) against its numpy specification
(`rsparse_amd.rng.sample_negatives`): out_p and out_j are compared with ==, there is no tolerance -- the feature is integer-only.
The shapes are the smallest that reach each branch: the wave / workgroup class break at n = 64 | 65, both sides of the complement
rule (2 n <= M or not), M = 0 / 1 and tiny M where duplicate draws are certain, a full table (n = 8192 with 2 n = M), a seen row
of 40 000 items (a long binary search with nothing staged), and global rows around 2^31 (counter word 1)."""
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


def _want(n, row0=0):
    """the specification's rows of the pattern, computed once per (n, row0) and shared"""
    if ("want", n, row0) not in _cache:
        sp_, sj, kp, kj = _pattern()
        _cache["want", n, row0] = R.sample_negatives(SEED, row0, sp_, sj, kp, kj, N_ITEM, n)
    return _cache["want", n, row0]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _device(seed, row0, sp_, sj, kp, kj, n_item, n):
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    op, oj = be.sample_negatives(seed, row0, _dev(sp_), _dev(sj), None if kp is None else _dev(kp), None if kj is None else _dev(kj),
                                 n_item, n)
    torch.cuda.synchronize()
    assert op.dtype == torch.int32 and oj.dtype == torch.int32
    return op.cpu().numpy(), oj.cpu().numpy()


@pytest.mark.parametrize("n", [1, 10, 63, 64, 65, 99, 256, 999])
def test_kernel_equals_the_specification(n):
    sp_, sj, kp, kj = _pattern()
    want_p, want_j = _want(n)
    got_p, got_j = _device(SEED, 0, sp_, sj, kp, kj, N_ITEM, n)
    assert np.array_equal(got_p, want_p)
    assert np.array_equal(got_j, want_j)
    # what the rows are, whatever the stream: |keep| + min(n, M) entries, ascending and unique, keep inside, no other seen item
    M = N_ITEM - np.diff(sp_)
    assert np.array_equal(np.diff(got_p), np.diff(kp) + np.minimum(n, M))
    for u in (0, 7, 8, 9, 10, ROW_KEEP_ALL, ROW_KEEP_NONE, 299):
        row, seen, keep = got_j[got_p[u]:got_p[u + 1]], sj[sp_[u]:sp_[u + 1]], kj[kp[u]:kp[u + 1]]
        assert np.all(np.diff(row) > 0) and np.all(np.isin(keep, row)) and not np.any(np.isin(np.setdiff1d(row, keep), seen))
        assert row.size == 0 or (row[0] >= 0 and row[-1] < N_ITEM)


def test_without_keep_rows():
    sp_, sj, _, _ = _pattern()
    want = R.sample_negatives(SEED, 0, sp_, sj, None, None, N_ITEM, 65)
    got = _device(SEED, 0, sp_, sj, None, None, N_ITEM, 65)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_tiny_admissible_sets(n):
    """M = 0 .. 12 of 40 items: duplicate draws are certain, and n = M, M - 1, 2 n = M, 2 n = M + 1 all occur"""
    n_item = 40
    rng = np.random.default_rng(5)
    seen = [np.sort(rng.choice(n_item, size=n_item - M, replace=False)) for M in list(range(13)) * 6]
    keep = [s[1::4] for s in seen]
    sp_, sj = _csr(seen)
    kp, kj = _csr(keep)
    want = R.sample_negatives(77, 0, sp_, sj, kp, kj, n_item, n)
    got = _device(77, 0, sp_, sj, kp, kj, n_item, n)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("M", [16384, 16383, 8000])
def test_the_largest_n(M):
    """n = 8192: 2 n = M (the most draws, a full table), M = 16383 (the complement: 8191 ranks left out), M = 8000 (take all)"""
    n, S = 8192, 100
    n_item = M + S
    rng = np.random.default_rng(M)
    seen = [np.sort(rng.choice(n_item, size=S, replace=False)) for _ in range(3)]
    sp_, sj = _csr(seen)
    kp, kj = _csr([s[::10] for s in seen])
    want = R.sample_negatives(9, 5, sp_, sj, kp, kj, n_item, n)
    got = _device(9, 5, sp_, sj, kp, kj, n_item, n)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(np.diff(got[0]), np.full(3, 10 + min(n, M)))


@pytest.mark.parametrize("n", [99, 999])
def test_a_long_seen_row_beyond_16_bits(n):
    n_item = 70001
    rng = np.random.default_rng(11)
    seen = [np.sort(rng.choice(n_item, size=l, replace=False)) for l in (40000, 0, 70, 69000, 40000)]
    sp_, sj = _csr(seen)
    kp, kj = _csr([s[::1000] for s in seen])
    want = R.sample_negatives(1 << 40, 0, sp_, sj, kp, kj, n_item, n)
    got = _device(1 << 40, 0, sp_, sj, kp, kj, n_item, n)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[1].max() > 65535


def test_global_rows_around_2_to_the_31():
    sp_, sj, kp, kj = _pattern()
    row0 = 2 ** 31 - 400
    want_p, want_j = _want(99, row0)
    got_p, got_j = _device(SEED, row0, sp_, sj, kp, kj, N_ITEM, 99)
    assert np.array_equal(got_p, want_p) and np.array_equal(got_j, want_j)
    assert not np.array_equal(want_j, _want(99)[1])                    # the row index is part of the stream
    past = _device(SEED, 2 ** 31 + 5, sp_[:3], sj, kp[:3], kj, N_ITEM, 99)     # and rows past 2^31
    want = R.sample_negatives(SEED, 2 ** 31 + 5, sp_[:3], sj, kp[:3], kj, N_ITEM, 99)
    assert np.array_equal(past[0], want[0]) and np.array_equal(past[1], want[1])


def test_a_repeat_and_a_split_of_the_rows_are_identical():
    sp_, sj, kp, kj = _pattern()
    want_p, want_j = _want(99)
    for _ in range(2):
        got_p, got_j = _device(SEED, 0, sp_, sj, kp, kj, N_ITEM, 99)
        assert np.array_equal(got_p, want_p) and np.array_equal(got_j, want_j)
    # the row pointers of a part are a slice of the whole's: absolute positions into seen_j / keep_j
    a_p, a_j = _device(SEED, 0, sp_[:138], sj, kp[:138], kj, N_ITEM, 99)
    b_p, b_j = _device(SEED, 137, sp_[137:], sj, kp[137:], kj, N_ITEM, 99)
    assert np.array_equal(np.concatenate([a_p, a_p[-1] + b_p[1:]]), want_p)
    assert np.array_equal(np.concatenate([a_j, b_j]), want_j)
    other = _device(SEED + 1, 0, sp_, sj, kp, kj, N_ITEM, 99)
    assert np.array_equal(other[0], want_p) and not np.array_equal(other[1], want_j)


def test_nothing_is_written_past_the_last_row():
    lib = _lib.load()
    sp_, sj, kp, kj = _pattern()
    want_p, want_j = _want(99)
    total = int(want_p[-1])
    d_sp, d_sj, d_kp, d_kj = _dev(sp_), _dev(sj), _dev(kp), _dev(kj)
    out_p = torch.full((N_ROWS + 1,), -7, dtype=torch.int32, device="cuda:0")
    out_j = torch.full((total + 5000,), -7, dtype=torch.int32, device="cuda:0")

    def call(cap):
        return lib.rsparse_hip_sample_negatives_device(SEED, 0, N_ROWS, N_ITEM, 99, d_sp.data_ptr(), d_sj.data_ptr(), d_kp.data_ptr(),
                                                       d_kj.data_ptr(), out_p.data_ptr(), out_j.data_ptr(), cap, None)
    assert call(total - 1) == _lib.ERR_INVALID           # refused before the sampling launch: nothing of out_j is written
    torch.cuda.synchronize()
    assert bool((out_j == -7).all())
    _lib.check(call(total))                              # exactly enough
    torch.cuda.synchronize()
    got = out_j.cpu().numpy()
    assert np.array_equal(out_p.cpu().numpy(), want_p) and np.array_equal(got[:total], want_j) and np.all(got[total:] == -7)


@pytest.mark.parametrize("negatives", [99, 999])
def test_evaluate_with_negatives_equals_the_candidates_route(ml_train, negatives):
    from rsparse_amd import WRMF
    n_user, n_item, p, i, x = ml_train
    train = sp.csc_matrix((x, i, p), shape=(n_user, n_item)).tocsr()
    model = WRMF(rank=8, lambda_=0.1, feedback="implicit", solver="cholesky", precision="float", rng=1)
    model.fit_transform(train[:300], n_iter=2, convergence_tol=-1)
    seen, held = train[:120].copy(), train[:120].copy()
    seen.data[1::2] = 0.0
    held.data[0::2] = 0.0
    seen.eliminate_zeros(); held.eliminate_zeros()
    cand = model.sample_negatives(seen, negatives, actual=held, seed=7)
    spec = model._negatives_lists(seen, n_item, sp.csr_matrix(held), seen, np.zeros(0, np.int64))
    want_p, want_j = R.sample_negatives(7, 0, spec[0].indptr, spec[0].indices, spec[1].indptr, spec[1].indices, n_item, negatives)
    assert np.array_equal(cand.indptr, want_p) and np.array_equal(cand.indices, want_j) and np.all(cand.data == 1.0)
    direct = model.evaluate(seen, held, 10, negatives=negatives, seed=7)
    model.negatives_batch = 20000                      # several sampling calls: the batching cannot change a row
    batched = model.evaluate(seen, held, 10, negatives=negatives, seed=7)
    model.negatives_batch = None
    routed = model.evaluate(seen, held, 10, candidates=cand)
    for name in ("ap", "ndcg"):
        assert np.array_equal(direct[name], routed[name], equal_nan=True) and np.array_equal(batched[name], routed[name], equal_nan=True)
    assert np.nanmean(direct["ndcg"]) > 0.3            # a fitted model ranks the held-out items above sampled negatives
    assert not np.array_equal(model.evaluate(seen, held, 10, negatives=negatives, seed=8)["ndcg"], direct["ndcg"])
