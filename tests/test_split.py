"""The train / test split on the device (wrmf_split.hip behind `HipBackend.split_rows`) against its numpy specification
(`rsparse_amd.rng.split_rows`): both row-pointer arrays, both index arrays and both value arrays are compared with ==, there is no
tolerance -- the feature is integer-only and values are copied as opaque words.  One matrix serves every test: row lengths on
both sides of every class break of the kernels (a wave per row up to 256 entries, keys staged in LDS up to 4096, a workgroup's
round of 1024 positions, the four positions that share a Philox call) plus one row of 300 000 entries, which takes the select in
passes over recomputed keys."""
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import _lib
from rsparse_amd import rng as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
N_COL, SEED = 400_000, 20241
LENS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 40_000)
N_TILED, LONG = 320, 300_000
ROW_EQUAL, ROW_RISING = 19, 39          # two rows of 40 000 entries: `by` all equal / strictly increasing
PALETTES = ((-2.5, -0.0, 0.0), (1.0, 2.0, 3.0), (-np.inf, 0.0, np.inf), (-1e300, -1e-300, 1.7e9))
_cache = {}


def _matrix():
    """321 rows over 400 000 columns: lengths tiled from LENS, then the long row -> (p, j) int32"""
    if "mat" not in _cache:
        rng = np.random.default_rng(3)
        lens = [LENS[u % len(LENS)] for u in range(N_TILED)] + [LONG]
        rows = [np.sort(rng.choice(N_COL, size=l, replace=False)) for l in lens]
        p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        _cache["mat"] = (p, np.concatenate(rows).astype(np.int32))
    return _cache["mat"]


def _values(kind):
    """random bit patterns (NaNs and denormals among them): they must come out as they went in"""
    if ("val", kind) not in _cache:
        nnz = int(_matrix()[0][-1])
        rng = np.random.default_rng(5)
        _cache["val", kind] = {"f32": lambda: rng.integers(0, 2 ** 32, size=nnz, dtype=np.uint64).astype(np.uint32).view(np.int32),
                               "f64": lambda: rng.integers(-2 ** 63, 2 ** 63 - 1, size=nnz, dtype=np.int64),
                               "none": lambda: None}[kind]()
    return _cache["val", kind]


def _by():
    """three distinct values per row (ties everywhere), negative values and both zeros; one row all equal, one rising"""
    if "by" not in _cache:
        p, _ = _matrix()
        rng = np.random.default_rng(7)
        by = np.empty(int(p[-1]), np.float64)
        for u in range(p.size - 1):
            by[p[u]:p[u + 1]] = rng.choice(PALETTES[u % len(PALETTES)], size=p[u + 1] - p[u])
        by[p[ROW_EQUAL]:p[ROW_EQUAL + 1]] = 4.0
        by[p[ROW_RISING]:p[ROW_RISING + 1]] = np.arange(p[ROW_RISING + 1] - p[ROW_RISING]) - 777.0
        _cache["by"] = by
    return _cache["by"]


def _want(row0=0, with_by=False, **kw):
    """the specification's split of the matrix, computed once per parameter set and shared: (train_p, train_j, train_pos, test_p,
    test_j, test_pos)"""
    key = ("want", row0, with_by) + tuple(sorted(kw.items()))
    if key not in _cache:
        p, j = _matrix()
        _cache[key] = R.split_rows(SEED, row0, p, j, by=_by() if with_by else None, **kw)
    return _cache[key]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _device(seed, row0, p, j, v, by=None, **kw):
    from rsparse_amd.engine import HipBackend
    out = HipBackend().split_rows(seed, row0, _dev(p), _dev(j), _dev(v), by=_dev(by), **kw)
    torch.cuda.synchronize()
    assert out[0].dtype == out[1].dtype == out[3].dtype == out[4].dtype == torch.int32
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def _check(got, want, v):
    for o in (0, 3):
        assert np.array_equal(got[o], want[o])
        assert np.array_equal(got[o + 1], want[o + 1])
        if v is None:
            assert got[o + 2] is None
        else:
            assert got[o + 2].dtype == v.dtype and np.array_equal(got[o + 2], v[want[o + 2]])


@pytest.mark.parametrize("T", [0, 1, int(np.floor(0.1 * 2.0 ** 32)), 2 ** 31, int(np.floor(0.999 * 2.0 ** 32)), 2 ** 32])
def test_proportion_mode_equals_the_specification(T):
    p, j = _matrix()
    v = _values("f32")
    want = _want(test_threshold=T)
    got = _device(SEED, 0, p, j, v, test_threshold=T)
    _check(got, want, v)
    n_test, nnz = int(got[3][-1]), int(p[-1])
    assert n_test + int(got[0][-1]) == nnz
    if T in (0, 2 ** 32):
        assert n_test == (0 if T == 0 else nnz)
    elif T > 1:
        assert abs(n_test - nnz * T / 2.0 ** 32) < 6 * np.sqrt(nnz * 0.25)


@pytest.mark.parametrize("kind", ["f64", "none"])
@pytest.mark.parametrize("kw", [dict(test_threshold=2 ** 31), dict(leave_out=65, min_train=1)], ids=["proportion", "leave_out"])
def test_eight_byte_values_and_the_pattern_alone(kind, kw):
    p, j = _matrix()
    v = _values(kind)
    _check(_device(SEED, 0, p, j, v, **kw), _want(**kw), v)


@pytest.mark.parametrize("min_train", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 5000])
def test_leave_out_with_random_keys_equals_the_specification(n, min_train):
    """h = 0 (short rows), h = L (n above L with min_train = 0) and h on both sides of every class break"""
    p, j = _matrix()
    v = _values("f32")
    want = _want(leave_out=n, min_train=min_train)
    got = _device(SEED, 0, p, j, v, leave_out=n, min_train=min_train)
    _check(got, want, v)
    assert np.array_equal(np.diff(got[3]), np.minimum(n, np.maximum(np.diff(p) - min_train, 0)))


@pytest.mark.parametrize("n,min_train", [(1, 1), (2, 0), (3, 1), (64, 1), (1000, 1), (5000, 0), (39_999, 1)])
def test_leave_out_by_keys_equals_the_specification(n, min_train):
    p, j = _matrix()
    v = _values("f32")
    by = _by()
    want = _want(with_by=True, leave_out=n, min_train=min_train)
    got = _device(SEED, 0, p, j, v, by=by, leave_out=n, min_train=min_train)
    _check(got, want, v)
    h = np.minimum(n, np.maximum(np.diff(p) - min_train, 0))
    for u, first in ((ROW_EQUAL, True), (ROW_RISING, False)):    # all equal: the FIRST h positions; rising: the LAST h
        test_rows = got[4][got[3][u]:got[3][u + 1]]
        row = j[p[u]:p[u + 1]]
        assert np.array_equal(test_rows, row[:h[u]] if first else row[row.size - h[u]:])
    assert np.array_equal(_device(SEED + 9, 0, p, j, v, by=by, leave_out=n, min_train=min_train)[4], want[4])   # no random word


@pytest.mark.parametrize("row0", [2 ** 31 - 3, 2 ** 32 - (N_TILED + 1)])
@pytest.mark.parametrize("kw", [dict(test_threshold=2 ** 31), dict(leave_out=2, min_train=1)], ids=["proportion", "leave_out"])
def test_global_rows_up_to_2_to_the_32(row0, kw):
    p, j = _matrix()
    v = _values("f32")
    want = _want(row0=row0, **kw)
    _check(_device(SEED, row0, p, j, v, **kw), want, v)
    assert not np.array_equal(want[4], _want(**kw)[4])          # the row index is part of the stream


@pytest.mark.parametrize("kw", [dict(test_threshold=2 ** 31), dict(leave_out=65, min_train=1)], ids=["proportion", "leave_out"])
def test_a_slice_of_the_row_pointers_a_repeat_and_another_seed(kw):
    p, j = _matrix()
    v = _values("f32")
    want = _want(**kw)
    first = _device(SEED, 0, p, j, v, **kw)
    again = _device(SEED, 0, p, j, v, **kw)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    _check(first, want, v)
    # rows [137, end) with row0 = 137 and the row pointers as they stand (absolute positions): the same rows
    cut = 137
    part = _device(SEED, cut, p[cut:], j, v, **kw)
    for o in (0, 3):
        assert np.array_equal(part[o], want[o][cut:] - want[o][cut])
        assert np.array_equal(part[o + 1], want[o + 1][want[o][cut]:])
        assert np.array_equal(part[o + 2], v[want[o + 2][want[o][cut]:]])
    other = _device(SEED + 1, 0, p, j, v, **kw)
    assert not np.array_equal(other[4], want[4])


def test_a_small_capacity_is_refused_and_nothing_is_written_past_the_end():
    lib = _lib.load()
    p, j = _matrix()
    v = _values("f32")
    want = _want(test_threshold=2 ** 31)
    n_rows, n_tr, n_te = p.size - 1, int(want[0][-1]), int(want[3][-1])
    d_p, d_j, d_v = _dev(p), _dev(j), _dev(v)
    mk = lambda n: torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    tr_p, te_p, tr_j, tr_v, te_j, te_v = mk(n_rows + 1), mk(n_rows + 1), mk(n_tr + 100), mk(n_tr + 100), mk(n_te + 100), mk(n_te + 100)

    def call(cap_tr, cap_te, outputs=True):
        o = (lambda t: t.data_ptr()) if outputs else (lambda t: None)
        return lib.rsparse_hip_split_rows_device(SEED, 0, n_rows, 0, 2 ** 31, 0, 1, d_p.data_ptr(), d_j.data_ptr(), d_v.data_ptr(), 4, None,
                                                 tr_p.data_ptr(), o(tr_j), o(tr_v), te_p.data_ptr(), o(te_j), o(te_v), cap_tr, cap_te, None)
    for caps in ((n_tr - 1, n_te), (n_tr, n_te - 1)):
        assert call(*caps) == _lib.ERR_INVALID                # refused before the compaction: no entry is written
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in (tr_j, tr_v, te_j, te_v))
    assert np.array_equal(tr_p.cpu().numpy(), want[0]) and np.array_equal(te_p.cpu().numpy(), want[3])   # the sizes are there
    tr_p.fill_(-7); te_p.fill_(-7)
    _lib.check(call(0, 0, outputs=False))                      # the counting call
    torch.cuda.synchronize()
    assert np.array_equal(tr_p.cpu().numpy(), want[0]) and np.array_equal(te_p.cpu().numpy(), want[3])
    _lib.check(call(n_tr, n_te))                               # exactly enough
    torch.cuda.synchronize()
    for t, n, w in ((tr_j, n_tr, want[1]), (tr_v, n_tr, v[want[2]]), (te_j, n_te, want[4]), (te_v, n_te, v[want[5]])):
        got = t.cpu().numpy()
        assert np.array_equal(got[:n], w) and np.all(got[n:] == -7)
    # row pointers that decrease or are negative: refused, nothing written
    tr_j.fill_(-7)
    for bad in (np.array([3, 2, 3], np.int32), np.array([-1, 0, 2], np.int32), np.array([0, 3, 2], np.int32)):
        d_bad = _dev(bad)
        rc = lib.rsparse_hip_split_rows_device(SEED, 0, 2, 0, 2 ** 31, 0, 1, d_bad.data_ptr(), d_j.data_ptr(), None, 0, None,
                                               tr_p.data_ptr(), tr_j.data_ptr(), None, te_p.data_ptr(), te_j.data_ptr(), None, 100, 100, None)
        torch.cuda.synchronize()
        assert rc == _lib.ERR_INVALID and bool((tr_j == -7).all())


@pytest.mark.parametrize("kw", [dict(test_proportion=0.3), dict(leave_out=2), dict(leave_out=1, min_train=0, by=True)],
                         ids=["proportion", "leave_out", "by"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_train_test_split_equals_the_cpu_stand_in(kw, dtype):
    sys.path.insert(0, str(ROOT / "tests"))
    from test_metrics_abi import _oracle_metrics_backend
    from rsparse_amd import WRMF, train_test_split
    from rsparse_amd import split as S
    rng = np.random.default_rng(12)
    x = sp.random(2000, 3000, density=0.01, format="csr", dtype=np.float64, random_state=rng).astype(dtype)
    kw = dict(kw)
    if kw.pop("by", False):
        kw["by"] = sp.csr_matrix((np.floor(rng.random(x.nnz) * 5.0), x.indices, x.indptr), shape=x.shape)
    want = train_test_split(x, seed=77, backend=_oracle_metrics_backend(), **kw)
    got = train_test_split(x, seed=77, **kw)
    model = WRMF(rank=4, feedback="implicit", precision="float")
    model.split_batch = 5000                                   # several device calls: the batching cannot change a row
    batched = model.train_test_split(x, seed=77, **kw)
    for res in (got, batched):
        for a, b in zip(res, want):
            assert a.dtype == dtype and a.shape == x.shape and a.has_sorted_indices
            assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data)
    back = (got[0] + got[1]).tocsr()
    back.sort_indices()
    assert np.array_equal(back.indptr, x.indptr) and np.array_equal(back.indices, x.indices) and np.array_equal(back.data, x.data)
    assert got[1].nnz > 0 and got[0].nnz > got[1].nnz
    assert S.SPLIT_BATCH > x.nnz


@pytest.mark.parametrize("kw", [dict(test_proportion=0.5), dict(leave_out=1)], ids=["proportion", "leave_out"])
def test_rows_without_a_stored_entry(kw):
    """nnz = 0: the backend call and the public function give empty outputs, as the CPU stand-in does"""
    from rsparse_amd import train_test_split
    from rsparse_amd.engine import HipBackend
    spec = dict(test_threshold=2 ** 31) if "test_proportion" in kw else dict(leave_out=1, min_train=1)
    for v in (None, torch.zeros(0, dtype=torch.int32, device="cuda:0")):
        out = HipBackend().split_rows(3, 0, torch.zeros(6, dtype=torch.int32, device="cuda:0"), torch.zeros(0, dtype=torch.int32, device="cuda:0"),
                                      v, **spec)
        assert all(int(t.sum()) == 0 and t.numel() == 6 for t in (out[0], out[3])) and out[1].numel() == 0 and out[4].numel() == 0
    for dtype in (np.float32, np.float64):
        train, test = train_test_split(sp.csr_matrix((5, 7), dtype=dtype), seed=3, **kw)
        for m in (train, test):
            assert m.shape == (5, 7) and m.nnz == 0 and m.dtype == dtype and np.array_equal(m.indptr, np.zeros(6))
    # a matrix whose LAST rows are empty and fall into a batch of their own
    x = sp.csr_matrix((np.ones(4, np.float32), np.array([0, 1, 2, 3]), np.array([0, 4, 4, 4])), shape=(3, 7))
    from rsparse_amd import WRMF
    model = WRMF(rank=4, feedback="implicit", precision="float")
    model.split_batch = 2
    train, test = model.train_test_split(x, seed=3, **kw)
    assert train.nnz + test.nnz == 4 and ((train + test) != x).nnz == 0
