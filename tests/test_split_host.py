"""The train / test split without a device: the numpy specification of the stream (`rsparse_amd.rng.split_flags` / `split_rows`: the
draw against a scalar re-statement in Python integers, what every row must be, independence from the batching, uniformity, the
order-preserving `by` keys) and the public functions on the CPU stand-in backend, which has no `split_rows` and so gets the
specification through the `hasattr` fallback: `rsparse_amd.train_test_split`, `WRMF.train_test_split`, the argument errors, and
two gloo ranks against one."""
import math
import os
import socket
import struct
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import rng as R

ROOT = Path(__file__).resolve().parent.parent


def _philox(counter, seed):
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    return [int(v) for v in R.philox4x32_10(np.array(counter, dtype=np.uint64), key)]


def _scalar_flags(seed, g, L, T=None, n=None, min_train=1, by=None):
    """one row, in Python integers, straight from the definition"""
    if T is not None:
        return [_philox([t >> 2, g, 3, 0], seed)[t & 3] < T for t in range(L)]
    if by is None:
        w = []
        for t in range(L):
            o = _philox([t >> 1, g, 4, 0], seed)
            w.append((o[1] << 32 | o[0]) if t % 2 == 0 else (o[3] << 32 | o[2]))
    else:
        w = []
        for b in by:
            u = struct.unpack("<Q", struct.pack("<d", b))[0]
            w.append((~u & (2 ** 64 - 1)) if u >> 63 else (u | 2 ** 63))
    h = min(n, max(L - min_train, 0))
    first = sorted(range(L), key=lambda t: (-w[t], t))[:h]
    return [t in first for t in range(L)]


@pytest.mark.parametrize("seed,g", [(0xFEDCBA9876543210, 2 ** 32 - 1), (20241, 0), (7, 2 ** 31 + 5)])
def test_the_flags_equal_a_scalar_restatement_in_python_integers(seed, g):
    ip = np.array([0, 37])
    for T in (0, 1, 2 ** 31, int(math.floor(0.3 * 2.0 ** 32)), 2 ** 32):
        assert list(R.split_flags(seed, g, ip, test_threshold=T)) == _scalar_flags(seed, g, 37, T=T)
    for n, mt in ((1, 1), (5, 0), (36, 1), (40, 0)):
        assert list(R.split_flags(seed, g, ip, leave_out=n, min_train=mt)) == _scalar_flags(seed, g, 37, n=n, min_train=mt)
    by = np.array([3.0, -0.0, 0.0, 3.0, -2.0, np.inf, -np.inf] * 6)[:37]
    assert list(R.split_flags(seed, g, ip, leave_out=9, min_train=1, by=by)) == _scalar_flags(seed, g, 37, n=9, by=by)
    # positions past 2^20 (counter word 0 = t >> 2 / t >> 1): the tail of one long row, entry by entry
    L = 2 ** 20 + 9
    long_ip = np.array([0, L])
    prop = R.split_flags(seed, g, long_ip, test_threshold=2 ** 31)
    for t in (2 ** 20 - 1, 2 ** 20, 2 ** 20 + 3, 2 ** 20 + 8):
        assert bool(prop[t]) == (_philox([t >> 2, g, 3, 0], seed)[t & 3] < 2 ** 31)
    # leave-out keys at and beyond 2^20 (counter word 0 = t >> 1): the key of such a position, in Python integers, decides its flag.
    # With h of L entries held out the cut w* is the (1 - h / L) quantile of L uniform keys, known to 0.0005 (one sigma), so a
    # position whose key is further than 0.01 from it is test iff its key lies above -- and the positions held out of the tail
    # are exactly those with the largest keys of the tail, whatever the cut
    tail = list(range(2 ** 20 - 2, L))
    keys = {}
    for t in tail:
        o = _philox([t >> 1, g, 4, 0], seed)
        keys[t] = (o[1] << 32 | o[0]) if t % 2 == 0 else (o[3] << 32 | o[2])
    decided = 0
    for h in (L // 4, L // 2, (3 * L) // 4):
        lo = R.split_flags(seed, g, long_ip, leave_out=h, min_train=0)
        assert int(lo.sum()) == h
        cut = 1.0 - h / L
        for t in tail:
            u = keys[t] / 2.0 ** 64
            if abs(u - cut) > 0.01:
                assert bool(lo[t]) == (u > cut), (h, t)
                decided += 1
        held, kept = [keys[t] for t in tail if lo[t]], [keys[t] for t in tail if not lo[t]]
        assert not held or not kept or min(held) > max(kept)
    assert decided >= 3 * len(tail) - 3


def _random_csr(n_rows=120, n_col=500, seed=2, max_len=60):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len, size=n_rows)
    lens[:6] = (0, 1, 2, 3, 4, 5)
    rows = [np.sort(rng.choice(n_col, size=l, replace=False)) for l in lens]
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return p, np.concatenate(rows).astype(np.int32)


@pytest.mark.parametrize("kw", [dict(test_threshold=2 ** 30), dict(leave_out=3, min_train=1), dict(leave_out=2, min_train=0, by=True)],
                         ids=["proportion", "leave_out", "by"])
def test_train_plus_test_is_the_matrix_and_the_batching_changes_no_row(kw):
    p, j = _random_csr()
    kw = dict(kw)
    by = np.floor(np.random.default_rng(1).random(j.size) * 3.0) if kw.pop("by", False) else None
    tr_p, tr_j, tr_pos, te_p, te_j, te_pos = R.split_rows(9, 1000, p, j, by=by, **kw)
    n_rows = p.size - 1
    assert tr_p.dtype == te_p.dtype == tr_j.dtype == te_j.dtype == np.int32 and tr_p[0] == 0 and te_p[0] == 0
    assert np.array_equal(np.diff(tr_p) + np.diff(te_p), np.diff(p))
    assert np.array_equal(np.sort(np.concatenate([tr_pos, te_pos])), np.arange(j.size))   # every entry exactly once
    assert np.array_equal(tr_j, j[tr_pos]) and np.array_equal(te_j, j[te_pos])
    for q, pos in ((tr_p, tr_pos), (te_p, te_pos)):                                    # canonical: rows keep their order
        for u in range(n_rows):
            row = pos[q[u]:q[u + 1]]
            assert np.all(np.diff(row) > 0) and (row.size == 0 or (row[0] >= p[u] and row[-1] < p[u + 1]))
    # [0, N) at once, and as [0, a) + [a, N) with row0 = a and the row pointers as they stand
    for a in (1, 57, n_rows - 1):
        lo = R.split_rows(9, 1000, p[:a + 1], j, by=by, **kw)
        hi = R.split_rows(9, 1000 + a, p[a:], j, by=by, **kw)
        for o in (0, 3):
            assert np.array_equal(np.concatenate([lo[o], lo[o][-1] + hi[o][1:]]), (tr_p, te_p)[o // 3])
            assert np.array_equal(np.concatenate([lo[o + 2], hi[o + 2]]), (tr_pos, te_pos)[o // 3])
    if by is None:
        assert not np.array_equal(R.split_rows(10, 1000, p, j, **kw)[5], te_pos)      # the seed and the row index are part of it
        assert not np.array_equal(R.split_rows(9, 1001, p, j, **kw)[5], te_pos)


@pytest.mark.parametrize("min_train", [0, 1, 3])
@pytest.mark.parametrize("n", [1, 4, 30, 70])
def test_leave_out_row_counts(n, min_train):
    p, j = _random_csr()
    L = np.diff(p)
    assert (L < n).any() and (L > n + min_train).any() or n == 70
    flags = R.split_flags(5, 0, p, leave_out=n, min_train=min_train)
    got = np.add.reduceat(np.r_[flags, False].astype(np.int64), p[:-1])
    got[L == 0] = 0
    assert np.array_equal(got, np.minimum(n, np.maximum(L - min_train, 0)))


def test_threshold_zero_and_two_to_the_32():
    p, j = _random_csr()
    assert not R.split_flags(5, 0, p, test_threshold=0).any() and R.split_flags(5, 0, p, test_threshold=2 ** 32).all()
    some = R.split_flags(5, 0, np.array([0, 2 ** 16]), test_threshold=2 ** 16)        # p = 2^-16 over 2^16 entries
    assert 0 <= some.sum() < 12
    for bad in (dict(test_threshold=-1), dict(test_threshold=2 ** 32 + 1), dict(), dict(test_threshold=5, leave_out=1), dict(leave_out=0),
                dict(leave_out=1, min_train=-1), dict(test_threshold=5, by=np.zeros(j.size)), dict(leave_out=1, by=np.zeros(3)),
                dict(leave_out=1, by=np.full(j.size, np.nan))):
        with pytest.raises(ValueError):
            R.split_flags(5, 0, p, **bad)
    with pytest.raises(ValueError):
        R.split_flags(5, 2 ** 32 - 3, p, test_threshold=5)
    with pytest.raises(ValueError):
        R.split_flags(5, 0, np.array([0, 3, 2]), test_threshold=5)


# ---- statistics: seeds 20241 and 7, bound 4.5 sigma (the specification stays within 2.8 sigma on exactly these inputs: the bound
# catches a wrong word choice or a biased threshold without being tight) ------------------------------------------------------------

@pytest.mark.parametrize("seed", [20241, 7])
@pytest.mark.parametrize("prob", [0.1, 0.3, 0.5])
def test_proportion_mode_share(seed, prob):
    rows, L = 200, 1000
    flags = R.split_flags(seed, 0, np.arange(0, rows * L + 1, L), test_threshold=int(math.floor(prob * 2.0 ** 32)))
    z = (flags.sum() - rows * L * prob) / math.sqrt(rows * L * prob * (1 - prob))
    print("seed %d p = %.1f: z = %.2f" % (seed, prob, z))
    assert abs(z) < 4.5
    per_word = flags.reshape(-1, 4).sum(axis=0)                                        # each of the four words of a call
    zw = (per_word - rows * L / 4 * prob) / math.sqrt(rows * L / 4 * prob * (1 - prob))
    assert np.abs(zw).max() < 4.5


@pytest.mark.parametrize("seed", [20241, 7])
@pytest.mark.parametrize("L,h", [(8, 1), (8, 3), (100, 10)])
def test_random_leave_out_is_uniform_over_the_positions(seed, L, h):
    rows = 20_000
    flags = R.split_flags(seed, 0, np.arange(0, rows * L + 1, L), leave_out=h, min_train=1).reshape(rows, L)
    assert np.all(flags.sum(axis=1) == h)
    q = h / L
    z = (flags.sum(axis=0) - rows * q) / math.sqrt(rows * q * (1 - q))
    print("seed %d (L, h) = (%d, %d): largest standardised deviation %.2f" % (seed, L, h, np.abs(z).max()))
    assert np.abs(z).max() < 4.5


def test_by_keys_are_strictly_monotone_and_by_mode_is_a_stable_descending_argsort():
    ladder = np.array([-np.inf, -3.5, -0.0, 0.0, 1e-300, 2.0, 1.7e9, np.inf])
    k = R.by_keys(ladder)
    assert k.dtype == np.uint64 and np.all(k[1:] > k[:-1])
    with pytest.raises(ValueError):
        R.by_keys(np.array([1.0, np.nan]))
    rng = np.random.default_rng(3)
    rows = [np.full(9, 2.5),                                   # all equal: the first h positions
            rng.choice([1.0, 2.0, 3.0], size=40),              # three distinct values
            np.array([0.0, -0.0, np.inf, -np.inf, 0.0, -0.0, np.inf, -np.inf, 1.0]),
            rng.standard_normal(33), np.zeros(0), np.array([7.0])]
    p = np.concatenate([[0], np.cumsum([r.size for r in rows])])
    by = np.concatenate(rows)
    for n, mt in ((1, 1), (3, 1), (4, 0), (50, 0)):
        flags = R.split_flags(1, 0, p, leave_out=n, min_train=mt, by=by)
        assert np.array_equal(flags, R.split_flags(2, 5, p, leave_out=n, min_train=mt, by=by))   # no random word
        for u, r in enumerate(rows):
            h = min(n, max(r.size - mt, 0))
            # -0.0 orders just below +0.0: a stable argsort of (-value, with the sign of zero kept apart)
            order = sorted(range(r.size), key=lambda t: (-r[t], math.copysign(1.0, r[t]) < 0, t))
            want = np.zeros(r.size, bool)
            want[order[:h]] = True
            assert np.array_equal(flags[p[u]:p[u + 1]], want), (n, mt, u)
    first = R.split_flags(1, 0, p, leave_out=4, min_train=1, by=by)[:9]
    assert np.array_equal(first, np.arange(9) < 4)


# ---- the public functions on the CPU stand-in ---------------------------------------------------------------------------------

def _backend():
    sys.path.insert(0, str(ROOT / "tests"))
    from test_metrics_abi import _oracle_metrics_backend
    return _oracle_metrics_backend()


def _model(rng=1, rank=6, fit=False):
    sys.path.insert(0, str(ROOT / "tests"))
    from test_metrics_abi import _eval_problem
    from rsparse_amd import WRMF
    m, _ = _eval_problem()
    model = WRMF(rank=rank, lambda_=0.1, feedback="implicit", solver="cholesky", precision="float", backend=_backend(), rng=rng)
    if fit:
        model.fit_transform(m, n_iter=1, convergence_tol=-1)
    return model, sp.csr_matrix(m)


def _same(a, b):
    return all(np.array_equal(u.indptr, v.indptr) and np.array_equal(u.indices, v.indices) and
               np.array_equal(u.data.view(np.uint8), v.data.view(np.uint8)) and u.dtype == v.dtype and u.shape == v.shape
               for u, v in zip(a, b))


def _messy():
    """unsorted columns, a duplicate, a stored zero, an empty row; as COO"""
    rng = np.random.default_rng(8)
    base = sp.random(60, 90, density=0.1, format="coo", random_state=rng)
    free = int(np.setdiff1d(np.arange(90), base.col[base.row == 5])[0])
    r = np.r_[base.row, base.row[:3], 5]
    c = np.r_[base.col, base.col[:3], free]
    d = np.r_[base.data, base.data[:3], 0.0]
    perm = rng.permutation(r.size)
    return sp.coo_matrix((d[perm], (r[perm], c[perm])), shape=(60, 90))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_results_equal_the_specification_on_the_canonicalised_matrix(dtype):
    from rsparse_amd import train_test_split
    x = _messy().astype(dtype)
    canon = sp.csr_matrix(x)
    canon.sum_duplicates()
    assert (canon.data == 0).any()                                                    # the stored zero is an entry
    by = sp.csr_matrix((np.floor(np.random.default_rng(2).random(canon.nnz) * 4.0), canon.indices, canon.indptr), shape=canon.shape)
    before = (x.row.copy(), x.col.copy(), x.data.copy())
    for kw, spec in ((dict(test_proportion=0.25), dict(test_threshold=2 ** 30)), (dict(leave_out=2), dict(leave_out=2, min_train=1)),
                     (dict(leave_out=1, min_train=0, by=by), dict(leave_out=1, min_train=0, by=by.data))):
        train, test = train_test_split(x, seed=31, backend=_backend(), **kw)
        want = R.split_rows(31, 0, canon.indptr, canon.indices, **spec)
        for got, o in ((train, 0), (test, 3)):
            assert sp.issparse(got) and got.format == "csr" and got.shape == x.shape and got.dtype == dtype
            assert np.array_equal(got.indptr, want[o]) and np.array_equal(got.indices, want[o + 1])
            assert np.array_equal(got.data.view(np.uint8), canon.data[want[o + 2]].view(np.uint8))   # bit for bit
            assert got.has_sorted_indices and np.all(np.diff(got.indptr) >= 0)
        back = (train + test).tocsr()
        assert (back != canon).nnz == 0 and train.nnz + test.nnz == canon.nnz
    assert all(np.array_equal(a, b) for a, b in zip(before, (x.row, x.col, x.data)))  # x itself is left alone


@pytest.mark.parametrize("route", ["module", "model"])
def test_a_csr_input_that_is_not_canonical_is_left_alone(route):
    """sp.csr_matrix of a CSR shares its arrays and sum_duplicates works in place: x and `by` given as CSR with unsorted and
    duplicated columns must come back with their three arrays as they were"""
    from rsparse_amd import train_test_split
    indptr = np.array([0, 3, 4, 4, 8], np.int32)
    indices = np.array([5, 1, 5, 2, 7, 0, 3, 0], np.int32)                            # row 0: unsorted + duplicate; row 3 too
    x = sp.csr_matrix((np.arange(1.0, 9.0), indices.copy(), indptr.copy()), shape=(4, 9))
    by = sp.csr_matrix((np.array([3.0, 1.0, 4.0, 1.0, 5.0, 9.0, 2.0, 6.0]), indices.copy(), indptr.copy()), shape=(4, 9))
    assert not x.has_canonical_format
    keep = [(m.indptr.copy(), m.indices.copy(), m.data.copy()) for m in (x, by)]
    fn = (lambda **kw: train_test_split(x, backend=_backend(), **kw)) if route == "module" else (lambda **kw: _model()[0].train_test_split(x, **kw))
    for kw in (dict(test_proportion=0.5, seed=1), dict(leave_out=1, seed=1), dict(leave_out=1, by=by, seed=1)):
        train, test = fn(**kw)
        assert train.nnz + test.nnz == 6                                              # the canonical matrix has 6 entries
        canon = x.copy()
        canon.sum_duplicates()
        assert ((train + test) != canon).nnz == 0
        for m, (ip, idx, dat) in zip((x, by), keep):
            assert np.array_equal(m.indptr, ip) and np.array_equal(m.indices, idx) and np.array_equal(m.data, dat)
            assert m.data.size == m.indptr[-1] == 8


def test_values_survive_untouched():
    """bit patterns that arithmetic would change: NaN payloads, -0.0, denormals; and an element type that is not 4 or 8 bytes"""
    from rsparse_amd import train_test_split
    p, j = _random_csr()
    for dtype, bits in ((np.float32, np.uint32), (np.float64, np.uint64)):
        raw = np.random.default_rng(6).integers(0, np.iinfo(bits).max, size=j.size, dtype=bits)
        x = sp.csr_matrix((raw.view(dtype), j, p), shape=(p.size - 1, 500))
        train, test = train_test_split(x, test_proportion=0.4, seed=3, backend=_backend())
        want = R.split_rows(3, 0, p, j, test_threshold=int(math.floor(0.4 * 2.0 ** 32)))
        assert np.array_equal(train.data.view(bits), raw[want[2]]) and np.array_equal(test.data.view(bits), raw[want[5]])
    xb = sp.csr_matrix((np.ones(j.size, bool), j, p), shape=(p.size - 1, 500))
    train, test = train_test_split(xb, leave_out=1, seed=3, backend=_backend())
    assert train.dtype == test.dtype == np.bool_ and test.nnz == int((np.diff(p) > 1).sum()) and train.nnz + test.nnz == j.size


def test_the_same_seed_gives_the_same_split_to_two_models_and_to_the_module_function():
    from rsparse_amd import train_test_split
    a, m = _model(rng=1, rank=6, fit=True)
    b, _ = _model(rng=2, rank=4)
    for kw in (dict(test_proportion=0.2), dict(leave_out=1)):
        one = a.train_test_split(m, seed=2 ** 63 + 5, **kw)
        assert _same(one, b.train_test_split(m, seed=2 ** 63 + 5, **kw))
        assert _same(one, train_test_split(m, seed=2 ** 63 + 5, backend=_backend(), **kw))
        a.split_batch = 50                                        # several calls: the batching cannot change a row
        assert _same(one, a.train_test_split(m, seed=2 ** 63 + 5, **kw))
        a.split_batch = None
        assert not _same(one, a.train_test_split(m, seed=6, **kw))
    # seed=None: one draw from the model's generator -- reproducible through rng=, different from call to call
    c, _ = _model(rng=2, rank=4)
    first, second = b.train_test_split(m), b.train_test_split(m)
    assert _same(first, c.train_test_split(m)) and not _same(first, second)
    assert not _same(train_test_split(m, backend=_backend()), train_test_split(m, backend=_backend()))


def test_argument_errors():
    from rsparse_amd import train_test_split
    model, m = _model()
    by = m.copy()
    for fn in (lambda **kw: train_test_split(m, backend=_backend(), **kw), lambda **kw: model.train_test_split(m, **kw)):
        with pytest.raises(ValueError):
            fn(test_proportion=0.2, leave_out=1)
        for kw in (dict(test_proportion=-0.1), dict(test_proportion=1.5), dict(leave_out=0), dict(leave_out=-2), dict(leave_out=1, min_train=-1),
                   dict(by=by), dict(leave_out=1, by=by[:, :20]), dict(leave_out=1, by=by[:10]), dict(leave_out=1, by=by.toarray()),
                   dict(seed=-1), dict(seed=2 ** 64)):
            with pytest.raises(ValueError):
                fn(**kw)
        with pytest.raises(TypeError):
            fn(leave_out=1.5)
        other = by.copy()
        other.data[3] = np.nan
        with pytest.raises(ValueError):
            fn(leave_out=1, by=other)
        fewer = by.copy()
        fewer.data[0] = 0.0
        fewer.eliminate_zeros()
        with pytest.raises(ValueError):
            fn(leave_out=1, by=fewer)                             # not x's pattern
        assert fn(leave_out=1, by=by, seed=1)[1].nnz > 0
    with pytest.raises(TypeError):
        train_test_split(m.toarray(), backend=_backend())


# ---- two gloo ranks against one -------------------------------------------------------------------------------------------------

def _both(rng):
    model, m = _model(rng=1)
    model._rng = np.random.default_rng(rng)            # the ranks would draw different seeds: rank 0's is used
    out = {}
    by = sp.csr_matrix((np.floor(np.random.default_rng(4).random(m.nnz) * 6.0), m.indices, m.indptr), shape=m.shape)
    for name, kw in (("prop", dict(test_proportion=0.3)), ("lo", dict(leave_out=2)), ("by", dict(leave_out=1, by=by, seed=3))):
        train, test = model.train_test_split(m.astype(np.float32) if name == "lo" else m, **kw)
        out[name] = [a.copy() for mat in (train, test) for a in (mat.indptr, mat.indices, mat.data)]
    return out


def _worker(rank, ws, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT / "tests"))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        torch.save(_both(100 + rank), os.path.join(out_dir, "s%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_give_the_one_process_result(tmp_path):
    import torch.multiprocessing as mp
    one = _both(100)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        got = torch.load(tmp_path / ("s%d.pt" % r), weights_only=False)
        for name in one:
            assert len(got[name]) == 6
            for a, b in zip(got[name], one[name]):
                assert a.dtype == b.dtype and np.array_equal(a, b), name
