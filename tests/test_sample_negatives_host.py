"""Negative sampling without a device: the numpy specification of the stream (`rsparse_amd.rng.sample_negatives`: what every row
must be, independence from the split of the rows, uniformity, the draw's 64-bit arithmetic against Python integers) and the class
on the CPU stand-in backend, which has no `sample_negatives` and so gets the specification through the `hasattr` fallback:
`WRMF.sample_negatives`, `evaluate(negatives=)` against `evaluate(candidates=)`, the argument errors, and two gloo ranks against
one."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import rng as R

ROOT = Path(__file__).resolve().parent.parent


def _csr(rows):
    p = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    j = (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)
    return p, j


N_ITEM = 24


def _edge_pattern():
    """24 items; M = 24 (nothing seen), 0 (everything seen), 1, 2, 3 and 4 .. 11, four rows each; keep = every other seen item,
    and an empty keep in the last row of each M"""
    rng = np.random.default_rng(2)
    seen, keep = [], []
    for M in (24, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11):
        for c in range(4):
            s = np.sort(rng.choice(N_ITEM, size=N_ITEM - M, replace=False))
            seen.append(s)
            keep.append(s[:0] if c == 3 else s[::2])
    return seen, keep


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 30])
def test_every_row_is_what_it_must_be(n):
    """n = 1 .. 4 against M = 1, 2, 3 (duplicate draws are certain); n = M, n = M - 1, 2 n = M and 2 n = M + 1 all occur (M = 2 ..
    11 against n = 2 .. 5); M = 0 gives the keep items only"""
    seen, keep = _edge_pattern()
    sp_, sj = _csr(seen)
    kp, kj = _csr(keep)
    out_p, out_j = R.sample_negatives(31, 0, sp_, sj, kp, kj, N_ITEM, n)
    assert out_p.dtype == np.int32 and out_j.dtype == np.int32 and out_p[0] == 0 and out_p.size == len(seen) + 1
    hit = set()
    for u, (s, k) in enumerate(zip(seen, keep)):
        row = out_j[out_p[u]:out_p[u + 1]]
        M = N_ITEM - s.size
        assert row.size == k.size + min(n, M)
        assert np.all(np.diff(row) > 0)
        assert np.all(np.isin(k, row))
        neg = np.setdiff1d(row, k)
        assert neg.size == min(n, M) and not np.any(np.isin(neg, s)) and np.all((neg >= 0) & (neg < N_ITEM))
        hit |= {w for w, c in (("all", n >= M), ("n=M", n == M), ("n=M-1", n == M - 1), ("2n=M", 2 * n == M), ("2n=M+1", 2 * n == M + 1),
                               ("M=0", M == 0), ("nokeep", k.size == 0)) if c}
    if n in (2, 3, 4, 5):
        assert {"n=M", "n=M-1", "2n=M", "2n=M+1", "M=0", "nokeep"} <= hit
    # both keep pointers None = every keep row empty
    none_p, none_j = R.sample_negatives(31, 0, sp_, sj, None, None, N_ITEM, n)
    zero = np.zeros(len(seen) + 1, np.int32)
    same_p, same_j = R.sample_negatives(31, 0, sp_, sj, zero, np.zeros(0, np.int32), N_ITEM, n)
    assert np.array_equal(none_p, same_p) and np.array_equal(none_j, same_j)
    # the negatives do not depend on the keep rows
    for u, k in enumerate(keep):
        assert np.array_equal(np.setdiff1d(out_j[out_p[u]:out_p[u + 1]], k), none_j[none_p[u]:none_p[u + 1]])


def test_arguments_are_checked():
    sp_, sj = _csr([np.array([1, 2])])
    for bad in (dict(n=0), dict(n=-1), dict(row0=-1), dict(seed=-1), dict(seed=2 ** 64), dict(n_item=-1), dict(keep_p=np.zeros(2, np.int32))):
        kw = dict(seed=1, row0=0, seen_p=sp_, seen_j=sj, keep_p=None, keep_j=None, n_item=5, n=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            R.sample_negatives(**kw)
    with pytest.raises(NotImplementedError):
        R.sample_negatives(1, 0, sp_, sj, None, None, 5, 8193)


def _random_pattern(n_rows=97, n_item=400, seed=6):
    rng = np.random.default_rng(seed)
    seen = [np.sort(rng.choice(n_item, size=l, replace=False)) for l in rng.integers(0, 390, size=n_rows)]
    return n_item, _csr(seen), _csr([s[::4] for s in seen])


@pytest.mark.parametrize("n", [5, 150])
def test_rows_do_not_depend_on_the_split(n):
    n_item, (sp_, sj), (kp, kj) = _random_pattern()
    whole_p, whole_j = R.sample_negatives(8, 1000, sp_, sj, kp, kj, n_item, n)
    for a, b in ((0, 40), (40, 97), (96, 97), (13, 13)):
        # a part's row pointers are a slice of the whole's: absolute positions into seen_j / keep_j
        part_p, part_j = R.sample_negatives(8, 1000 + a, sp_[a:b + 1], sj, kp[a:b + 1], kj, n_item, n)
        assert np.array_equal(part_p, whole_p[a:b + 1] - whole_p[a]) and np.array_equal(part_j, whole_j[whole_p[a]:whole_p[b]])
    other_seed = R.sample_negatives(9, 1000, sp_, sj, kp, kj, n_item, n)
    other_row0 = R.sample_negatives(8, 1001, sp_, sj, kp, kj, n_item, n)
    assert np.array_equal(other_seed[0], whole_p) and not np.array_equal(other_seed[1], whole_j)
    assert np.array_equal(other_row0[0], whole_p) and not np.array_equal(other_row0[1], whole_j)


@pytest.mark.parametrize("n,seed", [(10, 12345), (30, 777)])
def test_every_admissible_item_is_equally_likely(n, seed):
    """n_item = 50, 10 seen, 4000 rows: the inclusion count of each of the 40 admissible items is Binomial(4000, n / 40); the
    largest standardised deviation stays below 4.5 (Bonferroni-safe for 40 items: P(|z| > 4.5) = 7e-6 each).  n = 30 takes the
    complement branch (the row draws the 10 ranks it leaves out)."""
    n_item, S, rows = 50, 10, 4000
    seen = np.sort(np.random.default_rng(0).choice(n_item, size=S, replace=False))
    out_p, out_j = R.sample_negatives(seed, 0, np.arange(0, S * rows + 1, S), np.tile(seen, rows), None, None, n_item, n)
    assert np.all(np.diff(out_p) == n)
    counts = np.bincount(out_j, minlength=n_item)
    adm = np.setdiff1d(np.arange(n_item), seen)
    assert counts[seen].sum() == 0
    q = n / adm.size
    z = (counts[adm] - rows * q) / np.sqrt(rows * q * (1 - q))
    print("n = %d: largest standardised deviation %.2f" % (n, np.abs(z).max()))
    assert np.abs(z).max() < 4.5


def test_the_draw_in_64_bit_arithmetic_equals_python_integers():
    M, g, seed = 2 ** 31 - 1, 2 ** 31 - 5, 0xFEDCBA9876543210
    got = R.negative_draws(seed, g, 0, 64, M)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    for t in range(64):
        o = [int(v) for v in R.philox4x32_10(np.array([(t >> 1) & 0xFFFFFFFF, g, 2, (t >> 1) >> 32], dtype=np.uint64), key)]
        w = (o[1] << 32 | o[0]) if t % 2 == 0 else (o[3] << 32 | o[2])
        assert int(got[t]) == (w * M) >> 64
    assert got.max() < M and got.max() > M // 2
    # draws further along the sequence are the same numbers (t is a counter, not a state)
    assert np.array_equal(R.negative_draws(seed, g, 40, 24, M), got[40:])
    # ... and the first d distinct of a sequence with certain repeats, by hand
    seq = [int(v) for v in R.negative_draws(5, 3, 0, 200, 4)]
    first = list(dict.fromkeys(seq))
    assert np.array_equal(R.first_distinct(5, 3, 4, 2), first[:2]) and len(first) == 4


# ---- the class on the CPU stand-in --------------------------------------------------------------------------------------------

def _model(rng=1, rank=6, fit=True):
    sys.path.insert(0, str(ROOT / "tests"))
    from test_metrics_abi import _eval_problem, _oracle_metrics_backend
    from rsparse_amd import WRMF
    m, held = _eval_problem()
    model = WRMF(rank=rank, lambda_=0.1, feedback="implicit", solver="cholesky", precision="float", backend=_oracle_metrics_backend(),
                 rng=rng)
    if fit:
        model.fit_transform(m, n_iter=2, convergence_tol=-1)
    return model, m, held


def _spec(x, held, nr, excl, n, seed, n_item):
    """the candidate matrix straight from the specification, the lists joined with numpy sets"""
    seen_rows, keep_rows = [], []
    for u in range(x.shape[0]):
        k = np.unique(held[u].indices) if held is not None else np.zeros(0, np.int64)
        s = np.unique(np.concatenate([k, nr[u].indices if nr is not None else [], excl])).astype(np.int64)
        seen_rows.append(s)
        keep_rows.append(k)
    sp_, sj = _csr(seen_rows)
    kp, kj = _csr(keep_rows)
    return R.sample_negatives(seed, 0, sp_, sj, kp, kj, n_item, n)


def test_sample_negatives_is_the_specification_on_the_joined_lists():
    model, m, held = _model()
    n_item = m.shape[1]
    for n, nr, excl in ((5, "x", ()), (5, None, (3, 7, 7, 50)), (40, "x", (0,))):
        cand = model.sample_negatives(m, n, actual=held, not_recommend=nr, items_exclude=excl, seed=11)
        want_p, want_j = _spec(m, held, m if isinstance(nr, str) else nr, np.unique(np.array(excl, dtype=np.int64)), n, 11, n_item)
        assert sp.issparse(cand) and cand.format == "csr" and cand.shape == m.shape and np.all(cand.data == 1.0)
        assert np.array_equal(cand.indptr, want_p) and np.array_equal(cand.indices, want_j)
        dense = cand.toarray() > 0
        held_mask = np.zeros(m.shape, bool)
        held_mask[np.repeat(np.arange(m.shape[0]), np.diff(held.indptr)), held.indices] = True      # (stored zeros are held out too)
        assert np.all(dense[held_mask])
        negatives = dense & ~held_mask
        assert not np.any(negatives[:, list(excl)])                    # items_exclude: never a negative
        if isinstance(nr, str):
            assert not np.any(negatives & (m.toarray() != 0))          # not_recommend = x: no negative the user interacted with
        else:
            assert np.any(negatives & (m.toarray() != 0))              # not_recommend = None: they are admissible
    # no held-out items: negatives only; several sampling calls give the same rows
    plain = model.sample_negatives(m, 7, seed=11)
    model.negatives_batch = 64
    again = model.sample_negatives(m, 7, seed=11)
    model.negatives_batch = None
    assert np.array_equal(plain.indptr, again.indptr) and np.array_equal(plain.indices, again.indices)
    assert np.array_equal(np.diff(plain.indptr), np.minimum(7, n_item - np.diff(sp.csr_matrix(m).indptr)))


def test_the_same_seed_gives_the_same_negatives_to_two_models_and_to_no_model():
    a, m, held = _model(rng=1, rank=6)
    b, _, _ = _model(rng=2, rank=4)
    unfitted, _, _ = _model(rng=3, fit=False)
    assert not np.array_equal(a.components.shape, b.components.shape)
    mats = [mod.sample_negatives(m, 9, actual=held, seed=2 ** 63 + 5) for mod in (a, b, unfitted)]
    for other in mats[1:]:
        assert np.array_equal(mats[0].indptr, other.indptr) and np.array_equal(mats[0].indices, other.indices)
    # seed=None: one draw from the model's generator -- reproducible through rng=, different from call to call
    c, _, _ = _model(rng=1, rank=6)
    first, second = a.sample_negatives(m, 9), a.sample_negatives(m, 9)
    assert np.array_equal(first.indices, c.sample_negatives(m, 9).indices) and not np.array_equal(first.indices, second.indices)
    with pytest.raises(ValueError):
        a.sample_negatives(m[:, :20], 9)              # a fitted model knows its number of items


@pytest.mark.parametrize("n", [5, 30])
def test_evaluate_with_negatives_equals_the_candidates_route(n):
    model, m, held = _model()
    cand = model.sample_negatives(m, n, actual=held, items_exclude=(1, 2), seed=4)
    routed = model.evaluate(m, held, 5, items_exclude=(1, 2), candidates=cand)
    direct = model.evaluate(m, held, 5, items_exclude=(1, 2), negatives=n, seed=4)
    model.negatives_batch = 100
    batched = model.evaluate(m, held, 5, items_exclude=(1, 2), negatives=n, seed=4)
    model.negatives_batch = None
    for name in ("ap", "ndcg"):
        assert np.array_equal(direct[name], routed[name], equal_nan=True) and np.array_equal(batched[name], routed[name], equal_nan=True)
    assert np.isfinite(direct["ap"]).sum() > 50
    other = model.evaluate(m, held, 5, items_exclude=(1, 2), negatives=n, seed=5)
    assert not np.array_equal(other["ap"], direct["ap"], equal_nan=True)


def test_argument_errors():
    from rsparse_amd import _lib
    model, m, held = _model()
    cand = model.sample_negatives(m, 5, actual=held, seed=1)
    with pytest.raises(ValueError):
        model.evaluate(m, held, 5, negatives=5, candidates=cand)
    for n in (0, -3):
        with pytest.raises(ValueError):
            model.evaluate(m, held, 5, negatives=n)
        with pytest.raises(ValueError):
            model.sample_negatives(m, n)
    with pytest.raises(TypeError):
        model.sample_negatives(m, 2.5)
    with pytest.raises(_lib.UnsupportedOnDevice):
        model.sample_negatives(m, 8193)
    with pytest.raises(_lib.UnsupportedOnDevice):
        model.evaluate(m, held, 5, negatives=8193)
    with pytest.raises(ValueError):
        model.evaluate(m, held, 0, negatives=5)
    with pytest.raises(ValueError):
        model.sample_negatives(m, 5, items_exclude=[m.shape[1]])
    with pytest.raises(ValueError):
        model.sample_negatives(m, 5, not_recommend=m[:10])
    with pytest.raises(ValueError):
        model.sample_negatives(m, 5, actual=held[:10])
    with pytest.raises(ValueError):
        model.sample_negatives(m, 5, seed=-1)
    with pytest.raises(TypeError):
        model.sample_negatives(m, 5, not_recommend=m.toarray())


# ---- two gloo ranks against one -------------------------------------------------------------------------------------------------

def _both(rng):
    model, m, held = _model(rng=1)
    model._rng = np.random.default_rng(rng)            # the ranks would draw different seeds: rank 0's is used
    cand = model.sample_negatives(m, 12, actual=held)
    ev = model.evaluate(m, held, 5, negatives=12, seed=21)
    return {"indptr": cand.indptr.copy(), "indices": cand.indices.copy(), "ap": ev["ap"], "ndcg": ev["ndcg"]}


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
        assert np.array_equal(got["indptr"], one["indptr"]) and np.array_equal(got["indices"], one["indices"])
        assert np.array_equal(got["ap"], one["ap"], equal_nan=True) and np.array_equal(got["ndcg"], one["ndcg"], equal_nan=True)
    assert not np.array_equal(_both(101)["indices"], one["indices"])          # rank 1's own seed would have given other rows
