"""Popularity-weighted negative sampling without a device: the numpy specification of the stream
(`rsparse_amd.rng.sample_negatives_weighted`: the 128-bit product from 32-bit halves, the prefix and the quantization at their
edges, what every row must be, independence from the split of the rows, the fill of a row whose budget ends, the frequencies of
the draw) and the class on the CPU stand-in backend, which has no sampler and so gets the specification: `WRMF.sample_negatives(
weights=)`, `evaluate(negatives=, negative_weights=)` against `evaluate(candidates=)`, the warning on filled rows, the argument
errors.  Everything is integers: every comparison is ==."""
import random
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from rsparse_amd import rng as R

ROOT = Path(__file__).resolve().parent.parent


def _csr(rows):
    p = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    j = (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)
    return p, j


def test_the_high_product_equals_python_integers():
    rnd = random.Random(5)
    vs = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1, 2 ** 63] + [rnd.getrandbits(64) for _ in range(3000)]
    Ws = [1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1, 2 ** 62 + 12345] + [rnd.randrange(1, 2 ** 63) for _ in range(3000)]
    for W in Ws[:8]:     # every v against a few W at once (the array form)
        got = R.mul_hi64(np.array(vs, dtype=np.uint64), np.uint64(W))
        assert got.dtype == np.uint64 and [int(g) for g in got] == [(v * W) >> 64 for v in vs]
    n = min(len(vs), len(Ws))
    got = R.mul_hi64(np.array(vs[:n], dtype=np.uint64), np.array(Ws[:n], dtype=np.uint64))
    assert [int(g) for g in got] == [(v * W) >> 64 for v, W in zip(vs[:n], Ws[:n])]


def test_the_draw_equals_python_integers():
    """draw t of row g: the counter words, the word pairing, r = (v W) >> 64 and the search, spelled out with Python integers;
    W = 40 (2^32 - 1) needs the high half of the product"""
    w = np.full(40, 2 ** 32 - 1, dtype=np.uint32)
    C = R.weights_prefix(w)
    W = 40 * (2 ** 32 - 1)
    assert int(C[-1]) == W and C.dtype == np.uint64
    seed, g = 0xFEDCBA9876543210, 2 ** 31 + 3
    got = R.weighted_draws(seed, g, 0, 64, C)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    for t in range(64):
        o = [int(v) for v in R.philox4x32_10(np.array([(t >> 1) & 0xFFFFFFFF, g, 5, (t >> 1) >> 32], dtype=np.uint64), key)]
        v = (o[1] << 32 | o[0]) if t % 2 == 0 else (o[3] << 32 | o[2])
        r = (v * W) >> 64
        assert int(got[t]) == sum(1 for c in C if int(c) <= r) == r // (2 ** 32 - 1)
    assert np.array_equal(R.weighted_draws(seed, g, 40, 24, C), got[40:])      # t is a counter, not a state
    assert R.STREAM_WEIGHTED_NEGATIVES == 5 and R.weighted_budget(8) == 64 * 8 + 4096


def test_prefix_and_quantization_at_their_edges():
    assert np.array_equal(R.weights_prefix(np.ones(5, np.uint32)), np.arange(1, 6, dtype=np.uint64))
    big = R.weights_prefix(np.full(3, 2 ** 32 - 1, dtype=np.uint32))
    assert [int(c) for c in big] == [2 ** 32 - 1, 2 * (2 ** 32 - 1), 3 * (2 ** 32 - 1)]
    assert R.weights_prefix(np.zeros(0, np.uint32)).size == 0
    for bad in (np.array([1, 0, 2]), np.array([1, -1]), np.array([2 ** 32], dtype=np.int64), np.ones((2, 2), np.int32), np.ones(3)):
        with pytest.raises(ValueError):
            R.weights_prefix(bad)
    # floats: max(1, floor(v 2^24 / max v)), uint32
    q = R.quantize_weights(np.array([3.0, 3.0, 3.0]))
    assert q.dtype == np.uint32 and np.array_equal(q, [2 ** 24] * 3)                     # all equal: every weight is the maximum
    assert np.array_equal(R.quantize_weights(np.array([0.0, 1.0, 0.5, 1e-12], dtype=np.float32)), [1, 2 ** 24, 2 ** 23, 1])
    assert np.array_equal(R.quantize_weights(np.array([7.0, 2.0 ** 24])), [7, 2 ** 24])   # max at 2^24: the floats' own integers
    assert np.array_equal(R.quantize_weights(np.array([1.0, 3.0])), [(2 ** 24) // 3, 2 ** 24])
    # integers: as they are
    iw = np.array([1, 5, 2 ** 32 - 1], dtype=np.int64)
    assert R.quantize_weights(iw).dtype == np.uint32 and np.array_equal(R.quantize_weights(iw), iw)
    u = np.array([9, 1], dtype=np.uint32)
    assert np.array_equal(R.quantize_weights(u), u)
    for bad in (np.array([1, 0]), np.array([2 ** 32, 1], dtype=np.int64), np.array([-1, 1]), np.array([0.0, 0.0]), np.array([1.0, -0.5]),
                np.array([1.0, np.inf]), np.array([1.0, np.nan]), np.zeros(0), np.ones((2, 2))):
        with pytest.raises(ValueError):
            R.quantize_weights(bad)
    with pytest.raises(TypeError):
        R.quantize_weights(np.array(["a"]))
    # popularity: (column nnz + smoothing) ** power
    x = sp.csr_matrix(np.array([[1, 0, 2, 0], [3, 0, 0, 0], [4, 5, 0, 0]], dtype=np.float64))
    assert np.array_equal(R.popularity_weights(x, power=1.0, smoothing=1.0), [2 ** 24, 2 ** 23, 2 ** 23, 2 ** 22])
    assert np.array_equal(R.popularity_weights(x), R.quantize_weights(np.array([4.0, 2.0, 2.0, 1.0]) ** 0.75))


N_ITEM = 400


def _random_pattern(n_rows=61, seed=6):
    rng = np.random.default_rng(seed)
    lens = np.r_[0, N_ITEM, N_ITEM - 1, N_ITEM - 2, 1, rng.integers(0, 390, size=n_rows - 5)]
    seen = [np.sort(rng.choice(N_ITEM, size=l, replace=False)) for l in lens]
    keep = [s[::4] for s in seen]
    keep[7] = seen[7].copy()
    keep[8] = seen[8][:0]
    return seen, keep


def _zipf(n_item, power=1.0, seed=1):
    """Zipf counts over the items in a shuffled order, as integer weights"""
    c = 1e6 / np.arange(1, n_item + 1, dtype=np.float64) ** power
    return R.quantize_weights(np.random.default_rng(seed).permutation(c))


@pytest.mark.parametrize("n", [1, 5, 150])
def test_every_row_is_what_it_must_be(n):
    seen, keep = _random_pattern()
    sp_, sj = _csr(seen)
    kp, kj = _csr(keep)
    w = _zipf(N_ITEM)
    out_p, out_j, filled = R.sample_negatives_weighted(31, 0, sp_, sj, kp, kj, N_ITEM, n, w)
    assert out_p.dtype == np.int32 and out_j.dtype == np.int32 and out_p[0] == 0 and out_p.size == len(seen) + 1 and filled == 0
    for u, (s, k) in enumerate(zip(seen, keep)):
        row = out_j[out_p[u]:out_p[u + 1]]
        M = N_ITEM - s.size
        assert row.size == k.size + min(n, M)
        assert np.all(np.diff(row) > 0) and np.all(np.isin(k, row))
        neg = np.setdiff1d(row, k)
        assert neg.size == min(n, M) and not np.any(np.isin(neg, s)) and np.all((neg >= 0) & (neg < N_ITEM))
    none_p, none_j, _ = R.sample_negatives_weighted(31, 0, sp_, sj, None, None, N_ITEM, n, w)
    for u, k in enumerate(keep):      # the negatives do not depend on the keep rows
        assert np.array_equal(np.setdiff1d(out_j[out_p[u]:out_p[u + 1]], k), none_j[none_p[u]:none_p[u + 1]])
    # rows [a, b) sampled with row0 = a are rows a .. b - 1 of the whole
    whole_p, whole_j, _ = R.sample_negatives_weighted(31, 1000, sp_, sj, kp, kj, N_ITEM, n, w)
    for a, b in ((0, 20), (20, 61), (60, 61), (13, 13)):
        part_p, part_j, _ = R.sample_negatives_weighted(31, 1000 + a, sp_[a:b + 1], sj, kp[a:b + 1], kj, N_ITEM, n, w)
        assert np.array_equal(part_p, whole_p[a:b + 1] - whole_p[a]) and np.array_equal(part_j, whole_j[whole_p[a]:whole_p[b]])
    assert not np.array_equal(whole_j, out_j)                         # the row index is part of the stream
    other_w = R.sample_negatives_weighted(31, 0, sp_, sj, kp, kj, N_ITEM, n, _zipf(N_ITEM, seed=2))
    assert np.array_equal(other_w[0], out_p) and not np.array_equal(other_w[1], out_j)
    # the popular items are the negatives: the 40 heaviest items take more than their share of 10 %
    if n == 5:
        heavy = np.argsort(w)[-40:]
        assert np.isin(none_j, heavy).mean() > 0.5


def test_arguments_are_checked():
    sp_, sj = _csr([np.array([1, 2])])
    w = np.ones(5, np.uint32)
    for bad in (dict(n=0), dict(n=-1), dict(row0=-1), dict(seed=-1), dict(seed=2 ** 64), dict(n_item=-1), dict(keep_p=np.zeros(2, np.int32)),
                dict(w=np.ones(4, np.uint32)), dict(w=np.array([1, 1, 0, 1, 1], np.uint32)), dict(w=np.ones(5))):
        kw = dict(seed=1, row0=0, seen_p=sp_, seen_j=sj, keep_p=None, keep_j=None, n_item=5, n=2, w=w)
        kw.update(bad)
        with pytest.raises(ValueError):
            R.sample_negatives_weighted(**kw)
    with pytest.raises(NotImplementedError):
        R.sample_negatives_weighted(1, 0, sp_, sj, None, None, 5, 8193, w)


def test_a_row_whose_budget_ends_is_filled():
    """n_item = 64, w = [2^31, 1, ..., 1], seen = {5}, n = 8: item 0 takes all but 63 / 2^31 of the weight, so the 4608 draws of
    the budget find item 0 and (with probability 1e-4) nothing else; the row is item 0 and the seven lowest other admissible
    items"""
    w = np.ones(64, np.uint32)
    w[0] = 2 ** 31
    sp_, sj = _csr([np.array([5])])
    out_p, out_j, filled = R.sample_negatives_weighted(7, 0, sp_, sj, None, None, 64, 8, w)
    assert np.array_equal(out_p, [0, 8]) and np.array_equal(out_j, [0, 1, 2, 3, 4, 6, 7, 8]) and filled == 1
    # the heavy item seen: nothing is drawn that counts, the row is the eight lowest admissible items; two rows, both filled
    sp2, sj2 = _csr([np.array([0, 5]), np.array([0, 1, 2])])
    out_p, out_j, filled = R.sample_negatives_weighted(7, 0, sp2, sj2, sp2, sj2, 64, 8, w)
    assert np.array_equal(out_j[:10], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]) and np.array_equal(out_j[10:], np.arange(11)) and filled == 2
    # n >= M draws nothing and is no fill
    full = np.arange(60)
    out_p, out_j, filled = R.sample_negatives_weighted(7, 0, *_csr([full]), None, None, 64, 8, w)
    assert np.array_equal(out_j, [60, 61, 62, 63]) and filled == 0


def test_first_draw_frequencies_follow_the_weights():
    """six items with weights 1 .. 884, the first draw of 6000 rows: the count of item i is Binomial(6000, w_i / W), and stays
    within five standard deviations of its mean (the seed is fixed: the test is deterministic)"""
    w = np.array([1, 4, 17, 70, 290, 884], dtype=np.uint32)
    C = R.weights_prefix(w)
    rows = 6000
    first = np.array([R.weighted_draws(2024, g, 0, 1, C)[0] for g in range(rows)])
    p = w / w.sum()
    counts = np.bincount(first, minlength=6)
    z = (counts - rows * p) / np.sqrt(rows * p * (1 - p))
    print("counts", counts, "expected", rows * p, "z", z)
    assert counts.sum() == rows and np.all(np.abs(z) < 5.0)
    # ... and through the sampler: n = 1, nothing seen
    out_p, out_j, filled = R.sample_negatives_weighted(2024, 0, np.zeros(rows + 1, np.int32), np.zeros(0, np.int32), None, None, 6, 1, w)
    assert np.array_equal(out_j, first) and filled == 0


# ---- the class on the CPU stand-in --------------------------------------------------------------------------------------------

def _model():
    sys.path.insert(0, str(ROOT / "tests"))
    from test_metrics_abi import _eval_problem, _oracle_metrics_backend
    from rsparse_amd import WRMF
    m, held = _eval_problem()
    model = WRMF(rank=6, lambda_=0.1, feedback="implicit", solver="cholesky", precision="float", backend=_oracle_metrics_backend(), rng=1)
    model.fit_transform(m, n_iter=2, convergence_tol=-1)
    return model, m, held


def _spec_rows(model, m, held, n, seed, w):
    seen, keep = model._negatives_lists(m, m.shape[1], sp.csr_matrix(held), m, np.zeros(0, np.int64))
    return R.sample_negatives_weighted(seed, 0, seen.indptr, seen.indices, keep.indptr, keep.indices, m.shape[1], n, w)


@pytest.mark.parametrize("n", [5, 30])
def test_the_class_equals_the_specification(n):
    model, m, held = _model()
    n_item = m.shape[1]
    w = R.popularity_weights(m, power=1.0)
    assert w.shape == (n_item,) and w.dtype == np.uint32 and w.max() == 2 ** 24 and w.min() >= 1
    want_p, want_j, filled = _spec_rows(model, m, held, n, 4, w)
    assert filled == 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # nothing is filled: no warning
        cand = model.sample_negatives(m, n, actual=held, seed=4, weights=w)
        assert sp.issparse(cand) and cand.format == "csr" and cand.shape == m.shape and np.all(cand.data == 1.0)
        assert np.array_equal(cand.indptr, want_p) and np.array_equal(cand.indices, want_j)
        model.negatives_batch = 100                         # several sampling calls: the batching cannot change a row
        again = model.sample_negatives(m, n, actual=held, seed=4, weights=w)
        batched = model.evaluate(m, held, 5, negatives=n, seed=4, negative_weights=w)
        model.negatives_batch = None
        assert np.array_equal(again.indptr, want_p) and np.array_equal(again.indices, want_j)
        direct = model.evaluate(m, held, 5, negatives=n, seed=4, negative_weights=w)
        routed = model.evaluate(m, held, 5, candidates=sp.csr_matrix((np.ones(want_j.size), want_j, want_p), shape=m.shape))
    for name in ("ap", "ndcg"):
        assert np.array_equal(direct[name], routed[name], equal_nan=True) and np.array_equal(batched[name], routed[name], equal_nan=True)
    assert np.isfinite(direct["ap"]).sum() > 50
    # float weights are quantized: the same rows as their integers
    fw = (np.bincount(m.indices, minlength=n_item) + 1.0).astype(np.float64)
    assert np.array_equal(model.sample_negatives(m, n, actual=held, seed=4, weights=fw).indices, want_j)
    # weights=None is the uniform stream, bit for bit
    seen, keep = model._negatives_lists(m, n_item, sp.csr_matrix(held), m, np.zeros(0, np.int64))
    uni_p, uni_j = R.sample_negatives(4, 0, seen.indptr, seen.indices, keep.indptr, keep.indices, n_item, n)
    plain = model.sample_negatives(m, n, actual=held, seed=4, weights=None)
    assert np.array_equal(plain.indptr, uni_p) and np.array_equal(plain.indices, uni_j) and not np.array_equal(uni_j, want_j)
    uniform = model.evaluate(m, held, 5, negatives=n, seed=4, negative_weights=None)
    assert np.array_equal(uniform["ap"], model.evaluate(m, held, 5, negatives=n, seed=4)["ap"], equal_nan=True)


def test_filled_rows_are_warned_of_once():
    model, m, held = _model()
    n_item = m.shape[1]
    w = np.ones(n_item, dtype=np.int64)
    w[int(np.argmax(np.bincount(m.indices, minlength=n_item)))] = 2 ** 31        # all the weight on the item most users have seen
    want_p, want_j, filled = _spec_rows(model, m, held, 5, 9, w)
    assert filled > 0
    with pytest.warns(RuntimeWarning, match=r"%d row\(s\)" % filled) as rec:
        cand = model.sample_negatives(m, 5, actual=held, seed=9, weights=w)
    assert len([r for r in rec if r.category is RuntimeWarning]) == 1
    assert np.array_equal(cand.indptr, want_p) and np.array_equal(cand.indices, want_j)
    with pytest.warns(RuntimeWarning, match=r"%d row\(s\)" % filled):
        model.evaluate(m, held, 5, negatives=5, seed=9, negative_weights=w)


def test_argument_errors():
    model, m, held = _model()
    n_item = m.shape[1]
    w = np.ones(n_item, np.uint32)
    with pytest.raises(ValueError):
        model.evaluate(m, held, 5, negative_weights=w)                            # weights of nothing
    cand = model.sample_negatives(m, 5, actual=held, seed=1, weights=w)
    with pytest.raises(ValueError):
        model.evaluate(m, held, 5, candidates=cand, negative_weights=w)
    for bad in (w[:-1], np.ones(n_item + 1), np.zeros(n_item, np.int32), np.zeros(n_item), np.full(n_item, -1.0), np.full(n_item, np.nan),
                np.ones((n_item, 1))):
        with pytest.raises(ValueError):
            model.sample_negatives(m, 5, weights=bad)
        with pytest.raises(ValueError):
            model.evaluate(m, held, 5, negatives=5, negative_weights=bad)
