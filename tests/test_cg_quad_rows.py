"""The rows of at most 16 non-zeros of the last bucket at rank 128, implicit feedback, no global bias, run FOUR to a wave
(wrmf_cgp.hip, als_cgp_kernel<false, true, 16, true>): one 16-lane group per row, the workgroup's 16 rows as the 16 columns of
the matrix-core tile, the products written over the published vectors' LDS.  Built like tests/test_cg_pair_wide.py: every row
against the fp64 oracle at that file's tolerances, 1500 fixed-side vectors.  Rows of every length 0..16 and at the edges of the
four-slot blocks, waves whose four rows differ as much as they can, row counts that leave groups, waves and a workgroup's last
waves idle, a list long enough for three visits per wave (both LDS-DMA slots reused), rows that stop in the first CG step beside
rows that do not, confidences below 1, 0 / 1 / 3 CG steps, a list that both launches of the bucket share, and the same short rows
at rank 124 and under a global bias, which stay on the two-rows-per-wave kernel."""
import ctypes

import numpy as np
import pytest

from conftest import rel_fro
from oracle import wrmf_oracle as O
from rsparse_amd import als

pytestmark = pytest.mark.gpu
TOL = 1e-4       # tests/test_cg_pair_wide.py
ROW_TOL = 5e-4
N_ITEM = 1500
QUAD = "als_cgp_kernel<false, true, 16, true>"

LENGTHS = {
    "every_length": list(range(17)) * 3,
    "block_edges": [4, 5, 8, 9, 12, 13, 16] * 4,
    "unequal_quads": [16, 9, 1, 0] * 10,     # (the order is longest first: ten 16s, ten 9s, ... -- the waves at the seams mix them)
    "one_long_three_empty": [16, 0, 0, 0] * 5,
    "both_launches": list(np.random.default_rng(7).integers(0, 41, size=301)) + [0, 1, 16, 17, 32, 33, 40],
}
COUNTS = [1, 2, 3, 5, 15, 17, 63, 65]


def _rows_of_lengths(lengths, k, seed, scale=0.1, low_conf=False):
    """a CSC (columns = the rows to solve) whose column j has lengths[j] distinct random items"""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    p = np.zeros(len(lengths) + 1, dtype=np.int32)
    p[1:] = np.cumsum(lengths)
    # (distinct items per row = the positions of the row's smallest random keys, 2000 rows at a time: 30 000 rng.choice calls
    #  would take seconds)
    top = int(lengths.max(initial=0))
    parts = [np.zeros(0, dtype=np.int64)]
    for j0 in range(0, len(lengths), 2000):
        keys = rng.random((min(2000, len(lengths) - j0), N_ITEM))
        first = np.argpartition(keys, top, axis=1)[:, :top + 1]
        parts += [np.sort(first[j, :n]) for j, n in enumerate(lengths[j0:j0 + 2000])]
    idx = np.concatenate(parts).astype(np.int32)
    if low_conf:   # confidences in (0, 1) beside confidences above 1
        x = np.where(rng.random(idx.size) < 0.5, rng.uniform(0.05, 0.95, size=idx.size), 1.0 + rng.gamma(1.0, 2.0, size=idx.size))
    else:
        x = 1.0 + rng.gamma(1.0, 2.0, size=idx.size)
    x = x.astype(np.float32).astype(np.float64)
    X = np.asfortranarray((rng.standard_normal((k, N_ITEM)) * scale).astype(np.float32))
    Y0 = np.asfortranarray((rng.standard_normal((k, len(lengths))) * scale).astype(np.float32))
    return (N_ITEM, len(lengths), p, idx, x), X, Y0


def _check(csc, X, Y0, lens, steps=3, gbias=0.0, lam=0.1):
    _, _, p, i, x = csc
    k = X.shape[0]
    X64 = np.asfortranarray(X, dtype=np.float64)
    Yref = np.asfortranarray(Y0, dtype=np.float64).copy(order="F")
    lref = O.als_implicit(p, i, x, X64, Yref, O.gramian(X64, lam), lam, 1, steps, n_threads=8, global_bias=gbias)
    Y = Y0.copy(order="F")
    if gbias:
        loss = als.als_implicit(csc, X, Y, lam, 1, 1, steps, "float", False, False, initialize_bias_base=True,
                                global_bias=gbias, global_bias_base=np.zeros(k, dtype=np.float32))
    else:
        loss = als.als_implicit(csc, X, Y, lam, 1, 1, steps, "float", False, False)
    nref = np.linalg.norm(Yref, axis=0)
    err = np.linalg.norm(Y - Yref, axis=0) / np.maximum(nref, 1e-30)
    err[nref == 0] = np.abs(Y[:, nref == 0]).max(axis=0, initial=0.0) if (nref == 0).any() else 0.0
    print("rel_fro %.3g  loss rel %.3g  worst row %.3g (%d non-zeros)"
          % (rel_fro(Y, Yref), abs(loss - lref) / max(abs(lref), 1e-300), err.max(), int(lens[err.argmax()])))
    assert rel_fro(Y, Yref) < TOL
    assert abs(loss - lref) <= TOL * abs(lref), (loss, lref)
    assert err.max() < ROW_TOL, (int(err.argmax()), int(lens[err.argmax()]), float(err.max()))
    return Y, Yref


def _last_bucket_kernels(fn):
    """names of the kernels that the profile segments timed (a bucket's first launch that has rows) while fn() ran"""
    from rsparse_amd import _lib
    lib = _lib.load()
    _lib.check(lib.rsparse_hip_profile_enable(1))
    try:
        fn()
        buf = ctypes.create_string_buffer(8192)
        _lib.check(lib.rsparse_hip_profile_last_names(buf, 8192))
    finally:
        _lib.check(lib.rsparse_hip_profile_enable(0))
    return buf.value.decode()


@pytest.mark.parametrize("low_conf", [False, True])
@pytest.mark.parametrize("case", sorted(LENGTHS))
def test_short_rows_four_per_wave_match_the_oracle_per_row(case, low_conf):
    lens = np.asarray(LENGTHS[case], dtype=np.int64)
    csc, X, Y0 = _rows_of_lengths(lens, 128, seed=13 + len(case) + 5 * low_conf, low_conf=low_conf)
    _check(csc, X, Y0, lens)


@pytest.mark.parametrize("length", [16, 1])
@pytest.mark.parametrize("count", COUNTS)
def test_row_counts_that_leave_groups_and_waves_idle(count, length):
    lens = np.full(count, length, dtype=np.int64)
    csc, X, Y0 = _rows_of_lengths(lens, 128, seed=100 * length + count)
    _check(csc, X, Y0, lens)


def test_the_short_rows_run_on_the_four_row_kernel():
    lens = np.asarray(LENGTHS["every_length"], dtype=np.int64)
    csc, X, Y0 = _rows_of_lengths(lens, 128, seed=5)
    assert QUAD in _last_bucket_kernels(lambda: _check(csc, X, Y0, lens))


def test_three_visits_per_wave_reuse_both_index_slots():
    """30 000 rows: 7500 sets of four on 469 workgroups, four visits per wave"""
    lens = np.random.default_rng(41).integers(0, 17, size=30_000)
    csc, X, Y0 = _rows_of_lengths(lens, 128, seed=43)
    _check(csc, X, Y0, lens)


def test_early_convergence_beside_rows_that_do_not():
    """every other row starts at its converged solution (the first CG step ends it: |r|^2 < 1e-10), its neighbours in the wave
    do three steps"""
    lens = np.asarray([3, 16, 9, 12, 1, 5, 14, 8] * 10, dtype=np.int64)
    lam = 0.1
    csc, X, Y0 = _rows_of_lengths(lens, 128, seed=29)
    _, _, p, i, x = csc
    X64 = np.asfortranarray(X, dtype=np.float64)
    Ysol = np.asfortranarray(Y0, dtype=np.float64).copy(order="F")
    O.als_implicit(p, i, x, X64, Ysol, O.gramian(X64, lam), lam, 1, 60)
    Y0 = Y0.copy(order="F")
    Y0[:, ::2] = Ysol[:, ::2].astype(np.float32)
    _check(csc, X, Y0, lens, lam=lam)


@pytest.mark.parametrize("steps", [0, 1, 3])
def test_cg_step_counts(steps):
    lens = np.asarray(LENGTHS["every_length"], dtype=np.int64)
    csc, X, Y0 = _rows_of_lengths(lens, 128, seed=61)
    Y, _ = _check(csc, X, Y0, lens, steps=steps)
    if steps == 0:   # nothing but the loss is computed: a row with non-zeros keeps its warm start, an empty one is zeroed
        assert np.array_equal(Y[:, lens > 0], Y0[:, lens > 0])


def test_rank_124_and_a_global_bias_stay_on_the_two_row_kernel():
    lens = np.asarray(LENGTHS["every_length"] + LENGTHS["unequal_quads"], dtype=np.int64)
    csc, X, Y0 = _rows_of_lengths(lens, 124, seed=71)
    names = _last_bucket_kernels(lambda: _check(csc, X, Y0, lens))
    assert "als_cgp_kernel<false, false, 8, false>" in names and QUAD not in names
    csc, X, Y0 = _rows_of_lengths(lens, 128, seed=73)
    names = _last_bucket_kernels(lambda: _check(csc, X, Y0, lens, gbias=0.013))
    assert "als_cgp_kernel<true, false, 8, false>" in names and QUAD not in names
