"""Bucket 1 of the quad-layout CG kernels (rows of 257..512 non-zeros) at rank 97..128 without a global bias runs in up to three
launches: the rows of more than W = 384 non-zeros on 8-wave teams, the rows of 321..W on 4-wave teams of 24 quads per wave and the
rows of 257..320 on 4-wave teams of 20 quads per wave (wrmf_cgq.hip; the cuts are QSchedule::team4_wide_first <= team4_first).
Checked per row and on the loss against the fp64 oracle at the tolerances of tests/test_cg_team_split.py: rows exactly on the
edges (320 | 321, W | W + 1, a last quad that is partly filled: 321, 322, W - 1; a last quad-pass block that is: W - 4), a
bucket 1 of wide rows only and one with none (the launch is skipped and owns no loss slot: the loss would show a shifted slot),
implicit and explicit feedback, the padded rank (128) and a rank below it (100: the instantiation that clamps and selects behind
its loads), and the global-bias variant, whose bucket 1 stays on the 8-wave kernel (the profile segment of the bucket names the
kernel that ran).

A launch of at most 512 rows gives every team one row (wrmf_cgq.hip team_grid), and a team does three things only from its
second row on: it takes the row's indices and values from the LDS slot that its previous row's sweeps filled by LDS-DMA, it
reuses the t-, confidence-, x- and loss-slots the previous row left, and at a padded rank it requests the next row's pointers
behind the first sweep.  The "many" case has 1100 rows of 321..W non-zeros -- three per team -- next to rows of the two
neighbouring launches.

The balanced shares give every wave of a team ceil(n / 4) non-zeros rounded up to 16, at most 96: from 321 non-zeros on no wave of
the wide launch is without a share (the last one holds n - 288 >= 33), so that path of the kernel is the 8-wave launch's alone."""
import ctypes

import numpy as np
import pytest

from conftest import rel_fro
from oracle import wrmf_oracle as O
from rsparse_amd import als

pytestmark = pytest.mark.gpu
TOL = 1e-4
ROW_TOL = 5e-4   # per row, as tests/test_cg_team_split.py
W = 384          # kTeam4WideMax (rsparse_amd/csrc/wrmf_schedule.h): 4 waves x 24 quads x 4 non-zeros

EDGES = [320, 321, 322, W - 4, W - 1, W, W + 1, 512]
LENGTHS = {
    "edges": EDGES * 24 + [1, 40, 130, 257, 700],                            # 197 columns
    "wide_only": [321, 322, 350, W - 4, W - 1, W] * 5 + [3, 64, 200],
    "no_wide": [257, 300, 320, W + 1, 450, 512] * 5 + [3, 64, 200],
    # ceil(1100 / 512) = 3 rows per wide team; lengths drawn once, edges included
    "many": list(np.random.default_rng(9).integers(321, W + 1, size=1092)) + [321, 322, W - 4, W - 1, W, W, 321, W]
            + list(np.random.default_rng(10).integers(257, 321, size=60)) + list(np.random.default_rng(11).integers(W + 1, 513, size=60))
            + [3, 64, 200, 700],
}
N_ITEM = 1500


def _rows_of_lengths(lengths, k, seed, scale=0.1):
    """a CSC (columns = the rows to solve) whose column j has lengths[j] distinct random items, values >= 1"""
    rng = np.random.default_rng(seed)
    p = np.zeros(len(lengths) + 1, dtype=np.int32)
    p[1:] = np.cumsum(lengths)
    idx = np.concatenate([np.sort(rng.choice(N_ITEM, size=int(n), replace=False)) for n in lengths]).astype(np.int32)
    x = (1.0 + rng.gamma(1.0, 2.0, size=idx.size)).astype(np.float32).astype(np.float64)
    X = np.asfortranarray((rng.standard_normal((k, N_ITEM)) * scale).astype(np.float32))
    Y0 = np.asfortranarray((rng.standard_normal((k, len(lengths))) * scale).astype(np.float32))
    return (N_ITEM, len(lengths), p, idx, x), X, Y0


def _check(Y, Yref, loss, lref, lens):
    err = np.linalg.norm(Y - Yref, axis=0) / np.maximum(np.linalg.norm(Yref, axis=0), 1e-30)
    print("rel_fro %.3g  loss rel %.3g  worst row %.3g (%d non-zeros)"
          % (rel_fro(Y, Yref), abs(loss - lref) / abs(lref), err.max(), int(lens[err.argmax()])))
    assert rel_fro(Y, Yref) < TOL
    assert abs(loss - lref) <= TOL * abs(lref), (loss, lref)
    assert err.max() < ROW_TOL, (int(err.argmax()), int(lens[err.argmax()]), float(err.max()))


def _solve_both(case, k, implicit, gbias=0.0):
    lens = np.asarray(LENGTHS[case], dtype=np.int64)
    csc, X, Y0 = _rows_of_lengths(lens, k, seed=k + 3 * implicit + len(case))
    _, _, p, i, x = csc
    cnt = np.bincount(i, minlength=N_ITEM).astype(np.float64)
    X64 = np.asfortranarray(X, dtype=np.float64)
    Yref = np.asfortranarray(Y0, dtype=np.float64).copy(order="F")
    Y = Y0.copy(order="F")
    if implicit:
        lref = O.als_implicit(p, i, x, X64, Yref, O.gramian(X64, 0.1), 0.1, 1, 3, n_threads=8, global_bias=gbias)
        if gbias:
            loss = als.als_implicit(csc, X, Y, 0.1, 1, 1, 3, "float", False, False, initialize_bias_base=True,
                                    global_bias=gbias, global_bias_base=np.zeros(k, dtype=np.float32))
        else:
            loss = als.als_implicit(csc, X, Y, 0.1, 1, 1, 3, "float", False, False)
    else:
        lref = O.als_explicit(p, i, x, X64, Yref, cnt, 0.1, 1, 3, True, n_threads=8)
        loss = als.als_explicit(csc, X, Y, cnt.astype(np.float32), 0.1, 1, 1, 3, True, "float", False, False)
    _check(Y, Yref, loss, lref, lens)


@pytest.mark.parametrize("implicit", [True, False])
@pytest.mark.parametrize("case", sorted(LENGTHS))
def test_bucket1_three_launches_match_the_oracle_per_row(implicit, case):
    _solve_both(case, 128, implicit)


@pytest.mark.parametrize("implicit", [True, False])
@pytest.mark.parametrize("case", ["edges", "many"])
def test_padded_rank_takes_the_wide_kernel_too(implicit, case):
    _solve_both(case, 100, implicit)


def _bucket1_kernel(gbias):
    """name of the kernel that the profile segment of bucket 1 timed (its first launch that has rows) in a solve of the wide_only case"""
    from rsparse_amd import _lib
    lib = _lib.load()
    _lib.check(lib.rsparse_hip_profile_enable(1))
    try:
        _solve_both("wide_only", 128, True, gbias=gbias)
        buf = ctypes.create_string_buffer(8192)
        _lib.check(lib.rsparse_hip_profile_last_names(buf, 8192))
    finally:
        _lib.check(lib.rsparse_hip_profile_enable(0))
    return buf.value.decode().split("\n")[1]


def test_global_bias_keeps_bucket1_on_the_8_wave_kernel():
    """bucket 1 of "wide_only" holds rows of 321..W only: without a global bias its one launch is the 24-quad team kernel, with
    one the 8-wave kernel (GB instantiation) -- and both agree with the oracle, as do the edges under a global bias"""
    assert "als_cgq_kernel<128, 24, 4, 4, 0, true, 0, false, true>" in _bucket1_kernel(0.0)
    assert "als_cgq_kernel<128, 16, 8, 8, 0, true, 0, true, true>" in _bucket1_kernel(0.013)
    _solve_both("edges", 128, True, gbias=0.013)
