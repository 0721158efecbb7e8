"""The one-wave-per-row conjugate-gradient kernel (wrmf_cg_mf.hip: rank 128, implicit feedback, rows of 513..16384 non-zeros)
between a wave's rows: what a row leaves behind -- the accumulator tiles (raw since the unscale pass went: the powers of two are
applied where the solve and the loss form read an entry), the ring and metadata slots, the operand ping-pong, the warm-start
buffer -- and what the next row on the wave finds.  (The cases are those a prefetch of the next row in front of the solve was
built and measured against, tools/probes/cg_mf_next_row_in_front_of_solve.patch; they hold for any form of the row switch.)
Every row against the fp64 oracle at the tolerance tests/test_hip_parity.py holds the same kernel's rows to, the loss of every
case against the oracle's, 3 CG steps, about 2000 source vectors.

Row lengths 513, 514, 527, 528, 529, 544, 575, 576 and 1040: 33, 34, 36 and 65 steps of 16 non-zeros (both parities of the
operand ping-pong; 9, 10 and 17 chunks of 64 indices), tails of 0, 1 and 15 mod 16.

Rows per wave.  The launcher (cg_mf_grid) starts min(ceil(rows / 4), 4096) workgroups of four waves, and wave w takes the rows
w, w + 4 grid, ... of the list, which is ordered longest first (ties in row order).  So up to 16 384 rows every wave has at most
one; THREE_PER_WAVE = 3 * 16 384 = 49 152 rows give every one of the 16 384 waves exactly three, and with a third of the rows at
each of 576, 527 and 513 non-zeros wave w solves a row of 576 (36 steps, tail 0), then one of 527 (33 steps, tail 15), then one
of 513 (33 steps, tail 1): consecutive rows that differ in length, in step parity and in tail.  81 920 rows give every wave five
rows.  40 140 rows of all nine lengths put the seams between the lengths inside the waves' turns.  26 rows give
26 of the 28 waves of seven workgroups one row and two none; 9 rows the same with three idle waves.

The same rows with some confidences below 1 go through the `_any` instantiation, and one case starts from a warm start of zero.
(The rows' items are not sorted within a row: the kernels and the oracle sum over a row's non-zeros in the order given.)

The long lists are a block of a few hundred different rows repeated: the device solves every copy on a wave and in a turn of its
own and every copy is compared, the oracle solves the block once (ten seconds otherwise).  Its loss for the whole list follows
from the block's -- sum of the rows' terms + lambda |X|^2, over the non-zeros --, which a host test checks against the oracle run
on a repeated block."""
import numpy as np
import pytest

from oracle import wrmf_oracle as O
from rsparse_amd import als
from test_hip_parity import TOL   # the tolerance of test_cg_wave_per_row_kernel_every_row_length_class: rows and loss

gpu = pytest.mark.gpu
K = 128
N_ITEM = 2003            # prime: (start + stride * t) mod N_ITEM, t < length <= N_ITEM, are distinct for every stride
LENGTHS = [513, 514, 527, 528, 529, 544, 575, 576, 1040]
WAVES = 4 * 4096         # cg_mf_grid's ceiling, four waves per workgroup
THREE_PER_WAVE = 3 * WAVES


def _rows(lengths, seed, below_one=False, zero_start=False):
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    p = np.zeros(len(lengths) + 1, dtype=np.int32)
    p[1:] = np.cumsum(lengths)
    row = np.repeat(np.arange(len(lengths)), lengths)
    t = np.arange(int(p[-1]), dtype=np.int64) - p[:-1].astype(np.int64)[row]
    start, stride = rng.integers(0, N_ITEM, size=len(lengths)), rng.integers(1, N_ITEM, size=len(lengths))
    idx = ((start[row] + stride[row] * t) % N_ITEM).astype(np.int32)
    x = 1.0 + rng.geometric(0.5, size=idx.size).astype(np.float64)
    if below_one:
        x[::9] = 0.3
    X = np.asfortranarray((rng.standard_normal((K, N_ITEM)) * 0.05).astype(np.float32))
    Y0 = np.asfortranarray((rng.standard_normal((K, len(lengths))) * 0.05).astype(np.float32))
    if zero_start:
        Y0[:] = 0.0
    return (N_ITEM, len(lengths), p, idx, x), X, Y0


def _oracle(csc, X, Y0, lam):
    _, _, p, i, x = csc
    X64 = np.asfortranarray(X, dtype=np.float64)
    Yref = np.asfortranarray(Y0, dtype=np.float64).copy(order="F")
    lref = O.als_implicit(p, i, x, X64, Yref, O.gramian(X64, lam), lam, 1, 3, n_threads=16)
    return Yref, lref


def _repeat(csc, Y0, copies):
    """the list `copies` times over: copy c of row j is row c * rows + j"""
    n_item, n, p, i, x = csc
    lens = np.tile(np.diff(p), copies)
    pp = np.zeros(len(lens) + 1, dtype=np.int32)
    pp[1:] = np.cumsum(lens)
    return (n_item, n * copies, pp, np.tile(i, copies), np.tile(x, copies)), np.asfortranarray(np.tile(Y0, (1, copies)))


def _repeated_loss(lref, nnz, X, lam, copies):
    """the oracle's loss (per non-zero) of the list repeated, from its loss of the list"""
    fixed = lam * float((X.astype(np.float64) ** 2).sum())
    return (copies * (lref * nnz - fixed) + fixed) / (copies * nnz)


def _check(lengths, seed, copies=1, **kw):
    csc, X, Y0 = _rows(lengths, seed, **kw)
    lam = 0.1
    Yref, lref = _oracle(csc, X, Y0, lam)
    if copies > 1:
        lref = _repeated_loss(lref, int(csc[2][-1]), X, lam, copies)
        csc, Y0 = _repeat(csc, Y0, copies)
        Yref = np.tile(Yref, (1, copies))
    lens = np.diff(csc[2])
    Y = Y0.copy(order="F")
    loss = als.als_implicit(csc, X, Y, lam, 1, 1, 3, "float", False, False)
    err = np.linalg.norm(Y - Yref, axis=0) / np.maximum(np.linalg.norm(Yref, axis=0), 1e-30)
    bad = int(err.argmax())
    print("rows %d  worst row %.3g (%d non-zeros, row %d)  loss rel %.3g"
          % (len(lens), err.max(), int(lens[bad]), bad, abs(loss - lref) / abs(lref)))
    assert np.isfinite(Y).all()
    assert err.max() < TOL, (bad, int(lens[bad]), float(err.max()))
    assert abs(loss - lref) <= TOL * abs(lref), (loss, lref)


def test_the_loss_of_a_repeated_list_follows_from_the_lists():
    csc, X, Y0 = _rows(np.asarray(LENGTHS), seed=3)
    _, lref = _oracle(csc, X, Y0, 0.1)
    csc3, Y03 = _repeat(csc, Y0, 3)
    Y3, lref3 = _oracle(csc3, X, Y03, 0.1)
    assert abs(_repeated_loss(lref, int(csc[2][-1]), X, 0.1, 3) - lref3) <= 1e-12 * abs(lref3)
    assert np.array_equal(Y3[:, :9], Y3[:, 18:])


@gpu
@pytest.mark.parametrize("below_one", [False, True])
def test_one_row_per_wave_some_waves_none(below_one):
    """26 rows on seven workgroups (28 waves): every length about three times, two waves idle; 9 rows: three idle waves"""
    _check(np.asarray((LENGTHS * 3)[:26]), seed=11 + below_one, below_one=below_one)
    _check(np.asarray(LENGTHS), seed=13 + below_one, below_one=below_one)


@gpu
@pytest.mark.parametrize("below_one", [False, True])
def test_three_rows_per_wave_that_differ_in_length_parity_and_tail(below_one):
    """49 152 rows: every wave takes a row of 576, one of 527 and one of 513 non-zeros, in that order (192 different rows, 256
    times: ordered by length on the device, the copies of one row spread over 256 waves)"""
    lengths = np.repeat([576, 527, 513], 64)
    np.random.default_rng(5).shuffle(lengths)   # (the row ids are mixed, not the waves' turns)
    assert len(lengths) * 256 == THREE_PER_WAVE
    _check(lengths, seed=17 + below_one, copies=256, below_one=below_one)


@gpu
@pytest.mark.parametrize("below_one", [False, True])
def test_two_and_three_rows_per_wave_of_every_length(below_one):
    """40 140 rows of the nine lengths in equal shares (180 different rows, 223 times), longest first on the device: the first
    7372 waves take three rows, the others two, and the seams between the lengths fall inside the waves' turns (a row of 1040
    before one of 576 or 575, 544 before 528, ...)"""
    _check(np.asarray(LENGTHS * 20), seed=23 + below_one, copies=223, below_one=below_one)


@gpu
def test_five_rows_per_wave():
    """81 920 rows: every wave takes rows of 576, 544, 529, 527 and 513 non-zeros (36, 34, 34, 33, 33 steps), so the metadata
    slot a row ends in differs from row to row (160 different rows, 512 times)"""
    lengths = np.repeat([576, 544, 529, 527, 513], 32)
    assert len(lengths) * 512 == 5 * WAVES
    _check(lengths, seed=29, copies=512)


@gpu
def test_warm_start_of_zero():
    _check(np.asarray((LENGTHS * 3)[:26]), seed=31, zero_start=True)
