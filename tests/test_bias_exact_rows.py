"""The fp32 exact (Cholesky) solver on the BIASED implicit fits, per row.  A BiasTerms pointer -- user/item biases, or a global
bias under solver = "cholesky" -- switches off the normal-equation kernel, the wave-per-row kernel of wrmf_chol_mf.hip and the
low-rank kernel, so every row of every length runs on the older k x k kernels, the only callers that pass rhs_vals / loss_tgt /
rhs_init / loss_tgt_const != 1:

  als_chol2_kernel<128, true, VEC, false>   solve orders 65..128, rows of 0..4096 non-zeros   (wrmf_chol.hip)
  als_chol_wave_kernel<64 | 32, true>       solve orders <= 64, the same rows                 (wrmf_chol_wave.hip)
  als_chol2_kernel<KP, true, VEC, true>     the two-level LONG launch, rows beyond 4096, on a side stream
  wrmf_lu.hip                               the rows these kernels give up

Every comparison is per row against the fp64 oracle on the same fp32 inputs widened, on the solved entries Y[keep]; the
placeholder entry of Y must come back bit-unchanged.

A. Length lattice, regular systems: every chunk / step / fold edge of the three kernel families, empty columns (solved against
   rhs_init), both bias layouts, a global bias with and without user/item biases, confidences below 1; one profiled call per
   family names the kernel and must give the bits of the unprofiled call (whose LONG launch ran on the side stream).
B. A workgroup's second row: the lattice tiled beyond kCholMaxGrid = 24576 columns (main launch) and kCholLongGrid = 512 LONG
   rows; every copy bit-identical to the same column in a launch of the distinct columns alone, the loss additive.
C. Indefinite but regular systems with bias operands, so that every kernel hands rows to the general solver.

The first and the last non-zero of every row of more than two non-zeros carry a heavy confidence (HEAVY_FIRST / HEAVY_LAST): each
parametrisation asserts, on the fp64 oracle alone and BEFORE its device call, that losing the last one moves the row's solution
by at least 10 x 1e-4 -- a dropped chunk tail or fold cannot hide in the bound.

Each test prints its figures (worst err / bound, the fp32 oracle's worst error, the smallest heavy-entry effect, fallback counts,
wall time) before it asserts: profiles/bias_exact_rows/README.md holds them."""
import ctypes
import re
import time

import numpy as np
import pytest

from oracle import wrmf_oracle as O
from rsparse_amd import _lib, als

pytestmark = pytest.mark.gpu
TOL = 1e-4
LAM = 0.1
N_ITEM = 6000
HEAVY_FIRST, HEAVY_LAST = 25.0, 40.0
MIN_EFFECT = 10.0 * TOL
K_CHOL_MAX_GRID, K_CHOL_LONG_GRID, K_CHOL_LONG_LEN = 24576, 512, 4096   # wrmf_internal.h


def _rows_of_lengths(lengths, n_item, k, seed, scale):
    """a CSC (columns = the rows to solve) whose column j has lengths[j] distinct random items, values 1 + Gamma(1, 2)"""
    rng = np.random.default_rng(seed)
    p = np.zeros(len(lengths) + 1, dtype=np.int32)
    p[1:] = np.cumsum(lengths)
    idx = np.concatenate([np.sort(rng.choice(n_item, size=int(n), replace=False)) for n in lengths]).astype(np.int32)
    x = (1.0 + rng.gamma(1.0, 2.0, size=idx.size)).astype(np.float32).astype(np.float64)
    X = np.asfortranarray((rng.standard_normal((k, n_item)) * scale).astype(np.float32))
    Y0 = np.asfortranarray((rng.standard_normal((k, len(lengths))) * scale).astype(np.float32))
    return p, idx, x, X, Y0


def _row_err(Y, Yref):
    return np.linalg.norm(Y - Yref, axis=0) / np.maximum(np.linalg.norm(Yref, axis=0), 1e-30)


def _f64(a):
    return np.asfortranarray(a, dtype=np.float64).copy(order="F")


def _report(tag, **figures):
    print("bias_exact_rows %s %s" % (tag, " ".join("%s=%s" % (n, ("%.3g" % v) if isinstance(v, float) else v)
                                                     for n, v in figures.items())))


def _layout(k, biases, bias_last):
    """-> (the rows of X that stay = the solved entries of Y, the row of X with the x biases, the placeholder entry of Y)"""
    if not biases:
        return slice(0, k), None, None
    return (slice(0, k - 1), k - 1, k - 1) if bias_last else (slice(1, k), 0, 0)


def _set_bias_layout(X, Y0, bias_last):
    """the driver's layout: X = [1, ..., x_bias], Y = [y_bias, ..., 1] (is_x_bias_last_row) or mirrored"""
    k = X.shape[0]
    if bias_last:
        X[0, :] = 1.0
        Y0[k - 1, :] = 1.0
    else:
        X[k - 1, :] = 1.0
        Y0[0, :] = 1.0


def _oracle(q, x, dt):
    """one half-iteration of the oracle in dtype dt on the fp32 inputs of q with the confidences x -> (Y, loss)"""
    X = np.asfortranarray(q["X"], dtype=dt)
    Y = np.asfortranarray(q["Y0"], dtype=dt).copy(order="F")
    if q["G64"] is None:
        G = O.gramian(np.asfortranarray(X[q["keep"]]), LAM)
    else:
        G = np.asfortranarray(q["G64"], dtype=dt)
    loss = O.als_implicit(q["p"], q["i"], x, X, Y, G, LAM, 0, 3, with_biases=q["biases"], is_x_bias_last_row=q["bias_last"],
                          global_bias=q["g"])
    return Y, loss


def _systems_eig(q):
    """float64 eigenvalues of every row's system: (smallest, condition number, number of negative ones)"""
    keep, X64 = q["keep"], _f64(q["X"])
    Xp = X64[keep]
    G = q["G64"] if q["G64"] is not None else O.gramian(np.asfortranarray(Xp), LAM)
    n_cols = len(q["lens"])
    ev_min, cond = np.zeros(n_cols), np.zeros(n_cols)
    p, i, x = q["p"], q["i"], q["x"]
    for c in range(n_cols):
        idx, val = i[p[c]:p[c + 1]], x[p[c]:p[c + 1]]
        ev = np.linalg.eigvalsh(G + (Xp[:, idx] * (val - 1.0)) @ Xp[:, idx].T)
        ev_min[c], cond[c] = ev.min(), np.abs(ev).max() / np.abs(ev).min()
    return ev_min, cond


def _finish(q, sensitivity=True):
    """the fp64 oracle's answer, the fp32 oracle's own error per row and -- for the rows with heavy entries -- how far the fp64
    solution moves when the LAST non-zero's confidence becomes 1.  Everything read-only afterwards: shared between tests."""
    keep = q["keep"]
    Y64, l64 = _oracle(q, q["x"], np.float64)
    Y32, l32 = _oracle(q, q["x"], np.float32)
    q.update(Y64=Y64, l64=l64, l32=l32, e32=_row_err(Y32[keep], Y64[keep]))
    if sensitivity:
        x2 = q["x"].copy()
        heavy = q["lens"] > 2
        x2[q["p"][1:][heavy] - 1] = 1.0
        Yb, _ = _oracle(q, x2, np.float64)
        q["effect"] = _row_err(Yb[keep], Y64[keep])[heavy]
    for a in q.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return q


_cache = {}


def _lattice_problem(tag, lens, rank, biases, g, bias_last=True, below_one=False, seed=0):
    """The common recipe: N_ITEM items, factors N(0, 0.1^2), lambda = 0.1, confidences 1 + Gamma(1, 2) (every ninth 0.3 with
    below_one), the heavy first / last entries; with biases the two rows of ones and an x-bias row ~ N(0, 0.1^2)."""
    key = (tag, rank, biases, g, bias_last, below_one)
    if key not in _cache:
        lens = np.asarray(lens, dtype=np.int64)
        p, i, x, X, Y0 = _rows_of_lengths(lens, N_ITEM, rank, seed=4000 + 7 * rank + seed, scale=0.1)
        if below_one:
            x[::9] = 0.3
        heavy = lens > 2
        x[p[:-1][heavy]] = HEAVY_FIRST
        x[p[1:][heavy] - 1] = HEAVY_LAST
        if biases:
            _set_bias_layout(X, Y0, bias_last)
        keep, xb, fixed = _layout(rank, biases, bias_last)
        q = dict(lens=lens, p=p, i=i, x=x, X=X, Y0=Y0, G64=None, keep=keep, fixed=fixed, biases=biases, bias_last=bias_last, g=g,
                 below_one=below_one)
        _cache[key] = _finish(q)
    return _cache[key]


def _device(q, XtX=None):
    Y = q["Y0"].copy(order="F")
    csc = (N_ITEM, len(q["lens"]), q["p"], q["i"], q["x"])
    loss = als.als_implicit(csc, q["X"], Y, LAM, 1, 0, 3, "float", q["biases"], q["bias_last"], global_bias=q["g"], XtX=XtX)
    return Y, loss


def _profiled(q):
    """the device call with the profile segments on (the LONG launch then runs on the caller's stream): + the kernel names"""
    lib = _lib.load()
    _lib.check(lib.rsparse_hip_profile_enable(1))
    try:
        Y, loss = _device(q)
        buf = ctypes.create_string_buffer(8192)
        _lib.check(lib.rsparse_hip_profile_last_names(buf, 8192))
    finally:
        _lib.check(lib.rsparse_hip_profile_enable(0))
    return Y, loss, buf.value.decode().split("\n")


def _device_layer(q, G32):
    """the same half-iteration through the device-resident layer -> (Y, rows its general solver took, unresolved rows)"""
    import torch
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    n_cols = len(q["lens"])
    h = be.make_csc(N_ITEM, n_cols, be.to_device(np.array(q["p"]), torch.int32), be.to_device(np.array(q["i"]), torch.int32),
                    be.to_device(q["x"].astype(np.float32), torch.float32))
    Xd = be.to_device(np.array(q["X"].T, order="C"), torch.float32)
    Yd = be.to_device(np.array(q["Y0"].T, order="C"), torch.float32)
    Gd = be.to_device(np.array(G32, order="C"), torch.float32)
    lossd = torch.zeros(1, dtype=torch.float64, device=be.device)
    be.half_iteration(h, True, Xd, Yd, Gd, LAM, 0, 3, True, lossd, bias_last_row=q["bias_last"] if q["biases"] else None,
                      global_bias=q["g"])
    bad, fell = be.numeric_counts()
    return Yd.cpu().numpy().T, fell, bad


def _assert_premises(tag, q):
    """from the oracle alone, before the device call: the bound is 1e-4 on (nearly) every row, the heavy last entry is visible,
    the empty columns have a non-zero solution -> the per-row bound"""
    bound = np.maximum(TOL, 3.0 * q["e32"])
    share = float((bound > TOL).mean())
    l32err = abs(q["l32"] - q["l64"]) / abs(q["l64"])
    _report(tag + " premises", oracle32_worst=float(q["e32"].max()), rows_above_tol=share, oracle32_loss_err=float(l32err),
            heavy_last=HEAVY_LAST, effect_min=float(q["effect"].min()) if q["effect"].size else -1.0)
    assert share <= 0.05, share
    assert np.all(q["effect"] >= MIN_EFFECT), (float(q["effect"].min()), int(q["lens"][q["lens"] > 2][q["effect"].argmin()]))
    empty = q["lens"] == 0
    assert np.all(np.linalg.norm(q["Y64"][q["keep"]][:, empty], axis=0) > 0.0)     # solved against rhs_init
    return bound


def _assert_rows_and_loss(tag, q, Y, loss, bound, t0, **more):
    keep, lens = q["keep"], q["lens"]
    err = _row_err(Y[keep], q["Y64"][keep])
    worst = int(np.argmax(err / bound))
    lerr = abs(loss - q["l64"]) / abs(q["l64"])
    _report(tag, worst_ratio=float(err[worst] / bound[worst]), worst_len=int(lens[worst]), err=float(err[worst]),
            oracle32_worst=float(q["e32"].max()), loss_err=float(lerr), wall_s=float(time.perf_counter() - t0), **more)
    assert np.all(np.isfinite(Y)) and np.isfinite(loss)
    if q["fixed"] is not None:
        assert np.array_equal(Y[q["fixed"]], q["Y0"][q["fixed"]])                     # the placeholder entry is never written
    assert np.all(err <= bound), ("row of %d non-zeros" % int(lens[worst]), worst, float(err[worst]), float(q["e32"][worst]))
    assert lerr <= TOL, (loss, q["l64"])


# ---------------------------------------------------------------------------------------------------------------------------
# A. length lattice, regular systems
# ---------------------------------------------------------------------------------------------------------------------------

LENGTHS_A = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2300,
             4095, 4096, 4097, 5000]
KERNEL_OF = {128: "als_chol2_kernel<128, true, ", 64: "als_chol_wave_kernel<64, true>", 32: "als_chol_wave_kernel<32, true>"}
# (kernel family = padded solve order, rank argument, user/item biases, global bias, is_x_bias_last_row, every ninth confidence 0.3)
CASES_A = [
    (128, 128, True, 0.0, True, False),    # order 127 -> 128
    (128, 101, True, 0.0, False, False),   # order 100: k < KP
    (128, 66, True, 0.03, True, False),    # order 65 -> 68
    (128, 128, False, 0.03, True, False),  # the caller's own X, no copy
    (128, 100, False, 0.03, True, False),
    (128, 128, True, 0.0, True, True),
    (64, 65, True, 0.0, True, False),      # order 64 = KP
    (64, 34, True, 0.0, False, False),     # order 33 -> 36
    (64, 64, True, 0.03, True, False),     # order 63 -> 64
    (64, 64, False, 0.03, True, False),
    (64, 36, False, 0.03, True, False),
    (64, 64, True, 0.03, True, True),
    (32, 33, True, 0.0, True, False),      # order 32 = KP
    (32, 5, True, 0.0, False, False),
    (32, 20, True, 0.03, True, False),     # order 19 -> 20
    (32, 32, False, 0.03, True, False),
    (32, 10, False, 0.03, True, False),    # padded to 12, rhs_init padded with it
]


def _lattice_a():
    lens = np.repeat(np.asarray(LENGTHS_A, dtype=np.int64), 2)
    np.random.default_rng(4100).shuffle(lens)
    return lens


def _case_a(rank, biases, g, bias_last, below_one):
    return _lattice_problem("A", _lattice_a(), rank, biases, g, bias_last, below_one, seed=3)


def _tag(name, rank, biases, g, bias_last, below_one=False):
    return "%s rank=%d biases=%d g=%g last=%d below_one=%d" % (name, rank, biases, g, bias_last, below_one)


@pytest.mark.parametrize("family,rank,biases,g,bias_last,below_one", CASES_A)
def test_length_lattice_of_the_biased_exact_kernels(family, rank, biases, g, bias_last, below_one):
    """Rows of 0 .. 5000 non-zeros around every edge of the kernels' loops: als_chol2_kernel's chunks of 32 and (LONG) folds of 4
    chunks, the wave kernel's steps of 16 with a clamped look-ahead (order 33..64) or chunks of 64 (order <= 32), the loss
    passes' chunks, the hand-over to the LONG launch at 4096.  The fp32 oracle stays at or below 5.9e-6 per row on this recipe
    (1.8e-5 with confidences below 1): the bound is 1e-4 on every row.  With confidences below 1 the systems are still positive
    definite (asserted from float64 eigenvalues).  In every cell the general solver must not have been asked, and the
    device-resident layer returns the bits of the stateless call."""
    t0 = time.perf_counter()
    q = _case_a(rank, biases, g, bias_last, below_one)
    tag = _tag("A", rank, biases, g, bias_last, below_one)
    bound = _assert_premises(tag, q)
    more = {}
    if below_one:
        ev_min, cond = _systems_eig(q)
        more.update(ev_min=float(ev_min.min()), cond_max=float(cond.max()))
        assert ev_min.min() > 0.05, float(ev_min.min())
    # (every cell, not only the ones with confidences below 1: a row that the general solver rescued would come back right)
    G32 = O.gramian(np.asfortranarray(q["X"][q["keep"]]), LAM)
    Y, loss = _device(q, XtX=G32)
    Yd, fell, bad = _device_layer(q, G32)
    _assert_rows_and_loss(tag, q, Y, loss, bound, t0, fallback_rows=int(fell), **more)
    assert (fell, bad) == (0, 0)
    assert np.array_equal(Yd, Y)


@pytest.mark.parametrize("family,rank,biases,g", [(128, 128, True, 0.0), (64, 65, True, 0.0), (32, 33, True, 0.0)])
def test_profiled_call_names_the_kernel_and_equals_the_side_stream_call(family, rank, biases, g):
    """The k x k segment of a profiled call names the kernel family of the table.  Profiling puts the LONG launch on the caller's
    stream behind the low-rank segment; the plain call runs it on the side stream between an event fork and join: the same rows,
    the same bits, the same loss."""
    t0 = time.perf_counter()
    q = _case_a(rank, biases, g, True, False)
    assert (q["lens"] > K_CHOL_LONG_LEN).sum() >= 2
    Y, loss = _device(q)
    Yp, lossp, names = _profiled(q)
    kernel = re.search(r"als_chol\w*<[^>]*>", names[2])
    _report("A-profiled rank=%d" % rank, kernel=kernel.group(0) if kernel else names[2], wall_s=float(time.perf_counter() - t0))
    assert KERNEL_OF[family] in names[2], names
    if family == 128:
        assert ", false>" in names[2], names          # the main instantiation names the segment, not LONG
    assert names[0] == "" and names[1] == "" and names[3] == "", names   # no normal-equation, low-rank or wave-per-row launch
    assert np.array_equal(Yp, Y) and lossp == loss
    err = _row_err(Y[q["keep"]], q["Y64"][q["keep"]])
    assert np.all(err <= np.maximum(TOL, 3.0 * q["e32"]))


# ---------------------------------------------------------------------------------------------------------------------------
# B. a workgroup's second row
# ---------------------------------------------------------------------------------------------------------------------------

LENGTHS_B_MAIN = [0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 23, 24, 31, 32, 33, 40, 47, 48, 49, 63, 64, 65, 66, 79, 80, 81, 95, 96, 97,
                  127, 128, 129, 130, 160, 191, 192, 193, 255, 256, 257, 300, 320, 384, 448, 511, 512, 513, 600]
COPIES_MAIN = 512
LENGTHS_B_LONG = [4097, 4224, 4225, 5000]      # 33 folds exactly (4224 = 33 x 128), one entry more, ragged tails
COPIES_LONG = 130


def _tiled(q, copies):
    """q's columns `copies` times over: column j of copy t is column t * n + j"""
    n = len(q["lens"])
    nnz = int(q["p"][-1])
    t = dict(q)
    t["lens"] = np.tile(q["lens"], copies)
    t["p"] = np.concatenate([[0], np.cumsum(t["lens"])]).astype(np.int32)
    t["i"] = np.tile(q["i"], copies)
    t["x"] = np.tile(q["x"], copies)
    t["Y0"] = np.asfortranarray(np.tile(q["Y0"], (1, copies)))
    assert t["p"][-1] == nnz * copies and t["Y0"].shape[1] == n * copies
    return t


def _second_row_case(name, lens, copies, grid, rank, g):
    t0 = time.perf_counter()
    q = _lattice_problem(name, lens, rank, True, g, True, False, seed=1)
    tag = _tag(name, rank, True, g, True) + " copies=%d" % copies
    bound = _assert_premises(tag, q)
    n = len(lens)
    assert n * copies > grid                                  # some workgroup takes a second row
    Y1, loss1 = _device(q)
    _assert_rows_and_loss(tag + " distinct", q, Y1, loss1, bound, t0)
    big = _tiled(q, copies)
    Yc, lossc = _device(big)
    Y2, loss2 = _device(_tiled(q, 2))
    same = np.array([np.array_equal(Yc[:, c], Y1[:, c % n]) for c in range(n * copies)])
    # loss * nnz = the rows' terms + lambda |X'|^2, the second the same in every call: the rows' terms of one copy are the
    # difference between the launches of two copies and of one
    nnz = float(q["p"][-1])
    L1, L2, Lc = loss1 * nnz, loss2 * 2 * nnz, lossc * copies * nnz
    rows = L2 - L1
    off = abs((Lc - L1) - (copies - 1) * rows) / ((copies - 1) * abs(rows))
    _report(tag + " tiled", columns=n * copies, second_rows=n * copies - grid, copies_differing=int((~same).sum()),
            loss_additivity=float(off), wall_s=float(time.perf_counter() - t0))
    assert rows > 0
    assert same.all(), ("first differing column", int(np.argmin(same)), int(big["lens"][np.argmin(same)]))
    assert np.array_equal(Y2, np.tile(Y1, (1, 2)))
    assert off <= 1e-9, (Lc, L1, L2)


@pytest.mark.parametrize("copies", [COPIES_MAIN, 560])
@pytest.mark.parametrize("rank", [128, 64, 20])
def test_second_row_of_a_workgroup_main_launch(rank, copies):
    """49 distinct columns of 0 .. 600 non-zeros (every chunk / step edge up to 512), 512 copies: 25088 columns > the grid of
    24576.  The launch walks the length-sorted order, so those 512 second rows are the empty columns (solved against rhs_init);
    with 560 copies the 2864 second rows are the columns of 0 .. 4 non-zeros and some of 7: a second row that assembles.  Every
    copy must be bit-identical to its column in the launch of the 49 alone -- a row must not see its workgroup's earlier row."""
    assert len(LENGTHS_B_MAIN) == 49 and len(set(LENGTHS_B_MAIN)) == 49
    _second_row_case("B-main", LENGTHS_B_MAIN, copies, K_CHOL_MAX_GRID, rank, 0.0)


@pytest.mark.parametrize("rank", [128, 33])
def test_second_row_of_a_workgroup_long_launch(rank):
    """4 distinct rows beyond 4096 non-zeros, 130 copies: 520 rows > the LONG grid of 512; its second rows are eight of the
    4097-rows behind eight of the 5000-rows (look-ahead of the row id two strides ahead, the fold counter and the second
    register block start again)."""
    _second_row_case("B-long", LENGTHS_B_LONG, COPIES_LONG, K_CHOL_LONG_GRID, rank, 0.03)


# ---------------------------------------------------------------------------------------------------------------------------
# C. rows handed to the general solver with bias operands
# ---------------------------------------------------------------------------------------------------------------------------

LENGTHS_C = [20, 40, 64, 65, 128, 300, 512, 513, 900, 2300, 4096, 4097, 5000]
GRAM_FACTOR = 0.001
SEED_C = {128: 0, 65: 0, 33: 0, 20: 0}
# The ranks at which the loss condition of case C holds (3 x the fp32 oracle's loss error below half of the smallest row's loss
# term).  None: the rows of 20 non-zeros stand beside rows of 5000 and beside indefinite rows whose solutions are large, so the
# smallest term is 2e-8 .. 4e-5 of the sum over six seeds per rank, and already the 1e-4 floor of the loss bound asks for
# 2e-4 (profiles/bias_exact_rows/README.md has the figures).  At these ranks the exact fallback count is the guard that every
# row's term has one owner.
LOSS_GUARD_RANKS = ()


def _indefinite_problem(rank, mixed, g):
    """Four rows of each length of LENGTHS_C; factors N(0, 0.3^2), G = 0.001 X' X'^T + 0.1 I passed as XtX (X' = X without its
    x-bias row), confidences 0.25 with probability 0.8, else 3.0: c - 1 = -0.75 against a Gramian that does not dominate it.
    `mixed`: every other row keeps 1 + Gamma(1, 2) and stays positive definite."""
    key = ("C", rank, mixed, g)
    if key not in _cache:
        lens = np.repeat(np.asarray(LENGTHS_C, dtype=np.int64), 4)
        seed = 7000 + 13 * rank + mixed + 1000 * SEED_C[rank]
        p, i, x, X, Y0 = _rows_of_lengths(lens, N_ITEM, rank, seed=seed, scale=0.3)
        _set_bias_layout(X, Y0, True)
        rng = np.random.default_rng(seed + 100)
        xi = np.where(rng.random(x.size) < 0.8, 0.25, 3.0)
        indef = np.ones(len(lens), dtype=bool)
        if mixed:
            indef[1::2] = False
        x = np.where(np.repeat(indef, lens), xi, x)
        keep, xb, fixed = _layout(rank, True, True)
        Xp = _f64(X)[keep]
        G = np.asfortranarray(GRAM_FACTOR * (Xp @ Xp.T) + LAM * np.eye(rank - 1))
        q = dict(lens=lens, p=p, i=i, x=x, X=X, Y0=Y0, G64=G, keep=keep, fixed=fixed, biases=True, bias_last=True, g=g,
                 indef=indef)
        q["ev_min"], q["cond"] = _systems_eig(q)
        _finish(q, sensitivity=False)
        # the rows' loss terms in numpy: sum_j c_j ((1 - g) - y . x'_j - b_j)^2 + lambda |y|^2
        X64, terms = _f64(X), np.zeros(len(lens))
        for c in range(len(lens)):
            idx, val = i[p[c]:p[c + 1]], x[p[c]:p[c + 1]]
            y = q["Y64"][keep, c]
            terms[c] = np.sum(val * ((1.0 - g) - y @ Xp[:, idx] - X64[xb, idx]) ** 2) + LAM * (y @ y)
        terms.setflags(write=False)
        q["terms"] = terms
        q["reg"] = LAM * float(np.sum(X64[1:] ** 2))          # every row of X but the ones
        _cache[key] = q
    return _cache[key]


@pytest.mark.parametrize("rank,mixed,g", [(128, False, 0.03), (128, True, 0.0), (65, False, 0.0), (65, True, 0.03),
                                          (33, False, 0.03), (33, True, 0.0), (20, False, 0.0), (20, True, 0.03)])
def test_biased_rows_handed_to_the_general_solver(rank, mixed, g):
    """Every kernel of the table above gives up its indefinite rows (a non-positive pivot) and wrmf_lu.hip re-solves them with
    rhs_vals / rhs_init and owns their loss terms (loss_tgt): per row the bound of test_exact_solver_classes.py case B, fp32
    elimination ~ cond x eps; the rows that stay positive definite meet 1e-4.  The fallback count is exact.  The loss would have
    no escape if 3 x the fp32 oracle's loss error stayed below half of the smallest row's term (computed here from the oracle
    alone and printed as loss_bound_over_smallest_term; asserted at LOSS_GUARD_RANKS): on this recipe it holds at no rank, so
    the exact count is what says that each row's term has one owner, and the loss bound catches the long rows only."""
    t0 = time.perf_counter()
    q = _indefinite_problem(rank, mixed, g)
    lens, indef, cond = q["lens"], q["indef"], q["cond"]
    tag = "C rank=%d mixed=%d g=%g" % (rank, mixed, g)
    nnz = float(q["p"][-1])
    l32err = abs(q["l32"] - q["l64"]) / abs(q["l64"])
    loss_bound = max(TOL, 3.0 * l32err)
    guard = loss_bound * abs(q["l64"]) * nnz / q["terms"].min()
    _report(tag + " premises", ev_min_indef_max=float(q["ev_min"][indef].max()),
            ev_min_def_min=float(q["ev_min"][~indef].min()) if mixed else 0.0, cond_max=float(cond[indef].max()),
            oracle32_worst_over_cond_eps=float((q["e32"] / (cond * 6e-8))[indef].max()),
            oracle32_worst_definite=float(q["e32"][~indef].max()) if mixed else 0.0, oracle32_loss_err=float(l32err),
            loss_bound_over_smallest_term=float(guard))
    assert abs((q["terms"].sum() + q["reg"]) / nnz - q["l64"]) <= 1e-9 * abs(q["l64"])   # the numpy terms are the oracle's
    assert np.all(q["ev_min"][indef] < -1.0), float(q["ev_min"][indef].max())
    assert np.all(q["ev_min"][~indef] > 0.05)
    if rank in LOSS_GUARD_RANKS:
        assert guard < 0.5, guard
    G32 = np.asfortranarray(q["G64"], dtype=np.float32)
    Y, loss = _device(q, XtX=G32)
    Yd, fell, bad = _device_layer(q, G32)
    keep = q["keep"]
    err = _row_err(Y[keep], q["Y64"][keep])
    bound = np.where(indef, np.maximum(TOL, 20.0 * cond * 6e-8), TOL)
    worst = int(np.argmax(err / bound))
    lerr = abs(loss - q["l64"]) / abs(q["l64"])
    _report(tag, worst_ratio=float(err[worst] / bound[worst]), worst_len=int(lens[worst]), err=float(err[worst]),
            fallback_rows=int(fell), indefinite_rows=int(indef.sum()), loss_err=float(lerr), loss_bound=float(loss_bound),
            wall_s=float(time.perf_counter() - t0))
    assert not np.isnan(Y).any() and np.isfinite(loss)
    assert np.array_equal(Y[q["fixed"]], q["Y0"][q["fixed"]])
    assert np.all(err <= bound), ("row of %d non-zeros" % int(lens[worst]), bool(indef[worst]), float(err[worst]), float(cond[worst]))
    assert lerr <= loss_bound, (loss, q["l64"], q["l32"])
    assert fell == int(indef.sum()) and bad == 0, (fell, bad, int(indef.sum()))
    assert np.array_equal(Yd, Y)
