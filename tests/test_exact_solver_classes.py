"""The exact (Cholesky) solver above rank 64, on the three paths that tests/test_hip_parity.py leaves out.  Every comparison is
per row against the fp64 oracle on the same fp32 inputs.

A. lambda = 0, explicit feedback: zero_padding_is_neutral() turns the padding off, the half-iteration runs at the TRUE rank.
   Ranks 68 / 100 / 124: rows of 65..512 ratings on rsparse_hip_als_chol_mf_explicit_padded (masked coordinates, the `vec` loss
   pass), longer ones on the exact solve of wrmf_ne.hip at a rank below its padded rank, shorter ones on the k x k kernel.
   Rank 128: the full wave-per-row kernel with nothing on its diagonal; no push-through kernel for the short rows.  Ranks 101 /
   127 and a biased fit of rank 102 (solves at 101): every row on launch_als_chol2 at an odd rank under the padded rank 128.
B. Indefinite but regular systems in every row-length class, so that EVERY Cholesky kernel hands rows to the general solver
   (wrmf_lu.hip): the `bad` path of wrmf_chol_mf.hip, the fail_rows append of wrmf_ne.hip (split rows included), the
   padded-to-128 route (rank 100) whose trailing block is the identity -- and the loss, which each row must enter exactly once.
C. Row-length lattice of the wave-per-row kernel (wrmf_chol_mf.hip, rank 128): steps of 16 non-zeros with a look-ahead fetch
   whose last step is clamped, loss pass in chunks of 64 -- every length 65..129 and 495..514, for the three instantiations the
   dispatch reaches at rank 128 (implicit, implicit with a confidence below 1, explicit).

Each test prints its figures (worst err / bound, the fp32 oracle's worst error, fallback counts) before it asserts:
profiles/exact_solver_tests/README.md holds them."""
import warnings

import numpy as np
import pytest

from conftest import rel_fro
from oracle import wrmf_oracle as O
from rsparse_amd import _lib, als

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _rows_of_lengths(lengths, n_item, k, seed, scale):
    """a CSC (columns = the rows to solve) whose column j has lengths[j] distinct random items, values >= 1"""
    rng = np.random.default_rng(seed)
    p = np.zeros(len(lengths) + 1, dtype=np.int32)
    p[1:] = np.cumsum(lengths)
    idx = np.concatenate([np.sort(rng.choice(n_item, size=int(n), replace=False)) for n in lengths]).astype(np.int32)
    x = (1.0 + rng.gamma(1.0, 2.0, size=idx.size)).astype(np.float32).astype(np.float64)
    X = np.asfortranarray((rng.standard_normal((k, n_item)) * scale).astype(np.float32))
    Y0 = np.asfortranarray((rng.standard_normal((k, len(lengths))) * scale).astype(np.float32))
    return (n_item, len(lengths), p, idx, x), X, Y0


def _row_err(Y, Yref):
    return np.linalg.norm(Y - Yref, axis=0) / np.maximum(np.linalg.norm(Yref, axis=0), 1e-30)


def _f64(a):
    return np.asfortranarray(a, dtype=np.float64).copy(order="F")


def _report(tag, **figures):
    print("exact_solver_classes %s %s" % (tag, " ".join("%s=%s" % (n, ("%.3g" % v) if isinstance(v, float) else v)
                                                          for n, v in figures.items())))


# ---------------------------------------------------------------------------------------------------------------------------
# A. lambda = 0, explicit feedback, true rank
# ---------------------------------------------------------------------------------------------------------------------------

LONG_A = [497, 505, 511, 512, 513, 514, 528, 700, 1100, 2300, 4095, 4096, 4097]
N_ITEM_A = 6000
_cache_a = {}


def _lambda_zero_problem(k, with_biases):
    """ratings 1..5, factors N(0, 0.4^2); rows of k + 8 .. k + 71 ratings (every residue mod 16 and mod 64, both step parities)
    and LONG_A: more ratings than factors everywhere, so every system is regular.  With the fp64 oracle's answer and the fp32
    oracle's own error per row -- computed once per (rank, bias) and shared."""
    if (k, with_biases) not in _cache_a:
        lens = np.asarray(list(range(k + 8, k + 72)) + LONG_A, dtype=np.int64)
        (n_item, n_cols, p, i, x), X, Y0 = _rows_of_lengths(lens, N_ITEM_A, k, seed=9000 + k, scale=0.4)
        x = np.random.default_rng(9100 + k).integers(1, 6, x.size).astype(np.float64)
        if with_biases:                      # the layout of the driver: ones in the first row of X, the x biases in the last
            X[0, :] = 1.0
            Y0[-1, :] = 1.0
        cnt = np.bincount(i, minlength=n_item).astype(np.float64)
        Y64 = _f64(Y0)
        l64 = O.als_explicit(p, i, x, _f64(X), Y64, cnt, 0.0, 0, 3, False, with_biases=with_biases, is_x_bias_last_row=True)
        Y32 = Y0.copy(order="F")
        l32 = O.als_explicit(p, i, x, X, Y32, cnt.astype(np.float32), 0.0, 0, 3, False, with_biases=with_biases,
                             is_x_bias_last_row=True)
        for a in (p, i, x, X, Y0, Y64, cnt):
            a.setflags(write=False)
        _cache_a[(k, with_biases)] = dict(lens=lens, p=p, i=i, x=x, X=X, Y0=Y0, cnt=cnt, Y64=Y64, l64=l64,
                                          e32=_row_err(Y32, Y64), l32=l32)
    return _cache_a[(k, with_biases)]


def _assert_rows_and_loss(tag, lens, Y, loss, Y64, l64, e32, l32):
    """the project's rule for unregularised systems, per row: err <= max(1e-4, 3 x the fp32 oracle's error on that row)"""
    err = _row_err(Y, Y64)
    bound = np.maximum(TOL, 3.0 * e32)
    worst = int(np.argmax(err / bound))
    lerr, l32err = abs(loss - l64) / abs(l64), abs(l32 - l64) / abs(l64)
    _report(tag, worst_ratio=float(err[worst] / bound[worst]), worst_len=int(lens[worst]), err=float(err[worst]),
            oracle32_worst=float(e32.max()), loss_err=float(lerr), oracle32_loss_err=float(l32err))
    assert np.all(np.isfinite(Y))
    assert np.all(err <= bound), ("row of %d ratings" % int(lens[worst]), worst, float(err[worst]), float(e32[worst]))
    assert lerr <= max(TOL, 3.0 * l32err), (loss, l64, l32)


@pytest.mark.parametrize("k,with_biases", [(68, False), (100, False), (124, False), (128, False), (101, False), (127, False),
                                           (102, True)])
def test_explicit_lambda_zero_above_rank_64_keeps_the_true_rank(k, with_biases):
    """lambda = 0 is the reference's default.  The fp32 oracle stays at or below 5.5e-5 per row on this recipe (the worst rows
    are the ones just above k ratings, condition number about 3e3; rows beyond 512 sit near 2e-6), so the bound is 1e-4 .. 2e-4
    everywhere and a wrong tail step cannot hide in it."""
    q = _lambda_zero_problem(k, with_biases)
    csc = (N_ITEM_A, len(q["lens"]), q["p"], q["i"], q["x"])
    Y = q["Y0"].copy(order="F")
    loss = als.als_explicit(csc, q["X"], Y, q["cnt"].astype(np.float32), 0.0, 1, 0, 3, False, "float", with_biases, True)
    _assert_rows_and_loss("A k=%d bias=%d" % (k, with_biases), q["lens"], Y, loss, q["Y64"], q["l64"], q["e32"], q["l32"])


@pytest.mark.parametrize("k", [100, 128])
def test_explicit_lambda_zero_with_a_few_singular_rows(k):
    """The same matrix plus five rows of fewer ratings than factors (lhs = X_nnz X_nnz^T is singular), one for each kernel that
    can meet them: 1 / 30 / 64 ratings (the k x k kernel), 65 and 3 k / 4 (the wave-per-row kernel).  No row closer to k: the
    non-zero part of the spectrum of a k x n Gaussian matrix closes in on zero as n -> k, and "reproduces the ratings" then asks
    fp32 for digits it does not have (the existing contract stops at 12 of 16 for the same reason).  The contract of
    test_singular_systems_are_an_error_or_a_consistent_solution: ERR_NUMERIC with "singular", or finite output that reproduces
    those rows' ratings -- and then the regular rows are what they are without the singular ones --; the library stays usable."""
    q = _lambda_zero_problem(k, False)
    short = np.asarray([1, 30, 64, 65, 3 * k // 4], dtype=np.int64)
    rng = np.random.default_rng(9200 + k)
    n_reg = len(q["lens"])
    lens = np.concatenate([q["lens"], short])
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    i = np.concatenate([q["i"]] + [np.sort(rng.choice(N_ITEM_A, size=int(n), replace=False)) for n in short]).astype(np.int32)
    x = np.concatenate([q["x"], rng.integers(1, 6, int(short.sum())).astype(np.float64)])
    Y0 = np.asfortranarray(np.concatenate([q["Y0"], (rng.standard_normal((k, short.size)) * 0.4).astype(np.float32)], axis=1))
    csc = (N_ITEM_A, len(lens), p, i, x)
    Y = Y0.copy(order="F")
    try:
        als.als_explicit(csc, q["X"], Y, None, 0.0, 1, 0, 3, False, "float", False, False)
        outcome = "solved"
        assert np.all(np.isfinite(Y))
        for c in range(n_reg, len(lens)):
            idx, val = i[p[c]:p[c + 1]], x[p[c]:p[c + 1]]
            res = np.linalg.norm(val - Y[:, c].astype(np.float64) @ q["X"][:, idx].astype(np.float64))
            assert res <= 5e-2 * np.linalg.norm(val), ("row of %d ratings" % int(lens[c]), float(res))
        err = _row_err(Y[:, :n_reg], q["Y64"])
        bound = np.maximum(TOL, 3.0 * q["e32"])
        worst = int(np.argmax(err / bound))
        assert np.all(err <= bound), ("row of %d ratings" % int(lens[worst]), float(err[worst]), float(q["e32"][worst]))
    except _lib.RsparseHipError as e:
        outcome = "error"
        assert e.code == _lib.ERR_NUMERIC and "singular" in str(e)
    _report("A-singular k=%d" % k, outcome=outcome)
    Y2 = Y0.copy(order="F")
    als.als_explicit(csc, q["X"], Y2, None, 0.1, 1, 0, 3, False, "float", False, False)
    assert np.all(np.isfinite(Y2))


# ---------------------------------------------------------------------------------------------------------------------------
# B. indefinite but regular systems in every row-length class
# ---------------------------------------------------------------------------------------------------------------------------

LENGTHS_B = [20, 40, 64, 65, 80, 100, 128, 200, 300, 400, 511, 512, 513, 600, 900, 1500, 2300]
N_ITEM_B = 3000
_cache_b = {}


def _indefinite_problem(k, mixed):
    """Six rows of each length of LENGTHS_B; X ~ N(0, 0.3^2), G = 0.01 X X^T + 0.1 I passed as XtX, confidences 0.25 with
    probability 0.8, else 3.0: c - 1 = -0.75 against a Gramian that does not dominate it.  `mixed`: every other row keeps
    confidences 1 + gamma instead (positive definite).  With the float64 eigenvalues of every system, the fp64 oracle's answer
    and the fp32 oracle's loss -- computed once per (rank, mixed) and shared."""
    if (k, mixed) not in _cache_b:
        lens = np.repeat(np.asarray(LENGTHS_B, dtype=np.int64), 6)
        (n_item, n_cols, p, i, x), X, Y0 = _rows_of_lengths(lens, N_ITEM_B, k, seed=7000 + k + mixed, scale=0.3)
        rng = np.random.default_rng(7100 + k + mixed)
        xi = np.where(rng.random(x.size) < 0.8, 0.25, 3.0)
        indef = np.ones(n_cols, dtype=bool)
        if mixed:
            indef[1::2] = False
        x = np.where(np.repeat(indef, lens), xi, x)
        X64 = _f64(X)
        G = np.asfortranarray(0.01 * (X64 @ X64.T) + 0.1 * np.eye(k))
        ev_min, cond = np.zeros(n_cols), np.zeros(n_cols)
        n_neg = np.zeros(n_cols, dtype=np.int64)
        for c in range(n_cols):
            idx, val = i[p[c]:p[c + 1]], x[p[c]:p[c + 1]]
            ev = np.linalg.eigvalsh(G + (X64[:, idx] * (val - 1.0)) @ X64[:, idx].T)
            ev_min[c], n_neg[c], cond[c] = ev.min(), (ev < 0).sum(), np.abs(ev).max() / np.abs(ev).min()
        Y64 = _f64(Y0)
        l64 = O.als_implicit(p, i, x, X64, Y64, G, 0.1, 0, 3)
        G32 = np.asfortranarray(G, dtype=np.float32)
        Y32 = Y0.copy(order="F")
        l32 = O.als_implicit(p, i, x, X, Y32, G32, 0.1, 0, 3)
        for a in (p, i, x, X, Y0, Y64, G32):
            a.setflags(write=False)
        _cache_b[(k, mixed)] = dict(lens=lens, p=p, i=i, x=x, X=X, Y0=Y0, G32=G32, indef=indef, ev_min=ev_min, n_neg=n_neg,
                                    cond=cond, Y64=Y64, l64=l64, e32=_row_err(Y32, Y64), l32=l32)
    return _cache_b[(k, mixed)]


@pytest.mark.parametrize("k", [128, 100, 64])
@pytest.mark.parametrize("mixed", [False, True])
def test_every_cholesky_kernel_hands_indefinite_rows_to_the_general_solver(k, mixed):
    """Rank 128: the k x k kernel (<= 64 non-zeros; the low-rank kernel stands down for a confidence below 1), the wave-per-row
    kernel's `bad` path (65..512) and the fail_rows append of the normal-equation kernel's exact solve (> 512, the rows of 1500 and
    2300 split across workgroups).  Rank 100: the same on copies padded to 128 -- wrmf_lu.hip eliminates a system whose trailing
    block is the identity.  Rank 64: the wave-per-row kernel of that rank and the normal-equation kernel.
    Per row the bound of test_cholesky_falls_back_to_the_general_solver, fp32 elimination ~ cond x eps (the fp32 oracle sits at or
    below 5.8 x cond x 6e-8 on this kind of input, cond 1e2 .. 2e5); the loss WITHOUT an escape: a row's term is owned by the
    fallback when the Cholesky kernel gave the row up and by that kernel otherwise -- counted twice or not at all, the sum is off by
    a row's share.  (The yardstick is the fp32 oracle's own loss error, which the worst conditioned row sets: 1e-4 .. 1e-3 at
    ranks 64 and 100, 8e-3 at rank 128 unmixed, against a mean share of 1 / 100 per row.)  `mixed`: half of the rows are positive definite and stay with their
    Cholesky launch, which then owns the loss term of some of its rows and not of others; those rows meet 1e-4."""
    import torch
    from rsparse_amd.engine import HipBackend
    q = _indefinite_problem(k, mixed)
    lens, indef, cond = q["lens"], q["indef"], q["cond"]
    n_cols = len(lens)
    # the premise, from float64 eigenvalues: every row meant to be indefinite is so by a margin no fp32 rounding closes, the
    # others are positive definite
    assert np.all(q["ev_min"][indef] < -1.0), (int(lens[indef][np.argmax(q["ev_min"][indef])]), float(q["ev_min"][indef].max()))
    assert np.all(q["ev_min"][~indef] > 0.05)
    csc = (N_ITEM_B, n_cols, q["p"], q["i"], q["x"])
    Y = q["Y0"].copy(order="F")
    loss = als.als_implicit(csc, q["X"], Y, 0.1, 1, 0, 3, "float", False, False, XtX=q["G32"])   # no error: the rows were re-solved
    err = _row_err(Y, q["Y64"])
    bound = np.where(indef, np.maximum(TOL, 20.0 * cond * 6e-8), TOL)
    worst = int(np.argmax(err / bound))
    lerr, l32err = abs(loss - q["l64"]) / abs(q["l64"]), abs(q["l32"] - q["l64"]) / abs(q["l64"])
    # the device-resident layer reports the count like the reference's warning
    be = HipBackend()
    h = be.make_csc(N_ITEM_B, n_cols, be.to_device(np.array(q["p"]), torch.int32), be.to_device(np.array(q["i"]), torch.int32),
                    be.to_device(q["x"].astype(np.float32), torch.float32))
    Xd = be.to_device(np.array(q["X"].T, order="C"), torch.float32)
    Yd = be.to_device(np.array(q["Y0"].T, order="C"), torch.float32)
    Gd = be.to_device(np.array(q["G32"], order="C"), torch.float32)
    lossd = torch.zeros(1, dtype=torch.float64, device=be.device)
    be.half_iteration(h, True, Xd, Yd, Gd, 0.1, 0, 3, True, lossd)
    with pytest.warns(RuntimeWarning, match="general"):
        be.check_numeric()
    fell = be.last_fallback_rows
    _report("B k=%d mixed=%d" % (k, mixed), worst_ratio=float(err[worst] / bound[worst]), worst_len=int(lens[worst]),
            err=float(err[worst]), cond_max=float(cond[indef].max()), oracle32_worst_over_cond_eps=float((q["e32"] / (cond * 6e-8))[indef].max()),
            oracle32_worst_definite=float(q["e32"][~indef].max()) if mixed else 0.0, ev_min_max=float(q["ev_min"][indef].max()),
            n_neg_min=int(q["n_neg"][indef].min()), fallback_rows=int(fell), indefinite_rows=int(indef.sum()),
            loss_err=float(lerr), oracle32_loss_err=float(l32err))
    assert np.all(np.isfinite(Y)) and np.isfinite(loss)
    assert np.all(err <= bound), ("row of %d non-zeros" % int(lens[worst]), bool(indef[worst]), float(err[worst]), float(cond[worst]))
    assert lerr <= max(TOL, 3.0 * l32err), (loss, q["l64"], q["l32"])
    assert fell == int(indef.sum()), (fell, int(indef.sum()))
    assert np.array_equal(Yd.cpu().numpy().T, Y)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        be.check_numeric()                                    # the counters were taken


# ---------------------------------------------------------------------------------------------------------------------------
# C. row-length lattice of the wave-per-row kernel
# ---------------------------------------------------------------------------------------------------------------------------

LENGTHS_C = list(range(65, 130)) + list(range(495, 515)) + [256, 300, 64, 40, 0]


@pytest.mark.parametrize("variant", ["implicit", "implicit_below_one", "explicit_dynamic_lambda", "explicit_plain_lambda"])
def test_wave_per_row_exact_kernel_every_row_length_class(variant):
    """wrmf_chol_mf.hip, rank 128, lambda = 0.1: every length 65..129 (all residues mod 16 and mod 64, 5..9 steps, both parities,
    one and two chunks of its loss pass, and the first lengths above the k x k kernel's 64) and 495..514 (the last steps below the
    hand-over to the normal-equation kernel at 512, and the first rows beyond it), a few rows of the neighbouring kernels and an
    empty one.  implicit: every confidence >= 1 (one operand set); implicit_below_one: x[::9] = 0.3 -- the `_any` instantiation,
    the low-rank kernel stands down --; explicit with lambda_use = lambda * n and plain lambda.  The systems are well
    conditioned (the fp32 oracle is near 1e-6 per row): 1e-4 per row."""
    k, n_item, lam = 128, 3000, 0.1
    implicit = variant.startswith("implicit")
    lens = np.asarray(LENGTHS_C, dtype=np.int64)
    (_, n_cols, p, i, x), X, Y0 = _rows_of_lengths(lens, n_item, k, seed=3000 + len(variant), scale=0.1)
    if variant == "implicit_below_one":
        x[::9] = 0.3
    if not implicit:
        x = np.random.default_rng(5).integers(1, 6, x.size).astype(np.float64)
    csc = (n_item, n_cols, p, i, x)
    cnt = np.bincount(i, minlength=n_item).astype(np.float64)
    dyn = variant == "explicit_dynamic_lambda"
    X64, Y64 = _f64(X), _f64(Y0)
    Y32 = Y0.copy(order="F")
    Y = Y0.copy(order="F")
    if implicit:
        l64 = O.als_implicit(p, i, x, X64, Y64, O.gramian(X64, lam), lam, 0, 3)
        O.als_implicit(p, i, x, X, Y32, O.gramian(X, lam), lam, 0, 3)
        loss = als.als_implicit(csc, X, Y, lam, 1, 0, 3, "float", False, False)
    else:
        l64 = O.als_explicit(p, i, x, X64, Y64, cnt, lam, 0, 3, dyn)
        O.als_explicit(p, i, x, X, Y32, cnt.astype(np.float32), lam, 0, 3, dyn)
        loss = als.als_explicit(csc, X, Y, cnt.astype(np.float32), lam, 1, 0, 3, dyn, "float", False, False)
    err, e32 = _row_err(Y, Y64), _row_err(Y32, Y64)
    err[lens == 0] = e32[lens == 0] = 0.0
    worst = int(err.argmax())
    _report("C %s" % variant, worst_ratio=float(err[worst] / TOL), worst_len=int(lens[worst]), err=float(err[worst]),
            oracle32_worst=float(e32.max()), loss_err=float(abs(loss - l64) / abs(l64)), fro=rel_fro(Y, Y64))
    assert np.all(Y[:, lens == 0] == 0.0)                            # the empty column (wrmf_implicit.hpp:281)
    assert err.max() < TOL, ("row of %d non-zeros" % int(lens[worst]), worst, float(err[worst]))
    assert abs(loss - l64) <= TOL * abs(l64), (loss, l64)
