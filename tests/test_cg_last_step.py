"""The last CG step of the register-resident kernels (wrmf_cgq.hip, wrmf_cgp.hip): p' A p from the dots of the step, no vector A p.

    p' A p = p' G p + sum_j (c_j - 1) (x_j . p)^2          (explicit feedback: sum_j (x_j . p)^2 + lambda_use p . p)

so the last step forms the dots, the dense product and scalar sums, takes alpha, updates the kept dots and x, and goes to the
loss: no residual, no beta, no new p.  What can go wrong is the scalar (a term counted per lane instead of per group, a team wave's
share lost, the dense part dotted with the wrong piece), the kept dots (the loss misses the last alpha) and the barrier count of
a workgroup whose rows do not all run the step.

    alpha per row    cg_steps = 1: the only step is the new path and y - x0 = alpha r0, so alpha_dev = <y - x0, r0> / <r0, r0> with
                     r0 in float64 on the host, against alpha64 = r0' r0 / r0' A r0.  The returned loss against the loss of the
                     returned rows here too: the only alpha is the largest, so a t_acc that missed alpha t_cur shows most.
                     The bound is derived per row:
                     (n + 2 k + 16) 2^-24 (|p|' |G| |p| + sum (c - 1) t^2) / p' A p for the denominator -- n + k products summed
                     in some order, the dense product's fp16 splitting (2^-21 per product, three products) and the 16-lane and
                     group sums inside the 16 -- plus the same expression for the numerator's dot, whose terms are all of one
                     sign (amplification 1).  Asserted on the host before the device call: below 1e-3 for 95 % of the rows.
    rows and loss    cg_steps = 2 and 3 against the fp64 oracle, per row ||y - y64|| / ||y64|| <= max(1e-4, 3 err32) with the
                     siblings' cap on the yardstick; the returned loss within 1e-4 of the loss recomputed in float64 from the
                     RETURNED rows (a t_acc that missed the last alpha t_cur shows here and nowhere else)
    lockstep         every other row starts from the oracle's 60-step solution and ends in its first step, its neighbour of the
                     same length does three: a stopped row sits through the barriers of the last step beside it
    no step          cg_steps = 0 twice: bit-identical rows and loss

Lengths: every class edge of the rank-128 launches twice in a row (1, 2, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 320, 321,
384, 385, 512), and 513 / 700 at ranks 32 and 20 for the streamed kernel.  Ranks 128, 100 (k < KP), 64, 32, 20.  Inputs as the
siblings': factors N(0, 0.1^2), lambda 0.1, confidences 1 + Gamma(1, 2), 3000 gathered rows.

Every test prints its figures before it asserts (pytest -s, lines starting with `cg_last_step`): profiles/r12/."""
import numpy as np
import pytest

from oracle import wrmf_oracle as O
from rsparse_amd import als

pytestmark = pytest.mark.gpu
TOL = 1e-4
YARDSTICK_SHARE = 0.05
N_ITEM = 3000
LAM, SCALE = 0.1, 0.1
CG = 1
GBIAS = 0.3
EDGES = [1, 2, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 320, 321, 384, 385, 512]
STREAMED = [513, 700]
RANKS = [128, 100, 64, 32, 20]
# (implicit, dynamic_lambda, global bias)
VARIANTS = {"implicit": (True, True, 0.0), "explicit_dynamic": (False, True, 0.0), "explicit_plain": (False, False, 0.0),
            "implicit_gbias": (True, True, GBIAS)}
CASES = [(k, v) for v in ("implicit", "explicit_dynamic", "explicit_plain") for k in RANKS] + [(128, "implicit_gbias")]


def _lengths(k):
    return np.repeat(np.asarray(EDGES + (STREAMED if k <= 32 else []), dtype=np.int64), 2)


_inputs = {}


def _problem(k):
    """column j has _lengths(k)[j] distinct random items; drawn once per rank and left unchanged"""
    if k not in _inputs:
        lens = _lengths(k)
        rng = np.random.default_rng([20, k])
        p = np.zeros(len(lens) + 1, dtype=np.int32)
        p[1:] = np.cumsum(lens)
        idx = np.concatenate([np.sort(rng.choice(N_ITEM, size=int(n), replace=False)) for n in lens]).astype(np.int32)
        x = (1.0 + rng.gamma(1.0, 2.0, size=idx.size)).astype(np.float32).astype(np.float64)
        X = np.asfortranarray((rng.standard_normal((k, N_ITEM)) * SCALE).astype(np.float32))
        Y0 = np.asfortranarray((rng.standard_normal((k, len(lens))) * SCALE).astype(np.float32))
        for a in (p, idx, x, X, Y0):
            a.setflags(write=False)
        _inputs[k] = (lens, (N_ITEM, len(lens), p, idx, x), X, Y0)
    return _inputs[k]


def _oracle(csc, X, Y0, variant, steps, dtype):
    implicit, dyn, gb = VARIANTS[variant]
    _, _, p, i, x = csc
    Xd = np.asfortranarray(X, dtype=dtype)
    Y = np.asfortranarray(Y0, dtype=dtype).copy(order="F")
    if implicit:
        loss = O.als_implicit(p, i, x, Xd, Y, O.gramian(Xd, LAM), LAM, CG, steps, n_threads=8, global_bias=gb)
    else:
        cnt = np.bincount(i, minlength=csc[0]).astype(dtype)
        loss = O.als_explicit(p, i, x, Xd, Y, cnt, LAM, CG, steps, dyn, n_threads=8)
    return Y, loss


def _device(csc, X, Y0, variant, steps):
    implicit, dyn, gb = VARIANTS[variant]
    Y = Y0.copy(order="F")
    if implicit:
        loss = als.als_implicit(csc, X, Y, LAM, 1, CG, steps, "float", False, False, global_bias=gb)
    else:
        cnt = np.bincount(csc[3], minlength=csc[0]).astype(np.float32)
        loss = als.als_explicit(csc, X, Y, cnt, LAM, 1, CG, steps, dyn, "float", False, False)
    return Y, loss


def _row_err(Y, Yref):
    return np.linalg.norm(Y - Yref, axis=0) / np.maximum(np.linalg.norm(Yref, axis=0), 1e-30)


def _loss64(csc, X, Y, variant):
    """the half-iteration's loss in float64 from the rows Y (wrmf_implicit.hpp:259-304, wrmf_explicit.hpp:131-173)"""
    implicit, dyn, gb = VARIANTS[variant]
    n_item, n_col, p, idx, x = csc
    X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
    total = 0.0
    for j in range(n_col):
        sl = slice(p[j], p[j + 1])
        t = X64[:, idx[sl]].T @ Y64[:, j]
        yy = float(Y64[:, j] @ Y64[:, j])
        if implicit:
            total += float(x[sl] @ ((1.0 - gb) - t) ** 2) + LAM * yy
        else:
            total += float(((x[sl] - t) ** 2).sum()) + LAM * (float(p[j + 1] - p[j]) if dyn else 1.0) * yy
    sq = (X64 * X64).sum(axis=0)
    total += LAM * float((sq * np.bincount(idx, minlength=n_item)).sum() if (not implicit and dyn) else sq.sum())
    return total / float(p[-1])


# ---------------------------------------------------------------------------------------------------------------------------
# alpha of the only step, per row
# ---------------------------------------------------------------------------------------------------------------------------

def _alpha_reference(k, variant):
    """per row in float64: r0, alpha64 = r0' r0 / r0' A r0 and the bound on the relative error of a float alpha"""
    implicit, dyn, gb = VARIANTS[variant]
    lens, csc, X, Y0 = _problem(k)
    _, n_col, p, idx, x = csc
    X64, Y64 = X.astype(np.float64), Y0.astype(np.float64)
    G = X64 @ X64.T + float(np.float32(LAM)) * np.eye(k)
    base = -gb * X64.sum(axis=1)
    R0 = np.zeros((k, n_col))
    alpha, bound = np.zeros(n_col), np.zeros(n_col)
    for j in range(n_col):
        sl = slice(p[j], p[j + 1])
        Xn, c, x0, n = X64[:, idx[sl]], x[sl], Y64[:, j], int(p[j + 1] - p[j])
        t0 = Xn.T @ x0
        if implicit:
            r0 = Xn @ (c - (c - 1.0) * (t0 + gb)) - G @ x0 + base
            t = Xn.T @ r0
            dense, dense_abs, quads = float(r0 @ G @ r0), float(np.abs(r0) @ np.abs(G) @ np.abs(r0)), float((c - 1.0) @ t ** 2)
        else:
            lam_use = float(np.float32(LAM)) * (n if dyn else 1.0)
            r0 = Xn @ (c - t0) - lam_use * x0
            t = Xn.T @ r0
            dense = dense_abs = lam_use * float(r0 @ r0)
            quads = float(t @ t)
        pap = dense + quads
        R0[:, j], alpha[j] = r0, float(r0 @ r0) / pap
        ops = (n + 2 * k + 16) * 2.0 ** -24
        bound[j] = ops * (dense_abs + quads) / pap + ops * 1.0      # denominator + numerator (|r|'|r| / r'r = 1)
    share = float(np.mean(bound < 1e-3))
    assert share >= 0.95, ("the bound says nothing", k, variant, share, float(bound.max()))
    return lens, csc, X, Y0, R0, alpha, bound


@pytest.mark.parametrize("k,variant", CASES)
def test_alpha_of_the_last_step_per_row(k, variant):
    """cg_steps = 1: y = x0 + alpha r0, the alpha from the dots-only sweep.  Two rows per class edge (a team's second row, the
    second half of a two-row wave, two groups of a four-row wave), 513 / 700 on the streamed kernel at ranks 32 and 20"""
    lens, csc, X, Y0, R0, alpha64, bound = _alpha_reference(k, variant)
    Y, loss = _device(csc, X, Y0, variant, 1)
    D = Y.astype(np.float64) - Y0.astype(np.float64)
    alpha_dev = (D * R0).sum(axis=0) / (R0 * R0).sum(axis=0)
    err = np.abs(alpha_dev - alpha64) / np.abs(alpha64)
    off = np.linalg.norm(D - alpha_dev * R0, axis=0) / np.linalg.norm(D, axis=0)   # what of y - x0 is not along r0
    worst = int(np.argmax(err / bound))
    lret = _loss64(csc, X, Y, variant)
    lerr = abs(loss - lret) / abs(lret)
    print("cg_last_step alpha k=%d %s rows=%d worst err/bound=%.3g (row %d, %d non-zeros: err %.3g bound %.3g alpha %.4g) "
          "max_bound=%.3g off_direction=%.3g loss_vs_returned_rows=%.3g"
          % (k, variant, len(lens), float(err[worst] / bound[worst]), worst, int(lens[worst]), float(err[worst]),
             float(bound[worst]), float(alpha64[worst]), float(bound.max()), float(off.max()), lerr))
    assert np.isfinite(loss) and np.all(np.isfinite(Y))
    assert np.all(err <= bound), ("row %d of %d non-zeros" % (worst, int(lens[worst])), float(err[worst]), float(bound[worst]))
    # the only alpha is the largest one: a t_acc that missed alpha * t_cur moves this loss most
    assert lerr <= TOL, (loss, lret)


# ---------------------------------------------------------------------------------------------------------------------------
# rows and loss at 2 and 3 steps
# ---------------------------------------------------------------------------------------------------------------------------

_refs = {}


def _reference(tag, csc, X, Y0, variant, steps):
    """the oracle in double and in float, the per-row bound and the cap on the yardstick: asserted here, on the CPU"""
    if tag not in _refs:
        Y64, l64 = _oracle(csc, X, Y0, variant, steps, np.float64)
        Y32, _ = _oracle(csc, X, Y0, variant, steps, np.float32)
        err32 = _row_err(Y32, Y64)
        bound = np.maximum(TOL, 3.0 * err32)
        share = float(np.mean(bound > TOL))
        assert np.all(np.isfinite(Y64)) and np.all(np.isfinite(Y32))
        assert share <= YARDSTICK_SHARE, ("the yardstick swallows the test", tag, share, float(err32.max()))
        _refs[tag] = (Y64, l64, err32, bound)
    return _refs[tag]


def _check_rows_and_loss(tag, lens, csc, X, variant, ref, Y, loss):
    Y64, l64, err32, bound = ref
    err = _row_err(Y, Y64)
    worst = int(np.argmax(err / bound))
    lret = _loss64(csc, X, Y, variant)
    lerr, lerr64 = abs(loss - lret) / abs(lret), abs(loss - l64) / abs(l64)
    print("cg_last_step %s rows=%d worst_row_err=%.3g (row %d, %d non-zeros, bound %.3g) max_err32=%.3g "
          "loss_vs_returned_rows=%.3g loss_vs_oracle=%.3g" % (tag, len(lens), float(err[worst]), worst, int(lens[worst]),
                                                             float(bound[worst]), float(err32.max()), lerr, lerr64))
    assert np.isfinite(loss) and np.all(np.isfinite(Y))
    assert np.all(err <= bound), ("row %d of %d non-zeros" % (worst, int(lens[worst])), float(err[worst]), float(bound[worst]))
    assert lerr <= TOL, (loss, lret)


@pytest.mark.parametrize("steps", [2, 3])
@pytest.mark.parametrize("k,variant", CASES)
def test_rows_and_loss_behind_the_last_step(k, variant, steps):
    """one or two full steps, then the dots-only one: the rows against the oracle, the loss against the returned rows"""
    lens, csc, X, Y0 = _problem(k)
    tag = "rows k=%d %s steps=%d" % (k, variant, steps)
    ref = _reference(tag, csc, X, Y0, variant, steps)
    Y, loss = _device(csc, X, Y0, variant, steps)
    _check_rows_and_loss(tag, lens, csc, X, variant, ref, Y, loss)


# ---------------------------------------------------------------------------------------------------------------------------
# a stopped row beside one that runs the last step
# ---------------------------------------------------------------------------------------------------------------------------

def test_stopped_rows_keep_in_step_with_the_last_step():
    """rank 128, three steps: the even columns start from the oracle's 60-step solution rounded to float and end in their first
    step (asserted on the oracle: steps 2 and 3 change nothing), the odd ones -- same length, so the same launch and, in the
    shared-product and team kernels, the same workgroup -- run all three.  The workgroups of the matrix-core, two-row, four-row and
    team launches then hold waves that run the last step and waves that only keep its barriers"""
    k, variant = 128, "implicit"
    lens, csc, X, Y0 = _problem(k)
    Ysol, _ = _oracle(csc, X, Y0, variant, 60, np.float64)
    Y0 = Y0.copy(order="F")
    Y0[:, ::2] = Ysol[:, ::2].astype(np.float32)
    tag = "lockstep k=%d" % k
    ref = _reference(tag, csc, X, Y0, variant, 3)
    one_step, _ = _oracle(csc, X, Y0, variant, 1, np.float64)
    stopped = (one_step == ref[0]).all(axis=0)
    assert stopped[::2].all(), ("a converged start went on", int(lens[::2][np.argmin(stopped[::2])]))
    assert not stopped[1::2].any()
    Y, loss = _device(csc, X, Y0, variant, 3)
    _check_rows_and_loss(tag, lens, csc, X, variant, ref, Y, loss)
    err = _row_err(Y, ref[0])
    print("cg_last_step lockstep worst stopped row %.3g, worst running row %.3g" % (float(err[::2].max()), float(err[1::2].max())))


# ---------------------------------------------------------------------------------------------------------------------------
# no step at all
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,variant", [(128, "implicit"), (100, "implicit"), (32, "implicit"), (128, "explicit_dynamic")])
def test_no_step_is_the_same_twice(k, variant):
    """cg_steps = 0: neither the loop nor the last step runs; two calls give the same bits (against the parent: case C of
    tests/test_cg_rank_classes.py)"""
    lens, csc, X, Y0 = _problem(k)
    Y1, l1 = _device(csc, X, Y0, variant, 0)
    Y2, l2 = _device(csc, X, Y0, variant, 0)
    print("cg_last_step no_step k=%d %s loss=%.9g" % (k, variant, l1))
    assert np.array_equal(Y1, Y2) and l1 == l2
    assert np.array_equal(Y1, Y0)     # a row that takes no step is its warm start
