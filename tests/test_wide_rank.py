"""Ranks 129..256: the reference has no rank limit (arma::Mat<T>, inst/include/wrmf_implicit.hpp:103); through round 3 the device
path answered RSPARSE_HIP_ERR_UNSUPPORTED above 128.  Two kernel files: rsparse_amd/csrc/wrmf_wide.hip (als_wide_kernel: the exact
solver, NNLS, every bias / global-bias operand set; launch_gramian_wide) and rsparse_amd/csrc/wrmf_wide_cg.hip (plain conjugate
gradient, launch_wide_cg_wave's two launches: the wave launch -- wide_cg_wave_kernel<EPL, IMPLICIT, 1>, one wave per row of at
most kWideCgMaxLen = 2048 non-zeros -- and the team launch -- wide_cg_wave_kernel<EPL, IMPLICIT, 8>, eight waves per longer row).
Every solver and operand set through the C ABI against the fp64 oracle on the same fp32 inputs, 1e-4 per row (NNLS: the yardstick
of tests/test_nnls.py -- its fp32 arithmetic squares the system).  The second half of the file (from _long_rows on) walks both
files' kernels over rows of chosen lengths up to 5000 non-zeros, at the ranks where the registers per lane change."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import rel_fro
from oracle import wrmf_oracle as O
from rsparse_amd import als, synth

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _problem(n_user, n_item, k, seed, feedback="implicit", scale=0.1, mean_deg=14, d_max=500):
    d = synth.make_dataset(n_user, n_item, seed=seed, mean_deg=mean_deg, d_max=d_max, feedback=feedback, device="cpu")
    p, i, x = d["c_iu"]
    p, i, x = p.numpy(), i.numpy(), x.numpy().astype(np.float64)
    rng = np.random.default_rng(seed)
    X = np.asfortranarray((rng.standard_normal((k, n_item)) * scale).astype(np.float32))
    Y0 = np.asfortranarray((rng.standard_normal((k, n_user)) * scale).astype(np.float32))
    return (n_item, n_user, p, i, x), X, Y0


def _row_err(Y, Yref):
    return np.linalg.norm(Y - Yref, axis=0) / np.maximum(np.linalg.norm(Yref, axis=0), 1e-30)


@pytest.mark.parametrize("k,n", [(129, 700), (160, 5000), (200, 333), (256, 3001)])
def test_gramian_wide(k, n):
    rng = np.random.default_rng(k + n)
    X = np.asfortranarray(rng.standard_normal((k, n)).astype(np.float32))
    X[0, :] += 3.0
    G = als.gramian(X, 0.1, "float")
    ref = X.astype(np.float64) @ X.astype(np.float64).T + float(np.float32(0.1)) * np.eye(k)
    assert rel_fro(G, ref) < 3e-6 and np.array_equal(G, G.T)


@pytest.mark.parametrize("k", [130, 160, 256])
@pytest.mark.parametrize("solver", [0, 1, 2])
def test_implicit_wide_half_iteration(k, solver):
    csc, X, Y0 = _problem(400, 300, k, seed=k + solver)
    n_rows, n_cols, p, i, x = csc
    if solver == 2:
        X, Y0 = np.abs(X), np.abs(Y0)
    X64 = np.asfortranarray(X, dtype=np.float64)
    G64 = O.gramian(X64, 0.1)
    Yref = np.asfortranarray(Y0, dtype=np.float64).copy(order="F")
    lref = O.als_implicit(p, i, x, X64, Yref, G64, 0.1, solver, 3, n_threads=8)
    Y = Y0.copy(order="F")
    loss = als.als_implicit(csc, X, Y, 0.1, 1, solver, 3, "float", False, False)
    err = _row_err(Y, Yref)
    if solver == 2:   # fp32 NNLS: yardstick = the oracle in float on the same inputs
        Y32 = Y0.copy(order="F")
        O.als_implicit(p, i, x, X, Y32, O.gramian(X, 0.1), 0.1, 2, 3, n_threads=8)
        assert rel_fro(Y, Yref) <= max(TOL, 3 * rel_fro(Y32, Yref)), (rel_fro(Y, Yref), rel_fro(Y32, Yref))
        assert Y.min() >= 0
    else:
        assert err.max() < TOL, (int(err.argmax()), float(err.max()))
        assert abs(loss - lref) <= TOL * abs(lref)
    assert np.all(Y[:, np.diff(p) == 0] == 0)


@pytest.mark.parametrize("k", [144, 256])
@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("dynamic_lambda", [True, False])
def test_explicit_wide_half_iteration(k, solver, dynamic_lambda):
    csc, X, Y0 = _problem(300, 250, k, seed=9 + k + solver, feedback="explicit", scale=0.3)
    n_rows, n_cols, p, i, x = csc
    cnt = np.diff(sp.csc_matrix((x, i, p), shape=(n_rows, n_cols)).tocsr().indptr).astype(np.float64)
    X64 = np.asfortranarray(X, dtype=np.float64)
    Yref = np.asfortranarray(Y0, dtype=np.float64).copy(order="F")
    lref = O.als_explicit(p, i, x, X64, Yref, cnt, 0.1, solver, 3, dynamic_lambda, n_threads=8)
    Y = Y0.copy(order="F")
    loss = als.als_explicit(csc, X, Y, cnt.astype(np.float32), 0.1, 1, solver, 3, dynamic_lambda, "float", False, False)
    if solver == 1:   # three fp32 CG steps from a warm start on lambda_use = 0.1 n systems: the oracle in float as the yardstick
        Y32 = Y0.copy(order="F")
        O.als_explicit(p, i, x, X, Y32, cnt.astype(np.float32), 0.1, 1, 3, dynamic_lambda, n_threads=8)
        assert rel_fro(Y, Yref) <= max(TOL, 3 * rel_fro(Y32, Yref))
    else:
        err = _row_err(Y, Yref)
        assert err.max() < TOL, (int(err.argmax()), float(err.max()))
    assert abs(loss - lref) <= 2e-4 * abs(lref)


@pytest.mark.parametrize("bias_last", [True, False])
def test_wide_with_biases_and_global_bias(bias_last):
    """rank 131 with user/item biases (a 130 x 130 system), explicit and implicit; implicit global bias with every solver at 140"""
    k = 131
    csc, X, Y0 = _problem(200, 150, k, seed=3, feedback="explicit", scale=0.3)
    n_rows, n_cols, p, i, x = csc
    X[0 if bias_last else k - 1, :] = 1.0
    Y0[k - 1 if bias_last else 0, :] = 1.0
    cnt = np.diff(sp.csc_matrix((x, i, p), shape=(n_rows, n_cols)).tocsr().indptr).astype(np.float64)
    X64 = np.asfortranarray(X, dtype=np.float64)
    Yref = np.asfortranarray(Y0, dtype=np.float64).copy(order="F")
    lref = O.als_explicit(p, i, x, X64, Yref, cnt, 0.1, 0, 3, True, with_biases=True, is_x_bias_last_row=bias_last)
    Y = Y0.copy(order="F")
    loss = als.als_explicit(csc, X, Y, cnt.astype(np.float32), 0.1, 1, 0, 3, True, "float", True, bias_last)
    assert _row_err(Y, Yref).max() < TOL and abs(loss - lref) <= TOL * abs(lref)
    csc, X, Y0 = _problem(200, 150, k, seed=4)
    n_rows, n_cols, p, i, x = csc
    X[0 if bias_last else k - 1, :] = 1.0
    Y0[k - 1 if bias_last else 0, :] = 1.0
    X64 = np.asfortranarray(X, dtype=np.float64)
    G64 = O.gramian(np.asfortranarray(X64[:-1] if bias_last else X64[1:]), 0.1)
    Yref = np.asfortranarray(Y0, dtype=np.float64).copy(order="F")
    lref = O.als_implicit(p, i, x, X64, Yref, G64, 0.1, 0, 3, with_biases=True, is_x_bias_last_row=bias_last, global_bias=0.02)
    Y = Y0.copy(order="F")
    loss = als.als_implicit(csc, X, Y, 0.1, 1, 0, 3, "float", True, bias_last, global_bias=0.02)
    assert _row_err(Y, Yref).max() < TOL and abs(loss - lref) <= TOL * abs(lref)
    if bias_last:
        k2 = 140
        csc, X, Y0 = _problem(200, 150, k2, seed=5)
        n_rows, n_cols, p, i, x = csc
        X64 = np.asfortranarray(X, dtype=np.float64)
        for solver in (0, 1):
            Yref = np.asfortranarray(Y0, dtype=np.float64).copy(order="F")
            lref = O.als_implicit(p, i, x, X64, Yref, O.gramian(X64, 0.1), 0.1, solver, 3, global_bias=0.03)
            Y = Y0.copy(order="F")
            loss = als.als_implicit(csc, X, Y, 0.1, 1, solver, 3, "float", False, False, global_bias=0.03)
            bound = TOL if solver == 0 else 5e-4      # (the global-bias CG is the reference's "very poor numerical precision" variant)
            assert _row_err(Y, Yref).max() < bound, solver
            assert abs(loss - lref) <= bound * abs(lref)


def test_wide_cholesky_falls_back_to_the_general_solver():
    k = 150
    csc, X, Y0 = _problem(120, 100, k, seed=4, scale=0.3, mean_deg=30)
    n_rows, n_cols, p, i, x = csc
    rng = np.random.default_rng(1)
    x = np.where(rng.random(x.size) < 0.5, 0.25, 3.0)
    X64 = X.astype(np.float64)
    G = np.asfortranarray(0.05 * (X64 @ X64.T) + 0.1 * np.eye(k))
    Yref = np.asfortranarray(Y0, dtype=np.float64).copy(order="F")
    O.als_implicit(p, i, x, np.asfortranarray(X64), Yref, G, 0.1, 0, 3)
    n_bad, cond = 0, np.ones(n_cols)
    for c in range(n_cols):
        idx, val = i[p[c]:p[c + 1]], x[p[c]:p[c + 1]]
        ev = np.linalg.eigvalsh(G + (X64[:, idx] * (val - 1.0)) @ X64[:, idx].T)
        cond[c] = np.abs(ev).max() / np.abs(ev).min()
        n_bad += ev.min() < -1e-4
    assert n_bad >= 3
    Y = Y0.copy(order="F")
    als.als_implicit((n_rows, n_cols, p, i, x), X, Y, 0.1, 1, 0, 3, "float", False, False, XtX=np.asfortranarray(G, dtype=np.float32))
    assert np.all(np.isfinite(Y))
    err = _row_err(Y, Yref)
    bound = np.maximum(1e-4, 20.0 * cond * 6e-8)
    assert np.all(err <= bound), (int(np.argmax(err / bound)), float(err.max()))


def test_wrmf_at_rank_160(ml_train):
    """the class end to end at a rank the reference accepts and the device path used to refuse: fit (CG), the final exact
    solve, transform and predict (the top-k kernel's rank-256 instantiation)"""
    from rsparse_amd import WRMF
    n_user, n_item, p, i, x = ml_train
    train = sp.csc_matrix((x, i, p), shape=(n_user, n_item))
    rng = np.random.default_rng(2)
    U0 = (rng.standard_normal((n_user, 160)) * 0.01).astype(np.float32)
    model = WRMF(rank=160, lambda_=0.1, feedback="implicit", solver="conjugate_gradient", precision="float")
    model._init_user_factors = U0
    emb = model.fit_transform(train, n_iter=2, convergence_tol=-1)
    ref = O.OracleWRMF(160, lam=0.1, feedback="implicit", solver="conjugate_gradient", dtype=np.float64, n_threads=8)
    ref_emb = ref.fit_transform(n_user, n_item, p, i, x, U0.T.astype(np.float64), n_iter=2, convergence_tol=-1)
    assert rel_fro(model.components, ref.components) < TOL and rel_fro(emb, ref_emb) < TOL
    assert np.allclose([l[1] for l in model.losses], [l[1] for l in ref.losses], rtol=TOL)
    assert np.array_equal(emb, model.transform(train))
    top = model.predict(train[:80], 9)
    sc = emb[:80].astype(np.float64) @ model.components.astype(np.float64)
    sc[train[:80].toarray() != 0] = -np.inf
    best = np.sort(sc, axis=1)[:, ::-1][:, :9]
    assert np.allclose(top.scores, best, rtol=1e-4, atol=1e-5)


# ---- long rows and the register edges ------------------------------------------------------------------------------------------
# Column lengths: the batch-of-16 / chunk-of-64 edges of the wave launch, its last rows (2047, 2048), the team launch with a last
# chunk of 1, 15, 16, 17, 63, 64, 1 + 64 non-zeros, 40 chunks (= 5 per wave exactly) and one non-zero either side, 64 chunks and one
# non-zero more, 5000.
LONG_EDGES = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129,
              2047, 2048,
              2049, 2063, 2064, 2065, 2111, 2112, 2113,
              2559, 2560, 2561,
              4096, 4097, 5000]
LONG_N_ITEM = 6000
TEAM_MIN = 2049      # kWideCgMaxLen + 1 (wrmf_internal.h): the shortest row of the team launch
LAM = 0.1


@functools.lru_cache(maxsize=None)
def _long_rows(k, feedback, max_len=None):
    """(csc, X, Y0, cnt): a CSC (columns = the rows to solve) whose column j has EXACTLY lens[j] distinct items out of 6000 --
    LONG_EDGES (those beyond max_len left out), then 60 random lengths in 1..199.  Implicit: confidences 1 + geometric(0.5),
    factors 0.05 N(0, 1); explicit: ratings 1..5, factors 0.3 N(0, 1), cnt = bincount of the items.  Shared between the tests and
    read-only."""
    rng = np.random.default_rng(1000 * k + (feedback == "explicit"))
    lens = np.asarray([n for n in LONG_EDGES if max_len is None or n <= max_len] + list(rng.integers(1, 200, size=60)), dtype=np.int64)
    p = np.zeros(lens.size + 1, dtype=np.int32)
    p[1:] = np.cumsum(lens)
    idx = np.concatenate([np.sort(rng.choice(LONG_N_ITEM, size=int(n), replace=False)) for n in lens]).astype(np.int32)
    if feedback == "implicit":
        x, scale = 1.0 + rng.geometric(0.5, size=idx.size).astype(np.float64), 0.05
    else:
        x, scale = rng.integers(1, 6, size=idx.size).astype(np.float64), 0.3
    X = np.asfortranarray((rng.standard_normal((k, LONG_N_ITEM)) * scale).astype(np.float32))
    Y0 = np.asfortranarray((rng.standard_normal((k, lens.size)) * scale).astype(np.float32))
    cnt = np.bincount(idx, minlength=LONG_N_ITEM).astype(np.float64)
    for a in (p, idx, x, X, Y0, cnt):
        a.flags.writeable = False
    return (LONG_N_ITEM, lens.size, p, idx, x), X, Y0, cnt


@functools.lru_cache(maxsize=None)
def _long_rows_ref(k, feedback, solver, max_len=None, global_bias=0.0):
    """the oracle in double on _long_rows' fp32 inputs: (Yref, loss), read-only"""
    (n_rows, n_cols, p, i, x), X, Y0, cnt = _long_rows(k, feedback, max_len)
    X64 = np.asfortranarray(X, dtype=np.float64)
    Yref = np.asfortranarray(Y0, dtype=np.float64).copy(order="F")
    if feedback == "implicit":
        lref = O.als_implicit(p, i, x, X64, Yref, O.gramian(X64, LAM), LAM, solver, 3, n_threads=8, global_bias=global_bias)
    else:
        lref = O.als_explicit(p, i, x, X64, Yref, cnt, LAM, solver, 3, True, n_threads=8)
    Yref.flags.writeable = False
    return Yref, lref


def _long_rows_device(k, feedback, solver, max_len=None, global_bias=0.0):
    csc, X, Y0, cnt = _long_rows(k, feedback, max_len)
    Y = Y0.copy(order="F")
    if feedback == "implicit":
        loss = als.als_implicit(csc, X, Y, LAM, 1, solver, 3, "float", False, False, global_bias=global_bias)
    else:
        loss = als.als_explicit(csc, X, Y, cnt.astype(np.float32), LAM, 1, solver, 3, True, "float", False, False)
    return Y, loss


def _check_long_rows(k, feedback, solver, bound, max_len=None, global_bias=0.0):
    """every solved row within `bound` of the oracle, the worst one named; the loss within `bound`; the empty column comes back
    as zeros (with a global bias the reference solves it like any other: wrmf_implicit.hpp:180)"""
    lens = np.diff(_long_rows(k, feedback, max_len)[0][2])
    Yref, lref = _long_rows_ref(k, feedback, solver, max_len, global_bias)
    Y, loss = _long_rows_device(k, feedback, solver, max_len, global_bias)
    assert np.all(np.isfinite(Y))
    solved = (lens > 0) | (global_bias != 0.0)
    err = np.where(solved, _row_err(Y, Yref), 0.0)
    worst = int(err.argmax())
    print("long rows: k %d %s solver %d max_len %s gbias %g: worst row %d (%d non-zeros) %.3g, worst beyond 2048 %.3g, loss %.3g"
          % (k, feedback, solver, max_len, global_bias, worst, lens[worst], err[worst], err[lens >= TEAM_MIN].max(initial=0.0),
             abs(loss - lref) / abs(lref)))
    bad = np.flatnonzero(~(err < bound))
    assert bad.size == 0, ("worst row %d, %d non-zeros, error %.3g; rows out of bound (index, length, error): %s"
                           % (worst, lens[worst], err[worst], [(int(c), int(lens[c]), float("%.3g" % err[c])) for c in bad]))
    assert abs(loss - lref) <= bound * abs(lref), (loss, lref)
    assert (lens == 0).any() and np.all(Y[:, ~solved] == 0)
    return lens


@pytest.mark.parametrize("feedback", ["implicit", "explicit"])
@pytest.mark.parametrize("k", [129, 192, 193, 256])
def test_wide_cg_long_rows_per_row(k, feedback):
    """plain CG (wrmf_wide_cg.hip), both launches in one call: rows of up to 2048 non-zeros on the wave launch, the longer ones
    on teams of eight waves; EPL = 3 with one live coordinate in the third register (129) and with it full (192), EPL = 4 with
    one live coordinate in the fourth (193) and full (256); 129 and 193: rows of X that are not 16-byte aligned.
    The oracle in FLOAT on exactly these inputs stays at or below 1.5e-5 per row and 1.3e-6 on the loss."""
    lens = _check_long_rows(k, feedback, 1, TOL)
    assert lens.max() > 2048     # (the team launch is reached)


def test_wide_cg_longest_row_at_the_threshold():
    """the longest row has exactly 2048 non-zeros: launch_wide_cg_wave with order == nullptr -- no team launch, its loss slots
    cleared by the memset and summed all the same (the oracle in float: 1.8e-6 per row, 2.2e-6 on the loss)"""
    _long_rows_device(193, "implicit", 1)     # (a call with a team launch first: it leaves that launch's loss slots non-zero)
    lens = _check_long_rows(193, "implicit", 1, TOL, max_len=2048)
    assert lens.max() == 2048


def _subset(csc, Y0, pick):
    n_rows, n_cols, p, i, x = csc
    lens = np.diff(p)[pick]
    p2 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = np.concatenate([np.arange(p[c], p[c + 1]) for c in pick])
    return (n_rows, len(pick), p2, i[idx], x[idx]), np.asfortranarray(Y0[:, pick])


@pytest.mark.parametrize("k,feedback", [(193, "implicit"), (192, "explicit")])
def test_wide_cg_long_rows_bits(k, feedback):
    """The same call, bit for bit: (1) again -- the team sums its waves' parts in wave order, nothing is atomic; (2) a shuffled
    subset of the columns (every row of the team launch and some short ones) -- a row depends on its own data only, so nothing
    that a team left in LDS may reach its next row; (3) on the device-resident path."""
    import torch
    from rsparse_amd.engine import HipBackend
    csc, X, Y0, cnt = _long_rows(k, feedback)
    n_rows, n_cols, p, i, x = csc
    lens = np.diff(p)
    implicit = feedback == "implicit"
    cnt32 = cnt.astype(np.float32)
    G = als.gramian(X, LAM, "float") if implicit else None

    def solve(csc_, Y):
        if implicit:
            return als.als_implicit(csc_, X, Y, LAM, 1, 1, 3, "float", False, False, XtX=G)
        return als.als_explicit(csc_, X, Y, cnt32, LAM, 1, 1, 3, True, "float", False, False)

    Y, loss = _long_rows_device(k, feedback, 1)
    Y2 = Y0.copy(order="F")
    loss2 = solve(csc, Y2)
    assert np.array_equal(Y, Y2) and loss == loss2
    rng = np.random.default_rng(5)
    long_rows, short_rows = np.flatnonzero(lens >= TEAM_MIN), np.flatnonzero(lens < TEAM_MIN)
    pick = rng.permutation(np.concatenate([long_rows, rng.choice(short_rows, size=20, replace=False)]))
    assert long_rows.size == sum(n >= TEAM_MIN for n in LONG_EDGES)
    sub, Ysub = _subset(csc, Y0, pick)
    solve(sub, Ysub)
    differ = [(int(c), int(lens[c])) for j, c in enumerate(pick) if not np.array_equal(Ysub[:, j], Y[:, c])]
    assert not differ, differ
    be = HipBackend()
    h = be.make_csc(n_rows, n_cols, be.to_device(p.copy(), torch.int32), be.to_device(i.copy(), torch.int32), be.to_device(x.astype(np.float32), torch.float32))
    Xd, Yd = be.to_device(np.array(X.T, order="C"), torch.float32), be.to_device(np.array(Y0.T, order="C"), torch.float32)   # (copies: the shared inputs are read-only)
    Gd = be.to_device(np.ascontiguousarray(G), torch.float32) if implicit else None
    lossd = torch.zeros(1, dtype=torch.float64, device=be.device)
    be.half_iteration(h, implicit, Xd, Yd, Gd, LAM, 1, 3, True, lossd)
    Yr = Yd.cpu().numpy().T
    differ = [(int(c), int(lens[c])) for c in range(n_cols) if not np.array_equal(Yr[:, c], Y[:, c])]
    assert not differ, differ


@pytest.mark.parametrize("feedback", ["implicit", "explicit"])
@pytest.mark.parametrize("k", [129, 256])
def test_wide_exact_solver_long_rows(k, feedback):
    """als_wide_kernel (wrmf_wide.hip) stages a row in chunks of CH vectors (16 at rank 256): rows of up to 5000 non-zeros, i.e. up
    to 313 chunks, chunk tails of every length.  The oracle in FLOAT on exactly these inputs stays at or below 1.2e-5 per row and 1e-6 on the loss."""
    _check_long_rows(k, feedback, 0, TOL)


def test_wide_global_bias_cg_long_rows():
    """als_wide_kernel's conjugate gradient (the global bias keeps it off wrmf_wide_cg.hip) on the same rows; 5e-4: the bound of
    test_wide_with_biases_and_global_bias for this variant (the oracle in float on exactly these inputs: 2.6e-6 per row).  With a global bias the reference solves the empty column too
    (wrmf_implicit.hpp:180): it is compared like the others."""
    _check_long_rows(193, "implicit", 1, 5e-4, global_bias=0.03)


@pytest.mark.parametrize("k,n", [(129, 1), (129, 15), (193, 63), (193, 65), (256, 16385), (192, 4097)])
def test_gramian_wide_edges(k, n):
    """launch_gramian_wide: fewer columns than one staged chunk, fewer than the 64 a block takes, one more than that, and
    256 * 64 + 1 -- 65 columns a block, so that the trailing blocks get an empty range"""
    rng = np.random.default_rng(k + n)
    X = np.asfortranarray(rng.standard_normal((k, n)).astype(np.float32))
    X[0, :] += 3.0
    for lam in (0.0, 0.1):
        G = als.gramian(X, lam, "float")
        ref = X.astype(np.float64) @ X.astype(np.float64).T + float(np.float32(lam)) * np.eye(k)
        assert rel_fro(G, ref) < 3e-6 and np.array_equal(G, G.T)
