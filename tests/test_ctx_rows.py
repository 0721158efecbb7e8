"""The multi-GPU context (rsparse_amd/csrc/wrmf_ctx.cpp, rsparse_amd/ctx.py) per ROW and over its call lifecycle.  The other
context tests compare whole matrices in a Frobenius norm after three iterations; a wrong row of a small sub-block, a misplaced
storage row or a regulariser term read at the wrong offset disappears there.  Here: ONE half-iteration through a
comm = "shared" context (rank threads on one device: ownership, sub-block storage, exchange points and summation orders are the
production code), compared per solved row with the fp64 oracle on the same fp32 inputs.

    rows:  err(row) <= max(1e-4, 3 x the fp32 oracle's error on that row); the bound may pass 1e-4 on at most 5 % of the rows
    loss:  relative error <= max(1e-4, 3 x the fp32 oracle's loss error)
    the fixed side comes back bit-unchanged; set_factors -> get_factors is the identity; info() is what engine.Layout predicts

Asserted on the oracle alone BEFORE a device call, so that a failure cannot hide: every solved non-empty row moves from its
warm start by at least 10 x its bound (with cg_steps = 0 the reference returns the warm start: there the oracle must BE the warm
start, and the bound holds the device to it), and any two non-empty rows' solutions differ by at least 1e-2 -- a row written to
another row's place cannot pass.

The solved side is a length lattice around every row-length class of the kernels (4 rows of each length, shuffled), with empty
rows first, last and at the head of the second block of a two-rank cut (a balanced cut always follows the non-empty row that
reached its share, so the empty rows begin the next block); the fixed side has 700 rows.  The lattice runs once as users and once
transposed, as items.

A. layout cells (ranks, sub-blocks solved, sub-blocks fixed) x feedback / solver / cg_steps / dynamic_lambda x rank; one matrix
   whose balanced cuts leave ranks without rows on either side.
B. the header's claim that results depend on the number of ranks only through the summation order of the Gramian and the loss:
   explicit feedback has no Gramian, so EVERY row of every explicit cell is bit-identical to the one-rank run; implicit results
   are bit-identical across the solved side's sub-block count, cell (8, 40, 1) against (8, 1, 1), row by row.  The exception,
   by the code: take_value_stats (wrmf_capi.cpp) scans the values of the HANDLE for max c, a context has one handle per rank
   and sub-block (with 40 sub-blocks a handle holds one row), and these kernels scale the fp16 operand terms of their
   matrix-core assemblies by a power of two taken from max c - 1 (times max |F|, which is the exchanged, global one):
       wrmf_ne.hip (a.ne_stats)          conjugate gradient, ranks 36..128 (ne_supported), rows of more than 512 non-zeros
       wrmf_cg_mf.hip (a.ne_stats)       conjugate gradient, rank 128, rows of 513..16384 non-zeros
       wrmf_chol_wave.hip (wave_stats)   Cholesky, ranks up to 64 -- a rank below 64 runs on copies padded to 64 -- every row
       wrmf_chol_mf.hip (wave_stats)     Cholesky, ranks 65..128, rows of 65..512 non-zeros; beyond 512 wrmf_ne.hip again
   _scaled_rows() marks exactly those rows: they are held to the oracle bound, and how many of them differ is printed (where
   none does -- seen for CG at rank 64 and Cholesky at rank 16 -- the one-row handle's power of two happened to be the whole
   block's: a coincidence of the data).  Every other row is asserted: all rows of CG at rank 16, the rows of at most 512
   non-zeros of CG at ranks 64 and 128, the rows of at most 64 of Cholesky at rank 128 (wrmf_chol_lr.hip takes max |F| and the
   Gramian's exponent only), all rows of NNLS and of cg_steps = 0, the empty rows everywhere.  Explicit feedback has no
   confidence in its operand terms (wmax = 1, max |F| over the whole replica).
C. the exchanged max |F| (12 fixed-side vectors scaled by 2^8 / 2^12 inside ONE sub-block of one rank, long rows that hold them
   solved by other ranks) and the exchanged sum(F^2) / the counts of the dynamic regulariser read at the sub-block's offset.
D. the numeric counters summed over the rank threads: indefinite but regular systems, exact fallback count at 1 / 4 / 8 ranks.
E. the lifecycle: set_matrix drops the factors, a reused context equals a fresh one bit for bit, refused arguments leave the
   context usable.

Every test prints its figures before it asserts (pytest -s, lines starting with `ctx_rows`): profiles/ctx_rows/README.md."""
import ctypes
import time

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import wrmf_oracle as O
from rsparse_amd import _lib, engine
from test_bias_exact_rows import _row_err

gpu = pytest.mark.gpu
TOL = 1e-4
LENGTHS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320, 321, 384, 385, 511, 512, 513]
N_FIXED = 700
CELLS = [(1, 1, 1), (2, 0, 0), (3, 2, 5), (4, 3, 2), (5, 7, 3), (8, 8, 4), (8, 1, 1), (8, 40, 1)]
SOLVER = {"cholesky": 0, "conjugate_gradient": 1, "nnls": 2}
# feedback, solver, cg_steps, dynamic_lambda, lambda, ranks.  NNLS: the regularisers of tests/test_nnls_rows.py (with lambda = 0.1
# the reference's own coordinate descent is not converged on the shortest rows and no per-row bound means anything)
VARIANTS = {
    "implicit_cg3": ("implicit", "conjugate_gradient", 3, True, 0.1, (16, 64, 128)),
    "implicit_cg1": ("implicit", "conjugate_gradient", 1, True, 0.1, (16, 64, 128)),
    "implicit_cg0": ("implicit", "conjugate_gradient", 0, True, 0.1, (16, 64, 128)),
    "implicit_chol": ("implicit", "cholesky", 3, True, 0.1, (16, 64, 128)),
    "implicit_nnls": ("implicit", "nnls", 3, True, 1.0, (16, 64)),
    "explicit_cg_dyn": ("explicit", "conjugate_gradient", 3, True, 0.1, (16, 64, 128)),
    "explicit_cg_plain": ("explicit", "conjugate_gradient", 3, False, 0.1, (16, 64, 128)),
    "explicit_chol": ("explicit", "cholesky", 3, True, 0.1, (16, 64, 128)),
    "explicit_nnls": ("explicit", "nnls", 3, True, 0.5, (16, 64)),
}


def _scaled_rows(variant, k, lens):
    """B: the rows whose kernel scales fp16 operand terms by the handle's own max c (the table in the module text)"""
    if variant in ("implicit_cg3", "implicit_cg1"):
        return (lens > 512) if (32 < k <= 128 and k % 4 == 0) else np.zeros(len(lens), dtype=bool)
    if variant == "implicit_chol":
        return (lens > 0) if k <= 64 else (lens > 64)
    return np.zeros(len(lens), dtype=bool)


def _report(tag, **figures):
    print("ctx_rows %s %s" % (tag, " ".join("%s=%s" % (n, ("%.3g" % v) if isinstance(v, float) else v) for n, v in figures.items())))


# ---------------------------------------------------------------------------------------------------------------------------
# problems and their oracle results (computed once per feedback, solver, rank and side; read-only afterwards)
# ---------------------------------------------------------------------------------------------------------------------------

def _lattice(per_length=4, seed=4100):
    lens = np.repeat(np.asarray(LENGTHS, dtype=np.int64), per_length)
    np.random.default_rng(seed).shuffle(lens)
    cut = int(np.searchsorted(np.cumsum(lens), lens.sum() // 2))          # the row that reaches half of the non-zeros
    return np.concatenate([[0], lens[:cut + 1], [0, 0, 0], lens[cut + 1:], [0]]).astype(np.int64)


def _pattern(lens, n_fixed, rng, weights=None):
    """p, i of a CSC whose column c holds lens[c] distinct ids of the fixed side, ascending"""
    cols = [np.sort(rng.choice(n_fixed, size=int(n), replace=False, p=weights)) for n in lens]
    p = np.zeros(len(lens) + 1, dtype=np.int32)
    p[1:] = np.cumsum([c.size for c in cols])
    i = (np.concatenate(cols) if cols else np.zeros(0)).astype(np.int32)
    return p, i


def _matrix_of(q):
    """users x items: the solved rows are the users (side = "users") or, transposed, the items"""
    n_s, n_f = len(q["lens"]), q["F"].shape[0]
    if q["side"] == "users":
        return sp.csr_matrix((q["x"], q["i"], q["p"]), shape=(n_s, n_f))
    return sp.csc_matrix((q["x"], q["i"], q["p"]), shape=(n_f, n_s))


def _oracle(q, dt):
    """one half-iteration of the oracle in dtype dt on the fp32 inputs of q -> (solved factors k x n, loss)"""
    X = np.asfortranarray(q["F"].T, dtype=dt)
    Y = np.asfortranarray(q["S0"].T, dtype=dt).copy(order="F")
    sc = SOLVER[q["solver"]]
    if q["feedback"] == "implicit":
        loss = O.als_implicit(q["p"], q["i"], q["x"], X, Y, O.gramian(X, q["lam"]), q["lam"], sc, q["cg_steps"], n_threads=4)
    else:
        cnt = np.bincount(q["i"], minlength=X.shape[1]).astype(dt)
        loss = O.als_explicit(q["p"], q["i"], q["x"], X, Y, cnt, q["lam"], sc, q["cg_steps"], q["dyn"], n_threads=4)
    return np.asarray(Y, dtype=np.float64), float(loss)


def _finish(q):
    q["Y64"], q["l64"] = _oracle(q, np.float64)
    Y32, q["l32"] = _oracle(q, np.float32)
    q["e32"] = _row_err(Y32, q["Y64"])
    q["x_sp"] = _matrix_of(q)
    for a in q.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return q


def _factors(rng, n, k, scale, nonneg):
    a = (rng.standard_normal((n, k)) * scale).astype(np.float32)
    return np.abs(a) if nonneg else a


def _scale(feedback, k):
    # explicit feedback above rank 32: a factor vector keeps the norm it has at rank 32 (tests/test_nnls_rows.py, EXPLICIT_NORM)
    return 0.1 if feedback == "implicit" else min(0.3, 1.7 / np.sqrt(k))


_cache = {}


def _problem(variant, k, side, lens=None, tag="A", weights=None, lam=None, scale=None):
    key = (tag, variant, k, side)
    if key not in _cache:
        feedback, solver, cg_steps, dyn, lam0, _ = VARIANTS[variant]
        lens = _lattice() if lens is None else np.asarray(lens, dtype=np.int64)
        seed = 9000 + 31 * k + 7 * sorted(VARIANTS).index(variant) + (side == "items")
        rng = np.random.default_rng(seed)
        p, i = _pattern(lens, N_FIXED, rng, weights)
        if feedback == "implicit":
            x = (1.0 + rng.gamma(1.0, 2.0, size=i.size)).astype(np.float32).astype(np.float64)
        else:
            x = rng.integers(1, 6, size=i.size).astype(np.float64)
        sc = _scale(feedback, k) if scale is None else scale
        q = dict(variant=variant, k=k, side=side, lens=lens, p=p, i=i, x=x, feedback=feedback, solver=solver, cg_steps=cg_steps,
                 dyn=dyn, lam=lam0 if lam is None else lam, F=_factors(rng, N_FIXED, k, sc, False),
                 S0=_factors(rng, len(lens), k, sc, solver == "nnls"))
        _cache[key] = _finish(q)
    return _cache[key]


def _premises(tag, q, cap=0.05, guards=True):
    """from the oracle alone, before a device call -> (per-row bound, loss bound)"""
    lens, Y64, S0 = q["lens"], q["Y64"], np.asarray(q["S0"].T, dtype=np.float64)
    bound = np.maximum(TOL, 3.0 * q["e32"])
    share = float((bound > TOL).mean())
    l32err = abs(q["l32"] - q["l64"]) / abs(q["l64"])
    full = lens > 0
    moved = _row_err(S0, Y64)            # |S0 - Y64| / |Y64|
    Yn = Y64[:, full]
    nrm = np.linalg.norm(Yn, axis=0)
    gram = Yn.T @ Yn
    d2 = nrm[:, None] ** 2 + nrm[None, :] ** 2 - 2.0 * gram
    apart = np.sqrt(np.maximum(d2, 0.0)) / np.maximum(np.maximum(nrm[:, None], nrm[None, :]), 1e-300)
    np.fill_diagonal(apart, np.inf)
    _report(tag + " premises", oracle32_worst=float(q["e32"].max()), oracle32_worst_len=int(lens[q["e32"].argmax()]),
            rows_above_tol=int((bound > TOL).sum()), rows=len(lens), oracle32_loss_err=float(l32err),
            moved_min_over_bound=float((moved / bound)[full].min()), apart_min=float(apart.min()))
    assert np.all(np.isfinite(Y64)) and np.isfinite(q["l64"])
    assert share <= cap, share
    if not guards:
        return bound, max(TOL, 3.0 * l32err)
    if q["solver"] == "conjugate_gradient" and q["cg_steps"] == 0:
        assert np.array_equal(Y64[:, full], S0[:, full])
    else:
        assert np.all(moved[full] >= 10.0 * bound[full]), float((moved / bound)[full].min())
    assert apart.min() >= 1e-2, float(apart.min())
    return bound, max(TOL, 3.0 * l32err)


def _predicted_info(q, ranks, n_sub):
    """what rsparse_hip_ctx_info must say, from engine.balanced_bounds / engine.Layout"""
    x = q["x_sp"]
    cnt_u, cnt_i = np.diff(sp.csr_matrix(x).indptr), np.diff(sp.csc_matrix(x).indptr)
    out = {"ranks": ranks, "n_user": x.shape[0], "n_item": x.shape[1], "nnz": int(x.nnz), "rank": q["k"]}
    for name, cnt, ns in (("users", cnt_u, n_sub[0]), ("items", cnt_i, n_sub[1])):
        lay = engine.Layout(len(cnt), engine.balanced_bounds(cnt, ranks), ns if ns > 0 else engine.default_subblocks(ranks))
        out["n_sub_" + name], out["rows_per_sub_" + name] = lay.n_sub, lay.Bs
        out[name + "_rank0"] = lay.bounds[0][1] - lay.bounds[0][0]
    return out


def _run(q, ranks, ns_solved, ns_fixed, F=None, want_counts=False):
    """set_matrix, set_factors, get_factors, info, one half-iteration, get_factors on a fresh context"""
    from rsparse_amd.ctx import MultiGpuALS
    users = q["side"] == "users"
    n_sub = (ns_solved, ns_fixed) if users else (ns_fixed, ns_solved)
    F = q["F"] if F is None else F
    U0, V0 = (q["S0"], F) if users else (F, q["S0"])
    ctx = MultiGpuALS(ranks, comm="shared")
    try:
        ctx.set_matrix(q["x_sp"], n_sub=n_sub)
        ctx.set_factors(U0, V0)
        Ui, Vi = ctx.get_factors()
        info = ctx.info()
        loss = ctx.half_iteration(q["side"], q["feedback"], q["lam"], q["solver"], q["cg_steps"], q["dyn"])
        U, V = ctx.get_factors()
        counts = (ctx.numeric_counts(), ctx.numeric_counts()) if want_counts else None
    finally:
        ctx.close()
    identity = np.array_equal(Ui, U0) and np.array_equal(Vi, V0)
    want = _predicted_info(q, ranks, n_sub)
    info_ok = all(info[key] == v for key, v in want.items())
    S, Fb = (U, V) if users else (V, U)
    return dict(S=np.ascontiguousarray(S.T), fixed_same=np.array_equal(Fb, F), loss=loss, identity=identity, info_ok=info_ok,
                info=info, want=want, counts=counts)


def _judge(tag, q, res, bound, lbound, t0, bad, **more):
    """prints the cell's figures and appends what is wrong with it to `bad`"""
    err = _row_err(np.asarray(res["S"], dtype=np.float64), q["Y64"])
    worst = int(np.argmax(err / bound))
    lerr = abs(res["loss"] - q["l64"]) / abs(q["l64"])
    _report(tag, worst_ratio=float(err[worst] / bound[worst]), worst_len=int(q["lens"][worst]), worst_row=worst, err=float(err[worst]),
            oracle32_worst=float(q["e32"].max()), rows_above_tol=int((bound > TOL).sum()), loss_err=float(lerr),
            loss_bound=float(lbound), wall_s=float(time.perf_counter() - t0), **more)
    if not (np.all(np.isfinite(res["S"])) and np.isfinite(res["loss"])):
        bad.append((tag, "non-finite"))
    if not np.all(err <= bound):
        bad.append((tag, "row %d of %d non-zeros: err %.3g bound %.3g" % (worst, int(q["lens"][worst]), err[worst], bound[worst])))
    if not lerr <= lbound:
        bad.append((tag, "loss %.12g oracle %.12g" % (res["loss"], q["l64"])))
    if not res["fixed_same"]:
        bad.append((tag, "the fixed side changed"))
    if not res["identity"]:
        bad.append((tag, "set_factors -> get_factors is not the identity"))
    if not res["info_ok"]:
        bad.append((tag, "info %r != %r" % ({n: res["info"][n] for n in res["want"]}, res["want"])))


# ---------------------------------------------------------------------------------------------------------------------------
# A + B. layout cells
# ---------------------------------------------------------------------------------------------------------------------------

CASES_A = [(v, k, side) for v in VARIANTS for k in VARIANTS[v][5] for side in ("users", "items")]
CASES_A.append(("implicit_cg3", 100, "users"))       # a padded rank: run on the (4, 3, 2) cell and the one-rank cell only
CASES_A.append(("explicit_chol", 100, "items"))


def test_the_lattice_has_its_empty_rows_where_the_text_says():
    lens = _lattice()
    assert len(lens) == 4 * len(LENGTHS) + 5 and lens[0] == 0 and lens[-1] == 0
    (a0, a1), (b0, b1) = engine.balanced_bounds(lens, 2)
    assert lens[a1 - 1] > 0 and np.all(lens[b0:b0 + 3] == 0) and lens[b0 + 3] > 0      # the second block begins with the empty rows
    for ranks, ns, _ in CELLS:                                                        # n_sub = 40: more sub-blocks than rows
        bounds = engine.balanced_bounds(lens, ranks)
        lay = engine.Layout(len(lens), bounds, ns if ns else engine.default_subblocks(ranks))
        if ns == 40:
            assert lay.Bs * 40 > max(b - a for a, b in bounds) + lay.Bs             # whole sub-blocks without a row


@gpu
@pytest.mark.parametrize("variant,k,side", CASES_A)
def test_rows_at_every_layout_cell(variant, k, side):
    """A and B of the module text, every cell of CELLS on one problem.

    What this test found (profiles/ctx_rows/README.md): explicit Cholesky came back with NaN on every row of at most 64
    non-zeros of a rank's FIRST sub-block, in about one run of ten.  A host thread's first call zeroed its workspace with
    hipMemset, which runs on the null stream and may return before it has run; the rank threads work on non-blocking streams,
    which the null stream does not order, so the zeroing of the statistics block could land between the scan of max |F| and
    the kernels that scale their fp16 operand terms by it.  The workspace now waits for its zeroing."""
    t_all = time.perf_counter()
    q = _problem(variant, k, side)
    tag = "A %s k=%d %s" % (variant, k, side)
    bound, lbound = _premises(tag, q)
    cells = CELLS if k != 100 else [(1, 1, 1), (4, 3, 2)]
    bad, got = [], {}
    for cell in cells:
        t0 = time.perf_counter()
        res = _run(q, *cell)
        got[cell] = res
        more = {}
        if q["feedback"] == "explicit":                      # B: no Gramian, so nothing of the rank count enters
            more["same_bits_as_one_rank"] = bool(np.array_equal(res["S"], got[(1, 1, 1)]["S"]))
            if not more["same_bits_as_one_rank"]:
                bad.append((tag, cell, "explicit factors differ from the one-rank run"))
        elif cell == (8, 40, 1):                             # B: the same fixed side's sub-blocks, another solved side's
            differs = np.any(res["S"] != got[(8, 1, 1)]["S"], axis=0)
            scaled = _scaled_rows(variant, k, q["lens"])
            more.update(same_bits_as_8_1_1=bool(not differs.any()), scaled_rows=int(scaled.sum()),
                        scaled_rows_differing=int((differs & scaled).sum()), other_rows_differing=int((differs & ~scaled).sum()))
            if (differs & ~scaled).any():
                worst_len = sorted(set(q["lens"][differs & ~scaled].tolist()))
                bad.append((tag, cell, "implicit rows of %r non-zeros depend on the solved side's sub-block count" % worst_len))
        _judge("%s cell=%d,%d,%d" % ((tag,) + cell), q, res, bound, lbound, t0, bad, **more)
    _report(tag + " total", wall_s=float(time.perf_counter() - t_all))
    assert not bad, bad


def _unbalanced():
    """200 x 200: user 5 holds every item, item 7 every user, a shifted diagonal (no two rows or columns with the same pattern)
    and 100 entries at random -- each of the two hubs owns more than a quarter of the non-zeros, so at 8 ranks two of the
    balanced targets fall inside it and a rank is left without users, another without items"""
    rng = np.random.default_rng(9)
    n = 200
    rows = np.concatenate([np.full(n, 5), np.arange(n), np.arange(n), rng.integers(0, n, 100)])
    cols = np.concatenate([np.arange(n), np.full(n, 7), (np.arange(n) + 37) % n, rng.integers(0, n, 100)])
    x = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(n, n))
    x.sum_duplicates()
    x.data = (1.0 + rng.gamma(2.0, 1.0, size=x.data.size)).astype(np.float32).astype(np.float64)   # (no two rows alike)
    return x


@gpu
@pytest.mark.parametrize("variant,k", [("implicit_cg3", 64), ("implicit_chol", 16), ("explicit_cg_dyn", 128), ("explicit_chol", 64),
                                       ("implicit_nnls", 16)])
@pytest.mark.parametrize("side", ["users", "items"])
def test_rows_when_ranks_own_nothing(variant, k, side):
    """8 ranks, (8, 4) sub-blocks: every collective is entered by every rank, and the rows of the ranks that do own some are right"""
    t0 = time.perf_counter()
    key = ("A-empty", variant, k, side)
    if key not in _cache:
        feedback, solver, cg_steps, dyn, lam, _ = VARIANTS[variant]
        x = _unbalanced()
        m = sp.csc_matrix(x.T if side == "users" else x)          # columns = the solved rows
        m.sort_indices()
        rng = np.random.default_rng(9100 + k)
        n_f, n_s = m.shape
        sc = _scale(feedback, k)
        q = dict(variant=variant, k=k, side=side, lens=np.diff(m.indptr).astype(np.int64), p=m.indptr.astype(np.int32),
                 i=m.indices.astype(np.int32), x=m.data.astype(np.float64), feedback=feedback, solver=solver, cg_steps=cg_steps, dyn=dyn,
                 lam=lam, F=_factors(rng, n_f, k, sc, False), S0=_factors(rng, n_s, k, sc, solver == "nnls"))
        _cache[key] = _finish(q)
        _cache[key]["x_sp"] = x
    q = _cache[key]
    cnt_u, cnt_i = np.diff(sp.csr_matrix(q["x_sp"]).indptr), np.diff(sp.csc_matrix(q["x_sp"]).indptr)
    assert any(a == b for a, b in engine.balanced_bounds(cnt_u, 8)) and any(a == b for a, b in engine.balanced_bounds(cnt_i, 8))
    tag = "A-empty %s k=%d %s" % (variant, k, side)
    bound, lbound = _premises(tag, q)
    bad = []
    ns = (8, 4) if side == "users" else (4, 8)
    _judge(tag, q, _run(q, 8, *ns), bound, lbound, t0, bad)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------
# C. the exchanged max |F| and sum(F^2)
# ---------------------------------------------------------------------------------------------------------------------------

N_HUGE = 12
# The 12 vectors are part of the Gramian, whose condition number grows with ratio^2 |x|^2 / lambda.  With the lattice's factors
# N(0, 0.1^2) the exact solve is beyond fp32 itself (fp32 oracle: 8e-3 per row at 2^8, no digit left at 2^12 -- the finding of
# test_factor_rows_of_very_different_norms_on_the_fp16_paths), and no bound taken from it means anything.  N(0, (2e-5)^2) keeps
# the scaled vectors at a norm of 0.9 against lambda = 0.1: the fp32 oracle stays at or below 3.2e-5 on every row at both ratios
# and both solvers, so the 5 % cap and both guards hold as on the lattice.  What the kernels scale by is the RATIO to the
# global max |F|, which this does not change.
C_MAX_SCALE = 2e-5


def _huge_ids(q, ranks, ns_fixed, where):
    """12 fixed-side ids inside ONE sub-block: the last non-empty sub-block of the last rank that owns rows, or rank 0's first"""
    cnt = np.bincount(q["i"], minlength=N_FIXED)
    bounds = engine.balanced_bounds(cnt, ranks)
    lay = engine.Layout(N_FIXED, bounds, ns_fixed)
    if where == "first":
        r, j = 0, 0
    else:
        r = max(r for r in range(ranks) if bounds[r][1] > bounds[r][0])
        j = max(j for j in range(ns_fixed) if lay.sub_rows(r, j)[1] > lay.sub_rows(r, j)[0])
    c0, c1 = lay.sub_rows(r, j)
    assert c1 - c0 >= N_HUGE, (c0, c1)
    ids = bounds[r][0] + c0 + np.arange(N_HUGE)
    return ids, r, bounds


@gpu
@pytest.mark.parametrize("where", ["last", "first"])
@pytest.mark.parametrize("ratio", [2.0 ** 8, 2.0 ** 12])
@pytest.mark.parametrize("solver", ["conjugate_gradient", "cholesky"])
def test_max_abs_of_one_sub_block_reaches_every_rank(solver, ratio, where):
    """Implicit, rank 128.  The long-row kernels scale their fp16 operand terms by the max |F| that rides along with the Gramian
    partials: 12 fixed-side vectors, all in one sub-block of one rank, are `ratio` times the others, and rows of more than 512
    non-zeros that hold them are solved by OTHER ranks -- a rank that took its own maximum would overflow or flush those terms."""
    variant = "implicit_cg3" if solver == "conjugate_gradient" else "implicit_chol"
    ns_fixed, ns_solved = 3, 2
    bad = []
    for ranks in (4, 8):
        t0 = time.perf_counter()
        key = ("C-max", variant, ratio, where, ranks)
        if key not in _cache:
            base = _problem(variant, 128, "users", tag="C-max-base", scale=C_MAX_SCALE)
            # the rows of 513 non-zeros all hold the 12.  Moving entries moves the fixed side's counts and with them its cuts: the
            # ids are taken from the pattern they are put into (a fixed point, reached in a few rounds)
            rng = np.random.default_rng(300 + ranks)
            p, long_rows = base["p"], np.flatnonzero(base["lens"] > 512)
            pick, ids = base, None
            for _ in range(8):
                new_ids, owner, _ = _huge_ids(pick, ranks, ns_fixed, where)
                if ids is not None and np.array_equal(new_ids, ids):
                    break
                ids, i = new_ids, base["i"].copy()
                for c in long_rows:
                    row = i[p[c]:p[c + 1]]
                    others = rng.permutation(np.setdiff1d(row, ids))[:row.size - N_HUGE]
                    i[p[c]:p[c + 1]] = np.sort(np.concatenate([others, ids]))
                pick = dict(i=i)
            F = base["F"].copy()
            F[ids] *= np.float32(ratio)
            q = dict(base, i=i, F=F)
            for name in ("Y64", "l64", "l32", "e32", "x_sp"):
                q.pop(name)
            q = _finish(q)
            q["ids"], q["owner"] = ids, owner
            _cache[key] = q
        q = _cache[key]
        ids, owner, bounds = _huge_ids(q, ranks, ns_fixed, where)
        assert np.array_equal(ids, q["ids"])                       # moving the entries did not move the cuts enough to matter
        long_rows = np.flatnonzero(q["lens"] > 512)
        sb = engine.balanced_bounds(q["lens"], ranks)
        solvers_of_long = {r for c in long_rows for r in range(ranks) if sb[r][0] <= c < sb[r][1]}
        assert all(np.all(np.isin(ids, q["i"][q["p"][c]:q["p"][c + 1]])) for c in long_rows)
        assert solvers_of_long - {owner}, (solvers_of_long, owner)
        tag = "C-max %s ratio=2^%d %s ranks=%d" % (solver, int(np.log2(ratio)), where, ranks)
        bound, lbound = _premises(tag, q)
        _judge(tag, q, _run(q, ranks, ns_solved, ns_fixed), bound, lbound, t0, bad, owner=owner,
               long_rows_elsewhere=len(solvers_of_long - {owner}))
    assert not bad, bad


def _reg_explicit(q, cnt, ranks, ns_fixed, shift):
    """sum over the fixed side of count x |F row|^2 as the context forms it: per rank and sub-block, the counts read at the
    sub-block's first local row (shift = False) or, wrongly, at the block's first row for every sub-block (shift = True)"""
    bounds = engine.balanced_bounds(cnt, ranks)
    lay = engine.Layout(len(cnt), bounds, ns_fixed)
    sq = (np.asarray(q["F"], dtype=np.float64) ** 2).sum(axis=1)
    total = 0.0
    for r, (g0, g1) in enumerate(bounds):
        for j in range(ns_fixed):
            c0, c1 = lay.sub_rows(r, j)
            w = cnt[g0:g0 + (c1 - c0)] if shift else cnt[g0 + c0:g0 + c1]
            total += float(np.dot(w, sq[g0 + c0:g0 + c1]))
    return total


@gpu
@pytest.mark.parametrize("k", [16, 64])
@pytest.mark.parametrize("side", ["users", "items"])
def test_dynamic_regulariser_reads_the_counts_of_its_own_sub_block(k, side):
    """Explicit feedback, dynamic_lambda = 1: the loss's regulariser is lambda x sum_g count(g) |F_g|^2 over the FIXED side, formed
    per rank and sub-block and all-reduced.  The fixed side's popularity falls steeply with the id, so the sub-blocks of a rank
    have very different counts; lambda = 2 makes the regulariser a tenth of the loss or more; counts read one sub-block off move
    the loss by more than 10 x the loss bound (all asserted on the CPU first)."""
    t0 = time.perf_counter()
    w = 1.0 / (1.0 + np.arange(N_FIXED)) ** 0.8
    q = _problem("explicit_cg_dyn", k, side, tag="C-sumsq", weights=w / w.sum(), lam=2.0)
    tag = "C-sumsq k=%d %s" % (k, side)
    bound, lbound = _premises(tag, q)
    cnt = np.bincount(q["i"], minlength=N_FIXED).astype(np.float64)
    nnz = float(q["p"][-1])
    bad = []
    for ranks, ns_fixed in ((4, 3), (8, 5)):
        reg = _reg_explicit(q, cnt, ranks, ns_fixed, False)
        off = _reg_explicit(q, cnt, ranks, ns_fixed, True)
        share = q["lam"] * reg / nnz / q["l64"]
        moved = abs(q["lam"] * (off - reg) / nnz) / abs(q["l64"])
        _report(tag + " ranks=%d premises" % ranks, regulariser_share=float(share), one_sub_block_off=float(moved), loss_bound=float(lbound))
        assert abs(reg - float(np.dot(cnt, (np.asarray(q["F"], dtype=np.float64) ** 2).sum(axis=1)))) <= 1e-9 * reg
        assert share >= 0.10, share
        assert moved > 10.0 * lbound, (moved, lbound)
        _judge(tag + " ranks=%d" % ranks, q, _run(q, ranks, 2, ns_fixed), bound, lbound, t0, bad)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------
# D. the numeric counters over the ranks
# ---------------------------------------------------------------------------------------------------------------------------

N_FIXED_D = 600


@gpu
@pytest.mark.parametrize("k", [16, 64, 128])
def test_fallback_rows_are_counted_once_over_the_ranks(k):
    """Implicit Cholesky.  Half of the rows hold the value -3 on 450 of the 600 fixed-side rows: G + sum (c - 1) x x^T is negative
    definite (every eigenvalue, asserted in float64) and regular (condition numbers 2 .. 2.5 at rank 16, 5.5 .. 8.3 at rank 64,
    23 .. 142 at rank 128) -- every exact kernel meets a
    non-positive pivot and hands the row to the general solver, on whichever rank thread solves it.  The counters are
    thread_local per rank thread: summed over the ranks they give the number of such rows exactly, nothing unresolved, and (0, 0)
    on the second call.  Indefinite rows: max(1e-4, 20 cond 6e-8) as in tests/test_bias_exact_rows.py; the others: the bound
    above."""
    key = ("D", k)
    if key not in _cache:
        rng = np.random.default_rng(7700 + k)
        pd = np.repeat(np.asarray(LENGTHS, dtype=np.int64), 2)
        lens = np.concatenate([pd, np.full(pd.size, 450, dtype=np.int64)])
        order = rng.permutation(lens.size)
        lens, indef = lens[order], (np.arange(2 * pd.size) >= pd.size)[order]
        p, i = _pattern(lens, N_FIXED_D, rng)
        x = (1.0 + rng.gamma(1.0, 2.0, size=i.size)).astype(np.float32).astype(np.float64)
        x[np.repeat(indef, lens)] = -3.0
        q = dict(variant="implicit_chol", k=k, side="users", lens=lens, p=p, i=i, x=x, feedback="implicit", solver="cholesky",
                 cg_steps=3, dyn=True, lam=0.1, F=_factors(rng, N_FIXED_D, k, 0.3, False), S0=_factors(rng, lens.size, k, 0.3, False),
                 indef=indef)
        X = np.asarray(q["F"].T, dtype=np.float64)
        G = X @ X.T + np.float64(np.float32(0.1)) * np.eye(k)
        ev_max, cond = np.zeros(lens.size), np.ones(lens.size)
        for c in range(lens.size):
            idx, val = i[p[c]:p[c + 1]], x[p[c]:p[c + 1]]
            ev = np.linalg.eigvalsh(G + (X[:, idx] * (val - 1.0)) @ X[:, idx].T)
            ev_max[c], cond[c] = ev.max(), np.abs(ev).max() / np.abs(ev).min()
        q["ev_max"], q["cond"] = ev_max, cond
        _cache[key] = _finish(q)
    q = _cache[key]
    indef, cond, lens = q["indef"], q["cond"], q["lens"]
    n_indef = int(indef.sum())
    tag = "D k=%d" % k
    _report(tag + " premises", indefinite_rows=n_indef, ev_max_indef=float(q["ev_max"][indef].max()), cond_min=float(cond[indef].min()),
            cond_max=float(cond[indef].max()), oracle32_worst_indef_over_cond_eps=float((q["e32"] / (cond * 6e-8))[indef].max()),
            oracle32_worst_definite=float(q["e32"][~indef].max()))
    assert n_indef == len(lens) // 2
    assert np.all(q["ev_max"][indef] < 0.0) and cond[indef].max() <= 200.0         # indefinite, and regular
    bound = np.where(indef, np.maximum(TOL, 20.0 * cond * 6e-8), np.maximum(TOL, 3.0 * q["e32"]))
    assert (bound[~indef] > TOL).mean() <= 0.05
    _premises(tag + " guards", q)     # the common guards on ALL rows: the cap, moved from the warm start, no two solutions alike
    lbound = max(TOL, 3.0 * abs(q["l32"] - q["l64"]) / abs(q["l64"]))
    bad = []
    for ranks, ns in ((1, 1), (4, 3), (8, 8)):
        t0 = time.perf_counter()
        res = _run(q, ranks, ns, 2 if ranks > 1 else 1, want_counts=True)
        first, second = res["counts"]
        _judge(tag + " ranks=%d" % ranks, q, res, bound, lbound, t0, bad, unresolved=first[0], fallback=first[1], again=second)
        if first != (0, n_indef):
            bad.append((tag, ranks, "counters %r, expected (0, %d)" % (first, n_indef)))
        if second != (0, 0):
            bad.append((tag, ranks, "the second call returned %r" % (second,)))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------
# E. lifecycle
# ---------------------------------------------------------------------------------------------------------------------------

def _life_matrix(n_user, n_item, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, min(n_item, 60), size=n_user)
    p, i = _pattern(lens, n_item, rng)
    x = (1.0 + rng.gamma(1.0, 2.0, size=i.size)).astype(np.float32).astype(np.float64)
    return sp.csr_matrix((x, i, p), shape=(n_user, n_item))


def _life_factors(x, k, seed):
    rng = np.random.default_rng(seed)
    return _factors(rng, x.shape[0], k, 0.1, False), _factors(rng, x.shape[1], k, 0.1, False)


def _iterate(ctx, x, n_sub, U0, V0, set_matrix=True, solver="conjugate_gradient"):
    if set_matrix:
        ctx.set_matrix(x, n_sub=n_sub)
    ctx.set_factors(U0, V0)
    li = ctx.half_iteration("items", "implicit", 0.1, solver)
    lu = ctx.half_iteration("users", "implicit", 0.1, solver)
    U, V = ctx.get_factors()
    return U, V, (li, lu)


def _fresh(ranks, x, n_sub, U0, V0, solver="conjugate_gradient"):
    from rsparse_amd.ctx import MultiGpuALS
    ctx = MultiGpuALS(ranks, comm="shared")
    try:
        return _iterate(ctx, x, n_sub, U0, V0, solver=solver)
    finally:
        ctx.close()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _refused_without_factors(ctx):
    lib = ctx.lib
    loss = ctypes.c_double(0.0)
    assert lib.rsparse_hip_ctx_half_iteration(ctx.h, 1, 1, 0.1, 1, 3, 1, ctypes.byref(loss)) == _lib.ERR_INVALID
    n_user, n_item = ctx.shape
    U, V = np.zeros((n_user, 256), np.float32), np.zeros((n_item, 256), np.float32)   # (room for any rank: nothing may be written)
    assert lib.rsparse_hip_ctx_get_factors(ctx.h, U.ctypes.data_as(ctypes.c_void_p), V.ctypes.data_as(ctypes.c_void_p)) == _lib.ERR_INVALID
    assert not U.any() and not V.any()
    assert ctx.info()["rank"] == 0 and ctx.rank is None
    with pytest.raises(_lib.RsparseHipError):
        ctx.get_factors()


@gpu
def test_a_reused_context_equals_a_fresh_one():
    """One context at 4 ranks: matrix A, factors, an iteration; then a LARGER matrix on both sides at the same rank, a smaller one,
    the same matrix with other sub-block counts, another rank, set_factors twice.  After every set_matrix the context is without
    factors (half_iteration and get_factors: ERR_INVALID); after set_factors it gives the bits of a fresh context."""
    from rsparse_amd.ctx import MultiGpuALS
    t0 = time.perf_counter()
    k = 64
    A, B, C = _life_matrix(105, 300, 1), _life_matrix(230, 520, 2), _life_matrix(40, 90, 3)
    ctx = MultiGpuALS(4, comm="shared")
    try:
        steps = []
        fa = _life_factors(A, k, 11)
        steps.append(("A", _same(_iterate(ctx, A, (3, 2), *fa), _fresh(4, A, (3, 2), *fa))))
        for name, x, n_sub, kk in (("B larger", B, (3, 2), k), ("C smaller", C, (3, 2), k), ("C other n_sub", C, (7, 1), k),
                                   ("B again", B, (2, 5), k)):
            ctx.set_matrix(x, n_sub=n_sub)
            _refused_without_factors(ctx)
            f = _life_factors(x, kk, 12 + len(steps))
            steps.append((name, _same(_iterate(ctx, x, n_sub, *f, set_matrix=False), _fresh(4, x, n_sub, *f))))
        # another rank over the same matrix (set_factors alone reallocates), then the same rank twice
        for name, kk in (("rank 128", 128), ("rank 16", 16), ("rank 16 again", 16)):
            f = _life_factors(B, kk, 40 + kk + len(steps))
            steps.append((name, _same(_iterate(ctx, B, (2, 5), *f, set_matrix=False), _fresh(4, B, (2, 5), *f))))
        # set_factors twice in a row: the second pair is the one that counts
        f1, f2 = _life_factors(B, 16, 71), _life_factors(B, 16, 72)
        ctx.set_factors(*f1)
        steps.append(("set_factors twice", _same(_iterate(ctx, B, (2, 5), *f2, set_matrix=False), _fresh(4, B, (2, 5), *f2))))
    finally:
        ctx.close()
    _report("E reuse", wall_s=float(time.perf_counter() - t0), **{n.replace(" ", "_"): ok for n, ok in steps})
    assert all(ok for _, ok in steps), steps


@gpu
def test_refused_arguments_leave_a_one_rank_context_usable():
    """ONE rank (no collective can block): a pointer array that starts at 1, one that decreases, an index outside the matrix and
    solver code 7 each give ERR_INVALID with a message that names the trouble; the context then completes a fit that equals a
    fresh context's."""
    from rsparse_amd.ctx import MultiGpuALS
    t0 = time.perf_counter()
    k = 32
    A = _life_matrix(105, 300, 5)
    fa = _life_factors(A, k, 6)
    want = _fresh(1, A, (1, 1), *fa)
    ctx = MultiGpuALS(1, comm="shared")
    lib = ctx.lib
    try:
        before = _iterate(ctx, A, (1, 1), *fa)
        c_ui = sp.csc_matrix(A); c_ui.sort_indices()
        c_iu = sp.csc_matrix(c_ui.T); c_iu.sort_indices()
        good = [np.ascontiguousarray(a, dtype=t) for a, t in ((c_ui.indptr, np.int32), (c_ui.indices, np.int32), (c_ui.data, np.float64),
                                                                 (c_iu.indptr, np.int32), (c_iu.indices, np.int32), (c_iu.data, np.float64))]

        def set_matrix(arrays):
            return lib.rsparse_hip_ctx_set_matrix(ctx.h, A.shape[0], A.shape[1], *[a.ctypes.data_as(ctypes.c_void_p) for a in arrays], 1, 1)

        def changed(slot, edit):
            arrays = [a.copy() for a in good]
            edit(arrays[slot])
            return arrays

        def from_one(a):
            a[0] = 1

        def decrease(a):
            a[5] = a[6] + 1

        def out_of_range(a):
            a[3] = A.shape[0]

        for arrays, word in ((changed(0, from_one), b"ui_p"), (changed(3, from_one), b"iu_p"), (changed(0, decrease), b"ui_p decreases"),
                             (changed(3, decrease), b"iu_p decreases"), (changed(1, out_of_range), b"n_user")):
            assert set_matrix(arrays) == _lib.ERR_INVALID
            assert word in lib.rsparse_hip_last_error(), lib.rsparse_hip_last_error()
            # refused before anything was touched: the matrix and the factors of the context are still there
            U, V = ctx.get_factors()
            assert np.array_equal(U, before[0]) and np.array_equal(V, before[1])
        loss = ctypes.c_double(0.0)
        assert lib.rsparse_hip_ctx_half_iteration(ctx.h, 1, 1, 0.1, 7, 3, 1, ctypes.byref(loss)) == _lib.ERR_INVALID
        assert b"solver" in lib.rsparse_hip_last_error()
        assert lib.rsparse_hip_ctx_half_iteration(ctx.h, 1, 0, 0.1, 7, 3, 1, ctypes.byref(loss)) == _lib.ERR_INVALID
        U, V = ctx.get_factors()
        assert np.array_equal(U, before[0]) and np.array_equal(V, before[1])
        after = _iterate(ctx, A, (1, 1), *fa)
    finally:
        ctx.close()
    _report("E refused", wall_s=float(time.perf_counter() - t0))
    assert _same(before, want) and _same(after, want)
