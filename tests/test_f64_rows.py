"""precision = "double" on the device, per ROW, at the edges of the fp64 kernels' own loops (rsparse_amd/csrc/wrmf_f64.hip).

The other fp64 tests draw row lengths from synth.make_dataset or from small random shapes and never give a workgroup or a wave
a second row.  Here every row length and rank is chosen, and the matrices are large enough for both row loops to wrap:
    A. the wave-per-row conjugate gradient (f64_cg_wave_kernel, W = 16 / 32 / 64 and two coordinates per lane): RANKS_WAVE x
       {implicit, explicit with dynamic lambda, explicit without} x LENGTHS; cg_steps 0 / 1 / 5 at one rank per instantiation
    B. long rows at the PRODUCTION thresholds (more than 2048 non-zeros, chunks of 1024 = 16 inner chunks of 64 with metadata
       fetched two ahead): the lengths around 2048, 3072 and 4096, ranks 16 / 32 / 64 / 128, and the early exit of a chunked row
    C. the generic kernel (f64_als_kernel<64 / 256 / 512>): RANKS_GENERIC (the order k1 of the solved system) x LENGTHS for the
       Cholesky branch without and with user/item biases and a global bias, the generic conjugate-gradient branch (a global bias
       alone) and the re-packed explicit conjugate gradient with biases
    D. the general-solver fallback in all three geometries (ranks 24 / 48 / 100), with the number of fallback rows exact
    E. the SECOND pass of both row loops: kF64MaxGrid + 48 columns on the generic kernel, 4 kF64MaxGrid + 192 on the wave kernel

The reference is oracle.wrmf_oracle in double on the same inputs; every device call goes through als.als_implicit /
als.als_explicit with "double" (D counts its fallback rows through the device-resident entry, which is the only one that
reports them).  Bounds are those of tests/test_f64.py and no others: per row ||y - y_ref|| / ||y_ref|| < 1e-9 (Cholesky,
conjugate gradient) or 1e-6 (NNLS), loss 1e-9 (NNLS 1e-6) relative; D: max(1e-9, 50 cond 2.3e-16) per row and 1e-7 on the loss
(test_double_cholesky_falls_back_to_the_general_solver).  A bound means something only where double arithmetic can keep it,
so every parametrisation outside D first asserts, on the CPU, 50 cond 2.3e-16 < 1e-10 for the assembled system of every row.

Inputs: factors N(0, 0.1^2) (explicit feedback 0.3^2), lambda 0.1, confidences 1 + Gamma(1, 2) or ratings 1..5, as many items as
the longest row needs.  The columns lie in a shuffled order, every length twice.

Two combinations that would belong here cannot run: conjugate gradient with user/item biases on implicit feedback is refused by
the C ABI (and by the reference, wrmf_implicit.hpp:189,197), so the generic conjugate-gradient branch is reached through a
global bias alone; and with biases the rank counts two extra coordinates, so the largest biased system has order 127 (rank
128, the fp64 layer's limit) -- the biased variants meet "128" as that rank.

Every test prints its figures before it asserts (pytest -s, lines starting with `f64_rows`): profiles/f64_rows/README.md."""
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import wrmf_oracle as O

pytestmark = pytest.mark.gpu

CHOL, CG, NNLS = 0, 1, 2
LAMBDA = 0.1
TOL = 1e-9          # tests/test_f64.py, _bound(): Cholesky and conjugate gradient
TOL_NNLS = 1e-6     # ... NNLS
COND_RULE = 50.0 * 2.3e-16      # x cond: what double arithmetic can cost a row (test_double_cholesky_falls_back_...)

LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 66, 79, 80, 81, 95, 96, 97, 127, 128, 129,
           130, 191, 192, 193, 255, 256, 257]
RANKS_WAVE = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 71, 72, 73, 96, 127, 128]
RANKS_GENERIC = [1, 4, 7, 8, 9, 15, 16, 17, 20, 24, 28, 32, 33, 63, 64, 65, 72, 100, 112, 120, 121, 127, 128]
RANKS_EVERY_VARIANT = [8, 33, 64, 65, 100, 128]
N_ITEM = 260
MAX_RANK = 128      # RSPARSE_HIP_MAX_RANK_F64

_CSRC = Path(__file__).resolve().parent.parent / "rsparse_amd" / "csrc"


@pytest.fixture(autouse=True)
def _default_long_rows():
    yield
    _long_rows(0, 0)


def _long_rows(min_len, chunk_len):
    from rsparse_amd import _lib
    _lib.check(_lib.load().rsparse_hip_set_f64_long_rows(int(min_len), int(chunk_len)))


# ---------------------------------------------------------------------------------------------------------------------------
# helpers (the shape of test_nnls_rows / test_cg_rank_classes)
# ---------------------------------------------------------------------------------------------------------------------------

def _shuffled(lengths, seed):
    lens = np.asarray(lengths, dtype=np.int64)
    return lens[np.random.default_rng(seed).permutation(lens.size)]


def _rows_of_lengths(lengths, n_item, k, seed, scale, ratings=False, non_negative=False):
    """a CSC (columns = the rows to solve) whose column j has lengths[j] distinct random items, values 1 + Gamma(1, 2) or ratings
    1..5; factors and warm start N(0, scale^2) in double (their absolute values for NNLS, every third start all zeros)"""
    rng = np.random.default_rng(seed)
    p = np.zeros(len(lengths) + 1, dtype=np.int32)
    p[1:] = np.cumsum(lengths)
    idx = np.concatenate([np.sort(rng.choice(n_item, size=int(n), replace=False)) for n in lengths] +
                         [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    x = rng.integers(1, 6, idx.size).astype(np.float64) if ratings else 1.0 + rng.gamma(1.0, 2.0, size=idx.size)
    X = np.asfortranarray(rng.standard_normal((k, n_item)) * scale)
    Y0 = np.asfortranarray(rng.standard_normal((k, len(lengths))) * scale)
    if non_negative:
        X, Y0 = np.abs(X), np.abs(Y0)
        Y0[:, ::3] = 0.0
    return (n_item, len(lengths), p, idx, x), X, Y0


def _row_err(Y, Yref):
    return np.linalg.norm(Y - Yref, axis=0) / np.maximum(np.linalg.norm(Yref, axis=0), 1e-300)


def _report(tag, **figures):
    print("f64_rows %s %s" % (tag, " ".join("%s=%s" % (n, ("%.3g" % v) if isinstance(v, float) else v)
                                             for n, v in figures.items())))


def _freeze(q):
    for a in q.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return q


# a variant: feedback, solver, and the operands that change the row's system
def _variant(implicit, solver, dyn=False, bias=None, gbias=0.0, lam=LAMBDA):
    return dict(implicit=implicit, solver=solver, dyn=dyn, bias=bias is not None, bias_last=bool(bias), gbias=gbias, lam=lam,
                scale=0.1 if implicit else 0.3)


def _layout(v, k):
    """(first kept row of X, order of the system, row of X with the x biases or None, first written coordinate of Y) --
    wrmf_explicit.hpp:41-64,86-91, wrmf_implicit.hpp:114-154,186-252"""
    if not v["bias"]:
        return 0, k, None, 0
    return (0, k - 1, k - 1, 0) if v["bias_last"] else (1, k - 1, 0, 1)


def _gramian(v, X):
    if not v["implicit"]:
        return None
    xoff, k1, _, _ = _layout(v, X.shape[0])
    return O.gramian(np.asfortranarray(X[xoff:xoff + k1]), v["lam"])


def _systems(v, q):
    """the assembled k1 x k1 system of every column that is solved, in double (None: an empty column that is zeroed)"""
    X, G, p, i, x = q["X"], q["G"], q["p"], q["i"], q["x"]
    xoff, k1, _, _ = _layout(v, X.shape[0])
    Xp = X[xoff:xoff + k1]
    solve_empty = v["implicit"] and (v["bias"] or v["gbias"] != 0.0)
    out = []
    for c in range(len(p) - 1):
        idx, val = i[p[c]:p[c + 1]], x[p[c]:p[c + 1]]
        if len(idx) == 0 and not solve_empty:
            out.append(None)
        elif v["implicit"]:
            out.append(G + (Xp[:, idx] * (val - 1.0)) @ Xp[:, idx].T)
        else:
            out.append(Xp[:, idx] @ Xp[:, idx].T + v["lam"] * (len(idx) if v["dyn"] else 1.0) * np.eye(k1))
    return out


def _conditions(v, q):
    """cond_2 of every solved column's system (1 for a zeroed one) and its smallest eigenvalue"""
    cond, low = np.ones(len(q["lens"])), np.ones(len(q["lens"]))
    for c, A in enumerate(_systems(v, q)):
        if A is not None:
            ev = np.linalg.eigvalsh(A)
            cond[c], low[c] = np.abs(ev).max() / np.abs(ev).min(), ev.min()
    return cond, low


def _oracle(v, q, Y, cg_steps=3):
    """one half-iteration of the reference in double, Y in place; returns the loss"""
    if v["implicit"]:
        return O.als_implicit(q["p"], q["i"], q["x"], q["X"], Y, q["G"], v["lam"], v["solver"], cg_steps, n_threads=8,
                              with_biases=v["bias"], is_x_bias_last_row=v["bias_last"], global_bias=v["gbias"])
    return O.als_explicit(q["p"], q["i"], q["x"], q["X"], Y, q["cnt"], v["lam"], v["solver"], cg_steps, v["dyn"], n_threads=8,
                          with_biases=v["bias"], is_x_bias_last_row=v["bias_last"])


def _device(v, q, cg_steps=3, csc=None, Y0=None, cnt=None):
    from rsparse_amd import als
    Y = np.array(q["Y0"] if Y0 is None else Y0, order="F")
    X = np.array(q["X"], order="F")
    csc = (q["n_item"], len(q["lens"]), q["p"], q["i"], q["x"]) if csc is None else csc
    if v["implicit"]:
        loss = als.als_implicit(csc, X, Y, v["lam"], 1, v["solver"], cg_steps, "double", v["bias"], v["bias_last"],
                                global_bias=v["gbias"], XtX=np.array(q["G"], order="F"))
    else:
        loss = als.als_explicit(csc, X, Y, np.array(q["cnt"] if cnt is None else cnt), v["lam"], 1, v["solver"], cg_steps,
                                v["dyn"], "double", v["bias"], v["bias_last"])
    return Y, loss


_cache = {}


def _case(v, k, lengths, seed, n_item=N_ITEM, cg_steps=3, each_twice=True, values=None):
    """the lattice `lengths` (each twice, shuffled) at rank k (the leading dimension: with biases it counts the row of ones and
    the bias row) with the oracle's answer, the rows' condition numbers -- computed once per key and shared, read-only"""
    key = (tuple(sorted(v.items())), k, tuple(lengths), seed, n_item, cg_steps, each_twice, values)
    if key not in _cache:
        lens = _shuffled(list(lengths) * (2 if each_twice else 1), seed)
        (n_item, n_cols, p, i, x), X, Y0 = _rows_of_lengths(lens, n_item, k, seed + 1, v["scale"], ratings=not v["implicit"],
                                                            non_negative=v["solver"] == NNLS)
        if values is not None:          # D: confidences below and above 1
            x = np.where(np.random.default_rng(seed + 2).random(x.size) < 0.5, values[0], values[1])
        if v["bias"]:
            X[0 if v["bias_last"] else k - 1, :] = 1.0
            Y0[k - 1 if v["bias_last"] else 0, :] = 1.0
        q = dict(k=k, lens=lens, n_item=n_item, p=p, i=i, x=x, X=X, Y0=Y0, cnt=np.bincount(i, minlength=n_item).astype(np.float64))
        q["G"] = _gramian(v, X)
        if values is not None:          # D: a Gramian too weak to keep the rows positive definite
            q["G"] = np.asfortranarray(0.05 * (X @ X.T) + v["lam"] * np.eye(k))
        q["Yref"] = Y0.copy(order="F")
        q["lref"] = _oracle(v, q, q["Yref"], cg_steps)
        q["cond"], q["low"] = _conditions(v, q)
        _cache[key] = _freeze(q)
    return _cache[key]


def _assert_well_conditioned(v, q):
    """the project's conditioning rule an order under the bound, on the CPU, before the device is looked at"""
    worst = int(np.argmax(q["cond"]))
    assert COND_RULE * q["cond"][worst] < 1e-10, ("row of %d non-zeros" % int(q["lens"][worst]), float(q["cond"][worst]))
    assert q["low"].min() > 0.0


def _assert_rows_and_loss(tag, v, q, Y, loss, bound=None, loss_tol=None, Yref=None, lref=None, lens=None):
    Yref = q["Yref"] if Yref is None else Yref
    lref = q["lref"] if lref is None else lref
    lens = q["lens"] if lens is None else lens
    tol = TOL_NNLS if v["solver"] == NNLS else TOL
    bound = np.full(Yref.shape[1], tol) if bound is None else bound
    loss_tol = tol if loss_tol is None else loss_tol
    err = _row_err(Y, Yref)
    worst = int(np.argmax(err / bound))
    lerr = abs(loss - lref) / abs(lref)
    _report(tag, worst_row=worst, worst_len=int(lens[worst]), err=float(err[worst]), bound=float(bound[worst]),
            cond_max=float(q["cond"].max()), loss_err=float(lerr), loss_bound=float(loss_tol))
    assert np.all(np.isfinite(Y)) and np.isfinite(loss)
    assert np.all(err < bound), ("row of %d non-zeros" % int(lens[worst]), worst, float(err[worst]), float(bound[worst]))
    assert lerr <= loss_tol, (loss, lref)
    xoff, k1, xb, ooff = _layout(v, Yref.shape[0])
    empty = lens == 0
    if v["implicit"] and (v["bias"] or v["gbias"] != 0.0):
        # wrmf_implicit.hpp:178: the empty column is solved (and held to the bound above), not zeroed
        assert np.all(np.linalg.norm(Yref[ooff:ooff + k1, empty], axis=0) > 1e-6)
        assert np.all(np.linalg.norm(Y[ooff:ooff + k1, empty], axis=0) > 1e-6)
    else:
        assert np.all(Y[ooff:ooff + k1, empty] == 0.0) and np.all(Yref[ooff:ooff + k1, empty] == 0.0)
    if v["bias"]:
        keep = Yref.shape[0] - 1 if v["bias_last"] else 0
        assert np.all(Y[keep] == 1.0)                                  # the placeholder coordinate is never written


# ---------------------------------------------------------------------------------------------------------------------------
# A. the wave-per-row conjugate gradient
# ---------------------------------------------------------------------------------------------------------------------------

WAVE_VARIANTS = {
    "implicit": _variant(True, CG),
    "explicit_dynamic_lambda": _variant(False, CG, dyn=True),
    "explicit_plain_lambda": _variant(False, CG, dyn=False),
}


@pytest.mark.parametrize("variant", list(WAVE_VARIANTS))
@pytest.mark.parametrize("k", RANKS_WAVE)
def test_wave_kernel_every_rank_class_and_row_length(k, variant):
    """W = 16 (ranks 1..16), 32 (17..32), 64 (33..64) and two coordinates per lane with the packed-triangle Gramian (65..128);
    chunks of 64 non-zeros with the metadata two chunks ahead, 64 / W non-zeros per step in batches of 16 steps (16, 32 and 64
    non-zeros per batch), the first batch of the next chunk fetched across the boundary: every length of LENGTHS, twice."""
    v = WAVE_VARIANTS[variant]
    q = _case(v, k, LENGTHS, 2000 + k)
    _assert_well_conditioned(v, q)
    Y, loss = _device(v, q)
    _assert_rows_and_loss("A k=%d %s" % (k, variant), v, q, Y, loss)


@pytest.mark.parametrize("variant", ["implicit", "explicit_dynamic_lambda"])
@pytest.mark.parametrize("cg_steps", [0, 1, 5])
@pytest.mark.parametrize("k", [16, 32, 64, 128])
def test_wave_kernel_cg_steps(k, cg_steps, variant):
    """0 steps: the warm start comes back bit for bit (and the loss is the warm start's), empty rows as zeros; 1 and 5: the
    loop's first and a late iteration at every instantiation"""
    v = WAVE_VARIANTS[variant]
    q = _case(v, k, LENGTHS, 2200 + k, cg_steps=cg_steps)
    _assert_well_conditioned(v, q)
    Y, loss = _device(v, q, cg_steps=cg_steps)
    _assert_rows_and_loss("A k=%d %s cg_steps=%d" % (k, variant, cg_steps), v, q, Y, loss)
    if cg_steps == 0:
        live = q["lens"] > 0
        assert np.array_equal(Y[:, live], q["Y0"][:, live])
        assert np.all(q["Y0"][:, ~live] != 0.0) and np.all(Y[:, ~live] == 0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# B. long rows at the production thresholds
# ---------------------------------------------------------------------------------------------------------------------------

LENGTHS_LONG = [2047, 2048, 2049, 3071, 3072, 3073, 4097, 5000]
LENGTHS_SHORT = [0, 1, 5, 16, 17, 33, 63, 64, 65, 130, 193, 257]
N_ITEM_LONG = 5100


def _long_row_thresholds():
    """(kF64LongRowMin, kF64LongRowChunk) as the library's source states them"""
    text = (_CSRC / "wrmf_f64_capi.cpp").read_text()
    m = re.search(r"constexpr\s+int\s+kF64LongRowMin\s*=\s*(\d+)\s*,\s*kF64LongRowChunk\s*=\s*(\d+)\s*;", text)
    assert m, "kF64LongRowMin / kF64LongRowChunk are no longer where this test reads them"
    return int(m.group(1)), int(m.group(2))


def _assert_split(lens):
    """2048 stays with the wave-per-row kernel, 2049 is the first chunked row; chunks of more than one inner chunk of 64"""
    long_min, chunk = _long_row_thresholds()
    assert (long_min, chunk) == (2048, 1024)
    chunked = lens > long_min                                   # list_long_rows: `n <= lmin` stays
    assert long_min in lens and not chunked[lens == long_min].any()
    assert long_min + 1 in lens and chunked[lens == long_min + 1].all()
    assert chunked.sum() >= 6 and (~chunked & (lens > 0)).sum() >= 10
    tails = sorted(set(int(n % chunk) for n in lens[chunked]))  # a last chunk of 1 non-zero, of 1023, a whole one
    assert 1 in tails and chunk - 1 in tails and 0 in tails, tails
    return chunked


@pytest.mark.parametrize("variant", ["implicit", "explicit_dynamic_lambda"])
@pytest.mark.parametrize("k", [16, 32, 64, 128])
def test_long_rows_at_the_production_thresholds(k, variant):
    """Rows of 2049 .. 5000 non-zeros run as chunks of 1024 (16 inner chunks of 64: every phase of the two-ahead metadata and of
    the cross-chunk prefetch inside a chunk, which the lowered thresholds of tests/test_f64.py never reach), 2047 and 2048 on
    one wave.  The thresholds are the library's defaults: rsparse_hip_set_f64_long_rows(0, 0)."""
    _long_rows(0, 0)
    v = WAVE_VARIANTS[variant]
    q = _case(v, k, LENGTHS_LONG + LENGTHS_SHORT, 2400 + k, n_item=N_ITEM_LONG, each_twice=False)
    chunked = _assert_split(q["lens"])
    _assert_well_conditioned(v, q)
    Y, loss = _device(v, q)
    err = _row_err(Y, q["Yref"])
    _report("B k=%d %s chunked" % (k, variant), rows=int(chunked.sum()), worst_err=float(err[chunked].max()),
            worst_len=int(q["lens"][chunked][np.argmax(err[chunked])]))
    _assert_rows_and_loss("B k=%d %s" % (k, variant), v, q, Y, loss)


def test_long_rows_stop_like_short_ones_at_the_production_thresholds():
    """test_double_cg_long_rows_stop_like_short_ones with rows that are chunked by the DEFAULT thresholds: every item vector a
    unit coordinate vector, so every system is diagonal with at most 16 distinct entries and the residual of a row falls below
    CG_TOL within the 20 steps (wrmf_implicit.hpp:44) -- on the chunked path the flag lives in scratch between launches."""
    _long_rows(0, 0)
    v = _variant(True, CG)
    k, cg_steps = 16, 20
    lens = _shuffled(LENGTHS_LONG + LENGTHS_SHORT, 2500)
    chunked = _assert_split(lens)
    (n_item, n_cols, p, i, x), X, Y0 = _rows_of_lengths(lens, N_ITEM_LONG, k, 2501, 0.1)
    rng = np.random.default_rng(2502)
    X = np.zeros((k, n_item), order="F")
    X[rng.integers(0, k, n_item), np.arange(n_item)] = 1.0
    x = 1.0 + rng.random(x.size)
    q = dict(k=k, lens=lens, n_item=n_item, p=p, i=i, x=x, X=X, Y0=Y0, cnt=None)
    q["G"] = _gramian(v, X)
    q["Yref"] = Y0.copy(order="F")
    q["lref"] = _oracle(v, q, q["Yref"], cg_steps)
    q["cond"], q["low"] = _conditions(v, q)
    _assert_well_conditioned(v, q)
    # the rows do stop early: two steps fewer give the same answer
    Y18 = Y0.copy(order="F")
    _oracle(v, q, Y18, cg_steps - 2)
    assert np.array_equal(Y18, q["Yref"])
    Y, loss = _device(v, q, cg_steps=cg_steps)
    _report("B early-exit k=16", chunked_rows=int(chunked.sum()))
    _assert_rows_and_loss("B early-exit k=16", v, q, Y, loss)


# ---------------------------------------------------------------------------------------------------------------------------
# C. the generic kernel
# ---------------------------------------------------------------------------------------------------------------------------

GENERIC_FAMILIES = {
    # Cholesky: blocks of 8 columns with a non-FULL last block, the masked trailing tile, the back-substitution split at 64
    "cholesky": {
        "implicit": _variant(True, CHOL),
        "explicit_dynamic_lambda": _variant(False, CHOL, dyn=True),
    },
    "cholesky_biases": {
        "implicit_bias_last": _variant(True, CHOL, bias=True),
        "implicit_bias_first": _variant(True, CHOL, bias=False),
        "implicit_bias_last_global": _variant(True, CHOL, bias=True, gbias=0.03),
        "implicit_bias_first_global": _variant(True, CHOL, bias=False, gbias=0.03),
        "explicit_bias_last": _variant(False, CHOL, dyn=True, bias=True),
        "explicit_bias_first": _variant(False, CHOL, dyn=True, bias=False),
    },
    # conjugate gradient off the plain wave kernel: a global bias alone takes the generic kernel's CG branch (the only variant
    # that does: CG with biases on implicit feedback is refused), explicit feedback with biases is re-packed (f64_pack_rows /
    # f64_shift_values / f64_unpack_rows) and runs the wave kernel at order k1
    "conjugate_gradient": {
        "implicit_global": _variant(True, CG, gbias=0.03),
        "explicit_bias_last_repacked": _variant(False, CG, dyn=True, bias=True),
        "explicit_bias_first_repacked": _variant(False, CG, dyn=True, bias=False),
    },
}


def _generic_cases():
    """every variant at RANKS_EVERY_VARIANT; the other ranks of RANKS_GENERIC dealt out within each family, so that every rank
    meets every family"""
    cases = []
    rest = [r for r in RANKS_GENERIC if r not in RANKS_EVERY_VARIANT]
    for family, variants in GENERIC_FAMILIES.items():
        names = list(variants)
        for name in names:
            cases += [(family, name, r) for r in RANKS_EVERY_VARIANT]
        cases += [(family, names[j % len(names)], r) for j, r in enumerate(rest)]
    return cases


def test_generic_cases_cover_every_rank_and_variant():
    cases = _generic_cases()
    for family, variants in GENERIC_FAMILIES.items():
        assert sorted(set(r for f, n, r in cases if f == family)) == sorted(RANKS_GENERIC)
        for name in variants:
            assert set(RANKS_EVERY_VARIANT) <= set(r for f, n, r in cases if (f, n) == (family, name))
    assert len(set(cases)) == len(cases)


@pytest.mark.parametrize("family,variant,k1", _generic_cases())
def test_generic_kernel_every_rank_class_and_row_length(family, variant, k1):
    """k1 is the order of the solved system; with biases the rank is k1 + 1, and rank 128 (order 127) stands for "128" there.
    Orders 1..32 run 64 threads, 33..64 256, beyond 512; the staged chunk is 32 / 64 / 16 vectors depending on the rank, and
    LENGTHS has CH - 1, CH, CH + 1 and 2 CH + 1 for each of them."""
    v = GENERIC_FAMILIES[family][variant]
    k = min(k1 + 1, MAX_RANK) if v["bias"] else k1
    q = _case(v, k, LENGTHS, 3000 + k1)
    _assert_well_conditioned(v, q)
    Y, loss = _device(v, q)
    _assert_rows_and_loss("C %s k1=%d rank=%d" % (variant, k1, k), v, q, Y, loss)


# ---------------------------------------------------------------------------------------------------------------------------
# D. the general-solver fallback in every geometry
# ---------------------------------------------------------------------------------------------------------------------------

INDEFINITE = _variant(True, CHOL)
INDEFINITE["scale"] = 0.3
LENGTH_CLASSES = [(1, 16), (17, 64), (65, 128), (129, 1 << 30)]
D_SEEDS = {24: 4024, 48: 4048, 100: 4100, 40: 4040}


def _indefinite_case(k, lengths, each_twice=True):
    """test_double_cholesky_falls_back_to_the_general_solver's recipe on LENGTHS: confidences 0.25 / 3.0 against
    0.05 X X^T + 0.1 I.  Asserted on the CPU: at least 5 indefinite rows in at least three length classes, none with an
    eigenvalue within 1e-6 of zero (so that `Cholesky fails` and `indefinite` are the same rows), and at most 5 % of the rows
    with a bound above 1e-7."""
    q = _case(INDEFINITE, k, lengths, D_SEEDS[k], each_twice=each_twice, values=(0.25, 3.0))
    solved = q["lens"] > 0
    bad = solved & (q["low"] < 0.0)
    classes = set(c for c, (lo, hi) in enumerate(LENGTH_CLASSES) for n in q["lens"][bad] if lo <= n <= hi)
    assert bad.sum() >= 5 and len(classes) >= 3, (int(bad.sum()), classes)
    assert np.abs(q["low"][solved]).min() >= 1e-6, float(np.abs(q["low"][solved]).min())
    bound = np.maximum(TOL, COND_RULE * q["cond"])
    assert np.mean(bound > 1e-7) <= 0.05
    return q, bad, bound


@pytest.mark.parametrize("k", [24, 48, 100])
def test_fallback_to_the_general_solver_in_every_geometry(k):
    """64, 256 and 512 threads: the RT / CG split of the elimination (RT = 32, 64, 128 rows by 2, 4, 4 column groups) and the
    two-register back-substitution beyond coordinate 64.  Every indefinite row is re-solved, and only those."""
    import torch
    from rsparse_amd.engine import HipBackend
    v = INDEFINITE
    q, bad, bound = _indefinite_case(k, LENGTHS)
    Y, loss = _device(v, q)
    _report("D k=%d" % k, indefinite_rows=int(bad.sum()), lengths=",".join(str(n) for n in sorted(set(q["lens"][bad].tolist()))),
            bound_max=float(bound.max()))
    _assert_rows_and_loss("D k=%d" % k, v, q, Y, loss, bound=bound, loss_tol=1e-7)
    be = HipBackend()
    be.numeric_counts()                                             # (whatever an earlier call left)
    h = be.make_csc(q["n_item"], len(q["lens"]), be.to_device(np.array(q["p"]), torch.int32),
                    be.to_device(np.array(q["i"]), torch.int32), be.to_device(np.array(q["x"]), torch.float64))
    Xd = be.to_device(np.array(q["X"].T, order="C"), torch.float64)        # (copies: the shared case is read-only)
    Yd = be.to_device(np.array(q["Y0"].T, order="C"), torch.float64)
    lossd = torch.zeros(1, dtype=torch.float64, device=be.device)
    be.half_iteration(h, True, Xd, Yd, be.to_device(np.array(q["G"], order="C"), torch.float64), v["lam"], CHOL, 3, True, lossd)
    with pytest.warns(RuntimeWarning, match="general"):
        be.check_numeric()
    _report("D k=%d" % k, fallback_rows=int(be.last_fallback_rows), expected=int(bad.sum()))
    assert be.last_fallback_rows == int(bad.sum())
    assert np.array_equal(Yd.cpu().numpy().T, Y)


# ---------------------------------------------------------------------------------------------------------------------------
# E. the second pass of both row loops
# ---------------------------------------------------------------------------------------------------------------------------

N_DISTINCT = 48
MID_MAX_LEN = 33        # the columns that fill the middle of a tiled matrix: keeps its mean length under 40
LENGTHS_TILE = LENGTHS + [1, 2, 3, 4, 5, 7, 8, 9, 15, 16]
assert len(LENGTHS_TILE) == N_DISTINCT and LENGTHS_TILE.count(0) == 1


def _max_grid():
    """kF64MaxGrid as the kernels' header states it: if the constant moves, the test moves with it"""
    m = re.search(r"constexpr\s+int\s+kF64MaxGrid\s*=\s*(\d+)\s*\*\s*(\d+)\s*;", (_CSRC / "wrmf_f64.h").read_text())
    assert m, "kF64MaxGrid is no longer where this test reads it"
    return int(m.group(1)) * int(m.group(2))


def _tile(q, stride, tail):
    """the 48 distinct columns of q repeated up to stride + tail columns, every copy with the same items, values and warm
    start.  Both kernels walk the rows in natural order, `stride` rows per pass (kF64MaxGrid workgroups, or four waves in each of
    as many workgroups), so the rows of the second pass are the last `tail` columns and the row that the same workgroup or wave
    took first lies `stride` columns before.  Layout: tail = the 48 columns in order (four times over for the wave kernel);
    head = for the column of length rank r the column of rank 47 - r (shifted by 12 more in every further copy), so about half
    of the second-pass rows follow a longer row and half a shorter one; middle = the columns of at most 33 non-zeros, shuffled."""
    lens0 = q["lens"]
    n0 = len(lens0)
    assert n0 == N_DISTINCT and tail % n0 == 0
    by_len = np.argsort(lens0, kind="stable")
    rank_of = np.argsort(by_len)
    tail_src = np.tile(np.arange(n0), tail // n0)
    head_src = np.concatenate([by_len[(n0 - 1 - rank_of + 12 * m) % n0] for m in range(tail // n0)])
    short = np.flatnonzero(lens0 <= MID_MAX_LEN)
    n_mid = stride - tail
    mid = short[np.arange(n_mid) % len(short)]
    mid = mid[np.random.default_rng(stride).permutation(n_mid)]
    src = np.concatenate([head_src, mid, tail_src])
    assert src.size == stride + tail
    lens = lens0[src]
    p = np.zeros(src.size + 1, dtype=np.int32)
    p[1:] = np.cumsum(lens)
    starts = np.asarray(q["p"][:-1], dtype=np.int64)[src]
    pos = np.repeat(starts - p[:-1], lens) + np.arange(int(p[-1]))
    t = dict(src=src, lens=lens, p=p, i=np.ascontiguousarray(q["i"][pos]), x=np.ascontiguousarray(q["x"][pos]),
             Y0=np.asfortranarray(q["Y0"][:, src]))
    t["cnt"] = np.bincount(t["i"], minlength=q["n_item"]).astype(np.float64)
    return t


def _check_tiling(q, t, stride, tail, skipped_above=None):
    """from the lengths alone: what the second pass consists of"""
    n_total = stride + tail
    src, lens = t["src"], t["lens"]
    assert lens.size == n_total and lens.mean() <= 40.0 and set(src.tolist()) == set(range(N_DISTINCT))
    for c in (0, tail - 1, tail, n_total // 2, stride - 1, stride, n_total - 1):
        a, b = t["p"][c], t["p"][c + 1]
        a0, b0 = q["p"][src[c]], q["p"][src[c] + 1]
        assert np.array_equal(t["i"][a:b], q["i"][a0:b0]) and np.array_equal(t["x"][a:b], q["x"][a0:b0])
        assert np.array_equal(t["Y0"][:, c], q["Y0"][:, src[c]])
    second = np.arange(stride, n_total)
    first = second - stride
    sl, fl = lens[second], lens[first]
    assert (sl > 0).sum() >= 46 and len(set(sl[sl > 0].tolist())) >= 11
    assert np.mean(fl >= sl) >= 0.5 and (fl < sl).sum() >= 12
    if skipped_above is not None:       # wave kernel with long rows: first rows that belong to the long launch, and long copies
        assert ((fl > skipped_above) & (sl > 0) & (sl <= skipped_above)).sum() >= 12 and (sl > skipped_above).sum() >= 12
    return second


def _row_terms(v, q, Y):
    """what a column adds to the loss, in double, at the answer Y: sum_j w_j (t_j - x_j . y)^2 + lambda_use y . y
    (wrmf_implicit.hpp:256-270, wrmf_explicit.hpp:113-132); no biases here"""
    X, lens = q["X"], q["lens"]
    out = np.zeros(len(lens))
    for c in range(len(out)):
        idx, val = q["i"][q["p"][c]:q["p"][c + 1]], q["x"][q["p"][c]:q["p"][c + 1]]
        y = Y[:, c]
        if len(idx) == 0 and not (v["implicit"] and v["gbias"] != 0.0):
            continue
        if v["implicit"]:
            out[c] = float(val @ ((1.0 - v["gbias"]) - y @ X[:, idx]) ** 2) + v["lam"] * float(y @ y)
        else:
            out[c] = float(np.sum((val - y @ X[:, idx]) ** 2)) + v["lam"] * (len(idx) if v["dyn"] else 1.0) * float(y @ y)
    return out


def _regulariser(v, q, cnt):
    """lambda * accu(X % X) [* cnt_X]: what the stateless entry points add to the rows' loss terms"""
    X2 = q["X"] ** 2
    return v["lam"] * float((X2 * cnt).sum() if v["dyn"] else X2.sum())


TILE_GENERIC = {
    "cholesky_k8": (_variant(True, CHOL), 8),
    "cholesky_k40": (_variant(True, CHOL), 40),
    "cholesky_k100": (_variant(True, CHOL), 100),
    "cholesky_k40_indefinite": (INDEFINITE, 40),               # second rows behind rows that took the fallback
    "nnls_k64": (_variant(True, NNLS, lam=1.0), 64),           # M2 in LDS; lambda 1: test_nnls_rows.py's well-posed recipe
    "nnls_k100": (_variant(True, NNLS, lam=1.0), 100),         # M2 in m2_scratch + blockIdx.x * ...
    "cg_global_bias_k40": (_variant(True, CG, gbias=0.03), 40),
}
TILE_WAVE = {
    "implicit_k16": (WAVE_VARIANTS["implicit"], 16, None),
    "implicit_k32": (WAVE_VARIANTS["implicit"], 32, None),
    "implicit_k64": (WAVE_VARIANTS["implicit"], 64, None),
    "implicit_k128": (WAVE_VARIANTS["implicit"], 128, None),
    "explicit_k64": (WAVE_VARIANTS["explicit_dynamic_lambda"], 64, None),
    "implicit_k32_long_rows": (WAVE_VARIANTS["implicit"], 32, (40, 64)),
}


def _second_pass(tag, v, k, stride, tail, long_rows=None):
    """`tail` columns more than one pass of the row loop takes.  Asserted first, from the lengths alone (_check_tiling): the
    second-pass rows are at least 46 solved rows of at least 11 distinct lengths, at least half of them behind a first row that
    is at least as long.  Then: every copy is BIT-identical to that column's answer in a launch of the 48 columns alone, where
    every row is a first row -- a second row that starts from anything its workgroup or wave kept (the LDS system, rhs, sv, x,
    the fallback's verdict, M2, the look-ahead registers) differs from it even where the difference is far inside any bound;
    the 48 columns meet the per-row bound against the oracle; the loss is the sum of the copies' row terms, evaluated in double
    at the oracle's answer."""
    if v is INDEFINITE:
        q, _, bound = _indefinite_case(k, LENGTHS_TILE, each_twice=False)
        loss_tol = 1e-7
    else:
        q = _case(v, k, LENGTHS_TILE, 5000 + k, each_twice=False)
        _assert_well_conditioned(v, q)
        bound, loss_tol = None, None
    t = _tile(q, stride, tail)
    second = _check_tiling(q, t, stride, tail, skipped_above=long_rows[0] if long_rows else None)
    n_total, nnz, src = stride + tail, float(t["p"][-1]), t["src"]
    # the row terms of the oracle's answer add up to the oracle's loss: the tiled matrix' loss is their sum over the copies
    terms = _row_terms(v, q, q["Yref"])
    l48 = (terms.sum() + _regulariser(v, q, q["cnt"])) / float(q["p"][-1])
    assert abs(l48 - q["lref"]) <= 1e-12 * abs(q["lref"]), (l48, q["lref"])
    lref = (terms[src].sum() + _regulariser(v, q, t["cnt"])) / nnz
    if long_rows:
        _long_rows(*long_rows)
    Y1, loss1 = _device(v, q)                                        # 48 columns: every row is a first row
    Y, loss = _device(v, q, csc=(q["n_item"], n_total, t["p"], t["i"], t["x"]), Y0=t["Y0"], cnt=t["cnt"])
    same = (Y == Y1[:, src]).all(axis=0)
    first_bad = int(np.argmin(same))
    _report(tag, columns=n_total, copies_identical=bool(same.all()), differing=int((~same).sum()),
            differing_in_second_pass=int((~same[second]).sum()),
            second_pass_lengths=",".join(str(n) for n in sorted(set(t["lens"][second].tolist()))))
    assert same.all(), ("column %d, a copy of the row of %d non-zeros" % (first_bad, int(t["lens"][first_bad])),
                        "second pass" if first_bad >= stride else "first pass")
    _assert_rows_and_loss(tag + " 48 columns", v, q, Y1, loss1, bound=bound, loss_tol=loss_tol)
    _assert_rows_and_loss(tag, v, q, Y[:, stride:stride + N_DISTINCT], loss, bound=bound, loss_tol=loss_tol, lref=lref)


@pytest.mark.parametrize("case", list(TILE_GENERIC))
def test_second_row_of_a_workgroup_reads_nothing_left_by_the_first(case):
    """f64_als_kernel: row = blockIdx.x; row += gridDim.x with gridDim = kF64MaxGrid -- 48 workgroups take a second row."""
    v, k = TILE_GENERIC[case]
    _second_pass("E generic %s" % case, v, k, _max_grid(), N_DISTINCT)


@pytest.mark.parametrize("case", list(TILE_WAVE))
def test_second_row_of_a_wave_reads_nothing_left_by_the_first(case):
    """f64_cg_wave_kernel: row = blockIdx.x * 4 + wv; row += gridDim.x * 4 with gridDim = kF64MaxGrid -- 192 waves take a second
    row.  With rsparse_hip_set_f64_long_rows(40, 64) the rows of more than 40 non-zeros belong to the long launch: waves whose
    first row is one of those skip it (`continue`) and start with their second, and the copies of the chunked rows must be
    bit-identical too (their partial sums are added in chunk order)."""
    v, k, long_rows = TILE_WAVE[case]
    _second_pass("E wave %s" % case, v, k, 4 * _max_grid(), 4 * N_DISTINCT, long_rows=long_rows)
