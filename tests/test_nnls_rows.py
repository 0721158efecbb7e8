"""solver = "nnls" on the device, per ROW, at every kernel the dispatch reaches and at the row lengths where each one branches.

Five kernels run the non-negative half-iteration: the one-wave-per-row kernel of wrmf_nnls.hip (padded rank 32 / 64), the
256-thread kernel of the same file (padded rank 128) as `VEC + GLHS` (lhs in a global scratch, 16-vector tile) and as non-`VEC`
(lhs in LDS, 32-vector tile), the NNLS branch of wrmf_wide.hip (rank 129..256) and the NNLS branch of the generic fp64 kernel
(wrmf_f64.hip; the squared system in LDS up to rank 92, in a global scratch beyond).

What the device is compared with, per row, with rowerr(A, B) = ||A - B|| / max(||B||, 1e-30) over the row's coordinates:
    Y64    the fp64 oracle on the same fp32 inputs        Y32    the oracle's own float build
    EX     scipy.optimize.nnls(lhs, rhs) in float64 on lhs / rhs formed as test_oracle_nnls_solves_the_constrained_least_squares
    slack = rowerr(Y64, EX)   what the reference's stopping rule (largest relative step of a sweep <= 1e-4) leaves
    d32   = rowerr(Y32, Y64)  what fp32 arithmetic costs the reference itself
    bound: rowerr(Y, Y64) <= max(1e-4, 3 * d32, slack)    fp64 entry points: max(1e-6, slack) -- 1e-6 is test_f64.py's NNLS bound
    loss:  |loss - l64| <= max(1e-4, 3 * |l32 - l64| / |l64|) * |l64|                            fp64: 1e-6 * |l64|
and exactly: Y >= 0, every value finite, an empty column without a right-hand-side offset all zeros.

The bound means something only on inputs where the reference itself is close to the exact minimiser and the constraint is
active, so every test first asserts, on the CPU and on the reference alone: slack <= 1e-3 on every row, and between 30 % and 70 %
of the coordinates of EX over the non-empty rows exactly zero.  Inputs: implicit feedback, factors N(0, 0.1^2), lambda 1; explicit
feedback, factors N(0, 0.3^2) up to rank 32 and N(0, 1.7^2 / k) beyond (EXPLICIT_NORM), lambda 0.5 times the row length, or plain
lambda 1 (cond(lhs) below 50: slack at or below 5.4e-4; with lambda 0.1 the shortest rows sit at 1e-2 .. 1e-1 and no per-row bound
means anything).  Warm start |N(0, scale^2)|, all zeros for every third column (transform()'s start).  The columns lie in a
SHUFFLED order of distinct lengths: the kernels walk the rows longest first (nnls_order), and a wrong mapping lands a visibly
wrong answer in a named row.

Which instantiation a rank reaches (run_half_iteration, launch_als_nnls, wide_supported, f64_geometry): a rank below 128 that is
no multiple of 4 runs on copies padded with zero coordinates to the next multiple of 4, on an aligned buffer.  So ranks 1 / 5 /
17 / 31 / 33 / 47 / 63 reach the wave kernel as 4 / 8 / 20 / 32 / 36 / 48 / 64, ranks 65 / 101 / 127 the `VEC + GLHS` kernel
as 68 / 104 / 128, and the non-`VEC` instantiations -- the scalar loss pass of the wave kernel, lhs in LDS with the 32-vector
tile -- run only where the caller's X is not 16-byte aligned: the `unaligned` tests below (device-resident layer, a view offset
by one float).

Every test prints its figures before it asserts (pytest -s, lines starting with `nnls_rows`): profiles/nnls_tests/README.md."""
import numpy as np
import pytest
import scipy.optimize

from oracle import wrmf_oracle as O

gpu = pytest.mark.gpu
NNLS = 2
TOL = 1e-4          # the project's per-row floor (test_exact_solver_classes.TOL) and the reference's SCD_TOL
TOL_F64 = 1e-6      # tests/test_f64.py, _bound(solver = 2)
SLACK_MAX = 1e-3
ZERO_SHARE = (0.30, 0.70)
N_ITEM = 600

VARIANTS = {
    "implicit": dict(implicit=True, lam=1.0, scale=0.1, dyn=False),
    "explicit_dynamic_lambda": dict(implicit=False, lam=0.5, scale=0.3, dyn=True),
    "explicit_plain_lambda": dict(implicit=False, lam=1.0, scale=0.3, dyn=False),
}
# explicit feedback above rank 32: the factor scale falls as 1.7 / sqrt(k), so that a factor vector keeps the norm it has at rank
# 32 (1.7) and the shortest rows -- lhs = x x^T + lambda I, cond = 1 + |x|^2 / lambda -- stay as well conditioned at rank 256 as
# there.  With 0.3 at every rank the reference's own slack passes 1e-3 from rank 100 on (1.8e-2 at rank 255).
EXPLICIT_NORM = 1.7


# ---------------------------------------------------------------------------------------------------------------------------
# helpers (the shape of test_exact_solver_classes._rows_of_lengths / _row_err / _report)
# ---------------------------------------------------------------------------------------------------------------------------

def _shuffled(lengths, seed):
    lens = np.asarray(lengths, dtype=np.int64)
    return lens[np.random.default_rng(seed).permutation(lens.size)]


def _fill_to(lengths, n):
    """`lengths` plus the smallest lengths not in it, up to n distinct ones"""
    out, have, c = list(lengths), set(lengths), 0
    while len(out) < n:
        if c not in have:
            out.append(c)
        c += 1
    return out


def _rows_of_lengths(lengths, n_item, k, seed, scale):
    """a CSC (columns = the rows to solve) whose column j has lengths[j] distinct random items, values >= 1; factors
    N(0, scale^2), warm start |N(0, scale^2)| with every third column all zeros"""
    rng = np.random.default_rng(seed)
    p = np.zeros(len(lengths) + 1, dtype=np.int32)
    p[1:] = np.cumsum(lengths)
    idx = np.concatenate([np.sort(rng.choice(n_item, size=int(n), replace=False)) for n in lengths] +
                         [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    x = (1.0 + rng.gamma(1.0, 2.0, size=idx.size)).astype(np.float32).astype(np.float64)
    X = np.asfortranarray((rng.standard_normal((k, n_item)) * scale).astype(np.float32))
    Y0 = np.asfortranarray(np.abs(rng.standard_normal((k, len(lengths))) * scale).astype(np.float32))
    Y0[:, ::3] = 0.0
    return (n_item, len(lengths), p, idx, x), X, Y0


def _row_err(Y, Yref):
    return np.linalg.norm(Y - Yref, axis=0) / np.maximum(np.linalg.norm(Yref, axis=0), 1e-30)


def _f64(a):
    return np.asfortranarray(a, dtype=np.float64).copy(order="F")


def _report(tag, **figures):
    print("nnls_rows %s %s" % (tag, " ".join("%s=%s" % (n, ("%.3g" % v) if isinstance(v, float) else v)
                                              for n, v in figures.items())))


def _exact(p, i, x, systems):
    """scipy's active-set NNLS per column: systems(c, idx, val) -> (lhs, rhs) in float64, or None for a column that stays zero"""
    cols = []
    for c in range(len(p) - 1):
        s = systems(c, i[p[c]:p[c + 1]], x[p[c]:p[c + 1]])
        cols.append(None if s is None else scipy.optimize.nnls(s[0], s[1])[0])
    k = next(len(c) for c in cols if c is not None)
    return np.asfortranarray(np.stack([np.zeros(k) if c is None else c for c in cols], axis=1))


def _plain_systems(X64, v, G):
    k = X64.shape[0]

    def systems(c, idx, val):
        if len(idx) == 0:
            return None
        Xn = X64[:, idx]
        if v["implicit"]:
            return G + (Xn * (val - 1.0)) @ Xn.T, Xn @ val
        return Xn @ Xn.T + v["lam"] * (len(idx) if v["dyn"] else 1.0) * np.eye(k), Xn @ val
    return systems


def _freeze(q):
    for a in q.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return q


_cache = {}


def _case(k, variant, lengths, seed):
    """the lattice `lengths` (shuffled) at rank k with the oracle's answers in double and in float and scipy's exact ones --
    computed once per (rank, variant, lattice) and shared"""
    key = (k, variant, tuple(lengths), seed)
    if key not in _cache:
        v = dict(VARIANTS[variant])
        if not v["implicit"]:
            v["scale"] = min(v["scale"], EXPLICIT_NORM / np.sqrt(k))
        lens = _shuffled(lengths, seed)
        (n_item, n_cols, p, i, x), X, Y0 = _rows_of_lengths(lens, N_ITEM, k, seed=seed + 1, scale=v["scale"])
        cnt = np.bincount(i, minlength=n_item).astype(np.float64)
        X64, Y64, Y32 = _f64(X), _f64(Y0), Y0.copy(order="F")
        G = O.gramian(X64, v["lam"]) if v["implicit"] else None
        if v["implicit"]:
            l64 = O.als_implicit(p, i, x, X64, Y64, G, v["lam"], NNLS, 3)
            l32 = O.als_implicit(p, i, x, X, Y32, O.gramian(X, v["lam"]), v["lam"], NNLS, 3)
        else:
            l64 = O.als_explicit(p, i, x, X64, Y64, cnt, v["lam"], NNLS, 3, v["dyn"])
            l32 = O.als_explicit(p, i, x, X, Y32, cnt.astype(np.float32), v["lam"], NNLS, 3, v["dyn"])
        EX = _exact(p, i, x, _plain_systems(X64, v, G))
        _cache[key] = _freeze(dict(v, k=k, variant=variant, lens=lens, n_item=n_item, p=p, i=i, x=x, X=X, Y0=Y0, cnt=cnt, G=G,
                                   Y64=Y64, Y32=Y32, EX=EX, l64=l64, l32=l32, slack=_row_err(Y64, EX), d32=_row_err(Y32, Y64),
                                   solved=lens > 0))
    return _cache[key]


def _check_preconditions(q, zero_share=True):
    """on the reference alone, before the device is looked at"""
    solved = q["solved"]
    worst = int(np.argmax(np.where(solved, q["slack"], 0.0)))
    assert np.all(q["slack"][solved] <= SLACK_MAX), ("the reference is far from the exact minimiser: row of %d non-zeros"
                                                     % int(q["lens"][worst]), float(q["slack"][worst]))
    share = float(np.mean(q["EX"][:, solved] == 0.0))
    if zero_share:
        assert ZERO_SHARE[0] <= share <= ZERO_SHARE[1], share
    assert np.all(q["Y64"][:, ~solved] == 0.0) and np.all(q["EX"] >= 0.0)
    return share


def _assert_rows_and_loss(tag, q, Y, loss, share, fp64=False, l64=None, l32=None):
    lens, Y64 = q["lens"], q["Y64"]
    err = _row_err(Y, Y64)
    bound = np.maximum(TOL_F64, q["slack"]) if fp64 else np.maximum(np.maximum(TOL, 3.0 * q["d32"]), q["slack"])
    worst = int(np.argmax(err / bound))
    l64 = q["l64"] if l64 is None else l64
    l32 = q["l32"] if l32 is None else l32
    lerr = abs(loss - l64) / abs(l64)
    lbound = TOL_F64 if fp64 else max(TOL, 3.0 * abs(l32 - l64) / abs(l64))
    _report(tag, worst_ratio=float(err[worst] / bound[worst]), worst_len=int(lens[worst]), err=float(err[worst]),
            bound=float(bound[worst]), slack_max=float(q["slack"].max()), d32_max=float(q["d32"].max()), zero_share=float(share),
            loss_err=float(lerr), loss_bound=float(lbound))
    assert np.all(np.isfinite(Y)) and np.isfinite(loss)
    assert Y.min() >= 0.0
    assert np.all(Y[:, ~q["solved"]] == 0.0)                       # the empty column (wrmf_implicit.hpp:281, wrmf_explicit.hpp:142)
    assert np.all(err <= bound), ("row of %d non-zeros" % int(lens[worst]), worst, float(err[worst]), float(bound[worst]))
    assert lerr <= lbound, (loss, l64, l32)


def _run_stateless(q, precision="float", Y0=None, csc=None):
    from rsparse_amd import als
    dt = np.float32 if precision == "float" else np.float64
    X = np.asfortranarray(q["X"], dtype=dt)
    Y = np.asfortranarray(q["Y0"] if Y0 is None else Y0, dtype=dt).copy(order="F")
    csc = (q["n_item"], len(q["lens"]), q["p"], q["i"], q["x"]) if csc is None else csc
    if q["implicit"]:
        G = None if precision == "float" else q["G"]          # (double: the oracle's Gramian, as tests/test_f64.py passes it)
        loss = als.als_implicit(csc, X, Y, q["lam"], 1, NNLS, 3, precision, False, False, XtX=G)
    else:
        loss = als.als_explicit(csc, X, Y, q["cnt"].astype(dt), q["lam"], 1, NNLS, 3, q["dyn"], precision, False, False)
    return Y, loss


def _regulariser(q):
    """lambda * accu(X % X) [* cnt_X]: what the stateless entry points add to the rows' loss terms"""
    X2 = q["X"].astype(np.float64) ** 2
    return q["lam"] * float((X2 * q["cnt"]).sum() if q["dyn"] else X2.sum())


def _run_resident_unaligned(q):
    """the device-resident layer on an X that starts 4 bytes past a 16-byte boundary (a view into a larger buffer): the kernels'
    `vec` test fails at a rank that is a multiple of 4 and the element-wise instantiations run"""
    import torch
    from rsparse_amd import als
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    k, n_item, n_cols = q["k"], q["n_item"], len(q["lens"])
    assert k % 4 == 0
    h = be.make_csc(n_item, n_cols, be.to_device(np.array(q["p"]), torch.int32), be.to_device(np.array(q["i"]), torch.int32),
                    be.to_device(q["x"].astype(np.float32), torch.float32))
    buf = torch.zeros(n_item * k + 1, dtype=torch.float32, device=be.device)
    Xd = buf[1:].view(n_item, k)
    Xd.copy_(be.to_device(np.array(q["X"].T, order="C"), torch.float32))
    assert Xd.data_ptr() % 16 == 4
    Yd = be.to_device(np.array(q["Y0"].T, order="C"), torch.float32)
    Gd = None
    if q["implicit"]:
        Gd = be.to_device(np.array(als.gramian(np.array(q["X"], order="F"), q["lam"], "float"), order="C"), torch.float32)
    lossd = torch.zeros(1, dtype=torch.float64, device=be.device)
    be.half_iteration(h, q["implicit"], Xd, Yd, Gd, q["lam"], NNLS, 3, q["dyn"], lossd)
    Y = np.asfortranarray(Yd.cpu().numpy().T)
    return Y, (float(lossd.cpu()[0]) + _regulariser(q)) / float(q["p"][-1])


# ---------------------------------------------------------------------------------------------------------------------------
# CPU-only checks of the helpers
# ---------------------------------------------------------------------------------------------------------------------------

def test_lattice_is_shuffled_distinct_and_a_third_starts_from_zero():
    q = _case(5, "implicit", LENGTHS_WAVE, 1105)
    lens = q["lens"]
    assert sorted(lens.tolist()) == sorted(LENGTHS_WAVE) and len(set(lens.tolist())) == len(lens)
    assert not np.array_equal(lens, np.sort(lens)) and not np.array_equal(lens, np.sort(lens)[::-1])
    assert np.array_equal(np.diff(q["p"]), lens)
    for c in range(len(lens)):
        idx = q["i"][q["p"][c]:q["p"][c + 1]]
        assert np.all(np.diff(idx) > 0) and (len(idx) == 0 or (idx[0] >= 0 and idx[-1] < N_ITEM))
    zero_start = ~q["Y0"].any(axis=0)
    assert np.array_equal(np.flatnonzero(zero_start), np.arange(0, len(lens), 3)) and q["Y0"].min() >= 0.0
    assert sorted(_fill_to([0, 2, 5], 5)) == [0, 1, 2, 3, 5]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_exact_answers_satisfy_the_kkt_conditions(variant):
    """EX minimises ||lhs h - rhs|| over h >= 0: with g = lhs^T (lhs h - rhs), h >= 0, g >= 0 where h = 0 and g = 0 where h > 0"""
    q = _case(17, variant, LENGTHS_WAVE, 1117)
    X64 = _f64(q["X"])
    systems = _plain_systems(X64, q, q["G"])
    for c in range(len(q["lens"])):
        s = systems(c, q["i"][q["p"][c]:q["p"][c + 1]], q["x"][q["p"][c]:q["p"][c + 1]])
        h = q["EX"][:, c]
        if s is None:
            assert not h.any()
            continue
        g = s[0].T @ (s[0] @ h - s[1])
        scale = np.linalg.norm(s[0].T @ s[1])
        assert h.min() >= 0.0 and np.all(g[h == 0.0] >= -1e-10 * scale) and np.all(np.abs(g[h > 0.0]) <= 1e-10 * scale)
    _check_preconditions(q)


def test_tiling_repeats_columns_and_puts_solved_rows_of_several_lengths_into_the_second_pass():
    q = _case(8, "implicit", LENGTHS_TILE_WAVE, 1508)
    n0 = len(q["lens"])
    assert n0 == 48 and len(set(q["lens"].tolist())) == 48
    for n_total, grid, by_length in ((24576 + 48, 24576, True), (1024 + 48, 1024, False)):
        t = _tile(q, n_total)
        assert np.array_equal(t["src"][:n0], np.arange(n0)) and set(t["src"].tolist()) == set(range(n0))
        for c in (0, 47, 48, n_total // 2, n_total - 48, n_total - 1):
            a, b = t["p"][c], t["p"][c + 1]
            a0, b0 = q["p"][t["src"][c]], q["p"][t["src"][c] + 1]
            assert np.array_equal(t["i"][a:b], q["i"][a0:b0]) and np.array_equal(t["x"][a:b], q["x"][a0:b0])
            assert np.array_equal(t["Y0"][:, c], q["Y0"][:, t["src"][c]])
        tl = _check_second_pass(t, grid, by_length)
        assert (tl == 0).sum() == (2 if by_length else 1)   # natural order: the 48 distinct columns themselves
    # the row terms of the reference's answer add up to the reference's loss; the tiled matrix' loss is their sum over the copies
    t64 = _implicit_row_terms(q, q["Y64"])
    assert abs((t64.sum() + _regulariser(q)) / float(q["p"][-1]) - q["l64"]) <= 1e-12 * abs(q["l64"])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the one-wave-per-row kernel (als_nnls_wave_kernel), padded rank 32 / 64
# ---------------------------------------------------------------------------------------------------------------------------

# chunks of 64 non-zeros with a 4-deep look-ahead clamped at ccnt - 1: 0..9 = all four phases of the look-ahead and the clamp,
# 62..68 / 126..130 around one and two chunks, 200 = three full chunks and a tail of 8
LENGTHS_WAVE = list(range(0, 10)) + list(range(62, 69)) + list(range(126, 131)) + [200]


@gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("k", [1, 5, 17, 31, 32, 33, 47, 63, 64])
def test_wave_kernel_every_rank_class_and_row_length(k, variant):
    """Ranks 1 / 5 / 17 / 31 run padded to 4 / 8 / 20 / 32 and rank 32 as it is on <32>: in_range = (1 << k) - 1 up to 1 << 32;
    33 / 47 / 63 padded to 36 / 48 / 64 and rank 64 as it is on <64>: k < KP with lanes k..63 on the identity, and in_range = ~0
    at 64.  The padded coordinates must come back as exact zeros of the padded system and never reach Y."""
    q = _case(k, variant, LENGTHS_WAVE, 1100 + k)
    share = _check_preconditions(q)
    Y, loss = _run_stateless(q)
    _assert_rows_and_loss("wave k=%d %s" % (k, variant), q, Y, loss, share)


@gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("k", [32, 36, 64])
def test_wave_kernel_unaligned_x_takes_the_scalar_loss_pass(k, variant):
    """`vec` is false only for an X off the 16-byte grid: the loss pass then walks X element by element.  Rank 36 is k < KP on
    <64> with a TRUE rank below the padded one (in_range = (1 << 36) - 1, the `lk` lanes)."""
    q = _case(k, variant, LENGTHS_WAVE, 1100 + k)
    share = _check_preconditions(q)
    Y, loss = _run_resident_unaligned(q)
    _assert_rows_and_loss("wave-unaligned k=%d %s" % (k, variant), q, Y, loss, share)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the 256-thread kernel, both instantiations (als_nnls_kernel<128, ...>)
# ---------------------------------------------------------------------------------------------------------------------------

# the edges of both tile sizes (16 with lhs in the global scratch, 32 with lhs in LDS)
LENGTHS_WG = [0, 1, 2] + list(range(14, 19)) + list(range(30, 35)) + list(range(46, 51)) + list(range(62, 67)) + [96, 200]


@gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("k", [68, 100, 128, 65, 101, 127])
def test_workgroup_kernel_every_rank_class_and_row_length(k, variant):
    """All six reach `VEC + GLHS` (the stateless entry points upload X to an aligned buffer; 65 / 101 / 127 run padded to 68 /
    104 / 128): identity padding up to 128, the sweep limit min(KP, k), in_range of the second lane group (k - 64 = 4, 36, 40
    bits, ~0 at 128)."""
    q = _case(k, variant, LENGTHS_WG, 1200 + k)
    share = _check_preconditions(q)
    Y, loss = _run_stateless(q)
    _assert_rows_and_loss("workgroup k=%d %s" % (k, variant), q, Y, loss, share)


@gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("k", [128, 100, 68])
def test_workgroup_kernel_unaligned_x_keeps_lhs_in_lds(k, variant):
    """An X that is not 16-byte aligned: the non-`VEC` instantiation -- lhs in LDS (148 KB), 32-vector tile, element-wise gather
    -- at full rank and at two true ranks below the padded one."""
    q = _case(k, variant, LENGTHS_WG, 1200 + k)
    share = _check_preconditions(q)
    Y, loss = _run_resident_unaligned(q)
    _assert_rows_and_loss("workgroup-unaligned k=%d %s" % (k, variant), q, Y, loss, share)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the wide kernel's NNLS branch (wrmf_wide.hip), rank 129..256
# ---------------------------------------------------------------------------------------------------------------------------

LENGTHS_WIDE = [0, 1, 3] + list(range(63, 66)) + list(range(127, 130)) + [300]


@gpu
@pytest.mark.parametrize("variant", ["implicit", "explicit_dynamic_lambda"])
@pytest.mark.parametrize("k", [129, 130, 192, 193, 255, 256])
def test_wide_kernel_nnls_every_rank_class_and_row_length(k, variant):
    """k mod 4 = 1 and 2 against the 4 x 4 tiles of the squaring loop (129, 130; 193; 255 = 3), full tiles at 192 and 256; four
    lane groups of the sweep with 1, 2, 64 / 0, 1, 63 and 64 coordinates in the last one that is in use."""
    q = _case(k, variant, LENGTHS_WIDE, 1300 + k)
    share = _check_preconditions(q)
    Y, loss = _run_stateless(q)
    _assert_rows_and_loss("wide k=%d %s" % (k, variant), q, Y, loss, share)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. fp64 NNLS (the *_double entry points, wrmf_f64.hip)
# ---------------------------------------------------------------------------------------------------------------------------

# f64_geometry(k, solver = 2) stages CH = 32 vectors at ranks 4 and 32, 64 at 33, 65, 93 and 100, 16 at 64, 92 and 128; the squared
# system lives in LDS up to rank 92 (two matrices within 156 KB) and in m2_scratch from 93 on.  CH - 1, CH, CH + 1 and 2 CH + 1 for
# all three chunk sizes, so that the lattice does not depend on that table being read right:
LENGTHS_F64 = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129]


@gpu
@pytest.mark.parametrize("variant", ["implicit", "explicit_dynamic_lambda"])
@pytest.mark.parametrize("k", [4, 32, 33, 64, 65, 92, 93, 100, 128])
def test_double_entry_points_every_geometry_and_row_length(k, variant):
    """64 / 256 / 512 threads (rank <= 32, <= 64, beyond); 92 and 93 are the two sides of the LDS / m2_scratch threshold.  No d32
    term: max(1e-6, slack) per row, 1e-6 on the loss."""
    q = _case(k, variant, LENGTHS_F64, 1400 + k)
    share = _check_preconditions(q)
    Y, loss = _run_stateless(q, "double")
    _assert_rows_and_loss("f64 k=%d %s" % (k, variant), q, Y, loss, share, fp64=True)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the second pass of the grid-stride row loop
# ---------------------------------------------------------------------------------------------------------------------------

LENGTHS_TILE_WAVE = _fill_to(LENGTHS_WAVE, 48)
LENGTHS_TILE_WG = _fill_to(LENGTHS_WG, 48)
LENGTHS_TILE_WIDE = _fill_to(LENGTHS_WIDE, 48)


N_SHORT, N_TAIL = 12, 48


def _tile(q, n_total):
    """the 48 distinct columns of q repeated up to n_total columns, every copy with the same items, values and warm start.  The
    kernels of wrmf_nnls.hip walk the rows longest first (plan_schedule: a stable counting sort by length, descending, empty rows
    last), so the rows of a workgroup's SECOND pass are the shortest of the matrix; wrmf_wide.hip walks them in natural order, so
    they are the last columns.  Layout: the 48 distinct columns, a shuffled middle, the 48 distinct columns again in reverse;
    the N_SHORT shortest non-empty columns get two more copies in the middle and the empty one none, every other column fills
    the rest.  The last N_TAIL rows of the length-sorted order are then 2 empty and 46 solved rows of N_SHORT distinct lengths, the
    last N_TAIL columns one empty and 47 solved rows of 47 lengths."""
    lens0 = q["lens"]
    n0 = len(lens0)
    by_len = np.argsort(lens0, kind="stable")
    assert lens0[by_len[0]] == 0 and lens0[by_len[1]] > 0
    short, rest = by_len[1:1 + N_SHORT], by_len[1 + N_SHORT:]
    n_mid = n_total - 2 * n0 - 2 * N_SHORT
    mid = np.concatenate([short, short, rest[np.arange(n_mid) % len(rest)]])
    mid = mid[np.random.default_rng(n_total).permutation(mid.size)]
    src = np.concatenate([np.arange(n0), mid, np.arange(n0)[::-1]])
    assert src.size == n_total
    lens = lens0[src]
    p = np.zeros(n_total + 1, dtype=np.int32)
    p[1:] = np.cumsum(lens)
    pos = np.concatenate([np.arange(q["p"][c], q["p"][c + 1]) for c in src])
    return dict(src=src, lens=lens, p=p, i=np.ascontiguousarray(q["i"][pos]), x=np.ascontiguousarray(q["x"][pos]),
                Y0=np.asfortranarray(q["Y0"][:, src]))


def _second_pass_rows(lens, grid, by_length):
    """the rows that the workgroups of a `grid`-wide launch take in their second pass, from the lengths alone"""
    order = np.argsort(-lens, kind="stable") if by_length else np.arange(lens.size)
    return order[grid:]


def _check_second_pass(t, grid, by_length):
    tail = _second_pass_rows(t["lens"], grid, by_length)
    tl = t["lens"][tail]
    assert tail.size == N_TAIL and (tl > 0).sum() >= N_TAIL - 2 and len(set(tl[tl > 0].tolist())) >= N_SHORT - 1, tl
    first = (np.argsort(-t["lens"], kind="stable") if by_length else np.arange(t["lens"].size))[:N_TAIL]
    # longest first: the first pass leaves MORE state than the second one overwrites
    assert np.all(t["lens"][first] > tl.max()) or not by_length
    return tl


def _implicit_row_terms(q, Y):
    """sum_j c_j (1 - x_j . y)^2 + lambda y . y per column, in double (wrmf_implicit.hpp:256-270)"""
    X64, Yd = q["X"].astype(np.float64), np.asarray(Y, dtype=np.float64)
    out = np.zeros(len(q["lens"]))
    for c in range(len(out)):
        idx, val = q["i"][q["p"][c]:q["p"][c + 1]], q["x"][q["p"][c]:q["p"][c + 1]]
        if len(idx):
            out[c] = float(val @ (1.0 - Yd[:, c] @ X64[:, idx]) ** 2) + q["lam"] * float(Yd[:, c] @ Yd[:, c])
    return out


@gpu
@pytest.mark.parametrize("k,lengths,grid,by_length", [(8, LENGTHS_TILE_WAVE, 24576, True), (100, LENGTHS_TILE_WG, 24576, True),
                                                      (130, LENGTHS_TILE_WIDE, 1024, False)])
def test_second_pass_of_the_row_loop_reads_nothing_left_by_the_first(k, lengths, grid, by_length):
    """48 columns more than the grid has workgroups (24576 in wrmf_nnls.hip, 1024 in wrmf_wide.hip): 48 workgroups take a second
    row with the tile, the accumulator registers, the scratch slice, sH and the loss slot their first row left.  Asserted first,
    from the lengths alone (_check_second_pass): those 48 second rows are at least 46 solved rows of at least 11 distinct lengths
    and at most 2 empty ones, in wrmf_nnls.hip behind first rows that are longer.  48 distinct columns in many copies: every copy
    must be BIT-identical to that column's answer in a launch of the 48 columns alone, where every row is some workgroup's first
    (and so to every other copy) -- a second row that starts from anything its workgroup kept differs from it, even where the
    difference is far inside any bound (a warm start left in sH) or the same for all copies of a length (the second-pass
    workgroups all had a copy of the longest column first) --, the 48 distinct columns meet the per-row bound against a
    48-column reference, and the loss is the sum of the copies' terms (row terms evaluated in double at the oracle's double and
    float answers) within the loss rule.  Implicit feedback: the regulariser of X does not depend on the number of copies."""
    q = _case(k, "implicit", lengths, 1500 + k)
    share = _check_preconditions(q)
    n0 = len(q["lens"])
    t = _tile(q, grid + N_TAIL)
    tl = _check_second_pass(t, grid, by_length)
    n_total, nnz, src = grid + N_TAIL, float(t["p"][-1]), t["src"]
    Y1, _ = _run_stateless(q)                                       # 48 columns on 48 workgroups: every row in a first pass
    Y, loss = _run_stateless(q, Y0=t["Y0"], csc=(q["n_item"], n_total, t["p"], t["i"], t["x"]))
    same = np.array([np.array_equal(Y[:, c], Y1[:, src[c]]) for c in range(n_total)])
    l64 = (_implicit_row_terms(q, q["Y64"])[src].sum() + _regulariser(q)) / nnz
    l32 = (_implicit_row_terms(q, q["Y32"])[src].sum() + _regulariser(q)) / nnz
    first_bad = int(np.argmin(same))
    second = _second_pass_rows(t["lens"], grid, by_length)
    _report("tiled k=%d n=%d" % (k, n_total), copies_identical=bool(same.all()), differing=int((~same).sum()),
            differing_in_second_pass=int((~same[second]).sum()),
            second_pass_lengths=",".join(str(v) for v in sorted(set(tl.tolist()))))
    assert same.all(), ("column %d, a copy of the row of %d non-zeros" % (first_bad, int(t["lens"][first_bad])),
                        "second pass" if first_bad in set(second.tolist()) else "first pass")
    _assert_rows_and_loss("tiled k=%d" % k, q, Y[:, :n0], loss, share, l64=l64, l32=l32)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. an empty column with a right-hand-side offset is solved, not zeroed
# ---------------------------------------------------------------------------------------------------------------------------

def _bias_case(k, lengths, seed, with_biases, gbias):
    """implicit feedback with a global bias and / or user-item biases (X = [1, ..., x_bias], Y = [y_bias, ..., 1]): rhs_init =
    -X' (x_bias + g) enters every row, the empty one too (wrmf_implicit.hpp:108-112,146-157,178,228-229)"""
    key = ("bias", k, tuple(lengths), seed, with_biases, gbias)
    if key not in _cache:
        v = VARIANTS["implicit"]
        lens = _shuffled(lengths, seed)
        (n_item, n_cols, p, i, x), X, Y0 = _rows_of_lengths(lens, N_ITEM, k, seed=seed + 1, scale=v["scale"])
        if with_biases:
            X[0, :] = 1.0
            Y0[k - 1, :] = 1.0
        keep = slice(0, k - 1) if with_biases else slice(0, k)
        X64 = _f64(X)
        Xp, xb = X64[keep], (X64[k - 1] if with_biases else np.zeros(n_item))
        G = O.gramian(np.asfortranarray(Xp), v["lam"])
        G32 = O.gramian(np.asfortranarray(X[keep]), v["lam"])
        Y64, Y32 = _f64(Y0), Y0.copy(order="F")
        opts = dict(with_biases=with_biases, is_x_bias_last_row=True, global_bias=gbias)
        l64 = O.als_implicit(p, i, x, X64, Y64, G, v["lam"], NNLS, 3, **opts)
        l32 = O.als_implicit(p, i, x, X, Y32, G32, v["lam"], NNLS, 3, **opts)
        rhs_init = -Xp @ (xb + gbias)

        def systems(c, idx, val):
            Xn, b = Xp[:, idx], xb[idx]
            return G + (Xn * (val - 1.0)) @ Xn.T, rhs_init + Xn @ (val - b * (val - 1.0))
        EX = _exact(p, i, x, systems)
        _cache[key] = _freeze(dict(v, k=k, lens=lens, n_item=n_item, p=p, i=i, x=x, X=X, Y0=Y0, keep=keep, Y64=Y64[keep],
                                   Y32=Y32[keep],
                                   EX=EX, l64=l64, l32=l32, slack=_row_err(Y64[keep], EX), d32=_row_err(Y32[keep], Y64[keep]),
                                   solved=np.ones(len(lens), dtype=bool)))
    return _cache[key]


@gpu
@pytest.mark.parametrize("k,with_biases,gbias", [(33, False, 0.05), (100, False, 0.05), (34, True, 0.0), (101, True, 0.05)])
def test_empty_column_with_a_rhs_offset_is_solved(k, with_biases, gbias):
    """`cnt <= 0 && !a.rhs_init`: with a global bias or user/item biases the empty column has the system XtX h = rhs_init, h >= 0,
    and the oracle's answer for it is not zero.  The solve lands at rank 33 (the wave kernel, padded to 36) and at rank 100 (the
    workgroup kernel) -- with biases the rank counts the row of ones and the bias row, 34 and 101."""
    from rsparse_amd import als
    lengths = LENGTHS_WAVE if k < 64 else LENGTHS_WG
    q = _bias_case(k, lengths, 1600 + k, with_biases, gbias)
    share = _check_preconditions(q)
    empty = int(np.flatnonzero(q["lens"] == 0)[0])
    assert np.linalg.norm(q["Y64"][:, empty]) > 1e-3 and q["EX"][:, empty].any()
    Y = q["Y0"].copy(order="F")
    csc = (q["n_item"], len(q["lens"]), q["p"], q["i"], q["x"])
    loss = als.als_implicit(csc, np.array(q["X"], order="F"), Y, q["lam"], 1, NNLS, 3,
                            "float", with_biases, True, global_bias=gbias)
    if with_biases:
        assert np.array_equal(Y[k - 1], q["Y0"][k - 1])            # the placeholder entry is never written
    # (every column counts as solved here: the empty one is held to the per-row bound below, not to the all-zeros check)
    err_empty = float(_row_err(Y[q["keep"]], q["Y64"])[empty])
    _report("rhs_init k=%d biases=%d g=%g" % (k, with_biases, gbias), empty_col_err=err_empty,
            empty_col_norm=float(np.linalg.norm(q["Y64"][:, empty])))
    _assert_rows_and_loss("rhs_init k=%d biases=%d g=%g" % (k, with_biases, gbias), q, Y[q["keep"]], loss, share)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. a row that never leaves the bound
# ---------------------------------------------------------------------------------------------------------------------------

LENGTHS_BOUND = [0, 1, 5, 33, 64, 65, 130]


@gpu
@pytest.mark.parametrize("k", [33, 100, 130])
def test_rows_whose_minimiser_is_zero_come_back_as_exact_zeros(k):
    """Explicit feedback, every factor |N| and every rating negative: rhs < 0 and lhs >= 0 entry by entry, so the gradient
    XtX h - lhs^T rhs is positive for every h >= 0 and every coordinate of the minimiser is 0.  From a zero start `act` is empty
    and the sweep ends at once; from a positive start every coordinate steps onto the bound in the first sweep.  Either way the
    answer is EXACT zeros -- a sign slip or a lane left out of in_range shows as a surviving value.  (The 30..70 % precondition
    on the share of zeros does not apply: the share is 100 % by construction; the oracle and scipy must both say so.)"""
    from rsparse_amd import als
    lens = _shuffled(LENGTHS_BOUND, 1700 + k)
    (n_item, n_cols, p, i, x), X, Y0 = _rows_of_lengths(lens, N_ITEM, k, seed=1701 + k, scale=0.3)
    X = np.abs(X)
    x = -x
    lam = 0.5
    cnt = np.bincount(i, minlength=n_item).astype(np.float64)
    X64, Y64 = _f64(X), _f64(Y0)
    l64 = O.als_explicit(p, i, x, X64, Y64, cnt, lam, NNLS, 3, True)
    Y32 = Y0.copy(order="F")
    l32 = O.als_explicit(p, i, x, X, Y32, cnt.astype(np.float32), lam, NNLS, 3, True)
    EX = _exact(p, i, x, _plain_systems(X64, dict(implicit=False, lam=lam, dyn=True), None))
    assert not EX.any() and not Y64.any() and not Y32.any()
    assert Y0[:, 1::3].all() and not Y0[:, ::3].any()                  # positive and zero starts, both on rows of every class
    Y = Y0.copy(order="F")
    loss = als.als_explicit((n_item, n_cols, p, i, x), X, Y, cnt.astype(np.float32), lam, 1, NNLS, 3, True, "float", False, False)
    lerr, lbound = abs(loss - l64) / abs(l64), max(TOL, 3.0 * abs(l32 - l64) / abs(l64))
    left = np.flatnonzero(Y.any(axis=0))
    _report("at-the-bound k=%d" % k, nonzero_columns=len(left), largest=float(np.abs(Y).max()), loss_err=float(lerr),
            loss_bound=float(lbound))
    assert np.all(np.isfinite(Y))
    assert not Y.any(), ("row of %d non-zeros" % int(lens[left[0]]), "zero start" if left[0] % 3 == 0 else "positive start")
    assert lerr <= lbound, (loss, l64, l32)
