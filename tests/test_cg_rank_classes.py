"""The fp32 conjugate-gradient kernels per ROW below rank 97 and at the ranks that are no multiple of 4, at every row-length class
of the launch table (wrmf_cgq.hip kBuckets / launch_all / team_grid), through als.als_implicit / als.als_explicit with precision
"float" against the fp64 oracle on the same fp32 inputs widened.

Which kernels a rank reaches (run_half_iteration, launch_als_cgq):
    rank 4..32, rank % 4 == 0      als_cgq_kernel<32>: two floats of a vector per lane; rows beyond 512 non-zeros on the streamed
                                   8-wave instantiation (STREAM = 1), which keeps the per-non-zero products of up to
                                   kMaxSavedSweeps = 4 CG steps in a scratch and takes another path for more steps or none
    rank 36..64                    als_cgq_kernel<64> on launch table 1 (32 resident quads per wave, half the waves per class);
                                   rows beyond 512 non-zeros on the normal-equation kernel (wrmf_ne.hip)
    rank 68..128                   als_cgq_kernel<128> on launch table 0, bucket 1 in three launches (tests/test_cg_team_wide.py);
                                   rows beyond 512 on wrmf_ne.hip, at rank 128 with implicit feedback on wrmf_cg_mf.hip
    rank % 4 != 0 (10, 50, 101)    run_half_iteration solves them on copies padded with zero coordinates to the next multiple
                                   of 4 (12, 52, 104) and copies the solved rows back: the same kernels at k < KP behind
                                   launch_pad_rows / launch_pad_gramian.  The LDS-tile kernels (als_cg_short_kernel /
                                   als_cg_long_kernel) are NOT reached by these entry points at any rank: only an X or Y off the
                                   16-byte grid (the device-pointer ABI) sends a call there.  test_several_rows_per_team asserts
                                   from the profile segments that rank 12 runs on als_cgq_kernel<32>.

Cases:
    A  edges          every length of EDGE_LENGTHS three times in a shuffled order, ranks 32 / 20 / 4, 64 / 60 / 36, 10 / 50 / 101,
                      implicit and explicit feedback (dynamic_lambda on, and off once per padded rank)
    B  many rows      every resident launch holds more than 512 x (teams per workgroup) rows, so that team_grid gives every team a
                      second row: the row's indices come from the slot its previous row's sweeps filled, the slots of the previous
                      row are reused, and at k < KP the next row's pointers are requested behind the first sweep.  At rank <= 32
                      more than 512 streamed rows too.  The counts are asserted from the lengths before the device call, and the
                      kernel family of every bucket from the profile segments
    C  step counts    cg_steps 0, 1, 2, 4, 5, 8 on a matrix with long rows in the majority: both sides of kMaxSavedSweeps on the
                      streamed kernel (ranks 32, 20, 10), wrmf_ne.hip (64), wrmf_cg_mf.hip (128).  0 steps: bit-identical rows.
                      Again with 1, 2, 4, 5 steps on factors whose systems converge slowly, so that every step shows in the loss
    D  early exit     every other row starts from the oracle's 60-step solution and ends in its first CG step (|r|^2 < 1e-10),
                      its neighbour in the length-sorted order -- a row of the same length, so of the same launch and, in the
                      team kernels, of the same workgroup's barriers -- does not.  Once more behind a call that left NaNs in
                      every slot of the streamed kernel's saved-sweep scratch

Bounds, all the project's own: loss within 1e-4 relative, rel_fro below 1e-4, per row ||y - y64|| / ||y64|| <= max(1e-4, 3 err32)
with err32 that row's distance between the oracle in float and the oracle in double (tests/test_bias.py, tests/test_fuzz.py);
empty rows exactly the oracle's (zeros).  The yardstick must not swallow the test: every parametrisation asserts, on the oracle
alone and before the device call, that at most 5 % of the non-empty rows have a bound above 1e-4.  Inputs as the siblings': factors
N(0, 0.1^2), lambda 0.1, confidences 1 + Gamma(1, 2).

Every test prints its figures before it asserts (pytest -s, lines starting with `cg_rank_classes`):
profiles/cg_rank_classes/README.md."""
import ctypes

import numpy as np
import pytest

from conftest import rel_fro
from oracle import wrmf_oracle as O
from rsparse_amd import als

pytestmark = pytest.mark.gpu
TOL = 1e-4
YARDSTICK_SHARE = 0.05
N_ITEM = 3000
LAM, SCALE = 0.1, 0.1
CG = 1

EDGE_LENGTHS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 255, 256, 257, 511, 512, 513, 514, 527,
                528, 529, 640, 1023, 1024, 1025, 2300]

# wrmf_cgq.hip kBuckets: (waves, waves per row, resident quads per wave, streamed, longest row) of bucket 0..5
K_BUCKETS = {
    0: [(8, 8, 16, 1, None), (8, 8, 16, 0, 512), (4, 4, 16, 0, 256), (4, 2, 16, 0, 128), (4, 1, 16, 0, 64), (4, 1, 8, 0, 32)],
    1: [(8, 8, 16, 1, None), (4, 4, 32, 0, 512), (4, 2, 32, 0, 256), (4, 1, 32, 0, 128), (4, 1, 16, 0, 64), (4, 1, 8, 0, 32)],
}
# (shortest, longest, rows that give every team of the launch ONE row = 512 x teams per workgroup) per resident launch; at the
# padded rank 128 bucket 1 is three launches of one team per workgroup (kTeam4Max = 320, kTeam4WideMax = 384)
LAUNCHES = {
    "table0": [(1, 32, 2048), (33, 64, 2048), (65, 128, 1024), (129, 256, 512), (257, 512, 512)],
    "table0_streamed": [(1, 32, 2048), (33, 64, 2048), (65, 128, 1024), (129, 256, 512), (257, 512, 512), (513, 700, 512)],
    "table1": [(1, 32, 2048), (33, 64, 2048), (65, 128, 2048), (129, 256, 1024), (257, 512, 512)],
    "table0_rank128": [(1, 32, 2048), (33, 64, 2048), (65, 128, 1024), (129, 256, 512), (257, 320, 512), (321, 384, 512),
                       (385, 512, 512)],
}


def _padded_rank(k):
    return 32 if k <= 32 else (64 if k <= 64 else 128)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------

def _edge_lengths():
    """case A: every edge three times, shuffled (the kernels walk the rows longest first: a wrong mapping lands in a named row)"""
    lens = np.asarray(EDGE_LENGTHS * 3, dtype=np.int64)
    return lens[np.random.default_rng(41).permutation(lens.size)]


def _many_lengths(which):
    """case B: per launch its two edges twice and (rows + 8) lengths drawn once, shuffled, plus two empty rows"""
    rng = np.random.default_rng(77)
    parts = [np.zeros(2, dtype=np.int64)]
    for lo, hi, rows in LAUNCHES[which]:
        parts.append(np.asarray([lo, hi, lo, hi], dtype=np.int64))
        parts.append(rng.integers(lo, hi + 1, size=rows + 8))
    lens = np.concatenate(parts)
    return lens[rng.permutation(lens.size)]


def _step_lengths():
    """case C: 60 rows, 38 of them case A's lengths beyond 512 non-zeros, the rest one row per class edge"""
    long_rows = [n for n in EDGE_LENGTHS if n > 512]             # 10 lengths
    short_rows = [0, 1, 16, 17, 32, 33, 64, 65, 96, 127, 128, 129, 255, 256, 257, 320, 321, 384, 385, 511, 512, 2]
    lens = np.asarray(long_rows * 3 + [513, 514, 527, 640, 1023, 1024, 1025, 2300] + short_rows, dtype=np.int64)
    return lens[np.random.default_rng(43).permutation(lens.size)]


def _pair_lengths():
    """case D: every non-empty edge twice in a row -- columns 2 j (converged start) and 2 j + 1 (live) have the same length and
    are neighbours in the length-sorted order of the launches"""
    return np.repeat(np.asarray([n for n in EDGE_LENGTHS if n > 0], dtype=np.int64), 2)


_structures = {}


def _rows_of_lengths(lengths, n_item, k, seed, scale=SCALE):
    """a CSC (columns = the rows to solve) whose column j has lengths[j] distinct random items, values >= 1.  The sparsity and the
    values depend on (lengths, seed) only and are drawn once for all ranks; the factors on (seed, k)"""
    key = (lengths.tobytes(), n_item, seed)
    if key not in _structures:
        rng = np.random.default_rng(seed)
        p = np.zeros(len(lengths) + 1, dtype=np.int32)
        p[1:] = np.cumsum(lengths)
        idx = np.concatenate([np.sort(rng.choice(n_item, size=int(n), replace=False)) for n in lengths]).astype(np.int32)
        x = (1.0 + rng.gamma(1.0, 2.0, size=idx.size)).astype(np.float32).astype(np.float64)
        for a in (p, idx, x):
            a.setflags(write=False)
        _structures[key] = (p, idx, x)
    p, idx, x = _structures[key]
    rng = np.random.default_rng([seed, k])
    X = np.asfortranarray((rng.standard_normal((k, n_item)) * scale).astype(np.float32))
    Y0 = np.asfortranarray((rng.standard_normal((k, len(lengths))) * scale).astype(np.float32))
    return (n_item, len(lengths), p, idx, x), X, Y0


def _row_err(Y, Yref):
    return np.linalg.norm(Y - Yref, axis=0) / np.maximum(np.linalg.norm(Yref, axis=0), 1e-30)


def _oracle(csc, X, Y0, implicit, dyn, steps, dtype):
    _, _, p, i, x = csc
    Xd = np.asfortranarray(X, dtype=dtype)
    Y = np.asfortranarray(Y0, dtype=dtype).copy(order="F")
    if implicit:
        loss = O.als_implicit(p, i, x, Xd, Y, O.gramian(Xd, LAM), LAM, CG, steps, n_threads=8)
    else:
        cnt = np.bincount(i, minlength=csc[0]).astype(dtype)
        loss = O.als_explicit(p, i, x, Xd, Y, cnt, LAM, CG, steps, dyn, n_threads=8)
    return Y, loss


def _reference(tag, lens, csc, X, Y0, implicit, dyn, steps):
    """the oracle in double and in float, the per-row bound, and the cap on the yardstick -- asserted here, on the CPU"""
    Y64, l64 = _oracle(csc, X, Y0, implicit, dyn, steps, np.float64)
    Y32, _ = _oracle(csc, X, Y0, implicit, dyn, steps, np.float32)
    solved = lens > 0
    err32 = _row_err(Y32, Y64)
    bound = np.maximum(TOL, 3.0 * err32)
    share = float(np.mean(bound[solved] > TOL))
    q = dict(tag=tag, lens=lens, csc=csc, X=X, Y0=Y0, implicit=implicit, dyn=dyn, steps=steps, Y64=Y64, l64=l64, err32=err32,
             bound=bound, solved=solved, share=share)
    assert np.all(np.isfinite(Y64)) and np.all(np.isfinite(Y32))
    assert not Y64[:, ~solved].any()                     # an empty column comes back as zeros (implicit :281, explicit :142)
    assert share <= YARDSTICK_SHARE, ("the yardstick swallows the test", tag, share, float(err32[solved].max()))
    return q


def _device(q):
    csc, X = q["csc"], q["X"]
    Y = q["Y0"].copy(order="F")
    if q["implicit"]:
        loss = als.als_implicit(csc, X, Y, LAM, 1, CG, q["steps"], "float", False, False)
    else:
        cnt = np.bincount(csc[3], minlength=csc[0]).astype(np.float32)
        loss = als.als_explicit(csc, X, Y, cnt, LAM, 1, CG, q["steps"], q["dyn"], "float", False, False)
    return Y, loss


def _check(q, Y, loss):
    lens, Y64, l64, bound, solved = q["lens"], q["Y64"], q["l64"], q["bound"], q["solved"]
    err = np.where(solved, _row_err(Y, Y64), 0.0)
    worst = int(np.argmax(err / bound))
    fro, lerr = rel_fro(Y, Y64), abs(loss - l64) / abs(l64)
    print("cg_rank_classes %s rows=%d nnz=%d rel_fro=%.3g loss_err=%.3g worst_row_err=%.3g (row %d, %d non-zeros, bound %.3g) "
          "max_err32=%.3g share_above_1e-4=%.4f" % (q["tag"], len(lens), int(lens.sum()), fro, lerr, float(err[worst]), worst,
                                                   int(lens[worst]), float(bound[worst]), float(q["err32"][solved].max()),
                                                   q["share"]))
    assert np.isfinite(loss), loss
    assert np.all(np.isfinite(Y)), ("row %d" % int(np.flatnonzero(~np.isfinite(Y).all(axis=0))[0]))
    assert not Y[:, ~solved].any(), ("an empty row was written", int(np.flatnonzero(Y.any(axis=0) & ~solved)[0]))
    assert np.all(err <= bound), ("row %d of %d non-zeros" % (worst, int(lens[worst])), float(err[worst]), float(bound[worst]),
                                  float(q["err32"][worst]))
    assert fro < TOL, fro
    assert lerr <= TOL, (loss, l64)


# ---------------------------------------------------------------------------------------------------------------------------
# A. every class edge, every rank class
# ---------------------------------------------------------------------------------------------------------------------------

RANKS_A = [32, 20, 4, 64, 60, 36, 10, 50, 101]


def _case_a(k, implicit, dyn):
    lens = _edge_lengths()
    csc, X, Y0 = _rows_of_lengths(lens, N_ITEM, k, seed=100)
    tag = "A k=%d %s" % (k, "implicit" if implicit else ("explicit dynamic_lambda" if dyn else "explicit plain_lambda"))
    return _reference(tag, lens, csc, X, Y0, implicit, dyn, 3)


@pytest.mark.parametrize("implicit", [True, False])
@pytest.mark.parametrize("k", RANKS_A)
def test_every_class_edge_at_every_rank_class(k, implicit):
    """ranks 32 / 20 / 4: k = KP, k < KP and one quad of coordinates on <32>; 64 / 60 / 36 the same on geometry 1; 10 / 50 / 101
    the padded copies at 12 / 52 / 104.  Three rows on every edge of every launch, rows of 513 .. 2300 on the streamed kernel
    (rank <= 32) or the normal-equation kernel: 514 / 527 / 528 / 529 around the streamed prefix and its 16-wide blocks"""
    q = _case_a(k, implicit, True)
    assert sorted(set(q["lens"].tolist())) == EDGE_LENGTHS and min(np.bincount(q["lens"])[EDGE_LENGTHS]) >= 2
    Y, loss = _device(q)
    _check(q, Y, loss)


@pytest.mark.parametrize("k", [20, 60, 101])
def test_every_class_edge_explicit_without_dynamic_lambda(k):
    """lambda is not scaled by the row length: the diagonal term of the explicit sweeps is the plain lambda at every length"""
    q = _case_a(k, False, False)
    Y, loss = _device(q)
    _check(q, Y, loss)


# ---------------------------------------------------------------------------------------------------------------------------
# B. several rows per team
# ---------------------------------------------------------------------------------------------------------------------------

CASES_B = [(32, True), (12, True), (64, True), (64, False), (40, True), (40, False), (100, True), (128, False)]


def _launch_set(k):
    return "table0_streamed" if k <= 32 else ("table1" if k <= 64 else "table0_rank128")


def _assert_every_team_gets_a_second_row(lens, which):
    counts = {}
    for lo, hi, one_each in LAUNCHES[which]:
        n = int(((lens >= lo) & (lens <= hi)).sum())
        counts[(lo, hi)] = n
        assert n > one_each, (lo, hi, n, one_each)
        assert (lens == lo).sum() >= 2 and (lens == hi).sum() >= 2, (lo, hi)
    assert int(lens.sum()) <= 1_200_000
    return counts


def test_launch_sets_follow_the_bucket_table():
    """512 x teams per workgroup, from the copy of kBuckets above: the figures of LAUNCHES are not typed in twice by mistake"""
    for which, cfg in (("table0", 0), ("table1", 1)):
        resident = [b for b in K_BUCKETS[cfg] if not b[3]]
        by_longest = {b[4]: 512 * (b[0] // b[1]) for b in resident}
        assert {hi: rows for _, hi, rows in LAUNCHES[which]} == by_longest
    assert LAUNCHES["table0_streamed"][:5] == LAUNCHES["table0"] and LAUNCHES["table0_rank128"][:4] == LAUNCHES["table0"][:4]
    for which in LAUNCHES:
        _assert_every_team_gets_a_second_row(_many_lengths(which), which)


def _profiled(q):
    """the device call with the profile segments on: the names of the kernels that the buckets' segments timed"""
    from rsparse_amd import _lib
    lib = _lib.load()
    _lib.check(lib.rsparse_hip_profile_enable(1))
    try:
        Y, loss = _device(q)
        buf = ctypes.create_string_buffer(8192)
        _lib.check(lib.rsparse_hip_profile_last_names(buf, 8192))
    finally:
        _lib.check(lib.rsparse_hip_profile_enable(0))
    return Y, loss, buf.value.decode().split("\n")


def _assert_families(names, k, implicit):
    """segment b = bucket b of the launch table (its first launch that has rows); the template arguments are <KP, resident quads,
    waves, waves per row, streamed, implicit, matrix-core dense product, global bias, KFULL>"""
    kp = _padded_rank(k)
    table = K_BUCKETS[1 if kp == 64 else 0]
    short = [n.split("als_cgq_kernel", 1)[-1].split(">", 1)[0] + ">" if "als_cgq_kernel" in n else n for n in names[:6]]
    print("cg_rank_classes B k=%d kernels: %s" % (k, " | ".join(short)))
    for b, (waves, wpr, capq, stream, _) in enumerate(table):
        if stream and kp > 32:
            assert names[b] == "", names[b]      # rows beyond 512 non-zeros leave als_cgq_kernel above rank 32: the set has none
            continue
        # rank 128, implicit, one wave per row: the dense product on the matrix cores (1: <= 32 non-zeros, 2: 33..64)
        dmf = (1 if capq == 8 else 2) if (kp == 128 and implicit and waves == 4 and wpr == 1) else 0
        # KFULL: the instantiation for k == KP whose first sweep runs behind the gather (not streamed, not the <= 32 class of DMF)
        kfull = k == kp and not stream and dmf != 1
        want = "als_cgq_kernel<%d, %d, %d, %d, %d, %s, %d, false, %s>" % (kp, capq, waves, wpr, stream, str(implicit).lower(), dmf,
                                                                         str(kfull).lower())
        assert want in names[b], (b, want, names[b])


def _case_b(k, implicit):
    which = _launch_set(k)
    lens = _many_lengths(which)
    counts = _assert_every_team_gets_a_second_row(lens, which)
    csc, X, Y0 = _rows_of_lengths(lens, N_ITEM, k, seed=200)
    return _reference("B k=%d %s" % (k, "implicit" if implicit else "explicit"), lens, csc, X, Y0, implicit, True, 3), counts


@pytest.mark.parametrize("k,implicit", CASES_B)
def test_several_rows_per_team(k, implicit):
    """more than 512 x teams rows in every resident launch (and more than 512 streamed rows at rank <= 32): the second and later
    rows of a team at k = KP and at k < KP, implicit and explicit.  Rank 12 is also the padded copy of the reference's default
    rank 10; the profile segments name the kernel family that ran"""
    q, counts = _case_b(k, implicit)
    print("cg_rank_classes B k=%d rows per launch: %s" % (k, " ".join("%d..%d:%d" % (lo, hi, n) for (lo, hi), n in counts.items())))
    Y, loss, names = _profiled(q)
    _assert_families(names, k, implicit)
    _check(q, Y, loss)


# ---------------------------------------------------------------------------------------------------------------------------
# C. step counts
# ---------------------------------------------------------------------------------------------------------------------------

STEPS_C = [0, 1, 2, 4, 5, 8]
RANKS_C = [32, 20, 64, 128, 10]
STEPS_SLOW = [1, 2, 4, 5]
SLOW_TOP, SLOW_SPAN = 0.3, 10.0


def _case_c(k, steps, slow=False):
    lens = _step_lengths()
    assert len(lens) == 60 and (lens > 512).sum() == 38
    csc, X, Y0 = _rows_of_lengths(lens, N_ITEM, k, seed=300)
    if slow:   # coordinate i of every factor vector N(0, (SLOW_TOP * SLOW_SPAN^(-i / (k - 1)))^2)
        g = SLOW_TOP * SLOW_SPAN ** (-np.arange(k) / (k - 1.0))
        X = np.asfortranarray((X / SCALE * g[:, None]).astype(np.float32))
    return _reference("C%s k=%d steps=%d" % (" slow" if slow else "", k, steps), lens, csc, X, Y0, True, True, steps)


@pytest.mark.parametrize("steps", STEPS_C)
@pytest.mark.parametrize("k", RANKS_C)
def test_step_counts_on_long_rows(k, steps):
    """1..4 steps: the streamed kernel (ranks 32, 20 and 10 as 12) rebuilds t for the loss from the saved sweeps and alphas; 5 and 8
    steps and none take its other path.  Ranks 64 and 128 send the long rows to wrmf_ne.hip / wrmf_cg_mf.hip, whose step loops
    have no such split but no test beyond 3 steps either.  Implicit feedback"""
    q = _case_c(k, steps)
    lens = q["lens"]
    Y, loss = _device(q)
    if steps == 0:
        changed = np.flatnonzero((Y != q["Y0"]).any(axis=0) & q["solved"])
        assert changed.size == 0, ("row %d of %d non-zeros moved without a CG step" % (changed[0], int(lens[changed[0]])))
    _check(q, Y, loss)


@pytest.mark.parametrize("steps", STEPS_SLOW)
@pytest.mark.parametrize("k", RANKS_C)
def test_step_counts_where_every_step_moves_the_loss(k, steps):
    """With factors N(0, 0.1^2) the systems of the long rows are so well conditioned that the loss moves by 1e-6 of itself from the
    third CG step on: the loss that the streamed kernel rebuilds from its saved sweeps could leave the last ones out and stay
    within 1e-4.  Here the coordinates of the factor vectors fall off geometrically from 0.3 to 0.03: no row ends early, and
    every step up to the fifth moves the oracle's loss by more than five times the loss tolerance (8e-4 .. 8e-2 of it) --
    asserted on the oracle before the device call.  (Eight steps are left out: at rank 20 and below the float oracle then
    breaks down and the yardstick's cap fails.)"""
    q = _case_c(k, steps, slow=True)
    before = _oracle(q["csc"], q["X"], q["Y0"], True, True, steps - 1, np.float64)[1]
    assert abs(before - q["l64"]) > 5.0 * TOL * abs(q["l64"]), (before, q["l64"])
    Y, loss = _device(q)
    _check(q, Y, loss)


# ---------------------------------------------------------------------------------------------------------------------------
# D. early exit beside rows that go on
# ---------------------------------------------------------------------------------------------------------------------------

CASES_D = [(32, True), (20, True), (64, True), (36, True), (10, True), (64, False)]


def _case_d(k, implicit):
    lens = _pair_lengths()
    csc, X, Y0 = _rows_of_lengths(lens, N_ITEM, k, seed=400)
    Ysol, _ = _oracle(csc, X, Y0, implicit, True, 60, np.float64)
    Y0 = Y0.copy(order="F")
    Y0[:, ::2] = Ysol[:, ::2].astype(np.float32)
    q = _reference("D k=%d %s" % (k, "implicit" if implicit else "explicit"), lens, csc, X, Y0, implicit, True, 3)
    one_step, _ = _oracle(csc, X, Y0, implicit, True, 1, np.float64)
    stopped = (one_step == q["Y64"]).all(axis=0)
    assert stopped[::2].all(), ("a converged start went on", int(lens[::2][np.argmin(stopped[::2])]))
    assert not stopped[1::2].any()
    return q


@pytest.mark.parametrize("k,implicit", CASES_D)
def test_early_convergence_beside_rows_that_go_on(k, implicit):
    """tests/test_cg_pair_wide.py's construction at every class of case A: the even columns start from the oracle's 60-step
    solution rounded to float, and the oracle in double ends them in the first CG step (asserted: steps 2 and 3 change nothing);
    the odd ones do three steps.  A stopped row must keep its answer while its team sits through the barriers of the rows beside
    it, and the streamed kernel must not replay sweeps that a stopped row never saved"""
    q = _case_d(k, implicit)
    Y, loss = _device(q)
    _check(q, Y, loss)


@pytest.mark.parametrize("k", [32, 20])
def test_stopped_streamed_rows_do_not_replay_sweeps_they_never_saved(k):
    """A streamed row that ends in its first CG step writes the scratch slots of the first sweep and of step 1 only; the slots of
    steps 2 and 3 keep what an earlier call left there.  The call before this one solves the same matrix from a warm start of NaNs
    with four steps, so every slot of the scratch holds a NaN: a loss pass that multiplies a stale slot by an alpha of zero
    returns NaN.  (NaNs in a warm start change no address and no trip count: the step loop runs cg_steps times.)"""
    q = _case_d(k, True)
    poisoned = np.full_like(q["Y0"], np.nan)
    als.als_implicit(q["csc"], q["X"], poisoned, LAM, 1, CG, 4, "float", False, False)
    assert np.isnan(poisoned[:, q["solved"]]).all()
    Y, loss = _device(q)
    _check(q, Y, loss)
