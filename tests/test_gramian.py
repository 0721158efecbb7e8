"""The Gramian kernels per ELEMENT, with their two side outputs: G = X X^T + fl(lambda) I, sumsq = the trace before the ridge (the
regulariser term of the loss, engine.py scal[0]) and absmax = max |X| (the hint that saves the half-iteration its scan of X for the
fp16 operand scales, wrmf_ne.hip ne_stats_kernel).  Three kernel families write them:

    fp32   ranks 1..128     gramian_partial_kernel<32 | 64 | 128> + gramian_reduce_kernel (wrmf_kernels.hip): a wave takes 8 columns per
                            trip, gramian_waves(n) waves (one per 64 columns, at most 1024, a multiple of 4); a tail trip reads
                            column n - 1 / coordinate k - 1 again and multiplies the copy by 0; the per-wave partials are summed in
                            double and rounded once.  The only family that writes absmax
    wide   ranks 129..256   wide_gramian_partial_kernel + wide_gramian_reduce_kernel (wrmf_wide.hip): min(256, ceil(n / 64)) blocks of
                            ceil(n / blocks) columns each, staged 64, 32 or 16 at a time, partials summed in float in block order
    f64    ranks 1..128     f64_gramian_partial_kernel + f64_gramian_reduce_kernel (wrmf_f64.hip): the same geometry in double

The GPU tests call HipBackend.gramian(F, lam, out, sumsq_out, absmax_inout) on torch tensors (als.gramian, the host entry, cannot
reach the side outputs; one parametrisation per family goes through it all the same).

References, numpy only:
    exact     F integer-valued in [-4, 4] (coordinate 0 non-negative, coordinate k // 2 shifted by 2: no two coordinates of a
              mirrored or transposed tile look alike), scaled by s = 2^-40, 1 or 2^40.  Every product and every partial sum is then
              exact in fp32 as long as 16 n < 2^24 (asserted), so G, sumsq and absmax must EQUAL s^2 (F F^T in integers), s^2 trace
              and s max |F|, with the ridge added as the kernel adds it: float32(g) + float32(lam) in float32 (fp32, wide),
              g + float(float32(lam)) in double (f64).  No tolerance
    rounded   F ~ N(0, 1), coordinate 0 + 3, cast to the kernel's type; ref = the float64 product, S = |F| |F|^T; per element
              |G - ref| <= (m + 4) u S with u = 2^-24 (fp32, wide) or 2^-53 (f64) and m the longest chain of additions the launch
              geometry allows: fp32 m = 8 ceil(n / (8 waves)), wide and f64 m = ceil(n / blocks) + blocks.  That is the worst-case
              bound of a sum of m rounded terms (+ 4 for the products, the final rounding, the ridge and the reference's own
              rounding): derived, not tuned.  sumsq by the same rule against its float64 value

The unmarked tests at the end show on the CPU that both comparators reject a Gramian that is wrong by one column, one ridge or one
transposed tile, and that the kernels' own summation orders, simulated in numpy, pass the rounded one.

Every test prints its figures before it asserts (pytest -s, lines starting with `gramian_tests`): profiles/gramian_tests/README.md."""
import functools

import numpy as np
import pytest

gpu = pytest.mark.gpu

U = {"fp32": 2.0 ** -24, "wide": 2.0 ** -24, "f64": 2.0 ** -53}
SCALES = (2.0 ** -40, 1.0, 2.0 ** 40)
LAMS = (0.0, 0.1)
LAM = 0.1

FP32_RANKS = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128]
FP32_COLS = [0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4097, 20011, 65472, 65473, 65537, 131073]
FP32_BIG_RANKS = (5, 33, 97, 128)     # the four largest column counts run at these ranks only
WIDE_RANKS = [129, 130, 131, 132, 160, 191, 192, 193, 255, 256]
WIDE_COLS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 16384, 16385, 16639, 70001]
F64_RANKS = [1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 100, 127, 128]
N_MAX = 131073

ROUNDED = [("fp32", 5), ("fp32", 33), ("fp32", 64), ("fp32", 128), ("wide", 129), ("wide", 193), ("wide", 256), ("f64", 33), ("f64", 128)]


def _np_dtype(family):
    return np.float64 if family == "f64" else np.float32


def _cols(family):
    return FP32_COLS if family == "fp32" else WIDE_COLS


def _rounded_ns(family):
    return [9, 257, 4097, 20011, 131073 if family == "fp32" else 70001]


# ---------------------------------------------------------------------------------------------------------------------------
# launch geometry (wrmf_kernels.hip gramian_waves, launch_gramian_wide, launch_f64_gramian)
# ---------------------------------------------------------------------------------------------------------------------------

def gramian_waves(n):
    w = min(1024, max(1, (n + 63) // 64))
    return (w + 3) // 4 * 4


def gramian_blocks(n):
    return max(1, min(256, (n + 63) // 64))


def chain(family, n):
    """the longest chain of additions behind one element of G"""
    if family == "fp32":
        return 8 * -(-n // (8 * gramian_waves(n)))
    return -(-n // gramian_blocks(n)) + gramian_blocks(n)


# ---------------------------------------------------------------------------------------------------------------------------
# the exact reference
# ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _int_base():
    b = np.random.default_rng(20011).integers(-4, 5, size=(N_MAX, 256), dtype=np.int8)
    b.setflags(write=False)
    return b


def int_factors(k, n):
    """(n, k) int64 in [-4, 4]: coordinate 0 non-negative, coordinate k // 2 shifted by 2 (and clipped)"""
    F = _int_base()[:n, :k].astype(np.int64)
    F[:, 0] = np.abs(F[:, 0])
    if k > 1:
        F[:, k // 2] = np.clip(F[:, k // 2] + 2, -4, 4)
    return F


def int_gramian(F):
    """F^T F of an integer matrix, in int64.  (Through the float64 product: every sum stays far below 2^53, so it is the integer
    result, which the conversion back asserts -- numpy's own int64 product takes seconds at the large shapes.)"""
    Ff = F.astype(np.float64)
    g = Ff.T @ Ff
    gi = np.rint(g).astype(np.int64)
    assert np.array_equal(gi.astype(np.float64), g)
    return gi


def assemble(g, ridge, family):
    """the ridge on the diagonal of g (float64, exactly representable in the family's type) as that family's kernel adds it"""
    if family == "f64":
        G = np.array(g, dtype=np.float64)
        G[np.diag_indices_from(G)] += float(np.float32(ridge))
        return G
    G = g.astype(np.float32)
    assert np.array_equal(G.astype(np.float64), g), "the exact reference does not fit float32"
    d = np.diagonal(G) + np.float32(ridge)
    assert d.dtype == np.float32
    G[np.diag_indices_from(G)] = d
    return G


def exact_from_ints(gi, amax, s, lam, family):
    """(G, sumsq, absmax) from the integer Gramian gi of F, max |F| and the scale s of the factors"""
    assert int(np.abs(gi).max(initial=0)) < 2 ** 24, "a partial sum could round in float32"
    g = (s * s) * gi.astype(np.float64)
    return assemble(g, lam, family), (s * s) * float(np.trace(gi)), np.float32(s * amax)


def exact_ref(F, s, lam, family):
    n = F.shape[0]
    assert 16 * n < 2 ** 24
    return exact_from_ints(int_gramian(F), int(np.abs(F).max(initial=0)), s, lam, family)


def check_exact(G, sumsq, absmax, ref, what=()):
    """G, sumsq (None: not produced) and absmax (None: not produced) equal the reference's; G is symmetric"""
    Gr, sr, ar = ref
    assert G.dtype == Gr.dtype and G.shape == Gr.shape, (what, G.dtype, G.shape)
    bad = np.argwhere(~(G == Gr))
    assert bad.size == 0, (what, len(bad), [(int(i), int(j), float(G[i, j]), float(Gr[i, j])) for i, j in bad[:4]])
    assert np.array_equal(G, G.T), what
    if sumsq is not None:
        assert float(sumsq) == sr, (what, "sumsq", float(sumsq), sr)
    if absmax is not None:
        assert np.float32(absmax) == ar, (what, "absmax", float(absmax), float(ar))


# ---------------------------------------------------------------------------------------------------------------------------
# the rounded reference
# ---------------------------------------------------------------------------------------------------------------------------

def cont_factors(k, n, family):
    rng = np.random.default_rng([k, n, 7])
    F = rng.standard_normal((n, k))
    F[:, 0] += 3.0
    return F.astype(_np_dtype(family))


def rounded_ref(F, lam):
    """(ref with the ridge, S, sumsq) in float64 of the factors as the kernel sees them"""
    F64 = F.astype(np.float64)
    ref = F64.T @ F64
    sumsq = float(np.trace(ref))
    ref[np.diag_indices_from(ref)] += float(np.float32(lam))
    A = np.abs(F64)
    return ref, A.T @ A, sumsq


def rounded_ratios(G, sumsq, ref, family):
    """(worst |G - ref| / (u S) over the elements, |sumsq - ref| / (u ref))"""
    Gr, S, sr = ref
    u = U[family]
    return float((np.abs(G.astype(np.float64) - Gr) / (u * S)).max()), abs(float(sumsq) - sr) / (u * sr)


def check_rounded(G, sumsq, ref, family, n, what=()):
    m = chain(family, n)
    assert G.dtype == _np_dtype(family)
    worst, ws = rounded_ratios(G, sumsq, ref, family)
    assert np.array_equal(G, G.T), what
    assert worst <= m + 4, (what, "G", worst, m + 4)
    assert ws <= m + 4, (what, "sumsq", ws, m + 4)
    return worst, ws


# ---------------------------------------------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _be():
    from rsparse_amd.engine import HipBackend
    return HipBackend()


def _upload(F, family):
    import torch
    return _be().to_device(np.ascontiguousarray(F, dtype=_np_dtype(family)), torch.float64 if family == "f64" else torch.float32)


def _run(Fd, lam, absmax0=0.0, with_absmax=True):
    """one Gramian of the (n, k) device tensor Fd into poisoned outputs -> (G, sumsq, absmax word) on the host"""
    import torch
    be = _be()
    k = Fd.shape[1]
    G = torch.full((k, k), float("nan"), dtype=Fd.dtype, device=be.device)
    sumsq = torch.full((1,), float("nan"), dtype=torch.float64, device=be.device)
    word = torch.tensor([absmax0], dtype=torch.float32, device=be.device)
    be.gramian(Fd, lam, G, sumsq, word if with_absmax else None)
    return G.cpu().numpy(), float(sumsq.cpu()[0]), np.float32(word.cpu().numpy()[0])


def _family(k, dtype_family):
    return "f64" if dtype_family == "f64" else ("wide" if k > 128 else "fp32")


# ---------------------------------------------------------------------------------------------------------------------------
# 1  rank x column grid, exact
# ---------------------------------------------------------------------------------------------------------------------------

GRID = ([("fp32", k, "device") for k in FP32_RANKS] + [("wide", k, "device") for k in WIDE_RANKS] +
        [("f64", k, "device") for k in F64_RANKS] + [("fp32", 33, "host"), ("wide", 131, "host"), ("f64", 33, "host")])


@gpu
@pytest.mark.parametrize("family,k,entry", GRID)
def test_grid_exact(family, k, entry):
    """every column count of the family's list, lambda 0 and 0.1, the factors at 2^-40, 1 and 2^40: G, sumsq and absmax bit for bit.
    n = 0 is an empty slice of a non-empty tensor (no address): G = ridge I, sumsq = 0, absmax as it was"""
    from rsparse_amd import als
    calls = 0
    for n in _cols(family):
        if family == "fp32" and n > 20011 and k not in FP32_BIG_RANKS:
            continue
        F = int_factors(k, n)
        gi, amax = int_gramian(F), int(np.abs(F).max(initial=0))
        assert 16 * n < 2 ** 24
        Fd = _upload(F if n else int_factors(k, 4), family) if entry == "device" else None
        for s in SCALES:
            if entry == "device":
                Fs = Fd * s
                Fs = Fs if n else Fs[2:2]
                assert tuple(Fs.shape) == (n, k)
            else:
                X = np.asfortranarray(F.T.astype(_np_dtype(family)) * _np_dtype(family)(s))
            for lam in LAMS:
                ref = exact_from_ints(gi, amax, s, lam, family)
                what = (family, k, n, s, lam, entry)
                if entry == "host":
                    check_exact(als.gramian(X, lam, "double" if family == "f64" else "float"), None, None, ref, what)
                elif n == 0:
                    G, sumsq, word = _run(Fs, lam, absmax0=0.75)
                    check_exact(G, sumsq, word, (ref[0], 0.0, np.float32(0.75)), what)
                else:
                    G, sumsq, word = _run(Fs, lam)
                    check_exact(G, sumsq, word if family == "fp32" else None, ref, what)
                calls += 1
    print("gramian_tests grid family=%s k=%d entry=%s calls=%d all exact" % (family, k, entry, calls))


# ---------------------------------------------------------------------------------------------------------------------------
# 2  rounded reference
# ---------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("family,k", ROUNDED)
def test_rounded(family, k):
    rows = []
    for n in _rounded_ns(family):
        F = cont_factors(k, n, family)
        ref = rounded_ref(F, LAM)
        G, sumsq, word = _run(_upload(F, family), LAM)
        worst, ws = rounded_ratios(G, sumsq, ref, family)
        print("gramian_tests rounded family=%s k=%d n=%d m=%d worst_err_over_uS=%.3f sumsq_err_over_u=%.3f"
              % (family, k, n, chain(family, n), worst, ws))
        rows.append((n, G, sumsq, ref, word, F))
    for n, G, sumsq, ref, word, F in rows:
        check_rounded(G, sumsq, ref, family, n, (family, k, n))
        if family == "fp32":
            assert word == np.abs(F).max(), (n, word)


# ---------------------------------------------------------------------------------------------------------------------------
# 3  views at an offset
# ---------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("family,k", [("fp32", 5), ("fp32", 33), ("fp32", 127), ("wide", 131), ("f64", 33)])
def test_views_off_the_16_byte_grid(family, k):
    """F = big[a:a + n] at an odd rank (what a sharded fit passes): the slice's own Gramian; the rows around it hold 1e30"""
    calls = 0
    for a in (1, 3):
        for n in (1, 9, 257, 4097):
            F = int_factors(k, n + 7)[7:]          # (another window of the base matrix than the grid's)
            big = np.full((a + n + 2, k), 1e30, dtype=_np_dtype(family))
            big[a:a + n] = F
            view = _upload(big, family)[a:a + n]
            assert view.data_ptr() % 16 != 0 and view.is_contiguous()
            for lam in LAMS:
                G, sumsq, word = _run(view, lam)
                check_exact(G, sumsq, word if family == "fp32" else None, exact_ref(F, 1.0, lam, family), (family, k, a, n, lam))
                calls += 1
    print("gramian_tests views family=%s k=%d calls=%d all exact" % (family, k, calls))


# ---------------------------------------------------------------------------------------------------------------------------
# 4  where the maximum sits
# ---------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("k", [33, 97, 128])
def test_where_the_maximum_sits(k):
    """one entry of +-100 at the first / last coordinate, coordinates 31 and 32, in column 0 and in each of the last 8 columns (every
    residue of the last trip): absmax = 100 and G stays exact -- the clamped tail reads read that very entry again"""
    calls = 0
    for n in (9, 257, 65537):
        F = int_factors(k, n)
        Fd = _upload(F, "fp32")
        g0 = int_gramian(F)
        for c in sorted({0, 31, 32, k - 1}):
            for j in sorted({0, *range(max(0, n - 8), n)}):
                for v in (100, -100):
                    x, x2 = F[j].copy(), F[j].copy()
                    x2[c] = v
                    gi = g0 - np.outer(x, x) + np.outer(x2, x2)
                    Fd[j, c] = float(v)
                    G, sumsq, word = _run(Fd, LAM)
                    Fd[j, c] = float(F[j, c])
                    check_exact(G, sumsq, word, exact_from_ints(gi, 100, 1.0, LAM, "fp32"), (k, n, c, j, v))
                    calls += 1
        G, sumsq, word = _run(Fd, LAM)     # (and the matrix is as it was)
        check_exact(G, sumsq, word, exact_ref(F, 1.0, LAM, "fp32"), (k, n, "restored"))
    print("gramian_tests maximum k=%d calls=%d all exact" % (k, calls))


# ---------------------------------------------------------------------------------------------------------------------------
# 5  absmax in / out
# ---------------------------------------------------------------------------------------------------------------------------

@gpu
def test_absmax_contract():
    import torch
    be = _be()
    k, n = 33, 257
    F = int_factors(k, n)
    Fd = _upload(F, "fp32")
    ref = exact_ref(F, 1.0, LAM, "fp32")
    assert ref[2] == 4.0
    # content above max |F| stays, content below is replaced
    G, sumsq, word = _run(Fd, LAM, absmax0=1000.0)
    check_exact(G, sumsq, word, (ref[0], ref[1], np.float32(1000.0)))
    G, sumsq, word = _run(Fd, LAM, absmax0=1.0)
    check_exact(G, sumsq, word, ref)
    # None is accepted
    G, sumsq, word = _run(Fd, LAM, absmax0=0.5, with_absmax=False)
    check_exact(G, sumsq, word, (ref[0], ref[1], np.float32(0.5)))
    # two slices in succession: the maximum over both, whichever comes first
    F2 = F.copy()
    F2[40, 7], F2[200, 32] = -7, 9
    F2d = _upload(F2, "fp32")
    for first, second, after_first in (((0, 100), (100, n), 7.0), ((100, n), (0, 100), 9.0)):
        Gd = torch.zeros((k, k), dtype=torch.float32, device=be.device)
        word = torch.zeros(1, dtype=torch.float32, device=be.device)
        be.gramian(F2d[first[0]:first[1]], 0.0, Gd, None, word)
        assert float(word.cpu()[0]) == after_first
        G1 = Gd.cpu().numpy()
        be.gramian(F2d[second[0]:second[1]], 0.0, Gd, None, word)
        assert float(word.cpu()[0]) == 9.0
        check_exact(G1 + Gd.cpu().numpy(), None, None, exact_ref(F2, 1.0, 0.0, "fp32"), ("two slices", first))
    # an inf in F: the largest finite hint the long-row kernels take
    for j, c in ((0, 0), (n - 1, k - 1), (130, 5)):
        Fi = Fd.clone()
        Fi[j, c] = float("-inf")
        assert _run(Fi, LAM)[2] == np.float32(3.0e38)
    # at a wide rank the word is left as it was (only the rank <= 128 long-row kernels read it: include/rsparse_wrmf_hip.h)
    Fw = int_factors(131, 300)
    G, sumsq, word = _run(_upload(Fw, "fp32"), LAM, absmax0=0.5)
    rw = exact_ref(Fw, 1.0, LAM, "wide")
    check_exact(G, sumsq, word, (rw[0], rw[1], np.float32(0.5)))
    print("gramian_tests absmax contract holds")


# ---------------------------------------------------------------------------------------------------------------------------
# 6  the hint changes nothing
# ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _long_row_matrix():
    """CSC whose columns (the rows to solve) have 513, 700, 1100 and 2300 non-zeros, ten of each, and a few short ones"""
    rng = np.random.default_rng(61)
    n_item = 3000
    lens = np.asarray([513, 700, 1100, 2300] * 10 + [0, 1, 17, 64, 300, 512], dtype=np.int64)
    lens = lens[rng.permutation(lens.size)]
    p = np.zeros(lens.size + 1, dtype=np.int32)
    p[1:] = np.cumsum(lens)
    idx = np.concatenate([np.sort(rng.choice(n_item, size=int(m), replace=False)) for m in lens]).astype(np.int32)
    x = (1.0 + rng.gamma(1.0, 2.0, size=idx.size)).astype(np.float32)
    return n_item, int(lens.size), p, idx, x


@gpu
@pytest.mark.parametrize("solver", [1, 0], ids=["cg3", "exact"])
@pytest.mark.parametrize("k", [64, 128])
def test_hint_changes_nothing(k, solver):
    """half_iteration(absmax = the Gramian's word) against half_iteration(absmax = None): the same rows and the same loss, bit for bit,
    because the word IS max |F| bit for bit (rows beyond 512 non-zeros: wrmf_ne.hip at rank 64, wrmf_cg_mf.hip at rank 128)"""
    import torch
    be = _be()
    n_item, n_cols, p, idx, x = _long_row_matrix()
    h = be.make_csc(n_item, n_cols, be.to_device(p.copy(), torch.int32), be.to_device(idx.copy(), torch.int32),
                    be.to_device(x.copy(), torch.float32))
    rng = np.random.default_rng([k, solver])
    F0 = rng.standard_normal((n_item, k)) * 0.1
    Y0 = rng.standard_normal((n_cols, k)) * 0.1
    for scale in (2.0 ** -10, 1.0, 2.0 ** 10):
        Fd = be.to_device((F0 * scale).astype(np.float32), torch.float32)
        G = torch.zeros((k, k), dtype=torch.float32, device=be.device)
        sumsq = torch.zeros(1, dtype=torch.float64, device=be.device)
        word = torch.zeros(1, dtype=torch.float32, device=be.device)
        be.gramian(Fd, LAM, G, sumsq, word)
        assert torch.equal(word.view(torch.int32), Fd.abs().max().reshape(1).view(torch.int32)), (scale, float(word))
        res = []
        for hint in (word, None):
            Yd = be.to_device((Y0 / scale).astype(np.float32), torch.float32)
            loss = torch.zeros(1, dtype=torch.float64, device=be.device)
            be.half_iteration(h, True, Fd, Yd, G, LAM, solver, 3, False, loss, absmax=hint)
            res.append((Yd.cpu(), loss.cpu()))
        (Y1, l1), (Y2, l2) = res
        assert bool(torch.isfinite(Y1).all()) and bool(torch.isfinite(l1).all())
        assert not torch.equal(Y1, torch.as_tensor((Y0 / scale).astype(np.float32)))
        differ = torch.nonzero((Y1.view(torch.int32) != Y2.view(torch.int32)).any(dim=1)).flatten().tolist()
        assert not differ, (scale, [(c, int(p[c + 1] - p[c])) for c in differ[:8]])
        assert torch.equal(l1.view(torch.int64), l2.view(torch.int64)), (scale, float(l1), float(l2))
    print("gramian_tests hint k=%d solver=%d rows and loss bit-identical at 3 scales" % (k, solver))


# ---------------------------------------------------------------------------------------------------------------------------
# 7  scratch reuse and repeatability
# ---------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("family", ["fp32", "wide", "f64"])
def test_scratch_reuse_and_repeatability(family):
    """a large call, then small ones of other shapes on the same grow-only scratch (the wide and the fp32 kernels share it): a
    stale partial of the larger call must not reach a later result.  Then the large call twice: bit-identical"""
    kbig = 256 if family == "wide" else 128
    seq = [(kbig, 70001), (5, 3), (33, 257)] + ([(129, 3), (131, 257)] if family == "wide" else []) + [(kbig, 70001), (5, 3)]
    for k, n in seq:
        fam = _family(k, family)
        F = int_factors(k, n)
        G, sumsq, word = _run(_upload(F, fam), LAM)
        check_exact(G, sumsq, word if fam == "fp32" else None, exact_ref(F, 1.0, LAM, fam), (family, k, n))
    Fd = _upload(cont_factors(kbig, 70001, family), family)
    G1, s1, w1 = _run(Fd, LAM)
    _run(_upload(int_factors(33, 257), _family(33, family)), LAM)
    G2, s2, w2 = _run(Fd, LAM)
    assert np.array_equal(G1, G2) and s1 == s2 and w1 == w2 and np.isfinite(G1).all()
    print("gramian_tests scratch family=%s %d calls exact, repeat bit-identical" % (family, len(seq)))


# ---------------------------------------------------------------------------------------------------------------------------
# 8  ShardedALS.gramian with several pieces
# ---------------------------------------------------------------------------------------------------------------------------

def _sharded(n, k, family, n_sub, with_bias=False):
    """a one-process ShardedALS (no process group) whose user side is stored in n_sub pieces; every user has one item"""
    import torch
    from rsparse_amd.engine import Layout, ShardedALS
    be = _be()
    tdt = torch.float64 if family == "f64" else torch.float32
    n_item = 8
    users = np.arange(n, dtype=np.int32)
    items = users % n_item
    order = np.argsort(items, kind="stable")
    p_ui = np.concatenate([[0], np.cumsum(np.bincount(items, minlength=n_item))]).astype(np.int32)
    c_ui = (be.to_device(p_ui, torch.int32), be.to_device(users[order], torch.int32), torch.ones(n, dtype=tdt, device=be.device))
    c_iu = (be.to_device(np.arange(n + 1, dtype=np.int32), torch.int32), be.to_device(items, torch.int32),
            torch.ones(n, dtype=tdt, device=be.device))
    lay_u, lay_i = Layout(n, [(0, n)], n_sub), Layout(n_item, [(0, n_item)], 1)
    als = ShardedALS(be, n, n_item, k, c_ui, c_iu, n, feedback="implicit", lambda_=LAM, cg_steps=3, group=None, world_size=1,
                     my_rank=0, with_bias=with_bias, lay_user=lay_u, lay_item=lay_i)
    return als, lay_u


def _storage(lay, F, family):
    """F in the layout's storage order on the device; the padding rows hold 1e30 (nothing may read them)"""
    import torch
    S = lay.alloc(F.shape[1], _be().device, torch.float64 if family == "f64" else torch.float32)
    S.fill_(1e30)
    return lay.from_global(S, _upload(F, family))


@gpu
@pytest.mark.parametrize("family", ["fp32", "f64"])
@pytest.mark.parametrize("k", [33, 128])
def test_sharded_gramian_in_pieces(k, family):
    """four pieces at lambda = 0, summed, the ridge added once afterwards: exact, and equal to the one-piece result"""
    n = 1003     # pieces of 251, 251, 251 and 250 rows + one padding row: pieces 1..3 start off the 16-byte grid at rank 33
    F = int_factors(k, n)
    out = {}
    for n_sub in (1, 4):
        als, lay = _sharded(n, k, family, n_sub)
        assert len(als._my_pieces(lay)) == n_sub
        Fd = _storage(lay, F, family)
        G = als.gramian(Fd, lay)
        assert als.absmax_of is Fd
        out[n_sub] = (G.cpu().numpy(), float(als.scal[0].cpu()), np.float32(als.absmax.cpu().numpy()[0]))
    ref = exact_ref(F, 1.0, LAM, family)
    for n_sub, (G, sumsq, word) in out.items():
        check_exact(G, sumsq, word if family == "fp32" else None, ref, (family, k, n_sub))
    assert np.array_equal(out[1][0], out[4][0]) and out[1][1:] == out[4][1:]
    print("gramian_tests sharded family=%s k=%d 1 and 4 pieces exact and equal" % (family, k))


@gpu
@pytest.mark.parametrize("bias_last", [True, False])
@pytest.mark.parametrize("k", [34, 129])
def test_sharded_gramian_bias(k, bias_last):
    """the (k - 1) x (k - 1) Gramian of F without its bias coordinate, four pieces; order 129 takes it on the fp32 kernel"""
    n = 1003
    F = int_factors(k, n)
    als, lay = _sharded(n, k, "fp32", 4, with_bias=True)
    Gb = als.gramian_bias(_storage(lay, F, "fp32"), lay, bias_last).cpu().numpy()
    check_exact(Gb, None, None, exact_ref(F[:, :k - 1] if bias_last else F[:, 1:], 1.0, LAM, "fp32"), (k, bias_last))
    print("gramian_tests sharded bias k=%d bias_last=%s exact" % (k, bias_last))


# ---------------------------------------------------------------------------------------------------------------------------
# 9  CPU: the comparators reject near misses, the kernels' summation orders pass
# ---------------------------------------------------------------------------------------------------------------------------

MUTATIONS = ["none", "last column dropped", "last column twice", "ridge missing", "ridge doubled", "tile (1, 0) transposed",
             "sumsq after the ridge"]
NEAR_SHAPES = [(f, k, n) for f, k in ROUNDED for n in (9, 257, 4097)]


def mutated(name, g, x, lam, to_type):
    """(G, sumsq) of a kernel that is wrong in one way.  g: the float64 Gramian without its ridge, x: the last column"""
    g, ridge = g.copy(), float(np.float32(lam))
    k = g.shape[0]
    if name == "last column dropped":
        g -= np.outer(x, x)
    if name == "last column twice":
        g += np.outer(x, x)
    sumsq = float(np.trace(g))
    if name == "ridge missing":
        ridge = 0.0
    if name == "ridge doubled":
        ridge = 2.0 * float(np.float32(lam))
    if name == "tile (1, 0) transposed":      # (32 x 32 as the kernels' tiles; at a small rank the tile of half the rank)
        T = 32 if k >= 64 else k // 2
        g[T:2 * T, :T] = g[T:2 * T, :T].T.copy()
        g[:T, T:2 * T] = g[T:2 * T, :T].T
    G = to_type(g, ridge)
    if name == "sumsq after the ridge":
        sumsq = float(np.trace(G.astype(np.float64)))
    return G, sumsq


def _expect(name, fn):
    if name == "none":
        fn()
        return
    with pytest.raises(AssertionError):
        fn()


@pytest.mark.parametrize("family,k,n", NEAR_SHAPES)
def test_rounded_comparator_rejects_near_misses(family, k, n):
    F = cont_factors(k, n, family)
    ref = rounded_ref(F, LAM)
    g = F.astype(np.float64).T @ F.astype(np.float64)

    def to_type(g_, ridge):
        return (g_ + ridge * np.eye(k)).astype(_np_dtype(family))
    for name in MUTATIONS:
        G, sumsq = mutated(name, g, F[-1].astype(np.float64), LAM, to_type)
        _expect(name, lambda: check_rounded(G, sumsq, ref, family, n, name))


@pytest.mark.parametrize("family,k,n", NEAR_SHAPES + [(f, k, N_MAX) for f, k in ROUNDED])
def test_exact_comparator_rejects_near_misses(family, k, n):
    F = int_factors(k, n)
    ref = exact_ref(F, 1.0, LAM, family)
    g = int_gramian(F).astype(np.float64)
    for name in MUTATIONS:
        G, sumsq = mutated(name, g, F[-1].astype(np.float64), LAM, lambda g_, ridge: assemble(g_, ridge, family))
        _expect(name, lambda: check_exact(G, sumsq, ref[2], ref, name))
    with pytest.raises(AssertionError):
        check_exact(ref[0], ref[1], np.float32(3.0), ref)       # a stale absmax
    if k > 1:
        G = ref[0].copy()
        G[k - 1, 0] = np.nextafter(G[k - 1, 0], np.inf)          # one bit in one element, its mirror right
        with pytest.raises(AssertionError):
            check_exact(G, ref[1], ref[2], ref)


def simulate(F, lam, family):
    """(G, sumsq) in the kernel's summation order, every addition rounded to the kernel's type: the columns a wave (fp32) or a block
    (wide, f64) takes, one after the other into its partial; the partials in order -- in double and rounded once (fp32:
    gramian_reduce_kernel), in the kernel's type (wide, f64).  (A product is rounded before it is added here; the kernels fuse.)"""
    n, k = F.shape
    dt = _np_dtype(family)
    c = np.arange(n)
    if family == "fp32":
        groups = gramian_waves(n)
        grp, step = (c // 8) % groups, (c // 8) // groups * 8 + c % 8
    else:
        groups = gramian_blocks(n)
        per = -(-n // groups)
        grp, step = c // per, c % per
    steps = int(step.max()) + 1
    assert steps <= chain(family, n)
    col = np.full((groups, steps), n, dtype=np.int64)
    col[grp, step] = c
    Fp = np.concatenate([F.astype(dt), np.zeros((1, k), dtype=dt)])
    acc = np.zeros((groups, k, k), dtype=dt)
    for t in range(steps):
        X = Fp[col[:, t]]
        acc += X[:, :, None] * X[:, None, :]
    if family == "fp32":
        s = acc.astype(np.float64).sum(axis=0)     # (exact enough: doubles of floats, at most 1024 of them)
        diag = np.diagonal(s).copy()
        G = s.astype(np.float32)
    else:
        G = np.zeros((k, k), dtype=dt)
        for b in range(groups):
            G += acc[b]
        diag = np.diagonal(G).astype(np.float64)
    G[np.diag_indices(k)] = np.diagonal(G) + (np.float32(lam) if family != "f64" else float(np.float32(lam)))
    assert G.dtype == dt
    return G, float(diag.sum())


@pytest.mark.parametrize("family,k,n", NEAR_SHAPES)
def test_simulated_summation_order_passes(family, k, n):
    F = cont_factors(k, n, family)
    G, sumsq = simulate(F, LAM, family)
    ref = rounded_ref(F, LAM)
    worst, ws = rounded_ratios(G, sumsq, ref, family)
    print("gramian_tests simulated family=%s k=%d n=%d m=%d worst_err_over_uS=%.3f sumsq_err_over_u=%.3f"
          % (family, k, n, chain(family, n), worst, ws))
    check_rounded(G, sumsq, ref, family, n)


def test_simulated_order_is_exact_on_integers():
    """the simulation and the exact reference agree where nothing rounds: the two references check each other"""
    for family, k, n in (("fp32", 33, 4097), ("wide", 131, 700), ("f64", 5, 257)):
        F = int_factors(k, n)
        G, sumsq = simulate(F.astype(_np_dtype(family)), LAM, family)
        check_exact(G, sumsq, None, exact_ref(F, 1.0, LAM, family))


def test_launch_geometry():
    assert [gramian_waves(n) for n in (0, 1, 256, 257, 65472, 65473, 65537, 131073)] == [4, 4, 4, 8, 1024, 1024, 1024, 1024]
    assert [chain("fp32", n) for n in (9, 257, 4097, 65537, 131073)] == [8, 40, 64, 72, 136]
    assert [chain("wide", n) for n in (9, 64, 65, 16384, 16385, 70001)] == [10, 65, 35, 320, 321, 530]
