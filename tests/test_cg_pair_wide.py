"""The last bucket of the quad-layout CG kernels (rows of at most 32 non-zeros) at rank 128, implicit feedback, no global bias,
runs two rows per wave in both of its launches (wrmf_cgp.hip): the rows of 17..32 non-zeros in 32 slots per half-wave, the
rows of at most 16 in 16 slots.  Checked per row against the fp64 oracle at the parity tolerances of tests/test_hip_parity.py:
rows at every edge (0, 1, 8, 9, 16, 17, 31, 32, 33 non-zeros), pairs whose two rows differ in length, odd row counts that
leave a half-wave idle, rows that converge in the first CG step beside rows that do not, confidences below 1, and two- and
four-rank contexts whose shards cut the bucket."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import rel_fro
from oracle import wrmf_oracle as O
from rsparse_amd import als

pytestmark = pytest.mark.gpu
TOL = 1e-4
ROW_TOL = 5e-4   # per row, as tests/test_hip_parity.py::test_cg_long_rows_all_buckets

EDGES = [0, 1, 8, 9, 16, 17, 31, 32, 33]
LENGTHS = {
    "edges": EDGES * 3,
    "wide_only_odd": [17, 18, 24, 25, 31, 32] * 6 + [23],            # 37 rows: the last wave's second half idle
    "unequal_pairs": [32, 17] * 20 + [16, 1] * 20 + [9, 8] * 7,     # (the order is longest first: mixed lengths meet in a wave)
    "mix": list(np.random.default_rng(7).integers(0, 40, size=301)) + EDGES,
}


def _rows_of_lengths(lengths, n_item, k, seed, scale=0.1, low_conf=False):
    """a CSC (columns = the rows to solve) whose column j has lengths[j] distinct random items"""
    rng = np.random.default_rng(seed)
    p = np.zeros(len(lengths) + 1, dtype=np.int32)
    p[1:] = np.cumsum(lengths)
    idx = np.concatenate([np.sort(rng.choice(n_item, size=int(n), replace=False)) for n in lengths]).astype(np.int32)
    if low_conf:   # confidences in (0, 1) beside confidences above 1
        x = np.where(rng.random(idx.size) < 0.5, rng.uniform(0.05, 0.95, size=idx.size), 1.0 + rng.gamma(1.0, 2.0, size=idx.size))
    else:
        x = 1.0 + rng.gamma(1.0, 2.0, size=idx.size)
    x = x.astype(np.float32).astype(np.float64)
    X = np.asfortranarray((rng.standard_normal((k, n_item)) * scale).astype(np.float32))
    Y0 = np.asfortranarray((rng.standard_normal((k, len(lengths))) * scale).astype(np.float32))
    return (n_item, len(lengths), p, idx, x), X, Y0


def _check(csc, X, Y0, lens, lam=0.1):
    _, _, p, i, x = csc
    X64 = np.asfortranarray(X, dtype=np.float64)
    Yref = np.asfortranarray(Y0, dtype=np.float64).copy(order="F")
    lref = O.als_implicit(p, i, x, X64, Yref, O.gramian(X64, lam), lam, 1, 3)
    Y = Y0.copy(order="F")
    loss = als.als_implicit(csc, X, Y, lam, 1, 1, 3, "float", False, False)
    assert rel_fro(Y, Yref) < TOL
    assert abs(loss - lref) <= TOL * abs(lref), (loss, lref)
    err = np.linalg.norm(Y - Yref, axis=0) / np.maximum(np.linalg.norm(Yref, axis=0), 1e-30)
    err[np.linalg.norm(Yref, axis=0) == 0] = np.abs(Y[:, np.linalg.norm(Yref, axis=0) == 0]).max(initial=0.0)
    assert err.max() < ROW_TOL, (int(err.argmax()), int(lens[err.argmax()]), float(err.max()))


@pytest.mark.parametrize("low_conf", [False, True])
@pytest.mark.parametrize("case", sorted(LENGTHS))
def test_short_rows_two_per_wave_match_the_oracle_per_row(case, low_conf):
    lens = np.asarray(LENGTHS[case], dtype=np.int64)
    csc, X, Y0 = _rows_of_lengths(lens, 1500, 128, seed=11 + len(case) + 5 * low_conf, low_conf=low_conf)
    _check(csc, X, Y0, lens)


def test_early_convergence_beside_a_row_that_does_not():
    """every other row starts at its converged solution (the first CG step ends it: |r|^2 < 1e-10), its partner does not"""
    lens = np.asarray(([17, 32, 24, 20] * 10) + ([3, 16, 9, 12] * 10), dtype=np.int64)
    k, lam = 128, 0.1
    csc, X, Y0 = _rows_of_lengths(lens, 1500, k, seed=29)
    _, _, p, i, x = csc
    X64 = np.asfortranarray(X, dtype=np.float64)
    Ysol = np.asfortranarray(Y0, dtype=np.float64).copy(order="F")
    O.als_implicit(p, i, x, X64, Ysol, O.gramian(X64, lam), lam, 1, 60)
    Y0 = Y0.copy(order="F")
    Y0[:, ::2] = Ysol[:, ::2].astype(np.float32)
    _check(csc, X, Y0, lens, lam)


def _short_matrix(n_user, n_item, seed):
    """users of 0..40 non-zeros: every shard of the user half holds rows of both launches of the bucket"""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 41, size=n_user)
    rows = np.repeat(np.arange(n_user), deg)
    cols = np.concatenate([rng.choice(n_item, size=int(d), replace=False) for d in deg])
    vals = 1.0 + rng.geometric(0.5, size=rows.size).astype(np.float64)
    return sp.csr_matrix((vals, (rows, cols)), shape=(n_user, n_item))


def _fit(ctx, x, U0, V0, n_sub=(0, 0), n_iter=2, lam=0.1):
    ctx.set_matrix(x, n_sub=n_sub)
    ctx.set_factors(U0, V0)
    losses = []
    for _ in range(n_iter):
        li = ctx.half_iteration("items", "implicit", lam, "conjugate_gradient")
        lu = ctx.half_iteration("users", "implicit", lam, "conjugate_gradient")
        losses.append((li, lu))
    U, V = ctx.get_factors()
    return U, V, np.asarray(losses)


def _oracle_fit(x, U0, V0, n_iter=2, lam=0.1):
    c = sp.csc_matrix(x); c.sort_indices()
    ct = sp.csc_matrix(c.T); ct.sort_indices()
    Ur, Vr = np.array(U0.T, dtype=np.float64, order="F", copy=True), np.array(V0.T, dtype=np.float64, order="F", copy=True)
    for _ in range(n_iter):
        O.als_implicit(c.indptr, c.indices, c.data, Ur, Vr, O.gramian(Ur, lam), lam, 1, 3, n_threads=8)
        O.als_implicit(ct.indptr, ct.indices, ct.data, Vr, Ur, O.gramian(Vr, lam), lam, 1, 3, n_threads=8)
    return Ur.T, Vr.T


def _fro(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def test_sharded_context_cuts_through_the_bucket():
    from rsparse_amd.ctx import MultiGpuALS
    n_user, n_item, k = 901, 4000, 128
    x = _short_matrix(n_user, n_item, seed=23)
    lens = np.diff(x.indptr)
    assert (lens <= 16).sum() > 200 and ((lens > 16) & (lens <= 32)).sum() > 200
    rng = np.random.default_rng(3)
    U0 = (rng.standard_normal((n_user, k)) * 0.01).astype(np.float32)
    V0 = np.zeros((n_item, k), np.float32)
    Uo, Vo = _oracle_fit(x, U0, V0)
    one = MultiGpuALS(1, comm="shared")
    U1, V1, L1 = _fit(one, x, U0, V0)
    one.close()
    assert max(_fro(U1, Uo), _fro(V1, Vo)) < TOL
    for n_ranks, n_sub in ((2, (0, 0)), (4, (3, 2))):
        ctx = MultiGpuALS(n_ranks, comm="shared")
        U, V, L = _fit(ctx, x, U0, V0, n_sub=n_sub)
        ctx.close()
        assert max(_fro(U, Uo), _fro(V, Vo)) < TOL, (n_ranks, _fro(U, Uo), _fro(V, Vo))
        assert np.allclose(L, L1, rtol=2e-4, atol=0), (n_ranks, L, L1)
