"""Bucket 1 of the quad-layout CG kernels (rows of 257..512 non-zeros) at rank 97..128 runs in two launches: the rows of more
than 320 non-zeros on 8-wave teams, the rows of 257..320 on 4-wave teams of 20 quads per wave (wrmf_cgq.hip, the split is
QSchedule::team4_first).  Checked per row against the fp64 oracle at the parity tolerances of tests/test_hip_parity.py: rows at
the bucket's edges and at the split (255..258, 319..322, 511..513 non-zeros), a bucket 1 of short rows only, of long rows only and
a mix, implicit and explicit feedback, the padded rank (128) and a rank below it (124), and a two- and four-rank context whose
shards cut through the split."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import rel_fro
from oracle import wrmf_oracle as O
from rsparse_amd import als

pytestmark = pytest.mark.gpu
TOL = 1e-4
ROW_TOL = 5e-4   # per row, as tests/test_hip_parity.py::test_cg_long_rows_all_buckets

EDGES = [255, 256, 257, 258, 319, 320, 321, 322, 511, 512, 513]
LENGTHS = {
    "edges": EDGES + [1, 40, 130, 700],
    "short_only": [257, 258, 280, 300, 319, 320] * 5 + [3, 64, 200],
    "long_only": [321, 322, 380, 450, 511, 512] * 5 + [3, 64, 200],
    "mix": list(np.random.default_rng(5).integers(240, 530, size=97)) + EDGES,
}


def _rows_of_lengths(lengths, n_item, k, seed, scale=0.1):
    """a CSC (columns = the rows to solve) whose column j has lengths[j] distinct random items, values >= 1"""
    rng = np.random.default_rng(seed)
    p = np.zeros(len(lengths) + 1, dtype=np.int32)
    p[1:] = np.cumsum(lengths)
    idx = np.concatenate([np.sort(rng.choice(n_item, size=int(n), replace=False)) for n in lengths]).astype(np.int32)
    x = (1.0 + rng.gamma(1.0, 2.0, size=idx.size)).astype(np.float32).astype(np.float64)
    X = np.asfortranarray((rng.standard_normal((k, n_item)) * scale).astype(np.float32))
    Y0 = np.asfortranarray((rng.standard_normal((k, len(lengths))) * scale).astype(np.float32))
    return (n_item, len(lengths), p, idx, x), X, Y0


@pytest.mark.parametrize("k", [128, 124])
@pytest.mark.parametrize("implicit", [True, False])
@pytest.mark.parametrize("case", sorted(LENGTHS))
def test_bucket1_split_matches_the_oracle_per_row(k, implicit, case):
    lens = np.asarray(LENGTHS[case], dtype=np.int64)
    n_item = 1500
    csc, X, Y0 = _rows_of_lengths(lens, n_item, k, seed=k + 3 * implicit + len(case))
    _, _, p, i, x = csc
    cnt = np.bincount(i, minlength=n_item).astype(np.float64)
    X64 = np.asfortranarray(X, dtype=np.float64)
    Yref = np.asfortranarray(Y0, dtype=np.float64).copy(order="F")
    if implicit:
        lref = O.als_implicit(p, i, x, X64, Yref, O.gramian(X64, 0.1), 0.1, 1, 3)
    else:
        lref = O.als_explicit(p, i, x, X64, Yref, cnt, 0.1, 1, 3, True)
    Y = Y0.copy(order="F")
    if implicit:
        loss = als.als_implicit(csc, X, Y, 0.1, 1, 1, 3, "float", False, False)
    else:
        loss = als.als_explicit(csc, X, Y, cnt.astype(np.float32), 0.1, 1, 1, 3, True, "float", False, False)
    assert rel_fro(Y, Yref) < TOL
    assert abs(loss - lref) <= TOL * abs(lref), (loss, lref)
    err = np.linalg.norm(Y - Yref, axis=0) / np.maximum(np.linalg.norm(Yref, axis=0), 1e-30)
    assert err.max() < ROW_TOL, (int(err.argmax()), int(lens[err.argmax()]), float(err.max()))


def _split_matrix(n_user, n_item, seed):
    """users of 240..420 non-zeros: every shard of the user half holds rows on both sides of the split"""
    rng = np.random.default_rng(seed)
    deg = rng.integers(240, 421, size=n_user)
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


def test_sharded_context_cuts_through_the_split():
    from rsparse_amd.ctx import MultiGpuALS
    n_user, n_item, k = 600, 1200, 128
    x = _split_matrix(n_user, n_item, seed=17)
    lens = np.diff(x.indptr)
    assert (lens <= 320).sum() > 100 and (lens > 320).sum() > 100
    rng = np.random.default_rng(2)
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
