"""BPR without a device: the numpy definition of rsparse_amd/bpr.py against what it claims to be -- the triple stream, the step
structure, a plain per-triple loop of the same definition, the stated exponential --, the class on the CPU stand-in backend,
the quality on the MovieLens fixture, the refusals of the C ABI before any device work, and the ABI table."""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from rsparse_amd import BPR, _lib
from rsparse_amd import rng as prng
from rsparse_amd.bpr import (CHUNK, bpr_exp, bpr_fit_reference, bpr_step_reference, bpr_triples, n_steps_of, step_slots)
from test_ease_host import brute_lists, ndcg10, protocol
from test_metrics_abi import _oracle_metrics_backend

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("rsparse_hip_bpr_triples_device", "rsparse_hip_bpr_step_device", "rsparse_hip_bpr_step_f64_device",
         "rsparse_hip_bpr_epochs_device", "rsparse_hip_bpr_epochs_f64_device", "rsparse_hip_bpr_fit")


def pattern(n_users, n_items, density, seed):
    return sp.csr_matrix((np.random.default_rng(seed).random((n_users, n_items)) < density).astype(np.float64))


def all_steps(seed, mode, epoch, row0, m, n_steps):
    return [bpr_triples(seed, mode, epoch, row0, m.indptr, m.indices, m.shape[1], s, n_steps) for s in range(n_steps)]


# ---- the triple stream ---------------------------------------------------------------------------------------------------------------
def test_triples_do_not_depend_on_the_rows_sampled_together():
    m = pattern(30, 20, 0.3, 1)
    u, i, j = bpr_triples(9, 0, 4, 100, m.indptr, m.indices, 20)
    assert u.dtype == i.dtype == j.dtype == np.int32 and u.size == m.nnz
    for a, b in ((0, 7), (7, 8), (8, 30)):
        part = m[a:b]
        pu, pi, pj = bpr_triples(9, 0, 4, 100 + a, part.indptr, part.indices, 20)
        sel = (u >= a) & (u < b)
        assert np.array_equal(pu + a, u[sel]) and np.array_equal(pi, i[sel]) and np.array_equal(pj, j[sel])
    # the fold-in stream: a row's triples do not depend on where it stands
    fu, fi, fj = bpr_triples(9, 1, 4, 0, m.indptr, m.indices, 20)
    part = m[11:19]
    pu, pi, pj = bpr_triples(9, 1, 4, 0, part.indptr, part.indices, 20)
    sel = (fu >= 11) & (fu < 19)
    assert np.array_equal(pi, fi[sel]) and np.array_equal(pj, fj[sel])
    assert not np.array_equal(fi, i) or not np.array_equal(fj, j)            # (another stream than the fit's)
    # every positive is in its row, no valid negative is
    d = m.toarray() > 0
    assert d[u, i].all() and not d[u[j >= 0], j[j >= 0]].any()


def test_rows_of_0_1_all_but_one_and_all_items():
    n_items = 9
    d = np.zeros((4, n_items), dtype=bool)
    d[1, 4] = True
    d[2] = True
    d[2, 6] = False
    d[3] = True
    m = sp.csr_matrix(d.astype(np.float64))
    seen_neg = set()
    for epoch in range(60):
        u, i, j = bpr_triples(5, 0, epoch, 0, m.indptr, m.indices, n_items)
        assert u.tolist() == [1] + [2] * 8 + [3] * 9                         # (the empty row has no slot)
        assert i[0] == 4 and j[0] != 4                                       # (one candidate of three outside {4}: never void here)
        assert (j[u == 3] == -1).all()                                       # every item is in the row: always void
        assert set(j[u == 2].tolist()) <= {6, -1}                            # the single admissible negative, or void
        seen_neg |= set(j[u == 2].tolist())
    assert seen_neg == {6, -1}


def test_positives_and_negatives_are_uniform():
    n_items, row = 50, np.arange(3, 50, 5)                                   # a row of 10 items
    m = sp.csr_matrix((np.ones(row.size), row, [0, 0, row.size]), shape=(2, n_items))
    pos, neg = np.zeros(n_items), np.zeros(n_items)
    for epoch in range(400):
        _, i, j = bpr_triples(77, 0, epoch, 0, m.indptr, m.indices, n_items)
        pos += np.bincount(i, minlength=n_items)
        neg += np.bincount(j[j >= 0], minlength=n_items)
    n = 400 * row.size
    assert pos.sum() == n and (pos[np.setdiff1d(np.arange(n_items), row)] == 0).all() and (neg[row] == 0).all()
    assert (np.abs(pos[row] - n / 10) <= 4 * math.sqrt(n * 0.1 * 0.9)).all()
    out, nv = np.setdiff1d(np.arange(n_items), row), neg.sum()
    assert nv >= n * (1 - 0.2 ** 3) - 4 * math.sqrt(n * 0.008)               # void with probability (10 / 50)^3
    assert (np.abs(neg[out] - nv / 40) <= 4 * math.sqrt(nv * (1 / 40) * (39 / 40))).all()


def scalar_philox(counter, key):
    """Philox4x32-10 written out on Python integers (Random123's philox.h), sharing nothing with rsparse_amd/rng.py"""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def test_triples_worked_out_by_a_scalar_loop():
    """the counter layout (q, g, 6, epoch + 2^31 mode), the key halves and the word roles, from the issue's text alone"""
    assert scalar_philox((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)   # Random123's known answer
    m = pattern(9, 7, 0.5, 4)
    seed, epoch, row0, n_items = (0xABCDEF01 << 32) | 0x12345678, 5, 2 ** 31 + 3, 7
    for mode in (0, 1):
        expect = []
        for u in range(9):
            row = m.indices[m.indptr[u]:m.indptr[u + 1]].tolist()
            for q in range(len(row)):
                g = row0 + u if mode == 0 else row0
                o = scalar_philox((q, g, 6, epoch + (mode << 31)), (seed & 0xFFFFFFFF, seed >> 32))
                neg = -1
                for w in o[1:]:
                    cand = (w * n_items) >> 32
                    if cand not in row:
                        neg = cand
                        break
                expect.append((u, row[(o[0] * len(row)) >> 32], neg))
        got = bpr_triples(seed, mode, epoch, row0, m.indptr, m.indices, n_items)
        assert [tuple(int(v) for v in t) for t in zip(*got)] == expect


# ---- the step structure --------------------------------------------------------------------------------------------------------------
def test_every_slot_is_in_exactly_one_step_and_a_users_k_are_consecutive():
    m = pattern(25, 30, 0.35, 2)
    nnz, n_steps = m.nnz, 7
    assert nnz % n_steps != 0 and n_steps_of(nnz, -(-nnz // n_steps)) == n_steps and n_steps_of(0, 5) == 1
    slots = [step_slots(nnz, s, n_steps) for s in range(n_steps)]
    assert np.array_equal(np.sort(np.concatenate(slots)), np.arange(nnz))
    whole = bpr_triples(3, 0, 2, 0, m.indptr, m.indices, 30)
    for s, t in enumerate(all_steps(3, 0, 2, 0, m, n_steps)):
        assert all(np.array_equal(a[slots[s]], b) for a, b in zip(whole, t))   # a triple belongs to its slot, not to the step
        u = t[0]
        assert (np.diff(u) >= 0).all()                                       # ascending, hence every user's k are consecutive


# ---- the definition against a plain loop ---------------------------------------------------------------------------------------------
LOG2E, LN2_HI, LN2_LO = 1.4426950408889634, 6.93147180369123816490e-01, 1.90821492927058770002e-10


def plain_exp(d):
    d = min(max(d, -40.0), 40.0)
    kk = float(np.rint(d * LOG2E))
    r = (d - kk * LN2_HI) - kk * LN2_LO
    p = 1.0 / math.factorial(13)
    for n in range(12, -1, -1):
        p = p * r + 1.0 / math.factorial(n)
    return math.ldexp(p, int(kk))


def plain_dot(a, b):
    v = [0.0] * 16
    for c in range(len(a)):
        v[c % 16] = v[c % 16] + a[c] * b[c]
    for half in (8, 4, 2):
        v = [v[l] + v[l + half] for l in range(half)]
    return v[0] + v[1]


def plain_step(U, V, aU, aV, tu, ti, tj, lr, lam, update_items):
    """the definition, one triple and one coordinate at a time, in Python floats (every operation a rounded double operation)"""
    rank = U.shape[1]
    wide = lambda M: [[float(x) for x in row] for row in M]
    Uw, Vw = wide(U), wide(V)
    to_u, to_v = {}, {}
    n_valid = n_correct = 0
    for u, i, j in zip(tu.tolist(), ti.tolist(), tj.tolist()):
        if j < 0:
            continue
        diff = [Vw[i][c] - Vw[j][c] for c in range(rank)]
        d = plain_dot(Uw[u], diff)
        z = 1.0 / (1.0 + plain_exp(d))
        n_valid, n_correct = n_valid + 1, n_correct + (d > 0)
        to_u.setdefault(u, []).append([z * diff[c] for c in range(rank)])
        to_v.setdefault(i, []).append([z * Uw[u][c] for c in range(rank)])
        to_v.setdefault(j, []).append([(-z) * Uw[u][c] for c in range(rank)])

    def apply(M, Mw, a, contribs):
        M2, a2 = M.copy(), a.copy()
        for dest, rows in contribs.items():
            total = [0.0] * rank
            for c0 in range(0, len(rows), CHUNK):
                acc = [0.0] * rank
                for row in rows[c0:c0 + CHUNK]:
                    acc = [acc[c] + row[c] for c in range(rank)]
                total = [total[c] + acc[c] for c in range(rank)]
            lc = lam * float(len(rows))
            g = [total[c] - lc * Mw[dest][c] for c in range(rank)]
            an = float(a[dest]) + plain_dot(g, g) / float(rank)
            a2[dest] = an
            if an != 0:
                root = math.sqrt(an)
                M2[dest] = np.array([Mw[dest][c] + (lr * g[c]) / root for c in range(rank)]).astype(M.dtype)
        return M2, a2

    U2, aU2 = apply(U, Uw, aU, to_u)
    V2, aV2 = apply(V, Vw, aV, to_v) if update_items else (V.copy(), aV.copy())
    return U2, V2, aU2, aV2, n_valid, n_correct


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("rank", [3, 16, 21])
@pytest.mark.parametrize("copies", [1, 32])
def test_step_reference_is_the_plain_loop(copies, rank, dtype):
    """a 12 x 9 matrix, and 32 copies of it below each other so that every item's list passes several chunks"""
    rng = np.random.default_rng(rank)
    d = rng.random((12, 9)) < 0.5
    d[:, 0] = True
    d[5] = True                                                              # a row whose triples are all void
    d = np.tile(d, (copies, 1))
    n_users = d.shape[0]
    m = sp.csr_matrix(d.astype(np.float64))
    U, V = ((0.5 * rng.standard_normal((n, rank))).astype(dtype) for n in (n_users, 9))
    aU, aV = rng.random(n_users) * 0.1, rng.random(9) * 0.1
    aU[3] = 0.0
    for update_items in (True, False):
        t = bpr_triples(11, 0, 1, 0, m.indptr, m.indices, 9, copies > 1, 1 + (copies > 1))
        if copies > 1:
            assert np.bincount(np.concatenate([t[1][t[2] >= 0], t[2][t[2] >= 0]]), minlength=9).max() > 2 * CHUNK
        ref = bpr_step_reference(U, V, aU, aV, *t, 0.1, 0.02, update_items)
        plain = plain_step(U, V, aU, aV, *t, 0.1, 0.02, update_items)
        assert all(bits_equal(a, b) for a, b in zip(ref[:4], plain[:4])) and ref[4:] == plain[4:]
        assert ref[4] < t[0].size and 0 < ref[5] < ref[4]
        if not update_items:
            assert bits_equal(ref[1], V) and bits_equal(ref[3], aV)
        void_rows = np.flatnonzero(d.all(axis=1))
        assert void_rows.size and bits_equal(ref[0][void_rows], U[void_rows]) and bits_equal(ref[2][void_rows], aU[void_rows])


def test_the_stated_exponential():
    x = np.concatenate([np.linspace(-40, 40, 200001), [-1e3, -40.0, 0.0, -0.0, 40.0, 1e3, 1e-300, 0.5 * math.log(2)]])
    got, ref = bpr_exp(x), np.exp(np.clip(x, -40, 40))
    ulp = np.abs(got - ref) / np.spacing(ref)
    print("E against np.exp: at most %.2f ulp" % ulp.max())
    assert ulp.max() <= 2.0 and bpr_exp(0.0) == 1.0
    assert all(bpr_exp(v) == plain_exp(float(v)) for v in x[::997])
    z = 1.0 / (1.0 + got)
    assert np.isfinite(z).all() and (z > 0).all() and (z <= 1).all()


# ---- the class on the CPU stand-in -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model():
    x = pattern(40, 30, 0.25, 11)
    x = sp.vstack([sp.csr_matrix((1, 30)), x[1:]]).tocsr()                   # an empty row
    m = BPR(rank=5, learning_rate=0.1, lambda_=0.01, batch=64, transform_iter=7, precision="double", rng=3,
            backend=_oracle_metrics_backend())
    return x, m, m.fit_transform(x, 4)


def test_class_fit_is_the_definition(small_model):
    x, m, U = small_model
    assert U.shape == (40, 5) and U.dtype == np.float64 and m.components.shape == (5, 30) and m.components.dtype == np.float64
    U0, V0 = (prng.init_factors(m.seed, s, 0, n, 5, 0.01) for s, n in ((0, 40), (1, 30)))
    ref = bpr_fit_reference(x.indptr, x.indices, 30, U0, V0, 4, m.seed, 0.1, 0.01, 64)
    assert bits_equal(U, ref[0]) and bits_equal(m.components.T, ref[1])
    assert bits_equal(m.user_adagrad, ref[2]) and bits_equal(m.item_adagrad, ref[3])
    assert m.trace == ref[4] and len(m.trace) == 4
    assert all(isinstance(v, int) and 0 < c < v <= x.nnz for v, c in m.trace)
    f = BPR(rank=5, batch=64, rng=3, backend=_oracle_metrics_backend())
    Uf = f.fit_transform(x, 1)
    assert Uf.dtype == np.float32 and f.components.dtype == np.float32 and f.item_adagrad.dtype == np.float64


def test_class_fold_in_and_surface(small_model):
    x, m, _ = small_model
    V = m.components.T.copy()
    emb = m.transform(x)
    ref = bpr_fit_reference(x.indptr, x.indices, 30, np.zeros((40, 5)), V, 7, m.seed, 0.1, 0.01, 64, mode=1, update_items=False,
                            aV=m.item_adagrad)
    assert bits_equal(emb, ref[0]) and (emb[0] == 0).all() and bits_equal(m.components.T, V)
    assert bits_equal(m.transform(x[9:23]), emb[9:23])
    top = m.predict(x, 5)
    part = m.predict(x[9:23], 5)
    assert np.array_equal(np.asarray(part), np.asarray(top)[9:23]) and np.array_equal(part.scores, top.scores[9:23])
    lists, _ = brute_lists(emb @ V.T, 5, x, ())
    assert np.array_equal(np.asarray(top)[1:], lists[1:])                    # (row 0 is all ties: the stand-in has its own rule)
    held = sp.csr_matrix((np.random.default_rng(4).random(x.shape) < 0.2) * (1 - x.toarray()) * 2.0)
    ev = m.evaluate(x, held, (3, 5), metrics=("ndcg", "hit"), negatives=20, seed=7)
    assert ev["ndcg"].shape == (40, 2)
    pairs = sp.csr_matrix(np.random.default_rng(6).random(x.shape) < 0.1)
    sc = m.score(x, pairs)
    rows = np.repeat(np.arange(40), np.diff(sc.indptr))
    assert np.allclose(sc.data, (emb @ V.T)[rows, sc.indices], rtol=1e-12, atol=1e-15)
    with pytest.raises(_lib.UnsupportedOnDevice):
        m.explain(x, pairs)


def test_zero_rates_leave_the_initial_factors():
    x = pattern(20, 15, 0.3, 8)
    m = BPR(rank=4, learning_rate=0.0, lambda_=0.0, batch=16, precision="double", rng=5, backend=_oracle_metrics_backend())
    U = m.fit_transform(x, 2)
    assert np.array_equal(U, prng.init_factors(m.seed, 0, 0, 20, 4, 0.01))
    assert np.array_equal(m.components.T, prng.init_factors(m.seed, 1, 0, 15, 4, 0.01))
    assert (m.item_adagrad[np.bincount(x.indices, minlength=15) > 0] > 0).all()   # (the state still moves)


def test_argument_errors():
    for kw in ({"rank": 0}, {"rank": 2.5}, {"rank": True}, {"batch": 0}, {"transform_iter": 0}, {"learning_rate": -0.1},
               {"learning_rate": np.nan}, {"lambda_": -1.0}, {"lambda_": np.inf}, {"precision": "half"}):
        with pytest.raises(ValueError):
            BPR(**kw)
    for kw in ({"rank": _lib.MAX_RANK + 1}, {"rank": _lib.MAX_RANK_F64 + 1, "precision": "double"}):
        with pytest.raises(_lib.UnsupportedOnDevice):
            BPR(**kw)
    m = BPR(backend=_oracle_metrics_backend())
    x = sp.csr_matrix(np.eye(4))
    with pytest.raises(RuntimeError):
        m.predict(x, 2)
    with pytest.raises(RuntimeError):
        m.transform(x)
    with pytest.raises(ValueError):
        m.fit_transform(x, -1)
    with pytest.raises(TypeError):
        m.fit_transform(np.eye(4), 1)
    m.fit_transform(x, 1)
    with pytest.raises(ValueError):
        m.transform(sp.csr_matrix(np.eye(5)))
    with pytest.raises(ValueError):
        bpr_triples(1, 2, 0, 0, x.indptr, x.indices, 4)
    with pytest.raises(ValueError):
        bpr_triples(1, 0, 0, 0, x.indptr, x.indices, 4, 3, 3)


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def test_void_share_on_the_fixture():
    """a condition on the input: a triple is void with probability (L / n_items)^3"""
    train, _, _ = protocol()
    L = np.diff(train.indptr).astype(np.float64)
    expected = float((L * (L / train.shape[1]) ** 3).sum() / L.sum())
    _, _, j = bpr_triples(1, 0, 0, 0, train.indptr, train.indices, train.shape[1])
    print("void triples: %.2f %% (expected %.2f %%)" % (100 * (j < 0).mean(), 100 * expected))
    assert abs(expected - 0.0050) < 0.0005 and (j < 0).mean() < 0.02


def test_class_beats_popularity_on_the_fixture():
    train, hist, held = protocol()
    m = BPR(rank=16, learning_rate=0.1, lambda_=0.01, batch=4096, transform_iter=50, precision="double", rng=1,
            backend=_oracle_metrics_backend())
    m.fit_transform(train, 20)
    top = m.predict(hist, 10)
    pop_lists, _ = brute_lists(np.broadcast_to(np.asarray(train.sum(axis=0)).ravel().astype(np.float64), hist.shape), 10, hist, ())
    bpr, popularity = ndcg10(np.asarray(top), held), ndcg10(pop_lists, held)
    print("NDCG@10: BPR %.3f, popularity %.3f, ratio %.2f; AUC estimate of the last epoch %.3f"
          % (bpr, popularity, bpr / popularity, m.trace[-1][1] / m.trace[-1][0]))
    assert bpr >= 1.3 * popularity


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------
def test_library_exports_the_bpr_entry_points():
    lib = _lib.load()
    text = (ROOT / "include" / "rsparse_wrmf_hip.h").read_text()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert lib.rsparse_hip_abi_version() == 6                                # additive entries: the version stays
    assert int(re.search(r"#define RSPARSE_HIP_BPR_CHUNK (\d+)", text).group(1)) == _lib.BPR_CHUNK == CHUNK
    assert prng.STREAM_BPR == 6
    from rsparse_amd.engine import HipBackend
    assert callable(HipBackend.bpr_triples) and callable(HipBackend.bpr_step) and callable(HipBackend.bpr_epochs)
    import rsparse_amd
    assert rsparse_amd.BPR is BPR and rsparse_amd.bpr_step_reference is bpr_step_reference


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _answer(rc, code, text):
    assert rc == code, (rc, _lib.load().rsparse_hip_last_error())
    assert text in _lib.load().rsparse_hip_last_error().decode(), _lib.load().rsparse_hip_last_error()


# 3 users x 4 items: rows {0, 2}, {1}, {0, 1, 3}
P = np.array([0, 2, 3, 6], dtype=np.int32)
J = np.array([0, 2, 1, 0, 1, 3], dtype=np.int32)


def test_bpr_device_entries_status_codes():
    # (host pointers: every call here is rejected by the argument checks, or has no row, before device work)
    lib = _lib.load()
    out = [np.zeros(6, np.int32) for _ in range(3)]

    def triples(p=P, j=J, n_rows=3, n_items=4, nnz=6, row0=0, mode=0, epoch=0, step=0, n_steps=1, u=out[0], i=out[1], neg=out[2]):
        return lib.rsparse_hip_bpr_triples_device(_vp(p), _vp(j), n_rows, n_items, nnz, row0, 5, mode, epoch, step, n_steps, _vp(u),
                                                  _vp(i), _vp(neg), None)

    for missing in ("p", "j", "u", "i", "neg"):
        _answer(triples(**{missing: None}), _lib.ERR_INVALID, "NULL")
    for kw in ({"n_rows": -1}, {"n_items": -1}, {"nnz": -1}, {"nnz": 2 ** 31}):
        _answer(triples(**kw), _lib.ERR_INVALID, "bad dimensions")
    _answer(triples(row0=-1), _lib.ERR_INVALID, "32 bits")
    _answer(triples(row0=2 ** 32 - 2), _lib.ERR_INVALID, "32 bits")
    _answer(triples(mode=2), _lib.ERR_INVALID, "mode")
    _answer(triples(epoch=-1), _lib.ERR_INVALID, "epoch")
    _answer(triples(n_steps=0), _lib.ERR_INVALID, "n_steps < 1")
    _answer(triples(step=1), _lib.ERR_INVALID, "step outside")
    _answer(triples(step=-1, n_steps=2), _lib.ERR_INVALID, "step outside")
    _answer(triples(n_rows=0, nnz=0), _lib.OK, "")

    for f64 in (False, True):
        dt = np.float64 if f64 else np.float32
        U, V, aU, aV, cnt = np.zeros((3, 2), dt), np.zeros((4, 2), dt), np.zeros(3), np.zeros(4), np.zeros(8, np.int64)
        top = _lib.MAX_RANK_F64 if f64 else _lib.MAX_RANK

        def step(p=P, j=J, n_rows=3, n_items=4, nnz=6, step=0, n_steps=1, rank=2, lr=0.1, lam=0.01, U=U, V=V, aU=aU, aV=aV, cnt=cnt):
            fn = lib.rsparse_hip_bpr_step_f64_device if f64 else lib.rsparse_hip_bpr_step_device
            return fn(_vp(p), _vp(j), n_rows, n_items, nnz, 0, 5, 0, 0, step, n_steps, rank, lr, lam, 1, _vp(U), _vp(V), _vp(aU), _vp(aV),
                      _vp(cnt), None)

        def epochs(p=P, j=J, n_rows=3, n_items=4, nnz=6, n_epochs=2, batch=4, rank=2, lr=0.1, lam=0.01, U=U, V=V, aU=aU, aV=aV, cnt=cnt):
            fn = lib.rsparse_hip_bpr_epochs_f64_device if f64 else lib.rsparse_hip_bpr_epochs_device
            return fn(_vp(p), _vp(j), n_rows, n_items, nnz, 0, 5, 0, 0, n_epochs, batch, rank, lr, lam, 1, _vp(U), _vp(V), _vp(aU),
                      _vp(aV), _vp(cnt), None)

        for call in (step, epochs):
            for missing in ("p", "j", "U", "V", "aU", "aV", "cnt"):
                _answer(call(**{missing: None}), _lib.ERR_INVALID, "NULL")
            for kw in ({"n_rows": -1}, {"n_items": -1}, {"nnz": -1}):
                _answer(call(**kw), _lib.ERR_INVALID, "bad dimensions")
            _answer(call(rank=0), _lib.ERR_INVALID, "rank < 1")
            for bad in (-0.5, float("nan"), float("inf")):
                _answer(call(lr=bad), _lib.ERR_INVALID, "learning_rate or lambda")
                _answer(call(lam=bad), _lib.ERR_INVALID, "learning_rate or lambda")
            _answer(call(rank=top + 1), _lib.ERR_UNSUPPORTED, "rank > %d" % top)
            assert call(rank=top + 1, U=None) == _lib.ERR_INVALID               # the pointers are looked at first
            _answer(call(n_rows=0, nnz=0), _lib.OK, "")
        _answer(step(n_steps=0), _lib.ERR_INVALID, "n_steps < 1")
        _answer(step(step=2, n_steps=2), _lib.ERR_INVALID, "step outside")
        _answer(epochs(batch=0), _lib.ERR_INVALID, "batch < 1")
        _answer(epochs(nnz=2 ** 30, batch=2 ** 30), _lib.ERR_UNSUPPORTED, "2^30 or more triples")
        _answer(step(nnz=2 ** 30), _lib.ERR_UNSUPPORTED, "2^30 or more triples")
        _answer(step(nnz=2 ** 30, n_rows=0), _lib.ERR_UNSUPPORTED, "2^30 or more triples")
        _answer(epochs(n_epochs=-1), _lib.ERR_INVALID, "epoch")
        _answer(epochs(n_epochs=0), _lib.OK, "")


def test_bpr_fit_checks_its_arrays_first():
    lib = _lib.load()
    U, V, aU, aV, cnt = np.zeros((3, 2)), np.zeros((4, 2)), np.zeros(3), np.zeros(4), np.zeros(4, np.int64)

    def fit(p=P, j=J, n_users=3, n_items=4, n_epochs=2, batch=4, rank=2, lr=0.1, lam=0.01, U=U, V=V, aU=aU, aV=aV, cnt=cnt):
        return lib.rsparse_hip_bpr_fit(_vp(p), _vp(j), n_users, n_items, 5, n_epochs, batch, rank, lr, lam, _vp(U), _vp(V), _vp(aU),
                                       _vp(aV), _vp(cnt))

    for missing in ("p", "U", "V", "aU", "aV", "cnt"):
        _answer(fit(**{missing: None}), _lib.ERR_INVALID, "NULL")
    _answer(fit(j=None), _lib.ERR_INVALID, "j is NULL")
    _answer(fit(n_users=-1), _lib.ERR_INVALID, "bad dimensions")
    _answer(fit(n_items=-1), _lib.ERR_INVALID, "bad dimensions")
    _answer(fit(n_epochs=-1), _lib.ERR_INVALID, "epoch")
    _answer(fit(batch=0), _lib.ERR_INVALID, "batch < 1")
    _answer(fit(rank=0), _lib.ERR_INVALID, "rank < 1")
    _answer(fit(lr=-1.0), _lib.ERR_INVALID, "learning_rate or lambda")
    _answer(fit(lam=float("nan")), _lib.ERR_INVALID, "learning_rate or lambda")
    _answer(fit(rank=_lib.MAX_RANK_F64 + 1), _lib.ERR_UNSUPPORTED, "rank > 128")
    _answer(fit(p=np.array([1, 2, 3, 6], np.int32)), _lib.ERR_INVALID, "p[0] != 0")
    _answer(fit(p=np.array([0, 3, 2, 6], np.int32)), _lib.ERR_INVALID, "p decreases")
    _answer(fit(j=np.array([0, 4, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "a column outside [0, n_items)")
    _answer(fit(j=np.array([2, 0, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "not strictly ascending")
    cnt[:] = 9
    _answer(fit(p=np.zeros(1, np.int32), n_users=0), _lib.OK, "")            # no user: nothing to fit, and no device
    assert (cnt == 0).all()
