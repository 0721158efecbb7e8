"""Full-ranking metrics without a device: the numpy statement of the semantics (rsparse_amd.metrics.percentile_ranks /
rank_summary / rank_totals) on hand-made cases, the AUC identity against a brute-force pair count, `WRMF.held_out_ranks` /
`WRMF.evaluate_ranks` through the CPU stand-in backend on MovieLens -- equal to the numpy statement, and the same under
torch.distributed (gloo) at world sizes 1 and 2 --, and the argument errors."""
import os
import re
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import _lib
from rsparse_amd.metrics import canonical_actual, percentile_ranks, rank_summary, rank_totals

ROOT = Path(__file__).resolve().parent.parent


def _one_row(scores, held, weights=None, nr=(), excl=()):
    """one user: (above, tied, n_adm, summary) of the held-out items `held`"""
    S = np.asarray(scores, dtype=np.float64)[None, :]
    m = S.shape[1]
    w = np.ones(len(held)) if weights is None else np.asarray(weights, dtype=np.float64)
    act = sp.csr_matrix((w, (np.zeros(len(held), int), np.asarray(held, int))), shape=(1, m))
    not_rec = sp.csr_matrix((np.ones(len(nr)), (np.zeros(len(nr), int), np.asarray(nr, int))), shape=(1, m)) if len(nr) else None
    above, tied, n_adm = percentile_ranks(S, act, not_rec, excl)
    return above, tied, n_adm, rank_summary(above, tied, n_adm, act)


def test_the_batch_constant_of_the_header():
    text = (ROOT / "include" / "rsparse_wrmf_hip.h").read_text()
    assert int(re.search(r"#define RSPARSE_HIP_RANKS_BATCH (\d+)", text).group(1)) == _lib.RANKS_BATCH


def test_ties_take_the_midrank():
    #        item:  0    1    2    3    4    5
    scores = [3.0, 1.0, 2.0, 2.0, 2.0, 0.0]
    above, tied, n_adm, s = _one_row(scores, [2, 5])
    assert above.data.tolist() == [1, 5] and tied.data.tolist() == [2, 0] and n_adm.tolist() == [6]
    assert above.dtype == np.int32 and sp.isspmatrix_csr(above) and above.indices.tolist() == [2, 5]
    # r = 2 and 5: pct = 0.4 and 1
    assert s["mpr"][0] == pytest.approx((0.4 + 1.0) / 2, rel=1e-15)
    assert s["mrr"][0] == pytest.approx(1.0 / 3.0, rel=1e-15)
    # pairs (held-out, other): item 2 beats 1, ties 3 and 4, loses to 0 -> 1 + 2 / 2 of 4; item 5 beats none of 4 -> 2 / 8
    assert s["auc"][0] == pytest.approx(0.25, rel=1e-15)
    assert s["P"][0] == 2 and s["sum_w"][0] == 2.0
    # -0 and +0 are one score
    a2, t2, _, _ = _one_row([0.0, -0.0, 1.0], [0])
    assert a2.data.tolist() == [1] and t2.data.tolist() == [1]


def test_an_all_tied_row_is_in_the_middle():
    above, tied, n_adm, s = _one_row(np.zeros(9), [1, 4, 7], weights=[1.0, 2.0, 5.0])
    assert above.data.tolist() == [0, 0, 0] and tied.data.tolist() == [8, 8, 8]
    assert s["mpr"][0] == 0.5 and s["auc"][0] == 0.5 and s["mrr"][0] == 1.0 / 5.0


def test_rows_where_a_number_is_undefined():
    # P = 0: nothing held out
    above, tied, n_adm, s = _one_row([1.0, 2.0, 3.0], [])
    assert above.nnz == 0 and n_adm.tolist() == [3]
    assert np.isnan(s["mpr"][0]) and np.isnan(s["auc"][0]) and np.isnan(s["mrr"][0]) and s["P"][0] == 0 and s["sum_w"][0] == 0
    # n_adm = P: every admissible item is held out -> no pair to order; mpr and mrr stay defined
    above, tied, n_adm, s = _one_row([1.0, 2.0, 3.0], [0, 1, 2])
    assert above.data.tolist() == [2, 1, 0] and np.isnan(s["auc"][0])
    assert s["mpr"][0] == pytest.approx(0.5) and s["mrr"][0] == 1.0
    # n_adm = 1: no percentile
    above, tied, n_adm, s = _one_row([1.0, 2.0, 3.0], [1], nr=[0], excl=[2])
    assert above.data.tolist() == [0] and tied.data.tolist() == [0] and n_adm.tolist() == [1]
    assert np.isnan(s["mpr"][0]) and np.isnan(s["auc"][0]) and s["mrr"][0] == 1.0 and np.isnan(s["sum_w_pct"][0])
    # zero weights (stored zeros are entries): auc and mrr do not use them
    above, tied, n_adm, s = _one_row([1.0, 2.0, 3.0, 4.0], [1, 3], weights=[0.0, 0.0])
    assert above.data.tolist() == [2, 0] and s["P"][0] == 2
    assert np.isnan(s["mpr"][0]) and s["auc"][0] == pytest.approx(0.75) and s["mrr"][0] == 1.0


def test_an_inadmissible_entry_takes_no_part():
    scores = [5.0, 4.0, 3.0, 2.0, 1.0, 0.0]
    # item 0 is held out but not recommendable, item 3 held out but excluded; item 1 (also masked) is not held out
    above, tied, n_adm, s = _one_row(scores, [0, 2, 3, 4], weights=[9.0, 1.0, 9.0, 3.0], nr=[0, 1], excl=[3])
    assert above.data.tolist() == [-1, 0, -1, 1] and tied.data.tolist() == [-1, 0, -1, 0] and n_adm.tolist() == [3]
    assert s["P"][0] == 2 and s["sum_w"][0] == 4.0
    assert s["mpr"][0] == pytest.approx((1.0 * 0.0 + 3.0 * 0.5) / 4.0)
    assert s["auc"][0] == pytest.approx(1.0)      # the one other admissible item, 5, is below both
    # the same numbers as the row with the masked items cut out
    _, _, _, s2 = _one_row([3.0, 1.0, 0.0], [0, 1], weights=[1.0, 3.0])
    for k in s:
        assert s[k][0] == s2[k][0], k


def test_totals_skip_the_rows_without_a_defined_term():
    summ = {"sum_w": np.array([2.0, 1.0, 0.0, 4.0]), "sum_w_pct": np.array([0.5, np.nan, 0.0, 1.0]),
            "P": np.array([2.0, 1.0, 0.0, 3.0]), "auc": np.array([0.75, np.nan, np.nan, 0.25]),
            "mrr": np.array([1.0, 1.0, np.nan, 0.5])}
    t = rank_totals(summ)
    assert t == {"mpr": 1.5 / 6.0, "auc": 0.5, "mrr": 2.5 / 3.0, "n": 6}
    e = rank_totals({k: v[2:3] for k, v in summ.items()})
    assert np.isnan(e["mpr"]) and np.isnan(e["auc"]) and np.isnan(e["mrr"]) and e["n"] == 0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_auc_identity_against_a_brute_force_pair_count(seed):
    """integer scores from a small range: ties everywhere; a pair (held-out, other admissible) counts 1 when the held-out item
    is above, 1/2 when they tie"""
    rng = np.random.default_rng(seed)
    n, m = 12, 40
    S = rng.integers(-3, 4, size=(n, m)).astype(np.float64)
    act = sp.csr_matrix((rng.random((n, m)) < 0.2).astype(np.float64))
    nr = sp.csr_matrix((rng.random((n, m)) < 0.15).astype(np.float64))
    excl = [5, 17]
    above, tied, n_adm = percentile_ranks(S, act, nr, excl)
    s = rank_summary(above, tied, n_adm, act)
    adm = np.ones((n, m), bool)
    adm[nr.nonzero()] = False
    adm[:, excl] = False
    for u in range(n):
        held = [h for h in act.indices[act.indptr[u]:act.indptr[u + 1]] if adm[u, h]]
        others = [j for j in range(m) if adm[u, j] and j not in held]
        if not held or not others:
            assert np.isnan(s["auc"][u])
            continue
        good = sum(1.0 if S[u, h] > S[u, j] else (0.5 if S[u, h] == S[u, j] else 0.0) for h in held for j in others)
        assert s["auc"][u] == pytest.approx(good / (len(held) * len(others)), rel=1e-13)


# ---- the C ABI's argument checks (before any device work) ---------------------------------------------------------------------
def test_entry_points_and_status_codes_without_device():
    import ctypes
    lib = _lib.load()
    for name in ("rsparse_hip_held_out_ranks_device", "rsparse_hip_rank_summary_device", "rsparse_hip_held_out_ranks"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.rsparse_hip_abi_version() == 6
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    U, V = np.ones((2, 4), np.float32), np.ones((3, 4), np.float32)
    p, j = np.array([0, 2, 3], np.int32), np.array([0, 2, 1], np.int32)
    w = np.ones(3)
    ab, ti, na = np.empty(3, np.int32), np.empty(3, np.int32), np.empty(2, np.int32)
    ex = np.array([1], np.int32)

    def ranks(U=U, V=V, n=2, m=3, r=4, ex=None, n_ex=0, p=p, j=j, chunk=0, ab=ab, ti=ti, na=na):
        return lib.rsparse_hip_held_out_ranks_device(vp(U), vp(V), n, m, r, None, None, vp(ex), n_ex, vp(p), vp(j), chunk, vp(ab),
                                                     vp(ti), vp(na), None)

    for bad in (dict(U=None), dict(V=None), dict(p=None), dict(j=None), dict(ab=None), dict(ti=None), dict(na=None), dict(n=-1),
                dict(m=-1), dict(r=0), dict(chunk=-1), dict(n_ex=1), dict(n_ex=-1, ex=ex)):
        assert ranks(**bad) == _lib.ERR_INVALID, bad
    assert ranks(r=257) == _lib.ERR_UNSUPPORTED
    assert ranks(n=0) == _lib.OK                                          # no user: a no-op
    out = np.empty(2)

    def summary(n=2, p=p, w=w, ab=ab, ti=ti, na=na, mpr=out, auc=out, mrr=out, sums=None):
        return lib.rsparse_hip_rank_summary_device(n, vp(p), vp(w), vp(ab), vp(ti), vp(na), vp(mpr), vp(auc), vp(mrr), vp(sums), None)

    for bad in (dict(mpr=None, auc=None, mrr=None), dict(n=-1), dict(p=None), dict(ab=None), dict(ti=None), dict(na=None),
                dict(w=None), dict(w=None, mpr=None, auc=None, mrr=None, sums=np.empty(6))):
        assert summary(**bad) == _lib.ERR_INVALID, bad
    assert summary(n=0) == _lib.OK
    x, y = np.ones((2, 4), order="F"), np.ones((4, 3), order="F")

    def host(x=x, y=y, n=2, m=3, r=4, p=p, j=j, w=w, ab=ab, mpr=out):
        return lib.rsparse_hip_held_out_ranks(vp(x), vp(y), n, m, r, None, None, None, 0, vp(p), vp(j), vp(w), vp(ab), None, None,
                                              vp(mpr), None, None, None)

    for bad in (dict(x=None), dict(y=None), dict(p=None), dict(j=None), dict(ab=None, mpr=None), dict(w=None), dict(r=0), dict(n=-1),
                dict(p=np.array([1, 2, 3], np.int32)), dict(p=np.array([0, 3, 2], np.int32)), dict(j=np.array([2, 0, 1], np.int32))):
        assert host(**bad) == _lib.ERR_INVALID, bad
    assert host(r=257) == _lib.ERR_UNSUPPORTED
    assert host(n=0, p=np.zeros(1, np.int32)) == _lib.OK
    assert host() not in (_lib.ERR_INVALID, _lib.ERR_UNSUPPORTED)         # a valid call gets past every check (no device here)


# ---- the class through the CPU stand-in, on MovieLens -----------------------------------------------------------------------
N_EVAL = 120   # users evaluated: the first rows of the training matrix


_models = {}


def _ml_model(ml_train):
    if "m" not in _models:
        _models["m"] = _fit_ml_model(ml_train)
    return _models["m"]


def _fit_ml_model(ml_train):
    sys.path.insert(0, str(ROOT / "tests"))
    from oracle_backend import OracleBackend
    from rsparse_amd import WRMF
    n_user, n_item, p, i, x = ml_train
    train = sp.csc_matrix((x, i, p), shape=(n_user, n_item)).tocsr()
    seen, held = train[:N_EVAL].copy(), train[:N_EVAL].copy()
    seen.data[1::2] = 0.0
    held.data[0::2] = 0.0
    seen.eliminate_zeros(); held.eliminate_zeros()
    held.data[::5] = 0.0                       # stored zeros are entries (of weight 0)
    model = WRMF(rank=8, lambda_=0.1, feedback="implicit", solver="cholesky", precision="float", backend=OracleBackend(), rng=1)
    model.fit_transform(train[:300], n_iter=2, convergence_tol=-1)   # (one process: every rank holds the same model)
    return model, seen, held


def _reference(model, seen, held, not_recommend, excl):
    emb = model.transform(seen).astype(np.float64)
    comp = np.asarray(model.components, dtype=np.float64)
    S = (emb @ comp).astype(np.float32)        # the scores are fp32 ones
    return percentile_ranks(S, held, not_recommend, excl)


def test_class_equals_the_numpy_statement_on_movielens(ml_train):
    model, seen, held = _ml_model(ml_train)
    excl = [0, 49, 99]
    # some held-out items are also in not_recommend: the user's own `seen` row plus every fourth held-out entry
    extra = held.copy()
    extra.data[:] = 0.0
    extra.data[::4] = 1.0
    extra.eliminate_zeros()
    nr = (seen + extra).tocsr()
    above, tied, n_adm = model.held_out_ranks(seen, held, not_recommend=nr, items_exclude=excl)
    ra, rt, rn = _reference(model, seen, held, nr, excl)
    pat = canonical_actual(held, N_EVAL)
    for got in (above, tied):
        assert sp.isspmatrix_csr(got) and got.dtype == np.int32 and got.shape == held.shape
        assert np.array_equal(got.indptr, pat.indptr) and np.array_equal(got.indices, pat.indices)
    assert np.array_equal(above.data, ra.data) and np.array_equal(tied.data, rt.data) and np.array_equal(n_adm, rn)
    assert (above.data == -1).sum() >= held.nnz // 4 and np.array_equal(above.data == -1, tied.data == -1)
    # the default not_recommend is x itself; CSC / COO input is canonicalised
    a2, t2, n2 = model.held_out_ranks(seen, held.tocsc())
    ra2, rt2, rn2 = _reference(model, seen, held, seen, ())
    assert np.array_equal(a2.data, ra2.data) and np.array_equal(t2.data, rt2.data) and np.array_equal(n2, rn2)
    assert (a2.data >= 0).all()                # seen and held are disjoint
    # evaluate_ranks is the summary of those counts
    ev = model.evaluate_ranks(seen, held, not_recommend=nr, items_exclude=excl, per_user=True)
    ref = rank_summary(ra, rt, rn, held)
    tot = rank_totals(ref)
    assert set(ev) == {"mpr", "auc", "mrr", "n", "mpr_per_user", "auc_per_user", "mrr_per_user", "n_adm_per_user"}
    assert ev["n"] == tot["n"] == int((ra.data >= 0).sum())
    cnt = np.diff(pat.indptr)
    for name in ("mpr", "auc", "mrr"):
        got, want = ev[name + "_per_user"], ref[name]
        assert got.dtype == np.float64 and np.array_equal(np.isnan(got), np.isnan(want)), name
        ok = ~np.isnan(want)
        assert np.all(np.abs(got[ok] - want[ok]) <= 2.0 * (cnt[ok] + 2) * 2.0 ** -52 * np.abs(want[ok])), name
        assert abs(ev[name] - tot[name]) <= 2.0 * (pat.nnz + 2) * 2.0 ** -52 * abs(tot[name]), name
    assert np.array_equal(ev["n_adm_per_user"], rn)
    assert 0.0 < ev["mpr"] < 0.5 < ev["auc"] < 1.0      # a fitted model ranks held-out items above the middle
    assert set(model.evaluate_ranks(seen, held)) == {"mpr", "auc", "mrr", "n"}
    # nothing held out at all
    none = sp.csr_matrix(held.shape)
    a0, t0, n0 = model.held_out_ranks(seen, none)
    assert a0.nnz == 0 and t0.nnz == 0 and np.array_equal(n0, rn2)
    e0 = model.evaluate_ranks(seen, none)
    assert e0["n"] == 0 and np.isnan(e0["mpr"]) and np.isnan(e0["auc"]) and np.isnan(e0["mrr"])


def test_argument_errors(ml_train):
    model, seen, held = _ml_model(ml_train)
    for fn in (model.held_out_ranks, model.evaluate_ranks):
        with pytest.raises(ValueError, match="ncol"):
            fn(seen[:, :50], held)
        with pytest.raises(ValueError):
            fn(seen, held[:10])                          # row count
        with pytest.raises(ValueError):
            fn(seen, held[:, :50])                       # column count
        with pytest.raises(TypeError):
            fn(seen, held.toarray())                     # not sparse
        with pytest.raises(TypeError):
            fn(seen, held, not_recommend=seen.toarray())
        with pytest.raises(ValueError):
            fn(seen, held, not_recommend=seen[:10])
        with pytest.raises(ValueError):
            fn(seen, held, items_exclude=[seen.shape[1]])
    from rsparse_amd import WRMF
    with pytest.raises(RuntimeError):
        WRMF(rank=4, precision="float").held_out_ranks(seen, held)
    with pytest.raises(RuntimeError):
        WRMF(rank=4, precision="float").evaluate_ranks(seen, held)


# ---- world sizes 1 and 2 ----------------------------------------------------------------------------------------------------
def _both(model, seen, held):
    return {"ranks": model.held_out_ranks(seen, held, items_exclude=[3]),
            "plain": model.evaluate_ranks(seen, held, items_exclude=[3]),
            "per_user": model.evaluate_ranks(seen, held, items_exclude=[3], per_user=True)}


def _worker(rank, ws, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    sys.path.insert(0, str(ROOT / "tests"))
    from conftest import csc_take_rows, load_movielens
    n_user, n_item, p, i, x = load_movielens()
    model, seen, held = _ml_model((900, n_item) + tuple(csc_take_rows(900, p, i, x)))
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        torch.save(_both(model, seen, held), os.path.join(out_dir, "w%d_%d.pt" % (ws, rank)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("ws", [1, 2])
def test_gloo_world_sizes_give_the_one_process_result(ml_train, tmp_path, ws):
    import torch.multiprocessing as mp
    model, seen, held = _ml_model(ml_train)
    one = _both(model, seen, held)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(ws, port, str(tmp_path)), nprocs=ws, join=True)
    for r in range(ws):
        got = torch.load(tmp_path / ("w%d_%d.pt" % (ws, r)), weights_only=False)
        for k in range(2):
            a, b = got["ranks"][k], one["ranks"][k]
            assert a.dtype == b.dtype and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
            assert np.array_equal(a.data, b.data)
        assert np.array_equal(got["ranks"][2], one["ranks"][2])
        for key in ("plain", "per_user"):
            assert set(got[key]) == set(one[key])
            for name in one[key]:
                assert np.array_equal(got[key][name], one[key][name], equal_nan=True), (r, key, name)
