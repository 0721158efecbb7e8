"""EASE under the evaluation protocols without a GPU: the three numpy definitions (ease_score_pairs_reference,
ease_candidates_reference, ease_ranks_reference) against brute force -- dense score rows, a Python sort, counts --, the class on the
CPU stand-in on the MovieLens split, where it runs those definitions, the refusals, and the ABI table."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from rsparse_amd import EASE, WRMF, _lib
from rsparse_amd.ease import (ease_candidates_reference, ease_gram_reference, ease_ranks_reference, ease_recommend_reference,
                              ease_score_pairs_reference, ease_scores_reference, ease_weights_reference)
from rsparse_amd.itemknn import canonical_pattern
from rsparse_amd.metrics import rank_summary, rank_totals
from test_ease_host import protocol
from test_metrics_abi import _oracle_metrics_backend

ROOT = Path(__file__).resolve().parent.parent
DEVICE_NAMES = ("rsparse_hip_ease_score_pairs_device", "rsparse_hip_ease_top_candidates_device", "rsparse_hip_ease_held_out_ranks_device")
HOST_NAMES = ("rsparse_hip_ease_top_candidates", "rsparse_hip_ease_held_out_ranks")
METRICS = ("ap", "ndcg", "precision", "recall", "hit", "mrr", "coverage", "popularity", "novelty")


@pytest.fixture(scope="module")
def split():
    """-> (train, hist, held, B float64, the dense scores of hist): computed once, left unchanged"""
    train, hist, held = protocol()
    B = ease_weights_reference(ease_gram_reference(train, 500.0))
    score = ease_scores_reference(hist, B)
    score.setflags(write=False)
    return train, hist, held, B, score


@pytest.fixture(scope="module")
def model(split):
    return EASE(500.0, precision="double", backend=_oracle_metrics_backend()).fit(split[0])


def ties():
    """a 4-item B of small integers and three rows: exact ties, a row without a history"""
    B = np.array([[0.0, 1.0, 1.0, -2.0], [0.5, 0.0, 0.5, 0.5], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 0.0]])
    x = sp.csr_matrix(np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0]], dtype=float))
    return x, B


# ---- the definitions ----------------------------------------------------------------------------------------------------------------
def test_score_pairs_reference_is_the_dense_row_at_the_cells(split):
    _, hist, _, B, score = split
    pairs = sp.csr_matrix(np.random.default_rng(1).random(hist.shape) < 0.02)
    got = ease_score_pairs_reference(hist, B, pairs)
    pat = canonical_pattern(pairs)
    want = np.array([score[u, j] for u in range(hist.shape[0]) for j in pat.indices[pat.indptr[u]:pat.indptr[u + 1]]])
    assert got.dtype == np.float64 and got.shape == (pat.nnz,) and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    own = ease_score_pairs_reference(hist, B, hist)                          # nothing is masked: the row's own history has a score
    assert np.array_equal(own, score[hist.nonzero()]) and (own != 0).any()
    with pytest.raises(ValueError):
        ease_score_pairs_reference(hist, B, pairs[:5])


def test_candidates_reference_is_the_brute_force_order(split):
    _, hist, _, B, score = split
    rng = np.random.default_rng(2)
    d = rng.random(hist.shape) < 0.05
    d[3] = False                                                            # a row without candidates
    d[4] = hist[4].toarray()[0] != 0                                        # candidates that not_recommend = x masks, all of them
    cand, excl = sp.csr_matrix(d), (1, 49)
    seen = hist.toarray() != 0
    for k in (1, 10, 200):
        items, scores = ease_candidates_reference(hist, B, cand, k, hist, excl)
        for u in range(hist.shape[0]):
            adm = [j for j in np.flatnonzero(d[u]) if not seen[u, j] and j not in excl]
            want = sorted(adm, key=lambda j: (-score[u, j], j))[:k]
            assert items[u, :len(want)].tolist() == want and (items[u, len(want):] == -1).all()
            assert scores[u, :len(want)].tolist() == [score[u, j] for j in want] and (scores[u, len(want):] == 0).all()
        assert (items[3] == -1).all() and (items[4] == -1).all()
    # ties to the smaller item, candidates of score 0 are ranked, k above the admissible count
    x, Bt = ties()
    every = sp.csr_matrix(np.ones((3, 4)))
    it, sc = ease_candidates_reference(x, Bt, every, 5, x, (3,))
    assert np.array_equal(it, [[1, 2, -1, -1, -1], [0, 2, -1, -1, -1], [0, 1, 2, -1, -1]])
    assert np.array_equal(sc, [[1, 1, 0, 0, 0], [0.5, 0.5, 0, 0, 0], [0, 0, 0, 0, 0]])
    it, sc = ease_candidates_reference(x, Bt, sp.csr_matrix(np.array([[0, 0, 1, 1], [1, 0, 0, 1], [0, 1, 0, 1]])), 2)
    assert np.array_equal(it, [[2, 3], [0, 3], [1, 3]]) and np.array_equal(sc, [[1, -2], [0.5, 0.5], [0, 0]])
    with pytest.raises(ValueError):
        ease_candidates_reference(x, Bt, every[:2], 2)


def test_candidates_holding_every_item_are_ease_recommend(split):
    _, hist, _, B, _ = split
    every = sp.csr_matrix(np.ones(hist.shape))
    for k, nr, excl in ((10, hist, ()), (7, None, (0, 49, 180)), (25, hist, (1, 2, 3))):
        a, c = ease_recommend_reference(hist, B, k, nr, excl), ease_candidates_reference(hist, B, every, k, nr, excl)
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1].view(np.uint64), c[1].view(np.uint64))


def test_ranks_reference_is_the_brute_force_count(split):
    _, hist, held, B, score = split
    seen = hist.toarray() != 0
    excl = (5,)
    act = held[:12].tolil()
    act[0, 5] = 1.0                                                         # an excluded entry
    act[1, hist[1].indices[0]] = 1.0                                        # an entry of the row's own history
    act = act.tocsr()
    above, tied, n_adm = ease_ranks_reference(hist[:12], B, act, hist[:12], excl)
    assert above.dtype == tied.dtype == n_adm.dtype == np.int32 and above.shape == (act.nnz,)
    e = 0
    for u in range(12):
        adm = [j for j in range(hist.shape[1]) if not seen[u, j] and j not in excl]
        assert n_adm[u] == len(adm)
        for h in act.indices[act.indptr[u]:act.indptr[u + 1]]:
            if h in adm:
                assert above[e] == sum(score[u, j] > score[u, h] for j in adm)
                assert tied[e] == sum(score[u, j] == score[u, h] for j in adm if j != h)
            else:
                assert above[e] == -1 and tied[e] == -1
            e += 1
    assert e == act.nnz and (above == -1).sum() == 2
    # the row without a history is one tie; an entry outside the items; everything masked
    x, Bt = ties()
    wide = sp.csr_matrix(np.array([[0, 1, 1, 0, 1], [1, 0, 0, 1, 0], [0, 0, 1, 0, 0]], dtype=float))   # column 4: outside
    above, tied, n_adm = ease_ranks_reference(x, Bt, wide, x)
    assert above.tolist() == [0, 0, -1, 0, 0, 0] and tied.tolist() == [1, 1, -1, 2, 2, 3] and n_adm.tolist() == [3, 3, 4]
    above, tied, n_adm = ease_ranks_reference(x, Bt, wide, sp.csr_matrix(np.ones((3, 4))))
    assert (n_adm == 0).all() and (above == -1).all() and (tied == -1).all()


# ---- the class on the CPU stand-in ---------------------------------------------------------------------------------------------
def test_predict_with_candidates(split, model):
    _, hist, _, B, _ = split
    cand = sp.csr_matrix(np.random.default_rng(5).random(hist.shape) < 0.1)
    top = model.predict(hist, 10, items_exclude=(49,), candidates=cand.tocsc())   # any sparse format
    ref = ease_candidates_reference(hist, B, cand, 10, hist, (49,))
    assert np.array_equal(np.asarray(top), ref[0]) and top.scores.dtype == np.float64
    assert np.array_equal(top.scores, np.where(ref[0] < 0, np.nan, ref[1]), equal_nan=True)
    every = sp.csr_matrix(np.ones(hist.shape))
    a, c = model.predict(hist, 9), model.predict(hist, 9, candidates=every)
    assert np.array_equal(np.asarray(a), np.asarray(c)) and np.array_equal(a.scores, c.scores, equal_nan=True)


def test_evaluate_with_negatives_is_evaluate_on_the_sampled_candidates(split, model):
    _, hist, held, _, _ = split
    cand = WRMF(backend=_oracle_metrics_backend()).sample_negatives(hist, 99, actual=held, seed=7)
    mine = model.sample_negatives(hist, 99, actual=held, seed=7)
    assert np.array_equal(cand.indptr, mine.indptr) and np.array_equal(cand.indices, mine.indices)
    assert np.array_equal(np.diff(cand.indptr), np.diff(held.indptr) + 99)   # the held-out items are kept, 99 negatives beside them
    assert cand.multiply(hist).nnz == 0                                      # nothing of not_recommend = x is drawn
    a = model.evaluate(hist, held, (5, 10), metrics=METRICS, negatives=99, seed=7)
    c = model.evaluate(hist, held, (5, 10), metrics=METRICS, candidates=cand)
    plain = model.evaluate(hist, held, (5, 10), metrics=METRICS)
    assert set(a) == set(c) == set(METRICS)
    for name in METRICS:
        assert np.array_equal(a[name], c[name], equal_nan=True), name
    assert np.nanmean(a["hit"][:, 1]) > np.nanmean(plain["hit"][:, 1])       # 99 rivals are easier than 1682
    w = np.arange(1, hist.shape[1] + 1, dtype=np.float64)
    one = model.evaluate(hist, held, 5, negatives=20, seed=3, negative_weights=w)
    two = model.evaluate(hist, held, 5, candidates=model.sample_negatives(hist, 20, actual=held, seed=3, weights=w))
    assert set(one) == {"ap", "ndcg"} and all(np.array_equal(one[name], two[name], equal_nan=True) for name in one)


def test_score_has_the_bits_of_the_lists_scores(split, model):
    _, hist, _, B, score = split
    pairs = sp.csr_matrix(np.random.default_rng(6).random(hist.shape) < 0.03)
    got = model.score(hist, pairs)
    assert got.dtype == np.float64 and got.shape == hist.shape and np.array_equal(got.data, ease_score_pairs_reference(hist, B, pairs))
    top = model.predict(hist, 5, not_recommend=None)
    listed = sp.csr_matrix((np.ones(top.size), (np.repeat(np.arange(top.shape[0]), 5), np.asarray(top).ravel())), shape=hist.shape)
    dense = model.score(hist, listed).toarray()
    for u in range(hist.shape[0]):
        assert np.array_equal(top.scores[u], dense[u, np.asarray(top)[u]])
    # stored zeros of `pairs` are positions too, duplicates merge
    odd = sp.csr_matrix((np.array([0.0, 1.0, 1.0]), (np.array([1, 1, 1]), np.array([4, 2, 2]))), shape=hist.shape)
    assert model.score(hist, odd).indices.tolist() == [2, 4] and np.array_equal(model.score(hist, odd).data, score[1, [2, 4]])


def test_ranks_on_the_stand_in(split, model):
    _, hist, held, B, _ = split
    ref = ease_ranks_reference(hist, B, held, hist, (1,))
    above, tied, n_adm = model.held_out_ranks(hist, held, items_exclude=(1,))
    assert np.array_equal(above.data, ref[0]) and np.array_equal(tied.data, ref[1]) and np.array_equal(n_adm, ref[2])
    assert above.dtype == np.int32 and np.array_equal(above.indptr, held.indptr) and n_adm.dtype == np.int32
    ev = model.evaluate_ranks(hist, held, items_exclude=(1,), per_user=True)
    summ = rank_summary(above, tied, n_adm, held)
    tot = rank_totals(summ)
    assert set(ev) == {"mpr", "auc", "mrr", "n", "mpr_per_user", "auc_per_user", "mrr_per_user", "n_adm_per_user"}
    assert ev["n"] == tot["n"] == int((ref[0] >= 0).sum())
    for name in ("mpr", "auc", "mrr"):
        assert np.allclose(ev[name + "_per_user"], summ[name], rtol=1e-13, atol=0, equal_nan=True), name
        assert np.isclose(ev[name], tot[name], rtol=1e-13, atol=0), name
    assert set(model.evaluate_ranks(hist, held)) == {"mpr", "auc", "mrr", "n"} and ev["auc"] > 0.8
    none = model.evaluate_ranks(hist, sp.csr_matrix(hist.shape))
    assert none["n"] == 0 and np.isnan(none["mpr"])


def test_argument_refusals(split, model):
    _, hist, held, _, _ = split
    every = sp.csr_matrix(np.ones(hist.shape))
    with pytest.raises(ValueError, match="shape"):
        model.predict(hist, 3, candidates=every[:5])
    with pytest.raises(ValueError, match="shape"):
        model.predict(hist, 3, candidates=every[:, :5])
    with pytest.raises(TypeError):
        model.predict(hist, 3, candidates=every.toarray())
    with pytest.raises(ValueError, match="seed"):
        model.evaluate(hist, held, 3, negatives=3)
    with pytest.raises(ValueError, match="exclude each other"):
        model.evaluate(hist, held, 3, negatives=3, seed=1, candidates=every)
    with pytest.raises(ValueError, match="negative_weights needs negatives"):
        model.evaluate(hist, held, 3, negative_weights=np.ones(hist.shape[1]))
    with pytest.raises(ValueError, match="seed"):
        model.sample_negatives(hist, 3)
    with pytest.raises(ValueError):
        model.evaluate(hist, held, 3, negatives=0, seed=1)
    with pytest.raises(_lib.UnsupportedOnDevice):
        model.evaluate(hist, held, 3, negatives=3, seed=1, metrics=("diversity",))
    with pytest.raises(ValueError, match="shape"):
        model.score(hist, every[:, :5])
    with pytest.raises(TypeError):
        model.score(hist, every.toarray())
    with pytest.raises(ValueError, match="shape"):
        model.held_out_ranks(hist, held[:, :5])
    with pytest.raises(TypeError):
        model.evaluate_ranks(hist, held.toarray())
    with pytest.raises(ValueError):
        model.held_out_ranks(hist, held, items_exclude=(hist.shape[1],))
    unfitted = EASE(backend=_oracle_metrics_backend())
    for call in (lambda: unfitted.score(hist, every), lambda: unfitted.held_out_ranks(hist, held),
                 lambda: unfitted.predict(hist, 3, candidates=every)):
        with pytest.raises(RuntimeError):
            call()


def test_more_than_one_rank_is_refused(split, model, monkeypatch):
    import torch.distributed as dist
    _, hist, held, _, _ = split
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda: 2)
    every = sp.csr_matrix(np.ones(hist.shape))
    for call in (lambda: model.predict(hist, 3, candidates=every), lambda: model.score(hist, every), lambda: model.held_out_ranks(hist, held),
                 lambda: model.evaluate_ranks(hist, held), lambda: model.sample_negatives(hist, 3, seed=1),
                 lambda: model.evaluate(hist, held, 3, negatives=3, seed=1)):
        with pytest.raises(_lib.UnsupportedOnDevice):
            call()


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points():
    lib = _lib.load()
    text = (ROOT / "include" / "rsparse_wrmf_hip.h").read_text()
    for name in DEVICE_NAMES + HOST_NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert lib.rsparse_hip_abi_version() == 6                                # additive entries: the version stays
    from rsparse_amd.engine import HipBackend
    assert all(callable(getattr(HipBackend, name)) for name in ("ease_score_pairs", "ease_top_candidates", "ease_held_out_ranks"))
    ratio = int(re.search(r"#define RSPARSE_HIP_EASE_CELLS_RATIO (\d+)", text).group(1))
    assert ratio == _lib.EASE_CELLS_RATIO and ratio >= 1


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _answer(rc, code, text):
    assert rc == code, (rc, _lib.load().rsparse_hip_last_error())
    assert text in _lib.load().rsparse_hip_last_error().decode(), _lib.load().rsparse_hip_last_error()


# 3 users x 4 items: rows {0, 2}, {1}, {0, 1, 3}
P = np.array([0, 2, 3, 6], dtype=np.int32)
J = np.array([0, 2, 1, 0, 1, 3], dtype=np.int32)


def aligned_weights():
    raw = np.zeros(4 * 4 + 8, np.float32)
    return raw[(-raw.ctypes.data // 4) % 4:][:16]                           # 16-byte aligned


@pytest.mark.parametrize("entry", ("score_pairs", "top_candidates", "held_out_ranks"))
def test_device_entries_status_codes(entry):
    # (host pointers: every call here is rejected by the argument checks, or has no row, before device work)
    fn = getattr(_lib.load(), "rsparse_hip_ease_%s_device" % entry)
    B = aligned_weights()
    res, sc = np.empty((3, 2), np.int32), np.empty(6, np.uint64)
    a32 = np.empty(6, np.int32)

    def call(xp=P, xj=J, n_rows=3, n_items=4, B=B, ld=4, f64=0, pp=P, pj=J, nr_p=None, nr_j=None, ex=None, n_ex=0, k=2, ws_rows=0, o1=res,
             o2=sc, o3=a32):
        head = (_vp(xp), _vp(xj), n_rows, n_items, _vp(B), ld, f64, _vp(pp), _vp(pj))
        if entry == "score_pairs":
            return fn(*head, ws_rows, _vp(o2), None)
        if entry == "top_candidates":
            return fn(*head, _vp(nr_p), _vp(nr_j), _vp(ex), n_ex, k, ws_rows, _vp(o1), _vp(o2), None)
        return fn(*head, _vp(nr_p), _vp(nr_j), _vp(ex), n_ex, ws_rows, _vp(o1), _vp(o3), _vp(a32), None)

    outputs = {"score_pairs": ("o2",), "top_candidates": ("o1", "o2"), "held_out_ranks": ("o1", "o3")}[entry]
    for missing in ("xp", "xj", "B", "pp", "pj") + outputs:
        _answer(call(**{missing: None}), _lib.ERR_INVALID, "NULL")
    _answer(call(n_rows=-1), _lib.ERR_INVALID, "bad dimensions")
    _answer(call(n_items=-1), _lib.ERR_INVALID, "bad dimensions")
    _answer(call(ws_rows=-1), _lib.ERR_INVALID, "ws_rows < 0")
    _answer(call(ld=3), _lib.ERR_INVALID, "ld_B < n_items")
    _answer(call(ld=6), _lib.ERR_INVALID, "multiple of 16 bytes")
    _answer(call(ld=5, f64=1), _lib.ERR_INVALID, "multiple of 16 bytes")
    _answer(call(B=B[1:]), _lib.ERR_INVALID, "multiple of 16 bytes")
    big = _lib.EASE_MAX_ITEMS + 1
    _answer(call(n_items=big, ld=big + 3), _lib.ERR_UNSUPPORTED, "n_items > 32768")
    if entry != "score_pairs":
        _answer(call(nr_p=P), _lib.ERR_INVALID, "nr_p without nr_j")
        _answer(call(n_ex=-1), _lib.ERR_INVALID, "bad exclude")
        _answer(call(n_ex=1), _lib.ERR_INVALID, "bad exclude")
    if entry == "top_candidates":
        _answer(call(k=0), _lib.ERR_INVALID, "k < 1")
        _answer(call(k=_lib.KNN_MAX_TOPK + 1), _lib.ERR_UNSUPPORTED, "k > 1024")
    assert call(n_rows=0) == _lib.OK                                         # no row: a no-op


def test_host_forms_check_their_arrays_first():
    lib = _lib.load()
    B = np.zeros((4, 4), np.float64, order="F")
    res, sc = np.empty((3, 2), np.int32, order="F"), np.empty((3, 2), np.float64, order="F")
    a32, n32 = np.empty(6, np.int32), np.empty(3, np.int32)
    ex = np.array([1], dtype=np.int32)

    def cand(xp=P, xj=J, n_rows=3, n_items=4, B=B, f64=1, cp=P, cj=J, nr_p=None, nr_j=None, ex=None, n_ex=0, k=2, res=res, sc=sc):
        return lib.rsparse_hip_ease_top_candidates(_vp(xp), _vp(xj), n_rows, n_items, _vp(B), f64, _vp(cp), _vp(cj), _vp(nr_p), _vp(nr_j),
                                                   _vp(ex), n_ex, k, _vp(res), _vp(sc))

    def ranks(xp=P, xj=J, n_rows=3, n_items=4, B=B, f64=1, ap=P, aj=J, nr_p=None, nr_j=None, ex=None, n_ex=0, above=a32, tied=a32, n_adm=n32):
        return lib.rsparse_hip_ease_held_out_ranks(_vp(xp), _vp(xj), n_rows, n_items, _vp(B), f64, _vp(ap), _vp(aj), _vp(nr_p), _vp(nr_j),
                                                   _vp(ex), n_ex, _vp(above), _vp(tied), _vp(n_adm))

    for missing in ("xp", "B", "cp", "res", "sc"):
        _answer(cand(**{missing: None}), _lib.ERR_INVALID, "NULL")
    for missing in ("xp", "B", "ap", "above", "tied", "n_adm"):
        _answer(ranks(**{missing: None}), _lib.ERR_INVALID, "NULL")
    bad = B.copy(order="F")
    bad[2, 1] = np.nan
    for fn in (cand, ranks):
        _answer(fn(xj=None), _lib.ERR_INVALID, "x_j is NULL")
        _answer(fn(n_ex=1), _lib.ERR_INVALID, "bad exclude")
        _answer(fn(nr_p=P), _lib.ERR_INVALID, "nr_p without nr_j")
        _answer(fn(xp=np.array([0, 3, 2, 6], np.int32)), _lib.ERR_INVALID, "x_p decreases")
        _answer(fn(xj=np.array([0, 2, 1, 0, 1, 4], np.int32)), _lib.ERR_INVALID, "x_j has a column outside [0, n_items)")
        _answer(fn(nr_p=P, nr_j=np.array([0, 2, 1, 0, 1, 9], np.int32)), _lib.ERR_INVALID, "nr_j has a column outside [0, n_items)")
        _answer(fn(B=bad), _lib.ERR_INVALID, "not finite")
        _answer(fn(B=bad.astype(np.float32), f64=0), _lib.ERR_INVALID, "not finite")
        _answer(fn(n_items=_lib.EASE_MAX_ITEMS + 1), _lib.ERR_UNSUPPORTED, "n_items > 32768")
    _answer(cand(k=0), _lib.ERR_INVALID, "k < 1")
    _answer(cand(k=1025), _lib.ERR_UNSUPPORTED, "k > 1024")
    _answer(cand(cj=None), _lib.ERR_INVALID, "cand_j is NULL")
    _answer(cand(cp=np.array([1, 2, 3, 6], np.int32)), _lib.ERR_INVALID, "cand_p[0] != 0")
    _answer(cand(cp=np.array([0, 3, 2, 6], np.int32)), _lib.ERR_INVALID, "cand_p decreases")
    _answer(cand(cj=np.array([0, 2, 1, 0, 1, 4], np.int32)), _lib.ERR_INVALID, "cand_j has a column outside [0, n_items)")
    _answer(cand(cj=np.array([2, 0, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "not strictly ascending")   # the cell route's precondition
    _answer(ranks(aj=None), _lib.ERR_INVALID, "actual_j is NULL")
    _answer(ranks(ap=np.array([0, 3, 2, 6], np.int32)), _lib.ERR_INVALID, "actual_p decreases")
    _answer(ranks(aj=np.array([2, 0, 1, 0, 1, 3], np.int32)), _lib.ERR_INVALID, "not strictly ascending")
    assert cand(n_rows=0, xp=np.zeros(1, np.int32), cp=np.zeros(1, np.int32), ex=ex, n_ex=1) == _lib.OK     # no row: a no-op
    assert ranks(n_rows=0, xp=np.zeros(1, np.int32), ap=np.zeros(1, np.int32)) == _lib.OK
