"""The host-array forms of the C ABI (csrc/wrmf_capi_host.cpp) refuse a bad call with a status code and a text behind
rsparse_hip_last_error().  The other suites pin the code and that there is a text; this one pins the text, byte for byte, and
with it which check fires first when a call has two faults.  The expected strings were taken from the library as it was before
the host forms moved into their own file and onto shared validators.  Every call here returns before device work (host
pointers, no device needed), as do the no-op calls at the end, whose writes to the caller's arrays are part of the contract."""
import ctypes

import numpy as np
import pytest

from rsparse_amd import _lib

INVALID, UNSUPPORTED = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED


def I32(*a):
    return np.array(a, np.int32)


# two users, lists of three, five items; the actual / seen / candidate matrix: rows {1, 4} and {0}
PRED, SCORES, CUT = np.ones(6, np.int32), np.zeros(6), I32(1, 3)
P, J, X = I32(0, 2, 3), I32(1, 4, 0), np.array([1.0, 2.0, 3.0])
P_FROM_1, P_DOWN, J_UP = I32(1, 2, 3), I32(0, 3, 2), I32(0, 1, 4)     # P_DOWN goes with J_UP: its first row has to pass
J_DOWN, J_OUT, J_NEG = I32(4, 1, 0), I32(1, 5, 0), I32(-1, 4, 0)
D, OI, OD = np.zeros(1200), np.zeros(64, np.int32), np.zeros(64)         # any matrix of doubles; integer / double outputs
COUNT, INFO, W = I32(1, 1, 1, 1, 1), np.ones(5, np.int64), np.ones(5, np.uint32)
NAN = np.array([5.0, np.nan, 1.0])

_TOP = dict(x=D, y=D, nr=2, nc=5, rank=2, k=3, n_threads=1)
_TOP_TAIL = dict(nr_p=None, nr_j=None, exclude=None, n_exclude=0, glob_mean=0.0, res=OI, scores=OD)
_LISTS = dict(pred=PRED, n_users=2, k=3)
_CUTS = dict(cutoffs=CUT, n_cutoffs=2)
_WINDOW = dict(V=D, n_items=5, ld=4, c0=0, c1=4)
_MMR = dict(lists=PRED, scores=SCORES, n_users=2, n_pool=3, k=2, trade_off=0.5, **_WINDOW, items=OI, scores_out=None, positions=None,
            objective=None)
_SAMPLE = dict(seed=1, row0=0, n_rows=2, n_item=5, n=2, seen_p=P, seen_j=J, keep_p=None, keep_j=None)
_SAMPLE_OUT = dict(out_p=np.zeros(3, np.int32), out_j=OI, out_capacity=64)
DEFAULTS = {          # a good call of each entry, arguments in the order of the header
    "top_product": dict(**_TOP, **_TOP_TAIL),
    "top_candidates": dict(**_TOP, cand_p=P, cand_j=J, **_TOP_TAIL),
    "similar_items": dict(components=D, rank=4, n_items=5, first_row=0, n_rows=4, query=I32(1, 2), n_q=2, k=3, exclude_self=1, exclude=None,
                          n_exclude=0, res=OI, scores=OD),
    "ranking_metrics": dict(**_LISTS, p=P, j=J, x=X, ap_out=OD, ndcg_out=OD),
    "hit_metrics": dict(**_LISTS, p=P, j=J, **_CUTS, hits=OI, first=None, precision=None, recall=None, hit=None, mrr=None, first_seen=None,
                        n_items=5),
    "list_metrics": dict(**_LISTS, **_CUTS, item_count=COUNT, item_info=INFO, n_items=5, valid=OI, count_sum=None, info_sum=None,
                         popularity=None, novelty=None, exposure=None),
    "list_diversity": dict(**_LISTS, **_CUTS, **_WINDOW, counted=OI, diversity=None),
    "list_diversity_f64": dict(**_LISTS, **_CUTS, **_WINDOW, counted=OI, diversity=None),
    "mmr_rerank": _MMR,
    "mmr_rerank_f64": _MMR,
    "held_out_ranks": dict(x=D, y=D, nr=2, nc=5, rank=2, nr_p=None, nr_j=None, exclude=None, n_exclude=0, p=P, j=J, ax=X, above=OI, tied=OI,
                           n_adm=OI, mpr=None, auc=None, mrr=None, sums=None),
    "sparse_approximation": dict(n_rows=2, n_cols=5, p=P, idx=J, sparse_matrix_type=2, X=D, Y=D, rank=2, values_out=OD),
    "sample_negatives": dict(**_SAMPLE, **_SAMPLE_OUT),
    "sample_negatives_weighted": dict(**_SAMPLE, w=W, **_SAMPLE_OUT, filled_rows=None),
    "split_rows": dict(seed=1, row0=0, n_rows=2, mode=0, test_threshold=2 ** 31, leave_out=1, min_train=1, p=P, j=J, v=X, value_bytes=8,
                       by=None, train_p=OI, train_j=OI, train_v=OD, test_p=OI, test_j=OI, test_v=OD, train_capacity=8, test_capacity=8),
    "confidence": dict(kind=0, n_rows=2, n_cols=5, p=P, j=J, x=X, a=1.0, b=1.0, norm=2, by_columns=0, out=OD),
    "events_to_csr": dict(n_events=3, n_users=2, n_items=5, users=I32(0, 0, 1), items=J, values=X, timestamps=None, aggregate=0,
                          half_life=0.0, now=0.0, has_now=0, p=OI, j=OI, x=OD, count=None, latest=None, capacity=8,
                          n_cells=ctypes.c_int64(5)),
}


def _call(name, **over):
    args = dict(DEFAULTS[name])
    assert set(over) <= set(args), (name, over)
    args.update(over)
    raw = [ctypes.byref(v) if isinstance(v, ctypes.c_int64) else v.ctypes.data_as(ctypes.c_void_p) if isinstance(v, np.ndarray) else v
           for v in args.values()]
    return getattr(_lib.load(), "rsparse_hip_" + name)(*raw)


K_MSG = "k > 8192 (RSPARSE_HIP_MAX_TOPK_LARGE) is not on the device path"
CUT_MSG = "cutoffs must be strictly ascending within 1 .. k"
WIDE_MSG = "more than 256 latent coordinates are not on the device path"
WINDOW_MSG = "bad dimensions (n_items < 0 or not 0 <= c0 < c1 <= ld)"
ACTUAL = [(dict(p=P_FROM_1), "actual_p[0] != 0"), (dict(p=P_DOWN, j=J_UP), "actual_p decreases"),
          (dict(j=J_DOWN), "actual_j is not strictly ascending within a row")]
CUTS = [(dict(cutoffs=I32(3, 1)), CUT_MSG), (dict(cutoffs=I32(1, 4)), CUT_MSG), (dict(cutoffs=I32(0, 3)), CUT_MSG),
        (dict(n_cutoffs=17), "more than 16 cutoffs (RSPARSE_HIP_MAX_CUTOFFS) are not on the device path", UNSUPPORTED),
        (dict(n_cutoffs=0), "bad dimensions (n_users < 0, k < 1 or n_cutoffs < 1)"), (dict(k=8193), K_MSG, UNSUPPORTED)]
WINDOW = [(dict(V=None), "the factor matrix is NULL"), (dict(c0=2, c1=2), WINDOW_MSG), (dict(c1=5), WINDOW_MSG),
          (dict(ld=300, c1=257), WIDE_MSG, UNSUPPORTED), (dict(V=None, c0=-1), "the factor matrix is NULL")]
DIVERSITY = CUTS + WINDOW + [(dict(counted=None), "every output is NULL"), (dict(pred=None, n_users=-1), "predictions or cutoffs is NULL"),
                             (dict(n_items=0, V=None), "n_items < 1")]
MMR = WINDOW + [(dict(n_pool=8193), "a pool of more than 8192 (RSPARSE_HIP_MAX_TOPK_LARGE) is not on the device path", UNSUPPORTED),
                (dict(trade_off=1.5), "trade_off must lie in [0, 1]"), (dict(trade_off=float("nan")), "trade_off must lie in [0, 1]"),
                (dict(k=4), "bad dimensions (n_users < 0 or not 1 <= k <= n_pool)"), (dict(items=None), "the items output is NULL"),
                (dict(lists=None, items=None), "lists or scores is NULL"), (dict(n_items=0, trade_off=2.0), "trade_off must lie in [0, 1]")]
SAMPLE = [(dict(n=8193), "n > 8192 (RSPARSE_HIP_MAX_NEGATIVES) is not on the device path", UNSUPPORTED),
          (dict(seen_p=P_FROM_1), "seen_p[0] or keep_p[0] != 0"), (dict(keep_p=P_FROM_1, keep_j=J), "seen_p[0] or keep_p[0] != 0"),
          (dict(seen_p=P_DOWN, seen_j=J_UP), "seen_p or keep_p decreases"),
          (dict(seen_j=J_DOWN), "a seen index is outside the matrix, or a row's indices are not strictly ascending"),
          (dict(seen_j=J_OUT), "a seen index is outside the matrix, or a row's indices are not strictly ascending"),
          (dict(keep_p=I32(0, 2, 2), keep_j=I32(4, 1)), "a keep row's indices are not strictly ascending"),
          (dict(keep_p=I32(0, 1, 1), keep_j=I32(2)), "a keep row is not a subset of its seen row"),
          (dict(out_capacity=1), "out_capacity is 1, the rows need 4"),
          (dict(keep_p=P), "keep_p and keep_j must both be given or both be NULL"),
          (dict(seen_p=None, n_rows=-1), "bad dimensions (n_rows < 0, n_item < 0, n < 1, row0 < 0 or out_capacity < 0)"),
          (dict(row0=2 ** 32, seen_p=None), "the global row index row0 + n_rows does not fit 32 bits")]
WEIGHT_MSG = "a weight is 0: every weight is at least 1 (exclude an item through the seen rows)"

CASES = {
    "top_product": [(dict(k=8193), K_MSG, UNSUPPORTED), (dict(rank=257, k=8193), "rank > 256 is not on the device path", UNSUPPORTED),
                    (dict(x=None, nr=-1), "NULL matrix or output"), (dict(nr=-1, n_exclude=-1), "bad dimensions"), (dict(k=0), "bad dimensions"),
                    (dict(n_exclude=1), "bad exclude"), (dict(n_exclude=-1, k=8193), K_MSG, UNSUPPORTED)],
    "top_candidates": [(dict(k=8193), K_MSG, UNSUPPORTED), (dict(rank=129), "rank > 128 is not on the fp64 device path", UNSUPPORTED),
                       (dict(cand_p=P_FROM_1), "cand_p[0] != 0"), (dict(cand_p=P_DOWN), "cand_p decreases"),
                       (dict(cand_j=J_DOWN), "a candidate index is outside the matrix, or a row's indices are not strictly ascending"),
                       (dict(cand_j=J_OUT), "a candidate index is outside the matrix, or a row's indices are not strictly ascending"),
                       (dict(cand_j=None), "cand_j is NULL"), (dict(nr_p=P_FROM_1, nr_j=J), "nr_p[0] != 0"),
                       (dict(nr_p=P_DOWN, nr_j=J), "nr_p decreases"), (dict(cand_p=None, nr=-1), "cand_p is NULL"),
                       (dict(x=None, cand_p=None), "NULL matrix or output"), (dict(cand_p=P_FROM_1, n_exclude=1), "bad exclude"),
                       (dict(cand_p=P_FROM_1, nr_p=P_FROM_1, nr_j=J), "cand_p[0] != 0")],
    "similar_items": [(dict(k=8193), K_MSG, UNSUPPORTED), (dict(rank=300, n_rows=257), WIDE_MSG, UNSUPPORTED),
                      (dict(k=0), "bad dimensions (n_items < 0, n_q < 0, k < 1 or no latent coordinate)"), (dict(n_exclude=1), "bad exclude"),
                      (dict(first_row=-1), "first_row / n_rows do not select rows of components"),
                      (dict(first_row=1), "first_row / n_rows do not select rows of components"),
                      (dict(components=None, first_row=-1), "first_row / n_rows do not select rows of components"),
                      (dict(components=None, query=I32(0, 1)), "NULL matrix, query or output"), (dict(res=None), "NULL matrix, query or output"),
                      (dict(query=I32(1, 0)), "query item id out of range"), (dict(query=I32(6, 1)), "query item id out of range")],
    "ranking_metrics": ACTUAL + [(dict(k=8193), K_MSG, UNSUPPORTED), (dict(ap_out=None, ndcg_out=None, p=None), "ap_out and ndcg_out are both NULL"),
                                 (dict(p=None, n_users=-1), "predictions or actual (p, j) is NULL"),
                                 (dict(x=None, k=0), "ndcg needs the relevances: actual_x is NULL"),
                                 (dict(k=0), "bad dimensions (n_users < 0 or k < 1)")],
    "hit_metrics": ACTUAL + CUTS + [(dict(hits=None), "every output is NULL"),
                                    (dict(p=None, n_users=-1), "predictions, actual (p, j) or cutoffs is NULL"),
                                    (dict(first_seen=OI, n_items=0), "first_seen needs n_items >= 1"),
                                    (dict(p=P_FROM_1, cutoffs=I32(3, 1)), CUT_MSG)],
    "list_metrics": CUTS + [(dict(valid=None), "every output is NULL"), (dict(pred=None, n_users=-1), "predictions or cutoffs is NULL"),
                            (dict(n_items=0), "n_items < 1"), (dict(count_sum=OI, item_count=None), "count_sum / popularity need item_count"),
                            (dict(novelty=OD, item_info=None), "info_sum / novelty need item_info"),
                            (dict(item_count=I32(1, 1, -1, 1, 1)), "item_count holds a negative value"),
                            (dict(item_info=np.array([0, 0, 2 ** 40, 0, 0], np.int64)), "item_info must lie in 0 <= v < 2^40"),
                            (dict(item_count=I32(1, 1, -1, 1, 1), cutoffs=I32(3, 1)), CUT_MSG)],
    "list_diversity": DIVERSITY,
    "list_diversity_f64": DIVERSITY,
    "mmr_rerank": MMR,
    "mmr_rerank_f64": MMR,
    "held_out_ranks": ACTUAL + [(dict(rank=257), "rank > 256 is not on the device path", UNSUPPORTED),
                                (dict(p=None, nr=-1), "bad dimensions (n_users < 0, n_items < 0 or rank < 1)"),
                                (dict(p=None, n_exclude=1), "NULL matrix or actual (p, j)"), (dict(n_exclude=1), "bad exclude"),
                                (dict(above=None, tied=None, n_adm=None), "every output is NULL"),
                                (dict(mpr=OD, ax=None), "mpr and sums need the weights: actual_x is NULL"),
                                (dict(sums=OD, ax=None, p=P_FROM_1), "mpr and sums need the weights: actual_x is NULL")],
    "sparse_approximation": [(dict(sparse_matrix_type=3), "sparse_matrix_type should be CSC = 1 or CSR = 2"),
                             (dict(sparse_matrix_type=0, p=None), "sparse_matrix_type should be CSC = 1 or CSR = 2"),
                             (dict(rank=257), "rank > 256 is not on the device path", UNSUPPORTED),
                             (dict(rank=0), "bad dimensions (n_rows < 0, n_cols < 0 or rank < 1)"), (dict(p=None), "p, X or Y is NULL"),
                             (dict(p=P_FROM_1), "p[0] != 0"), (dict(p=P_DOWN), "p decreases"), (dict(idx=J_OUT), "an index is outside the matrix"),
                             (dict(idx=None), "the indices or values_out is NULL"),
                             (dict(sparse_matrix_type=1, n_rows=4, n_cols=2), "an index is outside the matrix")],   # CSC: rows are inner
    "sample_negatives": SAMPLE,
    "sample_negatives_weighted": SAMPLE + [(dict(w=None, seen_p=P_FROM_1), "w is NULL"), (dict(w=np.array([1, 0, 1, 1, 1], np.uint32)), WEIGHT_MSG),
                                           (dict(w=None, n=8193), "n > 8192 (RSPARSE_HIP_MAX_NEGATIVES) is not on the device path", UNSUPPORTED)],
    "split_rows": [(dict(mode=2), "mode is neither RSPARSE_HIP_SPLIT_PROPORTION nor RSPARSE_HIP_SPLIT_LEAVE_OUT"),
                   (dict(p=None, n_rows=-1), "bad dimensions (n_rows < 0, row0 < 0 or a negative capacity)"),
                   (dict(p=None, mode=2), "p, j, train_p or test_p is NULL"), (dict(by=X), "`by` has no meaning in proportion mode"),
                   (dict(value_bytes=2), "value_bytes must be 0, 4 or 8"), (dict(p=P_FROM_1), "p[0] != 0"), (dict(p=P_DOWN, j=J_UP), "p decreases"),
                   (dict(j=J_DOWN), "an index is negative, or a row's indices are not strictly ascending"),
                   (dict(j=J_NEG), "an index is negative, or a row's indices are not strictly ascending"),
                   (dict(mode=1, by=NAN), "NaN in `by`"), (dict(mode=1, by=NAN, j=J_DOWN), "an index is negative, or a row's indices are not strictly ascending")],
    "confidence": [(dict(kind=99), "unknown confidence kind 99"), (dict(p=None, n_rows=-1), "bad dimensions (n_rows < 0 or n_cols < 0)"),
                   (dict(p=None, kind=-1), "unknown confidence kind -1"), (dict(p=None), "p is NULL"), (dict(kind=4, norm=3), "norm must be 1 or 2"),
                   (dict(kind=1, b=0.0), "eps must not be 0"), (dict(p=P_FROM_1), "p[0] != 0"), (dict(p=P_DOWN), "p decreases"),
                   (dict(j=None), "j, x or out is NULL"), (dict(j=J_OUT), "a column index outside [0, n_cols)"),
                   (dict(j=J_NEG, p=P_FROM_1), "p[0] != 0")],
    "events_to_csr": [(dict(aggregate=9), "unknown aggregate 9"), (dict(aggregate=3), "the aggregate `last` needs timestamps"),
                      (dict(half_life=1.0), "a half life needs timestamps"),
                      (dict(half_life=1.0, aggregate=1, timestamps=X), "a half life goes with the aggregate `sum` only"),
                      (dict(n_events=2 ** 31), "n_events >= 2^31: cut the log into several calls"),
                      (dict(p=None, n_events=-1), "bad dimensions (n_events < 0, n_users < 0, n_items < 0 or capacity < 0)"),
                      (dict(p=None, aggregate=9), "p or n_cells is NULL"), (dict(users=None), "users, items, j or x is NULL"),
                      (dict(values=NAN), "NaN in values or timestamps"), (dict(timestamps=NAN, aggregate=9), "unknown aggregate 9")],
}


def test_every_host_form_is_covered():
    assert set(CASES) == set(DEFAULTS) and len(CASES) == 17
    for name in CASES:
        assert len(_lib.SIGNATURES["rsparse_hip_" + name][1]) == len(DEFAULTS[name]), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_rejected_calls_say_exactly_this(name):
    lib = _lib.load()
    for over, msg, *code in CASES[name]:
        assert _call(name, **over) == (code[0] if code else INVALID), (name, over)
        assert lib.rsparse_hip_last_error().decode() == msg, (name, over)


def test_what_an_early_return_writes():
    full = lambda n, v, t=np.int32: np.full(n, v, t)
    # hit_metrics: first_seen is initialised before the n_users == 0 return, and not before the checks of the matrix have passed
    seen = full(5, 7)
    assert _call("hit_metrics", p=P_DOWN, j=J_UP, first_seen=seen) == INVALID and (seen == 7).all()
    assert _call("hit_metrics", n_users=0, first_seen=seen) == _lib.OK and (seen == np.iinfo(np.int32).max).all()
    # list_metrics: exposure zeroed
    expo = full(10, 7)
    assert _call("list_metrics", n_users=0, exposure=expo) == _lib.OK and (expo == 0).all()
    # the samplers: the sizes-only call fills out_p; the weighted one has *filled_rows = 0 once the weights have passed
    out_p, filled = full(3, 7), full(1, 7, np.int64)
    assert _call("sample_negatives", out_p=out_p, out_j=None, out_capacity=0) == _lib.OK and out_p.tolist() == [0, 2, 4]
    assert _call("sample_negatives_weighted", w=None, filled_rows=filled) == INVALID and filled[0] == 7
    assert _call("sample_negatives_weighted", seen_p=P_FROM_1, filled_rows=filled) == INVALID and filled[0] == 0
    out_p[:] = 7
    assert _call("sample_negatives_weighted", out_p=out_p, out_j=None, out_capacity=0) == _lib.OK and out_p.tolist() == [0, 2, 4]
    # split_rows: train_p[0] = test_p[0] = 0 once the matrix has passed, nothing before
    trp, tep = full(3, 7), full(3, 7)
    assert _call("split_rows", p=P_DOWN, j=J_UP, train_p=trp, test_p=tep) == INVALID and trp[0] == 7 and tep[0] == 7
    assert _call("split_rows", n_rows=0, train_p=trp, test_p=tep) == _lib.OK and trp[0] == 0 and tep[0] == 0
    # events_to_csr: *n_cells = 0 and the row pointers of an empty log, after the checks
    cells, p = ctypes.c_int64(5), full(3, 7)
    assert _call("events_to_csr", values=NAN, n_cells=cells) == INVALID and cells.value == 5
    assert _call("events_to_csr", n_events=0, p=p, n_cells=cells) == _lib.OK and cells.value == 0 and (p == 0).all()
    # the other no-ops
    assert _call("similar_items", n_q=0) == _lib.OK and _call("ranking_metrics", n_users=0) == _lib.OK
    assert _call("confidence", p=I32(0, 0, 0), j=None) == _lib.OK and _call("sparse_approximation", p=I32(0, 0, 0), idx=None) == _lib.OK
    assert _call("held_out_ranks", nr=0) == _lib.OK and _call("list_diversity", n_users=0) == _lib.OK and _call("mmr_rerank_f64", n_users=0) == _lib.OK
