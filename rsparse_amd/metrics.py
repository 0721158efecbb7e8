"""Ranking metrics of top-k lists -- the reference's exported `ap_k()` / `ndcg_k()` (R/metrics.R:31-127), computed on the device
(wrmf_metrics.hip behind `rsparse_hip_ranking_metrics`).

    ap_k(predictions, actual)     average precision at k, per row
    ndcg_k(predictions, actual)   normalised discounted cumulative gain at k, per row

`predictions` is an integer n x k array of 0-based item indices with -1 where a list is short -- what `WRMF.predict` returns (a
`TopItems` is taken as is); `actual` any scipy sparse matrix with n rows whose stored entries are the relevant items and their
relevances.  The reference's semantics, not the textbook ones: with kk = min(k, stored entries of the row), ap is the mean over
positions 1..kk of (hits so far) / position, ndcg is dcg / idcg over the first kk positions; every position is looked up on its
own (missing, out-of-range and repeated predictions like `%in%` / `match`), stored zeros are relevant items of relevance 0.
An empty row gives ap = NaN and ndcg = 0; a row of zero relevances ndcg = NaN.  `WRMF.evaluate` scores the lists of `predict`
without moving them off the device.

Hit-based metrics, which the reference does not have, at up to 16 cutoffs from ONE pass over the lists (wrmf_hits.hip behind
`rsparse_hip_hit_metrics`; `WRMF.evaluate(k=(5, 10, 20), metrics=("hit", "recall", ...))` runs it on the lists of `predict`):

    hit_metrics_reference(predictions, actual, cutoffs, n_item)   the DEFINITION, plain numpy: the kernel equals it bit for bit
    topk_metrics(predictions, actual, cutoffs, metrics)           the same on the device, {name: (n, T) array}
    precision_k / recall_k / hit_rate_k / mrr_k / coverage_k      one metric; a vector for one cutoff, (n, T) for several
    summarize(ev)                                                 the means per cutoff of what `WRMF.evaluate` returns

Beyond-accuracy metrics of the same lists at the same cutoffs (wrmf_lists.hip and wrmf_diversity.hip behind
`rsparse_hip_list_metrics` / `rsparse_hip_list_diversity`; `WRMF.evaluate(metrics=("popularity", "novelty", "diversity", "gini",
"entropy"))` runs them on the lists of `predict`):

    list_metrics_reference(predictions, cutoffs, n_item, item_count, item_info)   the DEFINITION, integers only: bit for bit
    list_diversity_reference(predictions, cutoffs, item_factors, c0, c1)          the DEFINITION of the intra-list distance
    self_information(item_count)                                                  -log2 of the smoothed item shares, fixed point
    exposure_summary(exposure)                                                    Gini index and entropy of the exposure counts
    list_metrics(...) / list_diversity(...)                                       the same on the device

MMR re-ranking of a pool of ranked items per row down to k (wrmf_mmr.hip behind `rsparse_hip_mmr_rerank`;
`WRMF.predict(diversify=)` / `WRMF.evaluate(diversify=)` run it on the pools of `predict`):

    mmr_reference(predictions, scores, k, trade_off, item_factors, c0, c1)        the DEFINITION of the greedy re-ranking
    mmr_rerank(...)                                                               the same on the device

Full-ranking metrics (`WRMF.held_out_ranks` / `WRMF.evaluate_ranks` compute them on the device, wrmf_ranks.hip) have their
plain-numpy statement here, from a dense score matrix -- the reference the tests hold the kernels to, usable on its own:

    percentile_ranks(scores, actual, not_recommend, items_exclude)   per held-out entry: items above / tied, per row: n_adm
    rank_summary(above, tied, n_adm, actual)                         per row: mpr, auc, mrr and the sums behind the totals
    rank_totals(summary)                                             the data-set numbers {"mpr", "auc", "mrr", "n"}
"""
import ctypes

import numpy as np
import scipy.sparse as sp

from . import _lib

NA_INTEGER = -2147483648   # RSPARSE_HIP_NA_INTEGER


def canonical_actual(actual, n_rows):
    """`as(actual, "RsparseMatrix")`: CSR with sorted column indices and duplicates summed, stored zeros kept.  A row-count
    mismatch raises ValueError (stopifnot(n_u == nrow(actual)))."""
    if not sp.issparse(actual):
        raise TypeError("actual must be a scipy sparse matrix")
    if actual.shape[0] != n_rows:
        raise ValueError("n_u == nrow(actual) is not TRUE: %d rows of predictions, %d of actual" % (n_rows, actual.shape[0]))
    a = sp.csr_matrix(actual, dtype=np.float64, copy=True)
    a.sum_duplicates()   # (sorts the indices too; explicit zeros stay)
    return a


def _one_based(predictions):
    """0-based indices with -1 for NA -> R's 1-based integers with NA_integer_ (anything negative or past int32 is a miss
    either way: it maps to NA)"""
    p = np.asarray(predictions)
    if p.ndim != 2:
        raise ValueError("predictions must be a matrix (n x k)")
    if not np.issubdtype(p.dtype, np.integer):
        raise TypeError("predictions must hold integer item indices")
    p = p.astype(np.int64, copy=False)
    ok = (p >= 0) & (p < np.iinfo(np.int32).max)
    return np.where(ok, p + 1, NA_INTEGER).astype(np.int32)


def ranking_metrics(predictions, actual, ap=True, ndcg=True):
    """(ap, ndcg) per row, float64 vectors (None for a metric not asked for)."""
    pred = _one_based(predictions)
    n, k = pred.shape
    a = canonical_actual(actual, n)
    if k < 1:
        raise ValueError("predictions must have at least one column")
    pred = np.asfortranarray(pred)   # R's integer matrix: column-major
    p = np.ascontiguousarray(a.indptr, dtype=np.int32)
    j = np.ascontiguousarray(a.indices, dtype=np.int32)
    x = np.ascontiguousarray(a.data, dtype=np.float64)
    if j.size == 0:   # (no stored entry at all: the library still wants non-NULL slots)
        j, x = np.zeros(1, np.int32), np.zeros(1, np.float64)
    ap_out = np.empty(n, dtype=np.float64) if ap else None
    ndcg_out = np.empty(n, dtype=np.float64) if ndcg else None
    if n == 0:
        return ap_out, ndcg_out
    vp = lambda arr: None if arr is None else arr.ctypes.data_as(ctypes.c_void_p)
    _lib.check(_lib.load().rsparse_hip_ranking_metrics(vp(pred), n, k, vp(p), vp(j), vp(x) if ndcg else None, vp(ap_out),
                                                       vp(ndcg_out)))
    return ap_out, ndcg_out


def ap_k(predictions, actual):
    """R/metrics.R:31-57: average precision at k of every row of `predictions` against the same row of `actual`."""
    return ranking_metrics(predictions, actual, ap=True, ndcg=False)[0]


def ndcg_k(predictions, actual):
    """R/metrics.R:62-89: normalised discounted cumulative gain at k of every row, relevances from the values of `actual`."""
    return ranking_metrics(predictions, actual, ap=False, ndcg=True)[1]


# ---- hit-based metrics at several cutoffs: the numpy statement of DESIGN.md 3.21 and the device call -------------------------
HIT_METRICS = ("precision", "recall", "hit", "mrr")
MAX_CUTOFFS = _lib.MAX_CUTOFFS
MAX_TOPK = 8192   # RSPARSE_HIP_MAX_TOPK_LARGE
NEVER_SEEN = np.iinfo(np.int32).max   # first_seen of an item that no list names


def check_cutoffs(cutoffs, k=None):
    """`cutoffs` as a tuple of ints: strictly ascending, at least 1, at most k (where given) -- anything else is a ValueError;
    more than MAX_CUTOFFS of them are not on the device path"""
    cut = [cutoffs] if isinstance(cutoffs, (int, np.integer)) and not isinstance(cutoffs, bool) else list(cutoffs)
    if not cut or any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) for c in cut):
        raise ValueError("cutoffs must be one or more integers")
    cut = tuple(int(c) for c in cut)
    if cut[0] < 1 or any(b <= a for a, b in zip(cut, cut[1:])):
        raise ValueError("cutoffs must be strictly ascending and at least 1")
    if k is not None and cut[-1] > k:
        raise ValueError("a cutoff is larger than the lists are long (k = %d)" % k)
    if len(cut) > MAX_CUTOFFS:
        raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "more than %d cutoffs are not on the device path" % MAX_CUTOFFS)
    return cut


def coverage_from_first_seen(first_seen, cutoffs):
    """#{items with first_seen <= c_t} / n_item for every cutoff: float64 (T,)"""
    fs = np.asarray(first_seen)
    return np.array([np.count_nonzero(fs <= c) for c in cutoffs], dtype=np.int64) / np.int64(fs.size)


def hit_metrics_reference(predictions, actual, cutoffs, n_item=None):
    """The DEFINITION of the hit-based metrics, pure numpy, no device.  `predictions` n x k 0-based with -1 where a list is
    short, `actual` sparse with n rows (made canonical), `cutoffs` strictly ascending 1 <= c_1 < ... < c_T <= k.  Per row u with
    n_u stored entries, hit_i = the prediction at the 1-based position i is a stored column of the row (each position on its
    own: negative and out-of-range predictions miss, a repeated index hits every time, a stored zero is relevant):
        hits[u, t] = sum_{i <= c_t} hit_i (int32)          first[u] = the smallest i <= c_T with hit_i, 0 without one (int32)
        precision  = hits / c_t       recall = hits / n_u       hit = 1.0 where hits > 0       mrr = 1 / first where 0 < first <= c_t
    and NaN in the four of a row with n_u = 0.  With `n_item`, over ALL rows: first_seen[item] = the smallest position i <= c_T
    at which a row lists the item (int32, NEVER_SEEN without one; only items in 0 .. n_item - 1 count) and coverage[t] =
    #{first_seen <= c_t} / n_item.  Every double is one division of two integers."""
    p = np.asarray(predictions)
    if p.ndim != 2:
        raise ValueError("predictions must be a matrix (n x k)")
    if not np.issubdtype(p.dtype, np.integer):
        raise TypeError("predictions must hold integer item indices")
    p = p.astype(np.int64, copy=False)
    n, k = p.shape
    a = canonical_actual(actual, n)
    cut = np.asarray(check_cutoffs(cutoffs, k), dtype=np.int64)
    T, c_last = cut.size, int(cut[-1])
    hits = np.zeros((n, T), dtype=np.int32)
    first = np.zeros(n, dtype=np.int32)
    n_u = np.diff(a.indptr).astype(np.int64)
    for u in range(n):
        h = np.isin(p[u, :c_last], a.indices[a.indptr[u]:a.indptr[u + 1]])
        cum = np.concatenate([[0], np.cumsum(h)])
        hits[u] = cum[cut]
        if h.any():
            first[u] = int(np.argmax(h)) + 1
    empty = n_u == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        precision = hits.astype(np.float64) / cut.astype(np.float64)[None, :]
        recall = hits.astype(np.float64) / n_u.astype(np.float64)[:, None]
        mrr = np.where((first[:, None] > 0) & (first[:, None] <= cut[None, :]), 1.0 / first.astype(np.float64)[:, None], 0.0)
    hit = (hits > 0).astype(np.float64)
    for v in (precision, recall, hit, mrr):
        v[empty] = np.nan
    out = {"hits": hits, "first": first, "precision": precision, "recall": recall, "hit": hit, "mrr": mrr}
    if n_item is not None:
        n_item = int(n_item)
        if n_item < 1:
            raise ValueError("n_item must be at least 1")
        first_seen = np.full(n_item, NEVER_SEEN, dtype=np.int32)
        head = p[:, :c_last]
        ok = (head >= 0) & (head < n_item)
        pos = np.broadcast_to(np.arange(1, c_last + 1, dtype=np.int32), head.shape)
        np.minimum.at(first_seen, head[ok], pos[ok])
        out["first_seen"] = first_seen
        out["coverage"] = coverage_from_first_seen(first_seen, cut)
    return out


def topk_metrics(predictions, actual, cutoffs, metrics=HIT_METRICS, n_item=None):
    """The hit-based metrics of `hit_metrics_reference`, computed on the device in one pass over the lists (wrmf_hits.hip behind
    `rsparse_hip_hit_metrics`) and equal to it bit for bit.  `metrics` names some of "hits", "first", "precision", "recall",
    "hit", "mrr" and "coverage"; -> {name: array}: (n, T) per cutoff (first: n; coverage: (T,), with "first_seen" beside it).
    Coverage counts the items of 0 .. n_item - 1 (default: the columns of `actual`).  k <= 8192, at most 16 cutoffs."""
    names = tuple(metrics)
    known = ("hits", "first") + HIT_METRICS + ("coverage",)
    if not names or any(m not in known for m in names):
        raise ValueError("metrics must name some of %s" % ", ".join(repr(m) for m in known))
    pred = _one_based(predictions)
    n, k = pred.shape
    a = canonical_actual(actual, n)
    if k < 1:
        raise ValueError("predictions must have at least one column")
    cut = np.asarray(check_cutoffs(cutoffs, k), dtype=np.int32)
    T = cut.size
    if k > MAX_TOPK:
        raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "k > %d is not on the device path" % MAX_TOPK)
    out = {m: np.empty((n, T), dtype=np.int32 if m == "hits" else np.float64, order="F") for m in names
           if m not in ("first", "coverage")}
    if "first" in names:
        out["first"] = np.empty(n, dtype=np.int32)
    first_seen = None
    if "coverage" in names:
        n_item = a.shape[1] if n_item is None else int(n_item)
        if n_item < 1:
            raise ValueError("n_item must be at least 1")
        first_seen = np.full(n_item, NEVER_SEEN, dtype=np.int32)
    if n > 0:
        pred = np.asfortranarray(pred)   # R's integer matrix: column-major
        p = np.ascontiguousarray(a.indptr, dtype=np.int32)
        j = np.ascontiguousarray(a.indices, dtype=np.int32)
        if j.size == 0:   # (no stored entry at all: the library still wants a non-NULL slot)
            j = np.zeros(1, np.int32)
        vp = lambda arr: None if arr is None else arr.ctypes.data_as(ctypes.c_void_p)
        _lib.check(_lib.load().rsparse_hip_hit_metrics(vp(pred), n, k, vp(p), vp(j), vp(cut), T, vp(out.get("hits")),
                                                       vp(out.get("first")), vp(out.get("precision")), vp(out.get("recall")),
                                                       vp(out.get("hit")), vp(out.get("mrr")), vp(first_seen),
                                                       0 if first_seen is None else first_seen.size))
    if first_seen is not None:
        out["first_seen"] = first_seen
        out["coverage"] = coverage_from_first_seen(first_seen, cut)
    return {m: (np.ascontiguousarray(v) if v.ndim == 2 else v) for m, v in out.items()}


def _one_metric(name, predictions, actual, cutoffs):
    k = np.asarray(predictions).shape[-1]
    scalar = cutoffs is None or (isinstance(cutoffs, (int, np.integer)) and not isinstance(cutoffs, bool))
    v = topk_metrics(predictions, actual, k if cutoffs is None else cutoffs, metrics=(name,))[name]
    return v[:, 0] if scalar else v


def precision_k(predictions, actual, cutoffs=None):
    """hits among the first c predictions / c, per row: a float64 vector of n for one cutoff (default: k, the width of
    `predictions`), (n, T) for a sequence; NaN for a row of `actual` without a stored entry"""
    return _one_metric("precision", predictions, actual, cutoffs)


def recall_k(predictions, actual, cutoffs=None):
    """hits among the first c predictions / stored entries of the row; shapes and NaN as `precision_k`"""
    return _one_metric("recall", predictions, actual, cutoffs)


def hit_rate_k(predictions, actual, cutoffs=None):
    """1.0 where any of the first c predictions is a stored entry of the row, else 0.0; shapes and NaN as `precision_k`"""
    return _one_metric("hit", predictions, actual, cutoffs)


def mrr_k(predictions, actual, cutoffs=None):
    """1 / (position of the first hit) where it lies within the first c predictions, else 0.0; shapes and NaN as `precision_k`"""
    return _one_metric("mrr", predictions, actual, cutoffs)


def coverage_k(predictions, n_item, cutoffs=None):
    """the share of the items 0 .. n_item - 1 that some row names among its first c predictions: a float for one cutoff
    (default: k), a float64 (T,) vector for a sequence"""
    p = np.asarray(predictions)
    if p.ndim != 2:
        raise ValueError("predictions must be a matrix (n x k)")
    scalar = cutoffs is None or (isinstance(cutoffs, (int, np.integer)) and not isinstance(cutoffs, bool))
    nothing = sp.csr_matrix((p.shape[0], int(n_item)), dtype=np.float64)
    v = topk_metrics(p, nothing, p.shape[1] if cutoffs is None else cutoffs, metrics=("coverage",), n_item=n_item)["coverage"]
    return float(v[0]) if scalar else v


def summarize(ev):
    """The data-set numbers of a dict returned by `WRMF.evaluate`: for every per-row metric the mean over the rows where it is
    defined (NaN rows -- users with nothing held out -- left out; NaN when no row is defined), per cutoff: a float for a vector
    of n, a (T,) vector for an (n, T) array.  "coverage", "gini" and "entropy" are data-set numbers already and are passed
    through."""
    out = {}
    for name, v in ev.items():
        if name in ("coverage", "gini", "entropy"):
            out[name] = v
            continue
        v = np.asarray(v, dtype=np.float64)
        ok = ~np.isnan(v)
        cnt = ok.sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            m = np.where(ok, v, 0.0).sum(axis=0) / cnt
        out[name] = float(m) if np.ndim(m) == 0 else m
    return out


# ---- beyond-accuracy metrics: the numpy statement of DESIGN.md 3.23 and the device calls -------------------------------------
LIST_METRICS = ("popularity", "novelty")
EXPOSURE_METRICS = ("gini", "entropy")
MAX_RANK = 256          # RSPARSE_HIP_MAX_RANK: latent coordinates of list_diversity
INFO_LIMIT = 1 << 40    # item_info: fixed point in units of 2^-32, 0 <= v < 2^40 (a sum over 8192 positions stays below 2^53)


def _lists(predictions):
    p = np.asarray(predictions)
    if p.ndim != 2:
        raise ValueError("predictions must be a matrix (n x k)")
    if not np.issubdtype(p.dtype, np.integer):
        raise TypeError("predictions must hold integer item indices")
    return p.astype(np.int64, copy=False)


def _tables(n_item, item_count, item_info):
    """the two item tables checked: int32 counts >= 0 and int64 fixed-point values in [0, 2^40), n_item of each (or None)"""
    n_item = int(n_item)
    if n_item < 1:
        raise ValueError("n_item must be at least 1")
    if item_count is not None:
        c = np.asarray(item_count)
        if c.ndim != 1 or c.size != n_item or not np.issubdtype(c.dtype, np.integer):
            raise ValueError("item_count must be an integer vector of n_item")
        if c.size and (c.min() < 0 or c.max() > np.iinfo(np.int32).max):
            raise ValueError("item_count must lie in 0 .. 2^31 - 1")
        item_count = np.ascontiguousarray(c, dtype=np.int32)
    if item_info is not None:
        v = np.asarray(item_info)
        if v.ndim != 1 or v.size != n_item or not np.issubdtype(v.dtype, np.integer):
            raise ValueError("item_info must be an integer vector of n_item (fixed point in units of 2^-32)")
        if v.size and (v.min() < 0 or v.max() >= INFO_LIMIT):
            raise ValueError("item_info must lie in 0 <= v < 2^40")
        item_info = np.ascontiguousarray(v, dtype=np.int64)
    return n_item, item_count, item_info


def self_information(item_count):
    """rint(-log2((cnt_j + 1) / (sum cnt + n_item)) 2^32) as int64: the self-information in bits of the Laplace-smoothed share
    of interactions of every item, in the fixed point `list_metrics_reference` takes as `item_info`.  Never infinite, at least 0,
    and below 2^40 for any int32 counts (the share is at least 1 / (n_item 2^31 + n_item) > 2^-63)."""
    c = np.asarray(item_count)
    if c.ndim != 1 or c.size < 1 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError("item_count must be a non-empty integer vector")
    c = c.astype(np.int64)
    if c.min() < 0:
        raise ValueError("item_count must not be negative")
    total = int(c.sum()) + int(c.size)
    bits = -np.log2((c + 1).astype(np.float64) / np.float64(total))
    return np.rint(np.maximum(bits, 0.0) * 4294967296.0).astype(np.int64)


def exposure_summary(exposure):
    """How evenly the lists expose the catalogue, per cutoff, from the integer histogram exposure[t, item] (T x n_item, or one
    row): {"gini": (T,), "entropy": (T,)}.  Gini = sum_i (2 i - n - 1) e_(i) / (n sum e) over the ascending counts e_(1) <= ... <=
    e_(n) (0 = every item shown equally often, -> 1 = one item takes everything): numerator and denominator are exact Python
    integers, one division.  Entropy = the Shannon entropy in bits of e / sum e.  NaN where a cutoff's total is 0."""
    e = np.atleast_2d(np.asarray(exposure))
    if e.ndim != 2 or not np.issubdtype(e.dtype, np.integer):
        raise ValueError("exposure must be an integer (T, n_item) array")
    T, n = e.shape
    gini, ent = np.full(T, np.nan), np.full(T, np.nan)
    for t in range(T):
        row = np.sort(e[t].astype(np.int64))
        tot = int(row.sum())
        if tot <= 0:
            continue
        w = 2 * np.arange(1, n + 1, dtype=np.int64) - n - 1
        if n * float(row[-1]) * n < 2.0 ** 62:
            num = int(np.dot(w, row))
        else:
            num = sum(int(a) * int(b) for a, b in zip(w.tolist(), row.tolist()))
        gini[t] = num / (n * tot)
        q = row[row > 0].astype(np.float64) / np.float64(tot)
        ent[t] = float(-(q * np.log2(q)).sum()) + 0.0
    return {"gini": gini, "entropy": ent}


def list_metrics_reference(predictions, cutoffs, n_item, item_count=None, item_info=None):
    """The DEFINITION of the popularity, novelty and exposure metrics, integers only, no device.  `predictions` n x k 0-based
    with -1 where a list is short; `cutoffs` strictly ascending within 1 .. k.  A position is VALID when its item lies in
    0 .. n_item - 1 (anything else is skipped; a repeated item counts wherever it stands).  Per row u and cutoff c_t:
        valid[u, t] (int32) = the valid positions i <= c_t
        count_sum[u, t] (int64) = sum of item_count[item_i] over them       popularity = double(count_sum) / double(valid)
        info_sum[u, t] (int64) = sum of item_info[item_i] over them         novelty = double(info_sum) / double(valid 2^32)
    (NaN where valid = 0; what needs a table that is None is left out), and over ALL rows exposure[t, item] (int32) = the valid
    positions i <= c_t that name the item.  `item_count`: int32 >= 0; `item_info`: int64 fixed point in units of 2^-32,
    0 <= v < 2^40 (`self_information`).  Every double is one division of two exactly converted integers."""
    p = _lists(predictions)
    n, k = p.shape
    cut = np.asarray(check_cutoffs(cutoffs, k), dtype=np.int64)
    n_item, item_count, item_info = _tables(n_item, item_count, item_info)
    T, c_last = cut.size, int(cut[-1])
    head = p[:, :c_last]
    ok = (head >= 0) & (head < n_item)
    safe = np.where(ok, head, 0)
    zero = np.zeros((n, 1), dtype=np.int64)

    def at_cutoffs(per_position):
        return np.concatenate([zero, np.cumsum(per_position, axis=1, dtype=np.int64)], axis=1)[:, cut]
    valid = at_cutoffs(ok).astype(np.int32)
    out = {"valid": valid}
    vd = valid.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if item_count is not None:
            out["count_sum"] = at_cutoffs(np.where(ok, item_count.astype(np.int64)[safe], 0))
            out["popularity"] = np.where(valid > 0, out["count_sum"].astype(np.float64) / vd, np.nan)
        if item_info is not None:
            out["info_sum"] = at_cutoffs(np.where(ok, item_info[safe], 0))
            out["novelty"] = np.where(valid > 0, out["info_sum"].astype(np.float64) / (vd * 4294967296.0), np.nan)
    exposure = np.zeros((T, n_item), dtype=np.int32)
    for t in range(T):
        m = ok[:, :cut[t]]
        exposure[t] = np.bincount(head[:, :cut[t]][m], minlength=n_item).astype(np.int32)
    out["exposure"] = exposure
    return out


def _unit_rows(item_factors, c0, c1):
    """(unit rows in float64, degenerate flags) of the columns [c0, c1) of a factor matrix: the rule of `similar_items`"""
    V = np.asarray(item_factors)
    if V.ndim != 2 or V.dtype not in (np.float32, np.float64):
        raise ValueError("item_factors must be a float32 or float64 matrix (n_item x rank)")
    c1 = V.shape[1] if c1 is None else int(c1)
    c0 = int(c0)
    if not 0 <= c0 < c1 <= V.shape[1]:
        raise ValueError("c0 / c1 must satisfy 0 <= c0 < c1 <= columns of item_factors")
    W = V[:, c0:c1].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        ss = (W * W).sum(axis=1)
    bad = ~((ss > 0) & np.isfinite(ss))
    with np.errstate(divide="ignore", invalid="ignore"):
        unit = np.where(bad[:, None], 0.0, W / np.sqrt(np.where(bad, 1.0, ss))[:, None])
    return unit, bad, c0, c1


def list_diversity_reference(predictions, cutoffs, item_factors, c0=0, c1=None):
    """The DEFINITION of the intra-list diversity, float64, no device.  u_j = V[j, c0:c1] / |V[j, c0:c1]| in float64 from the
    factors as stored; an item whose sum of squares is 0 or not finite is DEGENERATE and its positions are skipped like invalid
    ones (items outside 0 .. n_item - 1).  Per row u and cutoff c_t:
        counted[u, t] (int32) = the valid, non-degenerate positions i <= c_t
        diversity[u, t] = the mean over the pairs i < j of those positions of 1 - <u_i, u_j>      NaN where counted < 2
    the pairwise form, O(k^2 r) per row.  -> {"counted", "diversity"}, (n, T) each."""
    p = _lists(predictions)
    n, k = p.shape
    cut = np.asarray(check_cutoffs(cutoffs, k), dtype=np.int64)
    unit, bad, _, _ = _unit_rows(item_factors, c0, c1)
    n_item = unit.shape[0]
    T = cut.size
    counted = np.zeros((n, T), dtype=np.int32)
    div = np.full((n, T), np.nan)
    for u in range(n):
        for t in range(T):
            it = p[u, :cut[t]]
            it = it[(it >= 0) & (it < n_item)]
            it = it[~bad[it]]
            m = int(it.size)
            counted[u, t] = m
            if m >= 2:
                G = unit[it] @ unit[it].T
                iu = np.triu_indices(m, 1)
                div[u, t] = float(np.mean(1.0 - G[iu]))
    return {"counted": counted, "diversity": div}


def list_metrics(predictions, cutoffs, n_item, item_count=None, item_info=None,
                 metrics=("valid", "count_sum", "info_sum", "popularity", "novelty", "exposure")):
    """`list_metrics_reference` on the device, one pass over the lists (wrmf_lists.hip behind `rsparse_hip_list_metrics`), equal
    to it bit for bit.  `metrics` names some of "valid", "count_sum", "info_sum", "popularity", "novelty", "exposure"; names
    that need a table that is None are left out, as the definition leaves them out.  -> {name: (n, T) array}; exposure (T, n_item)
    int32.  k <= 8192, at most 16 cutoffs."""
    known = ("valid", "count_sum", "info_sum", "popularity", "novelty", "exposure")
    names = tuple(metrics)
    if not names or any(m not in known for m in names):
        raise ValueError("metrics must name some of %s" % ", ".join(repr(m) for m in known))
    pred = _one_based(predictions)
    n, k = pred.shape
    if k < 1:
        raise ValueError("predictions must have at least one column")
    cut = np.asarray(check_cutoffs(cutoffs, k), dtype=np.int32)
    n_item, item_count, item_info = _tables(n_item, item_count, item_info)
    names = tuple(m for m in names if not (m in ("count_sum", "popularity") and item_count is None)
                  and not (m in ("info_sum", "novelty") and item_info is None))
    if not names:
        raise ValueError("every metric asked for needs a table that was not given")
    T = cut.size
    if k > MAX_TOPK:
        raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "k > %d is not on the device path" % MAX_TOPK)
    dt = {"valid": np.int32, "count_sum": np.int64, "info_sum": np.int64, "exposure": np.int32}
    out = {m: np.empty((n_item, T) if m == "exposure" else (n, T), dtype=dt.get(m, np.float64), order="F") for m in names}
    pred = np.asfortranarray(pred)   # R's integer matrix: column-major
    vp = lambda arr: None if arr is None else arr.ctypes.data_as(ctypes.c_void_p)
    _lib.check(_lib.load().rsparse_hip_list_metrics(vp(pred), n, k, vp(cut), T, vp(item_count), vp(item_info), n_item,
                                                    vp(out.get("valid")), vp(out.get("count_sum")), vp(out.get("info_sum")),
                                                    vp(out.get("popularity")), vp(out.get("novelty")), vp(out.get("exposure"))))
    return {m: np.ascontiguousarray(v.T if m == "exposure" else v) for m, v in out.items()}


def list_diversity(predictions, cutoffs, item_factors, c0=0, c1=None):
    """`list_diversity_reference` on the device (wrmf_diversity.hip behind `rsparse_hip_list_diversity`): counted exactly,
    diversity from the sum of the unit vectors, 1 - (|S|^2 - m) / (m (m - 1)), within about 2 (2 m + r) 2^-53 of the pairwise
    form.  `item_factors`: float32 or float64 (n_item x ld), used as stored; at most 256 columns in [c0, c1)."""
    pred = _one_based(predictions)
    n, k = pred.shape
    if k < 1:
        raise ValueError("predictions must have at least one column")
    cut = np.asarray(check_cutoffs(cutoffs, k), dtype=np.int32)
    V = np.asarray(item_factors)
    if V.ndim != 2 or V.dtype not in (np.float32, np.float64):
        raise ValueError("item_factors must be a float32 or float64 matrix (n_item x rank)")
    V = np.ascontiguousarray(V)
    n_item, ld = V.shape
    c1 = ld if c1 is None else int(c1)
    c0 = int(c0)
    if n_item < 1 or not 0 <= c0 < c1 <= ld:
        raise ValueError("c0 / c1 must satisfy 0 <= c0 < c1 <= columns of item_factors")
    if c1 - c0 > MAX_RANK:
        raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "more than %d latent coordinates are not on the device path" % MAX_RANK)
    if k > MAX_TOPK:
        raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "k > %d is not on the device path" % MAX_TOPK)
    T = cut.size
    counted = np.empty((n, T), dtype=np.int32, order="F")
    div = np.empty((n, T), dtype=np.float64, order="F")
    pred = np.asfortranarray(pred)
    vp = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    lib = _lib.load()
    fn = lib.rsparse_hip_list_diversity_f64 if V.dtype == np.float64 else lib.rsparse_hip_list_diversity
    _lib.check(fn(vp(pred), n, k, vp(cut), T, vp(V), n_item, ld, c0, c1, vp(counted), vp(div)))
    return {"counted": np.ascontiguousarray(counted), "diversity": np.ascontiguousarray(div)}


# ---- MMR re-ranking of the lists: the numpy statement of DESIGN.md 3.24 and the device call ---------------------------------
def check_trade_off(trade_off, what="trade_off"):
    """the MMR weight as a float in [0, 1]: anything else (NaN, a bool, not a number) is a ValueError"""
    if isinstance(trade_off, bool) or not isinstance(trade_off, (int, float, np.integer, np.floating)):
        raise ValueError("%s must be a number in [0, 1]" % what)
    t = float(trade_off)
    if not 0.0 <= t <= 1.0:   # (a NaN fails both)
        raise ValueError("%s must be a number in [0, 1]" % what)
    return t


def _mmr_args(predictions, scores, k, trade_off):
    p = _lists(predictions)
    s = np.asarray(scores)
    if s.shape != p.shape or s.dtype.kind != "f":
        raise ValueError("scores must be a floating-point matrix of the shape of predictions")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= p.shape[1]:
        raise ValueError("k must be an integer in 1 .. the width of the lists")
    return p, s.astype(np.float64), int(k), check_trade_off(trade_off)


def mmr_reference(predictions, scores, k, trade_off, item_factors, c0=0, c1=None):
    """The DEFINITION of the greedy Maximal-Marginal-Relevance re-ranking of a pool of N positions per row down to k, float64,
    no device.  `predictions` n x N 0-based (-1 where a list is short) with their `scores` (n x N); theta = `trade_off` in [0, 1].
    A position is VALID when its item lies in 0 .. n_item - 1 and its score is finite; a repeated item is a position of its own.
    inv_j = 1 / sqrt(sum of squares of V[j, c0:c1]) in float64 from the factors as stored, 0.0 for a DEGENERATE item (sum zero or
    not finite); u_j = V[j, c0:c1] inv_j, the zero vector for a degenerate item.  Per row, over its valid positions:
        rel_i = (s_i - s_min) / (s_max - s_min)                        all 0 where s_max == s_min
        step t = 0, 1, ..: pick the valid, untaken position that maximises
            (1 - theta) rel_i - theta max_{j picked} <u_i, u_j>        the max over nothing is 0; the LOWER position wins a tie
    until k are picked or no valid position is left.  -> {"items": (n, k) int64, -1 where nothing was picked, "positions":
    (n, k) int64 into the pool, -1 likewise, "objective": (n, k) float64, the maximised value of every step, NaN likewise}.
    theta = 0 returns the first k valid positions of a list sorted by score; the result for k is the k-prefix of the result for
    any larger k; two positions with bit-identical factor rows and equal scores tie exactly."""
    p, s, k, theta = _mmr_args(predictions, scores, k, trade_off)
    V = np.asarray(item_factors)
    if V.ndim != 2 or V.dtype not in (np.float32, np.float64):
        raise ValueError("item_factors must be a float32 or float64 matrix (n_item x rank)")
    c1 = V.shape[1] if c1 is None else int(c1)
    c0 = int(c0)
    if not 0 <= c0 < c1 <= V.shape[1]:
        raise ValueError("c0 / c1 must satisfy 0 <= c0 < c1 <= columns of item_factors")
    n, N = p.shape
    n_item = V.shape[0]
    items = np.full((n, k), -1, dtype=np.int64)
    positions = np.full((n, k), -1, dtype=np.int64)
    objective = np.full((n, k), np.nan)
    for u in range(n):
        ok = (p[u] >= 0) & (p[u] < n_item) & np.isfinite(s[u])
        if not ok.any():
            continue
        it = np.where(ok, p[u], 0)
        W = V[it, c0:c1].astype(np.float64)
        with np.errstate(all="ignore"):
            ss = (W * W).sum(axis=1)
            good = (ss > 0) & np.isfinite(ss)
            inv = np.where(good, 1.0 / np.sqrt(np.where(good, ss, 1.0)), 0.0)
            unit = np.where(good[:, None], W * inv[:, None], 0.0)
            s_min, s_max = s[u][ok].min(), s[u][ok].max()
            rel = np.where(ok, (s[u] - s_min) / (s_max - s_min), 0.0) if s_max != s_min else np.zeros(N)
        lead = (1.0 - theta) * rel
        free = ok.copy()
        sim = np.zeros(N)                        # the max over nothing
        for t in range(min(k, int(ok.sum()))):
            obj = np.where(free, lead - theta * sim, -np.inf)
            i = int(np.argmax(obj))              # (the first of equal maxima: the lower position)
            items[u, t], positions[u, t], objective[u, t] = p[u, i], i, obj[i]
            free[i] = False
            dots = (unit * unit[i]).sum(axis=1)   # (every row summed in the same order: equal rows give equal bits)
            sim = dots if t == 0 else np.maximum(sim, dots)
    return {"items": items, "positions": positions, "objective": objective}


def mmr_rerank(predictions, scores, k, trade_off, item_factors, c0=0, c1=None):
    """`mmr_reference` on the device (wrmf_mmr.hip behind `rsparse_hip_mmr_rerank`): one workgroup per row runs the k dependent
    steps with the dot products accumulated in double from the factors as stored.  Every pick maximises the definition's
    objective along the device's own path to within about (r + 8) 2^-53; exact ties go to the lower position.
    -> {"items", "positions" (int64, -1 where nothing was picked), "scores" (the picks' own scores), "objective" (float64, NaN
    likewise)}.  `item_factors`: float32 or float64 (n_item x ld), used as stored; N <= 8192, at most 256 columns in [c0, c1)."""
    _, s, k, theta = _mmr_args(predictions, scores, k, trade_off)
    pred = _one_based(predictions)
    n, N = pred.shape
    V = np.asarray(item_factors)
    if V.ndim != 2 or V.dtype not in (np.float32, np.float64):
        raise ValueError("item_factors must be a float32 or float64 matrix (n_item x rank)")
    V = np.ascontiguousarray(V)
    n_item, ld = V.shape
    c1 = ld if c1 is None else int(c1)
    c0 = int(c0)
    if n_item < 1 or not 0 <= c0 < c1 <= ld:
        raise ValueError("c0 / c1 must satisfy 0 <= c0 < c1 <= columns of item_factors")
    if c1 - c0 > MAX_RANK:
        raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "more than %d latent coordinates are not on the device path" % MAX_RANK)
    if N > MAX_TOPK:
        raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "a pool of more than %d is not on the device path" % MAX_TOPK)
    pred, s = np.asfortranarray(pred), np.asfortranarray(s)
    items = np.empty((n, k), dtype=np.int32, order="F")
    pos = np.empty((n, k), dtype=np.int32, order="F")
    picked = np.empty((n, k), dtype=np.float64, order="F")
    obj = np.empty((n, k), dtype=np.float64, order="F")
    vp = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    lib = _lib.load()
    fn = lib.rsparse_hip_mmr_rerank_f64 if V.dtype == np.float64 else lib.rsparse_hip_mmr_rerank
    _lib.check(fn(vp(pred), vp(s), n, N, k, theta, vp(V), n_item, ld, c0, c1, vp(items), vp(picked), vp(pos), vp(obj)))
    zero_based = lambda a: np.ascontiguousarray(np.where(a == NA_INTEGER, -1, a.astype(np.int64) - 1))
    return {"items": zero_based(items), "positions": zero_based(pos), "scores": np.ascontiguousarray(picked),
            "objective": np.ascontiguousarray(obj)}


# ---- full-ranking metrics: the numpy statement of DESIGN.md 3.15-------------------------------------------------------------
def percentile_ranks(scores, actual, not_recommend=None, items_exclude=()):
    """Where every stored entry (u, h) of `actual` stands among the ADMISSIBLE items of its row -- the items outside the row of
    `not_recommend` (sparse, n x n_item, or None) and outside `items_exclude` (0-based) --, from the dense `scores` (n x n_item):
    above = admissible items scored strictly higher, tied = other admissible items with an equal score (-0 equals +0); an entry
    that is not admissible itself gets -1 / -1.  -> (above, tied, n_adm): two scipy CSR matrices (int32) with the canonical
    pattern of `actual`, and the admissible items per row (int32)."""
    S = np.asarray(scores)
    if S.ndim != 2:
        raise ValueError("scores must be a matrix (n x n_item)")
    n, m = S.shape
    a = canonical_actual(actual, n)
    if a.shape[1] != m:
        raise ValueError("actual must have the shape of scores")
    adm = np.ones((n, m), dtype=bool)
    if not_recommend is not None:
        if not sp.issparse(not_recommend) or not_recommend.shape != (n, m):
            raise ValueError("not_recommend must be sparse and have the shape of scores")
        nr = sp.csr_matrix(not_recommend)
        adm[np.repeat(np.arange(n), np.diff(nr.indptr)), nr.indices] = False
    ex = np.asarray(list(items_exclude), dtype=np.int64)
    if ex.size:
        adm[:, ex] = False
    above = np.full(a.nnz, -1, dtype=np.int32)
    tied = np.full(a.nnz, -1, dtype=np.int32)
    for u in range(n):
        row, ok = S[u], adm[u]
        for e in range(a.indptr[u], a.indptr[u + 1]):
            h = a.indices[e]
            if ok[h]:
                above[e] = np.count_nonzero(ok & (row > row[h]))
                tied[e] = np.count_nonzero(ok & (row == row[h])) - 1
    mk = lambda v: sp.csr_matrix((v, a.indices.copy(), a.indptr.copy()), shape=a.shape)
    return mk(above), mk(tied), adm.sum(axis=1).astype(np.int32)


def rank_summary(above, tied, n_adm, actual):
    """Per row, from the counts of `percentile_ranks` (CSR matrices or flat arrays in the order of the canonical `actual`) and the
    stored values w of `actual`, over the admissible entries (P of them), with the midrank r = above + tied / 2:
        pct = r / (n_adm - 1)                                     NaN when n_adm <= 1
        mpr = sum w pct / sum w                                   NaN when sum w == 0 or P == 0 (expected percentile rank)
        auc = 1 - (sum r - P (P - 1) / 2) / (P (n_adm - P))       NaN when P == 0 or n_adm == P
        mrr = 1 / (1 + min r)                                     NaN when P == 0
    -> {"mpr", "auc", "mrr", "sum_w", "sum_w_pct", "P"}: float64 vectors of n."""
    n_adm = np.asarray(n_adm, dtype=np.int64)
    n = n_adm.size
    a = canonical_actual(actual, n)
    ab = np.asarray(above.data if sp.issparse(above) else above, dtype=np.int64)
    ti = np.asarray(tied.data if sp.issparse(tied) else tied, dtype=np.int64)
    if ab.size != a.nnz or ti.size != a.nnz:
        raise ValueError("above / tied must have one value per stored entry of actual")
    out = {k: np.full(n, np.nan) for k in ("mpr", "auc", "mrr")}
    out.update(sum_w=np.zeros(n), sum_w_pct=np.zeros(n), P=np.zeros(n))
    for u in range(n):
        sl = slice(a.indptr[u], a.indptr[u + 1])
        ok = ab[sl] >= 0
        r = ab[sl][ok] + 0.5 * ti[sl][ok]
        w = a.data[sl][ok]
        P, na = int(r.size), int(n_adm[u])
        pct = r / (na - 1.0) if na > 1 else np.full(P, np.nan)
        sw, swp = float(np.sum(w)), float(np.sum(w * pct))
        out["sum_w"][u], out["sum_w_pct"][u], out["P"][u] = sw, swp, P
        if P and sw != 0.0:
            out["mpr"][u] = swp / sw
        if P and na != P:
            out["auc"][u] = 1.0 - (float(np.sum(r)) - P * (P - 1.0) * 0.5) / (P * float(na - P))
        if P:
            out["mrr"][u] = 1.0 / (1.0 + float(np.min(r)))
    return out


def rank_totals(summary):
    """The data-set numbers of a `rank_summary`: mpr = sum_u sum w pct / sum_u sum w over the rows whose terms are finite (Hu,
    Koren and Volinsky's expected percentile rank), auc and mrr the means over the rows where they are defined, n the admissible
    entries.  NaN where nothing is defined."""
    sw, swp = np.asarray(summary["sum_w"], dtype=np.float64), np.asarray(summary["sum_w_pct"], dtype=np.float64)
    ok = np.isfinite(sw) & np.isfinite(swp) & (np.asarray(summary["P"]) > 0)
    tot_w, tot = float(np.sum(sw[ok])), float(np.sum(swp[ok]))

    def mean(v):
        v = np.asarray(v, dtype=np.float64)
        v = v[~np.isnan(v)]
        return float(np.mean(v)) if v.size else float("nan")
    return {"mpr": tot / tot_w if tot_w != 0.0 else float("nan"), "auc": mean(summary["auc"]), "mrr": mean(summary["mrr"]),
            "n": int(np.sum(summary["P"]))}
