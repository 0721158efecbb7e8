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
