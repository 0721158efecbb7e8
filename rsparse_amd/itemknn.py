"""ItemKNN: item-based k-nearest-neighbours on the co-occurrence of items, integer from end to end.

The definition (include/rsparse_wrmf_hip.h repeats it for C hosts; wrmf_itemknn.hip computes it on the device):

Fit.  B is the PATTERN of the users x items matrix in canonical CSR -- duplicates summed and explicit zeros eliminated here, on
the host, before the upload; the values are otherwise ignored.  n_j is the number of users of item j, c_ij = (B^T B)_ij for
i != j, and n_users <= 2^26 so that c^2 and n_i n_j are exact in double.  The order key of neighbour j of item i is ONE division
of two integers, evaluated in double:

    similarity   key                      reported value
    "count"      c / 1                    c
    "cosine"     c^2 / (n_i n_j)          sqrt(key), taken on the host
    "jaccard"    c / (n_i + n_j - c)      the key

The neighbours of i are the K items j != i with c_ij > 0 of largest key, ties to the smaller j: `neighbors` (n_items, K) int32,
0-based, padded with -1; `counts` (n_items, K) int32, 0 in the padding; `item_count` = n_j.  The device returns items and counts
only; every float the user sees is computed from them here.

Predict.  q (n_items, K) is an integer weight table: rint(sim * 2^30) for cosine and Jaccard (sim <= 1), c for count.  For a
row u of x (pattern only), score_u[j] = the sum of q[i, s] over the items i of the row and the slots s with neighbors[i, s] == j,
an int64 that cannot overflow (a row has fewer than 2^31 items, q <= 2^30).  The list is the k items of largest score among
those neither in the row's not_recommend entries nor in items_exclude, ties to the smaller item; items of score 0 are ranked
too, so a list is shorter than k only when fewer than k items are admissible, and is then padded as `WRMF.predict` pads: -1 in
the result, NaN in `.scores`.  `.scores` is score / 2^30 (the raw sum for "count") as float64.

  cooccurrence_reference    the fit, per item, in numpy integers
  knn_recommend_reference   the lists, per row
  ItemKNN                   the model: fit / similar_items / predict / evaluate
"""
import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from .wrmf import WRMF, TopItems

SIMILARITIES = {"count": _lib.KNN_COUNT, "cosine": _lib.KNN_COSINE, "jaccard": _lib.KNN_JACCARD}
Q_ONE = 1 << 30   # the fixed point of the weights


def canonical_pattern(x, n_items=None):
    """the pattern the model sees: CSR, duplicates summed, explicit zeros eliminated, columns ascending"""
    if not sp.issparse(x):
        raise TypeError("x must be a scipy sparse matrix (users x items)")
    m = sp.csr_matrix(x, dtype=np.float64, copy=True)
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    if n_items is not None and m.shape[1] != n_items:
        raise ValueError("x has %d columns, the model %d items" % (m.shape[1], n_items))
    return m


def _check_similarity(similarity):
    if similarity not in SIMILARITIES:
        raise ValueError("similarity must be one of 'cosine', 'jaccard', 'count'")
    return similarity


def _check_neighbors(K):
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
        raise ValueError("k_neighbors must be an integer >= 1")
    if K > _lib.KNN_MAX_NEIGHBORS:
        raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "k_neighbors > 256 is not on the device path")
    return int(K)


def order_key(c, n_i, n_j, similarity):
    """the order key of the definition: ONE division of two integers (int64 arrays or scalars), evaluated in double"""
    c, n_i, n_j = (np.asarray(a, dtype=np.int64) for a in (c, n_i, n_j))
    if similarity == "count":
        return c.astype(np.float64) / np.float64(1)
    if similarity == "cosine":
        return (c * c).astype(np.float64) / (n_i * n_j).astype(np.float64)
    return c.astype(np.float64) / (n_i + n_j - c).astype(np.float64)


def cooccurrence_reference(x, K, similarity="cosine"):
    """-> (neighbors (n_items, K) int32, counts (n_items, K) int32, item_count (n_items,) int64): the fit of the definition, one
    item at a time, on integers; no items x items array is formed."""
    _check_similarity(similarity)
    K = int(K)
    m = canonical_pattern(x)
    n_users, n_items = m.shape
    if n_users > _lib.KNN_MAX_USERS:
        raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "n_users > 2^26: c^2 and n_i n_j would not be exact in double")
    up, uj = m.indptr.astype(np.int64), m.indices.astype(np.int64)
    t = m.tocsc()
    t.sort_indices()
    ip, iu = t.indptr.astype(np.int64), t.indices.astype(np.int64)
    n = np.diff(ip)
    neighbors = np.full((n_items, K), -1, dtype=np.int32)
    counts = np.zeros((n_items, K), dtype=np.int32)
    for i in range(n_items):
        users = iu[ip[i]:ip[i + 1]]
        if users.size == 0:
            continue
        seen = np.concatenate([uj[up[u]:up[u + 1]] for u in users])
        if seen.size * 8 >= n_items:
            c = np.bincount(seen, minlength=n_items)
            j = np.flatnonzero(c)
            c = c[j]
        else:
            j, c = np.unique(seen, return_counts=True)
        keep = j != i
        j, c = j[keep], c[keep].astype(np.int64)
        key = order_key(c, n[i], n[j], similarity)
        first = np.lexsort((j, -key))[:K]
        neighbors[i, :first.size] = j[first]
        counts[i, :first.size] = c[first]
    return neighbors, counts, n.astype(np.int64)


def similarity_values(neighbors, counts, item_count, similarity):
    """the reported value of every slot of the table (float64, NaN in the padding), from the integers alone"""
    _check_similarity(similarity)
    neighbors, counts = np.asarray(neighbors), np.asarray(counts, dtype=np.int64)
    n = np.asarray(item_count, dtype=np.int64)
    pad = neighbors < 0
    n_i = np.broadcast_to(n[:, None], neighbors.shape) if neighbors.size else np.zeros(neighbors.shape, np.int64)
    n_j = n[np.where(pad, 0, neighbors)] if neighbors.size else n_i
    with np.errstate(divide="ignore", invalid="ignore"):
        key = order_key(np.where(pad, 0, counts), np.where(pad, 1, n_i), np.where(pad, 1, n_j), similarity)
        val = np.sqrt(key) if similarity == "cosine" else key
    return np.where(pad, np.nan, val)


def weight_table(neighbors, counts, item_count, similarity):
    """q of the definition: (n_items, K) int64 in 0 .. 2^30 (count: the counts themselves), 0 in the padding"""
    if similarity == "count":
        return np.where(np.asarray(neighbors) < 0, 0, np.asarray(counts, dtype=np.int64))
    sim = similarity_values(neighbors, counts, item_count, similarity)
    return np.where(np.isnan(sim), 0, np.rint(np.nan_to_num(sim) * Q_ONE)).astype(np.int64)


def knn_recommend_reference(x, neighbors, q, k, not_recommend=None, items_exclude=()):
    """-> (items (n, k) int64, 0-based with -1 where fewer than k items are admissible; scores (n, k) int64, 0 there): the lists
    of the definition, one row of x at a time.  not_recommend: a sparse matrix of x's shape, or None."""
    neighbors, q = np.asarray(neighbors, dtype=np.int64), np.asarray(q, dtype=np.int64)
    n_items = neighbors.shape[0]
    m = canonical_pattern(x, n_items)
    k = int(k)
    nr = None
    if not_recommend is not None:
        nr = sp.csr_matrix(not_recommend)
        if nr.shape != m.shape:
            raise ValueError("not_recommend must have the shape of x")
    excl = np.asarray(list(items_exclude), dtype=np.int64)
    items = np.full((m.shape[0], k), -1, dtype=np.int64)
    scores = np.zeros((m.shape[0], k), dtype=np.int64)
    for u in range(m.shape[0]):
        own = m.indices[m.indptr[u]:m.indptr[u + 1]]
        nb, w = neighbors[own].ravel(), q[own].ravel()
        score = np.zeros(n_items, dtype=np.int64)
        np.add.at(score, nb[nb >= 0], w[nb >= 0])
        adm = np.ones(n_items, dtype=bool)
        if nr is not None:
            adm[nr.indices[nr.indptr[u]:nr.indptr[u + 1]]] = False
        adm[excl] = False
        cand = np.flatnonzero(adm)
        first = cand[np.lexsort((cand, -score[cand]))[:k]]
        items[u, :first.size] = first
        scores[u, :first.size] = score[first]
    return items, scores


class ItemKNN:
    """Item-based k-nearest-neighbours on the co-occurrence of items (the module's docstring is the definition).

    k_neighbors: K, 1 .. 256; similarity: "cosine", "jaccard" or "count"; device / backend: as `WRMF`.  A backend without
    `cooc_neighbors` / `knn_recommend` (the CPU stand-in of the tests) runs the numpy definitions."""

    def __init__(self, k_neighbors=50, similarity="cosine", device=None, backend=None):
        self._K = _check_neighbors(k_neighbors)
        self._similarity = _check_similarity(similarity)
        self._device = device
        self._be = backend
        self.neighbors = self.counts = self.similarities = self.item_count = None
        self._d_tables = None   # (neighbors, q) on the device

    def _backend(self):
        if self._be is None:
            from .engine import HipBackend
            self._be = HipBackend(self._device)
        return self._be

    @staticmethod
    def _one_rank():
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "ItemKNN does not shard over torch.distributed ranks")

    def _fitted(self):
        if self.neighbors is None:
            raise RuntimeError("model is not fitted")

    # ------------------------------------------------------------------------------------------
    def fit(self, x, ws_rows=0):
        """the neighbour table of the users x items matrix x -> self (`neighbors`, `counts`, `similarities`, `item_count`)"""
        self._one_rank()
        m = canonical_pattern(x)
        n_users, n_items = m.shape
        if n_users > _lib.KNN_MAX_USERS:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "n_users > 2^26: c^2 and n_i n_j would not be exact in double")
        be = self._backend()
        self._d_tables = None
        if not hasattr(be, "cooc_neighbors"):
            nb, ct, cnt = cooccurrence_reference(m, self._K, self._similarity)
        else:
            up, uj = be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32)
            ones = torch.ones(int(uj.numel()), dtype=torch.float32, device=uj.device)
            # the CSR rows of x are the CSC columns of its transpose (items x users): transposed, item -> its users
            ip, iu, _ = be.transpose_csc(n_items, n_users, up, uj, ones)
            d_nb, d_ct = be.cooc_neighbors(ip, iu, up, uj, n_users, n_items, SIMILARITIES[self._similarity], self._K, ws_rows=ws_rows)
            nb, ct = d_nb.cpu().numpy(), d_ct.cpu().numpy()
            cnt = np.diff(ip.cpu().numpy().astype(np.int64))
        self.neighbors, self.counts, self.item_count = nb, ct, cnt
        self.similarities = similarity_values(nb, ct, cnt, self._similarity)
        return self

    def _weights(self):
        return weight_table(self.neighbors, self.counts, self.item_count, self._similarity)

    def similar_items(self, items=None, k=10):
        """rows of the table: the k <= k_neighbors nearest items of `items` (default: every item) as `TopItems` (-1 where an item
        has fewer) with the similarities in `.scores` (NaN there)"""
        self._fitted()
        k = int(k)
        if not 1 <= k <= self._K:
            raise ValueError("k must lie in 1 .. k_neighbors")
        n_items = self.neighbors.shape[0]
        q = np.arange(n_items) if items is None else np.atleast_1d(np.asarray(items, dtype=np.int64))
        if q.size and (q.min() < 0 or q.max() >= n_items):
            raise ValueError("some of items are not items of the model")
        out = self.neighbors[q, :k].astype(np.int64).view(TopItems)
        out.scores = self.similarities[q, :k].copy()
        return out

    def _lists(self, x, k, not_recommend, items_exclude, ws_rows=0):
        """-> (m: x as a canonical pattern, items int32 (n, k) 1-based with NA_integer_, scores int64 (n, k)), as tensors of the
        backend"""
        self._fitted()
        self._one_rank()
        n_items = self.neighbors.shape[0]
        m = canonical_pattern(x, n_items)
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError("k must be an integer >= 1")
        if k > _lib.KNN_MAX_TOPK:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "predict: k > 1024 is not on the device path")
        excl = np.unique(np.asarray(list(items_exclude), dtype=np.int64))
        if excl.size and (excl.min() < 0 or excl.max() >= n_items):
            raise ValueError("some of items_exclude indices are bigger than number of items")
        if isinstance(not_recommend, str) and not_recommend == "x":
            not_recommend = m
        if not_recommend is not None:
            if not sp.issparse(not_recommend):
                raise TypeError("'not_recommend' should be NULL or 'sparseMatrix'")
            not_recommend = sp.csr_matrix(not_recommend)
            if not_recommend.shape != m.shape:
                raise ValueError("not_recommend must have the shape of x")
        be = self._backend()
        if not hasattr(be, "knn_recommend"):
            it, sc = knn_recommend_reference(m, self.neighbors, self._weights(), k, not_recommend, excl)
            res = np.where(it < 0, np.int64(-2147483648), it + 1).astype(np.int32)
            return m, torch.from_numpy(res), torch.from_numpy(sc)
        if self._d_tables is None:
            self._d_tables = (be.to_device(self.neighbors, torch.int32), be.to_device(self._weights(), torch.int64))
        nr_p = nr_j = None
        if not_recommend is not None and not_recommend.nnz:
            nr_p, nr_j = be.to_device(not_recommend.indptr, torch.int32), be.to_device(not_recommend.indices, torch.int32)
        d_ex = be.to_device(excl, torch.int32) if excl.size else None
        res, sc = be.knn_recommend(be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32), self._d_tables[0],
                                   self._d_tables[1], k, nr_p, nr_j, d_ex, ws_rows=ws_rows)
        return m, res, sc

    def predict(self, x, k, not_recommend="x", items_exclude=(), ws_rows=0):
        """the k best items of every row of x, with the conventions of `WRMF.predict`: `not_recommend` (default: x itself; None =
        nothing) and `items_exclude` (0-based) are skipped; -> `TopItems` (n x k, 0-based, -1 where fewer than k items are
        admissible) with `.scores` (float64: score / 2^30, the raw sum for "count"; NaN in the padding).  1 <= k <= 1024."""
        _, res, sc = self._lists(x, k, not_recommend, items_exclude, ws_rows)
        idx = res.cpu().numpy().astype(np.int64)
        pad = idx == -2147483648
        out = np.where(pad, -1, idx - 1).view(TopItems)
        s = sc.cpu().numpy().astype(np.float64)
        if self._similarity != "count":
            s = s / np.float64(Q_ONE)
        out.scores = np.where(pad, np.nan, s)
        return out

    def evaluate(self, x, actual, k, not_recommend="x", items_exclude=(), metrics=("ap", "ndcg")):
        """`predict(x, max(k), ...)` once, scored against the held-out `actual` by the package's list metrics: "ap", "ndcg"
        (`rsparse_amd.metrics.ranking_metrics`), "precision", "recall", "hit", "mrr", "coverage" (`topk_metrics`), "popularity"
        and "novelty" (`list_metrics`, with the fitted item counts).  k: a cutoff or a strictly ascending sequence of them; a
        sequence returns (n, T) arrays (coverage: (T,)).  The lists stay on the device."""
        from .metrics import HIT_METRICS, LIST_METRICS, NEVER_SEEN, canonical_actual, check_cutoffs, coverage_from_first_seen, self_information
        metrics = tuple(metrics)
        known = ("ap", "ndcg") + HIT_METRICS + ("coverage",) + LIST_METRICS
        if not metrics or any(name not in known for name in metrics):
            raise ValueError("metrics must name some of %s" % ", ".join(repr(name) for name in known))
        scalar_k = not isinstance(k, (tuple, list, np.ndarray, range))
        cutoffs = check_cutoffs((int(k),) if scalar_k else k)
        m, res, _ = self._lists(x, int(cutoffs[-1]), not_recommend, items_exclude)
        act = canonical_actual(actual, m.shape[0])
        be = self._backend()
        n_items = self.neighbors.shape[0]
        d_p, d_j = be.to_device(act.indptr, torch.int32), be.to_device(act.indices, torch.int32)
        out = {}
        want_ap, want_ndcg = "ap" in metrics, "ndcg" in metrics
        if want_ap or want_ndcg:
            d_x = be.to_device(act.data, torch.float64)
            cols = [be.ranking_metrics(res[:, :c].contiguous(), d_p, d_j, d_x, want_ap, want_ndcg) for c in cutoffs]
            for pos, name in enumerate(("ap", "ndcg")):
                if name in metrics:
                    out[name] = torch.stack([c[pos] for c in cols], dim=1)
        hit_names = tuple(name for name in HIT_METRICS if name in metrics)
        if hit_names or "coverage" in metrics:
            first_seen = torch.full((n_items,), NEVER_SEEN, dtype=torch.int32, device=res.device) if "coverage" in metrics else None
            fn = be.hit_metrics if hasattr(be, "hit_metrics") else WRMF._hit_metrics_host
            out.update(fn(res, d_p, d_j, cutoffs, hit_names, first_seen))
        list_names = tuple(name for name in LIST_METRICS if name in metrics)
        if list_names:
            d_cnt = be.to_device(self.item_count, torch.int32) if "popularity" in metrics else None
            d_info = be.to_device(self_information(self.item_count), torch.int64) if "novelty" in metrics else None
            fn = be.list_metrics if hasattr(be, "list_metrics") else WRMF._list_metrics_host
            out.update(fn(res, cutoffs, n_items, list_names, d_cnt, d_info, None))
        out = {name: v.cpu().numpy() for name, v in out.items() if name in metrics}
        out = {name: (v[:, 0] if scalar_k else v) for name, v in out.items()}
        if "coverage" in metrics:
            cov = coverage_from_first_seen(first_seen.cpu().numpy(), np.asarray(cutoffs, dtype=np.int32))
            out["coverage"] = float(cov[0]) if scalar_k else cov
        return {name: out[name] for name in known if name in metrics}
