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

Weighted values (`similarity` "dot", "asymmetric", "rp3beta", and "cosine" with a `weighting`).  On the same canonical pattern
an entry (u, i) carries two unsigned integers: l_ui, used when i is the item whose neighbours are sought, and r_ui, used when i is
the neighbour.  Both are uint32 with max(l) max(r) max_j n_j < 2^53, so that

    c_ij = sum_u l_ui r_uj        (j != i; uint64, below 2^53: double(c_ij) is exact)
    key_ij = double(c_ij) / (a_i b_j + h)

with a, b tables of n_items doubles and h one double, all made on the host.  The key takes exactly three roundings, in double:
the product, the sum, the division; nothing is contracted into a fused multiply-add.  The neighbours of i are the K items j != i
with c_ij > 0 of largest key, ties to the smaller j: `neighbors` as above, `sums` (n_items, K) uint64 = c_ij, 0 in the padding.
The device returns integers only; the reported similarity of a slot is its key, recomputed here from `sums` and the tables.
Preconditions, checked here: a, b finite and in [2^-200, 2^200], h finite and in [0, 2^400]; every key of a non-empty cell is then
a positive normal double and 0 stays the mark of an empty cell.

Quantisation.  quantize_values(w, bits) for float64 weights w >= 0, finite (else ValueError): scale = (2^bits - 1) / max(w),
q = rint(w scale) in double, clipped to [1 if w > 0 else 0, 2^bits - 1].  An operand whose stored weights are all equal is
quantised to 1 with scale = 1 / value.  bits = min(the `bits` asked for (default 16, at most 24), floor((53 - ceil(log2(max_j
n_j))) / 2)); if the 2^53 bound still fails: ValueError.

The recipes are host rules for (l, r, a, b, h).  W is the weighted matrix in float64 (`weighting` None: the pattern of ones;
"values": the stored values; a `Confidence`: fitted on x at fit, applied by its own transform to new users at predict),
S_i = sum_u q_ui^2 an exact integer, s_l and s_r the two quantisation scales:

    similarity             l          r                            a_i                     b_j              h
    "dot"                  q(W)       q(W)                         s_l                     s_r              0
    "cosine" (weighting)   q(W)       q(W)                         sqrt(S_i)               sqrt(S_j)        shrinkage s_l s_r
    "asymmetric"           q(W)       q(W)                         S_i^alpha               S_j^(1 - alpha)  shrinkage s_l s_r
    "rp3beta"              q(W^alpha) q((w_uj / d_u)^alpha),       s_l (sum_u w_ui)^alpha  s_r n_j^beta     0
                                      d_u = sum_j w_uj

(beta = 0 is P3alpha.  A table entry that would be 0 -- an item without a positive weight -- is stored as 1: such an item has no
non-empty cell in its row and is in none of another's.)  ItemKNN(similarity in ("cosine", "jaccard", "count"), weighting=None) is
the binary path above, unchanged.

Weighted lists.  q[i, s] = rint(sim (2^30 / max(sim))) clipped to [0, 2^30]; xq holds the row's weights (W, W^alpha for
"rp3beta") quantised with the FIT's scale of l and clipped to 2^16 - 1, so that a list depends neither on the batch nor on the
other rows of the call; xq = 1 where the model has no weighting.  score_u[j] = sum of xq_ui q[i, s] over the items i of the row
and the slots with neighbors[i, s] == j.  A row whose xq sum to 2^31 or more is refused (`UnsupportedOnDevice`): a score stays
below 2^61.  Selection, ties, zero scores, padding and the filters are as above; `.scores` is score / (s_l 2^30 / max(sim)).

  cooccurrence_reference            the fit, per item, in numpy integers
  quantize_values, weighted_operands, weighted_cooccurrence_reference      the weighted fit
Evaluation.  Three more readers of score_u, integers like it, so that the model runs under the protocols of `WRMF`: the score at
given cells (nothing masked); the list within a row's own candidates -- admissible = the candidates minus the not_recommend row
minus items_exclude, the same order (score descending, equal scores to the SMALLER item: not the reference heap's rule that
`WRMF.predict(candidates=)` follows), candidates of score 0 ranked --; and, for a held-out entry (u, h) with A_u the items outside
the not_recommend row and outside items_exclude, above = #{j in A_u : s_j > s_h} and tied = #{j in A_u, j != h : s_j == s_h}
(-1 / -1 for h outside A_u), n_adm = |A_u|, from which `rank_summary` takes MPR, AUC and MRR.

  cooccurrence_reference            the fit, per item, in numpy integers
  quantize_values, weighted_operands, weighted_cooccurrence_reference      the weighted fit
  knn_recommend_reference           the lists, per row
  knn_score_pairs_reference, knn_candidates_reference, knn_ranks_reference      the evaluation, per row
  ItemKNN                           the model: fit / similar_items / predict / evaluate / sample_negatives / score / held_out_ranks /
                                    evaluate_ranks
"""
import types

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from .wrmf import WRMF, TopItems

SIMILARITIES = {"count": _lib.KNN_COUNT, "cosine": _lib.KNN_COSINE, "jaccard": _lib.KNN_JACCARD}
WEIGHTED = ("dot", "cosine", "asymmetric", "rp3beta")   # the kinds on weighted values ("cosine": with a weighting)
Q_ONE = 1 << 30   # the fixed point of the weights
MAX_BITS = 24     # of a quantised operand
XQ_MAX = (1 << 16) - 1   # of a row's weight at predict
TABLE_MIN, TABLE_MAX, H_MAX = 2.0 ** -200, 2.0 ** 200, 2.0 ** 400


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


def _check_bits(bits):
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not 1 <= bits <= MAX_BITS:
        raise ValueError("bits must be an integer in 1 .. %d" % MAX_BITS)
    return int(bits)


def quantize_values(w, bits=16, scale=None, top=None):
    """-> (q int64, scale float): the integers of the float64 weights w >= 0 by the module's rule.  scale: use this one (the
    fit's, at predict) instead of deriving it from w; top: the upper clip (default 2^bits - 1)."""
    w = np.asarray(w, dtype=np.float64)
    if w.size and not (np.isfinite(w).all() and w.min() >= 0):
        raise ValueError("the weights must be finite and non-negative")
    top = (1 << _check_bits(bits)) - 1 if top is None else int(top)
    if scale is None:
        w_max = np.float64(w.max()) if w.size else np.float64(0)
        if w_max == 0:
            return np.zeros(w.shape, dtype=np.int64), 1.0
        if w.min() == w_max:
            return np.ones(w.shape, dtype=np.int64), float(np.float64(1) / w_max)
        scale = np.float64(top) / w_max
        if not np.isfinite(scale):
            raise ValueError("the largest weight is too small to scale")
    q = np.rint(w * np.float64(scale))
    q = np.minimum(np.maximum(q, np.where(w > 0, 1.0, 0.0)), np.float64(top))
    return q.astype(np.int64), float(scale)


def operand_bits(bits, max_n):
    """min(bits, floor((53 - ceil(log2(max_n))) / 2)): two operands of that width over max_n users keep a sum below 2^53"""
    max_n = int(max_n)
    return min(_check_bits(bits), (53 - (max_n - 1).bit_length() if max_n > 1 else 53) // 2)


def check_exact_bound(l, r, max_n):
    """max(l) max(r) max_j n_j < 2^53, in Python integers, or ValueError"""
    top = (int(np.max(l)) if np.size(l) else 0) * (int(np.max(r)) if np.size(r) else 0) * int(max_n)
    if top >= 1 << 53:
        raise ValueError("max(l) max(r) max_j n_j = %d >= 2^53: a sum would not be exact in double" % top)


def check_tables(a, b, h):
    a, b, h = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), float(h)
    for t in (a, b):
        if t.size and not (np.isfinite(t).all() and t.min() >= TABLE_MIN and t.max() <= TABLE_MAX):
            raise ValueError("the tables a, b must be finite and in [2^-200, 2^200]")
    if not (np.isfinite(h) and 0.0 <= h <= H_MAX):
        raise ValueError("h must be finite and in [0, 2^400]")


def _check_recipe(similarity, shrinkage, alpha, beta):
    if similarity not in WEIGHTED:
        raise ValueError("a weighted similarity must be one of 'dot', 'cosine', 'asymmetric', 'rp3beta'")
    if alpha is None:
        alpha = 1.0 if similarity == "rp3beta" else 0.5
    shrinkage, alpha, beta = float(shrinkage), float(alpha), float(beta)
    if not (np.isfinite(shrinkage) and shrinkage >= 0):
        raise ValueError("shrinkage must be finite and >= 0")
    if not (np.isfinite(alpha) and alpha >= 0) or (similarity == "asymmetric" and alpha > 1):
        raise ValueError("alpha must be finite and >= 0 (asymmetric: in [0, 1])")
    if not (np.isfinite(beta) and beta >= 0):
        raise ValueError("beta must be finite and >= 0")
    return shrinkage, alpha, beta


def weighted_operands(w, similarity, shrinkage=0.0, alpha=None, beta=0.0, bits=16):
    """the recipe of `similarity` on the weighted matrix w (a canonical CSR, float64; its stored entries are the pattern)
    -> a namespace: l, r (int64, one per stored position of w), a, b (n_items float64), h, scale_l, scale_r, bits, item_count"""
    shrinkage, alpha, beta = _check_recipe(similarity, shrinkage, alpha, beta)
    n_items = w.shape[1]
    j, v = w.indices, np.asarray(w.data, dtype=np.float64)
    if v.size and not (np.isfinite(v).all() and v.min() >= 0):
        raise ValueError("the weights must be finite and non-negative")
    n = np.bincount(j, minlength=n_items).astype(np.int64)
    max_n = int(n.max()) if n_items else 0
    bits = operand_bits(bits, max_n)
    if bits < 1:
        raise ValueError("an item has too many users for a quantised operand")
    one = lambda t: np.where(t > 0, t, 1.0)   # (an item without a positive weight: the entry is never used)
    if similarity == "rp3beta":
        rows = np.repeat(np.arange(w.shape[0]), np.diff(w.indptr))
        d = np.bincount(rows, weights=v, minlength=w.shape[0])
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(d[rows] > 0, v / d[rows], 0.0)
        l, s_l = quantize_values(v ** alpha, bits)
        r, s_r = quantize_values(share ** alpha, bits)
        col = np.bincount(j, weights=v, minlength=n_items)
        a = one(s_l * col ** alpha)
        b = one(s_r * n.astype(np.float64) ** beta)
        h = 0.0
    else:
        l, s_l = quantize_values(v, bits)
        r, s_r = l, s_l
        if similarity == "dot":
            a, b, h = np.full(n_items, s_l), np.full(n_items, s_r), 0.0
        else:
            S = np.bincount(j, weights=(l * l).astype(np.float64), minlength=n_items)   # (integers below 2^53: exact)
            if similarity == "cosine":
                a = b = one(np.sqrt(S))
            else:
                a, b = one(S ** alpha), one(S ** (1.0 - alpha))
            h = shrinkage * s_l * s_r
    check_exact_bound(l, r, max_n)
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    check_tables(a, b, h)
    return types.SimpleNamespace(l=l, r=r, a=a, b=b, h=float(h), scale_l=s_l, scale_r=s_r, bits=bits, item_count=n)


def weighted_key(c, a_i, b_j, h):
    """the order key of the weighted definition: double(c) / (a_i b_j + h), three roundings"""
    return np.asarray(c).astype(np.float64) / (np.asarray(a_i, dtype=np.float64) * np.asarray(b_j, dtype=np.float64) + np.float64(h))


def weighted_cooccurrence_reference(indptr, indices, l, r, n_items, a, b, h, K):
    """-> (neighbors (n_items, K) int32, sums (n_items, K) uint64): the weighted fit of the definition on the canonical CSR
    pattern (indptr, indices) with the operands l, r by stored position, one item at a time, on integers; no items x items array
    is formed."""
    K, n_items = int(K), int(n_items)
    up, uj = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    l, r = np.asarray(l, dtype=np.int64), np.asarray(r, dtype=np.int64)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    check_tables(a, b, h)
    n = np.bincount(uj, minlength=n_items)
    check_exact_bound(l, r, n.max() if n_items else 0)
    rows = np.repeat(np.arange(up.size - 1), np.diff(up))
    order = np.argsort(uj, kind="stable")          # the item-major orientation: users ascending within an item
    ip = np.concatenate([[0], np.cumsum(n)])
    iu, il = rows[order], l[order]
    neighbors = np.full((n_items, K), -1, dtype=np.int32)
    sums = np.zeros((n_items, K), dtype=np.uint64)
    for i in range(n_items):
        users, lv = iu[ip[i]:ip[i + 1]], il[ip[i]:ip[i + 1]]
        if users.size == 0:
            continue
        seen = np.concatenate([uj[up[u]:up[u + 1]] for u in users])
        add = np.concatenate([lu * r[up[u]:up[u + 1]] for u, lu in zip(users, lv)])
        j, inv = np.unique(seen, return_inverse=True)
        c = np.zeros(j.size, dtype=np.int64)
        np.add.at(c, inv, add)
        keep = (j != i) & (c > 0)
        j, c = j[keep], c[keep]
        key = weighted_key(c, a[i], b[j], h)
        first = np.lexsort((j, -key))[:K]
        neighbors[i, :first.size] = j[first]
        sums[i, :first.size] = c[first].astype(np.uint64)
    return neighbors, sums


def weighted_similarity_values(neighbors, sums, a, b, h):
    """the key of every slot (float64, NaN in the padding), recomputed from the sums and the tables"""
    neighbors, a, b = np.asarray(neighbors), np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    pad = neighbors < 0
    if not neighbors.size:
        return np.zeros(neighbors.shape, dtype=np.float64)
    key = weighted_key(np.where(pad, 0, np.asarray(sums)), a[:, None], np.where(pad, 1.0, b[np.where(pad, 0, neighbors)]), h)
    return np.where(pad, np.nan, key)


def weighted_weight_table(similarities):
    """-> (q (n_items, K) int64 in 0 .. 2^30, 0 in the padding; the scale 2^30 / max(sim), 1.0 for an empty table)"""
    sim = np.asarray(similarities, dtype=np.float64)
    live = ~np.isnan(sim)
    top = sim[live].max() if live.any() else 0.0
    scale = np.float64(Q_ONE) / np.float64(top) if top > 0 else np.float64(1)
    q = np.minimum(np.maximum(np.rint(np.where(live, sim, 0.0) * scale), 0.0), np.float64(Q_ONE))
    return np.where(live, q, 0.0).astype(np.int64), float(scale)


def knn_recommend_reference(x, neighbors, q, k, not_recommend=None, items_exclude=(), xv=None):
    """-> (items (n, k) int64, 0-based with -1 where fewer than k items are admissible; scores (n, k) int64, 0 there): the lists
    of the definition, one row of x at a time.  not_recommend: a sparse matrix of x's shape, or None.  xv: the integer weight of
    every stored entry of canonical_pattern(x), in its order (None: all ones); a neighbour's addend is xv q."""
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
    if xv is not None:
        xv = np.asarray(xv, dtype=np.int64)
        if xv.shape != (m.nnz,):
            raise ValueError("xv must hold one weight per stored entry of the canonical pattern of x")
    for u in range(m.shape[0]):
        own = m.indices[m.indptr[u]:m.indptr[u + 1]]
        nb, w = neighbors[own].ravel(), q[own].ravel()
        if xv is not None:
            w = (xv[m.indptr[u]:m.indptr[u + 1], None] * q[own]).ravel()
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


def _scored_rows(x, neighbors, q, xv):
    """-> (m: the canonical pattern of x, score(u): the int64 score of every item for row u, as knn_recommend_reference sums it)"""
    neighbors, q = np.asarray(neighbors, dtype=np.int64), np.asarray(q, dtype=np.int64)
    n_items = neighbors.shape[0]
    m = canonical_pattern(x, n_items)
    if xv is not None:
        xv = np.asarray(xv, dtype=np.int64)
        if xv.shape != (m.nnz,):
            raise ValueError("xv must hold one weight per stored entry of the canonical pattern of x")

    def score(u):
        own = m.indices[m.indptr[u]:m.indptr[u + 1]]
        w = q[own] if xv is None else xv[m.indptr[u]:m.indptr[u + 1], None] * q[own]
        nb, w = neighbors[own].ravel(), w.ravel()
        s = np.zeros(n_items, dtype=np.int64)
        np.add.at(s, nb[nb >= 0], w[nb >= 0])
        return s
    return m, score


def _admissible_rows(shape, not_recommend, items_exclude):
    """-> adm(u): the bool mask of the items outside row u of not_recommend (a sparse matrix of `shape`, or None) and outside
    items_exclude"""
    nr = None
    if not_recommend is not None:
        nr = sp.csr_matrix(not_recommend)
        if nr.shape != shape:
            raise ValueError("not_recommend must have the shape of x")
    excl = np.asarray(list(items_exclude), dtype=np.int64)

    def adm(u):
        a = np.ones(shape[1], dtype=bool)
        if nr is not None:
            a[nr.indices[nr.indptr[u]:nr.indptr[u + 1]]] = False
        a[excl] = False
        return a
    return adm


def knn_score_pairs_reference(x, neighbors, q, pairs, xv=None):
    """-> int64, one per stored position of canonical_pattern(pairs) (a sparse matrix of x's shape): score_u[j] of
    knn_recommend_reference at that cell, one row at a time.  Nothing is masked."""
    m, score = _scored_rows(x, neighbors, q, xv)
    pat = canonical_pattern(pairs, m.shape[1])
    if pat.shape != m.shape:
        raise ValueError("pairs must have the shape of x")
    out = np.zeros(pat.nnz, dtype=np.int64)
    for u in range(m.shape[0]):
        a, b = pat.indptr[u], pat.indptr[u + 1]
        if b > a:
            out[a:b] = score(u)[pat.indices[a:b]]
    return out


def knn_candidates_reference(x, neighbors, q, candidates, k, not_recommend=None, items_exclude=(), xv=None):
    """-> (items (n, k) int64 with -1, scores (n, k) int64 with 0 in the padding): knn_recommend_reference within per-row
    candidates.  The admissible items of a row are the stored positions of its row of canonical_pattern(candidates) minus the
    row's not_recommend entries minus items_exclude.  The order is ItemKNN's own -- score descending, equal scores to the SMALLER
    item -- and NOT the reference heap's rule that `WRMF.predict(candidates=)` follows.  Candidates of score 0 are ranked; a list
    is shorter than k only when fewer than k candidates are admissible."""
    m, score = _scored_rows(x, neighbors, q, xv)
    cand = canonical_pattern(candidates, m.shape[1])
    if cand.shape != m.shape:
        raise ValueError("candidates must have the shape of x")
    adm = _admissible_rows(m.shape, not_recommend, items_exclude)
    k = int(k)
    items = np.full((m.shape[0], k), -1, dtype=np.int64)
    scores = np.zeros((m.shape[0], k), dtype=np.int64)
    for u in range(m.shape[0]):
        c = cand.indices[cand.indptr[u]:cand.indptr[u + 1]].astype(np.int64)
        c = c[adm(u)[c]]
        s = score(u)[c]
        first = np.lexsort((c, -s))[:k]
        items[u, :first.size] = c[first]
        scores[u, :first.size] = s[first]
    return items, scores


def knn_ranks_reference(x, neighbors, q, actual, not_recommend=None, items_exclude=(), xv=None):
    """-> (above, tied: int32, one per stored entry of `actual` (CSR with sorted columns, duplicates merged, stored zeros kept);
    n_adm: int32 per row): the counts of rsparse_hip_held_out_ranks_device with s the integer score.  A_u = the items outside the
    not_recommend row and outside items_exclude, n_adm = |A_u|; above = #{j in A_u : s_j > s_h}, tied = #{j in A_u, j != h : s_j
    == s_h}; an entry outside A_u (or outside the items) gets -1 / -1."""
    from .metrics import canonical_actual
    m, score = _scored_rows(x, neighbors, q, xv)
    n, n_items = m.shape
    act = canonical_actual(actual, n)
    adm = _admissible_rows(m.shape, not_recommend, items_exclude)
    above = np.full(act.nnz, -1, dtype=np.int32)
    tied = np.full(act.nnz, -1, dtype=np.int32)
    n_adm = np.zeros(n, dtype=np.int32)
    for u in range(n):
        a = adm(u)
        n_adm[u] = a.sum()
        if act.indptr[u + 1] == act.indptr[u]:
            continue
        s = score(u)
        s_adm = s[a]
        for e in range(act.indptr[u], act.indptr[u + 1]):
            h = int(act.indices[e])
            if 0 <= h < n_items and a[h]:
                above[e] = np.count_nonzero(s_adm > s[h])
                tied[e] = np.count_nonzero(s_adm == s[h]) - 1
    return above, tied, n_adm


def evaluate_lists(be, res, actual, n_items, item_count, metrics, cutoffs, scalar_k):
    """the list metrics `metrics` (checked by the caller) of the lists `res` ((n, max(cutoffs)) int32 on the backend, 1-based with
    NA_integer_) against the held-out `actual`, at every cutoff: what `ItemKNN.evaluate` and `EASE.evaluate` return.  The lists
    stay on the device."""
    from .metrics import HIT_METRICS, LIST_METRICS, NEVER_SEEN, canonical_actual, coverage_from_first_seen, self_information
    known = ("ap", "ndcg") + HIT_METRICS + ("coverage",) + LIST_METRICS
    act = canonical_actual(actual, int(res.shape[0]))
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
        d_cnt = be.to_device(item_count, torch.int32) if "popularity" in metrics else None
        d_info = be.to_device(self_information(item_count), torch.int64) if "novelty" in metrics else None
        fn = be.list_metrics if hasattr(be, "list_metrics") else WRMF._list_metrics_host
        out.update(fn(res, cutoffs, n_items, list_names, d_cnt, d_info, None))
    out = {name: v.cpu().numpy() for name, v in out.items() if name in metrics}
    out = {name: (v[:, 0] if scalar_k else v) for name, v in out.items()}
    if "coverage" in metrics:
        cov = coverage_from_first_seen(first_seen.cpu().numpy(), np.asarray(cutoffs, dtype=np.int32))
        out["coverage"] = float(cov[0]) if scalar_k else cov
    return {name: out[name] for name in known if name in metrics}


class ItemKNN:
    """Item-based k-nearest-neighbours on the co-occurrence of items (the module's docstring is the definition).

    k_neighbors: K, 1 .. 256; similarity: "cosine", "jaccard" or "count" on the pattern, "dot", "asymmetric", "rp3beta" -- and
    "cosine" with a weighting -- on weighted values; weighting: None (the pattern of ones), "values" (the stored values) or a
    `rsparse_amd.Confidence`, fitted on x at `fit` and applied to new users at `predict`; shrinkage: added to the denominator
    of "cosine" / "asymmetric"; alpha: the exponent of "asymmetric" (default 0.5) and "rp3beta" (default 1); beta: the
    popularity exponent of "rp3beta" (0 = P3alpha); bits: of a quantised operand (at most 24); device / backend: as `WRMF`.
    A backend without `cooc_neighbors` / `cooc_neighbors_weighted` / `knn_recommend` / `knn_top_candidates` / `knn_score_pairs` /
    `knn_held_out_ranks` (the CPU stand-in of the tests) runs the numpy definitions.  Fitted: `neighbors`, `similarities`, `item_count`, and `counts` (pattern kinds) or `sums` (weighted)."""

    def __init__(self, k_neighbors=50, similarity="cosine", weighting=None, shrinkage=0.0, alpha=None, beta=0.0, bits=16, device=None,
                 backend=None):
        self._K = _check_neighbors(k_neighbors)
        if similarity not in SIMILARITIES and similarity not in WEIGHTED:
            raise ValueError("similarity must be one of 'cosine', 'jaccard', 'count', 'dot', 'asymmetric', 'rp3beta'")
        from .confidence import Confidence
        if not (weighting is None or isinstance(weighting, Confidence) or (isinstance(weighting, str) and weighting == "values")):
            raise ValueError("weighting must be None, 'values' or a Confidence")
        if weighting is not None and similarity in ("jaccard", "count"):
            raise ValueError("similarity %r is defined on the pattern: it takes no weighting" % similarity)
        self._similarity = similarity
        self._weighted = similarity not in SIMILARITIES or weighting is not None
        self._weighting = weighting
        self._bits = _check_bits(bits)
        self._recipe = _check_recipe(similarity, shrinkage, alpha, beta) if self._weighted else None
        self._device = device
        self._be = backend
        self.neighbors = self.counts = self.sums = self.similarities = self.item_count = None
        self._ops = None        # the weighted fit's tables and scales (weighted_operands, without l and r)
        self._q = None          # the weighted fit's (q, its scale)
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
        """the neighbour table of the users x items matrix x -> self (`neighbors`, `counts` or `sums`, `similarities`, `item_count`)"""
        self._one_rank()
        m = canonical_pattern(x)
        n_users, n_items = m.shape
        if self._weighted:
            return self._fit_weighted(m, ws_rows)
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

    def _weigh(self, m, be, fit):
        """the weighted matrix W of the canonical pattern m (float64, m's pattern): the model's `weighting`, fitted on m or applied"""
        wt = self._weighting
        if wt is None:
            w = m.copy()
            w.data[:] = 1.0
            return w
        if isinstance(wt, str):
            return m
        w = wt.fit_transform(m, backend=be) if fit else wt.transform(m, backend=be)
        if not (np.array_equal(w.indptr, m.indptr) and np.array_equal(w.indices, m.indices)):
            raise RuntimeError("the weighting changed the pattern of the matrix")
        return w

    def _fit_weighted(self, m, ws_rows):
        n_users, n_items = m.shape
        be = self._backend()
        self._d_tables = None
        shrinkage, alpha, beta = self._recipe
        w = self._weigh(m, be, True)
        ops = weighted_operands(w, self._similarity, shrinkage, alpha, beta, self._bits)
        if not hasattr(be, "cooc_neighbors_weighted"):
            nb, sums = weighted_cooccurrence_reference(m.indptr, m.indices, ops.l, ops.r, n_items, ops.a, ops.b, ops.h, self._K)
        else:
            up, uj = be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32)
            # the CSR rows of x are the CSC columns of its transpose: transposed, item -> its users, l with its entry (float64
            # carries the integers exactly)
            ip, iu, il = be.transpose_csc(n_items, n_users, up, uj, be.to_device(ops.l, torch.float64))
            d_nb, d_sums = be.cooc_neighbors_weighted(ip, iu, il, up, uj, be.to_device(ops.r, torch.int64), n_users, n_items,
                                                      be.to_device(ops.a, torch.float64), be.to_device(ops.b, torch.float64), ops.h,
                                                      self._K, ws_rows=ws_rows)
            nb, sums = d_nb.cpu().numpy(), d_sums.cpu().numpy().view(np.uint64)
        self.neighbors, self.sums, self.counts, self.item_count = nb, sums, None, ops.item_count
        self.similarities = weighted_similarity_values(nb, sums, ops.a, ops.b, ops.h)
        self._q = weighted_weight_table(self.similarities)
        ops.l = ops.r = None
        self._ops = ops
        return self

    def _weights(self):
        if self._weighted:
            return self._q[0]
        return weight_table(self.neighbors, self.counts, self.item_count, self._similarity)

    def _row_weights(self, m, be):
        """xq of the definition for the canonical pattern m of new rows, or None (no weighting: all ones)"""
        if not self._weighted or self._weighting is None:
            return None
        v = self._weigh(m, be, False).data
        if self._similarity == "rp3beta":
            if v.size and not (np.isfinite(v).all() and v.min() >= 0):
                raise ValueError("the weights must be finite and non-negative")
            v = v ** self._recipe[1]
        xq, _ = quantize_values(v, scale=self._ops.scale_l, top=XQ_MAX)
        rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
        if xq.size and np.bincount(rows, weights=xq).max() >= 1 << 31:   # (sums of integers below 2^53: exact in double)
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "predict: the quantised weights of a row sum to 2^31 or more")
        return xq

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

    def _rows(self, x, not_recommend="x", items_exclude=()):
        """what every scoring call starts with -> (m: x as a canonical pattern, be, xq: the rows' weights or None, not_recommend as
        CSR or None, items_exclude sorted and unique)"""
        self._fitted()
        self._one_rank()
        n_items = self.neighbors.shape[0]
        m = canonical_pattern(x, n_items)
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
        return m, be, self._row_weights(m, be), not_recommend, excl

    def _device_rows(self, be, m, xq, not_recommend=None, excl=()):
        """the operands of the backend's knn_* calls -> ((xp, xj, neighbors, q), {nr_p, nr_j, exclude0}, {xv})"""
        if self._d_tables is None:
            self._d_tables = (be.to_device(self.neighbors, torch.int32), be.to_device(self._weights(), torch.int64))
        nr_p = nr_j = None
        if not_recommend is not None and not_recommend.nnz:
            nr_p, nr_j = be.to_device(not_recommend.indptr, torch.int32), be.to_device(not_recommend.indices, torch.int32)
        d_ex = be.to_device(excl, torch.int32) if len(excl) else None
        kw = {} if xq is None else {"xv": be.to_device(xq, torch.int64)}
        rows = (be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32), self._d_tables[0], self._d_tables[1])
        return rows, {"nr_p": nr_p, "nr_j": nr_j, "exclude0": d_ex}, kw

    def _pattern(self, pairs, m, what):
        """`pairs` (a scipy sparse of x's shape) as a canonical CSR pattern of ones: columns ascending, duplicates merged, every
        stored position kept (a stored zero too)"""
        if not sp.issparse(pairs):
            raise TypeError("'%s' should be a 'sparseMatrix'" % what)
        if pairs.shape != m.shape:
            raise ValueError("%s must have the shape of x" % what)
        pat = sp.csr_matrix(pairs, dtype=np.float64, copy=True)
        pat.data[:] = 1.0
        return canonical_pattern(pat)

    def _lists(self, x, k, not_recommend, items_exclude, ws_rows=0, candidates=None):
        """-> (m: x as a canonical pattern, items int32 (n, k) 1-based with NA_integer_, scores int64 (n, k)), as tensors of the
        backend; candidates: a scipy sparse of x's shape, or None (the whole catalogue)"""
        m, be, xq, not_recommend, excl = self._rows(x, not_recommend, items_exclude)
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError("k must be an integer >= 1")
        if k > _lib.KNN_MAX_TOPK:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "predict: k > 1024 is not on the device path")
        cand = None if candidates is None else self._pattern(candidates, m, "candidates")
        if not hasattr(be, "knn_recommend" if cand is None else "knn_top_candidates"):
            if cand is None:
                it, sc = knn_recommend_reference(m, self.neighbors, self._weights(), k, not_recommend, excl, xv=xq)
            else:
                it, sc = knn_candidates_reference(m, self.neighbors, self._weights(), cand, k, not_recommend, excl, xv=xq)
            res = np.where(it < 0, np.int64(-2147483648), it + 1).astype(np.int32)
            return m, torch.from_numpy(res), torch.from_numpy(sc)
        rows, filters, kw = self._device_rows(be, m, xq, not_recommend, excl)
        if cand is None:
            res, sc = be.knn_recommend(*rows, k, filters["nr_p"], filters["nr_j"], filters["exclude0"], ws_rows=ws_rows, **kw)
        else:
            res, sc = be.knn_top_candidates(*rows, k, be.to_device(cand.indptr, torch.int32), be.to_device(cand.indices, torch.int32),
                                            ws_rows=ws_rows, **filters, **kw)
        return m, res, sc

    def predict(self, x, k, not_recommend="x", items_exclude=(), ws_rows=0, candidates=None):
        """the k best items of every row of x, with the conventions of `WRMF.predict`: `not_recommend` (default: x itself; None =
        nothing) and `items_exclude` (0-based) are skipped; -> `TopItems` (n x k, 0-based, -1 where fewer than k items are
        admissible) with `.scores` (float64: score / 2^30, the raw sum for "count", score / (s_l 2^30 / max(sim)) for the weighted
        kinds; NaN in the padding).  1 <= k <= 1024.

        `candidates` (a scipy sparse of x's shape; its values are ignored): every row is ranked within its own stored positions
        -- two-stage serving, a catalogue slice per user, sampled-negative evaluation.  The filters still apply; candidates of
        score 0 are ranked; a list is shorter than k only when fewer than k candidates are admissible.  The order is ItemKNN's
        own -- score descending, equal scores to the SMALLER item -- and NOT the reference heap's rule that
        `WRMF.predict(candidates=)` follows.  `candidates` holding every item reproduces `predict(x, k)` exactly."""
        _, res, sc = self._lists(x, k, not_recommend, items_exclude, ws_rows, candidates)
        return self._top_items(res, sc)

    def _scale(self, s):
        """integer scores -> what `.scores` reports (float64)"""
        s = np.asarray(s).astype(np.float64)
        if self._weighted:
            return s / (np.float64(self._ops.scale_l) * np.float64(self._q[1]))
        if self._similarity != "count":
            return s / np.float64(Q_ONE)
        return s

    def _top_items(self, res, sc):
        idx = res.cpu().numpy().astype(np.int64)
        pad = idx == -2147483648
        out = np.where(pad, -1, idx - 1).view(TopItems)
        out.scores = np.where(pad, np.nan, self._scale(sc.cpu().numpy()))
        return out

    def sample_negatives(self, x, n, actual=None, not_recommend="x", items_exclude=(), seed=None, weights=None):
        """`WRMF.sample_negatives` for the shape of x: the candidate matrix of a sampled-metric evaluation -- every row's stored
        positions of `actual` plus min(n, admissible) items drawn without replacement from those neither in `not_recommend`, nor
        in `actual`, nor in `items_exclude`.  The negatives depend on (seed, row, the row's exclusions, n_items, n) alone, so they
        ARE the ones `WRMF.sample_negatives(x, n, actual=, seed=)` returns for that seed.  `seed` is required: ItemKNN has no
        generator to draw one from."""
        if seed is None:
            raise ValueError("sample_negatives needs a seed: ItemKNN has no generator to draw one from")
        self._one_rank()
        return WRMF(backend=self._backend()).sample_negatives(x, n, actual=actual, not_recommend=not_recommend,
                                                              items_exclude=items_exclude, seed=seed, weights=weights)

    def score(self, x, pairs):
        """the model's score of the rows of x at given (user, item) cells: a scipy CSR matrix (float64) with the pattern of `pairs`
        (x's shape; columns sorted, duplicates merged, stored zeros are positions too) and, as values, the score scaled exactly as
        `predict`'s `.scores` are.  Nothing is masked: an item of the row's own history has its score too."""
        m, be, xq, _, _ = self._rows(x, None)
        pat = self._pattern(pairs, m, "pairs")
        if not hasattr(be, "knn_score_pairs"):
            sc = knn_score_pairs_reference(m, self.neighbors, self._weights(), pat, xv=xq)
        else:
            rows, _, kw = self._device_rows(be, m, xq)
            sc = be.knn_score_pairs(*rows, be.to_device(pat.indptr, torch.int32), be.to_device(pat.indices, torch.int32), **kw).cpu().numpy()
        return sp.csr_matrix((self._scale(sc), pat.indices, pat.indptr), shape=pat.shape)

    def _ranks(self, x, actual, not_recommend, items_exclude, ws_rows=0):
        """-> (be, actual as canonical CSR, (above, tied, n_adm) as tensors of the backend)"""
        from .metrics import canonical_actual
        m, be, xq, not_recommend, excl = self._rows(x, not_recommend, items_exclude)
        if not sp.issparse(actual):
            raise TypeError("'actual' should be a 'sparseMatrix'")
        if actual.shape != m.shape:
            raise ValueError("actual must have the shape of x")
        act = canonical_actual(actual, m.shape[0])
        if not hasattr(be, "knn_held_out_ranks"):
            got = knn_ranks_reference(m, self.neighbors, self._weights(), act, not_recommend, excl, xv=xq)
            return be, act, tuple(be.to_device(v, torch.int32) for v in got)
        rows, filters, kw = self._device_rows(be, m, xq, not_recommend, excl)
        got = be.knn_held_out_ranks(*rows, be.to_device(act.indptr, torch.int32), be.to_device(act.indices, torch.int32), ws_rows=ws_rows,
                                    **filters, **kw)
        return be, act, got

    def held_out_ranks(self, x, actual, not_recommend="x", items_exclude=(), ws_rows=0):
        """where every held-out interaction stands among ALL the items the user could be shown, by the model's integer score:
        `WRMF.held_out_ranks` for this model.  The admissible items of a row are those outside its `not_recommend` row (default:
        x itself) and outside `items_exclude`; for every stored entry (u, h) of `actual` (x's shape; stored zeros are entries):
        above = admissible items scored strictly higher than h, tied = other admissible items with an equal score, -1 / -1 when h
        itself is not admissible.  -> (above, tied: scipy CSR (int32) with the canonical pattern of `actual`; n_adm: the
        admissible items per row, int32).  The 0-based midrank of an entry is above + tied / 2."""
        _, act, (above, tied, n_adm) = self._ranks(x, actual, not_recommend, items_exclude, ws_rows)
        mk = lambda v: sp.csr_matrix((v.cpu().numpy().astype(np.int32), act.indices.copy(), act.indptr.copy()), shape=act.shape)
        return mk(above), mk(tied), n_adm.cpu().numpy().astype(np.int32)

    def evaluate_ranks(self, x, actual, not_recommend="x", items_exclude=(), per_user=False):
        """the full-ranking metrics of the held-out interactions `actual` (values = weights) from `held_out_ranks`' counts, with
        the formulas and the return shape of `WRMF.evaluate_ranks`: {"mpr", "auc", "mrr", "n"}; per_user=True adds "mpr_per_user",
        "auc_per_user", "mrr_per_user" and "n_adm_per_user"."""
        from .metrics import rank_totals
        be, act, (above, tied, n_adm) = self._ranks(x, actual, not_recommend, items_exclude)
        fn = be.rank_summary if hasattr(be, "rank_summary") else WRMF._rank_summary_host
        mpr, auc, mrr, sums = fn(be.to_device(act.indptr, torch.int32), be.to_device(act.data, torch.float64), above, tied, n_adm)
        sums = sums.cpu().numpy()
        per = {"mpr": mpr.cpu().numpy(), "auc": auc.cpu().numpy(), "mrr": mrr.cpu().numpy()}
        out = rank_totals({"sum_w": sums[:, 0], "sum_w_pct": sums[:, 1], "P": sums[:, 2], "auc": per["auc"], "mrr": per["mrr"]})
        if per_user:
            out.update({name + "_per_user": v for name, v in per.items()})
            out["n_adm_per_user"] = n_adm.cpu().numpy().astype(np.int32)
        return out

    def evaluate(self, x, actual, k, not_recommend="x", items_exclude=(), metrics=("ap", "ndcg"), candidates=None, negatives=None,
                 seed=None, negative_weights=None):
        """`predict(x, max(k), ...)` once, scored against the held-out `actual` by the package's list metrics: "ap", "ndcg"
        (`rsparse_amd.metrics.ranking_metrics`), "precision", "recall", "hit", "mrr", "coverage" (`topk_metrics`), "popularity"
        and "novelty" (`list_metrics`, with the fitted item counts).  k: a cutoff or a strictly ascending sequence of them; a
        sequence returns (n, T) arrays (coverage: (T,)).  The lists stay on the device.

        `candidates`: as in `predict` -- every metric is computed on the lists ranked within the rows' candidates.
        `negatives=n` with `seed` makes those candidates itself, the sampled protocol of `WRMF.evaluate(negatives=)`: every row's
        held-out items against n negatives, exactly `candidates=self.sample_negatives(x, n, actual, not_recommend,
        items_exclude, seed, negative_weights)` -- the negatives `WRMF.sample_negatives` returns for that seed.  `seed` is
        required with `negatives`; `negatives` excludes `candidates`; `negative_weights` needs `negatives`."""
        from .metrics import HIT_METRICS, LIST_METRICS, check_cutoffs
        metrics = tuple(metrics)
        known = ("ap", "ndcg") + HIT_METRICS + ("coverage",) + LIST_METRICS
        if not metrics or any(name not in known for name in metrics):
            raise ValueError("metrics must name some of %s" % ", ".join(repr(name) for name in known))
        scalar_k = not isinstance(k, (tuple, list, np.ndarray, range))
        cutoffs = check_cutoffs((int(k),) if scalar_k else k)
        if negatives is not None and candidates is not None:
            raise ValueError("negatives and candidates exclude each other: the negatives ARE the candidates")
        if negative_weights is not None and negatives is None:
            raise ValueError("negative_weights needs negatives: they weight the sampled negatives")
        if negatives is not None:
            if seed is None:
                raise ValueError("negatives needs a seed: ItemKNN has no generator to draw one from")
            candidates = self.sample_negatives(x, negatives, actual=actual, not_recommend=not_recommend, items_exclude=items_exclude,
                                               seed=seed, weights=negative_weights)
        m, res, _ = self._lists(x, int(cutoffs[-1]), not_recommend, items_exclude, candidates=candidates)
        return evaluate_lists(self._backend(), res, actual, self.neighbors.shape[0], self.item_count, metrics, cutoffs, scalar_k)
