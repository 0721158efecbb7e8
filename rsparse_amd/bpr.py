"""BPR (Rendle et al. 2009, "BPR: Bayesian Personalized Ranking from Implicit Feedback"): matrix factorisation trained on the
pairwise ranking loss, by deterministic mini-batch SGD with a scalar Adagrad state per embedding (the `RankMF` solver of the
modelled-on package with `update_items = TRUE / FALSE`), in a form that has no race: a mini-batch is taken from a snapshot of the
factors, its triples come from a counter-based stream that does not depend on the model, and the gradient rows are summed per
destination in a fixed order.

The definition (include/rsparse_wrmf_hip.h repeats it for C hosts; wrmf_bpr.hip runs it on the device):

Input.  x is reduced with `itemknn.canonical_pattern`: the binary model, columns ascending and unique per row.

Triples: stream 6 of the Philox4x32-10 of rsparse_amd/rng.py (its docstring has the specification).  An epoch has one triple per
stored entry; slot p of the CSR belongs to row u, position q = p - indptr[u], length L.  (u, i, j) = (the row, a uniform positive
of the row, the first of three uniform candidates that is not in the row); j = -1 -- a VOID triple, which takes no part in
anything -- when all three are in the row.  mode 0 is the fit (global row index g = row0 + u), mode 1 the fold-in (g = row0 for
EVERY row: a folded-in row's triples depend on the row alone, not on where it stands in x.  The price: in a fold-in epoch all rows
share the Philox outputs of a position q, so they draw the same three negative CANDIDATES there -- which one a row takes, and its
positive, still depend on the row; with the items frozen no row sees another's update, so nothing couples them).

Steps.  n_steps = ceil(nnz / batch) for the fit, 1 for the fold-in.  Step s holds the slots p = s, s + n_steps, s + 2 n_steps, ...
in ascending p; k = 0, 1, ... numbers them.  A user's triples in a step are consecutive in k.

One step, from the snapshot (U, V) at its start.  Every operation is a separately rounded float64 operation, the factors
widened from the model's dtype; nothing is fused.

    dot(a, b)   16 partial sums, partial l = the products a[c] * b[c] of c = l, l + 16, ... added in ascending c from +0.0;
                then v[0:8] + v[8:16], v[0:4] + v[4:8], v[0:2] + v[2:4], v[0] + v[1]
    d_k         dot(U[u], V[i] - V[j])                       (the differences rounded first)
    E(d)        d clamped to [-40, 40]; kk = rint(d * 1.4426950408889634);
                r = (d - kk * 6.93147180369123816490e-01) - kk * 1.90821492927058770002e-10;
                the polynomial sum_{n <= 13} r^n / n! in Horner form (coefficients 1.0 / n!), then ldexp(., kk)
    z_k         1 / (1 + E(d_k))
    rows        user u receives z_k (V[i] - V[j]); item i receives z_k U[u]; item j receives (-z_k) U[u]
    order       a destination sums its contributions in ascending k, within one k the positive role before the negative one.
                The list is cut into chunks of CHUNK = 64 consecutive contributions (RSPARSE_HIP_BPR_CHUNK); a chunk is summed
                sequentially from +0.0; the chunk sums are added sequentially to a total that starts at +0.0
    update      a destination with c >= 1 contributions (the others keep their bits):
                g = total - (lambda * c) * row;  a' = a + dot(g, g) / rank;
                row' = row + (lr * g) / sqrt(a')  unless a' == 0 (the row is then left alone);  row' rounded once into the dtype
    counts      per epoch (n_valid, n_correct): the triples that are not void, and those of them with d_k > 0

`a` is one float64 per user and per item (Adagrad's state) and is part of the fitted model.  update_items = False (the fold-in)
neither reads the items for update nor writes them.  A fit starts from `rng.init_factors` (streams 0 and 1, scale 0.01) with
a = 0; a fold-in from zero rows with a = 0 and runs `transform_iter` epochs of one step each.

Item features (`fit_transform(x, item_features=F)`): an item's embedding is not a free row but F[i, :] H, a
combination of the embeddings H (n_feat x rank) of the item's features, and every gradient goes through F to H -- the hybrid
model of the modelled-on `RankMF` (LightFM), which gives an item nobody has interacted with an embedding from its metadata.
F: n_items x n_feat, canonical CSR, finite values in the factors' dtype; aH: one float64 per feature, from 0.  One step:

    compose     V[i, c] = the sum over the stored features f of row i, in ascending f, of F[i, f] * H[f, c], sequentially from
                +0.0, rounded once into the dtype; an item without features has a zero row
    triples, z_k, the user side: as above, from the snapshot (U, V)
    item i      with c_i >= 1 contributions: G_i = its `total` above (before the regularisation term); V is not updated from it
    feature f   its column of F (the items that carry f, ascending) is cut into chunks of CHUNK consecutive STORED POSITIONS;
                within a chunk the items with c_i >= 1 contribute F[i, f] * G_i, summed sequentially from +0.0 (the others are
                skipped); the chunk sums are added sequentially to a total that starts at +0.0; C_f = the sum of those c_i.
                C_f >= 1: `update` with count = C_f, row = H[f], a = aH[f]; every other feature keeps its bits

The cut by stored position is known from F alone.  With F the identity this is the definition above with H = V, bit for bit.
The modelled-on solver hands every feature of an item the same gradient, whatever the feature's value (rankmf.cpp:254-265); here
the gradient is scaled by F[i, f], the derivative of the composition.

  bpr_triples, bpr_exp, bpr_step_reference, bpr_fit_reference     the definition, in numpy
  compose_reference, bpr_feat_step_reference, bpr_feat_fit_reference     the same through item features
  BPR                                                             the model: `WRMF`'s inference surface on these factors
"""
import math

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from . import rng as _rng
from .itemknn import canonical_pattern
from .wrmf import WRMF

CHUNK = _lib.BPR_CHUNK
_LOG2E, _LN2_HI, _LN2_LO = 1.4426950408889634, 6.93147180369123816490e-01, 1.90821492927058770002e-10
_COEF = [1.0 / float(math.factorial(n)) for n in range(14)]


def n_steps_of(nnz, batch):
    """ceil(nnz / batch), at least 1"""
    return max(1, -(-int(nnz) // int(batch)))


def step_slots(nnz, step, n_steps):
    """the CSR slots of step `step`: p = step, step + n_steps, ... below nnz, ascending (their order is k)"""
    return np.arange(int(step), int(nnz), int(n_steps), dtype=np.int64)


def step_slot_rows(seed, mode, epoch, row0, indptr, indices, n_items, step, n_steps):
    """What the triples of one step are drawn from -> (u, L, counter01, key, idx, ip, inside): per slot of the step, in the order k,
    the local row, its length and the first two counter words (q, g) of its Philox calls; the key; `inside(cand)`: whether each
    slot's candidate is in its row."""
    seed, mode, epoch, row0, n_items, step, n_steps = (int(v) for v in (seed, mode, epoch, row0, n_items, step, n_steps))
    ip, idx = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n_rows = ip.size - 1
    if (not 0 <= seed < 2 ** 64 or mode not in (0, 1) or not 0 <= epoch < 2 ** 31 or row0 < 0 or row0 + n_rows > 2 ** 32
            or not 0 <= n_items < 2 ** 31 or n_steps < 1 or not 0 <= step < n_steps or ip[0] != 0):
        raise ValueError("bpr_triples: bad arguments")
    p = step_slots(ip[-1], step, n_steps)
    u = np.searchsorted(ip, p, side="right") - 1
    L, q = (ip[u + 1] - ip[u]).astype(np.uint64), (p - ip[u]).astype(np.uint64)
    g = np.full(p.size, row0, dtype=np.uint64) + (u.astype(np.uint64) if mode == 0 else np.uint64(0))
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    # membership of a candidate in its row: the entries of a canonical pattern are sorted by (row, column)
    cells = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(ip)) * n_items + idx

    def inside(cand):
        want = u * n_items + cand
        at = np.searchsorted(cells, want)
        return (at < cells.size) & (cells[np.minimum(at, max(cells.size - 1, 0))] == want) if cells.size else np.zeros(p.size, bool)

    return u, L, np.stack([q, g], axis=-1), key, idx, ip, inside


def bpr_triples(seed, mode, epoch, row0, indptr, indices, n_items, step=0, n_steps=1):
    """The triples of one step -> (u, i, j): int32 arrays over k, u the LOCAL row, j = -1 for a void triple.  (indptr, indices): a
    canonical CSR pattern whose row pointers start at 0; row0: the global index of its first row."""
    u, L, qg, key, idx, ip, inside = step_slot_rows(seed, mode, epoch, row0, indptr, indices, n_items, step, n_steps)
    tail = np.broadcast_to(np.array([_rng.STREAM_BPR, int(epoch) + (int(mode) << 31)], dtype=np.uint64), qg.shape)
    o = _rng.philox4x32_10(np.concatenate([qg, tail], axis=-1), key).astype(np.uint64)
    s32 = np.uint64(32)
    pos = idx[ip[u] + ((o[:, 0] * L) >> s32).astype(np.int64)] if u.size else np.zeros(0, np.int64)
    neg = np.full(u.size, -1, dtype=np.int64)
    for t in (3, 2, 1):
        cand = ((o[:, t] * np.uint64(int(n_items))) >> s32).astype(np.int64)
        neg = np.where(inside(cand), neg, cand)
    return u.astype(np.int32), pos.astype(np.int32), neg.astype(np.int32)


def sum16(prod):
    """the definition's summation order over the last axis of an (n, rank) array of products -> (n,)"""
    n, rank = prod.shape
    r16 = -(-rank // 16)
    if r16 * 16 != rank:
        prod = np.concatenate([prod, np.zeros((n, r16 * 16 - rank))], axis=1)   # (+0.0 added to a partial changes nothing)
    prod = prod.reshape(n, r16, 16)
    v = np.zeros((n, 16))
    for q in range(r16):
        v = v + prod[:, q, :]
    v = v[:, :8] + v[:, 8:]
    v = v[:, :4] + v[:, 4:]
    v = v[:, :2] + v[:, 2:]
    return v[:, 0] + v[:, 1]


def bpr_exp(d):
    """E(d): the stated exponential, plain float64 arithmetic"""
    d = np.minimum(np.maximum(np.asarray(d, dtype=np.float64), -40.0), 40.0)
    kk = np.rint(d * _LOG2E)
    r = (d - kk * _LN2_HI) - kk * _LN2_LO
    p = np.full_like(r, _COEF[13])
    for n in range(12, -1, -1):
        p = p * r + _COEF[n]
    return np.ldexp(p, kk.astype(np.int64))


def _ordered_sums(dest, contrib, n_dest):
    """the definition's per-destination sums: dest (m,) in the order of the contributions, contrib (m, rank) float64
    -> (totals (n_dest, rank), counts (n_dest,))"""
    rank = contrib.shape[1]
    counts = np.bincount(dest, minlength=n_dest).astype(np.int64)
    totals = np.zeros((n_dest, rank))
    if not dest.size:
        return totals, counts
    order = np.argsort(dest, kind="stable")
    d_sorted = dest[order]
    first = np.concatenate([[0], np.cumsum(counts)])[d_sorted]
    pos = np.arange(dest.size, dtype=np.int64) - first
    chunk_of, t = pos // CHUNK, pos % CHUNK
    n_chunks = -(-counts // CHUNK)
    chunk0 = np.concatenate([[0], np.cumsum(n_chunks)])
    slot = chunk0[d_sorted] + chunk_of
    acc = np.zeros((int(chunk0[-1]), rank))
    for tt in range(int(t.max()) + 1):
        sel = np.flatnonzero(t == tt)
        acc[slot[sel]] = acc[slot[sel]] + contrib[order[sel]]
    slot_dest = np.repeat(np.arange(n_dest, dtype=np.int64), n_chunks)
    slot_m = np.arange(acc.shape[0], dtype=np.int64) - chunk0[slot_dest]
    for m in range(int(n_chunks.max())):
        sel = np.flatnonzero(slot_m == m)
        totals[slot_dest[sel]] = totals[slot_dest[sel]] + acc[sel]
    return totals, counts


def _apply(rows, a, totals, counts, lr, lam):
    """the update of the destinations with counts >= 1 -> (rows', a'), rows' in rows' dtype"""
    out, a2 = rows.copy(), a.copy()
    hit = np.flatnonzero(counts > 0)
    if not hit.size:
        return out, a2
    row = rows[hit].astype(np.float64)
    g = totals[hit] - (np.float64(lam) * counts[hit].astype(np.float64))[:, None] * row
    an = a[hit] + sum16(g * g) / np.float64(rows.shape[1])
    move = an != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        new = row + (np.float64(lr) * g) / np.sqrt(an)[:, None]
    out[hit[move]] = new[move].astype(rows.dtype)
    a2[hit] = an
    return out, a2


def step_from_z(U, V, aU, aV, u, i, j, z, diff, learning_rate, lambda_, update_items):
    """the rows, sums and updates of one step for the triples (u, i, j) (none void, int64) with their z and diff = V[i] - V[j] ->
    (U', V', aU', aV')"""
    rank = U.shape[1]
    tot_u, cnt_u = _ordered_sums(u, z[:, None] * diff, U.shape[0])
    U2, aU2 = _apply(U, aU, tot_u, cnt_u, learning_rate, lambda_)
    V2, aV2 = V.copy(), aV.copy()
    if update_items:
        Uu = U[u].astype(np.float64)
        dest = np.stack([i, j], axis=1).reshape(-1)
        contrib = np.stack([z[:, None] * Uu, (-z)[:, None] * Uu], axis=1).reshape(-1, rank)
        tot_v, cnt_v = _ordered_sums(dest, contrib, V.shape[0])
        V2, aV2 = _apply(V, aV, tot_v, cnt_v, learning_rate, lambda_)
    return U2, V2, aU2, aV2


def bpr_step_reference(U, V, aU, aV, tu, ti, tj, learning_rate, lambda_, update_items=True):
    """One step of the definition on the triples (tu, ti, tj) (in the order k; tj = -1: void) from the snapshot (U, V) with the
    Adagrad states (aU, aV) -> (U', V', aU', aV', n_valid, n_correct); nothing is changed in place."""
    U, V = np.asarray(U), np.asarray(V)
    aU, aV = np.asarray(aU, dtype=np.float64), np.asarray(aV, dtype=np.float64)
    keep = np.flatnonzero(np.asarray(tj) >= 0)
    u, i, j = (np.asarray(t, dtype=np.int64)[keep] for t in (tu, ti, tj))
    diff = V[i].astype(np.float64) - V[j].astype(np.float64)
    d = sum16(U[u].astype(np.float64) * diff)
    z = 1.0 / (1.0 + bpr_exp(d))
    return step_from_z(U, V, aU, aV, u, i, j, z, diff, learning_rate, lambda_, update_items) + (int(keep.size), int((d > 0).sum()))


def bpr_fit_reference(indptr, indices, n_items, U, V, n_iter, seed, learning_rate, lambda_, batch, mode=0, row0=0,
                      update_items=True, aU=None, aV=None, epoch0=0):
    """n_iter epochs of the definition from the factors (U, V) -> (U, V, aU, aV, trace), trace = [(n_valid, n_correct)] per epoch.
    mode 1 (the fold-in) takes one step per epoch whatever `batch` is."""
    ip = np.asarray(indptr, dtype=np.int64)
    U, V = np.array(U), np.array(V)
    aU = np.zeros(U.shape[0]) if aU is None else np.array(aU, dtype=np.float64)
    aV = np.zeros(V.shape[0]) if aV is None else np.array(aV, dtype=np.float64)
    n_steps = 1 if mode == 1 else n_steps_of(ip[-1], batch)
    trace = []
    for e in range(epoch0, epoch0 + int(n_iter)):
        nv = nc = 0
        for s in range(n_steps):
            t = bpr_triples(seed, mode, e, row0, ip, indices, n_items, s, n_steps)
            U, V, aU, aV, v, c = bpr_step_reference(U, V, aU, aV, *t, learning_rate, lambda_, update_items)
            nv, nc = nv + v, nc + c
        trace.append((nv, nc))
    return U, V, aU, aV, trace


def canonical_features(item_features, n_items, dtype):
    """item_features (anything scipy makes a matrix of, n_items rows) -> canonical CSR in `dtype`: duplicates summed, columns
    ascending, explicit zeros kept out, values finite"""
    F = sp.csr_matrix(item_features, dtype=np.float64)
    if F.shape[0] != int(n_items) or F.shape[1] < 1:
        raise ValueError("item_features must be n_items x n_feat with n_feat >= 1")
    F = sp.csr_matrix(F.astype(dtype))
    F.sum_duplicates()
    F.eliminate_zeros()
    F.sort_indices()
    if not np.isfinite(F.data).all():
        raise ValueError("item_features holds a value that is not finite in the factors' precision")
    return F


def compose_reference(F, H):
    """V = F H of the definition: per item its stored features in ascending order, sequentially from +0.0, one rounding into
    H's dtype.  F: canonical scipy CSR"""
    H = np.asarray(H)
    ip, idx, val = F.indptr.astype(np.int64), F.indices, F.data.astype(np.float64)
    acc, length = np.zeros((F.shape[0], H.shape[1])), np.diff(ip)
    for t in range(int(length.max()) if length.size else 0):
        rows = np.flatnonzero(length > t)
        acc[rows] = acc[rows] + val[ip[rows] + t][:, None] * H[idx[ip[rows] + t]].astype(np.float64)
    return acc.astype(H.dtype)


def _feature_sums(Fc, G, counts):
    """the definition's per-feature sums: Fc = F as canonical CSC, G (n_items, rank) and counts (n_items,) the items' totals
    and contribution counts -> (totals (n_feat, rank), C (n_feat,))"""
    n_feat, rank = Fc.shape[1], G.shape[1]
    cp, item, val = Fc.indptr.astype(np.int64), Fc.indices.astype(np.int64), Fc.data.astype(np.float64)
    length = np.diff(cp)
    col = np.repeat(np.arange(n_feat, dtype=np.int64), length)
    pos = np.arange(item.size, dtype=np.int64) - cp[col]
    live = counts[item] > 0
    C = np.zeros(n_feat, dtype=np.int64)
    np.add.at(C, col[live], counts[item[live]])
    n_chunks = -(-length // CHUNK)
    chunk0 = np.concatenate([[0], np.cumsum(n_chunks)])
    slot, t = chunk0[col] + pos // CHUNK, pos % CHUNK
    acc, totals = np.zeros((int(chunk0[-1]), rank)), np.zeros((n_feat, rank))
    for tt in range(CHUNK):
        sel = np.flatnonzero(live & (t == tt))
        acc[slot[sel]] = acc[slot[sel]] + val[sel][:, None] * G[item[sel]]
    slot_col = np.repeat(np.arange(n_feat, dtype=np.int64), n_chunks)
    slot_m = np.arange(acc.shape[0], dtype=np.int64) - chunk0[slot_col]
    for m in range(int(n_chunks.max()) if n_chunks.size else 0):
        sel = np.flatnonzero(slot_m == m)
        totals[slot_col[sel]] = totals[slot_col[sel]] + acc[sel]
    return totals, C


def feat_step_from_z(U, H, aU, aH, F, u, i, j, z, diff, learning_rate, lambda_):
    """the rows, sums and updates of one step through the features F (canonical CSR) for the triples (u, i, j) (none void,
    int64) with their z and diff = V[i] - V[j] of the composed V -> (U', H', aU', aH')"""
    rank = U.shape[1]
    tot_u, cnt_u = _ordered_sums(u, z[:, None] * diff, U.shape[0])
    U2, aU2 = _apply(U, aU, tot_u, cnt_u, learning_rate, lambda_)
    Uu = U[u].astype(np.float64)
    dest = np.stack([i, j], axis=1).reshape(-1)
    contrib = np.stack([z[:, None] * Uu, (-z)[:, None] * Uu], axis=1).reshape(-1, rank)
    G, cnt_v = _ordered_sums(dest, contrib, F.shape[0])
    Fc = sp.csc_matrix(F)
    Fc.sort_indices()
    tot_h, cnt_h = _feature_sums(Fc, G, cnt_v)
    H2, aH2 = _apply(H, aH, tot_h, cnt_h, learning_rate, lambda_)
    return U2, H2, aU2, aH2


def bpr_feat_step_reference(U, H, aU, aH, F, tu, ti, tj, learning_rate, lambda_):
    """One step of the definition through the item features F on the triples (tu, ti, tj) (in the order k; tj = -1: void) from
    the snapshot (U, H) with the Adagrad states (aU, aH) -> (U', H', aU', aH', n_valid, n_correct); nothing is changed in place.
    The gradient of a feature is scaled by F[i, f] (the modelled-on solver leaves the value out)."""
    U, H = np.asarray(U), np.asarray(H)
    aU, aH = np.asarray(aU, dtype=np.float64), np.asarray(aH, dtype=np.float64)
    V = compose_reference(F, H)
    keep = np.flatnonzero(np.asarray(tj) >= 0)
    u, i, j = (np.asarray(t, dtype=np.int64)[keep] for t in (tu, ti, tj))
    diff = V[i].astype(np.float64) - V[j].astype(np.float64)
    d = sum16(U[u].astype(np.float64) * diff)
    z = 1.0 / (1.0 + bpr_exp(d))
    return feat_step_from_z(U, H, aU, aH, F, u, i, j, z, diff, learning_rate, lambda_) + (int(keep.size), int((d > 0).sum()))


def bpr_feat_fit_reference(indptr, indices, F, U, H, n_iter, seed, learning_rate, lambda_, batch, aU=None, aH=None, epoch0=0):
    """n_iter epochs of the definition through the item features F (canonical CSR, n_items x n_feat) from (U, H) ->
    (U, H, aU, aH, trace), trace = [(n_valid, n_correct)] per epoch; the items are `compose_reference(F, H)`"""
    ip = np.asarray(indptr, dtype=np.int64)
    U, H = np.array(U), np.array(H)
    aU = np.zeros(U.shape[0]) if aU is None else np.array(aU, dtype=np.float64)
    aH = np.zeros(H.shape[0]) if aH is None else np.array(aH, dtype=np.float64)
    n_steps = n_steps_of(ip[-1], batch)
    trace = []
    for e in range(epoch0, epoch0 + int(n_iter)):
        nv = nc = 0
        for s in range(n_steps):
            t = bpr_triples(seed, 0, e, 0, ip, indices, F.shape[0], s, n_steps)
            U, H, aU, aH, v, c = bpr_feat_step_reference(U, H, aU, aH, F, *t, learning_rate, lambda_)
            nv, nc = nv + v, nc + c
        trace.append((nv, nc))
    return U, H, aU, aH, trace


def _check_args(rank, learning_rate, lambda_, batch, transform_iter):
    for name, v in (("rank", rank), ("batch", batch), ("transform_iter", transform_iter)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError("%s must be an integer >= 1" % name)
    learning_rate, lambda_ = float(learning_rate), float(lambda_)
    for name, v in (("learning_rate", learning_rate), ("lambda_", lambda_)):
        if not (np.isfinite(v) and v >= 0):
            raise ValueError("%s must be finite and >= 0" % name)
    return int(rank), learning_rate, lambda_, int(batch), int(transform_iter)


class BPR(WRMF):
    """Matrix factorisation on the BPR loss (the module's docstring is the definition).

    rank; learning_rate and lambda_: finite and >= 0; batch: the triples of one step of a fit; transform_iter: the epochs of a
    fold-in; precision "float" or "double": the dtype of the factors (the arithmetic is float64 either way); rng: a seed or a
    numpy Generator, from which ONE 63-bit seed is taken per fit for the initial factors and the triples.  A backend without
    `bpr_epochs` (the CPU stand-in of the tests) runs the numpy definition.
    Fitted: `components` (rank x n_items), `user_adagrad` / `item_adagrad` (float64), `trace` = [(n_valid, n_correct)] per epoch
    (n_correct / n_valid is the AUC estimate the modelled-on solver prints), `seed`.  `transform` / `predict` / `evaluate` and the
    rest of WRMF's surface fold the rows of x in with the items frozen; `explain` is not available.
    `fit_transform(x, item_features=F)` (F: scipy sparse, n_items x n_feat) fits the hybrid model of the module's docstring:
    `components` is then the composed (F H)', `feature_embeddings` / `feature_adagrad` hold H and aH (`item_adagrad` is None);
    `compose_items(F_new)` gives the embeddings of unseen items and `with_items(F_new)` a model whose catalogue they are."""

    def __init__(self, rank=10, learning_rate=0.1, lambda_=0.01, batch=4096, transform_iter=50, precision="float", rng=None,
                 device=None, backend=None):
        rank, self._lr, lam, self._batch, self._transform_iter = _check_args(rank, learning_rate, lambda_, batch, transform_iter)
        if precision == "double" and rank > _lib.MAX_RANK_F64 or rank > _lib.MAX_RANK:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "rank > %d is not on the device path"
                                           % (_lib.MAX_RANK_F64 if precision == "double" else _lib.MAX_RANK))
        super().__init__(rank=rank, lambda_=lam, dynamic_lambda=False, feedback="implicit", solver="cholesky", precision=precision,
                         rng=rng, device=device, backend=backend, factor_init="device")
        self.seed = None
        self.trace = []
        self.user_adagrad = self.item_adagrad = None
        self.feature_embeddings = self.feature_adagrad = None
        self._aV = self._H = None

    def _epochs(self, m, U, V, aU, aV, n_iter, mode, update_items):
        """n_iter epochs on the canonical rows m, in place where the backend has the kernels -> (U, V, aU, aV, trace)"""
        be = self._backend()
        if not hasattr(be, "bpr_epochs"):
            out = bpr_fit_reference(m.indptr, m.indices, m.shape[1], U.numpy(), V.numpy(), n_iter, self.seed, self._lr, self._lambda,
                                    self._batch, mode, 0, update_items, aU.numpy(), aV.numpy())
            return tuple(torch.from_numpy(np.ascontiguousarray(t)) for t in out[:4]) + (out[4],)
        p, j = be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32)
        counts = be.bpr_epochs(p, j, m.shape[1], m.nnz, 0, self.seed, mode, 0, n_iter, self._batch, U, V, aU, aV, self._lr, self._lambda,
                               update_items)
        return U, V, aU, aV, [(int(v), int(c)) for v, c in counts.cpu().numpy()]

    def _epochs_feat(self, m, F, U, H, aU, aH, n_iter):
        """n_iter epochs of a fit through the canonical item features F -> (U, H, aU, aH, V = F H, trace)"""
        be = self._backend()
        if not hasattr(be, "bpr_feat_epochs"):
            out = bpr_feat_fit_reference(m.indptr, m.indices, F, U.numpy(), H.numpy(), n_iter, self.seed, self._lr, self._lambda, self._batch)
            U, H, aU, aH = (torch.from_numpy(np.ascontiguousarray(t)) for t in out[:4])
            return U, H, aU, aH, torch.from_numpy(compose_reference(F, H.numpy())), out[4]
        p, j = be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32)
        feat = be.item_features(F, H.dtype)
        counts, _ = be.bpr_feat_epochs(p, j, m.nnz, 0, self.seed, 0, 0, n_iter, self._batch, feat, U, H, aU, aH, self._lr, self._lambda)
        return U, H, aU, aH, be.compose_rows(feat, H), [(int(v), int(c)) for v, c in counts.cpu().numpy()]

    def _fit_features(self, m, item_features, n_iter):
        n_user, n_item = m.shape
        be, k, tdt = self._backend(), self._rank, self._dev_t()
        F = canonical_features(item_features, n_item, self._dev_np())
        if hasattr(be, "init_factors"):
            U, H = be.init_factors(self.seed, _rng.STREAM_USERS, n_user, k, tdt), be.init_factors(self.seed, _rng.STREAM_ITEMS, F.shape[1], k, tdt)
        else:
            U, H = (be.to_device(_rng.init_factors(self.seed, s, 0, n, k, 0.01, dtype=self._dev_np()), tdt)
                    for s, n in ((_rng.STREAM_USERS, n_user), (_rng.STREAM_ITEMS, F.shape[1])))
        aU, aH = (torch.zeros(n, dtype=torch.float64, device=U.device) for n in (n_user, F.shape[1]))
        U, H, aU, aH, V, self.trace = self._epochs_feat(m, F, U, H, aU, aH, int(n_iter))
        self._drop_replicas(be)
        self._set_items(V, np.bincount(m.indices, minlength=n_item).astype(np.int64))
        self._H = H
        self.feature_embeddings, self.feature_adagrad = H.cpu().numpy().astype(self._np_dtype()), aH.cpu().numpy()
        self.user_adagrad, self.item_adagrad = aU.cpu().numpy(), None
        return U.cpu().numpy().astype(self._np_dtype())

    def _set_items(self, V, cnt_item):
        """the composed items V (frozen: a fold-in never reads their Adagrad state) as the model's catalogue"""
        self._V, self._aV = V, torch.zeros(V.shape[0], dtype=torch.float64, device=V.device)
        self._cnt_item = cnt_item
        self.components = V.cpu().numpy().T.astype(self._np_dtype())

    def compose_items(self, item_features):
        """the embeddings F_new H of items given by their features (n_new x n_feat) -> (n_new x rank); a model fitted with
        item_features only"""
        if self._H is None:
            raise RuntimeError("model is not fitted with item_features")
        return self._compose_device(item_features).cpu().numpy().astype(self._np_dtype())

    def _compose_device(self, item_features):
        be = self._backend()
        F = sp.csr_matrix(item_features)
        if F.shape[1] != self._H.shape[0]:
            raise ValueError("item_features must have the fitted model's n_feat columns")
        F = canonical_features(F, F.shape[0], self._dev_np())
        if not hasattr(be, "compose_rows"):
            return torch.from_numpy(compose_reference(F, self._H.numpy()))
        return be.compose_rows(be.item_features(F, self._H.dtype), self._H)

    def with_items(self, item_features):
        """a model with the same users' space whose catalogue is the items given by their features (n_new x n_feat): `predict`,
        `score`, `similar_items` and the rest then rank those items, cold-start ones included.  No item of it counts as seen in
        training."""
        import copy
        if self._H is None:
            raise RuntimeError("model is not fitted with item_features")
        V = self._compose_device(item_features)
        other = copy.copy(self)
        other._set_items(V, np.zeros(V.shape[0], dtype=np.int64))
        return other

    def fit_transform(self, x, n_iter=10, item_features=None):
        """n_iter epochs over the users x items matrix x -> the user factors (n_users x rank).  item_features (scipy sparse,
        n_items x n_feat): the items are composed from feature embeddings (the class docstring); None: a free row per item."""
        if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or n_iter < 0:
            raise ValueError("n_iter must be an integer >= 0")
        if self._dist()[0] > 1:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "BPR fits on one rank")
        m = canonical_pattern(x)
        n_user, n_item = m.shape
        be = self._backend()
        self.seed = int(self._rng.integers(2 ** 63))
        if item_features is not None:
            return self._fit_features(m, item_features, n_iter)
        self._H = self.feature_embeddings = self.feature_adagrad = None
        k, tdt = self._rank, self._dev_t()
        if hasattr(be, "init_factors"):
            U, V = be.init_factors(self.seed, _rng.STREAM_USERS, n_user, k, tdt), be.init_factors(self.seed, _rng.STREAM_ITEMS, n_item, k, tdt)
        else:
            U, V = (be.to_device(_rng.init_factors(self.seed, s, 0, n, k, 0.01, dtype=self._dev_np()), tdt)
                    for s, n in ((_rng.STREAM_USERS, n_user), (_rng.STREAM_ITEMS, n_item)))
        aU, aV = (torch.zeros(n, dtype=torch.float64, device=U.device) for n in (n_user, n_item))
        U, V, aU, aV, self.trace = self._epochs(m, U, V, aU, aV, int(n_iter), 0, True)
        self._drop_replicas(be)
        self._V, self._aV = V, aV
        self._cnt_item = np.bincount(m.indices, minlength=n_item).astype(np.int64)
        self.components = V.cpu().numpy().T.astype(self._np_dtype())
        self.user_adagrad, self.item_adagrad = aU.cpu().numpy(), aV.cpu().numpy()
        return U.cpu().numpy().astype(self._np_dtype())

    def _transform_device(self, x_csr):
        """the fold-in: `transform_iter` epochs of one step each on zero rows, the items frozen -> a device tensor"""
        if self._V is None:
            raise RuntimeError("model is not fitted")
        self._my_rows(x_csr)
        m = canonical_pattern(x_csr)
        U = torch.zeros((m.shape[0], self._rank), dtype=self._V.dtype, device=self._V.device)
        aU = torch.zeros(m.shape[0], dtype=torch.float64, device=self._V.device)
        if m.nnz:
            U = self._epochs(m, U, self._V, aU, self._aV, self._transform_iter, 1, False)[0]
        return U

    def transform(self, x):
        if self._V is None:
            raise RuntimeError("model is not fitted")
        x = sp.csr_matrix(x, dtype=np.float64)
        if x.shape[1] != self._V.shape[0]:
            raise ValueError("ncol(x) == ncol(self$components) is not TRUE")
        return self._transform_device(x).cpu().numpy().astype(self._np_dtype())

    def explain(self, x, pairs, n=None):
        raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "BPR has no per-user system to explain a score with")
