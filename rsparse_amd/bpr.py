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

  bpr_triples, bpr_exp, bpr_step_reference, bpr_fit_reference     the definition, in numpy
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


def bpr_triples(seed, mode, epoch, row0, indptr, indices, n_items, step=0, n_steps=1):
    """The triples of one step -> (u, i, j): int32 arrays over k, u the LOCAL row, j = -1 for a void triple.  (indptr, indices): a
    canonical CSR pattern whose row pointers start at 0; row0: the global index of its first row."""
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
    counter = np.stack([q, g, np.full_like(q, _rng.STREAM_BPR), np.full_like(q, epoch + (mode << 31))], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    o = _rng.philox4x32_10(counter, key).astype(np.uint64)
    s32 = np.uint64(32)
    pos = idx[ip[u] + ((o[:, 0] * L) >> s32).astype(np.int64)] if p.size else np.zeros(0, np.int64)
    # membership of a candidate in its row: the entries of a canonical pattern are sorted by (row, column)
    cells = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(ip)) * n_items + idx
    neg = np.full(p.size, -1, dtype=np.int64)
    for t in (3, 2, 1):
        cand = ((o[:, t] * np.uint64(n_items)) >> s32).astype(np.int64)
        want = u * n_items + cand
        at = np.searchsorted(cells, want)
        inside = (at < cells.size) & (cells[np.minimum(at, max(cells.size - 1, 0))] == want) if cells.size else np.zeros(p.size, bool)
        neg = np.where(inside, neg, cand)
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


def bpr_step_reference(U, V, aU, aV, tu, ti, tj, learning_rate, lambda_, update_items=True):
    """One step of the definition on the triples (tu, ti, tj) (in the order k; tj = -1: void) from the snapshot (U, V) with the
    Adagrad states (aU, aV) -> (U', V', aU', aV', n_valid, n_correct); nothing is changed in place."""
    U, V = np.asarray(U), np.asarray(V)
    aU, aV = np.asarray(aU, dtype=np.float64), np.asarray(aV, dtype=np.float64)
    keep = np.flatnonzero(np.asarray(tj) >= 0)
    u, i, j = (np.asarray(t, dtype=np.int64)[keep] for t in (tu, ti, tj))
    rank = U.shape[1]
    Uu = U[u].astype(np.float64)
    diff = V[i].astype(np.float64) - V[j].astype(np.float64)
    d = sum16(Uu * diff)
    z = 1.0 / (1.0 + bpr_exp(d))
    tot_u, cnt_u = _ordered_sums(u, z[:, None] * diff, U.shape[0])
    U2, aU2 = _apply(U, aU, tot_u, cnt_u, learning_rate, lambda_)
    V2, aV2 = V.copy(), aV.copy()
    if update_items:
        dest = np.stack([i, j], axis=1).reshape(-1)
        contrib = np.stack([z[:, None] * Uu, (-z)[:, None] * Uu], axis=1).reshape(-1, rank)
        tot_v, cnt_v = _ordered_sums(dest, contrib, V.shape[0])
        V2, aV2 = _apply(V, aV, tot_v, cnt_v, learning_rate, lambda_)
    return U2, V2, aU2, aV2, int(keep.size), int((d > 0).sum())


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
    rest of WRMF's surface fold the rows of x in with the items frozen; `explain` is not available."""

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
        self._aV = None

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

    def fit_transform(self, x, n_iter=10):
        """n_iter epochs over the users x items matrix x -> the user factors (n_users x rank)"""
        if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or n_iter < 0:
            raise ValueError("n_iter must be an integer >= 0")
        if self._dist()[0] > 1:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "BPR fits on one rank")
        m = canonical_pattern(x)
        n_user, n_item = m.shape
        be = self._backend()
        self.seed = int(self._rng.integers(2 ** 63))
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
