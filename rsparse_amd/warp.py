"""WARP (Weston, Bengio and Usunier 2011, "WSABIE: Scaling Up To Large Vocabulary Image Annotation"; `loss = "warp"` of the
modelled-on package's `RankMF`): BPR's deterministic mini-batch SGD (rsparse_amd/bpr.py) with a SEARCHED negative.  BPR takes the
first admissible candidate; WARP keeps drawing until one comes within `margin` of the positive and weights the update by how few
draws that took.

The definition (include/rsparse_wrmf_hip.h repeats it for C hosts; warp_search_kernel of wrmf_bpr.hip runs it on the device).
Everything not said here is BPR's: the input pattern, steps, slots, k, `dot`, E(d), the row order, chunks of 64, the update, modes 0
and 1, the initial factors.

Stream.  `rng.STREAM_WARP` = 7.  Slot p of the CSR stands in row u at position q = p - indptr[u] of L.  Philox CALL c of the slot has
counter (q, g, 7 + 256 c, epoch + 2^31 mode) and key (lo32(seed), hi32(seed)), g as in BPR (the third counter word of every other
stream is 0..6).  Word 0 of call 0 gives the positive, i = indices[indptr[u] + ((o0 L) >> 32)].  TRIAL t, 1 <= t <= T = max_trials
<= 64, is word t & 3 of call t >> 2; its candidate is c_t = (o n_items) >> 32.

Search, from the snapshot (U, V) at the start of the step, over the trials in ascending t:

    a candidate that is in the row is skipped (it still consumes its t, as in the modelled-on loop)
    an admissible candidate is scored: d_t = dot(U[u], V[i] - V[c_t])                    (the differences rounded first)
    the first admissible trial with d_t <= margin is the VIOLATOR; the search stops there:
        j = c_t,  t_k = t,  z_k = weights[t - 1] / (1 + E(d_t))
    no violator: the triple is VOID, j = -1, t_k = 0, z_k = 0, and takes no part in anything

`weights`: T finite doubles >= 0 of the caller; neither side calls a logarithm, which is why they can agree bit for bit.  The
model's table is `rank_weights(n_items, T)`: rho[t - 1] = log(2 + (n_items - 1) / t) / log(2 + n_items), the modelled-on solver's
rank weight (its estimate of the positive's rank after t draws, (n_items - 1) / t, through log1p(1 + .), over the same of n_items).

Rows, order, update: BPR's with this z_k.  Counts, four per epoch: n_valid (triples with a violator), n_looked (slots with at least
one admissible trial), n_correct (of those, the slots whose first admissible trial has d > 0: n_correct / n_looked is the AUC
estimate), n_scored (admissible trials scored, the violator included: n_scored / n_slots is the oversampling).

Not here: the `sigmoid` kernel, RMSprop, user and item feature matrices, per-role lambdas, and the classic hinge WARP without the
logistic factor.

Item features (`fit_transform(x, item_features=F)`): BPR's hybrid model (the docstring of rsparse_amd/bpr.py) with this search on
the composed items.

  rank_weights, warp_triples, warp_step_reference, warp_fit_reference     the definition, in numpy
  warp_feat_step_reference, warp_feat_fit_reference                       the same through item features
  WARP                                                                    the model: `BPR`'s surface on this loss
"""
import math

import numpy as np

from . import _lib
from . import rng as _rng
from .bpr import BPR, bpr_exp, compose_reference, feat_step_from_z, n_steps_of, step_from_z, step_slot_rows, sum16

MAX_TRIALS = _lib.WARP_MAX_TRIALS


def rank_weights(n_items, max_trials):
    """rho[t - 1] = log(2 + (n_items - 1) / t) / log(2 + n_items), t = 1 .. max_trials, in float64 on the host"""
    n = float(int(n_items))
    return np.array([math.log(2.0 + (n - 1.0) / float(t)) / math.log(2.0 + n) for t in range(1, int(max_trials) + 1)], dtype=np.float64)


def _check_search(max_trials, margin, weights, finite_margin=False):
    if isinstance(max_trials, bool) or not isinstance(max_trials, (int, np.integer)) or not 1 <= max_trials <= MAX_TRIALS:
        raise ValueError("max_trials must be an integer in [1, %d]" % MAX_TRIALS)
    margin = float(margin)
    if np.isnan(margin) or finite_margin and not np.isfinite(margin):
        raise ValueError("margin must be finite")
    if weights is not None:
        weights = np.asarray(weights, dtype=np.float64)
        if weights.shape != (int(max_trials),) or not (np.isfinite(weights).all() and (weights >= 0).all()):
            raise ValueError("weights: max_trials finite values >= 0")
    return int(max_trials), margin, weights


def warp_triples(seed, mode, epoch, row0, indptr, indices, n_items, U, V, max_trials, margin, weights, step=0, n_steps=1):
    """The search of one step from the factors (U, V) -> (u, i, j, t, z, scored, (n_looked, n_correct, n_scored)): over k, u the
    LOCAL row (int32), the positive, the violator (-1: void), its trial (0: void), z (float64; 0: void) and the trials the slot
    scored (t - scored: the in-row candidates it skipped on the way).  (the definition takes margin = +-inf too; the device
    entries refuse it)"""
    T, margin, w = _check_search(max_trials, margin, weights)
    u, L, qg, key, idx, ip, inside = step_slot_rows(seed, mode, epoch, row0, indptr, indices, n_items, step, n_steps)
    U, V = np.asarray(U), np.asarray(V)
    c3, s32, n = int(epoch) + (int(mode) << 31), np.uint64(32), u.size

    def call(c):
        tail = np.broadcast_to(np.array([_rng.STREAM_WARP + 256 * c, c3], dtype=np.uint64), qg.shape)
        return _rng.philox4x32_10(np.concatenate([qg, tail], axis=-1), key).astype(np.uint64)

    o = call(0)
    pos = idx[ip[u] + ((o[:, 0] * L) >> s32).astype(np.int64)] if n else np.zeros(0, np.int64)
    Uu, Vi = U[u].astype(np.float64), V[pos].astype(np.float64)
    neg, tk, dk = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n)
    searching, seen = np.ones(n, dtype=bool), np.zeros(n, dtype=bool)
    scored, n_correct = np.zeros(n, dtype=np.int64), 0
    for t in range(1, T + 1):
        if t & 3 == 0:
            o = call(t >> 2)
        cand = ((o[:, t & 3] * np.uint64(int(n_items))) >> s32).astype(np.int64)
        sc = np.flatnonzero(searching & ~inside(cand))
        d = sum16(Uu[sc] * (Vi[sc] - V[cand[sc]].astype(np.float64)))
        scored[sc] += 1
        n_correct += int((d[~seen[sc]] > 0).sum())
        seen[sc] = True
        hit = sc[d <= margin]
        neg[hit], tk[hit], dk[hit] = cand[hit], t, d[d <= margin]
        searching[hit] = False
    z = np.where(tk > 0, w[np.maximum(tk, 1) - 1] / (1.0 + bpr_exp(dk)), 0.0)
    return (u.astype(np.int32), pos.astype(np.int32), neg.astype(np.int32), tk.astype(np.int32), z, scored.astype(np.int32),
            (int(seen.sum()), n_correct, int(scored.sum())))


def warp_step_reference(U, V, aU, aV, seed, mode, epoch, row0, indptr, indices, max_trials, margin, weights, learning_rate, lambda_,
                        update_items=True, step=0, n_steps=1):
    """One step of the definition from the snapshot (U, V) with the Adagrad states (aU, aV) ->
    (U', V', aU', aV', n_valid, n_looked, n_correct, n_scored); nothing is changed in place."""
    U, V = np.asarray(U), np.asarray(V)
    aU, aV = np.asarray(aU, dtype=np.float64), np.asarray(aV, dtype=np.float64)
    tu, ti, tj, _, z, _, counts = warp_triples(seed, mode, epoch, row0, indptr, indices, V.shape[0], U, V, max_trials, margin, weights,
                                               step, n_steps)
    keep = np.flatnonzero(tj >= 0)
    u, i, j = (t.astype(np.int64)[keep] for t in (tu, ti, tj))
    diff = V[i].astype(np.float64) - V[j].astype(np.float64)
    return step_from_z(U, V, aU, aV, u, i, j, z[keep], diff, learning_rate, lambda_, update_items) + (int(keep.size),) + counts


def warp_fit_reference(indptr, indices, n_items, U, V, n_iter, seed, max_trials, margin, weights, learning_rate, lambda_, batch, mode=0,
                       row0=0, update_items=True, aU=None, aV=None, epoch0=0):
    """n_iter epochs of the definition from the factors (U, V) -> (U, V, aU, aV, trace),
    trace = [(n_valid, n_looked, n_correct, n_scored)] per epoch.  mode 1 (the fold-in) takes one step per epoch."""
    ip = np.asarray(indptr, dtype=np.int64)
    U, V = np.array(U), np.array(V)
    aU = np.zeros(U.shape[0]) if aU is None else np.array(aU, dtype=np.float64)
    aV = np.zeros(V.shape[0]) if aV is None else np.array(aV, dtype=np.float64)
    n_steps = 1 if mode == 1 else n_steps_of(ip[-1], batch)
    trace = []
    for e in range(epoch0, epoch0 + int(n_iter)):
        total = np.zeros(4, dtype=np.int64)
        for s in range(n_steps):
            out = warp_step_reference(U, V, aU, aV, seed, mode, e, row0, ip, indices, max_trials, margin, weights, learning_rate, lambda_,
                                      update_items, s, n_steps)
            U, V, aU, aV = out[:4]
            total += np.array(out[4:], dtype=np.int64)
        trace.append(tuple(int(c) for c in total))
    return U, V, aU, aV, trace


def warp_feat_step_reference(U, H, aU, aH, F, seed, epoch, indptr, indices, max_trials, margin, weights, learning_rate, lambda_, step=0,
                             n_steps=1):
    """One step of the definition through the item features F (canonical CSR; rsparse_amd.bpr has the feature side) from the
    snapshot (U, H) -> (U', H', aU', aH', n_valid, n_looked, n_correct, n_scored); nothing is changed in place."""
    U, H = np.asarray(U), np.asarray(H)
    aU, aH = np.asarray(aU, dtype=np.float64), np.asarray(aH, dtype=np.float64)
    V = compose_reference(F, H)
    tu, ti, tj, _, z, _, counts = warp_triples(seed, 0, epoch, 0, indptr, indices, V.shape[0], U, V, max_trials, margin, weights, step, n_steps)
    keep = np.flatnonzero(tj >= 0)
    u, i, j = (t.astype(np.int64)[keep] for t in (tu, ti, tj))
    diff = V[i].astype(np.float64) - V[j].astype(np.float64)
    return feat_step_from_z(U, H, aU, aH, F, u, i, j, z[keep], diff, learning_rate, lambda_) + (int(keep.size),) + counts


def warp_feat_fit_reference(indptr, indices, F, U, H, n_iter, seed, max_trials, margin, weights, learning_rate, lambda_, batch, aU=None,
                            aH=None, epoch0=0):
    """n_iter epochs of the definition through the item features F from (U, H) -> (U, H, aU, aH, trace),
    trace = [(n_valid, n_looked, n_correct, n_scored)] per epoch"""
    ip = np.asarray(indptr, dtype=np.int64)
    U, H = np.array(U), np.array(H)
    aU = np.zeros(U.shape[0]) if aU is None else np.array(aU, dtype=np.float64)
    aH = np.zeros(H.shape[0]) if aH is None else np.array(aH, dtype=np.float64)
    n_steps = n_steps_of(ip[-1], batch)
    trace = []
    for e in range(epoch0, epoch0 + int(n_iter)):
        total = np.zeros(4, dtype=np.int64)
        for s in range(n_steps):
            out = warp_feat_step_reference(U, H, aU, aH, F, seed, e, ip, indices, max_trials, margin, weights, learning_rate, lambda_, s,
                                           n_steps)
            U, H, aU, aH = out[:4]
            total += np.array(out[4:], dtype=np.int64)
        trace.append(tuple(int(c) for c in total))
    return U, H, aU, aH, trace


class WARP(BPR):
    """Matrix factorisation on the WARP loss (the module's docstring is the definition): `BPR` with max_trials (1 .. 64) draws per
    slot at most and a finite margin.  Fitted, beyond BPR's: `trace` = [(n_valid, n_looked, n_correct, n_scored)] per epoch and
    `rank_weights`, the table that was used.  The fold-in searches too, with the items frozen.  A backend without `warp_epochs`
    runs the numpy definition."""

    def __init__(self, rank=10, learning_rate=0.1, lambda_=0.01, batch=4096, max_trials=50, margin=0.1, transform_iter=50,
                 precision="float", rng=None, device=None, backend=None):
        self._max_trials, self._margin, _ = _check_search(max_trials, margin, None, finite_margin=True)
        super().__init__(rank=rank, learning_rate=learning_rate, lambda_=lambda_, batch=batch, transform_iter=transform_iter,
                         precision=precision, rng=rng, device=device, backend=backend)
        self.rank_weights = None

    def _epochs(self, m, U, V, aU, aV, n_iter, mode, update_items):
        import torch
        be = self._backend()
        T, margin = self._max_trials, self._margin
        self.rank_weights = w = rank_weights(m.shape[1], T)
        if not hasattr(be, "warp_epochs"):
            out = warp_fit_reference(m.indptr, m.indices, m.shape[1], U.numpy(), V.numpy(), n_iter, self.seed, T, margin, w, self._lr,
                                     self._lambda, self._batch, mode, 0, update_items, aU.numpy(), aV.numpy())
            return tuple(torch.from_numpy(np.ascontiguousarray(t)) for t in out[:4]) + (out[4],)
        p, j = be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32)
        counts = be.warp_epochs(p, j, m.shape[1], m.nnz, 0, self.seed, mode, 0, n_iter, self._batch, T, margin, w, U, V, aU, aV, self._lr,
                                self._lambda, update_items)
        return U, V, aU, aV, [tuple(int(c) for c in row) for row in counts.cpu().numpy()]

    def _epochs_feat(self, m, F, U, H, aU, aH, n_iter):
        import torch
        be = self._backend()
        T, margin = self._max_trials, self._margin
        self.rank_weights = w = rank_weights(m.shape[1], T)
        if not hasattr(be, "warp_feat_epochs"):
            out = warp_feat_fit_reference(m.indptr, m.indices, F, U.numpy(), H.numpy(), n_iter, self.seed, T, margin, w, self._lr,
                                          self._lambda, self._batch)
            U, H, aU, aH = (torch.from_numpy(np.ascontiguousarray(t)) for t in out[:4])
            return U, H, aU, aH, torch.from_numpy(compose_reference(F, H.numpy())), out[4]
        p, j = be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32)
        feat = be.item_features(F, H.dtype)
        counts, _ = be.warp_feat_epochs(p, j, m.nnz, 0, self.seed, 0, 0, n_iter, self._batch, T, margin, w, feat, U, H, aU, aH, self._lr,
                                        self._lambda)
        return U, H, aU, aH, be.compose_rows(feat, H), [tuple(int(c) for c in row) for row in counts.cpu().numpy()]
