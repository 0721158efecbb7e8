"""Elastic-net generalised linear model by FTRL-proximal (McMahan et al. 2013, "Ad click prediction: a view from the trenches")
over a sparse samples x features matrix: the `FTRL` of the modelled-on package -- the first-order baseline beside
`FactorizationMachine`, on the same input -- in a form that has no race.  A mini-batch is taken from a snapshot of the state and
every sum has a fixed order, so a fit has the same bits on every run, in numpy and on the device.

The definition (include/rsparse_wrmf_hip.h repeats it for C hosts; wrmf_ftrl.hip runs it on the device).  Every arithmetic operation
is a separately rounded float64 operation on values widened from the model's dtype; nothing is fused.

Input.  x: `fm.canonical_design(x, dtype)`.  y: binomial takes {0, 1}; gaussian any finite value; poisson finite and >= 0.  weights
omega: finite and >= 0, default 1.

State.  z and n, one pair per feature in the model's dtype, both from +0.0.

Parameters.  alpha = learning_rate > 0, beta = learning_rate_decay > 0, lambda_ >= 0, l1_ratio in [0, 1] (l1 = lambda_ * l1_ratio,
l2 = lambda_ * (1 - l1_ratio), both formed once in float64), dropout in [0, 1), clip_grad = CLIP_GRAD = 1000.

Steps.  The factorization machine's rule: n_steps = ceil(n / batch); step s holds the rows r = s, s + n_steps, ... in ascending r,
numbered k.  Everything in a step is computed from the snapshot (z, n) at its start.  `epoch` starts at 0 and increases by one
per epoch over the life of the model.

    w_j         +0.0 where |z_j| <= l1, else (-1 / ((beta + sqrt(n_j)) / alpha + l2)) * (z_j - sgn(z_j) * l1)
    dropout     stream 8 of the Philox generator (rng.STREAM_FTRL): the entry at position t of row r takes word o[t & 3] of the
                call with counter (t >> 2, r, 8, epoch), key (lo32(seed), hi32(seed)); KEPT iff word >= T, T = floor(dropout *
                2^32); x' = x * keep_scale, keep_scale = 1.0 / (1.0 - dropout).  dropout = 0: everything kept, x' = x exactly
    tsum(list)  the list in its stated order is cut into chunks of 64 consecutive terms, a short last one padded with +0.0; a
                chunk is reduced by the tree v[t] = v[t] + v[t + 32], then the same with 16, 8, 4, 2, 1; the chunk sums are
                added sequentially to a total that starts at +0.0

Forward, row r with ALL its stored entries in ascending column:

    raw    tsum_e(w[j_e] * x'_e for a kept entry, +0.0 for a dropped one -- it keeps its place: nothing is compacted)
    p      binomial 1 / (1 + E(-raw)), gaussian raw, poisson E(raw);  E = `bpr_exp`, its clamp at +-40 part of the definition
    d      omega * (p - y)
    g_e    min(max(d * x'_e, -clip_grad), clip_grad) for a kept entry, +0.0 for a dropped one

Backward, column j, its stored entries of the step in ascending k:  G = tsum(g), Q = tsum(g * g), c = the KEPT entries.
Update of a column with c >= 1 (every other keeps its bits):

    nn = n_j + Q;  sigma = (sqrt(nn) - sqrt(n_j)) / alpha;  z_j' = z_j + (G - sigma * w_j);  n_j' = nn;  each rounded once

`partial_fit` returns p of every row as computed at its step's snapshot, with dropout: the progressive validation of the
modelled-on `partial_fit`.  `predict` is the forward pass without dropout; `coef()` is w.

Deliberate differences from the modelled-on solver (src/FTRL.cpp), a Hogwild OpenMP loop with racing double updates and a
thread-local twister -- other bits on every run:
  * mini-batches from a snapshot replace Hogwild: the per-sample n += g^2 and the telescoping sigma become Q and one sigma per
    column and step (equal in exact arithmetic for a fixed w); batch = 1, dropout = 0, gaussian is the plain per-sample loop bit
    for bit;
  * dropout comes from a counter-based stream;
  * x * keep_scale replaces x / (1 - dropout);
  * the exponential is stated;
  * all three families are reachable (the R class admits binomial only, its C++ has all three).

  tsum, ftrl_weights_reference, ftrl_keep_reference, ftrl_forward_reference, ftrl_step_reference, ftrl_fit_reference   the definition
  FTRL                                                                                                              the model
"""
import numpy as np
import torch

from . import _lib
from . import rng as _rng
from .bpr import bpr_exp, n_steps_of
from .fm import _entries, canonical_design, step_rows

FAMILIES = {"binomial": _lib.FTRL_BINOMIAL, "gaussian": _lib.FTRL_GAUSSIAN, "poisson": _lib.FTRL_POISSON}
CLIP_GRAD = _lib.FTRL_CLIP
CHUNK = 64


def tsum(dest, terms, n_dest):
    """the definition's sums per destination: dest (m,) in the order of the terms, terms (m,) float64 -> totals (n_dest,)"""
    dest, terms = np.asarray(dest, dtype=np.int64), np.asarray(terms, dtype=np.float64)
    totals = np.zeros(n_dest)
    if not dest.size:
        return totals
    counts = np.bincount(dest, minlength=n_dest).astype(np.int64)
    order = np.argsort(dest, kind="stable")
    d_sorted = dest[order]
    pos = np.arange(dest.size, dtype=np.int64) - np.concatenate([[0], np.cumsum(counts)])[d_sorted]
    n_chunks = -(-counts // CHUNK)
    chunk0 = np.concatenate([[0], np.cumsum(n_chunks)])
    v = np.zeros((int(chunk0[-1]), CHUNK))                                    # (the padding is +0.0)
    v[chunk0[d_sorted] + pos // CHUNK, pos % CHUNK] = terms[order]
    h = CHUNK // 2
    while h:
        v = v[:, :h] + v[:, h:]
        h //= 2
    slot_dest = np.repeat(np.arange(n_dest, dtype=np.int64), n_chunks)
    slot_m = np.arange(v.shape[0], dtype=np.int64) - chunk0[slot_dest]
    for m in range(int(n_chunks.max())):
        sel = np.flatnonzero(slot_m == m)
        totals[slot_dest[sel]] = totals[slot_dest[sel]] + v[sel, 0]
    return totals


def ftrl_weights_reference(z, n, alpha, beta, l1, l2):
    """w of the definition for the pairs (z, n) -> float64"""
    z, n = np.asarray(z).astype(np.float64), np.asarray(n).astype(np.float64)
    alpha, beta, l1, l2 = (np.float64(v) for v in (alpha, beta, l1, l2))
    w = (-1.0 / ((beta + np.sqrt(n)) / alpha + l2)) * (z - np.sign(z) * l1)
    return np.where(np.abs(z) <= l1, 0.0, w)


def ftrl_keep_reference(seed, epoch, indptr, rows, dropout):
    """the keep flags of the stored entries of `rows` in the order (k, position) -> bool; a function of (seed, epoch, row,
    position) alone"""
    seed, epoch = int(seed), int(epoch)
    if not (0 <= seed < 2 ** 64 and 0 <= epoch < 2 ** 31 and 0.0 <= float(dropout) < 1.0):
        raise ValueError("ftrl_keep_reference: bad arguments")
    ip, rows = np.asarray(indptr, dtype=np.int64), np.asarray(rows, dtype=np.int64)
    lens = ip[rows + 1] - ip[rows]
    r = np.repeat(rows, lens).astype(np.uint64)
    t = (np.arange(r.size, dtype=np.int64) - np.repeat(np.concatenate([[0], np.cumsum(lens)])[:-1], lens)).astype(np.uint64)
    counter = np.stack([t >> np.uint64(2), r, np.full_like(r, _rng.STREAM_FTRL), np.full_like(r, epoch)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    o = _rng.philox4x32_10(counter, key).astype(np.uint64)
    word = o[np.arange(r.size), (t & np.uint64(3)).astype(np.int64)] if r.size else np.zeros(0, dtype=np.uint64)
    return word >= np.uint64(int(np.floor(float(dropout) * 2.0 ** 32)))


def _link(raw, family):
    if family == "binomial":
        return 1.0 / (1.0 + bpr_exp(-raw))
    return bpr_exp(raw) if family == "poisson" else raw


def ftrl_forward_reference(indptr, indices, data, rows, z, n, family, alpha, beta, l1, l2, dropout=0.0, seed=0, epoch=0):
    """the forward pass of the definition on `rows` (in the order k) from the snapshot (z, n) -> (raw, p, (k_of, j, x', keep)):
    raw and p over k, the rest over the stored entries of the rows in the order (k, column)"""
    rows = np.asarray(rows, dtype=np.int64)
    k_of, j, x = _entries(indptr, indices, data, rows)
    keep = ftrl_keep_reference(seed, epoch, indptr, rows, dropout) if dropout else np.ones(x.size, dtype=bool)
    xs = x * np.float64(1.0 / (1.0 - float(dropout))) if dropout else x
    w = ftrl_weights_reference(z, n, alpha, beta, l1, l2)
    raw = tsum(k_of, np.where(keep, w[j] * xs, 0.0), rows.size)
    return raw, _link(raw, family), (k_of, j, xs, keep)


def ftrl_step_reference(indptr, indices, data, rows, y, omega, z, n, family, alpha, beta, l1, l2, dropout=0.0, seed=0, epoch=0):
    """One step of the definition on `rows` (y and omega are indexed by row) from the snapshot (z, n) -> (z', n', p over k, the kept
    count per column); nothing is changed in place"""
    z, n = np.asarray(z), np.asarray(n)
    rows = np.asarray(rows, dtype=np.int64)
    raw, p, (k_of, j, xs, keep) = ftrl_forward_reference(indptr, indices, data, rows, z, n, family, alpha, beta, l1, l2, dropout, seed, epoch)
    d = np.asarray(omega, dtype=np.float64)[rows] * (p - np.asarray(y, dtype=np.float64)[rows])
    g = np.where(keep, np.minimum(np.maximum(d[k_of] * xs, -CLIP_GRAD), CLIP_GRAD), 0.0)
    G, Q = tsum(j, g, z.size), tsum(j, g * g, z.size)
    kept = np.bincount(j[keep], minlength=z.size)
    zd, nd = z.astype(np.float64), n.astype(np.float64)
    nn = nd + Q
    sigma = (np.sqrt(nn) - np.sqrt(nd)) / np.float64(alpha)
    z2 = (zd + (G - sigma * ftrl_weights_reference(z, n, alpha, beta, l1, l2))).astype(z.dtype)
    return np.where(kept > 0, z2, z), np.where(kept > 0, nn.astype(n.dtype), n), p, kept


def ftrl_fit_reference(indptr, indices, data, y, omega, z, n, n_iter, batch, family, alpha, beta, lambda_, l1_ratio, dropout=0.0, seed=0,
                       epoch0=0):
    """n_iter epochs of the definition, numbered from epoch0 -> (z, n, p): p of every row at its step's snapshot in the LAST epoch"""
    rows_n = np.asarray(indptr).size - 1
    n_steps = n_steps_of(rows_n, batch)
    l1, l2 = np.float64(lambda_) * np.float64(l1_ratio), np.float64(lambda_) * (1.0 - np.float64(l1_ratio))
    z, n, p = np.array(z), np.array(n), np.zeros(rows_n)
    for e in range(int(n_iter)):
        for s in range(n_steps):
            rows = step_rows(rows_n, s, n_steps)
            z, n, p[rows], _ = ftrl_step_reference(indptr, indices, data, rows, y, omega, z, n, family, alpha, beta, l1, l2, dropout, seed,
                                                   int(epoch0) + e)
    return z, n, p


class FTRL:
    """Elastic-net GLM by FTRL-proximal (the module's docstring is the definition).

    learning_rate > 0 (alpha), learning_rate_decay > 0 (beta), lambda_ >= 0, l1_ratio in [0, 1], dropout in [0, 1); family
    "binomial", "gaussian" or "poisson"; batch: the rows of one step; precision "float" or "double": the dtype of z and n (the
    arithmetic is float64 either way); rng: a seed or a numpy Generator, from which ONE 63-bit seed is taken at the first fit for
    the dropout stream.  A backend without `ftrl_epochs` (the CPU stand-in of the tests) runs the numpy definition.
    `partial_fit(x, y, weights=None)` runs one epoch and returns p of every row at its step's snapshot (progressive validation);
    `fit(..., n_iter=)` runs n_iter epochs; `predict(x)` is the forward pass without dropout; `coef()` the weights (float64);
    `dump()` / `load(state)` carry the parameters, z, n, seed and epoch, so that a loaded model continues with the same bits.
    Fitted: `z`, `n`, `seed`, `epoch`."""

    def __init__(self, learning_rate=0.1, learning_rate_decay=0.5, lambda_=0.0, l1_ratio=1.0, dropout=0.0, family="binomial",
                 batch=1 << 16, precision="float", rng=None, device=None, backend=None):
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
            raise ValueError("batch must be an integer >= 1")
        for name, v in (("learning_rate", learning_rate), ("learning_rate_decay", learning_rate_decay)):
            if not (np.isfinite(float(v)) and float(v) > 0):
                raise ValueError("%s must be finite and > 0" % name)
        if not (np.isfinite(float(lambda_)) and float(lambda_) >= 0):
            raise ValueError("lambda_ must be finite and >= 0")
        if not 0.0 <= float(l1_ratio) <= 1.0:
            raise ValueError("l1_ratio must be in [0, 1]")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError("dropout must be in [0, 1)")
        if family not in FAMILIES:
            raise ValueError("family must be one of %s" % list(FAMILIES))
        if precision not in ("float", "double"):
            raise ValueError("precision must be 'double' or 'float'")
        self._par = dict(learning_rate=float(learning_rate), learning_rate_decay=float(learning_rate_decay), lambda_=float(lambda_),
                         l1_ratio=float(l1_ratio), dropout=float(dropout), family=family, batch=int(batch), precision=precision)
        self._rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        self._device, self._be = device, backend
        self._zn = None   # (d, 2): a tensor where the backend works, else numpy
        self.seed = None
        self.epoch = 0

    def _backend(self):
        if self._be is None:
            from .engine import HipBackend
            self._be = HipBackend(self._device)
        return self._be

    def _np(self):
        return np.float64 if self._par["precision"] == "double" else np.float32

    def _t(self):
        return torch.float64 if self._par["precision"] == "double" else torch.float32

    def _on_device(self):
        return hasattr(self._backend(), "ftrl_epochs")

    def _host_zn(self):
        return self._zn.cpu().numpy() if isinstance(self._zn, torch.Tensor) else self._zn

    def _set_zn(self, zn):
        zn = np.ascontiguousarray(zn, dtype=self._np())
        self._zn = self._backend().to_device(zn, self._t()) if self._on_device() else zn

    def _glm(self):
        """(family, alpha, beta, lambda_, l1_ratio) as the backend and the definition take them"""
        p = self._par
        return p["family"], p["learning_rate"], p["learning_rate_decay"], p["lambda_"], p["l1_ratio"]

    def _l12(self):
        lam, ratio = np.float64(self._par["lambda_"]), np.float64(self._par["l1_ratio"])
        return lam * ratio, lam * (1.0 - ratio)

    @property
    def z(self):
        return None if self._zn is None else self._host_zn()[:, 0].copy()

    @property
    def n(self):
        return None if self._zn is None else self._host_zn()[:, 1].copy()

    def _targets(self, m, y, weights):
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        if m.shape[0] != y.size:
            raise ValueError("nrow(x) == length(y) is not TRUE")
        if not np.isfinite(y).all():
            raise ValueError("!anyNA(y) is not TRUE")
        if self._par["family"] == "binomial" and not np.isin(y, (0.0, 1.0)).all():
            raise ValueError("binomial y must be in {0, 1}")
        if self._par["family"] == "poisson" and (y < 0).any():
            raise ValueError("poisson y must be >= 0")
        om = np.ones(y.size) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
        if om.size != y.size:
            raise ValueError("length(weights) == length(y) is not TRUE")
        if not (np.isfinite(om).all() and (om >= 0).all()):
            raise ValueError("weights must be finite and >= 0")
        return y, om

    def _csr(self, m):
        be = self._backend()
        return be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32), be.to_device(m.data, self._t())

    def _epochs(self, x, y, weights, n_iter):
        if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or n_iter < 0:
            raise ValueError("n_iter must be an integer >= 0")
        m = canonical_design(x, self._np(), None if self._zn is None else self._zn.shape[0])
        y, om = self._targets(m, y, weights)
        if self.epoch + int(n_iter) >= 2 ** 31:
            raise ValueError("the model has no epochs left (epoch < 2^31)")
        if self._zn is None:
            self.seed = int(self._rng.integers(2 ** 63))
            self._set_zn(np.zeros((m.shape[1], 2)))
        p, batch, dropout = np.zeros(m.shape[0]), self._par["batch"], self._par["dropout"]
        if not self._on_device():
            zn = self._zn
            z, n, p = ftrl_fit_reference(m.indptr, m.indices, m.data, y, om, zn[:, 0], zn[:, 1], int(n_iter), batch, *self._glm(), dropout,
                                         self.seed, self.epoch)
            self._zn = np.ascontiguousarray(np.stack([z, n], axis=1))
        elif m.shape[0] and n_iter:
            be, csr = self._backend(), self._csr(m)
            index = be.fm_index(csr[0], csr[1], m.shape[1], n_steps_of(m.shape[0], batch))
            p = be.ftrl_epochs(*csr, index, int(n_iter), *self._glm(), dropout, self.seed, self.epoch, be.to_device(y, torch.float64),
                               be.to_device(om, torch.float64), self._zn).cpu().numpy()
        self.epoch += int(n_iter)
        return p

    def partial_fit(self, x, y, weights=None):
        """one epoch, keeping the state -> p of every row at its step's snapshot, with dropout (float64)"""
        return self._epochs(x, y, weights, 1)

    def fit(self, x, y, weights=None, n_iter=1):
        """n_iter epochs over the samples x features matrix x with the targets y (and the sample weights) -> self; a fitted model
        goes on from its state and its epoch counter"""
        self._epochs(x, y, weights, n_iter)
        return self

    def predict(self, x):
        """the forward pass without dropout on every row of x: the probability of y = 1 (binomial), the value (gaussian) or the
        rate (poisson) -> float64"""
        if self._zn is None:
            raise RuntimeError("model is not fitted")
        m = canonical_design(x, self._np(), self._zn.shape[0])
        if not self._on_device():
            fam, alpha, beta = self._glm()[:3]
            return ftrl_forward_reference(m.indptr, m.indices, m.data, np.arange(m.shape[0]), self._zn[:, 0], self._zn[:, 1], fam, alpha,
                                          beta, *self._l12())[1]
        return self._backend().ftrl_predict(*self._csr(m), *self._glm(), self._zn).cpu().numpy()

    def coef(self):
        """w of every feature -> float64"""
        if self._zn is None:
            raise RuntimeError("model is not fitted")
        if not self._on_device():
            return ftrl_weights_reference(self._zn[:, 0], self._zn[:, 1], *self._glm()[1:3], *self._l12())
        return self._backend().ftrl_weights(*self._glm()[1:], self._zn).cpu().numpy()

    def dump(self):
        """the model as a dict: the parameters, z, n, seed and epoch"""
        return dict(self._par, z=self.z, n=self.n, seed=self.seed, epoch=self.epoch)

    def load(self, state):
        """take the parameters, z, n, seed and epoch of a `dump()` -> self; the next fit continues with the same bits"""
        state = dict(state)
        z, n, seed, epoch = (state.pop(k) for k in ("z", "n", "seed", "epoch"))
        other = FTRL(**state, device=self._device, backend=self._be)
        self._par, self.seed, self.epoch = other._par, (None if seed is None else int(seed)), int(epoch)
        self._zn = None
        if z is not None:
            if np.shape(z) != np.shape(n) or np.ndim(z) != 1 or self.seed is None:
                raise ValueError("z and n must be vectors of one length, with a seed")
            self._set_zn(np.stack([np.asarray(z), np.asarray(n)], axis=1))
        return self
