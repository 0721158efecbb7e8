"""GloVe (Pennington, Socher, Manning 2014, "GloVe: Global Vectors for Word Representation") over a square co-occurrence matrix,
trained by deterministic mini-batch SGD with a per-coordinate Adagrad state: the `GloVe` of the modelled-on package, in a form that
has no race.  A mini-batch is taken from a snapshot of the parameters and every gradient coordinate is summed per destination in a
fixed order, so a fit has the same bits on every run, in numpy and on the device.  Inside this project the matrix is an item
co-occurrence (x' x of an interaction matrix) and the vectors are item embeddings.

The definition (include/rsparse_wrmf_hip.h repeats it for C hosts; wrmf_glove.hip runs it on the device).  Every arithmetic
operation is a separately rounded float64 operation on parameters widened from the model's dtype; nothing is fused.

Input.  x: n x n, made canonical CSR: duplicates summed, columns ascending.  Every stored value must be finite and > 0 (a stored zero
is a stored value).  n < 2^31 and nnz < 2^31.  If every stored entry lies on one side of the diagonal or on it, x is replaced by
x + x' with the diagonal kept once.  Per stored position p, in float64 numpy, each rounded once into the model's dtype:

    fx[p] = (x / x_max) ** alpha if x < x_max else 1.0          lx[p] = log(x)

The steps consume rows[p] (the row of position p, int32), cols[p], fx[p] and lx[p]; no transcendental is evaluated on the device.

Parameters.  W_i, W_j (n x rank) and b_i, b_j (n) in the model's dtype, each with a float64 Adagrad state aW_i, aW_j, ab_i, ab_j that
starts at 1.0.  W_i starts from `rng.init_factors(seed, STREAM_USERS, 0, n, rank, 0.1)`, W_j likewise from STREAM_ITEMS, the biases
from 0; `init` overrides any of them.

Steps.  n_steps = ceil(nnz / batch).  Step s holds the stored positions p = s, s + n_steps, ... in ascending p; k = 0, 1, ... numbers
them (BPR's rule for its slots), so the slots of one row are a contiguous run of k.  Everything in a step is computed from the
snapshot at its start.  Per slot k with (r, c) = (rows[p], cols[p]):

    dot    BPR's `dot` order over q of W_i[r, q] * W_j[c, q]: 16 partials over q = l, l + 16, ... then the 8/4/2/1 tree
    inner  clip(((dot + b_i[r]) + b_j[c]) - lx[p], -100, 100)
    cost   fx[p] * inner
    term   cost * inner

    osum(list)  BPR's ordered sum: the list in its stated order is cut into chunks of CHUNK = 64 consecutive terms; a chunk is
                summed sequentially from +0.0; the chunk sums are added sequentially to a total that starts at +0.0

Per destination, the contributions in ascending k:

    row r,    coordinate q   osum_k(cost_k * W_j[c_k, q])     bias b_i[r]: osum_k(cost_k)     count = the slots of r in the step
    column c, coordinate q   osum_k(cost_k * W_i[r_k, q])     bias b_j[c]: osum_k(cost_k)     count = the slots of c in the step
    update                   `fm._adagrad` per coordinate theta with state a and count >= 1 (every other coordinate keeps its
                             bits): g = total + (lambda * count) * theta;  a' = a + g * g;  theta' = theta - (lr * g) / sqrt(a')
                             unless a' == 0, rounded once into the dtype.  lambda = lambda_ for W, 0 for b.

A diagonal entry (r = c) contributes to W_i[r] and to W_j[r] like any other entry.

Trace.  A step's term is 0.5 * osum_k(term_k); an epoch's cost is the sequential sum of its steps' terms from +0.0 (halving is
exact, so this is 0.5 * the sum of the osums).  `cost_history` holds it divided by nnz.

Deliberate differences from the modelled-on solver (src/GloVe.cpp), which is a Hogwild OpenMP loop -- racing float updates, other
bits on every run:
  * mini-batches from a snapshot replace Hogwild;
  * the Adagrad state is added to before the division (there: divided first);
  * lambda_ is an L2 term that scales with the count (there `lambda` is parsed and never used);
  * there is no `shuffle`: the strided steps already spread every step over all rows;
  * a triangular input is symmetrised once, so the diagonal is visited once per epoch and not twice;
  * the initial values are normal with scale 0.1 and zero biases (there: uniform in [-0.5, 0.5]).

  cooccurrence_slots, glove_slots_reference, glove_step_reference, glove_fit_reference     the definition, in numpy
  GloVe                                                                                    the model
"""
import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from . import rng as _rng
from .bpr import _ordered_sums, n_steps_of, step_slots, sum16
from .fm import _adagrad

MAX_RANK = _lib.GLOVE_MAX_RANK
CLIP_VALUE = 100.0
NAN_MESSAGE = "Cost becomes NaN, try to use smaller learning_rate."


def cooccurrence_slots(x, dtype, x_max, alpha):
    """x (anything scipy makes a matrix of, square) -> (rows int32, cols int32, fx, lx, n): the stored positions of the canonical
    (and, for a triangular x, symmetrised) matrix in CSR order, with the weights and the logarithms rounded once into `dtype`"""
    m = sp.csr_matrix(x, dtype=np.float64)
    m.sum_duplicates()
    if m.shape[0] != m.shape[1]:
        raise ValueError("ncol(x) == nrow(x) is not TRUE")
    if not (np.isfinite(m.data).all() and (m.data > 0).all()):
        raise ValueError("all(x@x > 0) is not TRUE: every stored value must be finite and > 0")
    n = m.shape[0]
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(m.indptr))
    if (rows <= m.indices).all():
        m = sp.csr_matrix(m + sp.triu(m, 1).T)
    elif (rows >= m.indices).all():
        m = sp.csr_matrix(m + sp.tril(m, -1).T)
    m.sort_indices()
    if n >= 2 ** 31 or m.nnz >= 2 ** 31:
        raise ValueError("x must have n < 2^31 and fewer than 2^31 stored entries")
    v = m.data.astype(np.float64)
    with np.errstate(over="ignore"):
        fx = np.where(v < np.float64(x_max), (v / np.float64(x_max)) ** np.float64(alpha), 1.0).astype(dtype)
        lx = np.log(v).astype(dtype)
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(m.indptr))
    return rows, m.indices.astype(np.int32), fx, lx, n


def glove_slots_reference(rows, cols, fx, lx, slots, W_i, W_j, b_i, b_j):
    """the per-slot quantities of the definition at the positions `slots` (in the order k) -> (inner, cost, term), float64"""
    r, c = np.asarray(rows, dtype=np.int64)[slots], np.asarray(cols, dtype=np.int64)[slots]
    dot = sum16(np.asarray(W_i)[r].astype(np.float64) * np.asarray(W_j)[c].astype(np.float64))
    raw = ((dot + np.asarray(b_i)[r].astype(np.float64)) + np.asarray(b_j)[c].astype(np.float64)) - np.asarray(lx)[slots].astype(np.float64)
    inner = np.where(raw < -CLIP_VALUE, -CLIP_VALUE, np.where(raw > CLIP_VALUE, CLIP_VALUE, raw))
    cost = np.asarray(fx)[slots].astype(np.float64) * inner
    return inner, cost, cost * inner


def glove_step_reference(rows, cols, fx, lx, slots, W_i, W_j, b_i, b_j, aW_i, aW_j, ab_i, ab_j, learning_rate, lambda_):
    """One step of the definition on the positions `slots` (in the order k) from the snapshot (W_i, W_j, b_i, b_j) with the Adagrad
    states -> (W_i', W_j', b_i', b_j', aW_i', aW_j', ab_i', ab_j', the step's trace term); nothing is changed in place."""
    W_i, W_j, b_i, b_j = (np.asarray(t) for t in (W_i, W_j, b_i, b_j))
    aW_i, aW_j, ab_i, ab_j = (np.asarray(t, dtype=np.float64) for t in (aW_i, aW_j, ab_i, ab_j))
    slots = np.asarray(slots, dtype=np.int64)
    n = W_i.shape[0]
    r, c = np.asarray(rows, dtype=np.int64)[slots], np.asarray(cols, dtype=np.int64)[slots]
    _, cost, term = glove_slots_reference(rows, cols, fx, lx, slots, W_i, W_j, b_i, b_j)
    out = []
    for dest, src, W, b, aW, ab in ((r, c, W_i, b_i, aW_i, ab_i), (c, r, W_j, b_j, aW_j, ab_j)):
        other = W_j if W is W_i else W_i
        tot, cnt = _ordered_sums(dest, cost[:, None] * other[src].astype(np.float64), n)
        lin = _ordered_sums(dest, cost[:, None], n)[0][:, 0]
        out.append(_adagrad(W, aW, tot, cnt[:, None], learning_rate, lambda_) + _adagrad(b, ab, lin, cnt, learning_rate, 0.0))
    (W_i2, aW_i2, b_i2, ab_i2), (W_j2, aW_j2, b_j2, ab_j2) = out
    total = _ordered_sums(np.zeros(slots.size, dtype=np.int64), term[:, None], 1)[0][0, 0]
    return W_i2, W_j2, b_i2, b_j2, aW_i2, aW_j2, ab_i2, ab_j2, float(0.5 * total)


def glove_fit_reference(rows, cols, fx, lx, W_i, W_j, b_i, b_j, aW_i, aW_j, ab_i, ab_j, n_iter, batch, learning_rate, lambda_):
    """n_iter epochs of the definition -> (W_i, W_j, b_i, b_j, aW_i, aW_j, ab_i, ab_j, trace), trace = the cost of every epoch
    (not yet divided by nnz)"""
    nnz = np.asarray(rows).size
    n_steps = n_steps_of(nnz, batch)
    state = tuple(np.array(t) for t in (W_i, W_j, b_i, b_j)) + tuple(np.array(t, dtype=np.float64) for t in (aW_i, aW_j, ab_i, ab_j))
    trace = []
    for _ in range(int(n_iter)):
        tot = 0.0
        for s in range(n_steps if nnz else 0):
            *state, term = glove_step_reference(rows, cols, fx, lx, step_slots(nnz, s, n_steps), *state, learning_rate, lambda_)
            tot = tot + term
        trace.append(tot)
    return (*state, trace)


class GloVe:
    """GloVe embeddings of a square co-occurrence matrix (the module's docstring is the definition).

    rank >= 1 (<= 128 on the device); x_max > 0 and alpha: the weighting function; learning_rate > 0; lambda_ >= 0; batch: the stored
    entries of one step; precision "float" or "double": the dtype of the parameters (the arithmetic is float64 either way); rng: a seed
    or a numpy Generator, from which ONE 63-bit seed is taken at the first fit; init: a dict with any of "w_i", "w_j" (rank x n) and
    "b_i", "b_j" (n), as the modelled-on class takes them.  A backend without `glove_epochs` (the CPU stand-in of the tests) runs the
    numpy definition.
    `fit_transform(x, n_iter=10, convergence_tol=-1)` returns W_i (n x rank); a fitted model goes on from its parameters and states.
    Fitted: `components` (W_j transposed, rank x n), `bias_i`, `bias_j`, `adagrad_w_i`, `adagrad_w_j` (rank x n), `adagrad_b_i`,
    `adagrad_b_j` (float64), `cost_history` / `get_history()`, `seed`.  `most_similar(ids, k, which=)`: cosine neighbours."""

    def __init__(self, rank, x_max, learning_rate=0.15, alpha=0.75, lambda_=0.0, batch=1 << 18, precision="float", rng=None, init=None,
                 device=None, backend=None):
        for name, v in (("rank", rank), ("batch", batch)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError("%s must be an integer >= 1" % name)
        for name, v, strict in (("x_max", x_max, True), ("learning_rate", learning_rate, True), ("lambda_", lambda_, False)):
            v = float(v)
            if not (np.isfinite(v) and v >= 0 and (v > 0 or not strict)):
                raise ValueError("%s must be finite and %s 0" % (name, ">" if strict else ">="))
        if not np.isfinite(float(alpha)):
            raise ValueError("alpha must be finite")
        if precision not in ("float", "double"):
            raise ValueError("precision must be 'double' or 'float'")
        init = dict(init or {})
        if not set(init) <= {"w_i", "b_i", "w_j", "b_j"}:
            raise ValueError("init takes w_i, b_i, w_j and b_j")
        if rank > MAX_RANK:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "rank > %d is not on the device path" % MAX_RANK)
        self._rank, self._batch, self._precision = int(rank), int(batch), precision
        self._x_max, self._alpha, self._lr, self._lam = float(x_max), float(alpha), float(learning_rate), float(lambda_)
        self._init = {k: v for k, v in init.items() if v is not None}
        self._rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        self._device, self._be = device, backend
        self._state = None   # (W_i, W_j, b_i, b_j, aW_i, aW_j, ab_i, ab_j): tensors where the backend works
        self.seed = None
        self.cost_history = []
        self.components = self.bias_i = self.bias_j = self._w_i = None
        self.adagrad_w_i = self.adagrad_w_j = self.adagrad_b_i = self.adagrad_b_j = None

    def _backend(self):
        if self._be is None:
            from .engine import HipBackend
            self._be = HipBackend(self._device)
        return self._be

    def _np(self):
        return np.float64 if self._precision == "double" else np.float32

    def _t(self):
        return torch.float64 if self._precision == "double" else torch.float32

    def _initial(self, n):
        be, k, tdt, ndt = self._backend(), self._rank, self._t(), self._np()
        self.seed = int(self._rng.integers(2 ** 63))
        up = getattr(be, "to_device", lambda a, dt: torch.as_tensor(a, dtype=dt).contiguous())
        out = []
        for name, stream in (("w_i", _rng.STREAM_USERS), ("w_j", _rng.STREAM_ITEMS)):
            if name in self._init:
                w = np.asarray(self._init[name], dtype=np.float64)
                if w.shape != (k, n):
                    raise ValueError("init values provided in the constructor don't match expected dimensions from the input matrix")
                out.append(up(np.ascontiguousarray(w.T).astype(ndt), tdt))
            elif hasattr(be, "glove_epochs"):
                out.append(be.init_factors(self.seed, stream, n, k, tdt, scale=0.1))
            else:
                out.append(up(_rng.init_factors(self.seed, stream, 0, n, k, 0.1, dtype=ndt), tdt))
        for name in ("b_i", "b_j"):
            b = np.asarray(self._init.get(name, np.zeros(n)), dtype=np.float64).reshape(-1)
            if b.size != n:
                raise ValueError("init values provided in the constructor don't match expected dimensions from the input matrix")
            out.append(up(b.astype(ndt), tdt))
        dev = out[0].device
        out += [torch.ones(s, dtype=torch.float64, device=dev) for s in ((n, k), (n, k), n, n)]
        return tuple(out)

    def _publish(self):
        W_i, W_j, b_i, b_j, aW_i, aW_j, ab_i, ab_j = (t.cpu().numpy() for t in self._state)
        self._w_i, self.components, self.bias_i, self.bias_j = W_i.copy(), W_j.T.copy(), b_i.copy(), b_j.copy()
        self.adagrad_w_i, self.adagrad_w_j, self.adagrad_b_i, self.adagrad_b_j = aW_i.T.copy(), aW_j.T.copy(), ab_i.copy(), ab_j.copy()

    def fit_transform(self, x, n_iter=10, convergence_tol=-1):
        """up to n_iter epochs over the co-occurrence matrix x -> W_i (n x rank).  Stops early when
        cost_history[-2] / cost_history[-1] - 1 < convergence_tol, as the modelled-on class does."""
        if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or n_iter < 0:
            raise ValueError("n_iter must be an integer >= 0")
        rows, cols, fx, lx, n = cooccurrence_slots(x, self._np(), self._x_max, self._alpha)
        if self._state is not None and self._state[0].shape[0] != n:
            raise ValueError("x has another size than the matrix the model was fitted on")
        if self._state is None:
            self._state = self._initial(n)
        be, nnz = self._backend(), rows.size
        device = hasattr(be, "glove_epochs")
        if device and nnz:
            d = (be.to_device(rows, torch.int32), be.to_device(cols, torch.int32), be.to_device(fx, self._t()), be.to_device(lx, self._t()))
            index = be.glove_index(d[0], d[1], n, n_steps_of(nnz, self._batch))
        # (a cost is >= 0, so with a tolerance <= -1 nothing stops the epochs early: they run as one call)
        done, per_call = 0, (int(n_iter) if convergence_tol <= -1 else 1)
        while done < int(n_iter):
            if not nnz:
                trace = [0.0] * per_call
            elif device:
                trace = be.glove_epochs(*d, index, per_call, *self._state, self._lr, self._lam).cpu().numpy().tolist()
            else:
                out = glove_fit_reference(rows, cols, fx, lx, *(t.numpy() for t in self._state), per_call, self._batch, self._lr, self._lam)
                self._state, trace = tuple(torch.from_numpy(np.ascontiguousarray(t)) for t in out[:8]), out[8]
            done += per_call
            if any(np.isnan(c) for c in trace):
                raise _lib.RsparseHipError(_lib.ERR_NUMERIC, NAN_MESSAGE)
            self.cost_history = self.cost_history + [c / max(nnz, 1) for c in trace]
            if done > 1 and len(self.cost_history) > 1 and self.cost_history[-2] / self.cost_history[-1] - 1 < convergence_tol:
                break
        self._publish()
        return self._w_i

    def get_history(self):
        """the cost of every epoch, as the modelled-on class returns it"""
        return {"cost_history": list(self.cost_history)}

    def most_similar(self, ids, k=10, which="sum"):
        """the k nearest items of each of `ids` (0-based) by cosine over W_i + W_j ("sum", the modelled-on package's advice), W_i
        ("w_i") or W_j ("w_j") -> (indices (n_q x k, -1 where fewer than k are admissible), cosines float64); the item itself is left
        out.  On the device this is `HipBackend.similar_items`."""
        if self._state is None:
            raise RuntimeError("model is not fitted")
        if which not in ("sum", "w_i", "w_j"):
            raise ValueError("which must be 'sum', 'w_i' or 'w_j'")
        W_i, W_j = self._state[:2]
        E = (W_i + W_j if which == "sum" else (W_i if which == "w_i" else W_j).clone()).contiguous()
        q = np.asarray(ids, dtype=np.int64).ravel()
        k = int(k)
        if k < 1 or (q.size and (q.min() < 0 or q.max() >= E.shape[0])):
            raise ValueError("k must be at least 1 and every id inside the matrix")
        be = self._backend()
        if hasattr(be, "similar_items") and E.is_cuda:
            res, sc = be.similar_items(E, 0, self._rank, be.to_device(q, torch.int32), k)
            idx = res.cpu().numpy().astype(np.int64)
            idx = np.where(idx == -2147483648, -1, idx - 1)       # 1-based with NA_integer_ on the device
            sc = sc.cpu().numpy().copy()
        else:
            En = E.numpy().astype(np.float64)
            norm = np.sqrt((En * En).sum(axis=1))
            cos = (En[q] @ En.T) / np.where(norm > 0, norm, np.inf)[None, :] / np.where(norm[q] > 0, norm[q], np.inf)[:, None]
            cos[np.arange(q.size), q] = -np.inf
            cos[:, norm == 0] = -np.inf
            idx = np.argsort(-cos, axis=1, kind="stable")[:, :k]
            sc = np.take_along_axis(cos, idx, axis=1)
            idx = np.where(np.isfinite(sc), idx, -1)
            if idx.shape[1] < k:
                idx = np.concatenate([idx, np.full((q.size, k - idx.shape[1]), -1)], axis=1)
                sc = np.concatenate([sc, np.full((q.size, k - sc.shape[1]), np.nan)], axis=1)
        sc[idx == -1] = np.nan
        return idx, sc
