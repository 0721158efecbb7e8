"""Second-order factorization machine (Rendle 2010, "Factorization Machines") over a sparse samples x features matrix, binomial
or gaussian, trained by deterministic mini-batch SGD with a per-coordinate Adagrad state: the `FactorizationMachine` of the
modelled-on package, in a form that has no race.  A mini-batch is taken from a snapshot of the parameters and every gradient
coordinate is summed per destination in a fixed order, so a fit has the same bits on every run, in numpy and on the device.
With one-hot user + one-hot item rows it is biased matrix factorisation; further columns are context, tags, attributes.

The definition (include/rsparse_wrmf_hip.h repeats it for C hosts; wrmf_fm.hip runs it on the device).  Every arithmetic operation
is a separately rounded float64 operation on parameters widened from the model's dtype; nothing is fused.

Input.  x: n x d, made canonical CSR: duplicates summed, columns ascending, explicit zeros dropped, values finite and rounded once
into the model's dtype.  y: binomial takes {0, 1} or {-1, 1} and maps to +-1; gaussian takes any finite value.  weights omega:
finite and >= 0, default 1.

Parameters.  w0 (a scalar), w (d) and V (d x rank) in the model's dtype, each with a per-coordinate Adagrad state a0, aw, aV in
float64 that starts at 0.  V starts from `rng.init_factors(seed, STREAM_ITEMS, 0, d, rank, 0.01)`, w and w0 from 0.

Steps.  n_steps = ceil(n / batch).  Step s holds the rows r = s, s + n_steps, ... in ascending r; k = 0, 1, ... numbers them (the
rule BPR uses for its slots).  An epoch is the steps 0 .. n_steps - 1; everything in a step is computed from the snapshot
(w0, w, V) at its start.

    osum(list)  BPR's ordered sum: the list in its stated order is cut into chunks of CHUNK = 64 consecutive terms; a chunk is
                summed sequentially from +0.0; the chunk sums are added sequentially to a total that starts at +0.0

Forward, row r with its stored entries e in ascending column (j_e, x_e):

    t_ec   V[j_e, c] * x_e
    s_c    osum_e(t_ec);   q_c = osum_e(t_ec * t_ec);   lin = osum_e(w[j_e] * x_e)
    pair   BPR's `dot` order over c of (s_c * s_c - q_c): 16 partials over c = l, l + 16, ... then the 8/4/2/1 tree
    raw    (w0 + lin) + 0.5 * pair
    delta  binomial: z = 1 / (1 + E(y * raw)), E = `bpr_exp`, the stated exponential;  delta = (-(omega * y)) * z
           gaussian: delta = omega * (raw - y)                                          (the loss is 1/2 (raw - y)^2)

Backward, per destination; the contributions in ascending k, one per stored entry of a row:

    column j, linear         osum_k(delta_k * x)                          count c_j = the stored entries of j in the step
    column j, coordinate c   osum_k((delta_k * x) * (s_kc - V[j, c] * x))
    intercept                osum_k(delta_k), count = the rows of the step            (intercept=True only)
    update                   of a coordinate theta with state a and count c >= 1 (every other coordinate keeps its bits):
                             g = total + (lambda * c) * theta;  a' = a + g * g;  theta' = theta - (lr * g) / sqrt(a') unless
                             a' == 0;  theta' rounded once into the dtype.  lambda = lambda_w for w, lambda_v for V, 0 for w0;
                             lr = learning_rate_w for w0 and w, learning_rate_v for V

Trace, per epoch, taken at each step's snapshot.  binomial: the integer number of rows with y * raw > 0.  gaussian:
osum_k(omega * ((raw - y) * (raw - y))) per step, the step sums added sequentially from +0.0.

Predict.  The forward pass alone: gaussian returns raw, binomial 1 / (1 + E(-raw)).

Deliberate differences from the modelled-on solver (src/factorization_machine.cpp), which is a Hogwild OpenMP loop -- racing float
updates, other bits on every run:
  * mini-batches from a snapshot replace Hogwild;
  * the regulariser multiplies the parameter and scales with the count, as BPR's does (the modelled-on line adds 2 * lambda without
    the weight);
  * the Adagrad state starts at 0 and is added to before the division (there: starts at 1, divided first);
  * nothing is clipped (there: the prediction and the gradient are);
  * the gaussian gradient has no factor 2.

  fm_forward_reference, fm_step_reference, fm_fit_reference, fm_predict_reference     the definition, in numpy
  FactorizationMachine                                                              the model
"""
import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from . import rng as _rng
from .bpr import _ordered_sums, bpr_exp, n_steps_of, sum16

MAX_RANK = _lib.FM_MAX_RANK
FAMILIES = {"binomial": 0, "gaussian": 1}


def canonical_design(x, dtype, n_feat=None):
    """x (anything scipy makes a matrix of) -> canonical CSR in `dtype`: duplicates summed, the values rounded once, explicit zeros
    dropped, columns ascending, values finite"""
    m = sp.csr_matrix(x, dtype=np.float64)
    m.sum_duplicates()
    m = sp.csr_matrix(m.astype(dtype))
    m.eliminate_zeros()
    m.sort_indices()
    if n_feat is not None and m.shape[1] != int(n_feat):
        raise ValueError("ncol(x) == n_features is not TRUE")
    if m.shape[1] < 1 or m.shape[1] >= 2 ** 31 or m.shape[0] >= 2 ** 31 or m.nnz >= 2 ** 31:
        raise ValueError("x must have 1 <= ncol < 2^31, nrow < 2^31 and fewer than 2^31 stored entries")
    if not np.isfinite(m.data).all():
        raise ValueError("x holds a value that is not finite in the model's precision")
    return m


def step_rows(n, step, n_steps):
    """the rows of step `step`: r = step, step + n_steps, ... below n, ascending (their order is k)"""
    return np.arange(int(step), int(n), int(n_steps), dtype=np.int64)


def _entries(ip, idx, val, rows):
    """the stored entries of `rows` in the order (k, column) -> (k, column, value as float64)"""
    ip = np.asarray(ip, dtype=np.int64)
    lens = ip[rows + 1] - ip[rows]
    k_of = np.repeat(np.arange(rows.size, dtype=np.int64), lens)
    first = np.concatenate([[0], np.cumsum(lens)])[:-1]
    pos = ip[rows][k_of] + (np.arange(k_of.size, dtype=np.int64) - first[k_of])
    return k_of, np.asarray(idx, dtype=np.int64)[pos], np.asarray(val)[pos].astype(np.float64)


def fm_forward_reference(indptr, indices, data, rows, w0, w, V):
    """the forward pass of the definition on `rows` (in the order k) from (w0, w, V) -> (raw (m,), S (m, rank)), float64"""
    w, V = np.asarray(w), np.asarray(V)
    rows = np.asarray(rows, dtype=np.int64)
    k_of, j, x = _entries(indptr, indices, data, rows)
    t = V[j].astype(np.float64) * x[:, None]
    s = _ordered_sums(k_of, t, rows.size)[0]
    q = _ordered_sums(k_of, t * t, rows.size)[0]
    lin = _ordered_sums(k_of, (w[j].astype(np.float64) * x)[:, None], rows.size)[0][:, 0]
    raw = (np.float64(np.asarray(w0).reshape(-1)[0]) + lin) + 0.5 * sum16(s * s - q)
    return raw, s


def fm_delta(raw, y, omega, family):
    """delta of the definition: y in +-1 (binomial) or any value (gaussian), omega the weights, all over k"""
    if family == "binomial":
        return (-(omega * y)) * (1.0 / (1.0 + bpr_exp(y * raw)))
    return omega * (raw - y)


def fm_link(raw, family):
    """what `predict` returns for the forward pass's raw"""
    return 1.0 / (1.0 + bpr_exp(-raw)) if family == "binomial" else raw


def fm_predict_reference(indptr, indices, data, w0, w, V, family):
    """predict of the definition on every row -> float64"""
    n = np.asarray(indptr).size - 1
    return fm_link(fm_forward_reference(indptr, indices, data, np.arange(n), w0, w, V)[0], family)


def _adagrad(theta, a, total, count, lr, lam):
    """the update of the coordinates with count >= 1 -> (theta', a'); count broadcasts against theta"""
    th = theta.astype(np.float64)
    cnt = np.broadcast_to(count, th.shape)
    g = total + (np.float64(lam) * cnt.astype(np.float64)) * th
    an = a + g * g
    with np.errstate(divide="ignore", invalid="ignore"):
        new = (th - (np.float64(lr) * g) / np.sqrt(an)).astype(theta.dtype)
    hit = cnt > 0
    return np.where(hit & (an != 0), new, theta), np.where(hit, an, a)


def fm_step_reference(indptr, indices, data, rows, y, omega, w0, w, V, a0, aw, aV, family, intercept, learning_rate_w,
                      learning_rate_v, lambda_w, lambda_v):
    """One step of the definition on `rows` (in the order k; y in +-1 for binomial, and omega, are indexed by row) from the snapshot
    (w0, w, V) with the Adagrad states -> (w0', w', V', a0', aw', aV', trace term); w0 and a0 are arrays of one element; nothing
    is changed in place.  The trace term: binomial the number of rows with y * raw > 0, gaussian the step's weighted squared error."""
    w0, w, V = np.asarray(w0).reshape(1), np.asarray(w), np.asarray(V)
    a0, aw, aV = (np.asarray(t, dtype=np.float64) for t in (np.reshape(a0, 1), aw, aV))
    rows = np.asarray(rows, dtype=np.int64)
    d = V.shape[0]
    yk, ok = np.asarray(y, dtype=np.float64)[rows], np.asarray(omega, dtype=np.float64)[rows]
    raw, s = fm_forward_reference(indptr, indices, data, rows, w0, w, V)
    delta = fm_delta(raw, yk, ok, family)
    k_of, j, x = _entries(indptr, indices, data, rows)
    dx = delta[k_of] * x
    tot_v, cnt = _ordered_sums(j, dx[:, None] * (s[k_of] - V[j].astype(np.float64) * x[:, None]), d)
    tot_w = _ordered_sums(j, dx[:, None], d)[0][:, 0]
    V2, aV2 = _adagrad(V, aV, tot_v, cnt[:, None], learning_rate_v, lambda_v)
    w2, aw2 = _adagrad(w, aw, tot_w, cnt, learning_rate_w, lambda_w)
    w02, a02 = w0.copy(), a0.copy()
    one = np.zeros(rows.size, dtype=np.int64)
    if intercept and rows.size:
        tot_0 = _ordered_sums(one, delta[:, None], 1)[0][0]
        w02, a02 = _adagrad(w0, a0, tot_0, np.array([rows.size]), learning_rate_w, 0.0)
    if family == "binomial":
        term = int((yk * raw > 0).sum())
    else:
        term = float(_ordered_sums(one, (ok * ((raw - yk) * (raw - yk)))[:, None], 1)[0][0, 0])
    return w02, w2, V2, a02, aw2, aV2, term


def fm_fit_reference(indptr, indices, data, y, omega, w0, w, V, a0, aw, aV, n_iter, batch, family, intercept, learning_rate_w,
                     learning_rate_v, lambda_w, lambda_v):
    """n_iter epochs of the definition -> (w0, w, V, a0, aw, aV, trace), trace = one entry per epoch: the number of rows with
    y * raw > 0 (binomial) or the weighted squared error (gaussian), both at the steps' snapshots"""
    n = np.asarray(indptr).size - 1
    n_steps = n_steps_of(n, batch)
    state = (np.array(w0).reshape(1), np.array(w), np.array(V), np.array(a0, dtype=np.float64).reshape(1),
             np.array(aw, dtype=np.float64), np.array(aV, dtype=np.float64))
    trace = []
    for _ in range(int(n_iter)):
        tot = 0 if family == "binomial" else 0.0
        for s in range(n_steps):
            *state, term = fm_step_reference(indptr, indices, data, step_rows(n, s, n_steps), y, omega, *state, family, intercept,
                                             learning_rate_w, learning_rate_v, lambda_w, lambda_v)
            tot = tot + term
        trace.append(tot)
    return (*state, trace)


class FactorizationMachine:
    """Second-order factorization machine (the module's docstring is the definition).

    learning_rate_w > 0: the step of w0 and w; rank >= 1 (<= 128 on the device); lambda_w, lambda_v >= 0; family "binomial" or
    "gaussian"; intercept: whether w0 is fitted; learning_rate_v > 0 (None: learning_rate_w); batch: the rows of one step;
    precision "float" or "double": the dtype of the parameters (the arithmetic is float64 either way); rng: a seed or a numpy
    Generator, from which ONE 63-bit seed is taken at the first fit for the initial V.  A backend without `fm_epochs` (the CPU
    stand-in of the tests) runs the numpy definition.
    `partial_fit(x, y, weights=None)` runs one epoch and keeps the parameters and their Adagrad states, `fit(..., n_iter=)` runs
    n_iter of them, `predict(x)` returns the probability of y = 1 (binomial) or the value (gaussian).
    Fitted: `w0`, `w` (d), `v` (rank x d), `adagrad_w0`, `adagrad_w`, `adagrad_v` (float64), `trace` (one entry per epoch),
    `seed`."""

    def __init__(self, learning_rate_w=0.2, rank=4, lambda_w=0.0, lambda_v=0.0, family="binomial", intercept=True, learning_rate_v=None,
                 batch=1 << 16, precision="float", rng=None, device=None, backend=None):
        if learning_rate_v is None:
            learning_rate_v = learning_rate_w
        for name, v in (("rank", rank), ("batch", batch)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError("%s must be an integer >= 1" % name)
        for name, v, strict in (("lambda_w", lambda_w, False), ("lambda_v", lambda_v, False), ("learning_rate_w", learning_rate_w, True),
                                ("learning_rate_v", learning_rate_v, True)):
            v = float(v)
            if not (np.isfinite(v) and v >= 0 and (v > 0 or not strict)):
                raise ValueError("%s must be finite and %s 0" % (name, ">" if strict else ">="))
        if family not in FAMILIES:
            raise ValueError("family must be one of %s" % list(FAMILIES))
        if precision not in ("float", "double"):
            raise ValueError("precision must be 'double' or 'float'")
        if rank > MAX_RANK:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "rank > %d is not on the device path" % MAX_RANK)
        self._rank, self._batch, self._family, self._intercept = int(rank), int(batch), family, bool(intercept)
        self._lr_w, self._lr_v, self._lam_w, self._lam_v = float(learning_rate_w), float(learning_rate_v), float(lambda_w), float(lambda_v)
        self._precision = precision
        self._rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        self._device, self._be = device, backend
        self._state = None   # (w0, w, V, a0, aw, aV): tensors where the backend works
        self.seed = None
        self.trace = []
        self.w0 = self.w = self.v = self.adagrad_w0 = self.adagrad_w = self.adagrad_v = None

    def _backend(self):
        if self._be is None:
            from .engine import HipBackend
            self._be = HipBackend(self._device)
        return self._be

    def _np(self):
        return np.float64 if self._precision == "double" else np.float32

    def _t(self):
        return torch.float64 if self._precision == "double" else torch.float32

    def _targets(self, m, y, weights):
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        if m.shape[0] != y.size:
            raise ValueError("nrow(x) == length(y) is not TRUE")
        if not np.isfinite(y).all():
            raise ValueError("!anyNA(y) is not TRUE")
        if self._family == "binomial":
            if np.isin(y, (0.0, 1.0)).all():
                y = 2.0 * y - 1.0
            elif not np.isin(y, (-1.0, 1.0)).all():
                raise ValueError("binomial y must be in {0, 1} or in {-1, 1}")
        om = np.ones(y.size) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
        if om.size != y.size:
            raise ValueError("length(weights) == length(y) is not TRUE")
        if not (np.isfinite(om).all() and (om >= 0).all()):
            raise ValueError("weights must be finite and >= 0")
        return y, om

    def _initial(self, d):
        be, k, tdt = self._backend(), self._rank, self._t()
        self.seed = int(self._rng.integers(2 ** 63))
        if hasattr(be, "init_factors"):
            V = be.init_factors(self.seed, _rng.STREAM_ITEMS, d, k, tdt)
        else:
            V = be.to_device(_rng.init_factors(self.seed, _rng.STREAM_ITEMS, 0, d, k, 0.01, dtype=self._np()), tdt)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=V.device)
        return (z(1, tdt), z(d, tdt), V, z(1, torch.float64), z(d, torch.float64), z((d, k), torch.float64))

    def _publish(self):
        w0, w, V, a0, aw, aV = (t.cpu().numpy() for t in self._state)
        self.w0, self.w, self.v = w0[0], w, V.T.copy()
        self.adagrad_w0, self.adagrad_w, self.adagrad_v = a0[0], aw, aV.T.copy()

    def fit(self, x, y, weights=None, n_iter=1):
        """n_iter epochs over the samples x features matrix x with the targets y (and the sample weights) -> self; a fitted model
        goes on from its parameters and Adagrad states"""
        if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or n_iter < 0:
            raise ValueError("n_iter must be an integer >= 0")
        m = canonical_design(x, self._np(), None if self._state is None else self._state[1].numel())
        y, om = self._targets(m, y, weights)
        if self._state is None:
            self._state = self._initial(m.shape[1])
        be = self._backend()
        if not hasattr(be, "fm_epochs"):
            out = fm_fit_reference(m.indptr, m.indices, m.data, y, om, *(t.numpy() for t in self._state), int(n_iter), self._batch,
                                   self._family, self._intercept, self._lr_w, self._lr_v, self._lam_w, self._lam_v)
            self._state, trace = tuple(torch.from_numpy(np.ascontiguousarray(t)) for t in out[:6]), out[6]
        elif m.shape[0] and n_iter:
            csr = (be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32), be.to_device(m.data, self._t()))
            n_steps = n_steps_of(m.shape[0], self._batch)
            index = be.fm_index(csr[0], csr[1], m.shape[1], n_steps)
            tr = be.fm_epochs(*csr, index, int(n_iter), self._family, self._intercept, be.to_device(y, torch.float64),
                              be.to_device(om, torch.float64), *self._state, self._lr_w, self._lr_v, self._lam_w, self._lam_v)
            trace = tr.cpu().numpy().tolist()
        else:
            trace = [0 if self._family == "binomial" else 0.0] * int(n_iter)
        self.trace = self.trace + list(trace)
        self._publish()
        return self

    def partial_fit(self, x, y, weights=None):
        """one epoch, keeping the parameters and their Adagrad states -> self"""
        return self.fit(x, y, weights, n_iter=1)

    def predict(self, x):
        """the probability of y = 1 (binomial) or the value (gaussian) of every row of x -> float64"""
        if self._state is None:
            raise RuntimeError("model is not fitted")
        m = canonical_design(x, self._np(), self._state[1].numel())
        be = self._backend()
        w0, w, V = self._state[:3]
        if not hasattr(be, "fm_predict"):
            return fm_predict_reference(m.indptr, m.indices, m.data, w0.numpy(), w.numpy(), V.numpy(), self._family)
        csr = (be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32), be.to_device(m.data, self._t()))
        return be.fm_predict(*csr, self._family, w0, w, V).cpu().numpy()
