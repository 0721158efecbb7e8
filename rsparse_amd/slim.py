"""SLIM (Ning and Karypis 2011, "SLIM: Sparse Linear Methods for Top-N Recommender Systems"): one non-negative elastic-net
regression of every item column on all the others, solved by cyclic coordinate descent; the sparse sibling of EASE, scored by the
same dense items x items matrix.

The definition (include/rsparse_wrmf_hip.h repeats it for C hosts; wrmf_slim.hip runs it on the device, one workgroup per column):

Input.  As for EASE: x is reduced with `itemknn.canonical_pattern`, so this is the binary model.  G is the float64 Gram matrix at
lambda = 0 (`ease.ease_gram_reference(x, 0)`): off the diagonal the co-occurrence counts c_ij, on it n_i, all exact integers.

Column j.  Minimise over w >= 0 with w_j = 0

    1/2 |h_j - H w|^2 + l2/2 |w|^2 + l1 |w|_1

(sklearn's ElasticNet(positive=True) per column: l1 = n_users * alpha * l1_ratio, l2 = n_users * alpha * (1 - l1_ratio)).

Support.  S_j = the i != j with c_ij > 0, ascending.  Coordinates outside S_j are never visited: with G >= 0 and w >= 0 their update
is max(0, <= 0 - l1) = 0, so the restriction is the problem itself, not an approximation.

State.  w and r, float64 over S_j, both from +0.0; r_s is (G w)_{S[s]}, kept by the updates; den_t = n_{S[t]} + l2 (one rounding).

One sweep.  t = 0 .. m - 1 in order; every operation is a separately rounded float64 operation, nothing is fused:

    i = S[t];  d = G[i, i];  c = G[j, i]
    u  = (c - (r[t] - d * w[t])) - l1
    wn = u / den_t  if u > 0  else +0.0
    delta = wn - w[t]
    if delta != 0:
        for every s: r[s] = r[s] + (delta * G[i, S[s]])          (the product rounded, then the sum)
        w[t] = wn
    dmax = max(dmax, |delta|);  wmax = max(wmax, |wn|)

Stopping.  After a sweep: stop if wmax == 0 or dmax <= tol * wmax; otherwise go on, up to max_iter sweeps.  An empty support takes
0 sweeps.

Outputs per column.  W[S[t], j] = w[t], rounded once into the model's dtype; every other cell of the column is +0.0.  The number of
sweeps.

Scoring.  `ease.ease_scores_reference` over W, and with it every list, candidate, cell and rank definition of EASE.

  slim_columns_reference, slim_weights_reference      the definition, in numpy, with a plain loop over the coordinates
  SLIM                                                the model: `EASE` with another fit
"""
import numpy as np
import torch

from . import _lib
from .ease import EASE, ROW_BYTES, ease_gram_reference
from .itemknn import canonical_pattern


def _check_fit_args(l1, l2, max_iter, tol):
    l1, l2, tol = float(l1), float(l2), float(tol)
    for name, v in (("l1", l1), ("l2", l2), ("tol", tol)):
        if not (np.isfinite(v) and v >= 0):
            raise ValueError("%s must be finite and >= 0" % name)
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError("max_iter must be an integer >= 1")
    return l1, l2, int(max_iter), tol


def slim_columns_reference(G, cols, l1, l2, max_iter, tol, dtype=np.float64, updates=None):
    """-> (W (n_items, n_items) of `dtype`: the columns `cols` of the definition, every other column zeros; sweeps: int32, one per
    element of cols).  G: the Gram matrix at lambda = 0, float64.  cols: any order, repeats allowed.  updates: a list that
    receives, per element of cols, the number of coordinates that changed (delta != 0) over all its sweeps."""
    l1, l2, max_iter, tol = _check_fit_args(l1, l2, max_iter, tol)
    G = np.ascontiguousarray(G, dtype=np.float64)
    n_items = G.shape[0]
    cols = np.atleast_1d(np.asarray(cols, dtype=np.int64))
    if cols.size and (cols.min() < 0 or cols.max() >= n_items):
        raise ValueError("a column outside [0, n_items)")
    W = np.zeros((n_items, n_items), dtype=np.float64)
    sweeps = np.zeros(cols.size, dtype=np.int32)
    diag = np.diag(G).copy() if n_items else np.zeros(0)
    for k, j in enumerate(cols):
        S = np.flatnonzero(G[j] > 0)
        S = S[S != j]
        m = int(S.size)
        c, d, den = G[j, S].tolist(), diag[S].tolist(), (diag[S] + np.float64(l2)).tolist()
        w, r = [0.0] * m, np.zeros(m, dtype=np.float64)
        n = changed = 0
        while m and n < max_iter:
            dmax = wmax = 0.0
            for t in range(m):
                wt = w[t]
                u = (c[t] - (r.item(t) - d[t] * wt)) - l1
                wn = u / den[t] if u > 0 else 0.0
                delta = wn - wt
                if delta != 0:
                    r += delta * G[S[t]][S]
                    w[t] = wn
                    changed += 1
                dmax, wmax = max(dmax, abs(delta)), max(wmax, abs(wn))
            n += 1
            if wmax == 0 or dmax <= tol * wmax:
                break
        W[S, j] = w
        sweeps[k] = n
        if updates is not None:
            updates.append(changed)
    return W.astype(dtype), sweeps


def slim_weights_reference(x, l1, l2, max_iter, tol, dtype=np.float64, cols=None):
    """-> (W, sweeps) of `slim_columns_reference` on the Gram matrix of x; cols: default every item, ascending"""
    G = ease_gram_reference(x, 0.0)
    return slim_columns_reference(G, np.arange(G.shape[0]) if cols is None else cols, l1, l2, max_iter, tol, dtype)


class SLIM(EASE):
    """The sparse linear method of Ning and Karypis 2011 (the module's docstring is the definition): `EASE` with the weights of a
    non-negative elastic net per item column instead of the ridge regression's closed form.

    l1, l2: the penalties, finite and >= 0 (in sklearn's terms n_users * alpha * l1_ratio and n_users * alpha * (1 - l1_ratio));
    max_iter: the sweep cap per column, >= 1; tol: a column stops when its largest change is at most tol times its largest
    weight, finite and >= 0; precision, device, backend: as `EASE`.  A backend without `slim_columns` (the CPU stand-in of the
    tests) runs the numpy definition.
    Fitted: `W` (= `B`, downloaded on access), `n_sweeps` (int32 per item), `item_count`.  Everything else -- `predict`,
    `candidates=`, `evaluate`, `negatives=`, `score`, `held_out_ranks`, `evaluate_ranks`, `similar_items`, `sample_negatives` --
    is `EASE`'s, on these weights."""

    def __init__(self, l1=1.0, l2=50.0, max_iter=100, tol=1e-4, precision="float", device=None, backend=None):
        super().__init__(lambda_=0.0, precision=precision, device=device, backend=backend)
        self._l1, self._l2, self._max_iter, self._tol = _check_fit_args(l1, l2, max_iter, tol)
        self.n_sweeps = None

    @property
    def W(self):
        """the weights, (n_items, n_items) of the model's dtype, as a numpy array: column j is the regression of item j"""
        return self.B

    def fit(self, x, ws_rows=0):
        """the weights of the users x items matrix x -> self (`W` stays on the device, `n_sweeps`, `item_count`)"""
        self._one_rank()
        m = canonical_pattern(x)
        n_users, n_items = m.shape
        if n_items > _lib.EASE_MAX_ITEMS:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "n_items > 32768: an items x items matrix of doubles would pass 8 GiB")
        be = self._backend()
        fit_args = (self._l1, self._l2, self._max_iter, self._tol)
        if not hasattr(be, "slim_columns"):
            W, sweeps = slim_weights_reference(m, *fit_args, dtype=self._dtype)
            W = torch.from_numpy(W)
            cnt = np.bincount(m.indices, minlength=n_items).astype(np.int64)
        else:
            up, uj = be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32)
            ones = torch.ones(int(uj.numel()), dtype=torch.float32, device=uj.device)
            ip, iu, _ = be.transpose_csc(n_items, n_users, up, uj, ones)   # (as EASE.fit: item -> its users)
            G = be.item_gram(ip, iu, up, uj, n_users, n_items, 0.0, ws_rows=ws_rows)
            cnt = np.diff(ip.cpu().numpy().astype(np.int64))
            # the long supports first: a workgroup owns a column, and the last ones to start should be the short ones
            support = (G > 0).sum(dim=1) - (G.diagonal() > 0).to(torch.int64)
            order = torch.argsort(support, descending=True, stable=True)
            elems = ROW_BYTES // np.dtype(self._dtype).itemsize
            W = torch.zeros((n_items, (n_items + elems - 1) // elems * elems), device=G.device,
                            dtype=torch.float32 if self._dtype == np.float32 else torch.float64)
            by_order = be.slim_columns(G, order.to(torch.int32), *fit_args, W)
            sweeps = torch.zeros(n_items, dtype=torch.int32, device=G.device)
            sweeps[order] = by_order
            sweeps = sweeps.cpu().numpy()
        self._B, self._n_items, self.item_count, self.n_sweeps = W, n_items, cnt, sweeps
        return self
