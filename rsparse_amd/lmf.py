"""Logistic matrix factorisation (Johnson 2014, "Logistic Matrix Factorization for Implicit Feedback Data"; the
`LogisticMatrixFactorization` of the `implicit` library) trained by the paper's alternating Adagrad ascent on the EXACT gradient:
every user-item pair takes part in every half-iteration, nothing is sampled and nothing races, so a repeated fit returns the same
bits.  The dense part of the gradient, sigma(A B') B, runs fused on the fp32 matrix cores (lmf_dense_kernel of wrmf_lmf.hip) and
never materialises the scores; DESIGN.md 3.37.

The definition (include/rsparse_wrmf_hip.h repeats it for C hosts):

Input.  x: users x items, made canonical CSR after `preprocess`, values > 0 rounded to float32; c_ui = alpha * x_ui.

Factors.  K = rank + 2.  A user row is [x_u (rank), b_u, 1], an item row [y_i (rank), 1, b_i]: s_ui = row_u . row_i = x_u . y_i +
b_u + b_i.  The coordinate that holds the 1 is FROZEN (K - 1 of users, K - 2 of items).  lambda applies to the first `rank`
coordinates only; the biases are not regularised.

One half-iteration over the rows A (n_rows x K) against the fixed side B (n_str x K) and the side's CSR (p, j, c):

    D[r, :]   = sum over ALL t < n_str of sigma(A[r] . B[t]) * B[t, :]                          (dense term)
    Sp[r, :]  = sum over the stored t of row r of c_rt * (1 - sigma(A[r] . B[j_t])) * B[j_t, :]   (sparse term)
    g         = Sp - D - lambda * A[r] on the first `rank` coordinates (no lambda term on the others); g[frozen] = 0
    a'        = a + g * g            (per coordinate, float64 state, from 0)
    A'[r, c]  = A[r, c] + lr * g[c] / sqrt(a'[c])   where a'[c] > 0 and g[c] != 0, otherwise unchanged; rounded once into float32

One iteration: the user half (B = the items), then the item half (B = the new users, on the transposed CSR).
Log-likelihood (optional, per half, at the factors the half started from):

    sum_stored c s - sum_stored c softplus(s) - sum_all softplus(s) - lambda / 2 (|X|^2 + |Y|^2),  softplus(s) = max(s, 0) + log1p(exp(-|s|))

A fit starts from `rng.init_factors` (streams 0 and 1, scale 0.01) in the first `rank` coordinates, biases 0, the frozen coordinate
1, a = 0.  The fold-in of new users starts from rows [0 ... 0, 0, 1] with a = 0 and runs `transform_iter` user halves, the items
untouched.  The definition is plain float64 numpy in no particular summation order; the device is held to it by the error bounds
of DESIGN.md 3.37, not bit for bit.

  lmf_dense_reference, lmf_half_reference, lmf_loglik_reference, lmf_fit_reference     the definition, in numpy
  LogisticMF                                                                            the model: `WRMF`'s inference surface on rank K
"""
import numpy as np
import scipy.sparse as sp
import torch
from scipy.special import expit

from . import _lib
from . import rng as _rng
from .wrmf import WRMF, _identity


def softplus(s):
    s = np.asarray(s, dtype=np.float64)
    return np.maximum(s, 0.0) + np.log1p(np.exp(-np.abs(s)))


def lmf_dense_reference(A, B):
    """D = sigma(A B') B in float64 -> (n_rows, K)"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    return expit(A @ B.T) @ B


def lmf_half_reference(indptr, indices, c, A, aA, B, rank, frozen, learning_rate, lambda_, D=None):
    """One half-iteration of the definition over the CSR (indptr, indices, c = alpha x) from the rows A with the Adagrad state aA
    against B -> (A' in A's dtype, a', g); nothing is changed in place.  D: the dense term to use instead of the definition's."""
    A0, B = np.asarray(A), np.asarray(B, dtype=np.float64)
    A = A0.astype(np.float64)
    ip, idx = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    S = A @ B.T
    D = expit(S) @ B if D is None else np.asarray(D, dtype=np.float64)
    rows = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(ip))
    W = np.zeros_like(S)
    W[rows, idx] = np.asarray(c, dtype=np.float64) * (1.0 - expit(S[rows, idx]))
    g = W @ B - D
    g[:, :rank] -= np.float64(lambda_) * A[:, :rank]
    if frozen >= 0:
        g[:, frozen] = 0.0
    a2 = np.asarray(aA, dtype=np.float64) + g * g
    move = (a2 > 0) & (g != 0)
    new = np.where(move, A + np.float64(learning_rate) * g / np.sqrt(np.where(a2 > 0, a2, 1.0)), A)
    return np.where(move, new.astype(A0.dtype), A0), a2, g


def lmf_loglik_reference(indptr, indices, c, A, B, rank, lambda_):
    """the log-likelihood of the definition at the factors (A, B); (indptr, indices, c): the CSR whose rows are A's"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    ip, idx, c = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64), np.asarray(c, dtype=np.float64)
    S = A @ B.T
    s = S[np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(ip)), idx]
    reg = 0.5 * np.float64(lambda_) * ((A[:, :rank] ** 2).sum() + (B[:, :rank] ** 2).sum())
    return float((c * s).sum() - (c * softplus(s)).sum() - softplus(S).sum() - reg)


def lmf_fit_reference(c_ui, U, V, n_iter, rank, learning_rate, lambda_, aU=None, aV=None, update_items=True):
    """n_iter iterations of the definition on c_ui (scipy CSR, users x items, values c = alpha x) from the rows (U, V) ->
    (U, V, aU, aV, trace), trace = the log-likelihood at the start of every half.  update_items=False: user halves only (the
    fold-in)."""
    c_ui = sp.csr_matrix(c_ui)
    c_iu = sp.csr_matrix(c_ui.T)
    c_iu.sort_indices()
    U, V, K = np.array(U), np.array(V), U.shape[1]
    aU = np.zeros(U.shape) if aU is None else np.array(aU, dtype=np.float64)
    aV = np.zeros(V.shape) if aV is None else np.array(aV, dtype=np.float64)
    trace = []
    for _ in range(int(n_iter)):
        trace.append(lmf_loglik_reference(c_ui.indptr, c_ui.indices, c_ui.data, U, V, rank, lambda_))
        U, aU, _ = lmf_half_reference(c_ui.indptr, c_ui.indices, c_ui.data, U, aU, V, rank, K - 1, learning_rate, lambda_)
        if update_items:
            trace.append(lmf_loglik_reference(c_iu.indptr, c_iu.indices, c_iu.data, V, U, rank, lambda_))
            V, aV, _ = lmf_half_reference(c_iu.indptr, c_iu.indices, c_iu.data, V, aV, U, rank, K - 2, learning_rate, lambda_)
    return U, V, aU, aV, trace


def _check_args(rank, alpha, learning_rate, lambda_, transform_iter):
    for name, v in (("rank", rank), ("transform_iter", transform_iter)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError("%s must be an integer >= 1" % name)
    out = []
    for name, v in (("alpha", alpha), ("learning_rate", learning_rate), ("lambda_", lambda_)):
        v = float(v)
        if not (np.isfinite(v) and v >= 0):
            raise ValueError("%s must be finite and >= 0" % name)
        out.append(v)
    return (int(rank), *out, int(transform_iter))


class LogisticMF(WRMF):
    """Logistic matrix factorisation (the module's docstring is the definition).

    rank <= 126 (K = rank + 2 <= 128); alpha: the confidence of a stored entry is alpha * x; learning_rate and lambda_: finite and
    >= 0; transform_iter: the user halves of a fold-in; precision: "float" only; preprocess: None or a function applied to the
    CsparseMatrix first, as in `WRMF`; rng: a seed or a numpy Generator, from which ONE 63-bit seed is taken per fit.  A backend
    without `lmf_half` (the CPU stand-in of the tests) runs the numpy definition.
    Fitted: `components` (K x n_items), `user_bias` / `item_bias`, `user_adagrad` / `item_adagrad` (float64, one per coordinate),
    `trace` (with fit_transform(trace=True): the log-likelihood at the start of every half), `seed`.  `transform`, `predict`,
    `evaluate`, `score` and the rest of WRMF's surface run on the rows of K coordinates, so a score is x_u . y_i + b_u + b_i;
    `similar_items` compares the first `rank` coordinates; `explain` is not available."""

    def __init__(self, rank=30, alpha=1.0, learning_rate=1.0, lambda_=0.6, transform_iter=20, precision="float", rng=None,
                 preprocess=None, device=None, backend=None):
        rank, self._alpha, self._lr, lam, self._transform_iter = _check_args(rank, alpha, learning_rate, lambda_, transform_iter)
        if precision not in ("float", "double"):
            raise ValueError("precision must be 'double' or 'float'")
        if precision == "double":
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "LogisticMF(precision='double'): the dense kernel holds fp32 factors")
        if rank + 2 > _lib.LMF_MAX_K:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "rank > %d is not on the device path" % (_lib.LMF_MAX_K - 2))
        if preprocess is not None and not callable(preprocess):
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "LogisticMF(preprocess=): None or a function")
        super().__init__(rank=rank + 2, lambda_=lam, dynamic_lambda=False, preprocess=_identity if preprocess is None else preprocess,
                         feedback="implicit", solver="cholesky", precision="float", rng=rng, device=device, backend=backend,
                         factor_init="device")
        self._lrank = rank
        self.seed = None
        self.trace = []
        self.user_bias = self.item_bias = self.user_adagrad = self.item_adagrad = None
        self._aV = None

    def _latent_window(self):
        return 0, self._lrank

    def _confidences(self, x):
        """x (users x items) -> the canonical CSR of c / alpha: `preprocess` applied, float32 values, all > 0"""
        m = sp.csr_matrix(self._preprocess(sp.csc_matrix(x, dtype=np.float64)), dtype=np.float64)
        m.sum_duplicates()
        m.sort_indices()
        m = m.astype(np.float32)
        if m.nnz and not (m.data > 0).all():
            raise ValueError("all(x@x > 0) is not TRUE")
        return m

    def _initial(self, be, stream, n, ones_col):
        K, r = self._rank, self._lrank
        if hasattr(be, "init_factors"):
            F = torch.zeros((n, K), dtype=torch.float32, device=be.device)
            if n:
                be.init_factors(self.seed, stream, n, r, torch.float32, out=F[:, :r])
        else:
            F = torch.zeros((n, K), dtype=torch.float32)
            F[:, :r] = torch.from_numpy(_rng.init_factors(self.seed, stream, 0, n, r, 0.01, dtype=np.float32))
        F[:, ones_col] = 1.0
        return F

    def _halves(self, m, U, V, aU, aV, n_iter, update_items, trace):
        """n_iter iterations on the canonical rows m, in place where the backend has the kernels -> (U, V, aU, aV, trace)"""
        be, r, K, lam = self._backend(), self._lrank, self._rank, self._lambda
        if not hasattr(be, "lmf_half"):
            out = lmf_fit_reference(m.astype(np.float64) * self._alpha, U.numpy(), V.numpy(), n_iter, r, self._lr, lam, aU.numpy(), aV.numpy(), update_items)
            return tuple(torch.from_numpy(np.ascontiguousarray(t)) for t in out[:4]) + (out[4] if trace else [],)
        up = (be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32), be.to_device(m.data, torch.float32))
        ip = be.transpose_csc(m.shape[1], m.shape[0], *up) if update_items else None   # the existing transposition: item-major
        lls = []
        reg = lambda: 0.5 * lam * ((U[:, :r].double() ** 2).sum() + (V[:, :r].double() ** 2).sum())
        for _ in range(int(n_iter)):   # (nothing here waits for the device unless the trace is asked for)
            for csr, A, aA, B, frozen in ((up, U, aU, V, K - 1),) + (((ip, V, aV, U, K - 2),) if update_items else ()):
                before = reg() if trace else None
                rows = be.lmf_half(*csr, self._alpha, A, aA, B, r, frozen, self._lr, lam, want_rowsums=trace)
                if trace:
                    lls.append(rows.sum() - before)
        return U, V, aU, aV, [float(v) for v in lls]

    def fit_transform(self, x, n_iter=30, trace=False):
        """n_iter iterations (user half, item half) over the users x items matrix x -> the user rows (n_users x K).
        trace=True records the log-likelihood at the start of every half in `trace` (one host synchronisation per fit)."""
        if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or n_iter < 0:
            raise ValueError("n_iter must be an integer >= 0")
        if self._dist()[0] > 1:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "LogisticMF fits on one rank")
        m = self._confidences(x)
        n_user, n_item = m.shape
        if n_user < 1 or n_item < 1:
            raise ValueError("x must have at least one row and one column")
        be, K = self._backend(), self._rank
        self.seed = int(self._rng.integers(2 ** 63))
        U, V = self._initial(be, _rng.STREAM_USERS, n_user, K - 1), self._initial(be, _rng.STREAM_ITEMS, n_item, K - 2)
        aU, aV = (torch.zeros(F.shape, dtype=torch.float64, device=F.device) for F in (U, V))
        U, V, aU, aV, self.trace = self._halves(m, U, V, aU, aV, n_iter, True, bool(trace))
        self._drop_replicas(be)
        self._V, self._aV = V, aV
        self._cnt_item = np.bincount(m.indices, minlength=n_item).astype(np.int64)
        Vh, Uh = V.cpu().numpy(), U.cpu().numpy()
        self.components = Vh.T.copy()
        self.user_bias, self.item_bias = Uh[:, K - 2].copy(), Vh[:, K - 1].copy()
        self.user_adagrad, self.item_adagrad = aU.cpu().numpy(), aV.cpu().numpy()
        return Uh

    def _transform_device(self, x_csr):
        """the fold-in: `transform_iter` user halves from rows [0 ... 0, 0, 1], the items untouched -> a device tensor"""
        if self._V is None:
            raise RuntimeError("model is not fitted")
        self._my_rows(x_csr)
        m = self._confidences(x_csr)
        U = torch.zeros((m.shape[0], self._rank), dtype=torch.float32, device=self._V.device)
        U[:, self._rank - 1] = 1.0
        aU = torch.zeros(U.shape, dtype=torch.float64, device=U.device)
        if m.shape[0]:
            U = self._halves(m, U, self._V, aU, self._aV, self._transform_iter, False, False)[0]
        return U

    def transform(self, x):
        if self._V is None:
            raise RuntimeError("model is not fitted")
        x = sp.csr_matrix(x, dtype=np.float64)
        if x.shape[1] != self._V.shape[0]:
            raise ValueError("ncol(x) == ncol(self$components) is not TRUE")
        return self._transform_device(x).cpu().numpy()

    def explain(self, x, pairs, n=None):
        raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "LogisticMF has no per-user linear system to explain a score with")
