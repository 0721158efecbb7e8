"""iALS++ (Rendle, Krichene, Zhang, Koren 2021, "iALS++: Speeding up Matrix Factorization with Subspace Optimization"): implicit
ALS that minimises WRMF's objective over one BLOCK of b coordinates of a row at a time and solves each block exactly.  A sweep
costs nnz k b + n k b^2 instead of nnz k^2 + n k^3, and the per-row system is b x b whatever the rank.  The block step runs on
the device (wrmf_subspace.hip: the b x b systems assembled on the fp32 matrix cores, factored in the wave); DESIGN.md 3.39.

The definition (include/rsparse_wrmf_hip.h repeats it for C hosts):

Objective.  WRMF's implicit one: sum over ALL cells of c_ui (p_ui - w_u . h_i)^2 + lambda (|W|^2 + |H|^2); at a stored cell c_ui
is the stored value (> 0) and p_ui = 1, elsewhere c = 1 and p = 0.

One half updates W (n x k) with H (m x k) fixed: G = H'H, e_ui = w_u . h_i at the stored cells, then for the blocks
pi = [0, b), [b, 2 b), ... in order (the last one narrower when b does not divide k):

    D = W G[:, pi] with the CURRENT W (n x |pi|), and for every row u, the empty ones included,
    g = D[u] + lambda w_u,pi + sum_{i in row} ((c_ui - 1) e_ui - c_ui) h_i,pi
    A = G_pi,pi + lambda I + sum_{i in row} (c_ui - 1) h_i,pi h_i,pi'
    delta = A^-1 g;   w_u,pi <- w_u,pi - delta;   e_ui <- e_ui - h_i,pi . delta for the row's cells.

g is half the gradient of the objective in w_u,pi and A half its Hessian, so a block step is the exact minimiser over the block: the
objective never increases, and with a single block (b >= k) a half is the exact solve (G + sum (c - 1) h h' + lambda I)^-1 sum c h
from any W.  One iteration is the item half, then the user half, in `WRMF`'s order.  The definition is plain float64 numpy; the
device is held to it by the measured bounds of DESIGN.md 3.39, not bit for bit.

  ialspp_block_reference, ialspp_half_reference, ialspp_fit_reference, ialspp_objective     the definition, in numpy
  IALSpp                                                                                   the model: `WRMF`'s inference surface
"""
import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from .wrmf import WRMF, _identity


def ialspp_block_reference(indptr, indices, c, H, G, c0, width, lambda_, W, e):
    """one block step of the definition on the columns [c0, c0 + width) -> (W', e') in float64; nothing is changed in place"""
    ip, idx = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    c, H, G = np.asarray(c, dtype=np.float64), np.asarray(H, dtype=np.float64), np.asarray(G, dtype=np.float64)
    W, e, lam = np.array(W, dtype=np.float64), np.array(e, dtype=np.float64), np.float64(lambda_)
    pi = slice(int(c0), int(c0) + int(width))
    D = W @ G[:, pi]
    base = G[pi, pi] + lam * np.eye(int(width))
    for u in range(W.shape[0]):
        a, b = ip[u], ip[u + 1]
        Hs, cu = H[idx[a:b], pi], c[a:b]
        g = D[u] + lam * W[u, pi] + ((cu - 1.0) * e[a:b] - cu) @ Hs
        A = base + (Hs * (cu - 1.0)[:, None]).T @ Hs
        delta = np.linalg.solve(A, g)
        W[u, pi] -= delta
        e[a:b] -= Hs @ delta
    return W, e


def ialspp_half_reference(indptr, indices, c, H, W, block, lambda_):
    """one half of the definition: the rows W of the CSR (indptr, indices, c) against the fixed H -> W' in float64"""
    ip, idx = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    H, W = np.asarray(H, dtype=np.float64), np.array(W, dtype=np.float64)
    k = W.shape[1]
    G = H.T @ H
    rows = np.repeat(np.arange(W.shape[0], dtype=np.int64), np.diff(ip))
    e = np.einsum("ij,ij->i", W[rows], H[idx])
    for c0 in range(0, k, int(block)):
        W, e = ialspp_block_reference(ip, idx, c, H, G, c0, min(int(block), k - c0), lambda_, W, e)
    return W


def ialspp_fit_reference(c_ui, U, V, n_iter, block, lambda_):
    """n_iter iterations (item half, user half) of the definition on c_ui (users x items, values c > 0) from (U, V) -> (U, V)"""
    c_ui = sp.csr_matrix(c_ui, dtype=np.float64)
    c_ui.sort_indices()
    c_iu = sp.csr_matrix(c_ui.T)
    c_iu.sort_indices()
    U, V = np.array(U, dtype=np.float64), np.array(V, dtype=np.float64)
    for _ in range(int(n_iter)):
        V = ialspp_half_reference(c_iu.indptr, c_iu.indices, c_iu.data, U, V, block, lambda_)
        U = ialspp_half_reference(c_ui.indptr, c_ui.indices, c_ui.data, V, U, block, lambda_)
    return U, V


def ialspp_objective(c_ui, U, V, lambda_):
    """the objective, evaluated densely in float64 (small matrices only)"""
    C = np.asarray(sp.csr_matrix(c_ui, dtype=np.float64).todense())
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    stored = C != 0
    R = stored.astype(np.float64) - U @ V.T
    return float((np.where(stored, C, 1.0) * R * R).sum() + np.float64(lambda_) * ((U * U).sum() + (V * V).sum()))


class IALSpp(WRMF):
    """Implicit ALS by exact block solves (the module's docstring is the definition).

    rank 1 ... 256; lambda_ finite and >= 0 (not scaled by the row lengths); block: 32 or 64, the coordinates solved together;
    precision: "float" only; rng: a seed or a numpy Generator; factor_init: "device" (the counter-based generator) or "host"
    (numpy's stream of `rng`), both N(0, 0.01^2) on either side; preprocess: None or a function applied to the CsparseMatrix
    first, as in `WRMF`.  Implicit feedback without biases: feedback=, solver=, with_user_item_bias=, with_global_bias= are
    accepted only at those values.
    `fit_transform` returns the user rows of the last user half; `transform` is `WRMF`'s exact fold-in (the Cholesky path, as `WRMF`
    does for its conjugate-gradient fits); `predict`, `evaluate`, `score`, `similar_items`, `held_out_ranks`, `evaluate_ranks` and
    `explain` are `WRMF`'s."""

    def __init__(self, rank=128, lambda_=0.1, block=64, precision="float", rng=None, factor_init="device", preprocess=None,
                 feedback="implicit", solver=None, with_user_item_bias=False, with_global_bias=False, device=None, backend=None):
        if isinstance(rank, bool) or not isinstance(rank, (int, np.integer)) or rank < 1:
            raise ValueError("rank must be an integer >= 1")
        if not (np.isfinite(float(lambda_)) and float(lambda_) >= 0):
            raise ValueError("lambda_ must be finite and >= 0")
        if precision not in ("float", "double"):
            raise ValueError("precision must be 'double' or 'float'")
        if block not in (32, 64):
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "IALSpp(block=): 32 or 64 coordinates per block")
        if precision == "double":
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "IALSpp(precision='double'): the block kernel holds fp32 factors")
        if rank > 256:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "rank > 256 is not on the device path")
        if feedback != "implicit":
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "IALSpp minimises the implicit objective only (feedback='implicit')")
        if with_user_item_bias or with_global_bias:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "IALSpp has no bias terms")
        if solver is not None:
            raise ValueError("IALSpp has one solver, the exact block solve: solver= selects among WRMF's")
        if preprocess is not None and not callable(preprocess):
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "IALSpp(preprocess=): None or a function")
        super().__init__(rank=int(rank), lambda_=float(lambda_), dynamic_lambda=False, preprocess=_identity if preprocess is None else preprocess,
                         feedback="implicit", solver="cholesky", precision="float", rng=rng, device=device, backend=backend,
                         factor_init=factor_init)
        self._block = int(block)

    def _confidences(self, x):
        """x (users x items) -> the canonical CSR of the confidences: `preprocess` applied, float32 values, all > 0"""
        m = sp.csr_matrix(self._preprocess(sp.csc_matrix(x, dtype=np.float64)), dtype=np.float64)
        m.sum_duplicates()
        m.sort_indices()
        m = m.astype(np.float32)
        if m.nnz and not (m.data > 0).all():
            raise ValueError("all(x@x > 0) is not TRUE")
        return m

    def _half(self, be, csr, W, H, G):
        """one half in place on the device: the rows W of the CSR against H"""
        k, b, lam = self._rank, self._block, self._lambda
        p, j, x = csr
        if not hasattr(be, "subspace_block"):
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "the backend has no iALS++ block kernel")
        be.gramian(H, 0.0, G, None)
        e = be.score_pairs(W, H, p, j)[0].to(torch.float32)
        for c0 in range(0, k, b):
            w = min(b, k - c0)
            D = torch.matmul(W, G[:, c0:c0 + w])   # (n k b flops and one read of W per block: not the hot path)
            be.subspace_block(p, j, x, H, c0, w, b, G[c0:c0 + w, c0:c0 + w], D, lam, W, e)

    def fit_transform(self, x, n_iter=10):
        """n_iter iterations (item half, user half) over the users x items matrix x -> the user rows (n_users x rank)"""
        if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or n_iter < 0:
            raise ValueError("n_iter must be an integer >= 0")
        if self._dist()[0] > 1:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "IALSpp fits on one rank")
        m = self._confidences(x)
        n_user, n_item = m.shape
        if n_user < 1 or n_item < 1:
            raise ValueError("x must have at least one row and one column")
        be, k = self._backend(), self._rank
        if self._factor_init == "device":
            U, V = self._initial_factors_device(be, n_user, n_item)
        else:
            draw = lambda given, n: (np.array(given, dtype=np.float32) if given is not None
                                     else (self._rng.standard_normal((n, k)) * 0.01).astype(np.float32))
            U0 = draw(self._init_user_factors, n_user)
            V0 = draw(None if self.components is None else self.components.T, n_item)
            if U0.shape != (n_user, k) or V0.shape != (n_item, k):
                raise ValueError("initial factors must be n_user x rank and rank x n_item")
            U, V = be.to_device(U0, torch.float32), be.to_device(V0, torch.float32)
        up = (be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32), be.to_device(m.data, torch.float32))
        ip = be.transpose_csc(n_item, n_user, *up)   # the existing transposition: item-major
        G = torch.empty((k, k), dtype=torch.float32, device=U.device)
        for _ in range(int(n_iter)):
            self._half(be, ip, V, U, G)
            self._half(be, up, U, V, G)
        be.check_numeric()
        self._drop_replicas(be)
        self._V, self._cnt_item = V, torch.diff(ip[0]).to(torch.float32)
        self._XtX = torch.empty((k, k), dtype=torch.float32, device=V.device)
        be.gramian(V, self._lambda, self._XtX, None)   # the fold-in's Gramian, lambda in it
        self.components = np.asfortranarray(V.cpu().numpy().T)
        return U.cpu().numpy()
