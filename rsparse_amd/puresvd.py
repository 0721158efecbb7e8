"""PureSVD (R/model_PureSVD.R): the soft-SVD recommender behind the MatrixFactorizationRecommender boundary.

The model is `soft_svd` / `soft_impute` (rsparse_amd/softals.py) of the preprocessed users x items matrix; an embedding is
`preprocess(x) %*% v` (one pass of wrmf_softals.hip, no per-user system) and the item side is `components = t(v diag(d))`.
Everything after the fit is WRMF's inference surface: the scores `transform(x) %*% components` are formed as ((x v) o d) v^T,
so that the item matrix the device holds is v itself -- the reference's `components_`, over which `similar_items`, the
"diversity" metric and MMR take their cosines (R/model_PureSVD.R:84, R/MatrixFactorizationRecommender.R:79-116).
"""
import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from .confidence import Confidence
from .softals import soft_impute, soft_svd, softals_half_reference
from .wrmf import WRMF, _identity


class PureSVD(WRMF):
    def __init__(self, rank=10, lambda_=0.0, init=None, preprocess=_identity, method="svd", precision="double", rng=None,
                 device=None, backend=None):
        if method not in ("svd", "impute"):
            raise ValueError("method must be 'svd' or 'impute'")                       # match.arg, :45
        if init is not None and not all(hasattr(init, n) or (isinstance(init, dict) and n in init) for n in ("u", "d", "v")):
            raise TypeError("init must be NULL or an svd-like object with u, d, v")
        # (the solver arguments of the base class play no part: no per-user system exists)
        super().__init__(rank=rank, lambda_=lambda_, preprocess=preprocess, feedback="explicit", solver="cholesky",
                         precision=precision, rng=rng, device=device, backend=backend)
        self._method = method
        self._svd_init = init
        self._d = None       # the singular values, numpy float64; the model's rank is their number after the fit
        self.svd = None      # the fitted SoftSVD (u, d, v, trace)

    # ------------------------------------------------------------------------------------------
    def _prepare(self, x, fit):
        """preprocess(x), users x items, as canonical CSR in double (R/model_PureSVD.R:61-62, :93-94)"""
        conf = self._confidence()
        if conf is not None:
            if not fit and not conf.fitted:
                raise RuntimeError("model is not fitted")
            be = self._backend()
            x = conf.fit_transform(x, backend=be) if fit else conf.transform(x, backend=be)
        elif self._preprocess is not _identity:
            x = self._preprocess(sp.csc_matrix(x, dtype=np.float64))
        x = sp.csr_matrix(x, dtype=np.float64)
        x.sum_duplicates()
        x.sort_indices()
        return x

    def _product(self, xp, scale):
        """xp %*% v (o d with `scale`) on the device, by the kernel; xp: prepared CSR"""
        be = self._backend()
        s = self._d if scale else None
        if not hasattr(be, "softals_half"):   # (the CPU stand-in of the tests)
            out, _ = softals_half_reference(xp.indptr, xp.indices, xp.data, self._V.numpy(), None, None,
                                            np.ones_like(self._d) if s is None else s, None)
            return torch.from_numpy(out).to(self._V.dtype)
        p, j = be.to_device(xp.indptr, torch.int32), be.to_device(xp.indices, torch.int32)
        return be.softals_half(p, j, be.to_device(xp.data, self._V.dtype), self._V, s=s)[0]

    def fit_transform(self, x, n_iter=100, convergence_tol=1e-3):
        """R/model_PureSVD.R:58-87 -> x %*% v (this is not u o d)"""
        be = self._backend()
        xp = self._prepare(x, True)
        fit = soft_svd if self._method == "svd" else soft_impute                       # :64-68
        self.svd = fit(xp, rank=self._rank, lambda_=self._lambda, n_iter=n_iter, convergence_tol=convergence_tol,
                       init=self._svd_init, precision="double" if self._f64 else "float", rng=self._rng, backend=be)
        self._d = np.asarray(self.svd.d, dtype=np.float64)
        self._rank = int(self._d.size)                                                 # (may be below `rank`: R/SoftALS.R:230)
        self._drop_replicas(be)
        self._V = be.to_device(self.svd.v, self._dev_t())
        self.components = (self.svd.v * self._d).T.astype(self._np_dtype())            # :80
        self.losses = [loss for _, loss in self.svd.trace]
        return self._product(xp, False).cpu().numpy().astype(self._np_dtype())         # :77

    def _transform_device(self, x_csr):
        """what the inherited scoring multiplies with the item matrix v: (preprocess(x) v) o d, complete on every rank"""
        if self._V is None:
            raise RuntimeError("model is not fitted")
        self._my_rows(x_csr)
        return self._product(self._prepare(x_csr, False), True)

    def transform(self, x):
        """R/model_PureSVD.R:91-99: preprocess(x) %*% v"""
        if self._V is None:
            raise RuntimeError("model is not fitted")
        x = sp.csr_matrix(x, dtype=np.float64)
        if x.shape[1] != self._V.shape[0]:
            raise ValueError("ncol(x) == ncol(self$components) is not TRUE")
        return self._product(self._prepare(x, False), False).cpu().numpy().astype(self._np_dtype())

    def explain(self, x, pairs, n=None):
        raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "PureSVD has no per-user system to explain a score with")
