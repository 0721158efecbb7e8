"""Confidence weighting of the interaction matrix: the reference's `preprocess` hook ("essentially the confidence transformation
from the WRMF article", R/model_WRMF.R:401-404) as shipped definitions -- linear, log, TF-IDF, BM25 -- and its ScaleNormalize
(R/model_ScaleNormalize.R), computed on the device by wrmf_confidence.hip.  `confidence_reference` is the definition in numpy.

x is users x items, v a stored value at (u, i).  Fitted on the training matrix: N = its number of rows, df_i = the stored entries
of column i, idf_i = log(N) - log1p(df_i) (as in the `implicit` library), sbar = (the sum of all values) / N.  Per-user quantities
(s_u = the sum of the row, the row norms) always come from the rows being transformed; per-item quantities and sbar from the fit.

    "linear"     alpha                       1 + alpha v
    "log"        alpha, eps                  1 + alpha log1p(v / eps)
    "tfidf"                                  sqrt(v) idf_i
    "bm25"       K1 = 100, B = 0.8           ((v (K1 + 1)) / (K1 L_u + v)) idf_i,   L_u = (1 - B) + (B s_u) / sbar
    "normalize"  scale = 0.5, norm, target   v t,   t = n^(scale - 1) where n != 0, else 0,   n = (sum |v|^norm)^(1 / norm) along target

in double, in the order written.  "tfidf" and "bm25" need v >= 0, "log" v / eps > -1 (ValueError).  With sbar == 0 the ratio
(B s_u) / sbar is taken as B (L_u = 1); an empty matrix comes back as it is.  idf_i <= 0 for an item that almost every user has is
kept (the values stay comparable with `implicit`); a fit then refuses the negative confidences as it refuses any others."""
import numpy as np
import scipy.sparse as sp
import torch

from . import _lib

KINDS = {"linear": 0, "log": 1, "tfidf": 2, "bm25": 3, "normalize": 4}     # RSPARSE_HIP_CONFIDENCE_*
TABLES = {"idf": 0, "bm25": 1, "norm": 2}                                   # RSPARSE_HIP_CONFIDENCE_TABLE_*
DEFAULTS = {"linear": {"alpha": 1.0}, "log": {"alpha": 1.0, "eps": 1.0}, "tfidf": {}, "bm25": {"K1": 100.0, "B": 0.8},
            "normalize": {"scale": 0.5, "norm": 2, "target": "rows"}}
TARGETS = ("rows", "columns")


def check_params(kind, params):
    """-> the parameters of `kind` with their defaults (ValueError: an unknown kind, parameter or value)"""
    if kind not in KINDS:
        raise ValueError("confidence kind must be one of %s" % list(KINDS))
    out = dict(DEFAULTS[kind])
    for name, value in params.items():
        if name not in out:
            raise ValueError("confidence kind %r has no parameter %r" % (kind, name))
        out[name] = value
    if kind == "normalize":
        if out["target"] not in TARGETS:
            raise ValueError("target must be 'rows' or 'columns'")
        if not float(out["norm"]) > 0:
            raise ValueError("norm must be positive")
        out["scale"] = float(out["scale"])
    else:
        out = {k: float(v) for k, v in out.items()}
    if kind == "log" and not out["eps"] > 0.0:
        raise ValueError("eps must be positive")
    if kind == "bm25" and (out["K1"] < 0 or not 0.0 <= out["B"] <= 1.0):
        raise ValueError("bm25 needs K1 >= 0 and B in [0, 1]")
    return out


def canonical_rows(x):
    """x (users x items) as a canonical CSR with float64 values: sorted, unique columns per row, duplicates summed, stored zeros
    kept.  A canonical float64 CSR is used as it stands; x itself is never changed."""
    if not sp.issparse(x):
        raise TypeError("x must be a scipy sparse matrix")
    m = x if (x.format == "csr" and x.dtype == np.float64) else sp.csr_matrix(x, dtype=np.float64)
    if not m.has_canonical_format:
        m = m.copy()
        m.sum_duplicates()
    if m.indptr[-1] >= 2 ** 31:
        raise ValueError("the matrix needs int32 row pointers")
    return m


def check_values(kind, params, data_min):
    """the domain of `kind` (data_min: the smallest stored value, None for an empty matrix)"""
    if data_min is None:
        return
    if kind in ("tfidf", "bm25") and data_min < 0:
        raise ValueError("confidence kind %r needs non-negative values" % kind)
    if kind == "log" and not data_min / params["eps"] > -1:
        raise ValueError("confidence kind 'log' needs v / eps > -1")


def norm_table(moment, scale, norm):
    """n^(scale - 1) where n != 0, else 0; n = moment^(1 / norm), moment = sum |v|^norm"""
    m = np.asarray(moment, dtype=np.float64)
    n = m if norm == 1 else (np.sqrt(m) if norm == 2 else m ** (1.0 / norm))
    t = np.zeros_like(n)
    nz = n != 0
    t[nz] = n[nz] ** (scale - 1.0)
    return t


def confidence_fit_reference(x, kind, **params):
    """the fitted state of `kind` on the training matrix x, in numpy: a dict with n_fit, item_count (int64), item_table (idf for
    "tfidf" / "bm25", the column table for "normalize" along the columns, else None) and mean_row_sum (sbar)."""
    par = check_params(kind, params)
    m = canonical_rows(x)
    check_values(kind, par, float(m.data.min()) if m.nnz else None)
    n, n_item = m.shape
    cnt = np.bincount(m.indices, minlength=n_item).astype(np.int64)
    table = None
    if kind in ("tfidf", "bm25"):
        with np.errstate(divide="ignore"):
            table = np.log(np.float64(n)) - np.log1p(cnt.astype(np.float64))
    elif kind == "normalize" and par["target"] == "columns":
        table = norm_table(np.bincount(m.indices, weights=np.abs(m.data) ** par["norm"], minlength=n_item), par["scale"], par["norm"])
    return {"n_fit": int(n), "n_item": int(n_item), "item_count": cnt, "item_table": table, "mean_row_sum": float(m.data.sum()) / n if n else 0.0}


def confidence_reference(x, kind, state=None, **params):
    """x weighted by `kind`, in numpy -> a canonical CSR of x's pattern.  state: confidence_fit_reference of the training matrix
    (None: fitted on x itself)."""
    par = check_params(kind, params)
    m = canonical_rows(x)
    if state is None:
        state = confidence_fit_reference(m, kind, **params)
    check_values(kind, par, float(m.data.min()) if m.nnz else None)
    v, j = m.data, m.indices
    rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
    if kind == "linear":
        w = 1.0 + par["alpha"] * v
    elif kind == "log":
        w = 1.0 + par["alpha"] * np.log1p(v / par["eps"])
    elif kind == "tfidf":
        w = np.sqrt(v) * state["item_table"][j]
    elif kind == "bm25":
        K1, B, sbar = par["K1"], par["B"], state["mean_row_sum"]
        s_u = np.bincount(rows, weights=v, minlength=m.shape[0])
        ratio = (B * s_u) / sbar if sbar != 0 else np.full(m.shape[0], B)
        KL = K1 * ((1.0 - B) + ratio)
        w = ((v * (K1 + 1.0)) / (KL[rows] + v)) * state["item_table"][j]
    elif par["target"] == "rows":
        t = norm_table(np.bincount(rows, weights=np.abs(v) ** par["norm"], minlength=m.shape[0]), par["scale"], par["norm"])
        w = v * t[rows]
    else:
        w = v * state["item_table"][j]
    out = sp.csr_matrix((np.asarray(w, dtype=np.float64), j.copy(), m.indptr.copy()), shape=m.shape)
    out.has_canonical_format = True
    return out


def device_backend(backend, device):
    """the backend of a stand-alone call: the one given; else HipBackend(device) when a device is present, else None (numpy)"""
    if backend is not None:
        return backend
    if not torch.cuda.is_available():
        return None
    from .engine import HipBackend
    return HipBackend(device)


def on_device(be):
    return be is not None and hasattr(be, "confidence_apply")


def upload_rows(be, m):
    """the canonical CSR m as the user-major device arrays (p, j, x): int32, int32, float64"""
    return be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32), be.to_device(m.data, torch.float64)


def device_norm(norm):
    if norm not in (1, 2):
        raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "the device path has the norms 1 and 2 only (norm = %r)" % (norm,))
    return int(norm)


class Confidence:
    """`WRMF(preprocess=Confidence("bm25"))`, or on its own: fit(x) / transform(x) / fit_transform(x), scipy in, canonical scipy CSR
    out (users as rows).  On the device (wrmf_confidence.hip) when one is present -- `backend`: an object with the HipBackend
    interface, default HipBackend(device) -- else `confidence_reference`.  The fitted state is readable as numpy: n_fit,
    item_count, item_table, mean_row_sum."""

    def __init__(self, kind, backend=None, device=None, **params):
        self.params = check_params(kind, params)
        self.kind = kind
        self._be, self._device = backend, device
        self._state = None      # host: confidence_fit_reference's dict; device: the same names, tensors

    # ---- the fitted state ---------------------------------------------------------------------------------------------------
    @property
    def fitted(self):
        return self._state is not None

    def _get(self, name):
        if self._state is None:
            raise RuntimeError("Confidence is not fitted")
        v = self._state[name]
        return v.cpu().numpy() if torch.is_tensor(v) else v

    @property
    def n_fit(self):
        return int(self._get("n_fit"))

    @property
    def item_count(self):
        c = self._get("item_count")
        return None if c is None else np.asarray(c).astype(np.int64)

    @property
    def item_table(self):
        return self._get("item_table")

    @property
    def mean_row_sum(self):
        if self._state is not None and "total" in self._state:   # (the device keeps the sum: the mean is taken where it is used)
            t, n = self._state["total"], self._state["n_fit"]
            return None if t is None else (float(t.cpu()[0]) / n if n else 0.0)
        return self._get("mean_row_sum")

    def _mean_args(self, be):
        """(a device double, a divisor) whose quotient is sbar, bit for bit, wherever the state was fitted"""
        if "total" in self._state:
            return self._state["total"], float(self._state["n_fit"])
        return be.to_device(np.array([self._state["mean_row_sum"]], dtype=np.float64), torch.float64), 1.0

    def reference_state(self):
        """the state in the form confidence_reference takes"""
        return {"n_fit": self.n_fit, "n_item": self._state["n_item"], "item_count": self.item_count, "item_table": self.item_table, "mean_row_sum": self.mean_row_sum}

    # ---- on the device arrays: what WRMF calls with its own resident arrays ----------------------------------------------------
    def _check_device_values(self, x):
        if self.kind in ("tfidf", "bm25", "log") and x.numel():
            check_values(self.kind, self.params, float(x.min()))

    def device_fit(self, be, n_rows, n_cols, um, im):
        """fit on the resident arrays: um = (p, j, x) user-major, im = (p, i, x) item-major (None where the kind needs no item
        side: "linear", "log", "normalize" along the rows), raw doubles.  -> the users' moments where the kind has some (so that
        weighting the same rows does not sum them again), else None."""
        kind, par = self.kind, self.params
        self._check_device_values(um[2])
        st = {"n_fit": int(n_rows), "n_item": int(n_cols), "item_count": None, "item_table": None, "total": None}
        mom = None
        if im is not None:
            st["item_count"] = torch.diff(im[0])
        else:   # (no item side to read them off: counted from the rows' columns, so that the state is the numpy fit's)
            st["item_count"] = torch.bincount(um[1].to(torch.int64), minlength=int(n_cols))
        if kind in ("tfidf", "bm25"):
            st["item_table"] = be.confidence_table("idf", n_cols, p=im[0], a=float(n_rows))
        if kind == "bm25":
            mom, st["total"] = be.confidence_moments(um[0], um[2], 1)
        elif kind == "normalize" and par["target"] == "columns":
            cm, _ = be.confidence_moments(im[0], im[2], device_norm(par["norm"]))
            st["item_table"] = be.confidence_table("norm", n_cols, moment=cm, a=par["scale"], b=float(par["norm"]))
        self._state = st
        return mom

    def needs_items(self):
        return self.kind in ("tfidf", "bm25") or (self.kind == "normalize" and self.params["target"] == "columns")

    def device_user_table(self, be, um, mom=None):
        """the per-user table of the rows um = (p, j, x): K1 L_u, the row scaling, or None"""
        kind, par = self.kind, self.params
        n = int(um[0].numel()) - 1
        if kind == "bm25":
            if mom is None:
                mom, _ = be.confidence_moments(um[0], um[2], 1)
            total, div = self._mean_args(be)
            return be.confidence_table("bm25", n, moment=mom, total=total, a=par["K1"], b=par["B"], c=div)
        if kind == "normalize" and par["target"] == "rows":
            mom, _ = be.confidence_moments(um[0], um[2], device_norm(par["norm"]))
            return be.confidence_table("norm", n, moment=mom, a=par["scale"], b=float(par["norm"]))
        return None

    def device_apply(self, be, arrays, user_table, item_major=False, out=None):
        """weight the resident arrays (p, i, x) of either orientation with the users' table and the fitted items' table.
        out: None = new doubles, "inplace" = over x, torch.float32 = new floats (the doubles rounded once)."""
        if self._state is None:
            raise RuntimeError("Confidence is not fitted")
        par = self.params
        a, b = {"linear": (par.get("alpha"), 0.0), "log": (par.get("alpha"), par.get("eps")), "bm25": (par.get("K1"), 0.0)}.get(self.kind, (0.0, 0.0))
        item_table = self._state["item_table"]
        if torch.is_tensor(arrays[2]) and item_table is not None and not torch.is_tensor(item_table):
            item_table = be.to_device(item_table, torch.float64)
        seg, idx = (item_table, user_table) if item_major else (user_table, item_table)
        return be.confidence_apply(self.kind, arrays[0], arrays[1], arrays[2], seg_table=seg, idx_table=idx, seg_is_item=item_major,
                                   a=a, b=b, out=out)

    def device_transform(self, be, um, out="inplace"):
        """new rows um = (p, j, x) on the device, weighted with their own row moments and the fitted item table"""
        self._check_device_values(um[2])
        return self.device_apply(be, um, self.device_user_table(be, um), out=out)

    # ---- scipy in, scipy out ------------------------------------------------------------------------------------------------
    def _backend(self):
        self._be = device_backend(self._be, self._device)
        return self._be

    def host_fit_transform(self, x):
        """fit and weight in numpy, whatever the backend (sharded fits: the statistics span the ranks' blocks)"""
        m = canonical_rows(x)
        self._state = confidence_fit_reference(m, self.kind, **self.params)
        return confidence_reference(m, self.kind, self._state, **self.params)

    def host_transform(self, x):
        return confidence_reference(x, self.kind, self.reference_state(), **self.params)

    def _fit(self, x, want, backend):
        """fit on x; want: also return x weighted"""
        m = canonical_rows(x)
        be = backend if backend is not None else self._backend()
        if not on_device(be):
            self._state = confidence_fit_reference(m, self.kind, **self.params)
            return confidence_reference(m, self.kind, self._state, **self.params) if want else None
        if self.kind == "normalize":
            device_norm(self.params["norm"])
        um = upload_rows(be, m)
        im = be.transpose_csc(m.shape[1], m.shape[0], *um) if self.needs_items() else None
        mom = self.device_fit(be, m.shape[0], m.shape[1], um, im)
        if not want:
            return None
        w = self.device_apply(be, um, self.device_user_table(be, um, mom), out="inplace")
        return _as_csr(m, w)

    def fit(self, x, backend=None):
        self._fit(x, False, backend)
        return self

    def fit_transform(self, x, backend=None):
        return self._fit(x, True, backend)

    def transform(self, x, backend=None):
        if self._state is None:
            raise RuntimeError("Confidence is not fitted")
        m = canonical_rows(x)
        if m.shape[1] != self._state["n_item"]:
            raise ValueError("x must have the columns of the matrix the confidence was fitted on")
        be = backend if backend is not None else self._backend()
        if not on_device(be):
            return self.host_transform(m)
        return _as_csr(m, self.device_transform(be, upload_rows(be, m)))


def _as_csr(m, w):
    out = sp.csr_matrix((w.cpu().numpy(), m.indices.copy(), m.indptr.copy()), shape=m.shape)
    out.has_canonical_format = True
    return out


class ScaleNormalize:
    """The reference's ScaleNormalize (R/model_ScaleNormalize.R): `fit` stores the scaling vector along `target` --
    norm_vec^(scale - 1) where norm_vec != 0, norm_vec = (sum |x|^norm)^(1 / norm) over the rows or the columns -- `transform`
    multiplies by the STORED vector (along the rows this needs the same number of rows, as in R), `fit_transform` does both.
    On the device by the kernels of `Confidence` when one is present (norm 1 or 2), else in numpy (any norm > 0)."""

    def __init__(self, scale=0.5, norm=2, target="rows", backend=None, device=None):
        par = check_params("normalize", {"scale": scale, "norm": norm, "target": target})
        self.scale, self.norm, self.target = par["scale"], par["norm"], par["target"]
        self._be, self._device = backend, device
        self._vec = None

    @property
    def scaling(self):
        """the stored vector (the diagonal of the reference's scaling_matrix), numpy"""
        if self._vec is None:
            raise RuntimeError("ScaleNormalize is not fitted")
        return self._vec.cpu().numpy() if torch.is_tensor(self._vec) else self._vec

    def _backend(self):
        self._be = device_backend(self._be, self._device)
        return self._be

    def fit(self, x):
        m = canonical_rows(x)
        be = self._backend()
        rows = self.target == "rows"
        if not on_device(be):
            idx = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr)) if rows else m.indices
            mom = np.bincount(idx, weights=np.abs(m.data) ** self.norm, minlength=m.shape[0 if rows else 1])
            self._vec = norm_table(mom, self.scale, self.norm)
            return self
        power = device_norm(self.norm)
        um = upload_rows(be, m)
        seg = um if rows else be.transpose_csc(m.shape[1], m.shape[0], *um)
        mom, _ = be.confidence_moments(seg[0], seg[2], power)
        self._vec = be.confidence_table("norm", int(mom.numel()), moment=mom, a=self.scale, b=float(power))
        return self

    def transform(self, x):
        vec = self._vec
        if vec is None:
            raise RuntimeError("ScaleNormalize is not fitted")
        m = canonical_rows(x)
        rows = self.target == "rows"
        if m.shape[0 if rows else 1] != int(vec.shape[0]):
            raise ValueError("x must have the %s of the fitted matrix" % ("number of rows" if rows else "number of columns"))
        be = self._backend()
        if not on_device(be):
            t = self.scaling
            idx = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr)) if rows else m.indices
            out = sp.csr_matrix((m.data * t[idx], m.indices.copy(), m.indptr.copy()), shape=m.shape)
            out.has_canonical_format = True
            return out
        um = upload_rows(be, m)
        if not torch.is_tensor(vec):
            vec = be.to_device(vec, torch.float64)
        w = be.confidence_apply("normalize", um[0], um[1], um[2], seg_table=vec if rows else None, idx_table=None if rows else vec,
                                out="inplace")
        return _as_csr(m, w)

    def fit_transform(self, x):
        return self.fit(x).transform(x)
