"""soft_svd / soft_impute: the reference's soft-ALS (R/SoftALS.R, R/utils_SoftALS.R) on the fused half-iteration kernel.

  soft_als_reference     the algorithm in numpy, line by line: the definition the device driver is tested against
  softals_half_reference one half-iteration per row, in double: the definition of wrmf_softals.hip
  soft_svd, soft_impute  the drivers: the matrix goes up once, the factors stay on the device for the whole fit, per iteration
                         only k x k matrices and scalars cross to the host

One half-iteration of solve_iter_als_* (R/SoftALS.R:68-102) with the `%*% diag(sqrt(d))` that follows it (:157, :174), per row r
of the CSR matrix at hand, s = d / (d + lambda), M the factor gathered by column index and W the row's own factor:
  target "svd":          out[r] = s o sum_t x_t M[j_t]
  target "soft_impute":  res_t = x_t - sum_c d_c W[r, c] M[j_t, c];   out[r] = s o (sum_t res_t M[j_t] + d o W[r])
"""
import numpy as np
import scipy.sparse as sp

from . import _lib

TARGETS = ("svd", "soft_impute")


class SoftSVD:
    """svd-like result: u (n_user x k), d (k), v (n_item x k) as numpy arrays, trace = [(frob_delta, loss)] per iteration
    (loss is NaN for target "svd", R/SoftALS.R:178-179)"""

    def __init__(self, u, d, v, trace):
        self.u, self.d, self.v, self.trace = u, d, v, trace


def softals_half_reference(p, j, x, M, W, w, s, t):
    """the kernel's formula in double: res_t = x_t - (w ? sum_c w_c W[row, c] M[j_t, c] : 0), out[row] = s o sum_t res_t M[j_t]
    + (t ? t o W[row] : 0) -> (out float64 (n_rows, r), sum_t res_t^2).  j may be unsorted and may repeat."""
    p = np.asarray(p, dtype=np.int64)
    j = np.asarray(j, dtype=np.int64)
    x = np.asarray(x, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64)
    n, r = p.size - 1, M.shape[1]
    rows = np.repeat(np.arange(n), np.diff(p))
    res = x.copy()
    if w is not None:
        Ww = np.asarray(W, dtype=np.float64) * np.asarray(w, dtype=np.float64)
        for a in range(0, res.size, 1 << 15):   # (blocks: the gathered rows of a block stay in cache)
            b = min(a + (1 << 15), res.size)
            res[a:b] -= np.einsum("tc,tc->t", Ww[rows[a:b]], M[j[a:b]])
    acc = sp.csr_matrix((res, j, p), shape=(n, M.shape[0])) @ M if res.size else np.zeros((n, r))
    out = np.asarray(acc) * np.asarray(s, dtype=np.float64)
    if t is not None:
        out = out + np.asarray(W, dtype=np.float64) * np.asarray(t, dtype=np.float64)
    return out, float(res @ res)


def shrinkage(d, lambda_):
    """s = d / (d + lambda) (R/SoftALS.R:86, :90, :101); d_c + lambda = 0 has no solution and raises as a singular system does"""
    d = np.asarray(d, dtype=np.float64)
    den = d + float(lambda_)
    if np.any(den == 0.0):
        raise _lib.RsparseHipError(_lib.ERR_NUMERIC, "soft_als: d + lambda is zero for %d singular values" % int(np.sum(den == 0.0)))
    return d / den


def half_coefficients(d, lambda_, target):
    """(w, s, t) of one half-iteration of `target` at the singular values d"""
    s = shrinkage(d, lambda_)
    if target == "soft_impute":
        return np.asarray(d, dtype=np.float64), s, s * d
    return None, s, None


def tall_skinny_factors(G):
    """svd_tall_skinny (R/SoftALS.R:250-257) from the k x k Gramian G = A^T A, in double: (d, v, R) with A = (A R) diag(d) v^T,
    R = solve(d * t(v)) -- the left factor is A R"""
    G = np.asarray(G, dtype=np.float64)
    _, sv, vt = np.linalg.svd(G)
    d = np.sqrt(sv)
    v = vt.T
    R = np.linalg.inv(d[:, None] * vt)
    return d, v, R


def frobenius_delta(d_old, utu, vtv, d_new):
    """calc_frobenius_norm_delta (R/utils_SoftALS.R:24-34) from utu = t(u_new) u_old and vtv = t(v_old) v_new"""
    denom = float(np.sum(d_old ** 2))
    a = d_new[:, None] * np.asarray(utu, dtype=np.float64)
    b = d_old[:, None] * np.asarray(vtv, dtype=np.float64)
    num = denom + float(np.sum(d_new ** 2)) - 2.0 * float(np.trace(a @ b))
    return num / max(denom, 1e-09)


def initial_left_factor(n_rows, rank, rng):
    """the starting point without `init` (R/SoftALS.R:118-123): R's RNG stream cannot be matched, so it is DEFINED as the left
    factor of the tall-skinny step applied to a standard normal draw -- orthonormal columns that span the space of qr.Q of the
    draw"""
    draw = rng.standard_normal((int(n_rows), int(rank)))
    return draw @ tall_skinny_factors(draw.T @ draw)[2]


def final_factors(sv, lambda_):
    """R/SoftALS.R:226-238: the thresholded singular values that stay, or ValueError when none does"""
    keep = np.maximum(np.asarray(sv, dtype=np.float64) - float(lambda_), 0.0)
    nz = int(np.sum(keep > 0))
    if nz == 0:
        raise ValueError("regularization lambda=%f is too high - all singular vectors are zero" % float(lambda_))
    return keep[:nz], nz


def soft_als_reference(x, rank, lambda_, n_iter, convergence_tol, target, u0, final_svd=True, dtype=np.float64, d0=None, v0=None):
    """soft_als (R/SoftALS.R:107-245) in numpy from the left factor u0 (n_user x rank), d = 1 and v = 0 (:129-135; d0, v0: a
    warm start's, :137-142).  The factors
    and the two sparse passes per iteration are in `dtype` (sums in double, one rounding: what the kernel does), the k x k
    algebra in double.  -> (u, d, v, trace)"""
    if target not in TARGETS:
        raise ValueError("target must be one of %s" % (TARGETS,))
    dt = np.dtype(dtype)
    x = sp.csr_matrix(x, dtype=np.float64)
    tx = sp.csr_matrix(x.T)                                                            # :117
    xv, txv = x.data.astype(dt), tx.data.astype(dt)
    lam = float(lambda_)
    u = np.ascontiguousarray(u0, dtype=dt)
    d = np.ones(int(rank)) if d0 is None else np.asarray(d0, dtype=np.float64)
    v = np.zeros((x.shape[1], int(rank)), dtype=dt) if v0 is None else np.ascontiguousarray(v0, dtype=dt)
    if u.shape != (x.shape[0], int(rank)):
        raise ValueError("u0 must be n_user x rank")

    def half(m, vals, M, W, dd, s1=False):
        w, s, t = half_coefficients(dd, lam, target)
        if s1:
            s, t = np.ones_like(dd), None
        out, sumsq = softals_half_reference(m.indptr, m.indices, vals, M, W, w, s, t)
        return out.astype(dt), sumsq

    def tall_skinny(A):                                                                # :250-257
        dd, vk, R = tall_skinny_factors((A.T @ A).astype(np.float64))
        return dd, vk, A @ R.astype(dt)

    trace = []
    for _ in range(int(n_iter)):
        u_old, d_old, v_old = u, d, v
        B, _ = half(tx, txv, u, v, d)                                                  # :155-160
        d, vk, v = tall_skinny(B)                                                      # :163-167
        u = u @ vk.astype(dt)                                                          # :169
        A, sumsq = half(x, xv, v, u, d)                                                # :172-177
        loss = (sumsq + lam * float(np.sum(d))) / x.nnz if target == "soft_impute" else float("nan")   # :83
        d, vk, u = tall_skinny(A)                                                      # :182-186
        v = v @ vk.astype(dt)                                                          # :188
        delta = frobenius_delta(d_old, (u.T @ u_old).astype(np.float64), (v_old.T @ v).astype(np.float64), d)   # :192
        trace.append((delta, loss))
        if delta < convergence_tol:                                                    # :203
            break
    if final_svd:                                                                      # :214-243
        m, _ = half(x, xv, v, u, d, s1=True)
        if target == "soft_impute":
            m = m + (u * d.astype(dt)) @ (v.T @ v)                                     # :220
        mu, sv, mvt = np.linalg.svd(m.astype(np.float64), full_matrices=False)
        d, nz = final_factors(sv, lam)
        u = mu[:, :nz].astype(dt)
        v = (v.astype(np.float64) @ mvt.T)[:, :nz].astype(dt)                          # :242
    return u, d, v, trace


def _check_init(init, n_user, n_item, rank):
    u, d, v = (np.asarray(getattr(init, n) if hasattr(init, n) else init[n], dtype=np.float64) for n in ("u", "d", "v"))
    if d.ndim != 1 or u.ndim != 2 or v.ndim != 2 or u.shape[1] != d.size or v.shape[1] != d.size:
        raise ValueError("init must hold u (n_user x k), d (k) and v (n_item x k)")
    if d.size > rank:
        raise ValueError("provided initial svd 'init' has bigger rank than model rank")   # R/SoftALS.R:140-141
    if d.size < rank:
        raise NotImplementedError("init of a smaller rank than the model's (the reference's pad_svd) is not implemented")
    if u.shape[0] != n_user or v.shape[0] != n_item:
        raise ValueError("init does not have the shape of x")
    return u, d, v


def _soft_als_device(be, x, rank, lam, n_iter, convergence_tol, target, u0, d0, v0, final_svd, dt):
    import torch
    tdt = torch.float64 if dt == np.float64 else torch.float32
    p, j = be.to_device(x.indptr, torch.int32), be.to_device(x.indices, torch.int32)
    xv = be.to_device(x.data, tdt)
    n_user, n_item = x.shape
    tp, tj, txv = be.transpose_csc(n_item, n_user, p, j, xv)                          # t(x), :117
    nnz = int(x.nnz)
    u = be.to_device(u0, tdt)
    v = be.to_device(v0, tdt)
    d = np.asarray(d0, dtype=np.float64)
    G = torch.empty((rank, rank), dtype=tdt, device=u.device)

    def small(a):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=tdt).to(u.device)

    def tall_skinny(A):                                                                # :250-257
        be.gramian(A, 0.0, G, None)
        dd, vk, R = tall_skinny_factors(G.cpu().numpy())
        return dd, vk, A @ small(R)

    trace = []
    for _ in range(int(n_iter)):
        u_old, d_old, v_old = u, d, v
        w, s, t = half_coefficients(d, lam, target)
        B, _ = be.softals_half(tp, tj, txv, u, v if w is not None else None, w, s, t)  # :155-160
        d, vk, v = tall_skinny(B)
        u = u @ small(vk)                                                              # :169
        w, s, t = half_coefficients(d, lam, target)
        A, sumsq = be.softals_half(p, j, xv, v, u if w is not None else None, w, s, t, want_sumsq=w is not None)   # :172-177
        loss = (float(sumsq.cpu()[0]) + lam * float(np.sum(d))) / nnz if target == "soft_impute" else float("nan")
        d, vk, u = tall_skinny(A)
        v = v @ small(vk)                                                              # :188
        delta = frobenius_delta(d_old, (u.T @ u_old).cpu().numpy(), (v_old.T @ v).cpu().numpy(), d)
        trace.append((delta, loss))
        if delta < convergence_tol:
            break
    if final_svd:                                                                      # :214-243
        impute = target == "soft_impute"
        m, _ = be.softals_half(p, j, xv, v, u if impute else None, d if impute else None, np.ones_like(d), None)
        if impute:
            be.gramian(v, 0.0, G, None)   # t(v) v by the Gramian kernel: its sum over n_item rows is rounded less than a GEMM's
            m = m + (u * small(d)) @ G                                                 # :220
        # svd(m) of the n_user x k matrix through its Gramian: m = (m mv diag(1 / sv)) diag(sv) mv^T.  The threshold acts on the
        # SMALL singular values, which a Gramian in float loses (their squares lie below the rounding of the largest): this
        # one product, once per fit, is taken in double whatever the factors' type
        if tdt == torch.float64:
            be.gramian(m, 0.0, G, None)
            Gm = G.cpu().numpy()
        else:
            m64 = m.to(torch.float64)
            Gm = (m64.T @ m64).cpu().numpy()
        _, ev, mvt = np.linalg.svd(Gm.astype(np.float64))
        sv = np.sqrt(ev)
        d, nz = final_factors(sv, lam)
        mv = mvt.T[:, :nz]
        u = m @ small(mv / sv[:nz])
        v = v @ small(mv)                                                              # :242
    return u.cpu().numpy(), d, v.cpu().numpy(), trace


def _soft_als(x, rank, lambda_, n_iter, convergence_tol, init, final_svd, precision, rng, device, backend, target):
    if precision not in ("double", "float"):
        raise ValueError("precision must be 'double' or 'float'")
    if not isinstance(final_svd, (bool, np.bool_)):
        raise TypeError("final_svd must be a logical")                                 # :114
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "soft_als does not shard: fit on one rank")
    rank = int(rank)
    if rank < 1:
        raise ValueError("rank must be at least 1")
    x = sp.csr_matrix(x, dtype=np.float64)
    x.sum_duplicates()
    x.sort_indices()
    if x.nnz == 0:
        raise ValueError("x has no stored entries")
    n_user, n_item = x.shape
    if init is None:
        gen = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        u0, d0, v0 = initial_left_factor(n_user, rank, gen), np.ones(rank), np.zeros((n_item, rank))   # :118-135
    else:
        u0, d0, v0 = _check_init(init, n_user, n_item, rank)
    dt = np.float64 if precision == "double" else np.float32
    if backend is None:
        from .engine import HipBackend
        backend = HipBackend(device)
    if not hasattr(backend, "softals_half"):   # (the CPU stand-in of the tests: the definition itself)
        return SoftSVD(*soft_als_reference(x, rank, lambda_, n_iter, convergence_tol, target, u0, bool(final_svd), dt, d0, v0))
    if rank > _lib.MAX_RANK:
        raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "soft_als: rank > %d is not on the device path" % _lib.MAX_RANK)
    if dt == np.float64 and rank > _lib.MAX_RANK_F64:
        raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "soft_als(precision='double'): rank > %d is not on the device path "
                                       "(the double Gramian ends there); use precision='float'" % _lib.MAX_RANK_F64)
    return SoftSVD(*_soft_als_device(backend, x, rank, float(lambda_), n_iter, convergence_tol, target, u0, d0, v0,
                                     bool(final_svd), dt))


def soft_svd(x, rank=10, lambda_=0.0, n_iter=100, convergence_tol=1e-3, init=None, final_svd=True, precision="double", rng=None,
             device=None, backend=None):
    """R/SoftALS.R:54-63: truncated SVD of a sparse users x items matrix by alternating least squares, with the singular values
    soft-thresholded by `lambda_` -> SoftSVD (u, d, v, trace); the rank may come out below `rank`"""
    return _soft_als(x, rank, lambda_, n_iter, convergence_tol, init, final_svd, precision, rng, device, backend, "svd")


def soft_impute(x, rank=10, lambda_=0.0, n_iter=100, convergence_tol=1e-3, init=None, final_svd=True, precision="double",
                rng=None, device=None, backend=None):
    """R/SoftALS.R:40-49: the same for a matrix whose absent entries are unknown, not zero (SoftImpute-ALS)"""
    return _soft_als(x, rank, lambda_, n_iter, convergence_tol, init, final_svd, precision, rng, device, backend, "soft_impute")
