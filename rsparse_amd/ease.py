"""EASE (Steck 2019, "Embarrassingly Shallow Autoencoders for Sparse Data"): ridge regression of every item column on all the others,
in closed form, scored by a dense items x items matrix.

The definition (include/rsparse_wrmf_hip.h repeats it for C hosts; wrmf_ease.hip computes the Gram rows and the lists on the device):

Input.  x is reduced to its canonical PATTERN with `itemknn.canonical_pattern` -- duplicates summed, explicit zeros dropped, values
otherwise ignored: this is the binary model.  H is that pattern as a 0 / 1 matrix, n_j the number of users of item j.

Gram.  A = G + lambda I in float64 with G = H^T H: off the diagonal c_ij, the co-occurrence count, an exact integer; on the diagonal
n_j + lambda, one rounding.  n_items <= 32768 (`_lib.EASE_MAX_ITEMS`: an items x items matrix of doubles is 8 GiB there).

Weights.  P = inv(A) in float64, whatever the model's precision; B = -(P / diag(P)[None, :]), one division per entry, then the
diagonal set to +0.0; B is cast to the model's dtype (float32 for precision "float", float64 for "double") with one rounding.  A
P_jj that is not positive and finite, or a factorisation that fails, is RsparseHipError(ERR_NUMERIC): at lambda = 0 the Gram matrix
of a real interaction matrix is singular (two items with the same users, an item without any).

Scores.  For a row u of x, acc starts as n_items doubles at +0.0; for the stored items i_t of the row IN ASCENDING STORED ORDER,
acc += double(B[i_t, :]).  A sequential sum in a stated order: a float32 B converts exactly, so each step is one rounding.  The score
row is acc itself, float64, not rounded to float.

Lists.  The k admissible items (outside the row's not_recommend entries and outside items_exclude) of largest score, ties to the
smaller item; fewer than k admissible items pad as `knn_recommend_reference` pads (-1, score 0).  The ORDER is that of the monotone
64-bit key of the double,

    key(v) = ~bits(v) if v is negative (sign bit set), bits(v) | 2^63 otherwise                                  (`score_keys`)

compared as an unsigned integer.  An accumulator that starts at +0.0 can never become -0.0 (x + y is -0.0 only if both are), so equal
scores have equal keys; and no finite score maps to the key 0 (that would be the NaN of all ones) or to the all-ones sentinel (a
positive NaN): the device keeps 0 for "no cell" and all ones for "masked".

  ease_gram_reference, ease_weights_reference, ease_scores_reference, ease_recommend_reference      the definition, in numpy
  ease_score_pairs_reference, ease_candidates_reference, ease_ranks_reference      the same scores under the evaluation protocols of
                                    the other models: at given cells, ranked within per-row candidates, counted against held-out items
  score_keys, key_scores            the order key and its inverse
  spd_inverse, cholesky_inverse_blocked, weights_from_inverse      the factorisation (torch.linalg.cholesky_ex, torch.cholesky_inverse /
                                    torch.cholesky_solve) and the step from P to B
  EASE                              the model: fit / predict / evaluate / similar_items, and score / sample_negatives /
                                    held_out_ranks / evaluate_ranks with the conventions of `ItemKNN`'s
"""
import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from .itemknn import _admissible_rows, canonical_pattern, evaluate_lists
from .wrmf import WRMF, TopItems

PRECISIONS = {"float": np.float32, "double": np.float64}
ROW_BYTES = 256   # every row of the resident B starts at a multiple of this


def _numeric(msg):
    return _lib.RsparseHipError(_lib.ERR_NUMERIC, msg)


def _check_lambda(lambda_):
    lambda_ = float(lambda_)
    if not (np.isfinite(lambda_) and lambda_ >= 0):
        raise ValueError("lambda_ must be finite and >= 0")
    return lambda_


def ease_gram_reference(x, lambda_):
    """-> A = G + lambda I, (n_items, n_items) float64: the co-occurrence counts off the diagonal, n_j + lambda on it"""
    lambda_ = _check_lambda(lambda_)
    m = canonical_pattern(x)
    h = sp.csr_matrix((np.ones(m.nnz, dtype=np.int64), m.indices, m.indptr), shape=m.shape)
    a = np.asarray((h.T @ h).todense(), dtype=np.int64).astype(np.float64)
    np.fill_diagonal(a, np.diff(h.tocsc().indptr).astype(np.float64) + np.float64(lambda_))
    return a


def ease_weights_reference(A, dtype=np.float64):
    """-> B (n_items, n_items) of `dtype`: P = inv(A) in float64, B = -(P / diag(P)[None, :]), the diagonal +0.0, one rounding into
    dtype.  A singular A, or a P_jj that is not positive and finite: RsparseHipError(ERR_NUMERIC)."""
    A = np.asarray(A, dtype=np.float64)
    try:
        P = np.linalg.inv(A)
    except np.linalg.LinAlgError as e:
        raise _numeric("EASE: G + lambda I is singular (%s); at lambda = 0 the Gram matrix of a real matrix is" % e)
    d = np.diag(P)
    if not (np.isfinite(d).all() and (d > 0).all()):
        raise _numeric("EASE: a diagonal entry of the inverse is not positive and finite (lambda = 0 makes the Gram matrix singular)")
    B = -(P / d[None, :])
    np.fill_diagonal(B, 0.0)
    return B.astype(dtype)


def ease_scores_reference(x, B):
    """-> (n_rows, n_items) float64: acc += double(B[i_t, :]) over the stored items of every row in ascending stored order.  A loop
    over the position t, vectorised over the rows that have one and over the columns."""
    B = np.asarray(B)
    m = canonical_pattern(x, B.shape[0])
    acc = np.zeros(m.shape, dtype=np.float64)
    lens = np.diff(m.indptr)
    for t in range(int(lens.max()) if lens.size else 0):
        rows = np.flatnonzero(lens > t)
        acc[rows] += B[m.indices[m.indptr[rows] + t]].astype(np.float64)
    return acc


def score_keys(v):
    """float64 -> uint64: the order key of the definition"""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def key_scores(key):
    """uint64 (or the same bits as int64) -> float64: the inverse of `score_keys`"""
    k = np.ascontiguousarray(key).view(np.uint64)
    return np.where(k >> np.uint64(63), k ^ np.uint64(1 << 63), ~k).view(np.float64)


def ease_recommend_reference(x, B, k, not_recommend=None, items_exclude=()):
    """-> (items (n, k) int64, 0-based with -1 where fewer than k items are admissible; scores (n, k) float64, 0 there): the lists
    of the definition, by the order key of the score, ties to the smaller item"""
    score = ease_scores_reference(x, B)
    n, n_items = score.shape
    k = int(k)
    nr = None
    if not_recommend is not None:
        nr = sp.csr_matrix(not_recommend)
        if nr.shape != score.shape:
            raise ValueError("not_recommend must have the shape of x")
    excl = np.asarray(list(items_exclude), dtype=np.int64)
    items = np.full((n, k), -1, dtype=np.int64)
    scores = np.zeros((n, k), dtype=np.float64)
    for u in range(n):
        adm = np.ones(n_items, dtype=bool)
        if nr is not None:
            adm[nr.indices[nr.indptr[u]:nr.indptr[u + 1]]] = False
        adm[excl] = False
        cand = np.flatnonzero(adm)
        first = cand[np.lexsort((cand, ~score_keys(score[u, cand])))[:k]]   # (~key ascending = key descending)
        items[u, :first.size] = first
        scores[u, :first.size] = score[u, first]
    return items, scores


def ease_score_pairs_reference(x, B, pairs):
    """-> float64, one per stored position of canonical_pattern(pairs) (a sparse matrix of x's shape): the score of
    `ease_scores_reference` at that cell.  Nothing is masked."""
    score = ease_scores_reference(x, B)
    pat = canonical_pattern(pairs, score.shape[1])
    if pat.shape != score.shape:
        raise ValueError("pairs must have the shape of x")
    rows = np.repeat(np.arange(pat.shape[0]), np.diff(pat.indptr))
    return score[rows, pat.indices].astype(np.float64)


def ease_candidates_reference(x, B, candidates, k, not_recommend=None, items_exclude=()):
    """-> (items (n, k) int64 with -1, scores (n, k) float64 with 0 in the padding): `ease_recommend_reference` within per-row
    candidates.  The admissible items of a row are the stored positions of its row of canonical_pattern(candidates) minus the
    row's not_recommend entries minus items_exclude; the order is that of the score's key, descending, equal scores to the SMALLER
    item.  Candidates of score 0 are ranked; a list is shorter than k only when fewer than k candidates are admissible."""
    score = ease_scores_reference(x, B)
    cand = canonical_pattern(candidates, score.shape[1])
    if cand.shape != score.shape:
        raise ValueError("candidates must have the shape of x")
    adm = _admissible_rows(score.shape, not_recommend, items_exclude)
    k = int(k)
    items = np.full((score.shape[0], k), -1, dtype=np.int64)
    scores = np.zeros((score.shape[0], k), dtype=np.float64)
    for u in range(score.shape[0]):
        c = cand.indices[cand.indptr[u]:cand.indptr[u + 1]].astype(np.int64)
        c = c[adm(u)[c]]
        first = c[np.lexsort((c, ~score_keys(score[u, c])))[:k]]
        items[u, :first.size] = first
        scores[u, :first.size] = score[u, first]
    return items, scores


def ease_ranks_reference(x, B, actual, not_recommend=None, items_exclude=()):
    """-> (above, tied: int32, one per stored entry of `actual` (CSR with sorted columns, duplicates merged, stored zeros kept);
    n_adm: int32 per row), exactly as `itemknn.knn_ranks_reference` defines them with s the double score: A_u = the items outside
    the not_recommend row and outside items_exclude, n_adm = |A_u|; above = #{j in A_u : s_j > s_h}, tied = #{j in A_u, j != h :
    s_j == s_h}; an entry outside A_u (or outside the items) gets -1 / -1."""
    from .metrics import canonical_actual
    score = ease_scores_reference(x, B)
    n, n_items = score.shape
    act = canonical_actual(actual, n)
    adm = _admissible_rows(score.shape, not_recommend, items_exclude)
    above = np.full(act.nnz, -1, dtype=np.int32)
    tied = np.full(act.nnz, -1, dtype=np.int32)
    n_adm = np.zeros(n, dtype=np.int32)
    for u in range(n):
        a = adm(u)
        n_adm[u] = a.sum()
        s_adm = score[u, a]
        for e in range(act.indptr[u], act.indptr[u + 1]):
            h = int(act.indices[e])
            if 0 <= h < n_items and a[h]:
                above[e] = np.count_nonzero(s_adm > score[u, h])
                tied[e] = np.count_nonzero(s_adm == score[u, h]) - 1
    return above, tied, n_adm


INVERSE_BLOCK = 2048   # right-hand sides of one torch.cholesky_solve


def cholesky_inverse_blocked(L, block=INVERSE_BLOCK):
    """-> inv(L L^T) for the lower Cholesky factor L: torch.cholesky_solve on `block` columns of the identity at a time.  Up to
    `block` items this is torch.cholesky_inverse itself (one potrs on the identity); beyond, the right-hand sides are cut, because
    hipSOLVER's potrs refuses n = nrhs = 20 000 (HIPSOLVER_STATUS_INTERNAL_ERROR from torch.cholesky_inverse) where it takes the
    same solve in pieces."""
    n = int(L.shape[0])
    if n <= block:
        return torch.cholesky_inverse(L)
    P = torch.empty_like(L)
    for c0 in range(0, n, block):
        c1 = min(c0 + block, n)
        rhs = torch.zeros((n, c1 - c0), dtype=L.dtype, device=L.device)
        rhs[c0:c1].fill_diagonal_(1.0)
        P[:, c0:c1] = torch.cholesky_solve(rhs, L)
    return P


def spd_inverse(A):
    """-> P = inv(A) for the symmetric positive definite float64 tensor A, on A's device: torch.linalg.cholesky_ex, then
    `cholesky_inverse_blocked`.  A factorisation that fails is RsparseHipError(ERR_NUMERIC).  A torch build without a dense solver
    for the device (it raises RuntimeError) is answered on the host, by LAPACK, and the result goes back: `spd_inverse.on_host`
    says whether that happened in the last call."""
    assert A.dtype == torch.float64 and A.dim() == 2 and A.shape[0] == A.shape[1]

    def run(a):
        L, info = torch.linalg.cholesky_ex(a)
        if int(info) != 0:
            raise _numeric("EASE: the Cholesky factorisation of G + lambda I failed at pivot %d; at lambda = 0 the Gram matrix of a "
                           "real interaction matrix is singular" % int(info))
        return cholesky_inverse_blocked(L)
    spd_inverse.on_host = False
    if not A.is_cuda:
        return run(A)
    try:
        return run(A)
    except _lib.RsparseHipError:
        raise
    except RuntimeError:
        spd_inverse.on_host = True
        return run(A.cpu()).to(A.device)


spd_inverse.on_host = False


def weights_from_inverse(P, dtype, ld=None):
    """-> B of the definition from P (a float64 tensor) as an (n_items, ld) tensor of `dtype` on P's device whose first n_items
    columns are B and whose others are zeros (ld: default n_items).  A P_jj that is not positive and finite: ERR_NUMERIC."""
    n = int(P.shape[0])
    d = P.diagonal()
    if n and not bool((torch.isfinite(d) & (d > 0)).all()):
        raise _numeric("EASE: a diagonal entry of the inverse is not positive and finite (lambda = 0 makes the Gram matrix singular)")
    B = torch.zeros((n, n if ld is None else int(ld)), dtype=dtype, device=P.device)
    if n:
        B[:, :n].copy_(-(P / d[None, :]))   # (one division, an exact negation, one rounding into dtype)
        B[:, :n].fill_diagonal_(0.0)
    return B


class EASE:
    """The closed-form item-item model of Steck 2019 (the module's docstring is the definition).

    lambda_: the ridge term, finite and >= 0 (500 suits MovieLens-sized data; 0 is singular on real data); precision: "float" or
    "double", the dtype of the resident weights B (the factorisation is float64 either way); device / backend: as `WRMF`.  A
    backend without `item_gram` / `ease_recommend` (the CPU stand-in of the tests) runs the numpy definitions.
    Fitted: `B` (downloaded on access), `item_count`."""

    def __init__(self, lambda_=500.0, precision="float", device=None, backend=None):
        self._lambda = _check_lambda(lambda_)
        if precision not in PRECISIONS:
            raise ValueError("precision must be 'float' or 'double'")
        self._dtype = PRECISIONS[precision]
        self._device = device
        self._be = backend
        self._B = None          # the (n_items, ld) tensor of the backend; its first n_items columns are B
        self.item_count = None
        self._n_items = None

    def _backend(self):
        if self._be is None:
            from .engine import HipBackend
            self._be = HipBackend(self._device)
        return self._be

    @staticmethod
    def _one_rank():
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "EASE does not shard over torch.distributed ranks")

    def _fitted(self):
        if self._B is None:
            raise RuntimeError("model is not fitted")

    @property
    def B(self):
        """the weights, (n_items, n_items) of the model's dtype, as a numpy array"""
        self._fitted()
        return self._B[:, :self._n_items].cpu().numpy().copy()

    def fit(self, x, ws_rows=0):
        """the weights of the users x items matrix x -> self (`B` stays on the device, `item_count`)"""
        self._one_rank()
        m = canonical_pattern(x)
        n_users, n_items = m.shape
        if n_items > _lib.EASE_MAX_ITEMS:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "n_items > 32768: an items x items matrix of doubles would pass 8 GiB")
        be = self._backend()
        t_dtype = torch.float32 if self._dtype == np.float32 else torch.float64
        if not hasattr(be, "item_gram"):
            B = torch.from_numpy(ease_weights_reference(ease_gram_reference(m, self._lambda), self._dtype))
            cnt = np.bincount(m.indices, minlength=n_items).astype(np.int64)
        else:
            up, uj = be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32)
            ones = torch.ones(int(uj.numel()), dtype=torch.float32, device=uj.device)
            # the CSR rows of x are the CSC columns of its transpose (items x users): transposed, item -> its users
            ip, iu, _ = be.transpose_csc(n_items, n_users, up, uj, ones)
            A = be.item_gram(ip, iu, up, uj, n_users, n_items, self._lambda, ws_rows=ws_rows)
            cnt = np.diff(ip.cpu().numpy().astype(np.int64))
            P = spd_inverse(A)
            del A
            elems = ROW_BYTES // np.dtype(self._dtype).itemsize
            B = weights_from_inverse(P, t_dtype, (n_items + elems - 1) // elems * elems)
        self._B, self._n_items, self.item_count = B, n_items, cnt
        return self

    def _rows(self, x, not_recommend="x", items_exclude=()):
        """what every scoring call starts with -> (m: x as a canonical pattern, be, not_recommend as CSR or None, items_exclude
        sorted and unique)"""
        self._fitted()
        self._one_rank()
        n_items = self._n_items
        m = canonical_pattern(x, n_items)
        excl = np.unique(np.asarray(list(items_exclude), dtype=np.int64))
        if excl.size and (excl.min() < 0 or excl.max() >= n_items):
            raise ValueError("some of items_exclude indices are bigger than number of items")
        if isinstance(not_recommend, str) and not_recommend == "x":
            not_recommend = m
        if not_recommend is not None:
            if not sp.issparse(not_recommend):
                raise TypeError("'not_recommend' should be NULL or 'sparseMatrix'")
            not_recommend = sp.csr_matrix(not_recommend)
            if not_recommend.shape != m.shape:
                raise ValueError("not_recommend must have the shape of x")
        return m, self._backend(), not_recommend, excl

    def _host_B(self):
        return self._B[:, :self._n_items].cpu().numpy()

    @staticmethod
    def _device_filters(be, not_recommend, excl):
        nr_p = nr_j = None
        if not_recommend is not None and not_recommend.nnz:
            nr_p, nr_j = be.to_device(not_recommend.indptr, torch.int32), be.to_device(not_recommend.indices, torch.int32)
        return {"nr_p": nr_p, "nr_j": nr_j, "exclude0": be.to_device(excl, torch.int32) if len(excl) else None}

    @staticmethod
    def _pattern(pairs, m, what):
        """`pairs` (a scipy sparse of x's shape) as a canonical CSR pattern of ones: columns ascending, duplicates merged, every
        stored position kept (a stored zero too)"""
        if not sp.issparse(pairs):
            raise TypeError("'%s' should be a 'sparseMatrix'" % what)
        if pairs.shape != m.shape:
            raise ValueError("%s must have the shape of x" % what)
        pat = sp.csr_matrix(pairs, dtype=np.float64, copy=True)
        pat.data[:] = 1.0
        return canonical_pattern(pat)

    def _lists(self, x, k, not_recommend, items_exclude, ws_rows=0, candidates=None):
        """-> (items int32 (n, k) 1-based with NA_integer_, scores float64 (n, k) numpy with NaN where NA); candidates: a scipy
        sparse of x's shape, or None (the whole catalogue)"""
        m, be, not_recommend, excl = self._rows(x, not_recommend, items_exclude)
        n_items = self._n_items
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError("k must be an integer >= 1")
        if k > _lib.KNN_MAX_TOPK:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "predict: k > 1024 is not on the device path")
        cand = None if candidates is None else self._pattern(candidates, m, "candidates")
        if not hasattr(be, "ease_recommend" if cand is None else "ease_top_candidates"):
            if cand is None:
                it, sc = ease_recommend_reference(m, self._host_B(), k, not_recommend, excl)
            else:
                it, sc = ease_candidates_reference(m, self._host_B(), cand, k, not_recommend, excl)
            res = np.where(it < 0, np.int64(-2147483648), it + 1).astype(np.int32)
            return torch.from_numpy(res), np.where(it < 0, np.nan, sc)
        filters = self._device_filters(be, not_recommend, excl)
        xp, xj = be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32)
        if cand is None:
            res, keys = be.ease_recommend(xp, xj, self._B, n_items, k, filters["nr_p"], filters["nr_j"], filters["exclude0"], ws_rows=ws_rows)
        else:
            res, keys = be.ease_top_candidates(xp, xj, self._B, n_items, k, be.to_device(cand.indptr, torch.int32),
                                               be.to_device(cand.indices, torch.int32), ws_rows=ws_rows, **filters)
        pad = (res == -2147483648).cpu().numpy()
        return res, np.where(pad, np.nan, key_scores(keys.cpu().numpy()))

    def predict(self, x, k, not_recommend="x", items_exclude=(), ws_rows=0, candidates=None):
        """the k best items of every row of x, with the conventions of `ItemKNN.predict`: `not_recommend` (default: x itself; None =
        nothing) and `items_exclude` (0-based) are skipped; -> `TopItems` (n x k, 0-based, -1 where fewer than k items are
        admissible) with `.scores` (float64, the sums of the definition; NaN in the padding).  1 <= k <= 1024.

        `candidates` (a scipy sparse of x's shape; its values are ignored): every row is ranked within its own stored positions
        -- two-stage serving, a catalogue slice per user, sampled-negative evaluation.  The filters still apply; candidates of
        score 0 are ranked; a list is shorter than k only when fewer than k candidates are admissible.  The order is the model's
        own -- score descending, equal scores to the SMALLER item -- and NOT the reference heap's rule that
        `WRMF.predict(candidates=)` follows.  `candidates` holding every item reproduces `predict(x, k)` exactly.  A row of few
        candidates is scored at its cells of B alone; one of many through its dense score row (`_lib.EASE_CELLS_RATIO`)."""
        res, sc = self._lists(x, k, not_recommend, items_exclude, ws_rows, candidates)
        idx = res.cpu().numpy().astype(np.int64)
        out = np.where(idx == -2147483648, -1, idx - 1).view(TopItems)
        out.scores = sc
        return out

    def sample_negatives(self, x, n, actual=None, not_recommend="x", items_exclude=(), seed=None, weights=None):
        """`WRMF.sample_negatives` for the shape of x: the candidate matrix of a sampled-metric evaluation -- every row's stored
        positions of `actual` plus min(n, admissible) items drawn without replacement from those neither in `not_recommend`, nor
        in `actual`, nor in `items_exclude`.  The negatives depend on (seed, row, the row's exclusions, n_items, n) alone, so they
        ARE the ones `WRMF.sample_negatives(x, n, actual=, seed=)` returns for that seed.  `seed` is required: EASE has no
        generator to draw one from."""
        if seed is None:
            raise ValueError("sample_negatives needs a seed: EASE has no generator to draw one from")
        self._one_rank()
        return WRMF(backend=self._backend()).sample_negatives(x, n, actual=actual, not_recommend=not_recommend,
                                                              items_exclude=items_exclude, seed=seed, weights=weights)

    def score(self, x, pairs, ws_rows=0):
        """the model's score of the rows of x at given (user, item) cells: a scipy CSR matrix (float64) with the pattern of `pairs`
        (x's shape; columns sorted, duplicates merged, stored zeros are positions too) and, as values, the sums of the definition,
        the bits `predict`'s `.scores` have.  Nothing is masked: an item of the row's own history has its score too."""
        m, be, _, _ = self._rows(x, None)
        pat = self._pattern(pairs, m, "pairs")
        if not hasattr(be, "ease_score_pairs"):
            sc = ease_score_pairs_reference(m, self._host_B(), pat)
        else:
            keys = be.ease_score_pairs(be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32), self._B, self._n_items,
                                       be.to_device(pat.indptr, torch.int32), be.to_device(pat.indices, torch.int32), ws_rows=ws_rows)
            sc = key_scores(keys.cpu().numpy())
        return sp.csr_matrix((sc, pat.indices, pat.indptr), shape=pat.shape)

    def _ranks(self, x, actual, not_recommend, items_exclude, ws_rows=0):
        """-> (be, actual as canonical CSR, (above, tied, n_adm) as tensors of the backend)"""
        from .metrics import canonical_actual
        m, be, not_recommend, excl = self._rows(x, not_recommend, items_exclude)
        if not sp.issparse(actual):
            raise TypeError("'actual' should be a 'sparseMatrix'")
        if actual.shape != m.shape:
            raise ValueError("actual must have the shape of x")
        act = canonical_actual(actual, m.shape[0])
        if not hasattr(be, "ease_held_out_ranks"):
            got = ease_ranks_reference(m, self._host_B(), act, not_recommend, excl)
            return be, act, tuple(be.to_device(v, torch.int32) for v in got)
        got = be.ease_held_out_ranks(be.to_device(m.indptr, torch.int32), be.to_device(m.indices, torch.int32), self._B, self._n_items,
                                     be.to_device(act.indptr, torch.int32), be.to_device(act.indices, torch.int32), ws_rows=ws_rows,
                                     **self._device_filters(be, not_recommend, excl))
        return be, act, got

    def held_out_ranks(self, x, actual, not_recommend="x", items_exclude=(), ws_rows=0):
        """where every held-out interaction stands among ALL the items the user could be shown, by the model's score:
        `WRMF.held_out_ranks` for this model.  The admissible items of a row are those outside its `not_recommend` row (default:
        x itself) and outside `items_exclude`; for every stored entry (u, h) of `actual` (x's shape; stored zeros are entries):
        above = admissible items scored strictly higher than h, tied = other admissible items with an equal score, -1 / -1 when h
        itself is not admissible.  -> (above, tied: scipy CSR (int32) with the canonical pattern of `actual`; n_adm: the
        admissible items per row, int32).  The 0-based midrank of an entry is above + tied / 2."""
        _, act, (above, tied, n_adm) = self._ranks(x, actual, not_recommend, items_exclude, ws_rows)
        mk = lambda v: sp.csr_matrix((v.cpu().numpy().astype(np.int32), act.indices.copy(), act.indptr.copy()), shape=act.shape)
        return mk(above), mk(tied), n_adm.cpu().numpy().astype(np.int32)

    def evaluate_ranks(self, x, actual, not_recommend="x", items_exclude=(), per_user=False):
        """the full-ranking metrics of the held-out interactions `actual` (values = weights) from `held_out_ranks`' counts, with
        the formulas and the return shape of `WRMF.evaluate_ranks`: {"mpr", "auc", "mrr", "n"}; per_user=True adds "mpr_per_user",
        "auc_per_user", "mrr_per_user" and "n_adm_per_user"."""
        from .metrics import rank_totals
        be, act, (above, tied, n_adm) = self._ranks(x, actual, not_recommend, items_exclude)
        fn = be.rank_summary if hasattr(be, "rank_summary") else WRMF._rank_summary_host
        mpr, auc, mrr, sums = fn(be.to_device(act.indptr, torch.int32), be.to_device(act.data, torch.float64), above, tied, n_adm)
        sums = sums.cpu().numpy()
        per = {"mpr": mpr.cpu().numpy(), "auc": auc.cpu().numpy(), "mrr": mrr.cpu().numpy()}
        out = rank_totals({"sum_w": sums[:, 0], "sum_w_pct": sums[:, 1], "P": sums[:, 2], "auc": per["auc"], "mrr": per["mrr"]})
        if per_user:
            out.update({name + "_per_user": v for name, v in per.items()})
            out["n_adm_per_user"] = n_adm.cpu().numpy().astype(np.int32)
        return out

    def evaluate(self, x, actual, k, not_recommend="x", items_exclude=(), metrics=("ap", "ndcg"), diversify=None, candidates=None,
                 negatives=None, seed=None, negative_weights=None):
        """`predict(x, max(k), ...)` once, scored against the held-out `actual` by the package's list metrics, routed exactly as
        `ItemKNN.evaluate` routes them: "ap", "ndcg", "precision", "recall", "hit", "mrr", "coverage", "popularity", "novelty".
        k: a cutoff or a strictly ascending sequence of them.  "diversity" and `diversify=` need item vectors, which this model
        does not have: `UnsupportedOnDevice`.

        `candidates`: as in `predict` -- every metric is computed on the lists ranked within the rows' candidates.
        `negatives=n` with `seed` makes those candidates itself, the sampled protocol of `WRMF.evaluate(negatives=)`: every row's
        held-out items against n negatives, exactly `candidates=self.sample_negatives(x, n, actual, not_recommend,
        items_exclude, seed, negative_weights)` -- the negatives `WRMF.sample_negatives` returns for that seed.  `seed` is
        required with `negatives`; `negatives` excludes `candidates`; `negative_weights` needs `negatives`."""
        from .metrics import HIT_METRICS, LIST_METRICS, check_cutoffs
        metrics = tuple(metrics)
        if "diversity" in metrics or diversify is not None:
            raise _lib.UnsupportedOnDevice(_lib.ERR_UNSUPPORTED, "EASE has no item vectors: no 'diversity' metric and no diversify=")
        known = ("ap", "ndcg") + HIT_METRICS + ("coverage",) + LIST_METRICS
        if not metrics or any(name not in known for name in metrics):
            raise ValueError("metrics must name some of %s" % ", ".join(repr(name) for name in known))
        scalar_k = not isinstance(k, (tuple, list, np.ndarray, range))
        cutoffs = check_cutoffs((int(k),) if scalar_k else k)
        if negatives is not None and candidates is not None:
            raise ValueError("negatives and candidates exclude each other: the negatives ARE the candidates")
        if negative_weights is not None and negatives is None:
            raise ValueError("negative_weights needs negatives: they weight the sampled negatives")
        if negatives is not None:
            if seed is None:
                raise ValueError("negatives needs a seed: EASE has no generator to draw one from")
            candidates = self.sample_negatives(x, negatives, actual=actual, not_recommend=not_recommend, items_exclude=items_exclude,
                                               seed=seed, weights=negative_weights)
        res, _ = self._lists(x, int(cutoffs[-1]), not_recommend, items_exclude, candidates=candidates)
        return evaluate_lists(self._backend(), res, actual, self._n_items, self.item_count, metrics, cutoffs, scalar_k)

    def similar_items(self, items=None, k=10):
        """the list of a user who holds only that item, the item itself excluded: `predict` on one-hot rows -> `TopItems` with the
        weights B[item, :] of the listed items in `.scores`.  items: default every item."""
        self._fitted()
        n_items = self._n_items
        q = np.arange(n_items) if items is None else np.atleast_1d(np.asarray(items, dtype=np.int64))
        if q.size and (q.min() < 0 or q.max() >= n_items):
            raise ValueError("some of items are not items of the model")
        one_hot = sp.csr_matrix((np.ones(q.size), q, np.arange(q.size + 1)), shape=(q.size, n_items))
        return self.predict(one_hot, k)
