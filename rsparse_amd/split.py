"""`train_test_split`: the train / test split of an interaction matrix (the reference's `train_test_split`, R/utils.R:1-28, plus
the leave-n-out protocols of sampled-metric evaluation), drawn on the device by wrmf_split.hip.  The split is a counter-based
function of (seed, row, position in the row) -- rsparse_amd/rng.py `split_flags` is its definition in numpy, the C header states
it for other hosts -- so it does not depend on the batches the rows are processed in, the number of ranks or the device."""
import math

import numpy as np
import scipy.sparse as sp
import torch

from . import rng as _rng

SPLIT_BATCH = 1 << 27   # stored entries per device call (whole rows; a longer row is a batch of its own)


def canonical_csr(x):
    """x as CSR with sorted, unique columns per row (duplicates summed); stored zeros stay entries.  x itself is not changed."""
    if not sp.issparse(x):
        raise TypeError("train_test_split: x must be a scipy sparse matrix")
    m = sp.csr_matrix(x)
    if not m.has_canonical_format:
        m = m.copy()          # (sp.csr_matrix of a CSR shares its arrays, and sum_duplicates works in place)
        m.sum_duplicates()
    return m


def split_arguments(x, test_proportion, leave_out, by, min_train):
    """-> (canonical x, by values or None, keyword arguments of the specification: test_threshold or leave_out / min_train)"""
    m = canonical_csr(x)
    if m.indptr[-1] >= 2 ** 31 or m.shape[0] > 2 ** 32:
        raise ValueError("train_test_split: the matrix needs int32 row pointers and at most 2^32 rows")
    if leave_out is None:
        if by is not None:
            raise ValueError("train_test_split: `by` orders a leave-out split; it has no meaning with test_proportion")
        p = float(test_proportion)
        if not 0.0 <= p <= 1.0:
            raise ValueError("train_test_split: test_proportion must lie in [0, 1]")
        return m, None, {"test_threshold": int(math.floor(p * 2.0 ** 32))}
    if test_proportion != 0.5:
        raise ValueError("train_test_split: give test_proportion or leave_out, not both")
    if isinstance(leave_out, bool) or int(leave_out) != leave_out or isinstance(min_train, bool) or int(min_train) != min_train:
        raise TypeError("train_test_split: leave_out and min_train must be integers")
    if leave_out < 1 or min_train < 0 or leave_out >= 2 ** 31 or min_train >= 2 ** 31:
        raise ValueError("train_test_split: leave_out >= 1 and min_train >= 0")
    by_v = None
    if by is not None:
        if not sp.issparse(by):
            raise ValueError("train_test_split: `by` must be a sparse matrix with the pattern of x")
        b = canonical_csr(by)
        if b.shape != m.shape or not np.array_equal(b.indptr, m.indptr) or not np.array_equal(b.indices, m.indices):
            raise ValueError("train_test_split: `by` must have exactly the pattern of x")
        by_v = np.ascontiguousarray(b.data, dtype=np.float64)
        if np.isnan(by_v).any():
            raise ValueError("train_test_split: NaN in `by`")
    return m, by_v, {"leave_out": int(leave_out), "min_train": int(min_train)}


def opaque_values(m):
    """(the values of m as 4- or 8-byte integers that are copied without being interpreted, gather): an element type of
    another size travels as its position instead (gather=True: the values are then taken from m.data at the positions)"""
    size = m.data.dtype.itemsize
    if size in (4, 8):
        return np.ascontiguousarray(m.data).view(np.int32 if size == 4 else np.int64), False
    return np.arange(m.data.size, dtype=np.int32), True


def split_batches(be, m, vals, by_v, a, b, seed, kw, batch=None):
    """the rows [a, b) of the canonical CSR m in batches of whole rows, each split with row0 = its first global row (so the
    batching cannot change a row): yields (train_p, train_j, train_v, test_p, test_j, test_v) as numpy arrays, row pointers
    from 0.  On the device when the backend has `split_rows`; else (the CPU stand-in of the tests) the numpy specification."""
    batch = int(batch or SPLIT_BATCH)
    ip = m.indptr.astype(np.int64)
    on_dev = hasattr(be, "split_rows")
    a0 = a
    while a0 < b:
        b0 = int(np.searchsorted(ip, ip[a0] + batch, side="right")) - 1
        b0 = min(b, max(b0, a0 + 1))
        e0, e1 = int(ip[a0]), int(ip[b0])
        if on_dev:
            tv = torch.int32 if vals.dtype == np.int32 else torch.int64
            out = be.split_rows(seed, a0, be.to_device(ip[a0:b0 + 1] - e0, torch.int32), be.to_device(m.indices[e0:e1], torch.int32),
                                be.to_device(vals[e0:e1], tv), by=None if by_v is None else be.to_device(by_v[e0:e1], torch.float64), **kw)
            yield tuple(t.cpu().numpy() for t in out)
        else:
            tr_p, tr_j, tr_pos, te_p, te_j, te_pos = _rng.split_rows(seed, a0, ip[a0:b0 + 1], m.indices, by=by_v, **kw)
            yield tr_p, tr_j, vals[tr_pos], te_p, te_j, vals[te_pos]
        a0 = b0


def assemble(m, gather, parts):
    """(train, test) scipy CSR of m's shape and dtype from the batches' arrays (parts: a list of split_batches' tuples that
    covers every row in order)"""
    out = []
    for o in (0, 3):
        lens = np.concatenate([np.zeros(0, np.int64)] + [np.diff(part[o].astype(np.int64)) for part in parts])
        idx = np.concatenate([np.zeros(0, np.int32)] + [part[o + 1] for part in parts])
        v = np.concatenate([np.zeros(0, parts[0][o + 2].dtype if parts else np.int32)] + [part[o + 2] for part in parts])
        data = m.data[v] if gather else v.view(m.data.dtype)
        indptr = np.concatenate([[0], np.cumsum(lens)])
        r = sp.csr_matrix((data, idx.astype(m.indices.dtype), indptr.astype(m.indptr.dtype)), shape=m.shape)
        r.has_canonical_format = True   # (a subset of a canonical matrix's entries, in their order)
        out.append(r)
    return tuple(out)


def train_test_split(x, test_proportion=0.5, leave_out=None, by=None, min_train=1, seed=None, device=None, backend=None):
    """Split the stored entries of the sparse matrix x (users as rows) into (train, test): two scipy CSR matrices of x's shape
    and dtype, canonical, with train + test == x -- pattern and values bit for bit (stored zeros count as entries).

      test_proportion=p   the reference's rule: every entry is test independently with probability p
      leave_out=n         exactly min(n, max(L - min_train, 0)) entries of a row of L entries are test, chosen uniformly at random;
                          with by= (a sparse matrix with exactly x's pattern, e.g. timestamps) the entries with the LARGEST `by`
                          values instead (temporal leave-last-out; ties go to the lower column)

    `seed` (None: 63 bits from numpy.random.default_rng()) fixes the split: it is a counter-based function of (seed, row,
    position in the row), the same for every model, batch size, rank count and device (rsparse_amd/rng.py split_flags is the
    definition).  Drawn and compacted on the device (wrmf_split.hip) in batches of whole rows; `backend`: an object with the
    HipBackend interface (default: HipBackend(device))."""
    m, by_v, kw = split_arguments(x, test_proportion, leave_out, by, min_train)
    seed = int(np.random.default_rng().integers(2 ** 63)) if seed is None else int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must fit 64 unsigned bits")
    if backend is None:
        from .engine import HipBackend
        backend = HipBackend(device)
    vals, gather = opaque_values(m)
    return assemble(m, gather, list(split_batches(backend, m, vals, by_v, 0, m.shape[0], seed, kw)))
