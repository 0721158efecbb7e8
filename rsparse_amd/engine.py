"""Device-resident ALS driver: one process per GPU, factors replicated, rows sharded.

This is the part of the reference's R driver that sits between `WRMF$fit_transform()` and the
`.Call` boundary -- `private$solver` and the two R wrappers (R/model_WRMF.R:111-147, 456-515) --
re-cut for data that lives in HBM for the whole fit:

  per half-iteration (solve side S given fixed side F):
    1. Gramian   G = F F^T + fl(lambda) I                (R/model_WRMF.R:474-486)
       each rank reduces only the block of F it owns (MFMA kernel), then ONE all-reduce of the
       k x k partial (+ the scalar sum(F^2) the loss needs);
    2. solve     every rank solves its own rows of S against the full replica of F
                 (als_implicit / als_explicit kernels, inst/include/wrmf_implicit.hpp:160-283);
    3. exchange  in-place all-gather of the solved blocks so every replica of S is current;
    4. loss      all-reduce of one double                (wrmf_implicit.hpp:286-304).

With world_size == 1 steps 1/3/4 degenerate to local calls and no collective is issued.

torch is used for device memory, streams and torch.distributed (RCCL) only; all numerics go through
the C ABI (`HipBackend`).  The backend is an explicit object so that the multi-rank control flow
can be exercised on CPU with gloo in tests (which plug in the CPU oracle); the product default is
the HIP backend and it raises if the extension or a GPU is missing -- there is no CPU fallback.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib

SOLVER_CODES = {"cholesky": 0, "conjugate_gradient": 1, "nnls": 2}   # R/model_WRMF.R:99-100


def balanced_bounds(counts, world_size):
    """Contiguous row blocks balanced by NON-ZEROS (the reference's analogue is `schedule(dynamic)`,
    inst/include/wrmf_implicit.hpp:173): `counts` = non-zeros per row (tensor or sequence); rank r owns rows
    [b[r], b[r+1]) where the prefix sum of counts first reaches r/world_size of the total."""
    c = torch.as_tensor(counts).to(torch.int64).flatten()
    n = int(c.numel())
    if world_size <= 1 or n == 0:
        return [(0, n)] + [(n, n)] * (world_size - 1)
    pre = torch.cumsum(c, 0)
    total = int(pre[-1])
    targets = torch.tensor([total * r // world_size for r in range(1, world_size)], dtype=torch.int64, device=pre.device)
    cuts = torch.searchsorted(pre, targets, right=False).tolist() if total > 0 else [n * r // world_size for r in range(1, world_size)]
    edges = [0] + [min(n, int(v) + 1) if total > 0 else int(v) for v in cuts] + [n]
    for r in range(1, len(edges)):   # monotone
        edges[r] = max(edges[r], edges[r - 1])
    return [(edges[r], edges[r + 1]) for r in range(world_size)]


def equal_bounds(n, world_size):
    B = max(1, math.ceil(n / world_size)) if n > 0 else 1
    return [(min(n, r * B), min(n, (r + 1) * B)) for r in range(world_size)]


def explain_segments(x_p, t_p):
    """the ragged layout of `explain_pairs`: target q of user u owns len(row u) contributions -> int64 indptr of n targets + 1
    (on the device of the inputs; x_p, t_p: the CSR row pointers of the rows and of the targets over the same users)"""
    lens = torch.diff(x_p.to(torch.int64))
    seg = torch.repeat_interleave(lens, torch.diff(t_p.to(torch.int64)))
    indptr = torch.zeros(int(seg.numel()) + 1, dtype=torch.int64, device=x_p.device)
    torch.cumsum(seg, dim=0, out=indptr[1:])
    return indptr


def explain_top_n(contrib, indptr, items, n):
    """the n largest contributions of every segment of the ragged output, descending, equal values in storage order (the lower
    item index of a canonical row) -> (top_items int32, top_contrib in contrib's type), both n_pairs x n, padded with -1 / 0.
    Two stable torch sorts where the data is: by value, then by segment."""
    n_pairs = int(indptr.numel()) - 1
    dev = contrib.device
    top_items = torch.full((n_pairs, n), -1, dtype=torch.int32, device=dev)
    top_contrib = torch.zeros((n_pairs, n), dtype=contrib.dtype, device=dev)
    if n_pairs == 0 or contrib.numel() == 0:
        return top_items, top_contrib
    seg = torch.repeat_interleave(torch.arange(n_pairs, device=dev), torch.diff(indptr))
    by_value = torch.argsort(contrib, descending=True, stable=True)
    perm = by_value[torch.argsort(seg[by_value], stable=True)]      # segments ascending, values descending inside
    pos = torch.arange(int(contrib.numel()), device=dev) - indptr[seg]   # (seg itself is sorted: seg[perm] == seg)
    keep = pos < n
    top_items[seg[keep], pos[keep]] = items[perm[keep]].to(torch.int32)
    top_contrib[seg[keep], pos[keep]] = contrib[perm[keep]]
    return top_items, top_contrib


def default_subblocks(world_size):
    """Sub-blocks per rank and half-iteration: with several ranks the all-gather of a solved block (640 MB per rank on
    the user side of config 3) costs about as much as the solve, so it is pipelined sub-block by sub-block.  A caller
    that wants another granularity passes `n_sub` to ShardedALS.layouts / WRMF(n_sub=...); nothing reads the environment."""
    return 1 if world_size <= 1 else 4


def _staged(t, group):
    """gloo moves host memory only: a device tensor goes through the host (the dry-run configuration of several ranks on one
    GPU, and nothing else -- RCCL takes device tensors as they are)"""
    return t.is_cuda and torch.distributed.get_backend(group) == "gloo"


def all_to_all_v(inp, in_splits, out_splits, group):
    """all_to_all_single with per-rank sizes: `inp` = the pieces for rank 0, 1, ... back to back (in_splits elements each);
    returns what the ranks sent here, in rank order (out_splits elements each)."""
    out = torch.empty(int(sum(out_splits)), dtype=inp.dtype, device=inp.device)
    if _staged(inp, group):
        host = torch.empty(out.shape, dtype=inp.dtype)
        torch.distributed.all_to_all_single(host, inp.cpu(), list(out_splits), list(in_splits), group=group)
        out.copy_(host)
    else:
        torch.distributed.all_to_all_single(out, inp.contiguous(), list(out_splits), list(in_splits), group=group)
    return out


def all_reduce_any(t, group, op=None):
    """all_reduce of a small tensor wherever it lives (staged through the host under gloo)"""
    op = torch.distributed.ReduceOp.SUM if op is None else op
    if _staged(t, group):
        host = t.cpu()
        torch.distributed.all_reduce(host, op=op, group=group)
        t.copy_(host)
    else:
        torch.distributed.all_reduce(t, op=op, group=group)
    return t


def item_block_from_user_blocks(be, group, ws, me, n_user, user_bounds, item_bounds, p, i, x):
    """The second orientation of a sharded fit without any rank holding the whole matrix (R/model_WRMF.R:190 is
    `c_iu = t(as.csr(c_ui))` on ONE host; here the matrix exists only as row blocks).

    p / i / x : this rank's USER block as a CSC by user on the device (p int32 from 0, i = global item ids ascending inside a
    user, x the resident values).  Every rank cuts its block by the item ranges of all ranks (per user a run of consecutive
    entries, the ids being sorted) and sends range s to rank s: per-user counts, item ids relative to the range, values --
    three all-to-alls of exactly the matrix's bytes.  What arrives, in rank order, IS the CSC by user of the (my items) x
    (all users) sub-matrix, users ascending because the blocks are contiguous in rank order; one on-device transposition
    (wrmf_ingest.hip) turns it into the CSC by item that the item half solves.  Returns (p, i, x) of that block:
    columns = my items, row indices = GLOBAL user ids ascending."""
    dev = i.device
    n_my = int(p.numel()) - 1
    assert n_my == user_bounds[me][1] - user_bounds[me][0]
    i64, p64 = i.to(torch.int64), p.to(torch.int64)
    cnts, idxs, vals = [], [], []
    pre = torch.zeros(int(i.numel()) + 1, dtype=torch.int64, device=dev)
    for s in range(ws):
        lo, hi = item_bounds[s]
        mask = (i64 >= lo) & (i64 < hi)
        torch.cumsum(mask, 0, out=pre[1:])
        cnts.append((pre[p64[1:]] - pre[p64[:-1]]).to(torch.int32))
        idxs.append((i64[mask] - lo).to(torch.int32))
        vals.append(x[mask])
    send_nnz = torch.tensor([int(t.numel()) for t in idxs], dtype=torch.int64, device=dev)
    recv_nnz = all_to_all_v(send_nnz, [1] * ws, [1] * ws, group).tolist()
    n_users_of = [b - a for a, b in user_bounds]
    cnt_all = all_to_all_v(torch.cat(cnts), [n_my] * ws, n_users_of, group)          # (n_user,) entries per user, global order
    idx_all = all_to_all_v(torch.cat(idxs), send_nnz.tolist(), recv_nnz, group)
    val_all = all_to_all_v(torch.cat(vals), send_nnz.tolist(), recv_nnz, group)
    total = int(sum(recv_nnz))
    if total >= 2 ** 31:
        raise ValueError("a rank's item block holds %d non-zeros: more than int32 column pointers address" % total)
    p_all = torch.zeros(n_user + 1, dtype=torch.int32, device=dev)
    p_all[1:] = torch.cumsum(cnt_all.to(torch.int64), 0).to(torch.int32)
    n_item_mine = item_bounds[me][1] - item_bounds[me][0]
    if n_item_mine == 0 or total == 0:   # a rank without items (fewer items with entries than ranks), or without entries
        return torch.zeros(n_item_mine + 1, dtype=torch.int32, device=dev), idx_all[:0], val_all[:0]
    return be.transpose_csc(n_item_mine, n_user, p_all, idx_all, val_all)


class Layout:
    """Who owns which rows of one factor matrix, and where they are stored.

    Ownership: rank r owns the contiguous global rows bounds[r] = [g0, g1) (nnz-balanced, so the blocks differ in
    size).  Storage: every block is cut into n_sub sub-blocks of Bs rows (Bs = the largest block's share, smaller
    blocks are padded with zero rows that nothing references), stored SUB-BLOCK-MAJOR:

        storage row of (rank r, sub-block j, local row l) = j * (ws * Bs) + r * Bs + l

    so sub-block j of all ranks is one contiguous slab and its exchange is a single in-place all_gather_into_tensor
    with every rank's input being its own slice of the output -- no staging copy, no variable-size collective.  The
    CSC indices that address the matrix are translated to storage rows once (to_storage).  With one rank the layout is
    the identity."""

    def __init__(self, n, bounds, n_sub=1):
        self.n, self.ws, self.n_sub = int(n), len(bounds), int(n_sub)
        self.bounds = [(int(a), int(b)) for a, b in bounds]
        assert self.bounds[0][0] == 0 and self.bounds[-1][1] == self.n
        biggest = max(1, max(b - a for a, b in self.bounds))
        self.Bs = -(-biggest // self.n_sub)
        self.rows = self.ws * self.n_sub * self.Bs
        self.identity = self.ws == 1 and self.n_sub == 1

    def sub_rows(self, r, j):
        """(first local row, one past the last) of sub-block j of rank r's block"""
        n_r = self.bounds[r][1] - self.bounds[r][0]
        return min(n_r, j * self.Bs), min(n_r, (j + 1) * self.Bs)

    def sub_start(self, r, j):
        return j * self.ws * self.Bs + r * self.Bs

    def slab(self, j):
        return j * self.ws * self.Bs, (j + 1) * self.ws * self.Bs

    def to_storage(self, ids):
        """global row ids (integer tensor) -> storage rows"""
        if self.identity:
            return ids
        starts = torch.tensor([a for a, _ in self.bounds], dtype=torch.int64, device=ids.device)
        g = ids.to(torch.int64)
        r = torch.searchsorted(starts, g, right=True) - 1
        # empty blocks share their start with the next one: searchsorted(right=True) - 1 lands on the LAST block with
        # that start, which is the non-empty one
        loc = g - starts[r]
        j = loc // self.Bs
        return (j * (self.ws * self.Bs) + r * self.Bs + (loc - j * self.Bs)).to(ids.dtype)

    def alloc(self, k, device, dtype=torch.float32):
        return torch.zeros((self.rows, k), dtype=dtype, device=device)

    def from_global(self, S, G):
        """write a global-order (n, k) matrix into storage S"""
        if self.identity:
            S[:self.n] = G
        else:
            S[self.to_storage(torch.arange(self.n, device=S.device))] = G.to(S.device)
        return S

    def to_global(self, S):
        if self.identity:
            return S[:self.n]
        return S[self.to_storage(torch.arange(self.n, device=S.device))]


class HipBackend:
    """Numerics on the current HIP device through librsparse_wrmf_hip.so."""

    name = "hip"
    # which build's cut-off applies to a small implicit global bias on the fp32 layer (wrmf_implicit.hpp:108-109): False =
    # als_implicit<float>'s 3.45e-4, True = als_implicit<double>'s 1.49e-8 (WRMF sets it from its `precision`)
    double_threshold = False
    top_product_batch = 1 << 18   # rows per `$predict` call of the library (bounds the re-scoring scratch)

    def __init__(self, device=None):
        self.lib = _lib.load()
        if torch.cuda.device_count() < 1 or self.lib.rsparse_hip_device_count() < 1:
            raise RuntimeError("rsparse_amd: no HIP device visible (the device path has no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        torch.cuda.set_device(self.device)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def to_device(self, a, dtype):
        return torch.as_tensor(a, dtype=dtype).to(self.device).contiguous()

    def init_factors(self, seed, stream, n_rows, rank, dtype, abs_values=False, ones_col=-1, row0=0, scale=0.01, out=None):
        """the rows [row0, row0 + n_rows) of the initial factor matrix of `stream` (0 = users, 1 = items) under `seed`, drawn on
        the device by the counter-based generator of wrmf_init.hip (rsparse_amd/rng.py is its definition): scale * N(0, 1),
        |.| with abs_values, the column ones_col (-1: none) exactly 1.  -> an (n_rows, rank) device tensor of `dtype` (float32
        or float64); `out`: write into this tensor instead (rows of `rank` elements, any row stride >= rank: what lies between
        the rows is left alone).  No host array and no upload are involved; a value does not depend on row0 / n_rows."""
        assert dtype in (torch.float32, torch.float64)
        n_rows, rank = int(n_rows), int(rank)
        if out is None:
            out = torch.empty((n_rows, rank), dtype=dtype, device=self.device)
        assert out.dtype == dtype and out.is_cuda and tuple(out.shape) == (n_rows, rank) and (rank == 1 or out.stride(1) == 1)
        ld = int(out.stride(0)) if n_rows > 1 else rank
        fn = self.lib.rsparse_hip_init_factors_f64_device if dtype == torch.float64 else self.lib.rsparse_hip_init_factors_device
        _lib.check(fn(int(seed), int(stream), int(row0), n_rows, rank, ld, float(scale), int(bool(abs_values)), int(ones_col),
                      out.data_ptr() if n_rows else None, self._stream()))
        return out

    def make_csc(self, n_rows, n_cols, p, i, x):
        """p/i/x: torch tensors already on the device (int32, int32, float32 -- or float64: the handle then belongs to the
        fp64 layer of the C ABI and every call that takes it computes in double)."""
        assert p.dtype == torch.int32 and i.dtype == torch.int32 and x.dtype in (torch.float32, torch.float64)
        h = ctypes.c_void_p()
        if x.dtype == torch.float64:
            _lib.check(self.lib.rsparse_hip_csc_f64_create_device(int(n_rows), int(n_cols), p.data_ptr(), i.data_ptr(),
                                                                  x.data_ptr(), ctypes.byref(h)))
            return _CscHandle(self.lib, h, (p, i, x), n_rows, n_cols, f64=True)
        _lib.check(self.lib.rsparse_hip_csc_create_device(int(n_rows), int(n_cols), p.data_ptr(), i.data_ptr(),
                                                          x.data_ptr(), ctypes.byref(h)))
        return _CscHandle(self.lib, h, (p, i, x), n_rows, n_cols)

    def transpose_csc(self, n_rows, n_cols, p, i, x):
        """CSC (p, i, x) of an n_rows x n_cols matrix, on the device -> CSC of its transpose, row indices ascending
        inside every column (the second orientation of a fit, R/model_WRMF.R:190)."""
        assert p.dtype == torch.int32 and i.dtype == torch.int32 and x.dtype in (torch.float32, torch.float64)
        nnz = int(i.numel())
        if x.dtype == torch.float64:
            # the ingest kernels move 32-bit payloads: send each entry's POSITION through them (bits are copied, never
            # computed with) and gather the doubles by the permutation that comes back
            # (positions >= 0x7f800000 would be NaN bit patterns; a copy keeps those too, but no int32-indexed matrix gets there:
            # asserted rather than assumed, tests/test_ingest.py::test_transpose_moves_payload_bits_untouched goes past 2^23)
            assert nnz < 0x7F800000, "transpose_csc: more positions than the 32-bit payload can carry"
            pos = torch.arange(nnz, dtype=torch.int32, device=self.device).view(torch.float32)
            pt, it, perm = self.transpose_csc(n_rows, n_cols, p, i, pos)
            return pt, it, x[perm.view(torch.int32).to(torch.int64)].contiguous()
        pt = torch.empty(n_rows + 1, dtype=torch.int32, device=self.device)
        it = torch.empty(max(nnz, 1), dtype=torch.int32, device=self.device)[:nnz]
        xt = torch.empty(max(nnz, 1), dtype=torch.float32, device=self.device)[:nnz]
        _lib.check(self.lib.rsparse_hip_csc_transpose_device(int(n_rows), int(n_cols), p.data_ptr(), i.data_ptr(),
                                                             x.data_ptr(), pt.data_ptr(), it.data_ptr(), xt.data_ptr(),
                                                             self._stream()))
        return pt, it, xt

    def values_to_float(self, x64):
        """f64 values as they arrive from a dgCMatrix -> f32 resident values (wrmf_implicit.hpp:182-183)."""
        assert x64.dtype == torch.float64 and x64.is_cuda
        out = torch.empty(x64.shape, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.rsparse_hip_values_to_float_device(int(x64.numel()), x64.data_ptr(), out.data_ptr(),
                                                               self._stream()))
        return out

    def gramian(self, F, lambda_, out, sumsq_out, absmax_inout=None):
        """absmax_inout (float32[1], optional): receives max(its content, max |F|) -- the Gramian reads F anyway."""
        n, k = F.shape
        if F.dtype == torch.float64:
            assert out.dtype == torch.float64
            _lib.check(self.lib.rsparse_hip_gramian_f64_device(
                F.data_ptr(), k, n, float(lambda_), out.data_ptr(), None if sumsq_out is None else sumsq_out.data_ptr(),
                self._stream()))
            return
        _lib.check(self.lib.rsparse_hip_gramian_absmax_device(
            F.data_ptr(), k, n, float(lambda_), out.data_ptr(), None if sumsq_out is None else sumsq_out.data_ptr(),
            None if absmax_inout is None else absmax_inout.data_ptr(), self._stream()))

    def half_iteration(self, csc, implicit, F, S_block, G, lambda_, solver, cg_steps, dynamic_lambda, loss_out,
                       bias_last_row=None, global_bias=0.0, absmax=None):
        """bias_last_row: None = no user/item biases; True/False = als_explicit's is_x_bias_last_row with
        with_biases = TRUE.  absmax (float32[1] on the device, optional): max |F| if the caller knows it (implicit
        feedback; the Gramian pass yields it) -- F is then not scanned for the fp16 operand scales."""
        k = F.shape[1]
        if csc.f64:   # the fp64 layer: one entry point for every variant
            assert F.dtype == torch.float64 and S_block.dtype == torch.float64 and (G is None or G.dtype == torch.float64)
            _lib.check(self.lib.rsparse_hip_als_f64_device(
                csc.h, int(bool(implicit)), F.data_ptr(), S_block.data_ptr(), None if G is None else G.data_ptr(), k,
                float(lambda_), int(solver), int(cg_steps), int(bool(dynamic_lambda)), int(bias_last_row is not None),
                int(bool(bias_last_row)), float(global_bias) if implicit else 0.0, loss_out.data_ptr(), self._stream()))
            return
        am = None if absmax is None else absmax.data_ptr()
        if implicit and global_bias:
            # implicit feedback with a global bias: every solver without user/item biases, Cholesky / NNLS with them
            _lib.check(self.lib.rsparse_hip_als_implicit_global_bias_device(
                csc.h, F.data_ptr(), S_block.data_ptr(), G.data_ptr(), k, float(lambda_), int(solver), int(cg_steps),
                int(bias_last_row is not None), int(bool(bias_last_row)), float(global_bias), int(self.double_threshold), am,
                loss_out.data_ptr(), self._stream()))
        elif bias_last_row is not None and implicit:
            # G: (k-1) x (k-1) Gramian of F without its bias row, ridge included (R/model_WRMF.R:463-486)
            _lib.check(self.lib.rsparse_hip_als_implicit_bias_device(csc.h, F.data_ptr(), S_block.data_ptr(), G.data_ptr(),
                                                                     k, float(lambda_), int(solver),
                                                                     int(bool(bias_last_row)), loss_out.data_ptr(),
                                                                     self._stream()))
        elif bias_last_row is not None:
            _lib.check(self.lib.rsparse_hip_als_explicit_bias_device(csc.h, F.data_ptr(), S_block.data_ptr(), k,
                                                                     float(lambda_), int(solver), int(cg_steps),
                                                                     int(bool(dynamic_lambda)), int(bool(bias_last_row)),
                                                                     loss_out.data_ptr(), self._stream()))
        elif implicit:
            _lib.check(self.lib.rsparse_hip_als_implicit_device(csc.h, F.data_ptr(), S_block.data_ptr(), G.data_ptr(),
                                                                k, float(lambda_), int(solver), int(cg_steps), am,
                                                                loss_out.data_ptr(), self._stream()))
        else:
            _lib.check(self.lib.rsparse_hip_als_explicit_device(csc.h, F.data_ptr(), S_block.data_ptr(), k,
                                                                float(lambda_), int(solver), int(cg_steps),
                                                                int(bool(dynamic_lambda)), loss_out.data_ptr(),
                                                                self._stream()))

    def top_product(self, U, V, k, nr_p, nr_j, exclude0, glob_mean):
        """top_product (src/matrix_top_product.cpp:20-102) for the rows of U (n x rank) against V (n_item x rank), both on the
        device: (indices int32 n x k, 1-based with NA_integer_; scores float64 n x k).  nr_p / nr_j: the rows' not_recommend
        entries as CSR slots (or None), exclude0: sorted 0-based item ids excluded for every row (or None)."""
        n, rank = U.shape
        n_item = V.shape[0]
        U32 = U.to(torch.float32).contiguous()
        V32 = self._v32(V)
        # the fp32 matrix-core pass nominates k + max(8, k / 4) candidates per row; their scores are recomputed in double
        # (from the double factors when the model holds them: find_top_product multiplies in double, R/utils.R:35-36) and
        # the reference's heap is replayed over them
        f64 = U.dtype == torch.float64 and V.dtype == torch.float64
        U64 = U.contiguous() if f64 else None
        V64 = V.contiguous() if f64 else None
        res = torch.empty((n, k), dtype=torch.int32, device=U.device)
        sc = torch.empty((n, k), dtype=torch.float64, device=U.device)
        # in batches of rows: the re-scoring pass takes n * (2 kc + 2 k + 1) words from a grow-only workspace (several GB for a
        # few million users in one call); a batch bounds it and the next batch reuses it.  The CSR slots of
        # not_recommend are absolute positions into nr_j, so a batch passes its slice of nr_p unchanged.
        B = self.top_product_batch
        if k > 256:
            # the large-k path (k <= 8192): the same budget of n * (2 kc + 2 k + 1) words as a full batch at k = 256
            kc = k + max(8, k // 4)
            B = max(1, min(B, B * (2 * 320 + 2 * 256 + 1) // (2 * kc + 2 * k + 1)))
        for a0 in range(0, max(n, 1), B):
            nb = min(B, n - a0)
            if nb <= 0:
                break
            _lib.check(self.lib.rsparse_hip_top_product_f64_device(
                U32[a0:].data_ptr(), V32.data_ptr(), None if U64 is None else U64[a0:].data_ptr(),
                None if V64 is None else V64.data_ptr(), nb, n_item, rank, k, -1,
                None if nr_p is None else nr_p[a0:].data_ptr(), None if nr_j is None else nr_j.data_ptr(),
                None if exclude0 is None else exclude0.data_ptr(), 0 if exclude0 is None else int(exclude0.numel()),
                float(glob_mean), res[a0:].data_ptr(), sc[a0:].data_ptr(), self._stream()))
        return res, sc

    top_candidates_batch = 1 << 28   # candidates per call: 8 bytes each in the library's grow-only workspace (2 GiB)

    def top_candidates(self, U, V, k, c_p, c_j, nr_p, nr_j, exclude0, glob_mean):
        """top_product WITHIN per-row candidate lists (wrmf_candidates.hip): for the rows of U (n x rank) the k best of the
        stored positions of the CSR pattern (c_p, c_j: int32 on the device, columns ascending and unique within a row) that are
        neither in the row's not_recommend slots (nr_p / nr_j, columns ascending, or None) nor in exclude0 (sorted 0-based ids,
        or None), by the scores of `score_pairs` (the factors as they are, fp32 or fp64, summed in double, + glob_mean) with the
        reference's tie rule.  -> (indices int32 n x k, 1-based with NA_integer_; scores float64 n x k, NaN where NA)."""
        if U.dtype != V.dtype:
            U = U.to(V.dtype)
        assert V.dtype in (torch.float32, torch.float64) and U.shape[1] == V.shape[1]
        assert c_p.dtype == torch.int32 and c_j.dtype == torch.int32 and int(c_p.numel()) == U.shape[0] + 1
        U, V = U.contiguous(), V.contiguous()
        n, rank = U.shape
        dev = U.device
        res = torch.empty((n, k), dtype=torch.int32, device=dev)
        sc = torch.empty((n, k), dtype=torch.float64, device=dev)
        if n == 0:
            return res, sc
        nnz = int(c_j.numel())
        if nnz == 0:   # no candidate at all: every list is empty, nothing to launch
            res.fill_(-2147483648)
            sc.fill_(float("nan"))
            return res, sc
        fn = self.lib.rsparse_hip_top_candidates_f64_device if V.dtype == torch.float64 else self.lib.rsparse_hip_top_candidates_device
        # in batches of rows when the pattern is larger than the workspace budget: the slots are absolute positions into c_j
        # (and nr_j), so a batch passes its slice of the row pointers unchanged
        bounds = [0, n]
        if nnz > self.top_candidates_batch:
            hp = c_p.cpu().numpy().astype(np.int64)
            bounds, a0 = [0], 0
            while a0 < n:
                b0 = int(np.searchsorted(hp, hp[a0] + self.top_candidates_batch, side="right")) - 1
                a0 = min(n, max(b0, a0 + 1))
                bounds.append(a0)
        for a0, b0 in zip(bounds[:-1], bounds[1:]):
            _lib.check(fn(U[a0:].data_ptr(), V.data_ptr(), b0 - a0, int(V.shape[0]), rank, int(k), c_p[a0:].data_ptr(), c_j.data_ptr(),
                          None if nr_p is None else nr_p[a0:].data_ptr(), None if nr_j is None else nr_j.data_ptr(),
                          None if exclude0 is None else exclude0.data_ptr(), 0 if exclude0 is None else int(exclude0.numel()),
                          float(glob_mean), res[a0:].data_ptr(), sc[a0:].data_ptr(), self._stream()))
        return res, sc

    def sample_negatives(self, seed, row0, seen_p, seen_j, keep_p, keep_j, n_item, n):
        """the candidate rows of a sampled-metric evaluation, made on the device (wrmf_sample.hip; rsparse_amd/rng.py
        sample_negatives is the definition): for every row of the CSR pattern (seen_p, seen_j: int32 on the device, columns
        ascending and unique; seen_p may be a slice of a larger pattern's row pointers) its `keep` items (keep_p / keep_j, a subset
        of the seen row, or both None) merged with min(n, n_item - |seen|) items drawn without replacement from outside the seen
        row, under `seed` and the global row index row0 + u.  -> (out_p, out_j): canonical CSR from 0, int32 on the device, out_j
        sliced to its true length."""
        assert seen_p.dtype == torch.int32 and seen_j.dtype == torch.int32 and (keep_p is None) == (keep_j is None)
        n_rows, n = int(seen_p.numel()) - 1, int(n)
        dev = seen_p.device
        out_p = torch.zeros(max(n_rows, 0) + 1, dtype=torch.int32, device=dev)
        if n_rows <= 0:
            return out_p, torch.empty(0, dtype=torch.int32, device=dev)
        kept = 0
        if keep_p is not None:
            assert keep_p.dtype == torch.int32 and keep_j.dtype == torch.int32 and int(keep_p.numel()) == n_rows + 1
            kept = int(keep_p[-1]) - int(keep_p[0])
        cap = max(0, kept) + n_rows * max(min(n, int(n_item)), 0)
        out_j = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        one = torch.zeros(1, dtype=torch.int32, device=dev)   # (a pattern without entries: the library still wants non-NULL slots)
        _lib.check(self.lib.rsparse_hip_sample_negatives_device(
            int(seed), int(row0), n_rows, int(n_item), n, seen_p.data_ptr(), (seen_j if seen_j.numel() else one).data_ptr(),
            None if keep_p is None else keep_p.data_ptr(), None if keep_p is None else (keep_j if keep_j.numel() else one).data_ptr(),
            out_p.data_ptr(), out_j.data_ptr(), cap, self._stream()))
        return out_p, out_j[:int(out_p[-1])]

    def weights_prefix(self, w_dev):
        """the inclusive 64-bit prefix of the item weights of the weighted negative stream (rsparse_amd/rng.py weights_prefix):
        w_dev the uint32 weights (every one >= 1) on the device as an int32 tensor of the same bits (`w.view(np.int32)`) -> an
        int64 tensor of their running sums (the bits of the library's uint64), to pass to `sample_negatives_weighted` any number
        of times.  A zero weight is refused by the library."""
        assert w_dev.dtype == torch.int32 and w_dev.is_contiguous()
        n_item = int(w_dev.numel())
        cum = torch.empty(max(n_item, 1), dtype=torch.int64, device=w_dev.device)
        if n_item:
            _lib.check(self.lib.rsparse_hip_weights_prefix_device(w_dev.data_ptr(), n_item, cum.data_ptr(), self._stream()))
        return cum[:n_item]

    def sample_negatives_weighted(self, seed, row0, seen_p, seen_j, keep_p, keep_j, n_item, n, cum):
        """`sample_negatives` with the negatives drawn in proportion to item weights (wrmf_sample_weighted.hip; rsparse_amd/rng.py
        sample_negatives_weighted is the definition): cum = `weights_prefix` of the n_item weights.  -> (out_p, out_j,
        filled_rows): the rows as `sample_negatives` gives them, and the number of rows whose draw budget ended before n distinct
        admissible items were drawn (filled with the lowest admissible items; 0 for ordinary weights)."""
        assert seen_p.dtype == torch.int32 and seen_j.dtype == torch.int32 and (keep_p is None) == (keep_j is None)
        assert cum.dtype == torch.int64 and int(cum.numel()) == int(n_item) and cum.is_contiguous()
        n_rows, n = int(seen_p.numel()) - 1, int(n)
        dev = seen_p.device
        out_p = torch.zeros(max(n_rows, 0) + 1, dtype=torch.int32, device=dev)
        if n_rows <= 0:
            return out_p, torch.empty(0, dtype=torch.int32, device=dev), 0
        kept = 0
        if keep_p is not None:
            assert keep_p.dtype == torch.int32 and keep_j.dtype == torch.int32 and int(keep_p.numel()) == n_rows + 1
            kept = int(keep_p[-1]) - int(keep_p[0])
        cap = max(0, kept) + n_rows * max(min(n, int(n_item)), 0)
        out_j = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        one = torch.zeros(2, dtype=torch.int32, device=dev)   # (a pattern without entries: the library still wants non-NULL slots)
        filled = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(self.lib.rsparse_hip_sample_negatives_weighted_device(
            int(seed), int(row0), n_rows, int(n_item), n, seen_p.data_ptr(), (seen_j if seen_j.numel() else one).data_ptr(),
            None if keep_p is None else keep_p.data_ptr(), None if keep_p is None else (keep_j if keep_j.numel() else one).data_ptr(),
            (cum if cum.numel() else one).data_ptr(), out_p.data_ptr(), out_j.data_ptr(), cap, filled.data_ptr(), self._stream()))
        return out_p, out_j[:int(out_p[-1])], int(filled[0])

    def split_rows(self, seed, row0, p, j, v=None, test_threshold=None, leave_out=None, min_train=1, by=None):
        """the train / test split of the rows of a canonical CSR, made on the device (wrmf_split.hip; rsparse_amd/rng.py split_flags
        is the definition): p, j int32 on the device (p may be a slice of a larger pattern's row pointers), v None or a tensor of
        4- or 8-byte elements that is copied without being interpreted, `by` None or float64, one per stored entry.  Exactly one
        of test_threshold (proportion mode, floor(p 2^32)) and leave_out (with min_train, by) is given; the global row index of
        row u is row0 + u.  -> (train_p, train_j, train_v, test_p, test_j, test_v): canonical CSR from 0 on the device, j / v
        sliced to their true lengths (v None without values)."""
        assert p.dtype == torch.int32 and j.dtype == torch.int32 and (test_threshold is None) != (leave_out is None)
        assert by is None or by.dtype == torch.float64
        n_rows, dev = int(p.numel()) - 1, p.device
        train_p = torch.zeros(max(n_rows, 0) + 1, dtype=torch.int32, device=dev)
        test_p = torch.zeros(max(n_rows, 0) + 1, dtype=torch.int32, device=dev)
        vb = 0 if v is None else int(v.element_size())
        nnz = max(int(p[-1]) - int(p[0]), 0) if n_rows > 0 else 0
        cap_test = nnz if leave_out is None else min(nnz, n_rows * max(int(leave_out), 0))
        outs = []
        for cap in (nnz, cap_test):
            outs.append(torch.empty(max(cap, 1), dtype=torch.int32, device=dev))
            outs.append(None if v is None else torch.empty(max(cap, 1), dtype=v.dtype, device=dev))
        train_j, train_v, test_j, test_v = outs
        if n_rows > 0 and nnz > 0:   # (rows without a stored entry: both row-pointer arrays are the zeros they already hold)
            mode = 0 if leave_out is None else 1
            _lib.check(self.lib.rsparse_hip_split_rows_device(
                int(seed), int(row0), n_rows, mode, int(test_threshold or 0), int(leave_out or 0), int(min_train), p.data_ptr(),
                j.data_ptr(), None if v is None else v.data_ptr(), vb, None if by is None else by.data_ptr(),
                train_p.data_ptr(), train_j.data_ptr(), None if v is None else train_v.data_ptr(), test_p.data_ptr(), test_j.data_ptr(),
                None if v is None else test_v.data_ptr(), nnz, cap_test, self._stream()))
        n_tr, n_te = int(train_p[-1]), int(test_p[-1])
        return (train_p, train_j[:n_tr], None if v is None else train_v[:n_tr], test_p, test_j[:n_te], None if v is None else test_v[:n_te])

    def events_to_csr(self, users, items, values, timestamps, n_users, n_items, aggregate="sum", half_life=None, now=None):
        """the canonical CSR over the cells of an event log, made on the device (wrmf_events.hip; rsparse_amd/events.py
        events_reference is the definition): users, items int32, values / timestamps float64 or None, one per event, on the
        device.  -> (p, j, x, count, latest) on the device, sliced to the number of cells; latest None without timestamps."""
        from .events import AGGREGATES
        assert users.dtype == torch.int32 and items.dtype == torch.int32 and users.numel() == items.numel()
        assert values is None or values.dtype == torch.float64
        assert timestamps is None or timestamps.dtype == torch.float64
        n, dev = int(users.numel()), self.device
        p = torch.empty(int(n_users) + 1, dtype=torch.int32, device=dev)
        j = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        x = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        count = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        latest = None if timestamps is None else torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        n_cells = ctypes.c_int64(0)
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(self.lib.rsparse_hip_events_to_csr_device(
            n, int(n_users), int(n_items), users.data_ptr(), items.data_ptr(), ptr(values), ptr(timestamps), AGGREGATES[aggregate],
            0.0 if half_life is None else float(half_life), 0.0 if now is None else float(now), int(now is not None), p.data_ptr(),
            j.data_ptr(), x.data_ptr(), count.data_ptr(), ptr(latest), max(n, 1), ctypes.byref(n_cells), self._stream()))
        c = int(n_cells.value)
        return p, j[:c], x[:c], count[:c], None if latest is None else latest[:c]

    def confidence_moments(self, p, x, power):
        """(out, total) on the device: out[r] = sum |x|^power over segment r of the arrays (p, x) -- p int32 from 0, x float64 --
        and the sum over all entries (one double), wrmf_confidence.hip: a fixed summation order, repeat calls bit-identical"""
        assert p.dtype == torch.int32 and x.dtype == torch.float64 and p.numel() >= 1
        n_seg = int(p.numel()) - 1
        out = torch.empty(max(n_seg, 1), dtype=torch.float64, device=self.device)[:n_seg]
        total = torch.empty(1, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.rsparse_hip_confidence_moments_device(n_seg, int(x.numel()), p.data_ptr(), x.data_ptr(), int(power),
                                                                  out.data_ptr(), total.data_ptr(), self._stream()))
        return out, total

    def confidence_table(self, table, n, p=None, moment=None, total=None, a=0.0, b=0.0, c=0.0):
        """the per-row or per-column table of rsparse_amd.confidence ("idf" from the counts diff(p), "bm25" from the row sums and
        the fit's total, "norm" from the moments): n doubles on the device"""
        from .confidence import TABLES
        out = torch.empty(max(int(n), 1), dtype=torch.float64, device=self.device)[:int(n)]
        ptr = [None if t is None else t.data_ptr() for t in (p, moment, total)]
        _lib.check(self.lib.rsparse_hip_confidence_table_device(TABLES[table], int(n), ptr[0], ptr[1], ptr[2], float(a), float(b),
                                                                float(c), out.data_ptr(), self._stream()))
        return out

    def confidence_apply(self, kind, p, i, x, seg_table=None, idx_table=None, seg_is_item=False, a=0.0, b=0.0, out=None):
        """x weighted by `kind` (rsparse_amd.confidence) on the resident arrays (p, i, x) of either orientation: seg_table has one
        entry per segment of p, idx_table is gathered by i; seg_is_item: the segments are the items.  out: None = new doubles,
        "inplace" = over x, torch.float32 = new floats (the double result rounded once)."""
        from .confidence import KINDS
        assert p.dtype == torch.int32 and i.dtype == torch.int32 and x.dtype == torch.float64
        nnz = int(x.numel())
        if out is None:
            dst = torch.empty(max(nnz, 1), dtype=torch.float64, device=self.device)[:nnz]
        elif out is torch.float32:
            dst = torch.empty(max(nnz, 1), dtype=torch.float32, device=self.device)[:nnz]
        else:
            assert out == "inplace"
            dst = x
        _lib.check(self.lib.rsparse_hip_confidence_apply_device(
            KINDS[kind], int(p.numel()) - 1, nnz, p.data_ptr(), i.data_ptr(), x.data_ptr(),
            None if seg_table is None else seg_table.data_ptr(), None if idx_table is None else idx_table.data_ptr(),
            0 if idx_table is None else int(idx_table.numel()), int(bool(seg_is_item)), float(a), float(b), dst.data_ptr(),
            int(dst.dtype == torch.float32), self._stream()))
        return dst

    def ranking_metrics(self, res, p, j, x, want_ap=True, want_ndcg=True):
        """ap_k / ndcg_k (R/metrics.R:31-127) of the lists `res` (n x k int32 on the device, 1-based with NA_integer_, as
        top_product returns them) against `actual` as CSR slots on the device (p, j int32 with j sorted within rows; x float64,
        needed for ndcg only): (ap, ndcg), float64 vectors of n on the device, None for a metric not asked for."""
        n, k = res.shape
        ap = torch.empty(n, dtype=torch.float64, device=res.device) if want_ap else None
        ndcg = torch.empty(n, dtype=torch.float64, device=res.device) if want_ndcg else None
        if n == 0:
            return ap, ndcg
        if j.numel() == 0:   # (no stored entry at all: the library still wants non-NULL slots)
            j = torch.zeros(1, dtype=torch.int32, device=res.device)
            x = torch.zeros(1, dtype=torch.float64, device=res.device)
        _lib.check(self.lib.rsparse_hip_ranking_metrics_device(
            res.data_ptr(), n, k, p.data_ptr(), j.data_ptr(), x.data_ptr() if want_ndcg else None,
            None if ap is None else ap.data_ptr(), None if ndcg is None else ndcg.data_ptr(), self._stream()))
        return ap, ndcg

    def hit_metrics(self, res, p, j, cutoffs, want, first_seen=None):
        """the hit-based metrics of the lists `res` (as for ranking_metrics) at the strictly ascending `cutoffs` (host ints, at
        most 16, within 1 .. k) in one launch (wrmf_hits.hip; rsparse_amd.metrics.hit_metrics_reference is the definition):
        {name: tensor on the device} for the names in `want` -- "hits" (n x T int32), "first" (n int32), "precision", "recall",
        "hit", "mrr" (n x T float64).  first_seen: int32 of n_item on the device, min-updated in place with the first position
        at which a list names each item (the caller initialises it, INT32_MAX = never; several calls accumulate)."""
        known = ("hits", "first", "precision", "recall", "hit", "mrr")
        want = tuple(want)
        if any(m not in known for m in want) or (not want and first_seen is None):
            raise ValueError("hit_metrics: want must name some of %s (or first_seen be given)" % ", ".join(known))
        assert res.dtype == torch.int32 and p.dtype == torch.int32 and j.dtype == torch.int32
        assert first_seen is None or (first_seen.dtype == torch.int32 and first_seen.is_contiguous())
        res = res.contiguous()
        n, k = res.shape
        cut = np.ascontiguousarray(np.asarray(list(cutoffs), dtype=np.int32))
        T = int(cut.size)
        out = {}
        for m in want:
            out[m] = torch.empty(n if m == "first" else (n, T), dtype=torch.int32 if m in ("hits", "first") else torch.float64,
                                 device=res.device)
        if n == 0:
            return out
        if j.numel() == 0:   # (no stored entry at all: the library still wants a non-NULL slot)
            j = torch.zeros(1, dtype=torch.int32, device=res.device)
        ptr = lambda m: out[m].data_ptr() if m in out else None
        _lib.check(self.lib.rsparse_hip_hit_metrics_device(
            res.data_ptr(), n, k, p.data_ptr(), j.data_ptr(), cut.ctypes.data_as(ctypes.c_void_p), T, ptr("hits"), ptr("first"),
            ptr("precision"), ptr("recall"), ptr("hit"), ptr("mrr"), None if first_seen is None else first_seen.data_ptr(),
            0 if first_seen is None else int(first_seen.numel()), self._stream()))
        return out

    def list_metrics(self, res, cutoffs, n_item, want, item_count=None, item_info=None, exposure=None):
        """the beyond-accuracy integer metrics of the lists `res` (as for ranking_metrics) at `cutoffs` in one launch
        (wrmf_lists.hip; rsparse_amd.metrics.list_metrics_reference is the definition): {name: (n, T) tensor on the device} for
        the names in `want` -- "valid" (int32), "count_sum", "info_sum" (int64), "popularity", "novelty" (float64).  item_count:
        int32 of n_item on the device (count_sum / popularity), item_info: int64 of n_item (info_sum / novelty).  exposure: int32
        (T, n_item) on the device, caller-zeroed; it receives the histogram per cutoff INTERVAL (several calls accumulate) and is
        cumulated along dim 0 by the caller."""
        known = ("valid", "count_sum", "info_sum", "popularity", "novelty")
        want = tuple(want)
        if any(m not in known for m in want) or (not want and exposure is None):
            raise ValueError("list_metrics: want must name some of %s (or exposure be given)" % ", ".join(known))
        if ("count_sum" in want or "popularity" in want) and item_count is None:
            raise ValueError("list_metrics: count_sum / popularity need item_count")
        if ("info_sum" in want or "novelty" in want) and item_info is None:
            raise ValueError("list_metrics: info_sum / novelty need item_info")
        assert res.dtype == torch.int32
        res = res.contiguous()
        n, k = res.shape
        cut = np.ascontiguousarray(np.asarray(list(cutoffs), dtype=np.int32))
        T = int(cut.size)
        n_item = int(n_item)
        assert item_count is None or (item_count.dtype == torch.int32 and item_count.is_contiguous() and item_count.numel() == n_item)
        assert item_info is None or (item_info.dtype == torch.int64 and item_info.is_contiguous() and item_info.numel() == n_item)
        assert exposure is None or (exposure.dtype == torch.int32 and exposure.is_contiguous() and tuple(exposure.shape) == (T, n_item))
        dt = {"valid": torch.int32, "count_sum": torch.int64, "info_sum": torch.int64}
        out = {m: torch.empty((n, T), dtype=dt.get(m, torch.float64), device=res.device) for m in want}
        if n == 0:
            return out
        ptr = lambda m: out[m].data_ptr() if m in out else None
        _lib.check(self.lib.rsparse_hip_list_metrics_device(
            res.data_ptr(), n, k, cut.ctypes.data_as(ctypes.c_void_p), T, None if item_count is None else item_count.data_ptr(),
            None if item_info is None else item_info.data_ptr(), n_item, ptr("valid"), ptr("count_sum"), ptr("info_sum"),
            ptr("popularity"), ptr("novelty"), None if exposure is None else exposure.data_ptr(), self._stream()))
        return out

    def item_inv_norms(self, V, c0, c1):
        """1 / the Euclidean norm of every row of V over its columns [c0, c1): float64 of n_item on the device, 0.0 for a
        degenerate item (zero or non-finite norm).  One streaming launch (wrmf_diversity.hip); kept until the matrix changes,
        keyed and dropped exactly like the cosine operands `normalized_items`."""
        key = (V._version, int(c0), int(c1))
        if getattr(self, "_inv_src", None) is not V or self._inv_key != key:
            assert V.is_contiguous() and V.dim() == 2 and V.dtype in (torch.float32, torch.float64)
            n, ld = V.shape
            inv = torch.empty(n, dtype=torch.float64, device=V.device)
            fn = (self.lib.rsparse_hip_item_inv_norms_f64_device if V.dtype == torch.float64
                  else self.lib.rsparse_hip_item_inv_norms_device)
            _lib.check(fn(V.data_ptr(), n, ld, int(c0), int(c1), inv.data_ptr(), self._stream()))
            self._inv_cache, self._inv_src, self._inv_key = inv, V, key
        return self._inv_cache

    def list_diversity(self, res, cutoffs, V, c0, c1, want=("counted", "diversity")):
        """the intra-list cosine distance of the lists `res` (as for ranking_metrics) over the columns [c0, c1) of V (n_item x
        ld, fp32 or fp64, on the device), at `cutoffs` in one launch (wrmf_diversity.hip; the definition is
        rsparse_amd.metrics.list_diversity_reference): {"counted": (n, T) int32, "diversity": (n, T) float64} on the device."""
        want = tuple(want)
        if not want or any(m not in ("counted", "diversity") for m in want):
            raise ValueError("list_diversity: want must name 'counted' and / or 'diversity'")
        assert res.dtype == torch.int32
        inv = self.item_inv_norms(V, c0, c1)
        res = res.contiguous()
        n, k = res.shape
        cut = np.ascontiguousarray(np.asarray(list(cutoffs), dtype=np.int32))
        T = int(cut.size)
        out = {m: torch.empty((n, T), dtype=torch.int32 if m == "counted" else torch.float64, device=res.device) for m in want}
        if n == 0:
            return out
        fn = self.lib.rsparse_hip_list_diversity_f64_device if V.dtype == torch.float64 else self.lib.rsparse_hip_list_diversity_device
        ptr = lambda m: out[m].data_ptr() if m in out else None
        _lib.check(fn(res.data_ptr(), n, k, cut.ctypes.data_as(ctypes.c_void_p), T, V.data_ptr(), int(V.shape[0]), int(V.shape[1]),
                      int(c0), int(c1), inv.data_ptr(), ptr("counted"), ptr("diversity"), self._stream()))
        return out

    def mmr_rerank(self, res, sc, V, c0, c1, k, trade_off, want=("scores", "positions", "objective")):
        """the greedy MMR re-ranking of the pools `res` / `sc` (n x N: int32 1-based with NA_integer_ and float64, on the device,
        as top_product / top_candidates write them) down to k over the columns [c0, c1) of V (n_item x ld, fp32 or fp64, on the
        device), one launch (wrmf_mmr.hip; the definition is rsparse_amd.metrics.mmr_reference): {"items": (n, k) int32 1-based
        and NA-padded, and of `want`: "scores" (the picks' own scores, float64, NaN where NA), "positions" (int32, 1-based into
        the pool), "objective" (float64)} on the device."""
        want = tuple(want)
        if any(m not in ("scores", "positions", "objective") for m in want):
            raise ValueError("mmr_rerank: want may name 'scores', 'positions' and 'objective'")
        assert res.dtype == torch.int32 and sc.dtype == torch.float64 and res.shape == sc.shape and res.dim() == 2
        inv = self.item_inv_norms(V, c0, c1)
        res, sc = res.contiguous(), sc.contiguous()
        n, N = res.shape
        k = int(k)
        out = {m: torch.empty((n, k), dtype=torch.float64 if m in ("scores", "objective") else torch.int32, device=res.device)
               for m in ("items",) + want}
        if n == 0:
            return out
        fn = self.lib.rsparse_hip_mmr_rerank_f64_device if V.dtype == torch.float64 else self.lib.rsparse_hip_mmr_rerank_device
        ptr = lambda m: out[m].data_ptr() if m in out else None
        _lib.check(fn(res.data_ptr(), sc.data_ptr(), n, N, k, float(trade_off), V.data_ptr(), int(V.shape[0]), int(V.shape[1]), int(c0),
                      int(c1), inv.data_ptr(), ptr("items"), ptr("scores"), ptr("positions"), ptr("objective"), self._stream()))
        return out

    def score_pairs(self, U, V, p, j, add=0.0, actual=None, want_scores=True):
        """the model's values at the stored positions of a CSR pattern (p, j: int32 on the device) whose rows are the rows of U
        (n x rank) and whose columns index V (n_item x rank): score[t] = add + U[row(t)] . V[j[t]], accumulated in double from
        the factors as they are -- fp32 or fp64, no replica (wrmf_score.hip).  With `actual` (float64, one per stored position)
        also the rows' sums of squared and of absolute errors.  -> (scores, sse, sae): float64 on the device, scores one per
        position, sse / sae one per row, None for what was not asked for."""
        if actual is None and not want_scores:
            raise ValueError("score_pairs: nothing asked for (no actual and want_scores=False)")
        if U.dtype != V.dtype:
            U = U.to(V.dtype)
        assert V.dtype in (torch.float32, torch.float64) and U.shape[1] == V.shape[1]
        assert p.dtype == torch.int32 and j.dtype == torch.int32
        U, V = U.contiguous(), V.contiguous()
        n, rank = U.shape
        nnz = int(j.numel())
        dev = U.device
        scores = torch.empty(nnz, dtype=torch.float64, device=dev) if want_scores else None
        sse = torch.zeros(n, dtype=torch.float64, device=dev) if actual is not None else None
        sae = torch.zeros(n, dtype=torch.float64, device=dev) if actual is not None else None
        if n == 0 or nnz == 0:   # (nothing stored: no scores, and every row's sums are zero)
            return scores, sse, sae
        if actual is not None:
            assert actual.dtype == torch.float64 and actual.numel() == nnz
            actual = actual.contiguous()
        fn = self.lib.rsparse_hip_score_pairs_f64_device if V.dtype == torch.float64 else self.lib.rsparse_hip_score_pairs_device
        _lib.check(fn(U.data_ptr(), V.data_ptr(), n, int(V.shape[0]), rank, p.data_ptr(), j.data_ptr(), float(add),
                      None if actual is None else actual.data_ptr(), None if scores is None else scores.data_ptr(),
                      None if sse is None else sse.data_ptr(), None if sae is None else sae.data_ptr(), self._stream()))
        return scores, sse, sae

    def softals_half(self, p, j, x, M, W=None, w=None, s=None, t=None, out=None, want_sumsq=False):
        """one soft-ALS half-iteration over a CSR matrix (p, j: int32, x: its values; wrmf_softals.hip), M (n_cols x r) gathered
        by column index, W (n_rows x r) the rows' own factor, w / s / t host vectors of r doubles (rsparse_amd.softals is the
        definition):  res_t = x_t - (w o W[row]) . M[j_t],  out[row] = s o sum_t res_t M[j_t] + t o W[row].  Without w and t it is
        CSR x dense scaled by s (s = None: ones).  x, M, W share one element type (float32 or float64), every sum is in double.
        -> (out in that type, sum of res^2 as a float64[1] tensor or None), both on the device."""
        assert p.dtype == torch.int32 and j.dtype == torch.int32 and M.dtype in (torch.float32, torch.float64) and x.dtype == M.dtype
        if (w is not None or t is not None) and W is None:
            raise ValueError("softals_half: w or t without W")
        n, r = int(p.numel()) - 1, int(M.shape[1])
        M = M if M.is_contiguous() else M.contiguous()
        if W is not None:
            assert W.dtype == M.dtype and tuple(W.shape) == (n, r)
            W = W if W.is_contiguous() else W.contiguous()
        vec = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(r)
        w, s, t = vec(w), vec(np.ones(r) if s is None else s), vec(t)
        ptr = lambda a: None if a is None else a.ctypes.data
        if out is None:
            out = torch.empty((n, r), dtype=M.dtype, device=M.device)
        assert out.dtype == M.dtype and tuple(out.shape) == (n, r) and out.is_contiguous()
        sumsq = torch.zeros(1, dtype=torch.float64, device=M.device) if want_sumsq else None
        fn = self.lib.rsparse_hip_softals_half_f64_device if M.dtype == torch.float64 else self.lib.rsparse_hip_softals_half_device
        _lib.check(fn(p.data_ptr(), j.data_ptr(), x.data_ptr() if x.numel() else p.data_ptr(), M.data_ptr() if M.numel() else p.data_ptr(),
                      None if W is None else W.data_ptr(), n, int(M.shape[0]), r, ptr(w), ptr(s), ptr(t),
                      out.data_ptr() if n else p.data_ptr(), None if sumsq is None else sumsq.data_ptr(), self._stream()))
        return out, sumsq

    def cooc_neighbors(self, ip, iu, up, uj, n_users, n_items, similarity, K, item0=0, item1=None, ws_rows=0):
        """the ItemKNN neighbour table of the items [item0, item1) (wrmf_itemknn.hip; rsparse_amd.itemknn.cooccurrence_reference is
        the definition): ip / iu the item-major orientation of the pattern (item -> its users), up / uj its CSR rows, int32 on the
        device; similarity: _lib.KNN_COUNT / KNN_COSINE / KNN_JACCARD.  -> (neighbors, counts): (item1 - item0, K) int32 on the
        device, 0-based with -1 where an item has fewer than K neighbours, counts 0 there.  ws_rows: dense rows per batch (0 =
        what the default workspace holds)."""
        item1 = int(n_items) if item1 is None else int(item1)
        n = max(item1 - int(item0), 0)
        assert all(t.dtype == torch.int32 for t in (ip, iu, up, uj))
        nb = torch.empty((n, int(K)), dtype=torch.int32, device=self.device)
        ct = torch.empty((n, int(K)), dtype=torch.int32, device=self.device)
        some = lambda t: t.data_ptr() if t.numel() else ip.data_ptr()   # (an empty tensor has no address to pass)
        _lib.check(self.lib.rsparse_hip_cooc_neighbors_device(ip.data_ptr(), some(iu), up.data_ptr(), some(uj), int(n_users), int(n_items),
                                                              int(item0), item1, int(similarity), int(K), int(ws_rows),
                                                              some(nb), some(ct), self._stream()))
        return nb, ct

    def cooc_neighbors_weighted(self, ip, iu, il, up, uj, ur, n_users, n_items, a, b, h, K, item0=0, item1=None, ws_rows=0):
        """the weighted ItemKNN neighbour table of the items [item0, item1) (wrmf_itemknn.hip;
        rsparse_amd.itemknn.weighted_cooccurrence_reference is the definition): c_ij = sum_u l_ui r_uj, ordered by double(c_ij) /
        (a_i b_j + h).  ip / iu / il: the item-major orientation with l by stored position, up / uj / ur: the CSR rows with r;
        the operands are integers below 2^32 held as int64, int32 or float64 here and handed on as uint32; a, b: n_items float64
        on the device, h a float.  The ranges of a, b and the 2^53 bound are the caller's to keep.  -> (neighbors (item1 - item0,
        K) int32, sums the same shape int64 holding the uint64 c_ij) on the device."""
        item1 = int(n_items) if item1 is None else int(item1)
        n = max(item1 - int(item0), 0)
        assert all(t.dtype == torch.int32 for t in (ip, iu, up, uj)) and a.dtype == b.dtype == torch.float64
        assert il.numel() == iu.numel() and ur.numel() == uj.numel() and a.numel() == b.numel() == int(n_items)
        u32 = lambda t: t.to(torch.int64).to(torch.int32).contiguous()   # (the low 32 bits: the same bits as uint32)
        il32, ur32, a, b = u32(il), u32(ur), a.contiguous(), b.contiguous()
        nb = torch.empty((n, int(K)), dtype=torch.int32, device=self.device)
        sums = torch.empty((n, int(K)), dtype=torch.int64, device=self.device)
        some = lambda t: t.data_ptr() if t.numel() else ip.data_ptr()   # (an empty tensor has no address to pass)
        _lib.check(self.lib.rsparse_hip_cooc_neighbors_weighted_device(
            ip.data_ptr(), some(iu), some(il32), up.data_ptr(), some(uj), some(ur32), int(n_users), int(n_items), int(item0), item1,
            some(a), some(b), float(h), int(K), int(ws_rows), some(nb), some(sums), self._stream()))
        return nb, sums

    def knn_recommend(self, xp, xj, neighbors, q, k, nr_p=None, nr_j=None, exclude0=None, ws_rows=0, xv=None):
        """the ItemKNN lists of the rows of a CSR pattern (xp, xj: int32 on the device) under the tables neighbors (n_items x K
        int32, 0-based, -1 = empty slot) and q (n_items x K integer weights <= 2^30, held as int64 or int32 here and handed on as
        uint32): wrmf_itemknn.hip, rsparse_amd.itemknn.knn_recommend_reference is the definition.  nr_p / nr_j: the rows'
        not_recommend entries as CSR slots (or None), exclude0: 0-based item ids (or None).  xv: the rows' integer weights, one
        per stored position (<= 2^16 - 1, a row's sum below 2^31; None = all ones): a neighbour's addend is xv * q.
        -> (items (n, k) int32, 1-based with NA_integer_; scores (n, k) int64, 0 where NA) on the device."""
        assert xp.dtype == torch.int32 and xj.dtype == torch.int32 and neighbors.dtype == torch.int32 and neighbors.shape == q.shape
        n, (n_items, K) = int(xp.numel()) - 1, neighbors.shape
        neighbors = neighbors.contiguous()
        q32 = q.to(torch.int64).to(torch.int32).contiguous()   # (q <= 2^30: the same bits as uint32)
        res = torch.empty((n, int(k)), dtype=torch.int32, device=self.device)
        sc = torch.empty((n, int(k)), dtype=torch.int64, device=self.device)
        some = lambda t: t.data_ptr() if t.numel() else xp.data_ptr()
        if xv is not None:
            assert xv.numel() == xj.numel()
            xv = xv.to(torch.int64).to(torch.int32).contiguous()
        _lib.check(self.lib.rsparse_hip_knn_recommend_weighted_device(
            xp.data_ptr(), some(xj), None if xv is None or not xv.numel() else xv.data_ptr(), n, int(n_items), some(neighbors), some(q32), int(K), None if nr_p is None else nr_p.data_ptr(),
            None if nr_p is None else some(nr_j), None if exclude0 is None or not exclude0.numel() else exclude0.data_ptr(),
            0 if exclude0 is None else int(exclude0.numel()), int(k), int(ws_rows), some(res), some(sc), self._stream()))
        return res, sc

    def item_gram(self, ip, iu, up, uj, n_users, n_items, lambda_, item0=0, item1=None, ws_rows=0, out=None):
        """rows [item0, item1) of G + lambda I of a binary pattern (wrmf_ease.hip behind the fit scatter of wrmf_itemknn.hip;
        rsparse_amd.ease.ease_gram_reference is the definition): the co-occurrence counts off the diagonal, n_i + lambda on it.
        ip / iu, up / uj: the two orientations, int32 on the device, as `cooc_neighbors` takes them.  -> (item1 - item0, n_items)
        float64 on the device; `out`: write there instead (rows of n_items doubles at any row stride >= n_items)."""
        item1 = int(n_items) if item1 is None else int(item1)
        n = max(item1 - int(item0), 0)
        assert all(t.dtype == torch.int32 for t in (ip, iu, up, uj))
        if out is None:
            out = torch.empty((n, int(n_items)), dtype=torch.float64, device=self.device)
        assert out.dtype == torch.float64 and out.is_cuda and tuple(out.shape) == (n, int(n_items)) and (n_items <= 1 or out.stride(1) == 1)
        ld = int(out.stride(0)) if n > 1 else int(n_items)
        some = lambda t: t.data_ptr() if t.numel() else ip.data_ptr()   # (an empty tensor has no address to pass)
        _lib.check(self.lib.rsparse_hip_item_gram_device(ip.data_ptr(), some(iu), up.data_ptr(), some(uj), int(n_users), int(n_items),
                                                         int(item0), item1, float(lambda_), some(out), ld, int(ws_rows), self._stream()))
        return out

    def ease_recommend(self, xp, xj, B, n_items, k, nr_p=None, nr_j=None, exclude0=None, ws_rows=0):
        """the EASE lists of the rows of a CSR pattern (xp, xj: int32 on the device) under the dense weights B: an (n_items, ld)
        float32 or float64 tensor on the device whose first n_items columns are the matrix, rows 16-byte aligned (wrmf_ease.hip;
        rsparse_amd.ease.ease_recommend_reference is the definition).  nr_p / nr_j / exclude0: as `knn_recommend`.
        -> (items (n, k) int32, 1-based with NA_integer_; keys (n, k) int64 holding the uint64 order keys of the float64 scores,
        0 where NA: rsparse_amd.ease.key_scores decodes them) on the device."""
        assert xp.dtype == torch.int32 and xj.dtype == torch.int32 and B.dtype in (torch.float32, torch.float64) and B.is_cuda
        n, n_items = int(xp.numel()) - 1, int(n_items)
        assert B.dim() == 2 and B.shape[0] == n_items and B.shape[1] >= n_items and (B.shape[1] <= 1 or B.stride(1) == 1)
        ld = int(B.stride(0)) if n_items > 1 else int(B.shape[1])
        res = torch.empty((n, int(k)), dtype=torch.int32, device=self.device)
        keys = torch.empty((n, int(k)), dtype=torch.int64, device=self.device)
        some = lambda t: t.data_ptr() if t.numel() else xp.data_ptr()
        _lib.check(self.lib.rsparse_hip_ease_recommend_device(
            xp.data_ptr(), some(xj), n, n_items, some(B), ld, int(B.dtype == torch.float64), None if nr_p is None else nr_p.data_ptr(),
            None if nr_p is None else some(nr_j), None if exclude0 is None or not exclude0.numel() else exclude0.data_ptr(),
            0 if exclude0 is None else int(exclude0.numel()), int(k), int(ws_rows), some(res), some(keys), self._stream()))
        return res, keys

    def _ease_rows(self, xp, xj, B, n_items):
        """the operands the EASE evaluation entries share with `ease_recommend`, as the C ABI takes them: -> (the leading
        arguments, `some`: the address of a tensor, or of xp for an empty one)"""
        assert xp.dtype == torch.int32 and xj.dtype == torch.int32 and B.dtype in (torch.float32, torch.float64) and B.is_cuda
        n, n_items = int(xp.numel()) - 1, int(n_items)
        assert B.dim() == 2 and B.shape[0] == n_items and B.shape[1] >= n_items and (B.shape[1] <= 1 or B.stride(1) == 1)
        ld = int(B.stride(0)) if n_items > 1 else int(B.shape[1])
        some = lambda t: t.data_ptr() if t.numel() else xp.data_ptr()
        return (xp.data_ptr(), some(xj), n, n_items, some(B), ld, int(B.dtype == torch.float64)), some

    def ease_score_pairs(self, xp, xj, B, n_items, pp, pj, ws_rows=0):
        """the EASE score of the rows of (xp, xj) -- operands as `ease_recommend` -- at the stored positions of the pattern (pp, pj:
        int32 on the device, over the same rows); nothing is masked, a column outside the items gives the key of +0.0.
        rsparse_amd.ease.ease_score_pairs_reference is the definition.  -> int64 holding the uint64 order keys, one per element of
        pj, on the device."""
        head, some = self._ease_rows(xp, xj, B, n_items)
        assert pp.dtype == torch.int32 and pj.dtype == torch.int32 and pp.numel() == xp.numel()
        out = torch.zeros(int(pj.numel()), dtype=torch.int64, device=self.device)
        _lib.check(self.lib.rsparse_hip_ease_score_pairs_device(*head, pp.data_ptr(), some(pj), int(ws_rows), some(out), self._stream()))
        return out

    def ease_top_candidates(self, xp, xj, B, n_items, k, cp, cj, nr_p=None, nr_j=None, exclude0=None, ws_rows=0):
        """`ease_recommend` within the rows' candidates (cp, cj: a canonical CSR pattern over the same rows -- columns strictly
        ascending within a row --, int32 on the device; cp may be a slice of the row pointers, its slots absolute).
        rsparse_amd.ease.ease_candidates_reference is the definition.  -> (items (n, k) int32, 1-based with NA_integer_; keys
        (n, k) int64 holding the uint64 order keys, 0 where NA) on the device."""
        head, some = self._ease_rows(xp, xj, B, n_items)
        assert cp.dtype == torch.int32 and cj.dtype == torch.int32 and cp.numel() == xp.numel()
        n = head[2]
        res = torch.empty((n, int(k)), dtype=torch.int32, device=self.device)
        keys = torch.empty((n, int(k)), dtype=torch.int64, device=self.device)
        _lib.check(self.lib.rsparse_hip_ease_top_candidates_device(*head, cp.data_ptr(), some(cj), *self._knn_filters(some, nr_p, nr_j, exclude0),
                                                                   int(k), int(ws_rows), some(res), some(keys), self._stream()))
        return res, keys

    def ease_held_out_ranks(self, xp, xj, B, n_items, ap, aj, nr_p=None, nr_j=None, exclude0=None, ws_rows=0):
        """where the entries of (ap, aj: CSR over the same rows, int32 on the device) stand among the row's admissible items by the
        EASE score (rsparse_amd.ease.ease_ranks_reference; the counts `held_out_ranks` defines).  -> (above, tied: int32, one per
        element of aj, -1 / -1 for an inadmissible entry; n_adm: int32 per row) on the device."""
        head, some = self._ease_rows(xp, xj, B, n_items)
        assert ap.dtype == torch.int32 and aj.dtype == torch.int32 and ap.numel() == xp.numel()
        n = head[2]
        above = torch.full((int(aj.numel()),), -1, dtype=torch.int32, device=self.device)
        tied = torch.full((int(aj.numel()),), -1, dtype=torch.int32, device=self.device)
        n_adm = torch.zeros(n, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.rsparse_hip_ease_held_out_ranks_device(*head, ap.data_ptr(), some(aj), *self._knn_filters(some, nr_p, nr_j, exclude0),
                                                                   int(ws_rows), some(above), some(tied), some(n_adm), self._stream()))
        return above, tied, n_adm

    def slim_columns(self, G, cols, l1, l2, max_iter, tol, W):
        """the SLIM columns `cols` (int32 on the device: any order, repeats allowed, long supports first) of the Gram matrix G
        ((n_items, >= n_items) float64 on the device, lambda = 0) by coordinate descent (wrmf_slim.hip;
        rsparse_amd.slim.slim_columns_reference is the definition), written into W: an (n_items, ld) float32 or float64 tensor
        on the device with the layout `ease_recommend` takes, ZEROED by the caller -- only the support cells of the columns are
        written.  -> the sweeps of every element of cols, int32 on the device."""
        n_items = int(W.shape[0])
        assert G.dtype == torch.float64 and G.is_cuda and G.dim() == 2 and G.shape[0] == n_items and G.shape[1] >= n_items
        assert W.dtype in (torch.float32, torch.float64) and W.is_cuda and W.dim() == 2 and W.shape[1] >= n_items
        assert (G.shape[1] <= 1 or G.stride(1) == 1) and (W.shape[1] <= 1 or W.stride(1) == 1) and cols.dtype == torch.int32
        ld_G = int(G.stride(0)) if n_items > 1 else int(G.shape[1])
        ld_W = int(W.stride(0)) if n_items > 1 else int(W.shape[1])
        sweeps = torch.zeros(int(cols.numel()), dtype=torch.int32, device=self.device)
        if not cols.numel():
            return sweeps
        some = lambda t: t.data_ptr() if t.numel() else sweeps.data_ptr()   # (an empty tensor has no address to pass)
        _lib.check(self.lib.rsparse_hip_slim_columns_device(some(G), ld_G, n_items, some(cols), int(cols.numel()), float(l1), float(l2),
                                                            int(max_iter), float(tol), some(W), ld_W, int(W.dtype == torch.float64),
                                                            some(sweeps), self._stream()))
        return sweeps

    def bpr_triples(self, p, j, n_items, nnz, row0, seed, mode, epoch, step, n_steps):
        """the BPR triples of one step of the canonical CSR rows (p, j: int32 on the device, p from 0, nnz = p[-1]) -> (u, i, neg):
        int32 on the device, neg = -1 for a void triple (wrmf_bpr.hip; rsparse_amd.bpr.bpr_triples is the definition)"""
        assert p.dtype == torch.int32 and j.dtype == torch.int32 and p.is_cuda
        cnt = max(0, -(-(int(nnz) - int(step)) // int(n_steps)))
        out = torch.empty((3, max(cnt, 1)), dtype=torch.int32, device=self.device)
        some = lambda t: t.data_ptr() if t.numel() else out.data_ptr()
        _lib.check(self.lib.rsparse_hip_bpr_triples_device(some(p), some(j), int(p.numel()) - 1, int(n_items), int(nnz), int(row0), int(seed),
                                                           int(mode), int(epoch), int(step), int(n_steps), out[0].data_ptr(),
                                                           out[1].data_ptr(), out[2].data_ptr(), self._stream()))
        return out[0, :cnt], out[1, :cnt], out[2, :cnt]

    def _bpr_call(self, name, p, j, n_items, nnz, row0, seed, mode, a, b, c, U, V, aU, aV, lr, lam, update_items, counts):
        assert p.dtype == torch.int32 and j.dtype == torch.int32 and U.dtype == V.dtype and U.dtype in (torch.float32, torch.float64)
        assert U.is_cuda and U.is_contiguous() and V.is_contiguous() and U.shape[1] == V.shape[1] and V.shape[0] == int(n_items)
        assert aU.dtype == torch.float64 and aV.dtype == torch.float64 and aU.numel() == U.shape[0] and aV.numel() == V.shape[0]
        assert U.shape[0] == p.numel() - 1 and aU.is_contiguous() and aV.is_contiguous()
        fn = getattr(self.lib, "rsparse_hip_bpr_%s%s_device" % (name, "_f64" if U.dtype == torch.float64 else ""))
        some = lambda t: t.data_ptr() if t.numel() else counts.data_ptr()   # (an empty tensor has no address to pass)
        _lib.check(fn(some(p), some(j), int(U.shape[0]), int(n_items), int(nnz), int(row0), int(seed), int(mode), int(a), int(b), int(c),
                      int(U.shape[1]), float(lr), float(lam), int(bool(update_items)), some(U), some(V), some(aU), some(aV),
                      counts.data_ptr(), self._stream()))
        return counts

    def bpr_step(self, p, j, n_items, nnz, row0, seed, mode, epoch, step, n_steps, U, V, aU, aV, lr, lam, update_items=True):
        """one BPR step in place on the factors U, V (float32 or float64, contiguous) and their Adagrad states aU, aV (float64)
        (wrmf_bpr.hip; rsparse_amd.bpr.bpr_step_reference is the definition) -> (n_valid, n_correct): int64 on the device"""
        counts = torch.zeros(2, dtype=torch.int64, device=self.device)
        return self._bpr_call("step", p, j, n_items, nnz, row0, seed, mode, epoch, step, n_steps, U, V, aU, aV, lr, lam, update_items, counts)

    def bpr_epochs(self, p, j, n_items, nnz, row0, seed, mode, epoch0, n_epochs, batch, U, V, aU, aV, lr, lam, update_items=True):
        """the epochs [epoch0, epoch0 + n_epochs) of ceil(nnz / batch) steps each (mode 1, the fold-in: one step), in place, on
        one stream -> (n_epochs, 2) int64 on the device: (n_valid, n_correct) per epoch"""
        counts = torch.zeros((max(int(n_epochs), 1), 2), dtype=torch.int64, device=self.device)
        self._bpr_call("epochs", p, j, n_items, nnz, row0, seed, mode, epoch0, n_epochs, batch, U, V, aU, aV, lr, lam, update_items, counts)
        return counts[:int(n_epochs)]

    def _knn_rows(self, xp, xj, neighbors, q, xv):
        """the operands the ItemKNN evaluation entries share with `knn_recommend`, as the C ABI takes them: -> (the leading
        arguments, `some`: the address of a tensor, or of xp for an empty one; the tensors that must outlive the call)"""
        assert xp.dtype == torch.int32 and xj.dtype == torch.int32 and neighbors.dtype == torch.int32 and neighbors.shape == q.shape
        n, (n_items, K) = int(xp.numel()) - 1, neighbors.shape
        neighbors = neighbors.contiguous()
        q32 = q.to(torch.int64).to(torch.int32).contiguous()   # (q <= 2^30: the same bits as uint32)
        some = lambda t: t.data_ptr() if t.numel() else xp.data_ptr()
        if xv is not None:
            assert xv.numel() == xj.numel()
            xv = xv.to(torch.int64).to(torch.int32).contiguous()
        head = (xp.data_ptr(), some(xj), None if xv is None or not xv.numel() else xv.data_ptr(), n, int(n_items), some(neighbors),
                some(q32), int(K))
        return head, some, (neighbors, q32, xv)

    @staticmethod
    def _knn_filters(some, nr_p, nr_j, exclude0):
        return (None if nr_p is None else nr_p.data_ptr(), None if nr_p is None else some(nr_j),
                None if exclude0 is None or not exclude0.numel() else exclude0.data_ptr(), 0 if exclude0 is None else int(exclude0.numel()))

    def knn_score_pairs(self, xp, xj, neighbors, q, pp, pj, ws_rows=0, xv=None):
        """the ItemKNN score of the rows of (xp, xj) -- operands as `knn_recommend` -- at the stored positions of the pattern
        (pp, pj: int32 on the device, over the same rows); nothing is masked, a column outside the items gives 0.
        rsparse_amd.itemknn.knn_score_pairs_reference is the definition.  -> int64, one per element of pj, on the device."""
        head, some, keep = self._knn_rows(xp, xj, neighbors, q, xv)
        assert pp.dtype == torch.int32 and pj.dtype == torch.int32 and pp.numel() == xp.numel()
        out = torch.zeros(int(pj.numel()), dtype=torch.int64, device=self.device)
        _lib.check(self.lib.rsparse_hip_knn_score_pairs_device(*head, pp.data_ptr(), some(pj), int(ws_rows), some(out), self._stream()))
        return out

    def knn_top_candidates(self, xp, xj, neighbors, q, k, cp, cj, nr_p=None, nr_j=None, exclude0=None, ws_rows=0, xv=None):
        """`knn_recommend` within the rows' candidates (cp, cj: a canonical CSR pattern over the same rows, int32 on the device;
        cp may be a slice of the row pointers, its slots absolute).  rsparse_amd.itemknn.knn_candidates_reference is the
        definition: score descending, equal scores to the smaller item.  -> (items (n, k) int32, 1-based with NA_integer_;
        scores (n, k) int64, 0 where NA) on the device."""
        head, some, keep = self._knn_rows(xp, xj, neighbors, q, xv)
        assert cp.dtype == torch.int32 and cj.dtype == torch.int32 and cp.numel() == xp.numel()
        n = head[3]
        res = torch.empty((n, int(k)), dtype=torch.int32, device=self.device)
        sc = torch.empty((n, int(k)), dtype=torch.int64, device=self.device)
        _lib.check(self.lib.rsparse_hip_knn_top_candidates_device(*head, cp.data_ptr(), some(cj), *self._knn_filters(some, nr_p, nr_j, exclude0),
                                                                  int(k), int(ws_rows), some(res), some(sc), self._stream()))
        return res, sc

    def knn_held_out_ranks(self, xp, xj, neighbors, q, ap, aj, nr_p=None, nr_j=None, exclude0=None, ws_rows=0, xv=None):
        """where the entries of (ap, aj: CSR over the same rows, int32 on the device) stand among the row's admissible items by the
        ItemKNN score (rsparse_amd.itemknn.knn_ranks_reference; the counts `held_out_ranks` defines).  -> (above, tied: int32,
        one per element of aj, -1 / -1 for an inadmissible entry; n_adm: int32 per row) on the device."""
        head, some, keep = self._knn_rows(xp, xj, neighbors, q, xv)
        assert ap.dtype == torch.int32 and aj.dtype == torch.int32 and ap.numel() == xp.numel()
        n = head[3]
        above = torch.full((int(aj.numel()),), -1, dtype=torch.int32, device=self.device)
        tied = torch.full((int(aj.numel()),), -1, dtype=torch.int32, device=self.device)
        n_adm = torch.zeros(n, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.rsparse_hip_knn_held_out_ranks_device(*head, ap.data_ptr(), some(aj), *self._knn_filters(some, nr_p, nr_j, exclude0),
                                                                  int(ws_rows), some(above), some(tied), some(n_adm), self._stream()))
        return above, tied, n_adm

    def explain_pairs(self, V, base, diag, diag_per_nnz, x_p, x_j, wa, wb, t_p, t_j):
        """what every interaction of a row contributes to the scores of the row's target items (wrmf_explain.hip): for the users
        of the CSR rows (x_p, x_j: int32 on the device; wa, wb: the assembly and contribution weight of every stored position, in
        V's type) and their targets (t_p, t_j: CSR over the same users), with A_u = base + (diag + diag_per_nnz len) I + sum_t wa_t
        v_t v_t^T and A_u z = V[target]: contrib = wb_t (z . v_t), one per (target, stored position of its user's row), and its
        sum per target.  base: rank x rank symmetric on the device, or None.  -> (contrib: V's type, total: float64 of n targets,
        flags: int32 of n users, 1 = not positive definite and the user's outputs NaN, indptr: int64 of n targets + 1 into
        contrib), all on the device."""
        assert V.dtype in (torch.float32, torch.float64) and x_p.dtype == t_p.dtype == torch.int32
        V = V.contiguous()
        dev, dt = V.device, V.dtype
        n_user, n_pairs = int(x_p.numel()) - 1, int(t_j.numel())
        assert int(t_p.numel()) == n_user + 1
        indptr = explain_segments(x_p, t_p)
        flags = torch.zeros(n_user, dtype=torch.int32, device=dev)
        total = torch.zeros(n_pairs, dtype=torch.float64, device=dev)
        n_out = int(indptr[-1]) if n_pairs else 0
        contrib_buf = torch.zeros(max(n_out, 1), dtype=dt, device=dev)   # (an empty view has no address to pass)
        if n_user == 0 or n_pairs == 0:
            return contrib_buf[:n_out], total, flags, indptr
        one = lambda t, d: t.to(d).contiguous() if t.numel() else torch.zeros(1, dtype=d, device=dev)
        x_j, wa, wb = one(x_j, torch.int32), one(wa, dt), one(wb, dt)
        if base is not None:
            base = base.to(dt).contiguous()
            assert tuple(base.shape) == (V.shape[1], V.shape[1])
        fn = self.lib.rsparse_hip_explain_f64_device if dt == torch.float64 else self.lib.rsparse_hip_explain_device
        _lib.check(fn(V.data_ptr(), int(V.shape[0]), int(V.shape[1]), None if base is None else base.data_ptr(), float(diag),
                      float(diag_per_nnz), n_user, x_p.data_ptr(), x_j.data_ptr(), wa.data_ptr(), wb.data_ptr(), t_p.data_ptr(),
                      t_j.contiguous().data_ptr(), indptr.data_ptr(), contrib_buf.data_ptr(), total.data_ptr(), flags.data_ptr(),
                      self._stream()))
        return contrib_buf[:n_out], total, flags, indptr

    def held_out_ranks(self, U, V, nr_p, nr_j, exclude0, act_p, act_j, max_chunk_users=0):
        """where the held-out items stand among all admissible items (wrmf_ranks.hip): for the rows of U (n x rank) against V
        (n_item x rank), both on the device, and the stored entries of `actual` as CSR slots (act_p, act_j: int32, j sorted within
        rows) -> (above, tied: int32, one per stored entry, -1 / -1 for an entry that is not admissible; n_adm: int32 of n).
        nr_p / nr_j / exclude0 as `top_product`.  The scores are the fp32 ones of the large-k `top_product` path: a double
        model's factors go through their fp32 replica, as for the nominating pass of `$predict`."""
        n, rank = U.shape
        n_item = V.shape[0]
        U32 = U.to(torch.float32).contiguous()
        V32 = self._v32(V).contiguous()
        assert act_p.dtype == torch.int32 and act_j.dtype == torch.int32 and act_p.numel() == n + 1
        nnz = int(act_j.numel())
        dev = U.device
        # (an empty view has no address to pass: the library gets the one-element buffers behind the views)
        above_buf = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
        tied_buf = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
        above, tied = above_buf[:nnz], tied_buf[:nnz]
        n_adm = torch.empty(n, dtype=torch.int32, device=dev)
        if n == 0:
            return above, tied, n_adm
        if nnz == 0:   # (no stored entry at all: the library still wants non-NULL slots)
            act_j = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(self.lib.rsparse_hip_held_out_ranks_device(
            U32.data_ptr(), V32.data_ptr(), n, n_item, rank, None if nr_p is None else nr_p.data_ptr(),
            None if nr_j is None else nr_j.data_ptr(), None if exclude0 is None else exclude0.data_ptr(),
            0 if exclude0 is None else int(exclude0.numel()), act_p.data_ptr(), act_j.data_ptr(), int(max_chunk_users),
            above_buf.data_ptr(), tied_buf.data_ptr(), n_adm.data_ptr(), self._stream()))
        return above, tied, n_adm

    def rank_summary(self, act_p, act_x, above, tied, n_adm):
        """the per-user numbers of those counts (weights act_x: float64, one per stored entry): (mpr, auc, mrr: float64 of n;
        sums: float64 n x 3 = sum w, sum w pct, admissible entries), on the device.  DESIGN.md 3.15."""
        n = int(n_adm.numel())
        dev = n_adm.device
        mpr, auc, mrr = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
        sums = torch.empty((n, 3), dtype=torch.float64, device=dev)
        if n == 0:
            return mpr, auc, mrr, sums
        assert act_x.dtype == torch.float64 and above.dtype == torch.int32 and tied.dtype == torch.int32
        if act_x.numel() == 0:
            act_x = torch.zeros(1, dtype=torch.float64, device=dev)
            above = tied = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(self.lib.rsparse_hip_rank_summary_device(
            n, act_p.data_ptr(), act_x.contiguous().data_ptr(), above.data_ptr(), tied.data_ptr(), n_adm.data_ptr(), mpr.data_ptr(),
            auc.data_ptr(), mrr.data_ptr(), sums.data_ptr(), self._stream()))
        return mpr, auc, mrr, sums

    def _v32(self, V):
        """the fp32 replica of a factor matrix the fp64 layer holds (kept until the matrix changes: ADVICE r04 -- `predict` of
        one user paid an n_item x rank conversion per call)"""
        if V.dtype == torch.float32:
            return V
        # keyed on the tensor OBJECT (held here, so its storage cannot be handed to a later fit's factors while the replica
        # lives) and on its version; the kernels write factors through raw pointers, which no version counter sees, so
        # whoever re-solves a matrix it keeps must call `drop_v32()` (WRMF does wherever it assigns `_V`: ADVICE r05)
        if getattr(self, "_v32_src", None) is not V or self._v32_ver != V._version:
            self._v32_cache, self._v32_src, self._v32_ver = V.to(torch.float32).contiguous(), V, V._version
        return self._v32_cache

    def drop_v32(self):
        self._v32_cache = self._v32_src = None
        self._v32_ver = -1
        self._vn_cache = self._vn_src = None   # the cosine operands derive from the same matrix
        self._vn_key = None
        self._inv_cache = self._inv_src = None   # ... and so do the inverse norms
        self._inv_key = None

    def normalized_items(self, V, c0, c1):
        """the cosine operands of a factor matrix V (n_item x ld, fp32 or fp64, on the device) over its columns [c0, c1):
        (Vn32, Vn64, exclude0) -- unit rows as float32 and float64 (n_item x (c1 - c0)) and the sorted int32 ids of the
        degenerate items (zero or non-finite norm: rows of zeros), which `similar_items` never returns.  One streaming launch
        (wrmf_similar.hip); kept until the matrix changes, keyed and dropped exactly like the fp32 replica `_v32`."""
        key = (V._version, int(c0), int(c1))
        if getattr(self, "_vn_src", None) is not V or self._vn_key != key:
            assert V.is_contiguous() and V.dim() == 2 and V.dtype in (torch.float32, torch.float64)
            n, ld = V.shape
            r = int(c1) - int(c0)
            Vn32 = torch.empty((n, max(r, 0)), dtype=torch.float32, device=V.device)
            Vn64 = torch.empty((n, max(r, 0)), dtype=torch.float64, device=V.device)
            flags = torch.empty(n, dtype=torch.int32, device=V.device)
            fn = (self.lib.rsparse_hip_normalize_items_f64_device if V.dtype == torch.float64
                  else self.lib.rsparse_hip_normalize_items_device)
            _lib.check(fn(V.data_ptr(), n, ld, int(c0), int(c1), Vn32.data_ptr(), Vn64.data_ptr(), flags.data_ptr(),
                          self._stream()))
            excl = torch.nonzero(flags).flatten().to(torch.int32)   # ascending
            self._vn_cache, self._vn_src, self._vn_key = (Vn32, Vn64, excl), V, key
        return self._vn_cache

    def similar_items(self, V, c0, c1, query, k, exclude0=None, exclude_self=True):
        """the k items most similar (cosine over the columns [c0, c1) of V) to each item of `query` (int32 ids on the device):
        (indices int32 n_q x k, 1-based with NA_integer_; cosines float64 n_q x k), as top_product returns them.  exclude0:
        sorted 0-based ids excluded for every query (or None); the degenerate items are excluded besides."""
        Vn32, Vn64, degenerate = self.normalized_items(V, c0, c1)
        n_item, r = Vn32.shape
        excl = degenerate
        if exclude0 is not None and exclude0.numel():
            excl = torch.unique(torch.cat([degenerate, exclude0.to(torch.int32)])).to(torch.int32)   # sorted
        query = query.to(torch.int32).contiguous()
        n_q = int(query.numel())
        res = torch.empty((n_q, k), dtype=torch.int32, device=V.device)
        sc = torch.empty((n_q, k), dtype=torch.float64, device=V.device)
        _lib.check(self.lib.rsparse_hip_similar_items_device(
            Vn32.data_ptr(), Vn64.data_ptr(), n_item, r, query.data_ptr(), n_q, int(k), int(bool(exclude_self)),
            excl.data_ptr() if excl.numel() else None, int(excl.numel()), res.data_ptr(), sc.data_ptr(), self._stream()))
        return res, sc

    def initialize_biases_explicit(self, csc_ui, csc_iu, user_bias, item_bias, lambda_, dynamic_lambda, non_negative,
                                   calculate_global_bias):
        """wrmf_utils.hpp:32-84 on the device; with calculate_global_bias the resident values of both handles
        lose their mean in place.  Returns the global bias."""
        gb = ctypes.c_double(0.0)
        if csc_ui.f64:
            _lib.check(self.lib.rsparse_hip_initialize_biases_f64_device(
                csc_ui.h, csc_iu.h, user_bias.data_ptr(), item_bias.data_ptr(), float(lambda_), int(bool(dynamic_lambda)),
                int(bool(non_negative)), int(bool(calculate_global_bias)), 1, ctypes.byref(gb), self._stream()))
            return gb.value
        _lib.check(self.lib.rsparse_hip_initialize_biases_explicit_device(
            csc_ui.h, csc_iu.h, user_bias.data_ptr(), item_bias.data_ptr(), float(lambda_), int(bool(dynamic_lambda)),
            int(bool(non_negative)), int(bool(calculate_global_bias)), ctypes.byref(gb), self._stream()))
        return gb.value

    def initialize_biases_implicit(self, csc_ui, csc_iu, user_bias, item_bias, lambda_, non_negative,
                                   calculate_global_bias=False):
        """wrmf_utils.hpp:86-165 on the device.  Returns the global bias (0 unless calculate_global_bias)."""
        gb = ctypes.c_double(0.0)
        if csc_ui.f64:
            _lib.check(self.lib.rsparse_hip_initialize_biases_f64_device(
                csc_ui.h, csc_iu.h, user_bias.data_ptr(), item_bias.data_ptr(), float(lambda_), 0,
                int(bool(non_negative)), int(bool(calculate_global_bias)), 0, ctypes.byref(gb), self._stream()))
            return gb.value
        _lib.check(self.lib.rsparse_hip_initialize_biases_implicit_device(
            csc_ui.h, csc_iu.h, user_bias.data_ptr(), item_bias.data_ptr(), float(lambda_), int(bool(non_negative)),
            int(bool(calculate_global_bias)), ctypes.byref(gb), self._stream()))
        return gb.value

    def bias_sweep_explicit(self, csc, other_bias, lambda_, dynamic_lambda, non_negative, out):
        """one sweep of initialize_biases_explicit over the columns of `csc` (a block): out[c] = sum (x - other_bias[idx]) /
        (lambda_use + n_c)  (wrmf_utils.hpp:56-81)"""
        fn = self.lib.rsparse_hip_bias_sweep_explicit_f64_device if csc.f64 else self.lib.rsparse_hip_bias_sweep_explicit_device
        _lib.check(fn(csc.h, other_bias.data_ptr(), float(lambda_), int(bool(dynamic_lambda)), int(bool(non_negative)),
                      out.data_ptr(), self._stream()))

    def bias_prep_implicit(self, csc, n_other, lambda_, means, adj):
        """means / adjustments of the columns of `csc` (wrmf_utils.hpp:97-124); n_other = the true size of the other side"""
        fn = self.lib.rsparse_hip_bias_prep_implicit_f64_device if csc.f64 else self.lib.rsparse_hip_bias_prep_implicit_device
        _lib.check(fn(csc.h, int(n_other), float(lambda_), means.data_ptr(), adj.data_ptr(), self._stream()))

    def bias_sweep_implicit(self, csc, other_bias, n_other, other_sum, means, adj, non_negative, global_bias, out):
        """one sweep of initialize_biases_implicit over the columns of `csc` (wrmf_utils.hpp:136-143, 152-159); other_sum:
        float64[1] on the device = sum of the other side's biases (None: 0)"""
        fn = self.lib.rsparse_hip_bias_sweep_implicit_f64_device if csc.f64 else self.lib.rsparse_hip_bias_sweep_implicit_device
        _lib.check(fn(csc.h, other_bias.data_ptr(), int(n_other), None if other_sum is None else other_sum.data_ptr(),
                      means.data_ptr(), adj.data_ptr(), int(bool(non_negative)), float(global_bias), out.data_ptr(),
                      self._stream()))

    def subtract_mean(self, x, x_other=None):
        """global_bias = mean(x), removed in place from x (and from the other orientation's values) -- R/model_WRMF.R:278-282"""
        m = ctypes.c_double(0.0)
        fn = (self.lib.rsparse_hip_values_subtract_mean_f64_device if x.dtype == torch.float64
              else self.lib.rsparse_hip_values_subtract_mean_device)
        _lib.check(fn(int(x.numel()), x.data_ptr(),
                      None if x_other is None else x_other.data_ptr(), ctypes.byref(m), self._stream()))
        return m.value

    def weighted_sumsq(self, F, w, out):
        n, k = F.shape
        fn = self.lib.rsparse_hip_weighted_sumsq_f64_device if F.dtype == torch.float64 else self.lib.rsparse_hip_weighted_sumsq_device
        assert w is None or w.dtype == F.dtype
        _lib.check(fn(F.data_ptr(), k, n, None if w is None else w.data_ptr(), out.data_ptr(), self._stream()))

    def set_launch_mode(self, mode):
        """0 = the launches of a CG half-iteration back to back on one stream (profilers), 2 = the default overlap"""
        _lib.check(self.lib.rsparse_hip_set_launch_mode(int(mode)))

    def profile(self, on):
        _lib.check(self.lib.rsparse_hip_profile_enable(int(bool(on))))

    def profile_last(self):
        """milliseconds of the kernels of the last device-layer call (see rsparse_hip_profile_last)"""
        buf = (ctypes.c_double * 8)()
        _lib.check(self.lib.rsparse_hip_profile_last(buf))
        return list(buf)

    def profile_last_names(self):
        """kernel names of the segments of the last profiled call, as the runtime's symbol table has them"""
        buf = ctypes.create_string_buffer(8192)
        _lib.check(self.lib.rsparse_hip_profile_last_names(buf, 8192))
        return buf.value.decode().split("\n")

    def numeric_counts(self):
        """(rows whose general solve failed too, rows that went to the general solver) since the last call; resets."""
        bad, fell = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self.lib.rsparse_hip_take_numeric_failures(ctypes.byref(bad), ctypes.byref(fell)))
        return int(bad.value), int(fell.value)

    def report_numeric(self, bad, fell):
        self.last_fallback_rows = fell
        if fell:
            import warnings
            warnings.warn("rsparse_amd: %d per-row systems were not positive definite; solved by the general (LU) solver "
                          "(the reference's arma::solve warns likewise)" % fell, RuntimeWarning, stacklevel=3)
        if bad:
            raise _lib.RsparseHipError(_lib.ERR_NUMERIC, "%d per-row systems were singular" % bad)

    def check_numeric(self):
        """Raises if per-row systems of the exact solver were singular for the general-solver fallback too; systems that
        were merely not positive definite were re-solved on the device and are reported like the reference's warning.
        (One rank's view: a sharded driver sums `numeric_counts()` over its ranks first -- WRMF._check_numeric.)"""
        self.report_numeric(*self.numeric_counts())


class _CscHandle:
    def __init__(self, lib, h, keep, n_rows, n_cols, f64=False):
        self.lib, self.h, self.keep = lib, h, keep
        self.n_rows, self.n_cols = n_rows, n_cols
        self.f64 = bool(f64)   # a handle of the fp64 layer (rsparse_hip_csc_f64): no launch schedule, no info()

    def freeze_values(self, frozen=True):
        """the values will not change until further notice: their statistics are scanned once, not per half-iteration
        (rsparse_hip_csc_freeze_values; no-op on the fp64 layer)"""
        if not self.f64:
            _lib.check(self.lib.rsparse_hip_csc_freeze_values(self.h, int(bool(frozen))))

    def info(self):
        if self.f64:
            raise RuntimeError("csc_info describes the fp32 launch schedule; an fp64 handle has none")
        buf = (ctypes.c_int64 * 40)()
        _lib.check(self.lib.rsparse_hip_csc_info(self.h, buf))
        return dict(n_rows=buf[0], n_cols=buf[1], nnz=buf[2], n_long=buf[3], max_len=buf[4], nnz_long=buf[5],
                    n_empty=buf[6], tile_nnz=buf[7], bucket_rows=list(buf[8:14]), bucket_nnz=list(buf[14:20]),
                    cgq_cfg=buf[20], ne_segments=buf[21], bucket_wpr=list(buf[22:28]), bucket_capq=list(buf[28:34]),
                    bucket_waves=[abs(v) for v in buf[34:40]], bucket_stream=[int(v < 0) for v in buf[34:40]])

    def __del__(self):
        try:
            if self.h:
                (self.lib.rsparse_hip_csc_f64_destroy if self.f64 else self.lib.rsparse_hip_csc_destroy)(self.h)
                self.h = None
        except Exception:
            pass


class ShardedALS:
    """Both orientations of one interaction matrix, row-sharded over the ranks of `group`.

    c_ui : CSC of the users x items matrix -> columns = items  (solved in the item half)
    c_iu : CSC of its transpose            -> columns = users  (solved in the user half)
    Each rank is given the column block it owns (p re-based to 0); row indices are GLOBAL ids of the other side and
    are translated to that side's storage rows here (Layout).  Factor matrices live in storage order: allocate them
    with `lay_user.alloc` / `lay_item.alloc`, convert with `Layout.from_global` / `to_global`.
    """

    def __init__(self, backend, n_user, n_item, rank_k, c_ui_block, c_iu_block, total_nnz, feedback="implicit",
                 lambda_=0.0, dynamic_lambda=True, cg_steps=3, group=None, world_size=1, my_rank=0, with_bias=False,
                 lay_user=None, lay_item=None, force_collectives=False):
        self.be, self.k = backend, int(rank_k)
        self.n_user, self.n_item, self.total_nnz = int(n_user), int(n_item), int(total_nnz)
        self.implicit = feedback == "implicit"
        self.with_bias = bool(with_bias)     # rank_k counts the row of ones and the bias row (R/model_WRMF.R:160)
        self.lambda_, self.dynamic_lambda, self.cg_steps = float(lambda_), bool(dynamic_lambda), int(cg_steps)
        self.group, self.ws, self.me = group, int(world_size), int(my_rank)
        # collectives are issued when there is more than one rank -- or when a test asks for them on a one-rank group
        # (the RCCL branches can then be executed on a single GPU: tests/test_nccl_single_rank.py)
        self.coll = self.ws > 1 or bool(force_collectives)
        if lay_user is None or lay_item is None:
            lay_user, lay_item = self.layouts(n_user, n_item, self.ws)
        self.lay_user, self.lay_item = lay_user, lay_item
        dev = c_ui_block[0].device
        self.dtype = c_ui_block[2].dtype   # float32, or float64: the fp64 layer (WRMF(precision="double"))
        # item half: fixed side = users, solved = my items; user half: fixed side = items, solved = my users
        self.csc_items, self.sub_items = self._make(c_ui_block, lay_user, lay_item)
        self.csc_users, self.sub_users = self._make(c_iu_block, lay_item, lay_user)
        self.x_items, self.x_users = c_ui_block[2], c_iu_block[2]   # the resident values (the sub-block handles view them)
        self.scal_sub = torch.zeros(max(lay_user.n_sub, lay_item.n_sub), dtype=torch.float64, device=dev)
        self.G = torch.zeros((self.k, self.k), dtype=self.dtype, device=dev)
        self.Gpart = torch.zeros((self.k, self.k), dtype=self.dtype, device=dev)
        self.scal = torch.zeros(4, dtype=torch.float64, device=dev)   # [0] sumsq, [1] loss rows, [2] spare
        # one collective per Gramian: every rank contributes [k x k partial, sum(F^2), max |F|] (doubles), all ranks get
        # all contributions and reduce them locally in rank order (sums and the maximum: deterministic, identical everywhere)
        self.red_in = torch.zeros(self.k * self.k + 2, dtype=torch.float64, device=dev)
        self.red_all = torch.zeros((self.ws, self.k * self.k + 2), dtype=torch.float64, device=dev)
        self.absmax = torch.zeros(1, dtype=torch.float32, device=dev)   # max |F| of the fixed side (gramian())
        self.absmax_of = None
        self.global_bias = 0.0 # implicit feedback: the model's global bias (R/model_WRMF.R:285-287); explicit: data are shifted
        self.cnt_user = None   # nnz per user / item in GLOBAL order (weights of the explicit regulariser)
        self.cnt_item = None

    @staticmethod
    def layouts(n_user, n_item, world_size, cnt_user=None, cnt_item=None, n_sub=None):
        """Layouts of the two factor matrices: nnz-balanced blocks when the per-row counts are given, equal row counts
        otherwise; callers cut their CSC blocks at exactly `lay.bounds`."""
        n_sub = default_subblocks(world_size) if n_sub is None else n_sub
        nsu, nsi = (n_sub if isinstance(n_sub, (tuple, list)) else (n_sub, n_sub))   # (users, items): the user side moves 10x the bytes
        bu = balanced_bounds(cnt_user, world_size) if cnt_user is not None else equal_bounds(n_user, world_size)
        bi = balanced_bounds(cnt_item, world_size) if cnt_item is not None else equal_bounds(n_item, world_size)
        return Layout(n_user, bu, int(nsu)), Layout(n_item, bi, int(nsi))

    def _make(self, block, lay_fixed, lay_solved):
        """CSC handle of my whole block (single-rank path, info, parity sampling) and one handle per sub-block, with the
        row indices translated to the fixed side's storage rows."""
        p, i, x = block
        i = lay_fixed.to_storage(i).contiguous()
        n_my = lay_solved.bounds[self.me][1] - lay_solved.bounds[self.me][0]
        whole = self.be.make_csc(lay_fixed.rows, n_my, p, i, x)
        subs = []
        if lay_solved.n_sub > 1:
            p64 = p.to(torch.int64)
            for j in range(lay_solved.n_sub):
                c0, c1 = lay_solved.sub_rows(self.me, j)
                lo, hi = int(p64[c0]), int(p64[c1])
                sp_ = (p64[c0:c1 + 1] - lo).to(torch.int32).contiguous()
                subs.append((c0, c1, self.be.make_csc(lay_fixed.rows, c1 - c0, sp_, i[lo:hi].contiguous(),
                                                      x[lo:hi].contiguous())))
        else:
            subs.append((0, n_my, whole))
        return whole, subs

    def _all_reduce(self, t):
        if self.coll:
            torch.distributed.all_reduce(t, group=self.group)

    def finish(self):
        """make the current stream wait for the exchanges a half_iteration left running (the last slab's all-gather):
        call before reading a factor matrix outside half_iteration()"""
        for w in getattr(self, "_pending", ()):
            w.wait()
        self._pending = []

    def _gather_slab(self, S, lay, j):
        """In-place all-gather of sub-block j of every rank (one contiguous slab of S); returns a work handle or None."""
        if not self.coll:
            return None
        a, b = lay.slab(j)
        out = S[a:b]
        mine = S[lay.sub_start(self.me, j):lay.sub_start(self.me, j) + lay.Bs]
        if S.is_cuda and torch.distributed.get_backend(self.group) == "gloo":
            host = out.cpu()   # dry-run configuration only (several ranks sharing one GPU): gloo has no device all-gather
            torch.distributed.all_gather_into_tensor(host, host[self.me * lay.Bs:(self.me + 1) * lay.Bs].clone(),
                                                     group=self.group)
            out.copy_(host)
            return None
        if not S.is_cuda:      # gloo on CPU tensors (tests): no in-place aliasing guarantees, gather from a copy
            torch.distributed.all_gather_into_tensor(out, mine.clone(), group=self.group)
            return None
        return torch.distributed.all_gather_into_tensor(out, mine, group=self.group, async_op=True)

    def _my_pieces(self, lay):
        """storage slices [a, b) holding my real rows (one per sub-block)"""
        out = []
        for j in range(lay.n_sub):
            c0, c1 = lay.sub_rows(self.me, j)
            if c1 > c0:
                a = lay.sub_start(self.me, j)
                out.append((a, a + (c1 - c0)))
        return out

    def gramian(self, F, lay):
        """G = F F^T + fl(lambda) I over the real rows of F (storage order, layout `lay`), reduced over the ranks;
        scal[0] = sum(F^2)."""
        pieces = self._my_pieces(lay)
        # max |F| rides along (the long-row kernel scales its fp16 operands by it): own blocks here, maximum over the
        # ranks below; half_iteration() hands it to the library so that no half-iteration call scans F again
        self.absmax.zero_()
        self.absmax_of = None
        if not self.coll and len(pieces) == 1:
            a, b = pieces[0]
            self.be.gramian(F[a:b], self.lambda_, self.G, self.scal[0:1], self.absmax)
            self.absmax_of = F
            return self.G
        self.G.zero_()
        self.scal[0:1].zero_()
        for a, b in pieces:
            self.be.gramian(F[a:b], 0.0, self.Gpart, self.scal[2:3], self.absmax)
            self.G += self.Gpart
            self.scal[0:1] += self.scal[2:3]
        if self.coll:   # ONE collective for the k x k partial, sum(F^2) and max |F| (see red_in / red_all)
            kk = self.k * self.k
            self.red_in[:kk] = self.G.reshape(-1)
            self.red_in[kk] = self.scal[0]
            self.red_in[kk + 1] = self.absmax[0]
            if self.red_in.is_cuda and torch.distributed.get_backend(self.group) == "gloo":
                host = self.red_all.cpu()   # dry-run configuration only (ranks sharing one GPU under gloo)
                torch.distributed.all_gather_into_tensor(host.view(-1), self.red_in.cpu(), group=self.group)
                self.red_all.copy_(host)
            else:
                torch.distributed.all_gather_into_tensor(self.red_all.view(-1), self.red_in, group=self.group)
            tot = self.red_all[:, :kk + 1].sum(dim=0)
            self.G.copy_(tot[:kk].view(self.k, self.k))
            self.scal[0] = tot[kk]
            self.absmax[0] = self.red_all[:, kk + 1].max()
        self.absmax_of = F
        self.G.diagonal().add_(float(np.float32(self.lambda_)))   # fl(diag(lambda)), R/model_WRMF.R:476
        return self.G

    def gramian_bias(self, F, lay, bias_last_row):
        """(k-1) x (k-1) Gramian of F without its bias row + fl(lambda) I (R/model_WRMF.R:463-486, 345-351)."""
        k1 = self.k - 1
        if getattr(self, "Gb", None) is None:
            self.Gb = torch.zeros((k1, k1), dtype=self.dtype, device=F.device)
            self.Gbp = torch.zeros((k1, k1), dtype=self.dtype, device=F.device)
        self.Gb.zero_()
        for a, b in self._my_pieces(lay):
            blk = (F[a:b, :k1] if bias_last_row else F[a:b, 1:]).contiguous()
            self.be.gramian(blk, 0.0, self.Gbp, None)
            self.Gb += self.Gbp
        self._all_reduce(self.Gb)
        self.Gb.diagonal().add_(float(np.float32(self.lambda_)))
        return self.Gb

    def _gather_vec(self, v, lay):
        """all sub-blocks of a storage-order vector (a bias vector) -> every rank"""
        for j in range(lay.n_sub):
            w = self._gather_slab(v, lay, j)
            if w is not None:
                w.wait()

    def initialize_biases(self, user_bias, item_bias, non_negative, calculate_global_bias):
        """initialize_biases_explicit / _implicit (inst/include/wrmf_utils.hpp:32-165) over the sharded matrix: user_bias
        (lay_user.rows,) and item_bias (lay_item.rows,) are storage-order vectors, complete on every rank on return.  Every
        sweep runs over the rank's own block against the full vector of the other side (the rule of a sweep is per column),
        then the swept block is all-gathered; sums that span the matrix (the global mean, the mean of a bias vector) are
        all-reduced or taken from the full vector.  With explicit feedback and calculate_global_bias the mean leaves the
        resident values of both orientations in place, as in the reference (:41-52).  Returns the global bias."""
        be, lu, li = self.be, self.lay_user, self.lay_item
        dev = user_bias.device
        gb = 0.0
        self.finish()

        def total(t):   # sum over all ranks of a local float64 scalar tensor
            self._all_reduce(t)
            return float(t)

        def sweep(subs, lay, fn):
            for j, (c0, c1, sub) in enumerate(subs):
                if c1 > c0:
                    a = lay.sub_start(self.me, j)
                    fn(sub, c0, c1, a)

        if not self.implicit:
            if calculate_global_bias and self.total_nnz > 0:   # :41-52 (the mean is global; each rank shifts its own values)
                gb = total(self.x_items.double().sum().reshape(1)) / float(self.total_nnz)
                self.x_items.sub_(gb)
                self.x_users.sub_(gb)
            for _ in range(5):                                 # :54-82
                sweep(self.sub_items, li, lambda sub, c0, c1, a: be.bias_sweep_explicit(
                    sub, user_bias, self.lambda_, self.dynamic_lambda, non_negative, item_bias[a:a + (c1 - c0)]))
                self._gather_vec(item_bias, li)
                sweep(self.sub_users, lu, lambda sub, c0, c1, a: be.bias_sweep_explicit(
                    sub, item_bias, self.lambda_, self.dynamic_lambda, non_negative, user_bias[a:a + (c1 - c0)]))
                self._gather_vec(user_bias, lu)
            return gb
        n_it = li.bounds[self.me][1] - li.bounds[self.me][0]
        n_us = lu.bounds[self.me][1] - lu.bounds[self.me][0]
        im, ia = (torch.zeros(max(n_it, 1), dtype=torch.float64, device=dev) for _ in range(2))
        um, ua = (torch.zeros(max(n_us, 1), dtype=torch.float64, device=dev) for _ in range(2))
        sweep(self.sub_items, li, lambda sub, c0, c1, a: be.bias_prep_implicit(sub, self.n_user, self.lambda_, im[c0:c1], ia[c0:c1]))
        sweep(self.sub_users, lu, lambda sub, c0, c1, a: be.bias_prep_implicit(sub, self.n_item, self.lambda_, um[c0:c1], ua[c0:c1]))
        if calculate_global_bias:                              # :90-93
            sm = total(self.x_items.double().sum().reshape(1))
            gb = sm / (sm + float(self.n_user) * float(self.n_item) - float(self.total_nnz))
        if non_negative:
            gb = max(0.0, gb)
        for it in range(5):                                    # :130-162 (padding rows of a bias vector are zero: the sums are the real ones)
            usum = user_bias.double().sum().reshape(1) if it > 0 else None
            sweep(self.sub_items, li, lambda sub, c0, c1, a: be.bias_sweep_implicit(
                sub, user_bias, self.n_user, usum, im[c0:c1], ia[c0:c1], non_negative, gb, item_bias[a:a + (c1 - c0)]))
            self._gather_vec(item_bias, li)
            isum = item_bias.double().sum().reshape(1)
            sweep(self.sub_users, lu, lambda sub, c0, c1, a: be.bias_sweep_implicit(
                sub, item_bias, self.n_item, isum, um[c0:c1], ua[c0:c1], non_negative, gb, user_bias[a:a + (c1 - c0)]))
            self._gather_vec(user_bias, lu)
        return gb

    def freeze_values(self, frozen=True):
        """Implicit feedback: the confidences never change during a fit (the explicit global mean and the bias initialisation
        do change explicit values, in place) -- tell the library, so that it scans them once per handle instead of once per
        half-iteration.  Called by the drivers once the values are final."""
        for h in [self.csc_items, self.csc_users] + [t[2] for t in self.sub_items] + [t[2] for t in self.sub_users]:
            if hasattr(h, "freeze_values"):
                h.freeze_values(frozen)

    def half_iteration(self, side, U, V, solver, G=None, want_loss=True, defer_exchange=False):
        """side 'items': solve V (item factors) given U; side 'users': solve U given V (both in storage order).
        Returns loss/nnz as the reference reports it: a python float (want_loss=True, synchronises), a 0-d device
        tensor (want_loss='device': no host sync, fetch it when convenient) or None.
        defer_exchange: leave the wait for the LAST sub-block's all-gather to the next half_iteration (which waits before
        its first solve, i.e. after its own Gramian partial) -- the caller then calls finish() before it reads U / V itself."""
        if side == "items":
            F, layF, S, layS, subs, cnt_F = U, self.lay_user, V, self.lay_item, self.sub_items, self.cnt_user
        else:
            F, layF, S, layS, subs, cnt_F = V, self.lay_item, U, self.lay_user, self.sub_users, self.cnt_item
        # user/item biases: solving the items means X = U = [1, ..., user_bias] (is_bias_last_row = TRUE), solving the
        # users X = components = [item_bias, ..., 1] (FALSE)  -- R/model_WRMF.R:321-329
        blr = (side == "items") if self.with_bias else None
        own_gramian = self.implicit and G is None
        if own_gramian:
            G = self.gramian_bias(F, layF, blr) if self.with_bias else self.gramian(F, layF)
        # solve sub-block j, start its exchange, solve sub-block j+1 meanwhile (both halves alike)
        works = []
        self.scal_sub.zero_()
        # max |F| rides along with THIS call's own Gramian (gramian() above); a Gramian supplied by the caller says
        # nothing about F's current content, so nothing is passed then and the library scans F itself
        extra = {}
        if self.implicit and own_gramian and self.absmax_of is F:
            extra["absmax"] = self.absmax
        self.absmax_of = None   # F's owner may change it before the next Gramian
        if self.global_bias:
            extra["global_bias"] = self.global_bias
        # the exchanges of the PREVIOUS half may still be running (their waits are deferred to here: what came in between --
        # that half's loss, this half's Gramian partial over the rank's own rows -- reads nothing they write)
        self.finish()
        for j, (c0, c1, sub) in enumerate(subs):
            if c1 > c0:
                a = layS.sub_start(self.me, j)
                self.be.half_iteration(sub, self.implicit, F, S[a:a + (c1 - c0)], G, self.lambda_, solver,
                                       self.cg_steps, self.dynamic_lambda, self.scal_sub[j:j + 1], blr, **extra)
            works.append(self._gather_slab(S, layS, j))
        # every slab but the last is waited for here; the last one's wait is deferred to the next reader of S -- the next
        # half_iteration's first solve, initialize_biases, or finish() (callers that read S themselves call it)
        for w in (works[:-1] if defer_exchange else works):
            if w is not None:
                w.wait()
        self._pending = [w for w in works[-1:] if w is not None] if defer_exchange else []
        self.scal[1:2] = self.scal_sub.sum()
        if not want_loss:
            return None
        # regulariser on the fixed side (wrmf_implicit.hpp:286-301, wrmf_explicit.hpp:146-173)
        if self.lambda_ > 0 and not (self.implicit and G is self.G):   # else scal[0] already holds sum(F^2)
            self.scal[0:1].zero_()
            g0 = layF.bounds[self.me][0]
            for j in range(layF.n_sub):
                c0, c1 = layF.sub_rows(self.me, j)
                if c1 <= c0:
                    continue
                a = layF.sub_start(self.me, j)
                w = None
                if (not self.implicit) and self.dynamic_lambda:
                    w = cnt_F[g0 + c0:g0 + c1]
                Freg = F[a:a + (c1 - c0)]
                if self.with_bias:   # every row of X but the ones (wrmf_explicit.hpp:147-159): ones first when the
                    Freg = (Freg[:, 1:] if blr else Freg[:, :self.k - 1]).contiguous()   # x bias is last, else last
                self.be.weighted_sumsq(Freg, w, self.scal[2:3])
                self.scal[0:1] += self.scal[2:3]
            self._all_reduce(self.scal[0:2])   # regulariser and row part of the loss in ONE all-reduce
        else:
            self._all_reduce(self.scal[1:2])
        loss = (self.scal[1] + self.lambda_ * self.scal[0]) / float(self.total_nnz)
        return loss.clone() if want_loss == "device" else float(loss)
