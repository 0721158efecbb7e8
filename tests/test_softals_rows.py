"""The soft-ALS half-iteration kernel (wrmf_softals.hip) per row against its numpy definition, softals_half_reference: every rank
class, both element types, the three modes, at the row lengths where the kernel changes course -- a lane group's share, a wave's
chunk, the span from which a row is split between waves -- and on rows far beyond it."""
import functools

import numpy as np
import pytest
import torch

from rsparse_amd import _lib
from rsparse_amd.softals import softals_half_reference
from test_softals_abi import half_bound

pytestmark = pytest.mark.gpu

N_COLS = 300
CHUNK, SPLIT = _lib.SOFTALS_CHUNK, _lib.SOFTALS_SPLIT
RANKS = [1, 3, 4, 10, 32, 64, 100, 128, 132, 256]
MODES = ["plain", "residual", "residual_own"]
LONG = 40000


def _lengths():
    rng = np.random.default_rng(11)
    edges = [1, 2, 3, 4, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7, SPLIT - 1, SPLIT, SPLIT + 1]
    run = rng.integers(1, 4, size=2000).tolist()
    # an empty row first and last; the 40 000-entry row second, in the middle and next to last (`inner` drops the two empty rows)
    return np.array([0, LONG] + edges + [0, 0] + run[:1000] + [LONG] + run[1000:] + edges[::-1] + [0, 7, LONG, 0], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def pattern():
    """(p, j, x64): j unsorted with repeats (a row of 40 000 over 300 columns), values N(0, 1)"""
    lens = _lengths()
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rng = np.random.default_rng(12)
    nnz = int(p[-1])
    assert len(lens) < 2200 and nnz < 200000
    return p, rng.integers(0, N_COLS, size=nnz).astype(np.int32), rng.standard_normal(nnz)


@functools.lru_cache(maxsize=None)
def case(r, dt, mode):
    """operands of one case in the element type `dt`, and the reference: (x, M, W, w, s, t, ref, mag, ssq, ssq_mag)"""
    p, j, x64 = pattern()
    n = p.size - 1
    rng = np.random.default_rng(1000 + r)
    npdt = np.float32 if dt == "float" else np.float64
    x = x64.astype(npdt)
    M = rng.standard_normal((N_COLS, r)).astype(npdt)
    W = rng.standard_normal((n, r)).astype(npdt) if mode != "plain" else None
    s = rng.random(r) + 0.5
    s[1::5] = 0.0                                                     # some s_c = 0
    w = rng.random(r) / r if mode != "plain" else None
    t = rng.random(r) if mode == "residual_own" else None
    ref, ssq = softals_half_reference(p, j, x, M, W, w, s, t)
    mag, ssq_mag = softals_half_reference(p, j, np.abs(x), np.abs(M), None if W is None else np.abs(W), None if w is None else -w,
                                          s, t)
    return x, M, W, w, s, t, ref, mag, ssq, ssq_mag


@pytest.fixture(scope="module")
def be():
    from rsparse_amd.engine import HipBackend
    return HipBackend()


def dev(be, a, offset=0):
    """`a` on the device; offset = 1: in a buffer of its own, one element behind a 16-byte boundary"""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(be.device)
    if not offset:
        return t
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=be.device)
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def run(be, r, dt, mode, rows=slice(None), offset=0, j_override=None):
    p, j, _ = pattern()
    x, M, W, w, s, t = case(r, dt, mode)[:6]
    p = p[rows]
    W = None if W is None else W[rows][:p.size - 1]
    j = j if j_override is None else j_override
    return be.softals_half(dev(be, p), dev(be, j), dev(be, x), dev(be, M, offset), dev(be, W, offset), w, s, t, want_sumsq=True)


def check(be, r, dt, mode, inner=False, offset=0):
    p, _, _ = pattern()
    ref, mag, ssq, ssq_mag = case(r, dt, mode)[6:]
    rows = slice(1, -1) if inner else slice(None)     # (the two outer rows are empty: p[1] = 0, and nothing is stored behind p[-2])
    out, ss = run(be, r, dt, mode, rows, offset)
    out2, ss2 = run(be, r, dt, mode, rows, offset)
    assert torch.equal(out, out2) and torch.equal(ss, ss2)            # no atomics: the same bits
    out, ss = out.cpu().numpy().astype(np.float64), float(ss.cpu()[0])
    sel = slice(1, -1) if inner else slice(None)
    ref, mag, length = ref[sel], mag[sel], np.diff(p.astype(np.int64))[sel]
    eps_out = 2.0 ** -24 if dt == "float" else 2.0 ** -53
    err = np.abs(out - ref)
    bound = half_bound(ref, mag, length[:, None], r, eps_out)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    nnz = int(p[-1])
    ss_err, ss_bound = abs(ss - ssq), float(half_bound(ssq, ssq_mag, nnz, r, 2.0 ** -53))
    print("r=%d %s %s inner=%s offset=%d: max error / bound %.3g, sumsq error %.3g (bound %.3g)"
          % (r, dt, mode, inner, offset, worst, ss_err, ss_bound))
    assert out.shape == ref.shape and np.all(np.isfinite(out))
    bad = np.argwhere(err > bound)
    assert bad.size == 0, "row %d (length %d) column %d: error %.3g > %.3g" % (
        bad[0][0], length[bad[0][0]], bad[0][1], err[tuple(bad[0])], bound[tuple(bad[0])])
    assert ss_err <= ss_bound


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", ["float", "double"])
@pytest.mark.parametrize("r", RANKS)
def test_rows_against_the_definition(be, r, dt, mode):
    check(be, r, dt, mode)


@pytest.mark.parametrize("dt", ["float", "double"])
@pytest.mark.parametrize("r", [4, 10, 128])
def test_a_long_row_first_and_last(be, r, dt):
    check(be, r, dt, "residual_own", inner=True)


@pytest.mark.parametrize("mode", ["plain", "residual_own"])
@pytest.mark.parametrize("dt", ["float", "double"])
@pytest.mark.parametrize("r", [4, 32, 128])
def test_misaligned_operands_take_the_element_wise_path(be, r, dt, mode):
    check(be, r, dt, mode, offset=1)


def test_empty_rows_get_the_own_term(be):
    p, _, _ = pattern()
    _, _, W, _, _, t, _, _, _, _ = case(10, "double", "residual_own")
    empty = np.flatnonzero(np.diff(p) == 0)
    assert empty.size == 5 and empty[0] == 0 and empty[-1] == p.size - 2
    out = run(be, 10, "double", "residual_own")[0].cpu().numpy()
    assert np.array_equal(out[empty], W[empty] * t)
    out = run(be, 10, "double", "plain")[0].cpu().numpy()
    assert np.array_equal(out[empty], np.zeros((5, 10)))


@pytest.mark.parametrize("dt", ["float", "double"])
@pytest.mark.parametrize("r,mode", [(10, "residual_own"), (128, "plain")])
def test_a_column_outside_the_matrix_makes_its_row_nan(be, r, dt, mode):
    p, j, _ = pattern()
    lens = np.diff(p)
    clean, _ = run(be, r, dt, mode)
    victims = [int(np.flatnonzero(lens == 3)[5]), int(np.flatnonzero(lens == SPLIT)[0]), int(np.flatnonzero(lens == LONG)[1])]
    jb = j.copy()
    for k, row in enumerate(victims):
        jb[p[row] + lens[row] // 2] = (N_COLS, -1, 2 ** 31 - 1)[k]
    out, ss = run(be, r, dt, mode, j_override=jb)
    keep = np.ones(lens.size, dtype=bool)
    keep[victims] = False
    keep_t = torch.from_numpy(keep).to(out.device)
    assert torch.isnan(out[~keep_t]).all()
    assert torch.equal(out[keep_t], clean[keep_t])                    # the neighbours keep their bits
    assert torch.isnan(ss).all()
