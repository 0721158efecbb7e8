"""Who owns which rows of the multi-GPU context and where they are stored (rsparse_amd/csrc/wrmf_ctx_layout.h: balanced_edges,
Lay, check_matrix_ptrs), without a device.  The reference is the Python pair engine.balanced_bounds / engine.Layout, which
tests/test_synth_and_engine.py covers on its own: the C++ must give the same edges, Bs, rows, sub_rows, sub_start, slab_start
and the same storage row for every id, over row counts 0 .. 400, 1 .. 8 ranks, 1 .. 40 sub-blocks (40: more than a rank has
rows) and count vectors that leave ranks without rows or put empty rows at both ends and across the cuts.  to_storage must be
a bijection onto storage rows that the sub-blocks own; a padding row is hit by nobody.  The header and
tests/ctx_layout_shim.cpp are compiled with g++ into pytest's temporary directory."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from rsparse_amd import engine

ROOT = Path(__file__).resolve().parent.parent
NS = [0, 1, 7, 400]
WS = [1, 2, 3, 5, 8]
N_SUB = [1, 2, 7, 40]
KINDS = ["uniform", "zero", "half_in_one_row", "empty_ends_and_cuts"]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("ctx_layout") / "libctx_layout_shim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(out), str(ROOT / "tests" / "ctx_layout_shim.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.ctx_layout.restype = None
    lib.ctx_layout.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6
    lib.ctx_check_ptrs.restype = ctypes.c_int
    lib.ctx_check_ptrs.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_char_p, ctypes.c_int]
    return lib


def counts_of(kind, n, ws):
    """non-zeros per row: the same everywhere / none / one row with half of all entries (its neighbours' ranks own nothing) /
    empty rows first, last and within two rows of every cut of an even split"""
    c = np.full(n, 3, dtype=np.int64)
    if kind == "zero":
        c[:] = 0
    elif kind == "half_in_one_row" and n:
        c[n // 3] = max(3, 3 * (n - 1))
    elif kind == "empty_ends_and_cuts" and n:
        c[:2] = 0
        c[-2:] = 0
        for r in range(1, ws):
            m = n * r // ws
            c[max(0, m - 2):m + 3] = 0
    return c


def cpp_layout(lib, counts, ws, n_sub):
    n = len(counts)
    p = np.zeros(n + 1, dtype=np.int32)
    p[1:] = np.cumsum(counts)
    edges = np.full(ws + 1, -1, dtype=np.int64)
    scal = np.full(4, -1, dtype=np.int64)
    sub_rows = np.full((ws, n_sub, 2), -1, dtype=np.int64)
    sub_start = np.full((ws, n_sub), -1, dtype=np.int64)
    slab_start = np.full(n_sub, -1, dtype=np.int64)
    storage = np.full(max(n, 1), -1, dtype=np.int64)
    lib.ctx_layout(p.ctypes.data, n, ws, n_sub, *[a.ctypes.data for a in (edges, scal, sub_rows, sub_start, slab_start, storage)])
    return edges, scal, sub_rows, sub_start, slab_start, storage[:n]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ws", WS)
@pytest.mark.parametrize("n", NS)
def test_cpp_layout_is_the_python_layout(shim, n, ws, kind):
    counts = counts_of(kind, n, ws)
    bounds = engine.balanced_bounds(counts, ws)
    if kind == "half_in_one_row" and n >= 7 and ws >= 5:     # (two or more of the targets fall inside the one row)
        assert any(b == a for a, b in bounds)          # the premise: some rank owns nothing
    for n_sub in N_SUB:
        lay = engine.Layout(n, bounds, n_sub)
        edges, scal, sub_rows, sub_start, slab_start, storage = cpp_layout(shim, counts, ws, n_sub)
        tag = (n, ws, n_sub, kind)
        assert edges.tolist() == [a for a, _ in bounds] + [n], tag
        assert scal.tolist() == [lay.Bs, lay.rows, ws, n_sub], tag
        for r in range(ws):
            for j in range(n_sub):
                assert tuple(sub_rows[r, j]) == lay.sub_rows(r, j), tag + (r, j)
                assert sub_start[r, j] == lay.sub_start(r, j), tag + (r, j)
        assert slab_start.tolist() == [lay.slab(j)[0] for j in range(n_sub)], tag
        # (ids as int64 and NOT through Layout's identity shortcut only: at ws = n_sub = 1 both must be the identity)
        ref = lay.to_storage(torch.arange(n, dtype=torch.int64)).numpy()
        assert np.array_equal(storage, ref), tag
        # a bijection onto rows that a sub-block owns: the union of [sub_start, sub_start + c1 - c0) over (r, j), nothing else
        owned = np.zeros(lay.rows, dtype=np.int64)
        for r in range(ws):
            for j in range(n_sub):
                c0, c1 = sub_rows[r, j]
                assert 0 <= c0 <= c1 <= c0 + lay.Bs, tag
                owned[sub_start[r, j]:sub_start[r, j] + (c1 - c0)] += 1
        assert owned.max(initial=0) <= 1 and owned.sum() == n, tag
        hit = np.bincount(storage, minlength=lay.rows) if n else np.zeros(lay.rows, dtype=np.int64)
        assert hit.size == lay.rows and np.array_equal(hit, owned), tag          # every owned row once, no padding row
        # the owner's block order is kept: the ids of (r, j) are consecutive from edges[r] + c0
        for r in range(ws):
            for j in range(n_sub):
                c0, c1 = sub_rows[r, j]
                ids = np.arange(edges[r] + c0, edges[r] + c1)
                assert np.array_equal(storage[ids], sub_start[r, j] + np.arange(c1 - c0)), tag + (r, j)


def _check(lib, ui_p, iu_p):
    ui_p, iu_p = np.asarray(ui_p, dtype=np.int32), np.asarray(iu_p, dtype=np.int32)
    msg = ctypes.create_string_buffer(256)
    rc = lib.ctx_check_ptrs(ui_p.ctypes.data, len(ui_p) - 1, iu_p.ctypes.data, len(iu_p) - 1, msg, 256)
    return rc, msg.value.decode()


def test_pointer_check(shim):
    good_ui, good_iu = [0, 2, 2, 5], [0, 1, 4, 5, 5]
    assert _check(shim, good_ui, good_iu) == (0, "")
    assert _check(shim, [0], [0]) == (0, "")                      # no items, no users
    assert _check(shim, [0, 0, 0], [0]) == (0, "")                # items without users
    assert _check(shim, [0], [0, 0]) == (0, "")
    assert _check(shim, [0, 0, 0], [0, 0, 0, 0]) == (0, "")       # an empty matrix
    rc, msg = _check(shim, [1, 2, 2, 5], good_iu)
    assert rc == 1 and "ui_p" in msg and "start at 0" in msg
    rc, msg = _check(shim, good_ui, [1, 1, 4, 5, 5])
    assert rc == 1 and "iu_p" in msg and "start at 0" in msg
    rc, msg = _check(shim, [0, 3, 2, 5], good_iu)
    assert rc == 1 and "ui_p decreases at column 1" in msg
    rc, msg = _check(shim, good_ui, [0, 1, 4, 3, 5])
    assert rc == 1 and "iu_p decreases at column 2" in msg
    rc, msg = _check(shim, [0, 3, 2, 2], [0, 1, 2])              # (a decreasing pair whose total would still match)
    assert rc == 1 and "ui_p decreases" in msg
    rc, msg = _check(shim, good_ui, [0, 1, 4, 4, 4])
    assert rc == 1 and "different numbers of non-zeros" in msg
    rc, msg = _check(shim, [-1, 2], [0, 2])
    assert rc == 1 and "ui_p" in msg
