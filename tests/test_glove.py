"""GloVe on the device (wrmf_glove.hip behind rsparse_hip_glove_*_device / rsparse_hip_glove_fit) against the numpy definition of
rsparse_amd/glove.py, bit for bit in both precisions: one step at every segment-length edge of both sides, whole fits through the
public class, the host-array form, the rank limit."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import GloVe, _lib
from rsparse_amd import rng as prng
from rsparse_amd.bpr import step_slots
from rsparse_amd.glove import cooccurrence_slots, glove_fit_reference, glove_slots_reference, glove_step_reference
from test_bpr import DTYPES, TORCH, backend, bits_equal

pytestmark = pytest.mark.gpu

N, X_MAX, ALPHA = 8400, 10.0, 0.75
EDGES = {0, 1, 2, 63, 64, 65, 64 * 64 + 1}


@functools.lru_cache(maxsize=None)
def step_matrix():
    """8400 x 8400 whose rows hold PAIRS of adjacent columns (2 j, 2 j + 1), so every row starts at an even position and the odd
    columns are exactly step 1 of 2.  In pairs: row 0 holds 4097, row 1 none, rows 5000 .. 5004 hold 1, 2, 63, 64, 65; pair 4199 is in
    4097 rows, pairs 4170 .. 4174 in 1, 2, 63, 64, 65 rows; row 6001 holds pair 3000, whose odd column is the diagonal."""
    inc = [(0, j) for j in range(4097)] + [(r, 4199) for r in range(100, 4197)] + [(6001, 3000)]
    for t, cnt in enumerate((1, 2, 63, 64, 65)):
        inc += [(5000 + t, 4100 + j) for j in range(cnt)] + [(6000 + i, 4170 + t) for i in range(cnt)]
    r, j = np.array(inc).T
    rng = np.random.default_rng(5)
    val = rng.uniform(1.0, 30.0, size=2 * r.size)                                    # both sides of x_max
    return sp.csr_matrix((val, (np.repeat(r, 2), np.stack([2 * j, 2 * j + 1], axis=1).reshape(-1))), shape=(N, N))


def start_state(n, rank, dt, rng):
    W = [(0.3 * rng.normal(size=(n, rank))).astype(dt) for _ in range(2)]
    b = [rng.normal(size=n).astype(dt) for _ in range(2)]
    return (*W, *b, 1.0 + rng.random((n, rank)), 1.0 + rng.random((n, rank)), 1.0 + rng.random(n), 1.0 + rng.random(n))


def device(arrays):
    return [backend().to_device(a, torch.int32 if a.dtype == np.int32 else TORCH[a.dtype.type]) for a in arrays]


@pytest.mark.parametrize("rank", [1, 16, 17, 128])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_step_equals_the_definition(precision, rank):
    dt, rng = DTYPES[precision], np.random.default_rng(rank + 1)
    rows, cols, fx, lx, n = cooccurrence_slots(step_matrix(), dt, X_MAX, ALPHA)
    slots = step_slots(rows.size, 1, 2)
    r, c = rows[slots], cols[slots]
    assert EDGES <= set(np.bincount(r, minlength=n)) and EDGES <= set(np.bincount(c, minlength=n))
    assert (r == c).any() and (fx[slots] == 1).any() and (fx[slots] < 1).any() and 1 not in r and 0 not in c
    start = start_state(n, rank, dt, rng)
    start[2][5000], start[2][5001] = 300.0, -300.0                                   # b_i: the clip at +100 and at -100
    inner = glove_slots_reference(rows, cols, fx, lx, slots, *start[:4])[0]
    assert (inner == 100.0).any() and (inner == -100.0).any() and (np.abs(inner) < 100.0).any()
    pos, index = device((rows, cols, fx, lx)), None
    for lam in (0.0, 0.05):
        ref = glove_step_reference(rows, cols, fx, lx, slots, *start, 0.15, lam)
        dev = device(start)
        index = index or backend().glove_index(pos[0], pos[1], n, 2)
        term = backend().glove_step(*pos, index, 1, *dev, 0.15, lam)
        assert all(bits_equal(g.cpu().numpy(), e) for g, e in zip(dev, ref[:8]))
        assert term.cpu().numpy()[0] == ref[8]
        assert all(bits_equal(ref[t][1], start[t][1]) for t in (0, 2, 4, 6)) and all(bits_equal(ref[t][0], start[t][0]) for t in (1, 3, 5, 7))
        assert not bits_equal(ref[0][0], start[0][0]) and not bits_equal(ref[1][1], start[1][1])


@pytest.mark.parametrize("batch", [1024, 334])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_fit_equals_the_definition(precision, batch):
    dt = DTYPES[precision]
    x = sp.random(300, 300, density=0.05, random_state=4, format="csr") * 20.0
    kw = dict(rank=17, x_max=X_MAX, batch=batch, lambda_=0.01, precision=precision, rng=6)
    a, b = GloVe(**kw), GloVe(**kw)
    ea, eb = a.fit_transform(x, n_iter=3), b.fit_transform(x, n_iter=3)
    rows, cols, fx, lx, n = cooccurrence_slots(x, dt, X_MAX, ALPHA)
    W0 = [backend().init_factors(a.seed, s, 300, 17, TORCH[dt], scale=0.1).cpu().numpy()          # (the device's draw, as the model took it)
          for s in (prng.STREAM_USERS, prng.STREAM_ITEMS)]
    ref = glove_fit_reference(rows, cols, fx, lx, *W0, np.zeros(300, dt), np.zeros(300, dt), np.ones((300, 17)), np.ones((300, 17)),
                              np.ones(300), np.ones(300), 3, batch, 0.15, 0.01)
    for got, emb in ((a, ea), (b, eb)):
        fit = (emb, got.components.T, got.bias_i, got.bias_j, got.adagrad_w_i.T, got.adagrad_w_j.T, got.adagrad_b_i, got.adagrad_b_j)
        assert all(bits_equal(g, e) for g, e in zip(fit, ref[:8]))
        assert got.cost_history == [t / rows.size for t in ref[8]] and got.seed == a.seed
    E = (ref[0] + ref[1]).astype(np.float64)
    E /= np.sqrt((E * E).sum(axis=1))[:, None]
    ids = np.array([0, 7, 299])
    cos = E[ids] @ E.T
    cos[np.arange(3), ids] = -np.inf
    assert np.array_equal(a.most_similar(ids, k=5)[0], np.argsort(-cos, axis=1)[:, :5])


def test_host_array_form_equals_the_definition():
    rng = np.random.default_rng(12)
    rows, cols, fx, lx, n = cooccurrence_slots(sp.random(300, 300, density=0.05, random_state=2, format="csr") * 20.0, np.float64, X_MAX, ALPHA)
    start = start_state(n, 5, np.float64, rng)
    ref = glove_fit_reference(rows, cols, fx, lx, *start, 2, 1000, 0.15, 0.02)
    got, trace = [np.array(a) for a in start], np.zeros(2)
    ptr = lambda a: a.ctypes.data
    _lib.check(_lib.load().rsparse_hip_glove_fit(ptr(rows), ptr(cols), ptr(fx), ptr(lx), n, rows.size, 2, 1000, 5, 0.15, 0.02,
                                                 *(ptr(a) for a in got), ptr(trace)))
    assert all(bits_equal(g, e) for g, e in zip(got, ref[:8])) and trace.tolist() == ref[8]


def test_rank_129_is_unsupported():
    with pytest.raises(_lib.UnsupportedOnDevice):
        GloVe(rank=129, x_max=X_MAX)
    rows, cols, fx, lx, n = cooccurrence_slots(sp.csr_matrix(np.ones((4, 4))), np.float32, X_MAX, ALPHA)
    pos = device((rows, cols, fx, lx))
    index = backend().glove_index(pos[0], pos[1], n, 1)
    with pytest.raises(_lib.UnsupportedOnDevice):
        backend().glove_step(*pos, index, 0, *device(start_state(n, 129, np.float32, np.random.default_rng(0))), 0.15, 0.0)
