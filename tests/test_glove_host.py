"""GloVe on the numpy definition of rsparse_amd/glove.py, through the public class on the CPU stand-in backend: batch = 1 against a
plain per-entry loop, the MovieLens item co-occurrence, the symmetrisation of a triangular input, the rejected values."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from rsparse_amd import GloVe
from rsparse_amd import rng as prng
from rsparse_amd.glove import cooccurrence_slots
from test_metrics_abi import _oracle_metrics_backend


def model(**kw):
    return GloVe(backend=_oracle_metrics_backend(), **kw)


def fitted(m):
    return [np.asarray(t).tobytes() for t in (m.components, m.bias_i, m.bias_j, m.adagrad_w_i, m.adagrad_w_j, m.adagrad_b_i, m.adagrad_b_j)] \
        + [list(m.cost_history)]


def cooccurrence(n, density, seed):
    """a symmetric n x n matrix of positive counts with a diagonal"""
    a = sp.random(n, n, density=density, random_state=seed, format="csr")
    a.data = np.ceil(a.data * 30)
    return sp.csr_matrix(sp.triu(a, 0) + sp.triu(a, 1).T)


@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_one_is_the_per_entry_loop(precision):
    dt = np.float32 if precision == "float" else np.float64
    x, rank, lr, lam, x_max, alpha = cooccurrence(12, 0.4, 1), 3, 0.15, 0.02, 10.0, 0.75
    m = model(rank=rank, x_max=x_max, learning_rate=lr, alpha=alpha, lambda_=lam, batch=1, precision=precision, rng=3)
    got = m.fit_transform(x, n_iter=2)
    rows, cols, fx, lx, n = cooccurrence_slots(x, dt, x_max, alpha)
    W = [prng.init_factors(m.seed, s, 0, n, rank, 0.1, dtype=dt) for s in (prng.STREAM_USERS, prng.STREAM_ITEMS)]
    b, aW, ab = [np.zeros(n, dt), np.zeros(n, dt)], [np.ones((n, rank)), np.ones((n, rank))], [np.ones(n), np.ones(n)]
    history = []

    def adagrad(theta, a, g):
        a2 = a + g * g
        return dt(float(theta) - (lr * g) / math.sqrt(a2)), a2

    for _ in range(2):
        total = 0.0
        for p in range(rows.size):
            r, c = int(rows[p]), int(cols[p])
            wi, wj = [float(v) for v in W[0][r]], [float(v) for v in W[1][c]]
            dot = (wi[0] * wj[0] + wi[2] * wj[2]) + wi[1] * wj[1]            # 16 partials of at most one product, then the tree
            inner = min(max(((dot + float(b[0][r])) + float(b[1][c])) - float(lx[p]), -100.0), 100.0)
            cost = float(fx[p]) * inner
            total = total + 0.5 * (cost * inner)
            for side, at, own, other in ((0, r, wi, wj), (1, c, wj, wi)):
                for q in range(rank):
                    W[side][at, q], aW[side][at, q] = adagrad(own[q], aW[side][at, q], cost * other[q] + (lam * 1.0) * own[q])
                b[side][at], ab[side][at] = adagrad(b[side][at], ab[side][at], cost)
        history.append(total / rows.size)
    assert fitted(m) == [t.tobytes() for t in (W[1].T.copy(), b[0], b[1], aW[0].T.copy(), aW[1].T.copy(), ab[0], ab[1])] + [history]
    assert got.tobytes() == W[0].tobytes() and got.shape == (12, rank) and m.get_history()["cost_history"] == history


def test_movielens_cooccurrence_cost_falls(movielens):
    n_user, n_item, p, i, x = movielens
    items = sp.csc_matrix((x, i, p), shape=(n_user, n_item))[:, :200]
    m = model(rank=8, x_max=10.0, learning_rate=0.15, batch=4096, rng=1)
    emb = m.fit_transform((items.T @ items).tocsr(), n_iter=5)
    assert emb.shape == (200, 8) and m.components.shape == (8, 200) and len(m.cost_history) == 5
    assert np.isfinite(m.cost_history).all() and m.cost_history[-1] < m.cost_history[0], m.cost_history
    idx, cos = m.most_similar([0, 5], k=4)
    assert idx.shape == (2, 4) and (idx != np.array([[0], [5]])).all() and (np.diff(cos, axis=1) <= 0).all()


def test_a_triangular_input_is_symmetrised():
    full = cooccurrence(30, 0.2, 2)
    kw = dict(rank=5, x_max=10.0, batch=64, lambda_=0.01, rng=4)
    a, b, c = model(**kw), model(**kw), model(**kw)
    ea, eb, ec = a.fit_transform(full, n_iter=2), b.fit_transform(sp.triu(full, 0), n_iter=2), c.fit_transform(sp.tril(full, 0), n_iter=2)
    assert fitted(a) == fitted(b) == fitted(c) and ea.tobytes() == eb.tobytes() == ec.tobytes()


def test_rejected_arguments():
    x = cooccurrence(8, 0.5, 3).tolil()
    for bad in (0.0, -1.0, np.nan, np.inf):
        y = x.copy().tocsr()
        y.data[1] = bad
        with pytest.raises(ValueError):
            model(rank=2, x_max=10.0).fit_transform(y)
    with pytest.raises(ValueError):
        model(rank=2, x_max=10.0).fit_transform(sp.csr_matrix(np.ones((3, 4))))
    for kw in (dict(rank=0), dict(x_max=0.0), dict(learning_rate=0.0), dict(lambda_=-1.0), dict(batch=0), dict(precision="half"),
               dict(init={"w": None})):
        with pytest.raises(ValueError):
            GloVe(**{"rank": 2, "x_max": 10.0, **kw})
    with pytest.raises(ValueError):
        model(rank=2, x_max=10.0, init={"w_i": np.zeros((2, 7))}).fit_transform(x.tocsr())
