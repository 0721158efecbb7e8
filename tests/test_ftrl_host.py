"""FTRL on the numpy definition of rsparse_amd/ftrl.py, through the public class on the CPU stand-in backend: the plain per-sample
loop, the dropout mask, a separable problem, dump / load, the argument errors."""
import numpy as np
import pytest
import scipy.sparse as sp

from rsparse_amd import FTRL
from rsparse_amd.fm import canonical_design
from rsparse_amd.ftrl import ftrl_fit_reference, ftrl_keep_reference
from test_metrics_abi import _oracle_metrics_backend


def model(**kw):
    return FTRL(backend=_oracle_metrics_backend(), **kw)


def test_batch_one_is_the_plain_per_sample_loop():
    rng = np.random.default_rng(1)
    m = canonical_design(sp.random(60, 12, density=0.3, random_state=1, format="csr"), np.float64)
    y = rng.normal(size=60)
    alpha, beta, l1, l2 = 0.1, 0.5, 0.08 * 0.25, 0.08 * (1.0 - 0.25)
    z, n = np.zeros(12), np.zeros(12)
    for r in range(60):
        j, x = m.indices[m.indptr[r]:m.indptr[r + 1]], m.data[m.indptr[r]:m.indptr[r + 1]]
        w = np.where(np.abs(z[j]) <= l1, 0.0, (-1.0 / ((beta + np.sqrt(n[j])) / alpha + l2)) * (z[j] - np.sign(z[j]) * l1))
        v = np.zeros(64)
        v[:j.size] = w * x
        for h in (32, 16, 8, 4, 2, 1):
            v = v[:h] + v[h:]
        g = np.minimum(np.maximum((0.0 + v[0] - y[r]) * x, -1000.0), 1000.0)
        sigma = (np.sqrt(n[j] + (0.0 + g * g)) - np.sqrt(n[j])) / alpha
        z[j], n[j] = z[j] + ((0.0 + g) - sigma * w), n[j] + (0.0 + g * g)
    ref = ftrl_fit_reference(m.indptr, m.indices, m.data, y, np.ones(60), np.zeros(12), np.zeros(12), 1, 1, "gaussian", alpha, beta, 0.08, 0.25)
    assert ref[0].tobytes() == z.tobytes() and ref[1].tobytes() == n.tobytes() and np.abs(z).max() > 0


def test_keep_mask_depends_on_seed_epoch_row_and_position_alone():
    ip = np.array([0, 3, 3, 70, 75])
    whole = ftrl_keep_reference(7, 2, ip, np.arange(4), 0.3)
    assert whole.size == 75 and 0.5 < whole.mean() < 0.9
    assert np.array_equal(ftrl_keep_reference(7, 2, ip, np.array([2]), 0.3), whole[3:70])
    assert np.array_equal(ftrl_keep_reference(7, 2, np.array([0, 9, 9, 76]), np.array([2]), 0.3), whole[3:70])
    assert not np.array_equal(ftrl_keep_reference(7, 3, ip, np.arange(4), 0.3), whole)
    assert not np.array_equal(ftrl_keep_reference(8, 2, ip, np.arange(4), 0.3), whole)
    assert ftrl_keep_reference(7, 2, ip, np.arange(4), 0.0).all()


def separable(n=400, d=30, seed=3):
    rng = np.random.default_rng(seed)
    x = sp.random(n, d, density=0.2, random_state=seed, format="csr")
    truth = np.where(np.arange(d) < 5, 3.0 * rng.normal(size=d), 0.0)            # five features carry the signal
    return x, (x @ truth > 0).astype(np.float64)


def test_log_loss_falls_and_l1_thins_the_coefficients():
    x, y = separable()
    m = model(learning_rate=0.5, batch=50, precision="double", rng=1)
    loss = []
    for _ in range(3):
        p = np.clip(m.partial_fit(x, y), 1e-12, 1 - 1e-12)
        loss.append(float(-(y * np.log(p) + (1 - y) * np.log(1 - p)).mean()))
    assert loss[2] < loss[0] and m.epoch == 3, loss
    nz = [int((model(learning_rate=0.5, batch=50, lambda_=lam, l1_ratio=1.0, rng=1).fit(x, y, n_iter=3).coef() != 0).sum()) for lam in (0.0, 5.0)]
    assert nz[1] <= nz[0] and nz[1] < 30, nz


@pytest.mark.parametrize("precision", ["float", "double"])
def test_a_loaded_model_continues_with_the_same_bits(precision):
    x, y = separable(150, 20, 5)
    kw = dict(lambda_=0.01, l1_ratio=0.5, dropout=0.25, batch=64, precision=precision, rng=9)
    two = model(**kw).fit(x, y, n_iter=2)
    one = model(**kw).fit(x, y, n_iter=1)
    again = model().load(one.dump())
    p = again.partial_fit(x, y)
    assert again.z.tobytes() == two.z.tobytes() and again.n.tobytes() == two.n.tobytes() and again.z.dtype == two.z.dtype
    assert (again.seed, again.epoch) == (two.seed, 2) and p.shape == (150,) and again.dump()["dropout"] == 0.25


def test_argument_errors():
    for bad in (dict(batch=0), dict(lambda_=-1.0), dict(lambda_=float("nan")), dict(learning_rate=0.0), dict(learning_rate_decay=-0.1),
                dict(l1_ratio=1.5), dict(dropout=1.0), dict(dropout=-0.1), dict(family="gamma"), dict(precision="half")):
        with pytest.raises(ValueError):
            model(**bad)
    x, y = separable(4, 3, 0)
    m = model()
    with pytest.raises(RuntimeError):
        m.predict(x)
    with pytest.raises(RuntimeError):
        m.coef()
    for args in ((x, y[:3]), (x, [0, 1, 2, 0]), (x, [0, 1, np.nan, 0]), (x, y, [1, 1, 1]), (x, y, [1, 1, -1, 1])):
        with pytest.raises(ValueError):
            m.fit(*args)
    with pytest.raises(ValueError):
        model(family="poisson").fit(x, [1, 2, -1, 0])
    with pytest.raises(ValueError):
        m.fit(x, y, n_iter=-1)
    m.fit(x, y)
    with pytest.raises(ValueError):
        m.partial_fit(sp.csr_matrix(np.ones((4, 5))), y)
    with pytest.raises(ValueError):
        m.predict(sp.csr_matrix(np.ones((4, 5))))
