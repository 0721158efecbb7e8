"""`WRMF(factor_init="device")` without a GPU: the generator's definition (rsparse_amd/rng.py: Philox4x32-10 known answers, row-range
independence, moments), the argument checks of the two C-ABI entries (status codes before a device is touched), and the class's
control flow on the CPU stand-in backend (tests/oracle_backend.py), which has no `init_factors` and so gets the numpy replica:
streams, scale, abs, ones columns, the CG-zeros rule, reproducibility through `rng=`, and the sharded path's broadcast seed."""
import ctypes
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import rel_fro

ROOT = Path(__file__).resolve().parent.parent


def test_philox4x32_10_known_answers():
    """the Random123 known-answer vectors of philox4x32_10"""
    from rsparse_amd.rng import philox4x32_10
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        got = philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert got.dtype == np.uint32 and " ".join("%08x" % v for v in got) == want
    # vectorised over a leading axis, the key broadcast
    both = philox4x32_10(np.array([kat[0][0], kat[0][0]], dtype=np.uint64), np.array(kat[0][1], dtype=np.uint64))
    assert both.shape == (2, 4) and np.array_equal(both[0], both[1])


def test_a_value_does_not_depend_on_the_row_range():
    from rsparse_amd.rng import init_factors
    whole = init_factors(3, 0, 0, 257, 10)
    parts = np.vstack([init_factors(3, 0, 0, 100, 10), init_factors(3, 0, 100, 157, 10)])
    assert whole.shape == (257, 10) and np.array_equal(whole, parts)
    assert np.array_equal(init_factors(3, 0, 7, 5, 5), init_factors(3, 0, 0, 12, 5)[7:])       # a range that starts inside a group
    assert not np.array_equal(init_factors(3, 0, 0, 257, 10), init_factors(3, 1, 0, 257, 10))  # the streams differ
    assert not np.array_equal(init_factors(3, 0, 0, 257, 10), init_factors(4, 0, 0, 257, 10))  # the seeds differ
    assert init_factors(3, 0, 0, 4, 8)[1, 0] != init_factors(3, 0, 0, 4, 4)[1, 0]              # `rank` places (row, col) in the stream
    assert init_factors(3, 0, 5, 0, 10).shape == (0, 10)
    # the options: scale, abs, the ones column, the element type
    a = init_factors(9, 1, 0, 33, 7, scale=0.5)
    assert np.allclose(a, 50.0 * init_factors(9, 1, 0, 33, 7), rtol=1e-14, atol=0)
    assert np.array_equal(init_factors(9, 1, 0, 33, 7, abs_values=True), np.abs(init_factors(9, 1, 0, 33, 7)))
    o = init_factors(9, 1, 0, 33, 7, ones_col=6)
    assert np.all(o[:, 6] == 1.0) and np.array_equal(o[:, :6], init_factors(9, 1, 0, 33, 7)[:, :6])
    assert init_factors(9, 1, 0, 33, 7, dtype=np.float32).dtype == np.float32
    for bad in (dict(stream=2), dict(rank=0), dict(n_rows=-1), dict(row0=-1), dict(ones_col=7), dict(ones_col=-2)):
        kw = dict(seed=1, stream=0, row0=0, n_rows=3, rank=7)
        kw.update(bad)
        with pytest.raises(ValueError):
            init_factors(**kw)


def test_moments_of_the_normals():
    """seed 7, stream 1, 4096 x 128: N = 524288 numbers, every bound 5 standard errors of its statistic under N(0, 1)"""
    from rsparse_amd.rng import init_factors
    z = init_factors(7, 1, 0, 4096, 128) / 0.01
    N = z.size
    assert N == 524288
    mean, var = z.mean(), z.var()
    m4 = (z ** 4).mean()
    corr = np.corrcoef(z[:, 0], z[:, 1])[0, 1]
    print("mean %.4f  var - 1 %.4f  m4 - 3 %.4f  corr %.4f  max |z| %.3f" % (mean, var - 1, m4 - 3, corr, np.abs(z).max()))
    assert abs(mean) <= 5 / np.sqrt(N)                 # 0.0069
    assert abs(var - 1) <= 5 * np.sqrt(2 / N)          # 0.0098
    assert abs(m4 - 3) <= 5 * np.sqrt(96 / N)          # 0.068
    assert abs(corr) <= 5 / np.sqrt(4096)              # 0.078
    assert np.abs(z).max() <= np.sqrt(48 * np.log(2))  # 5.77: u_a >= 2^-24
    assert not np.any(z == 0)


def _call(lib, name, seed=1, stream=0, row0=0, n_rows=4, rank=8, ld=8, scale=0.01, abs_values=0, ones_col=-1, out=0x1000):
    return getattr(lib, name)(seed, stream, row0, n_rows, rank, ld, scale, abs_values, ones_col, out, None)


@pytest.mark.parametrize("name", ["rsparse_hip_init_factors_device", "rsparse_hip_init_factors_f64_device"])
def test_status_codes_without_device(name):
    """every bad argument is answered with ERR_INVALID before any device call (there is no device here, and the made-up
    pointer is never used); n_rows == 0 is OK and launches nothing"""
    from rsparse_amd import _lib
    lib = _lib.load()
    for bad in (dict(n_rows=-1), dict(row0=-1), dict(rank=0), dict(rank=-3), dict(ld=7), dict(stream=-1), dict(stream=2),
                dict(ones_col=-2), dict(ones_col=8), dict(out=None), dict(row0=2 ** 62, rank=8)):
        assert _call(lib, name, **bad) == _lib.ERR_INVALID, bad
        assert lib.rsparse_hip_last_error()
    assert _call(lib, name, n_rows=0) == _lib.OK
    assert _call(lib, name, n_rows=0, out=None) == _lib.OK
    assert _call(lib, name, n_rows=0, row0=140_000_000, rank=1000, ld=1000, ones_col=999, stream=1) == _lib.OK   # no rank ceiling


# ---- the class on the CPU stand-in ------------------------------------------------------------------------------------------

def _problem(seed=11, n_user=173, n_item=59):
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.lognormal(1.5, 1.0, n_user).astype(int), 0, 40)
    rows = np.repeat(np.arange(n_user), lens)
    cols = np.concatenate([rng.choice(n_item, size=l, replace=False) for l in lens])
    vals = 1.0 + rng.geometric(0.5, size=rows.size)
    return sp.csr_matrix((vals, (rows, cols)), shape=(n_user, n_item))


def test_factor_init_is_validated():
    from rsparse_amd import WRMF
    with pytest.raises(ValueError):
        WRMF(factor_init="bogus")
    assert WRMF()._factor_init == "host" and WRMF(factor_init="device")._factor_init == "device"


VARIANTS = [  # feedback, solver, user/item biases
    ("implicit", "cholesky", False),
    ("implicit", "conjugate_gradient", False),
    ("implicit", "nnls", False),
    ("explicit", "cholesky", True),
]


def _model(feedback, solver, bias, factor_init, rng, precision="double"):
    from oracle_backend import OracleBackend
    from rsparse_amd import WRMF
    return WRMF(rank=6, lambda_=0.1, feedback=feedback, solver=solver, with_user_item_bias=bias, precision=precision,
                backend=OracleBackend(), rng=rng, factor_init=factor_init)


@pytest.mark.parametrize("feedback,solver,bias", VARIANTS)
def test_device_fit_equals_a_host_fit_given_the_replicas_matrices(feedback, solver, bias):
    """pins what the "device" path draws: one seed = rng.integers(2**63), users from stream 0 and items from stream 1 at scale
    0.01, both in the device dtype; and that the rules of the host draw hold (abs for NNLS, the two columns of ones, items from
    zeros under conjugate gradient): the "host" model applies them itself to the plain replica matrices it is handed"""
    from rsparse_amd.rng import init_factors
    m = _problem()
    k = 6 + (2 if bias else 0)
    dev = _model(feedback, solver, bias, "device", 42)
    emb_d = dev.fit_transform(m, n_iter=3, convergence_tol=-1)
    seed = int(np.random.default_rng(42).integers(2 ** 63))
    host = _model(feedback, solver, bias, "host", 42)
    host._init_user_factors = init_factors(seed, 0, 0, m.shape[0], k)
    if solver != "conjugate_gradient":
        host.components = np.ascontiguousarray(init_factors(seed, 1, 0, m.shape[1], k).T)
    emb_h = host.fit_transform(m, n_iter=3, convergence_tol=-1)
    assert len(dev.losses) == 3 and np.array_equal(np.array(dev.losses), np.array(host.losses), equal_nan=True)
    assert np.array_equal(dev.components, host.components)
    assert np.array_equal(emb_d, emb_h)
    if solver == "nnls":
        assert dev.components.min() >= 0 and emb_d.min() >= 0


def test_device_fit_is_reproducible_through_rng():
    m = _problem()
    fits = []
    for rng in (5, 5, 6):
        model = _model("implicit", "cholesky", False, "device", rng, precision="float")
        fits.append((model.fit_transform(m, n_iter=2, convergence_tol=-1), model.components))
    assert np.array_equal(fits[0][0], fits[1][0]) and np.array_equal(fits[0][1], fits[1][1])
    assert not np.array_equal(fits[0][0], fits[2][0]) and rel_fro(fits[0][1], fits[2][1]) > 1e-6


def test_given_matrices_still_replace_the_draws():
    """`_init_user_factors` replaces the user draw and `init` the item draw under "device" as under "host" """
    m = _problem()
    rng = np.random.default_rng(8)
    U0 = (rng.standard_normal((m.shape[0], 6)) * 0.01)
    V0 = (rng.standard_normal((6, m.shape[1])) * 0.01)
    out = []
    for fi in ("host", "device"):
        from oracle_backend import OracleBackend
        from rsparse_amd import WRMF
        model = WRMF(rank=6, lambda_=0.1, solver="cholesky", precision="double", backend=OracleBackend(), rng=1, init=V0.copy(),
                     factor_init=fi)
        model._init_user_factors = U0
        out.append((model.fit_transform(m, n_iter=2, convergence_tol=-1), model.components))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    bad = _model("implicit", "cholesky", False, "device", 1)
    bad._init_user_factors = U0[:, :5]
    with pytest.raises(ValueError):
        bad.fit_transform(m, n_iter=1)


# ---- sharded, gloo, world size 2 (in the style of tests/test_wrmf_sharded.py) -------------------------------------------------

def _sharded_problem():
    rng = np.random.default_rng(11)
    n_user, n_item = 211, 67
    lens = np.clip(rng.lognormal(1.5, 1.0, n_user).astype(int), 0, 50)
    rows = np.repeat(np.arange(n_user), lens)
    cols = np.concatenate([rng.choice(n_item, size=l, replace=False) for l in lens])
    vals = 1.0 + rng.geometric(0.5, size=rows.size)
    return sp.csr_matrix((vals, (rows, cols)), shape=(n_user, n_item))


def _sharded_fit(solver, rng):
    from oracle_backend import OracleBackend
    from rsparse_amd import WRMF
    m = _sharded_problem()
    model = WRMF(rank=8, lambda_=0.1, feedback="implicit", solver=solver, precision="float", backend=OracleBackend(), rng=rng,
                 factor_init="device")
    emb = model.fit_transform(m, n_iter=3, convergence_tol=-1)
    return {"emb": emb, "components": model.components, "losses": model.losses}


def _worker(rank, ws, port, solver, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT / "tests"))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        torch.save(_sharded_fit(solver, 100 + rank), os.path.join(out_dir, "d%d.pt" % rank))   # (differently seeded ranks)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("solver", ["conjugate_gradient", "cholesky", "nnls"])
def test_two_ranks_draw_the_same_factors_from_rank_zeros_seed(tmp_path, solver):
    """the ranks are seeded differently: rank 0's seed travels (8 bytes), every rank generates the replicated factors itself,
    and the fit agrees with the one-rank fit of rank 0's seed (tolerances: tests/test_wrmf_sharded.py)"""
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, solver, str(tmp_path)), nprocs=2, join=True)
    rs = [torch.load(tmp_path / ("d%d.pt" % r), weights_only=False) for r in range(2)]
    for key in ("emb", "components"):
        assert np.array_equal(rs[0][key], rs[1][key]), key
    assert rs[0]["losses"] == rs[1]["losses"]
    one = _sharded_fit(solver, 100)
    tol = 2e-3 if solver == "nnls" else 5e-5
    assert rel_fro(rs[0]["components"], one["components"]) < tol
    assert rel_fro(rs[0]["emb"], one["emb"]) < tol
    assert np.allclose([l[1] for l in rs[0]["losses"]], [l[1] for l in one["losses"]], rtol=tol)
    other = _sharded_fit(solver, 101)                       # rank 1's own seed would have given another fit
    assert rel_fro(other["components"], one["components"]) > 10 * tol
