"""The initial factors drawn on the device (rsparse_amd/csrc/wrmf_init.hip behind rsparse_hip_init_factors_device / _f64_device)
against the numpy definition of the generator (rsparse_amd/rng.py), element by element:

  fp64   |device - replica| <= 1e-15 * scale * max(1, r): both evaluate in double, the libms differ by a few ulp
  fp32   |device - replica| <= 2^-21 * scale * max(1, r), r = the element's Box-Muller radius: twice what <= 1 ulp of logf / sqrtf
         and <= 2 ulp of sincospif add up to; the replica is the double evaluation, not rounded to fp32

over shapes where groups of four straddle rows, ranges that start inside a group, a padded leading dimension, abs, the ones
column, and an element index beyond 2^34 (counter word 1 non-zero); then bit-for-bit determinism across calls, row ranges and
streams, and `WRMF(factor_init="device")` against a "host" model fed the same matrices."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import rel_fro

pytestmark = pytest.mark.gpu

SCALE = 0.01
BOUND = {torch.float32: 2.0 ** -21, torch.float64: 1e-15}


@pytest.fixture(scope="module")
def be():
    from rsparse_amd.engine import HipBackend
    return HipBackend()


def _check(be, dtype, n_rows, rank, row0=0, seed=0x1234567887654321, stream=0, abs_values=False, ones_col=-1, pad=0, scale=SCALE):
    from rsparse_amd.rng import init_factors
    ref, rad = init_factors(seed, stream, row0, n_rows, rank, scale, abs_values, ones_col, return_radius=True)
    if pad:
        buf = torch.full((n_rows, rank + pad), 7.0, dtype=dtype, device=be.device)
        got = be.init_factors(seed, stream, n_rows, rank, dtype, abs_values, ones_col, row0, scale, out=buf[:, :rank])
        torch.cuda.synchronize()
        assert bool((buf[:, rank:] == 7.0).all()), "the padding of ld > rank was written"
    else:
        got = be.init_factors(seed, stream, n_rows, rank, dtype, abs_values, ones_col, row0, scale)
    assert got.dtype == dtype and tuple(got.shape) == (n_rows, rank)
    g = got.cpu().numpy().astype(np.float64)
    lim = BOUND[dtype] * scale * np.maximum(1.0, rad)
    if ones_col >= 0:
        assert np.all(g[:, ones_col] == 1.0)
        lim[:, ones_col] = 0.0
    err = np.abs(g - ref)
    worst = float((err / np.where(lim > 0, lim, 1.0)).max()) if err.size else 0.0
    print("%s %dx%d row0=%d: max error / bound = %.3f" % (str(dtype).split(".")[1], n_rows, rank, row0, worst))
    assert np.all(err <= lim), "max error / bound = %.3f" % worst
    if abs_values:
        assert g.min() >= 0
    return got


CASES = [  # n_rows, rank, options
    (1, 1, {}),                                   # one element of one group
    (3, 5, {}),                                   # groups straddle rows, the range ends inside a group
    (257, 10, {}),                                # more than one workgroup of groups; 2570 % 4 != 0
    (1000, 128, {}),                              # the bench rank: the 16-byte path throughout
    (70, 130, {}),                                # rank % 4 == 2: every other row starts inside a group
    (64, 256, {}),
    (9, 5, {"row0": 7}),                          # e0 = 35: the range STARTS inside a group (element-wise path)
    (40, 8, {"row0": 3}),                         # a shard that starts on a group: the 16-byte path with g0 > 0
    (37, 12, {"pad": 3}),                         # ld = rank + 3: the padding must survive
    (61, 16, {"abs_values": True, "stream": 1}),
    (61, 16, {"ones_col": 0}),
    (61, 16, {"ones_col": 15, "stream": 1}),
    (50, 1, {"pad": 5, "ones_col": 0}),           # a strided column of ones: how a C host sets one column of a wider matrix
    (33, 7, {"ones_col": 6, "abs_values": True}),                 # the ones column on the element-wise path
    (4, 128, {"row0": 140_000_000}),              # e >= 2^34: counter word 1 is non-zero (catches 32-bit index arithmetic)
    (5, 3, {"row0": 1_500_000_000, "stream": 1}),                 # the same on the element-wise path, e0 % 4 != 0
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n_rows,rank,opts", CASES)
def test_device_matches_the_replica(be, dtype, n_rows, rank, opts):
    _check(be, dtype, n_rows, rank, **opts)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_bits_do_not_depend_on_the_call(be, dtype):
    seed = 99
    a = be.init_factors(seed, 1, 257, 10, dtype)
    b = be.init_factors(seed, 1, 257, 10, dtype)
    assert torch.equal(a, b)                                               # two calls
    two = torch.empty((257, 10), dtype=dtype, device=be.device)
    be.init_factors(seed, 1, 100, 10, dtype, out=two[:100])
    be.init_factors(seed, 1, 157, 10, dtype, row0=100, out=two[100:])      # (e0 = 1000: on a group; 2570 ends inside one)
    assert torch.equal(a, two)                                             # two row ranges == one
    odd = torch.empty((257, 10), dtype=dtype, device=be.device)
    be.init_factors(seed, 1, 101, 10, dtype, out=odd[:101])
    be.init_factors(seed, 1, 156, 10, dtype, row0=101, out=odd[101:])      # (e0 = 1010: inside a group)
    assert torch.equal(a, odd)
    flat = torch.empty(257 * 10 + 1, dtype=dtype, device=be.device)         # an output that is not 16-byte aligned: no wide store
    off = be.init_factors(seed, 1, 257, 10, dtype, out=flat[1:].view(257, 10))
    assert off.data_ptr() % 16 != 0 and torch.equal(a, off)
    side = torch.cuda.Stream(device=be.device)
    with torch.cuda.stream(side):                                          # a non-default HIP stream
        c = be.init_factors(seed, 1, 257, 10, dtype)
        d0 = be.init_factors(seed, 1, 100, 10, dtype)
        d1 = be.init_factors(seed, 1, 157, 10, dtype, row0=100)
    side.synchronize()
    assert torch.equal(a, c) and torch.equal(a, torch.cat([d0, d1]))
    assert not torch.equal(a, be.init_factors(seed, 0, 257, 10, dtype))    # the other stream is another matrix
    assert tuple(be.init_factors(seed, 0, 0, 10, dtype).shape) == (0, 10)


CLASS_CASES = [  # feedback, solver, user/item biases, precision, tolerance: the fp32 / fp64 rule of tests/test_wrmf_single.py
    ("implicit", "conjugate_gradient", False, "float", 1e-4),
    ("explicit", "cholesky", True, "double", 1e-9),
]


@pytest.mark.parametrize("feedback,solver,bias,precision,tol", CLASS_CASES)
def test_wrmf_device_init_equals_a_host_fit_fed_the_device_matrices(be, ml_train, feedback, solver, bias, precision, tol):
    from rsparse_amd import WRMF
    n_user, n_item, p, i, x = ml_train
    train = sp.csc_matrix((x, i, p), shape=(n_user, n_item))
    kw = dict(rank=16, lambda_=0.1, feedback=feedback, solver=solver, with_user_item_bias=bias, precision=precision, rng=5)
    dev = WRMF(factor_init="device", **kw)
    emb_d = dev.fit_transform(train, n_iter=3, convergence_tol=-1)
    seed = int(np.random.default_rng(5).integers(2 ** 63))
    k = 16 + (2 if bias else 0)
    tdt = torch.float64 if precision == "double" else torch.float32
    host = WRMF(factor_init="host", **kw)
    host._init_user_factors = be.init_factors(seed, 0, n_user, k, tdt).cpu().numpy()
    if solver != "conjugate_gradient":
        host.components = np.ascontiguousarray(be.init_factors(seed, 1, n_item, k, tdt).cpu().numpy().T)
    emb_h = host.fit_transform(train, n_iter=3, convergence_tol=-1)
    lu = [l[1] for l in dev.losses]
    print("losses (users half): device init %s, host init %s" % (lu, [l[1] for l in host.losses]))
    assert len(lu) == 3 and lu[0] > lu[1] > lu[2]                          # the losses decrease
    assert np.allclose(lu, [l[1] for l in host.losses], rtol=tol, atol=0)
    # (users without ratings start from a 0 / 0 bias under dynamic lambda, in the reference too: with biases the first item-half
    # loss is NaN in both fits, tests/test_wrmf_single.py)
    assert np.allclose([l[0] for l in dev.losses], [l[0] for l in host.losses], rtol=tol, atol=0, equal_nan=True)
    assert emb_d.shape == (n_user, k) and rel_fro(emb_d, emb_h) < tol
    assert rel_fro(dev.components, host.components) < tol
