"""The small C-ABI entries that exist in float and in double and share one host body (csrc/wrmf_capi_common.h), called
directly in both precisions: rsparse_hip_values_subtract_mean[_f64]_device and rsparse_hip_weighted_sumsq[_f64]_device,
against numpy in double, at the lengths where the sums' 1024 partial slots and the two-stage tail meet.

Bounds: those of tests/test_bias.py::test_hip_sweepwise_bias_initialisation_equals_the_fused_one for the same sums -- 1e-12
in double, 2e-6 in float, relative to the size of the operands (at most 1025 terms summed in double: 1025 * 2^-53 = 1.1e-13;
in float one rounding of the stored value, 2^-24 = 6e-8, of each entry)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 1024, 1025]


def _setup(precision):
    import torch
    from rsparse_amd.engine import HipBackend
    be = HipBackend(0)
    if precision == "double":
        return be, torch.float64, np.float64, "_f64", 1e-12
    return be, torch.float32, np.float32, "", 2e-6


@pytest.mark.parametrize("precision", ["float", "double"])
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("n", LENGTHS)
def test_values_subtract_mean(precision, two, n):
    import torch
    be, tdt, dt, f64, eps = _setup(precision)
    rng = np.random.default_rng(n + 17)
    # (one element at n = 0, so that the pointer is not NULL: the entry must leave it alone)
    a = (rng.standard_normal(max(n, 1)) + 3.0).astype(dt)
    b = rng.standard_normal(max(n, 1)).astype(dt)
    da, db = be.to_device(a, tdt), be.to_device(b, tdt)
    mean = ctypes.c_double(-1.0)
    fn = getattr(be.lib, "rsparse_hip_values_subtract_mean%s_device" % f64)
    assert fn(n, da.data_ptr(), db.data_ptr() if two else None, ctypes.byref(mean), be._stream()) == 0
    torch.cuda.synchronize()
    ref = float(a[:n].astype(np.float64).mean()) if n else 0.0
    assert abs(mean.value - ref) <= eps * max(1.0, abs(ref))
    got_a, got_b = da.cpu().numpy().astype(np.float64), db.cpu().numpy().astype(np.float64)
    scale = 1.0 + np.abs(a).max() + abs(ref)
    assert np.abs(got_a[:n] - (a[:n].astype(np.float64) - ref)).max(initial=0.0) <= eps * scale
    want_b = b[:n].astype(np.float64) - ref if two else b[:n].astype(np.float64)
    assert np.abs(got_b[:n] - want_b).max(initial=0.0) <= eps * scale
    assert got_a[n:].tolist() == a[n:].tolist() and got_b[n:].tolist() == b[n:].tolist()   # nothing past n is touched


@pytest.mark.parametrize("precision", ["float", "double"])
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("n", LENGTHS)
def test_weighted_sumsq(precision, weights, n):
    import torch
    be, tdt, dt, f64, eps = _setup(precision)
    rng = np.random.default_rng(n + 5)
    F = rng.standard_normal((max(n, 1), 3)).astype(dt)          # rank 3: n rows of 3 (row-major, as the factors are resident)
    w = (1.0 + rng.integers(0, 9, max(n, 1))).astype(dt)
    dF, dw = be.to_device(F, tdt), be.to_device(w, tdt)
    out = torch.full((1,), -1.0, dtype=torch.float64, device=be.device)
    fn = getattr(be.lib, "rsparse_hip_weighted_sumsq%s_device" % f64)
    assert fn(dF.data_ptr(), 3, n, dw.data_ptr() if weights else None, out.data_ptr(), be._stream()) == 0
    torch.cuda.synchronize()
    sq = (F[:n].astype(np.float64) ** 2).sum(axis=1)
    ref = float((sq * w[:n].astype(np.float64)).sum() if weights else sq.sum())
    assert abs(float(out[0]) - ref) <= eps * max(1.0, abs(ref))
