"""The blocked symmetric sweep without a device: the numpy definition against a Cholesky inverse, its failure cases, and the argument
checks of the C entry."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from rsparse_amd import EASE, _lib
from rsparse_amd.ease import spd_sweep_reference

HEADER = (Path(__file__).resolve().parent.parent / "include" / "rsparse_wrmf_hip.h").read_text()


def ridge_gram(n, lambda_, seed=0):
    h = (np.random.default_rng(seed + n).random((3 * n + 5, n)) < 0.2).astype(np.float64)
    return h.T @ h + lambda_ * np.eye(n)


def residual(P, A):
    return np.abs(P @ A - np.eye(A.shape[0])).max()


@pytest.mark.parametrize("lambda_", [0.01, 500.0])
@pytest.mark.parametrize("n", [1, 5, 64, 65, 150])
@pytest.mark.parametrize("block", [1, 7, 64])
def test_reference_is_as_accurate_as_a_cholesky_inverse(block, n, lambda_):
    """max |P A - I| within 4 x that of scipy's cho_solve on the same input (of np.linalg.inv without scipy's)"""
    A = ridge_gram(n, lambda_)
    try:
        from scipy.linalg import cho_factor, cho_solve
        P_ref = cho_solve(cho_factor(A), np.eye(n))
    except ImportError:
        P_ref = np.linalg.inv(A)
    P = spd_sweep_reference(A, block=block)
    print("n %d block %d lambda %g: sweep %.3g, yardstick %.3g" % (n, block, lambda_, residual(P, A), residual(P_ref, A)))
    assert residual(P, A) <= 4 * residual(P_ref, A)


@pytest.mark.parametrize("A", [-np.eye(5), np.zeros((3, 3))], ids=["minus_identity", "zeros"])
def test_reference_reports_a_matrix_that_is_not_positive_definite(A):
    with pytest.raises(_lib.RsparseHipError) as e:
        spd_sweep_reference(A)
    assert e.value.code == _lib.ERR_NUMERIC


def test_entry_checks_its_arguments_without_a_device():
    lib = _lib.load()
    a = np.eye(4)
    p = a.ctypes.data_as(ctypes.c_void_p)
    call = lib.rsparse_hip_spd_inverse_f64_device
    assert call(None, 4, 4, None) == _lib.ERR_INVALID
    assert call(p, -1, 4, None) == _lib.ERR_INVALID
    assert call(p, 4, 3, None) == _lib.ERR_INVALID
    assert call(p, 0, 0, None) == _lib.OK
    decl = re.search(r"int rsparse_hip_spd_inverse_f64_device\(([^)]*)\);", HEADER).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["rsparse_hip_spd_inverse_f64_device"][1]) == 4
    assert int(re.search(r"#define RSPARSE_HIP_SPDINV_BLOCK (\d+)", HEADER).group(1)) == _lib.SPDINV_BLOCK


def test_unknown_inverse_is_a_value_error():
    with pytest.raises(ValueError):
        EASE(inverse="nonsense")
    assert EASE(inverse="sweep")._inverse == "sweep" and EASE()._inverse == "torch"
