"""Grid, visits and loss slots of the short-row launches of rsparse_amd/csrc/wrmf_cgp.hip (rsparse_amd/csrc/wrmf_schedule.cpp:
cgp_grid / cgp_visits / cgp_loss_slots), without a device.  A workgroup is 4 waves; visit v of wave w (numbered over the whole
grid) takes rows [(w + v * waves) * R, + R) of the launch's list, R = 4 in the four-rows-per-wave form and 2 otherwise.  Every
row must be taken exactly once, and the launch owns one loss slot per wave: a launcher and a slot count that disagree write
outside the loss partials.  The planner and tests/cgp_quad_shim.cpp are compiled with g++ into pytest's temporary directory."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
ROW_COUNTS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 8191, 8192, 8193, 2_700_000]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("cgp_quad") / "libcgp_quad_shim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(out),
                           str(ROOT / "rsparse_amd" / "csrc" / "wrmf_schedule.cpp"), str(ROOT / "tests" / "cgp_quad_shim.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.cgp_launch_plan.restype = None
    lib.cgp_launch_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return lib


def plan(lib, n_rows, rpw):
    out = np.zeros(3, dtype=np.int64)
    lib.cgp_launch_plan(n_rows, rpw, out.ctypes.data)
    return int(out[0]), int(out[1]), int(out[2])


@pytest.mark.parametrize("rpw", [4, 2])
@pytest.mark.parametrize("n_rows", ROW_COUNTS)
def test_every_row_once_and_one_loss_slot_per_wave(shim, n_rows, rpw):
    grid, visits, slots = plan(shim, n_rows, rpw)
    assert slots == grid * 4
    if n_rows == 0:
        assert (grid, visits) == (0, 0)
        return
    waves = grid * 4
    assert grid >= 1 and visits >= 1
    # the positions the kernel forms: (wave + visit * waves) * rpw + row of the visit
    w = np.arange(waves, dtype=np.int64)[:, None, None]
    v = np.arange(visits, dtype=np.int64)[None, :, None]
    r = np.arange(rpw, dtype=np.int64)[None, None, :]
    pos = ((w + v * waves) * rpw + r).ravel()
    taken = np.bincount(pos[pos < n_rows], minlength=n_rows)
    assert taken.size == n_rows and np.all(taken == 1)
    # no visit in which no wave has a row, and small sets are spread over the workgroups before a wave gets a second visit
    assert (visits - 1) * waves * rpw < n_rows
    sets = -(-n_rows // rpw)
    if sets <= 4 * 512:
        assert visits == 1 and grid == -(-sets // 4)
    assert visits <= 32


def test_four_rows_per_wave_halve_the_waves_of_the_bench_bucket(shim):
    g2, v2, _ = plan(shim, 2_700_000, 2)
    g4, v4, _ = plan(shim, 2_700_000, 4)
    assert v2 == v4 == 32 and abs(2 * g4 - g2) <= 1
