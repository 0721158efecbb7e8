"""The two cuts of bucket 1 (rows of 257..512 non-zeros) in the host-side launch schedule (rsparse_amd/csrc/wrmf_schedule.cpp),
without a device: order[off[1], team4_wide_first) goes to the 8-wave teams, order[team4_wide_first, team4_first) -- the rows of
kTeam4Max + 1..kTeam4WideMax non-zeros -- to the 4-wave teams of 24 quads per wave, order[team4_first, off[2]) to those of 20.
The planner and tests/schedule_wide_shim.cpp are compiled with g++ into pytest's temporary directory."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("schedule_wide") / "libschedule_wide_shim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(out),
                           str(ROOT / "rsparse_amd" / "csrc" / "wrmf_schedule.cpp"), str(ROOT / "tests" / "schedule_wide_shim.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.sched_wide.restype = ctypes.c_int
    lib.sched_wide.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def plan(lib, lens, cus=256):
    lens = np.asarray(lens, dtype=np.int64)
    p = np.ascontiguousarray(np.concatenate([[0], np.cumsum(lens)]), dtype=np.int32)
    out, order = np.zeros(11, dtype=np.int64), np.zeros(max(len(lens), 1), dtype=np.int64)
    assert lib.sched_wide(p.ctypes.data, len(lens), cus, out.ctypes.data, order.ctypes.data) == 1
    return dict(t4=int(out[0]), W=int(out[1]), wide_first=int(out[2]), first=int(out[3]), off=[int(v) for v in out[4:]],
                order=order[:len(lens)])


def _rng_lens(seed, lo, hi, n):
    return np.random.default_rng(seed).integers(lo, hi, size=n)


CASES = {
    "all_three": lambda: _rng_lens(1, 200, 600, 4000),
    "edges": lambda: np.array([256, 257, 320, 321, 322, 380, 383, 384, 385, 511, 512, 513, 0, 1, 16, 17] * 3),
    "no_wide_rows": lambda: np.concatenate([_rng_lens(2, 257, 321, 300), _rng_lens(3, 385, 513, 300), _rng_lens(4, 0, 200, 300)]),
    "only_wide_rows": lambda: np.concatenate([_rng_lens(5, 321, 385, 300), _rng_lens(6, 0, 257, 300)]),
    "no_short_team_rows": lambda: np.concatenate([_rng_lens(7, 321, 513, 300), _rng_lens(8, 0, 257, 300)]),
    "no_8_wave_rows": lambda: np.concatenate([_rng_lens(9, 257, 385, 300), _rng_lens(10, 600, 900, 20)]),
    "bucket1_empty": lambda: np.concatenate([_rng_lens(11, 0, 257, 300), _rng_lens(12, 513, 900, 20)]),
    "everything_short": lambda: _rng_lens(13, 0, 30, 500),
    "everything_long": lambda: _rng_lens(14, 600, 700, 50),
    "no_rows": lambda: np.zeros(0, dtype=np.int64),
}


def test_the_wide_capacity_is_one_the_kernel_can_have(shim):
    pl = plan(shim, [1])
    assert pl["t4"] == 320 and pl["W"] in (352, 384)   # 4 waves x 22 / 24 quads x 4 non-zeros
    assert 256 < pl["t4"] < pl["W"] < 512


@pytest.mark.parametrize("cus", [256, 4])
@pytest.mark.parametrize("case", sorted(CASES))
def test_bucket1_cuts(shim, case, cus):
    lens = CASES[case]()
    pl = plan(shim, lens, cus)
    off, wf, f, W, t4 = pl["off"], pl["wide_first"], pl["first"], pl["W"], pl["t4"]
    assert wf <= f
    assert off[1] <= wf <= off[2] and off[1] <= f <= off[2]
    ol = lens[pl["order"]] if len(lens) else lens
    assert np.all(ol[off[1]:wf] > W) and np.all(ol[off[1]:wf] <= 512)
    assert np.all((ol[wf:f] > t4) & (ol[wf:f] <= W))
    assert np.all((ol[f:off[2]] > 256) & (ol[f:off[2]] <= t4))
    # ... and they are the counts numpy finds
    assert wf == int((lens > W).sum()) and f == int((lens > t4).sum())
    assert f - wf == int(((lens > t4) & (lens <= W)).sum())
    want_empty = {"no_wide_rows": (False, True, False), "only_wide_rows": (True, False, True),
                  "no_short_team_rows": (False, False, True), "no_8_wave_rows": (True, False, False),
                  "bucket1_empty": (True, True, True), "everything_short": (True, True, True),
                  "everything_long": (True, True, True), "no_rows": (True, True, True)}
    if case in want_empty:
        assert (wf == off[1], f == wf, off[2] == f) == want_empty[case]
