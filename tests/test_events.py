"""The event-log ingest on the device (wrmf_events.hip) against its numpy definition (rsparse_amd/events.py events_reference):
every output is compared with ==, bit for bit -- the sum has a stated order.  One shuffled log of about 4e5 events serves most
tests; its reference is computed once per aggregate."""
import ctypes
import functools

import numpy as np
import pytest

from rsparse_amd import _lib
from rsparse_amd.events import AGGREGATES, events_reference

pytestmark = pytest.mark.gpu

SPAN = 1024          # kEvSpan of wrmf_events.hip: sorted entries per span of the heads / reduce launches
N_USERS, N_ITEMS = 300, 400_000
SPECIAL = (1, 2, 3, 63, 64, 65, 127, 128, 129, 4096, 4097, 70_000)
HEAVY, SPECIAL_USER, EMPTY = 2, 3, (0, 1, 150, 298, 299)
# the ulp bound of the device's double exp2, measured on this test's own arguments against np.exp2 in np.longdouble and rounded
# up (profiles/events/README.md has the measurement; the installed math-library documents state none)
EXP2_ULP = 1


@functools.lru_cache(maxsize=None)
def _log():
    """-> (users, items, values, timestamps) of the shuffled log, the rising cell's item"""
    rng = np.random.default_rng(2024)
    users, items = [], []
    # the heavy user comes first in the sorted order (users 0 and 1 are empty), so its cells lie at sorted positions 0, 1, ...:
    # cells of 2 events, or 3 where a cell would otherwise end at a span boundary -- no cell begins at a multiple of SPAN, every
    # span boundary of its range lies inside a cell
    sizes, at = [], 0
    while at < 100 * SPAN + 7:
        c = 3 if (at + 2) % SPAN == 0 else 2
        sizes.append(c)
        at += c
    sizes = np.array(sizes)
    starts = np.cumsum(sizes) - sizes
    assert not np.isin(np.arange(1, 101) * SPAN, starts).any()
    heavy_items = np.sort(rng.choice(N_ITEMS, sizes.size, replace=False))
    users.append(np.full(at, HEAVY))
    items.append(np.repeat(heavy_items, sizes))
    # the special cells, in an order that puts short ones between the long ones
    special_items = rng.choice(N_ITEMS - 1, len(SPECIAL), replace=False)
    for c, it in zip(SPECIAL, special_items):
        users.append(np.full(c, SPECIAL_USER))
        items.append(np.full(c, it))
    users.append(np.array([SPECIAL_USER]))
    items.append(np.array([N_ITEMS - 1]))                # the last item id
    # the crowd: the other users, Zipf items, so that cells of a few events are common
    n_crowd = 220_000
    cu = rng.integers(4, N_USERS - 2, n_crowd)
    cu[cu == 150] = 151
    users.append(cu)
    items.append((rng.zipf(1.3, n_crowd) - 1) % N_ITEMS)
    u, i = np.concatenate(users), np.concatenate(items)
    perm = rng.permutation(u.size)
    u, i = u[perm], i[perm]
    v = rng.random(u.size) * 4.0 - 1.0                    # non-integers: the order of a sum matters
    # timestamps: three values per user (ties everywhere, negative values, both zeros) ...
    pick = rng.integers(0, 3, u.size)
    t = np.where(pick == 0, -(u + 1) / 4.0, np.where(pick == 1, 0.0, (u + 1) / 8.0))
    t[(pick == 1) & (rng.random(u.size) < 0.5)] = -0.0
    # ... and one strictly rising cell
    rising = int(special_items[SPECIAL.index(4097)])
    sel = np.flatnonzero((u == SPECIAL_USER) & (i == rising))
    t[sel] = 1000.0 + np.arange(sel.size)
    return u.astype(np.int32), i.astype(np.int32), v, t, rising


@functools.lru_cache(maxsize=None)
def _reference(aggregate):
    u, i, v, t, _ = _log()
    return events_reference(u, i, v, t, shape=(N_USERS, N_ITEMS), aggregate=aggregate)


def _device(u, i, v, t, shape, **kw):
    import torch
    from rsparse_amd.engine import HipBackend
    be = HipBackend()
    d = lambda a, dt: None if a is None else be.to_device(a, dt)
    out = be.events_to_csr(d(u, torch.int32), d(i, torch.int32), d(v, torch.float64), d(t, torch.float64), shape[0], shape[1], **kw)
    torch.cuda.synchronize()
    return [None if o is None else o.cpu().numpy() for o in out]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_same(got, want, names=("p", "j", "x", "count", "latest")):
    for name, g, w in zip(("p", "j", "x", "count", "latest"), got, want):
        if name not in names:
            continue
        assert (g is None) == (w is None), name
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), name


def test_the_log_has_the_cases_it_is_built_for():
    u, i, v, t, rising = _log()
    p, j, x, count, latest = _reference("sum")
    assert 3.9e5 < u.size < 4.1e5 and j.size > 1e5
    assert set(SPECIAL) <= set(count.tolist())
    lens = np.diff(p)
    assert all(lens[e] == 0 for e in EMPTY) and lens[HEAVY] > 40_000 and p[HEAVY] == 0
    # cells that straddle span boundaries: every boundary of the heavy user's range, and long cells elsewhere
    starts = np.cumsum(count.astype(np.int64)) - count
    bounds = np.arange(1, u.size // SPAN + 1) * SPAN
    owner = np.searchsorted(starts, bounds, side="right") - 1
    inside = starts[owner] < bounds
    heavy_end = starts[p[HEAVY + 1]]
    assert inside[bounds < heavy_end].all() and (bounds < heavy_end).sum() >= 100
    assert (inside & (count[owner] > 64)).sum() >= 60
    assert np.signbit(latest[latest == 0]).any() and not np.signbit(latest[latest == 0]).all() and (latest < 0).any()
    c = p[SPECIAL_USER] + int(np.searchsorted(j[p[SPECIAL_USER]:p[SPECIAL_USER + 1]], rising))
    assert count[c] == 4097 and latest[c] == 1000.0 + 4096


@pytest.mark.parametrize("aggregate", ["sum", "count", "max", "last"])
def test_every_output_equals_the_reference(aggregate):
    u, i, v, t, _ = _log()
    got = _device(u, i, v, t, (N_USERS, N_ITEMS), aggregate=aggregate)
    _assert_same(got, _reference(aggregate))


def test_without_values_and_without_timestamps():
    u, i, v, t, _ = _log()
    got = _device(u, i, None, None, (N_USERS, N_ITEMS))
    want = _reference("count")
    assert got[4] is None
    _assert_same(got, want, names=("p", "j", "x", "count"))                # the sum of ones is the count
    got = _device(u, i, None, t, (N_USERS, N_ITEMS), aggregate="count")
    _assert_same(got, want)


def test_a_second_permutation_leaves_count_max_and_latest():
    u, i, v, t, _ = _log()
    perm = np.random.default_rng(77).permutation(u.size)
    got = _device(u[perm], i[perm], v[perm], t[perm], (N_USERS, N_ITEMS), aggregate="max")
    _assert_same(got, _reference("max"))


def test_repeat_calls_are_bit_identical():
    u, i, v, t, _ = _log()
    a = _device(u, i, v, t, (N_USERS, N_ITEMS), half_life=1000.0)
    b = _device(u, i, v, t, (N_USERS, N_ITEMS), half_life=1000.0)
    _assert_same(a, b)


def test_one_user_and_one_item():
    rng = np.random.default_rng(1)
    for n in (1, 64, 65, 300):                                              # (n = 1: a single event)
        z = np.zeros(n, np.int32)
        v, t = rng.random(n) - 0.5, np.floor(rng.random(n) * 3.0)
        for aggregate in ("sum", "max", "last"):
            got = _device(z, z, v, t, (1, 1), aggregate=aggregate)
            _assert_same(got, events_reference(z, z, v, t, shape=(1, 1), aggregate=aggregate))
            assert got[3].tolist() == [n]


def test_a_single_event_in_a_large_shape():
    got = _device(np.array([5], np.int32), np.array([123_456], np.int32), np.array([0.3]), np.array([-2.0]), (9, 200_000))
    assert got[0].tolist() == [0] * 6 + [1] * 4 and got[1].tolist() == [123_456] and got[2].tolist() == [0.3]
    assert got[3].tolist() == [1] and got[4].tolist() == [-2.0]


@pytest.mark.parametrize("shape", [(40, 2 ** 31 - 1), (2 ** 12, 2 ** 20), (2 ** 12, 2 ** 20 + 1)], ids=["items_2^31-1", "32_key_bits", "33_key_bits"])
def test_key_widths(shape):
    rng = np.random.default_rng(9)
    n = 6000
    n_users, n_items = shape
    # ids at the top of both ranges (the largest key has every bit in use set), at the bottom, and a crowd with duplicates
    u = np.r_[np.full(70, n_users - 1), n_users - 1, 0, 0, rng.integers(0, n_users, n)]
    pool = np.r_[n_items - 1, n_items - 2, 0, rng.integers(0, n_items, 200)]
    i = np.r_[np.full(70, n_items - 1), n_items - 2, 0, n_items - 1, rng.choice(pool, n)]
    perm = rng.permutation(u.size)
    u, i = u[perm].astype(np.int32), i[perm].astype(np.int32)
    v, t = rng.random(u.size), np.floor(rng.random(u.size) * 4.0) - 2.0
    want = events_reference(u, i, v, t, shape=shape)
    assert want[3].max() >= 70 and want[1].max() == n_items - 1
    _assert_same(_device(u, i, v, t, shape), want)


def test_an_id_outside_the_shape_is_refused_with_the_outputs_untouched():
    import torch
    lib = _lib.load()
    for users, items in (([0, 3, 1], [0, 1, 2]), ([0, 1, -1], [0, 1, 2]), ([0, 1, 2], [0, 5, 2]), ([0, 1, 2], [-7, 1, 2])):
        u = torch.tensor(users, dtype=torch.int32, device="cuda")
        i = torch.tensor(items, dtype=torch.int32, device="cuda")
        outs = [torch.full((4,), -1, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.float64, torch.int32)]
        cells = ctypes.c_int64(-1)
        rc = lib.rsparse_hip_events_to_csr_device(3, 3, 5, u.data_ptr(), i.data_ptr(), None, None, 0, 0.0, 0.0, 0, outs[0].data_ptr(),
                                                  outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), None, 4, ctypes.byref(cells),
                                                  None)
        torch.cuda.synchronize()
        assert rc == _lib.ERR_INVALID and all(bool((o == -1).all()) for o in outs)
    # a capacity below the number of cells: refused before an output array is written
    u = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    rc = lib.rsparse_hip_events_to_csr_device(3, 3, 5, u.data_ptr(), u.data_ptr(), None, None, 0, 0.0, 0.0, 0, outs[0].data_ptr(),
                                              outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), None, 2, ctypes.byref(cells), None)
    torch.cuda.synchronize()
    assert rc == _lib.ERR_INVALID and cells.value == 3 and all(bool((o == -1).all()) for o in outs)
    # no event: p is all zeros
    rc = lib.rsparse_hip_events_to_csr_device(0, 3, 5, None, None, None, None, 0, 0.0, 0.0, 0, outs[0].data_ptr(), None, None, None, None, 0,
                                              ctypes.byref(cells), None)
    torch.cuda.synchronize()
    assert rc == _lib.OK and cells.value == 0 and outs[0].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("aggregate", ["sum", "last"])
def test_host_form_equals_device_form(aggregate):
    u, i, v, t, _ = _log()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n = u.size
    p, j, x = np.full(N_USERS + 1, -1, np.int32), np.full(n, -1, np.int32), np.full(n, -1.0)
    count, latest = np.full(n, -1, np.int32), np.full(n, -1.0)
    cells = ctypes.c_int64(-1)
    _lib.check(_lib.load().rsparse_hip_events_to_csr(n, N_USERS, N_ITEMS, vp(u), vp(i), vp(v), vp(t), AGGREGATES[aggregate], 0.0, 0.0, 0,
                                                     vp(p), vp(j), vp(x), vp(count), vp(latest), n, ctypes.byref(cells)))
    c = cells.value
    want = _reference(aggregate)
    assert c == want[1].size and np.all(j[c:] == -1) and np.all(x[c:] == -1.0)
    _assert_same((p, j[:c], x[:c], count[:c], latest[:c]), want)


def _weights(t, half_life, now):
    """the device's decay weights exp2((t - now) / half_life) of the timestamps t, read off the kernel itself: without values a
    cell of one event holds 1.0 * weight"""
    z, items = np.zeros(t.size, np.int32), np.arange(t.size, dtype=np.int32)
    got = _device(z, items, None, t, (1, t.size), half_life=half_life, now=now)
    assert got[3].tolist() == [1] * t.size
    return got[2]


def test_decayed_sum_within_the_derived_bound():
    """x = sum of v * exp2((t - now) / half_life) per cell, in the stated order on both sides.  The exponent is IEEE arithmetic on
    both sides; a weight is within EXP2_ULP ulp (device) / 1 ulp (numpy) of the true value, each product is rounded once, and a
    cell of m events has m - 1 roundings of its sums in the same order: |dev - ref| <= (m + EXP2_ULP + 2) * 2^-52 * sum |term_ref|
    per cell.

    The exponent: the device's double subtraction and division give numpy's bits (==, through torch on the device), and the
    kernel's own weights lie within EXP2_ULP ulp of exp2 of THAT exponent in extended precision -- an exponent one ulp off would
    move a weight by hundreds of ulps."""
    import torch
    u, i, v, t, _ = _log()
    half_life = 1000.0
    for now in (None, 7.25):
        got = _device(u, i, v, t, (N_USERS, N_ITEMS), half_life=half_life, now=now)
        want = events_reference(u, i, v, t, shape=(N_USERS, N_ITEMS), half_life=half_life, now=now)
        _assert_same(got, want, names=("p", "j", "count", "latest"))
        now_v = float(t.max()) if now is None else now
        arg = (t - now_v) / half_life
        t_dev = torch.from_numpy(t).cuda()
        arg_dev = torch.div(t_dev - torch.full_like(t_dev, now_v), torch.full_like(t_dev, half_life)).cpu().numpy()
        assert np.array_equal(_bits(arg), _bits(arg_dev))
        tu = np.unique(t)
        exact = np.exp2(((tu - now_v) / half_life).astype(np.longdouble))
        w_err = np.abs(_weights(tu, half_life, now).astype(np.longdouble) - exact) / np.spacing(exact.astype(np.float64))
        print("decay now=%r: the kernel's weights are within %.3f ulp of exp2 of the reference's exponent (%d timestamps)"
              % (now, float(w_err.max()), tu.size))
        assert float(w_err.max()) <= EXP2_ULP
        mag = events_reference(u, i, np.abs(v), t, shape=(N_USERS, N_ITEMS), half_life=half_life, now=now)[2]   # sum |term_ref|
        m = want[3].astype(np.float64)
        assert np.isfinite(mag).all() and mag.min() > 0.0
        bound = (m + EXP2_ULP + 2.0) * 2.0 ** -52 * mag
        err = np.abs(got[2] - want[2])
        print("decay now=%r: largest |dev - ref| / bound = %.3g, cells that differ: %d of %d"
              % (now, float((err / bound).max()), int((err > 0).sum()), err.size))
        assert np.all(err <= bound)
