"""The definition of `from_events` (rsparse_amd/events.py events_reference) without a device: against scipy's COO -> CSR route,
against a scalar restatement over a Python dict, the stated chunked summation order, the public function on the CPU stand-in
backend (which has no `events_to_csr` and so gets the numpy definition), the hand-over to train_test_split(by=), and the argument
errors."""
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from rsparse_amd.events import event_arguments, events_reference, f64_keys, keys_f64

ROOT = Path(__file__).resolve().parents[1]


def _backend():
    sys.path.insert(0, str(ROOT / "tests"))
    from oracle_backend import OracleBackend
    return OracleBackend()


def _log(n=5000, n_users=40, n_items=60, seed=3, integer_values=False):
    rng = np.random.default_rng(seed)
    u = rng.integers(0, n_users, n)
    u[u == 7] = 8                                    # an empty user in the middle
    i = (rng.zipf(1.6, n) - 1) % n_items
    v = rng.integers(1, 6, n).astype(float) if integer_values else rng.random(n) * 3.0 - 1.0
    t = np.floor(rng.random(n) * 5.0) - 2.0          # ties everywhere, negative values
    t[::11] = -0.0
    return u, i, v, t, (n_users + 2, n_items)        # (and two empty users at the end)


def _dict_restatement(u, i, v, t):
    """cell -> (count, max value, last value, latest timestamp), scalar code over the events in input order"""
    key = lambda d: int(f64_keys(np.array([d]))[0])
    cells = {}
    for e in range(u.size):
        c = (int(u[e]), int(i[e]))
        if c not in cells:
            cells[c] = [1, v[e], v[e], t[e]]
            continue
        s = cells[c]
        s[0] += 1
        if key(v[e]) > key(s[1]):
            s[1] = v[e]
        if key(t[e]) >= key(s[3]):                  # ties go to the later event
            s[2], s[3] = v[e], t[e]
    return cells


def test_pattern_and_integer_sums_equal_scipy():
    u, i, v, t, shape = _log(integer_values=True)
    p, j, x, count, latest = events_reference(u, i, v, shape=shape)
    m = sp.coo_matrix((v, (u, i)), shape=shape).tocsr()
    m.sum_duplicates()
    assert p.dtype == np.int32 and j.dtype == np.int32 and x.dtype == np.float64 and count.dtype == np.int32 and latest is None
    assert np.array_equal(p, m.indptr) and np.array_equal(j, m.indices)
    assert np.array_equal(x, m.data)                 # integers: any order gives the same sum
    assert p[8] == p[7] and p[-1] == p[-3] == j.size and count.sum() == u.size
    ones = events_reference(u, i, shape=shape)       # values=None: every value is 1
    assert np.array_equal(ones[2], count.astype(float)) and np.array_equal(ones[0], p)


def test_a_cell_that_sums_to_zero_stays_an_entry():
    p, j, x, count, _ = events_reference([0, 0, 1], [2, 2, 0], [1.5, -1.5, 2.0], shape=(2, 3))
    assert np.array_equal(p, [0, 1, 2]) and np.array_equal(j, [2, 0]) and np.array_equal(x, [0.0, 2.0]) and np.array_equal(count, [2, 1])


def test_count_max_last_latest_equal_the_dict_restatement():
    u, i, v, t, shape = _log()
    cells = _dict_restatement(u, i, v, t)
    order = sorted(cells)
    got = {a: events_reference(u, i, v, t, shape=shape, aggregate=a) for a in ("count", "max", "last")}
    p, j, _, count, latest = got["count"]
    rows = np.repeat(np.arange(shape[0]), np.diff(p))
    assert [(int(r), int(c)) for r, c in zip(rows, j)] == order
    assert np.array_equal(count, [cells[c][0] for c in order])
    assert np.array_equal(got["count"][2], count.astype(float))
    bits = lambda a: np.asarray(a, dtype=np.float64).view(np.uint64)
    assert np.array_equal(bits(got["max"][2]), bits([cells[c][1] for c in order]))
    assert np.array_equal(bits(got["last"][2]), bits([cells[c][2] for c in order]))
    assert np.array_equal(bits(latest), bits([cells[c][3] for c in order]))
    assert np.signbit(latest).any() and (latest == 0).any()
    for a in ("max", "last"):
        assert np.array_equal(got[a][0], p) and np.array_equal(got[a][1], j) and np.array_equal(got[a][3], count)


def test_the_bit_map_orders_the_zeros():
    k = f64_keys(np.array([-np.inf, -1.0, -0.0, 0.0, 5e-324, 1.0, np.inf]))
    assert np.all(np.diff(k.astype(object)) > 0)
    back = keys_f64(k)
    assert np.array_equal(back.view(np.uint64), np.array([-np.inf, -1.0, -0.0, 0.0, 5e-324, 1.0, np.inf]).view(np.uint64))
    _, _, x, _, latest = events_reference([0, 0], [0, 0], [0.0, -0.0], [-0.0, 0.0], shape=(1, 1), aggregate="max")
    assert not np.signbit(x[0]) and not np.signbit(latest[0])
    _, _, x, _, _ = events_reference([0, 0, 0], [0, 0, 0], [1.0, 2.0, 3.0], [4.0, 4.0, 1.0], shape=(1, 1), aggregate="last")
    assert x[0] == 2.0                               # the tie goes to the later event


def test_a_long_cell_is_summed_in_chunks_of_64():
    rng = np.random.default_rng(5)
    for seed in range(50):                           # values for which the two orders differ in the last bits
        v = np.random.default_rng(seed).random(200) * 10.0 ** rng.integers(-3, 4, 200)
        plain = 0.0
        for a in v:
            plain = plain + a
        chunks = []
        for c0 in range(0, 200, 64):
            s = v[c0]
            for a in v[c0 + 1:c0 + 64]:
                s = s + a
            chunks.append(s)
        chunked = chunks[0]
        for s in chunks[1:]:
            chunked = chunked + s
        if chunked != plain:
            break
    assert chunked != plain
    # the cell among others, its events spread over the log
    n = 1000
    u, i = rng.integers(0, 5, n), rng.integers(0, 7, n)
    other = rng.random(n)
    free = ~((u == 2) & (i == 3))
    u, i, other = u[free], i[free], other[free]
    where = np.sort(rng.choice(u.size + 200, 200, replace=False))
    uu, ii, vv = np.zeros(u.size + 200, int), np.zeros(u.size + 200, int), np.zeros(u.size + 200)
    mask = np.zeros(u.size + 200, bool)
    mask[where] = True
    uu[mask], ii[mask], vv[mask] = 2, 3, v
    uu[~mask], ii[~mask], vv[~mask] = u, i, other
    p, j, x, count, _ = events_reference(uu, ii, vv, shape=(5, 7))
    c = p[2] + int(np.searchsorted(j[p[2]:p[3]], 3))
    assert count[c] == 200 and x[c] == chunked and x[c] != plain
    # a cell of exactly 64 events is one chunk: left to right
    p, j, x, count, _ = events_reference(np.zeros(64, int), np.zeros(64, int), v[:64], shape=(1, 1))
    assert x[0] == chunks[0]


def test_decay_follows_the_stated_expression():
    u, i, v, t, shape = _log(n=400)
    p, j, x, count, latest = events_reference(u, i, v, t, shape=shape, half_life=1.5)
    now = t.max()
    w = v * np.exp2((t - now) / 1.5)
    cells = {}
    for e in range(u.size):
        c = (int(u[e]), int(i[e]))
        cells[c] = cells[c] + w[e] if c in cells else w[e]
    assert count.max() <= 64 and np.array_equal(x, [cells[c] for c in sorted(cells)])
    x2 = events_reference(u, i, v, t, shape=shape, half_life=1.5, now=now)[2]
    assert np.array_equal(x, x2)
    x3 = events_reference(u, i, v, t, shape=shape, half_life=1.5, now=now + 1.5)[2]
    assert np.allclose(x3, x / 2.0, rtol=1e-14)


def test_from_events_on_the_cpu_stand_in():
    from rsparse_amd import from_events
    u, i, v, t, shape = _log()
    res = from_events(u.astype(np.int64), i.astype(np.uint16), v, t, shape=shape, aggregate="max", backend=_backend())
    p, j, x, count, latest = events_reference(u, i, v, t, shape=shape, aggregate="max")
    for m, d, dt in ((res.x, x, np.float64), (res.count, count, np.int32), (res.latest, latest, np.float64)):
        assert sp.issparse(m) and m.format == "csr" and m.shape == shape and m.dtype == dt and m.has_canonical_format
        assert np.array_equal(m.indptr, p) and np.array_equal(m.indices, j) and np.array_equal(m.data.view(np.uint8), d.view(np.uint8))
    res = from_events(u, i, backend=_backend())       # shape=None: max id + 1; no timestamps: no .latest
    assert res.x.shape == (int(u.max()) + 1, int(i.max()) + 1) and res.latest is None
    assert np.array_equal(res.x.data, res.count.data.astype(float))
    empty = from_events(np.zeros(0, np.int64), np.zeros(0, np.int64), shape=(3, 4), backend=_backend())
    assert empty.x.shape == (3, 4) and empty.x.nnz == 0 and np.array_equal(empty.x.indptr, [0, 0, 0, 0])


def test_latest_drives_a_temporal_leave_last_out():
    from rsparse_amd import from_events, train_test_split
    rng = np.random.default_rng(12)
    n_users, n_items, n = 30, 50, 1500
    u, i = rng.integers(0, n_users, n), rng.integers(0, n_items, n)
    t = rng.permutation(n).astype(np.int64) + 1_600_000_000       # distinct integer timestamps
    res = from_events(u, i, None, t, shape=(n_users, n_items), backend=_backend())
    assert np.array_equal(res.latest.indptr, res.x.indptr) and np.array_equal(res.latest.indices, res.x.indices)
    train, test = train_test_split(res.x, leave_out=1, by=res.latest, backend=_backend())
    assert (train + test != res.x).nnz == 0
    for user in range(n_users):
        mine = u == user
        if len(set(i[mine])) < 2:
            continue
        newest = int(i[mine][np.argmax(t[mine])])                  # the item of the user's most recent event
        assert test[user].indices.tolist() == [newest]


def test_argument_errors():
    from rsparse_amd import from_events
    be = _backend()
    u, i, v, t = np.array([0, 1, 2]), np.array([0, 5, 1]), np.array([1.0, 2.0, 3.0]), np.array([1.0, 2.0, 3.0])
    ok = from_events(u, i, v, t, backend=be)
    assert ok.x.shape == (3, 6)
    bad = [dict(users=u[:2]), dict(users=u.astype(float)), dict(users=u.reshape(3, 1)), dict(values=v[:2]), dict(timestamps=t[:2]),
           dict(shape=(2, 6)), dict(shape=(3, 5)), dict(users=np.array([0, -1, 2])), dict(shape=(3, 2 ** 31)), dict(shape=(3,)),
           dict(users=np.array([0, 2 ** 32, 2], np.int64), shape=(3, 6)),              # judged before the narrowing to int32
           dict(items=np.array([0, 2 ** 32 + 1, 2], np.int64), shape=(3, 6)),
           dict(values=np.array([1.0, np.nan, 3.0])), dict(timestamps=np.array([1.0, np.nan, 3.0])),
           dict(timestamps=np.array([1, 2 ** 53 + 1, 3], np.int64)), dict(timestamps=np.array([1, -2 ** 53 - 1, 3], np.int64)),
           dict(aggregate="mean"), dict(aggregate="last", timestamps=None), dict(half_life=2.0, timestamps=None),
           dict(half_life=2.0, aggregate="max"), dict(half_life=0.0), dict(half_life=-1.0), dict(half_life=2.0, now=np.nan)]
    for b in bad:
        kw = dict(users=u, items=i, values=v, timestamps=t, backend=be)
        kw.update(b)
        with pytest.raises((ValueError, TypeError)):
            from_events(**kw)
    assert from_events(u, i, v, np.array([1, 2 ** 53, 3], np.int64), backend=be).latest.data.max() == 2.0 ** 53
    with pytest.raises((ValueError, TypeError)):
        events_reference(u, i, v, t, shape=(3, 6), aggregate="median")
    assert event_arguments(u, i, None, None, None, "sum", None, None)[4] == (3, 6)
