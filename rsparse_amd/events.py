"""`from_events`: the users x items interaction matrix from a raw event log -- one (user, item[, value][, timestamp]) record per
play, click or purchase -- built on the device by wrmf_events.hip.  `events_reference` is the definition in numpy (the C header
states it for other hosts): the canonical CSR over the CELLS, the distinct (user, item) pairs of the log, with an aggregate of
every cell's events, their count and their latest timestamp.  The sum has a STATED order, so the device result equals the
reference bit for bit."""
import numpy as np
import scipy.sparse as sp
import torch

AGGREGATES = {"sum": 0, "count": 1, "max": 2, "last": 3}   # RSPARSE_HIP_EVENTS_*
CHUNK = 64   # events per chunk of the summation order


def f64_keys(a):
    """the order-preserving 64-bit keys of doubles (the split's map: larger value <=> larger key, -0.0 just below +0.0)"""
    u = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def keys_f64(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63), k & np.uint64((1 << 63) - 1), ~k).view(np.float64)


def _ids(a, what):
    a = np.asarray(a)
    if a.ndim != 1 or not (np.issubdtype(a.dtype, np.integer) and a.dtype != np.bool_):
        raise TypeError("from_events: %s must be a one-dimensional array of integers" % what)
    return a


def event_arguments(users, items, values, timestamps, shape, aggregate, half_life, now):
    """-> (users int32, items int32, values float64 or None, timestamps float64 or None, (n_users, n_items), aggregate, half life
    or None, now or None), checked: what both the device route and the reference start from"""
    u, i = _ids(users, "users"), _ids(items, "items")
    n = u.size
    if i.size != n:
        raise ValueError("from_events: users and items differ in length")
    if n >= 2 ** 31:
        raise ValueError("from_events: a log of 2^31 events or more must be cut into several calls")
    if aggregate not in AGGREGATES:
        raise ValueError("from_events: aggregate must be one of %s" % ", ".join(sorted(AGGREGATES)))
    if shape is None:
        shape = (int(u.max()) + 1 if n else 0, int(i.max()) + 1 if n else 0)
    if len(shape) != 2 or any(isinstance(s, bool) or int(s) != s for s in shape):
        raise TypeError("from_events: shape must be two integers")
    n_users, n_items = int(shape[0]), int(shape[1])
    if not (0 <= n_users < 2 ** 31 and 0 <= n_items < 2 ** 31):
        raise ValueError("from_events: the shape must lie in [0, 2^31)")
    # the ids are judged in their own dtype, BEFORE they are narrowed to int32
    if n and (int(u.min()) < 0 or int(u.max()) >= n_users or int(i.min()) < 0 or int(i.max()) >= n_items):
        raise ValueError("from_events: a user or item id outside the shape %d x %d" % (n_users, n_items))
    v = t = None
    if values is not None:
        v = np.ascontiguousarray(values, dtype=np.float64)
        if v.shape != (n,):
            raise ValueError("from_events: values must have one entry per event")
        if np.isnan(v).any():
            raise ValueError("from_events: NaN in values")
    if timestamps is not None:
        t = np.asarray(timestamps)
        if t.shape != (n,):
            raise ValueError("from_events: timestamps must have one entry per event")
        if np.issubdtype(t.dtype, np.integer) and n and (int(t.max()) > 2 ** 53 or int(t.min()) < -2 ** 53):
            raise ValueError("from_events: integer timestamps beyond 2^53 in magnitude are not exact doubles")
        t = np.ascontiguousarray(t, dtype=np.float64)
        if np.isnan(t).any():
            raise ValueError("from_events: NaN in timestamps")
    if aggregate == "last" and t is None:
        raise ValueError("from_events: aggregate='last' needs timestamps")
    if half_life is not None:
        half_life = float(half_life)
        if aggregate != "sum":
            raise ValueError("from_events: half_life goes with aggregate='sum' only")
        if t is None:
            raise ValueError("from_events: half_life needs timestamps")
        if not half_life > 0.0 or half_life == np.inf:
            raise ValueError("from_events: half_life must be positive and finite")
    if now is not None:
        now = float(now)
        if now != now:
            raise ValueError("from_events: now is NaN")
    return (np.ascontiguousarray(u, dtype=np.int32), np.ascontiguousarray(i, dtype=np.int32), v, t, (n_users, n_items), aggregate,
            half_life, now)


def _reference(u, i, v, t, shape, aggregate, half_life, now):
    n_users = shape[0]
    n = u.size
    if n == 0:
        e = np.zeros(0)
        return np.zeros(n_users + 1, np.int32), np.zeros(0, np.int32), e, np.zeros(0, np.int32), None if t is None else e.copy()
    order = np.lexsort((np.arange(n), i, u))   # the events of a cell in input order
    us, it = u[order].astype(np.int64), i[order].astype(np.int64)
    head = np.ones(n, bool)
    head[1:] = (us[1:] != us[:-1]) | (it[1:] != it[:-1])
    starts = np.flatnonzero(head)
    n_cells = starts.size
    count = np.diff(np.append(starts, n)).astype(np.int32)
    j = it[starts].astype(np.int32)
    p = np.zeros(n_users + 1, np.int64)
    p[1:] = np.cumsum(np.bincount(us[starts], minlength=n_users))
    cell = np.cumsum(head) - 1
    pos = np.arange(n) - starts[cell]          # an event's position in its cell
    vs = np.ones(n) if v is None else v[order]
    latest = tk = None
    if t is not None:
        ts = t[order]
        tk = f64_keys(ts)
        latest = keys_f64(np.maximum.reduceat(tk, starts))
    if aggregate == "count":
        x = count.astype(np.float64)
    elif aggregate == "max":
        x = keys_f64(np.maximum.reduceat(f64_keys(vs), starts))
    elif aggregate == "last":
        pick = np.lexsort((order, tk, cell))   # per cell: ascending timestamp, ties by the place in the input
        x = vs[pick[starts + count - 1]]
    else:
        term = vs
        if half_life is not None:
            if now is None:
                now = float(keys_f64(tk.max(keepdims=True))[0])
            term = vs * np.exp2((ts - now) / half_life)
        # chunks of CHUNK events counted from the cell's first event, each summed left to right ...
        n_chunks = (count.astype(np.int64) + CHUNK - 1) // CHUNK
        chunk0 = np.cumsum(n_chunks) - n_chunks
        g = chunk0[cell] + pos // CHUNK
        k = pos % CHUNK
        csum = np.zeros(int(n_chunks.sum()))
        for kk in range(CHUNK):
            sel = np.flatnonzero(k == kk)      # (at most one event per chunk: the indexed update below is a plain loop step)
            if kk == 0:
                csum[g[sel]] = term[sel]
            else:
                csum[g[sel]] = csum[g[sel]] + term[sel]
        # ... and the chunk sums of a cell left to right
        x = np.zeros(n_cells)
        for c in range(int(n_chunks.max())):
            sel = np.flatnonzero(n_chunks > c)
            if c == 0:
                x[sel] = csum[chunk0[sel]]
            else:
                x[sel] = x[sel] + csum[chunk0[sel] + c]
    return p.astype(np.int32), j, x, count, latest


def events_reference(users, items, values=None, timestamps=None, *, shape, aggregate="sum", half_life=None, now=None):
    """The definition.  -> (p int32[n_users + 1], j int32[n_cells], x float64[n_cells], count int32[n_cells], latest
    float64[n_cells] or None): the canonical CSR over the cells of the log -- rows in order, columns ascending and unique within
    a row, empty rows included; a cell whose aggregate is 0 stays an entry.  The events of a cell are taken in input order.

      count    the number of events of the cell
      latest   its largest timestamp, compared through the order-preserving 64-bit map of the double's bits (-0.0 below +0.0)
      x        "count": count as a double; "max": the largest value, by the same map; "last": the value of the event with the
               largest timestamp, ties to the event later in the input; "sum": the sum of the terms v (1.0 without values), or
               with half_life v * exp2((t - now) / half_life) in double, now defaulting to the largest timestamp of the log.  A
               cell of at most 64 events is summed left to right; a longer one in consecutive chunks of 64 events from its first
               event, each left to right, and the chunk sums then left to right."""
    return _reference(*event_arguments(users, items, values, timestamps, shape, aggregate, half_life, now))


class Interactions:
    """what from_events returns: .x (float64), .count (int32) and .latest (float64, None without timestamps) -- scipy CSR
    matrices of one shared pattern, canonical"""
    __slots__ = ("x", "count", "latest")

    def __init__(self, x, count, latest):
        self.x, self.count, self.latest = x, count, latest

    def __repr__(self):
        return "Interactions(shape=%r, cells=%d, latest=%s)" % (self.x.shape, self.x.nnz, "no" if self.latest is None else "yes")


def _csr(data, j, p, shape):
    m = sp.csr_matrix((data, j, p), shape=shape)
    m.has_sorted_indices = True
    m.has_canonical_format = True   # (columns ascending and unique within a row, by construction)
    return m


def from_events(users, items, values=None, timestamps=None, shape=None, aggregate="sum", half_life=None, now=None, device=None,
                backend=None):
    """The interaction matrix of an event log: users, items (integers, one per event), optional values and timestamps ->
    an object with .x, .count and .latest (see events_reference for the aggregates "sum", "count", "max", "last", the decay
    half_life / now and the summation order).  shape=None takes max id + 1.  Packed, sorted and reduced on the device
    (wrmf_events.hip); `backend`: an object with the HipBackend interface (default: HipBackend(device)); one without
    `events_to_csr` gets the numpy definition.  .x goes into WRMF.fit_transform / train_test_split, .latest into
    train_test_split(by=)."""
    u, i, v, t, shape, aggregate, half_life, now = event_arguments(users, items, values, timestamps, shape, aggregate, half_life, now)
    if backend is None:
        from .engine import HipBackend
        backend = HipBackend(device)
    if hasattr(backend, "events_to_csr"):
        d = lambda a, dt: None if a is None else backend.to_device(a, dt)
        out = backend.events_to_csr(d(u, torch.int32), d(i, torch.int32), d(v, torch.float64), d(t, torch.float64), shape[0], shape[1],
                                    aggregate=aggregate, half_life=half_life, now=now)
        p, j, x, count, latest = (None if o is None else o.cpu().numpy() for o in out)
    else:
        p, j, x, count, latest = _reference(u, i, v, t, shape, aggregate, half_life, now)
    return Interactions(_csr(x, j, p, shape), _csr(count, j, p, shape), None if latest is None else _csr(latest, j, p, shape))
