"""The launch schedule planned on the host (rsparse_amd/csrc/wrmf_schedule.cpp) without a device: the planner and a few lines of
extern "C" (tests/schedule_shim.cpp) are compiled with g++ into pytest's temporary directory and checked against

  * a Python model of the cut and the deal (`cut`, `deal` below), entry for entry -- the loss partials are summed in list
    order, so the tables that reach the device decide the bits of the results;
  * invariants of a list set stated without the model (`check_list_set`);
  * numpy for the row order and the positions at which the launchers cut it.

One invariant is narrower than it reads: "every segment is at least 64 steps long" holds for all segments of a row but
possibly its last -- a row is cut into runs of per = ceil(steps / parts) >= 64 steps and the last run takes the remainder
(193 steps in three parts: 65, 65, 63).  That needs a row whose share-bound part count reaches steps // 64 without dividing
the steps; none of the sets below has one, so the check is made as stated, on every segment.
"""
import ctypes
import heapq
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
FIXED = 12                       # per-row cost of the CG solve in 16-non-zero steps: what plan_schedule cuts with
BOUNDS = (512, 256, 128, 64, 32)   # bucket b holds the rows of BOUNDS[b] < len <= BOUNDS[b - 1]
MAXSEG, MAXTOT = 16, 1024
CUS = (256, 4, 1)


# ---- the model -------------------------------------------------------------------------------------------------------
def cut(lens, fixed, cus):
    n_slots = 2 * max(cus, 1)
    st = [(l + 15) // 16 for l in lens]
    share = max(1, sum(s + fixed for s in st) // n_slots)
    items, segs = [], []                      # item = (cost, entry); entry >= 0: position r, -(s+1): segment s
    for r, (l, s) in enumerate(zip(lens, st)):
        parts = 1
        if n_slots >= 8 and 2 * (s + fixed) > share:
            parts = min(MAXSEG, s // 64, (4 * s + share - 1) // share)
        if parts < 2 or len(segs) + parts > MAXTOT:
            items.append((s + fixed, r))
            continue
        per = (s + parts - 1) // parts
        made, slot = len(range(0, s, per)), len(segs)
        for idx, s0 in enumerate(range(0, s, per)):
            n0, n1 = s0 * 16, min(l, (s0 + per) * 16)
            segs.append((r, n0, n1 - n0, idx, made, slot))
            items.append(((n1 - n0 + 15) // 16 + fixed, -len(segs)))
    return items, segs


def deal(items, n_prefix, cus, fine):
    n_slots = 2 * max(cus, 1)
    n_wg = max(n_slots, min(n_prefix // 8, 256 * max(cus, 1))) if fine else n_slots
    items = sorted(items, key=lambda t: -t[0])          # stable
    n_wg = min(n_wg, len(items))
    heap = [(0, w) for w in range(n_wg)]
    lists = [[] for _ in range(n_wg)]
    for c, e in items:
        load, w = heapq.heappop(heap)
        lists[w].append(e)
        heapq.heappush(heap, (load + c, w))
    return lists


# ---- the planner under test --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("schedule") / "libschedule_shim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(out),
                           str(ROOT / "rsparse_amd" / "csrc" / "wrmf_schedule.cpp"), str(ROOT / "tests" / "schedule_shim.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.sched_plan.restype = ctypes.c_void_p
    lib.sched_plan.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.sched_free.argtypes = [ctypes.c_void_p]
    lib.sched_counters.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.sched_vector.restype = ctypes.c_int64
    lib.sched_vector.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64]
    return lib


COUNTERS = ("max_len", "n_long", "nnz_long", "n_empty") + tuple("q_off%d" % b for b in range(7)) + \
    tuple("q_nnz%d" % b for b in range(6)) + ("q_pair_first", "q_team4_first", "q_gt32", "q_gt48", "q_lr_first", "q_n_lr",
                                               "q_n_chol_long", "q_n_nec", "nec_is_ne")
VECTORS = {"order": 0, "stream_off": 1, "cut_cost": 10, "cut_entry": 11, "cut_segs": 12, "cut_split_rows": 13,
           "cut_split_ptr": 14, "fine_rows": 15, "fine_ptr": 16, "coarse_rows": 17, "coarse_ptr": 18, "nec_cost": 20,
           "nec_entry": 21, "nec_segs": 22, "nec_split_rows": 23, "nec_split_ptr": 24, "nec_rows": 25, "nec_ptr": 26}


def plan(lib, lens, cus):
    """-> dict of the counters and vectors of the plan for a matrix whose columns have `lens` non-zeros"""
    p = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))])
    assert p[-1] < 2 ** 31
    p = np.ascontiguousarray(p, dtype=np.int32)
    h = lib.sched_plan(p.ctypes.data, len(lens), cus)
    assert h
    try:
        c = np.zeros(32, dtype=np.int64)
        lib.sched_counters(h, c.ctypes.data)
        res = dict(zip(COUNTERS, (int(v) for v in c)))
        for name, which in VECTORS.items():
            n = lib.sched_vector(h, which, None, 0)
            assert n >= 0
            v = np.zeros(n, dtype=np.int64)
            assert lib.sched_vector(h, which, v.ctypes.data, n) == n
            res[name] = v
    finally:
        lib.sched_free(h)
    return res


def list_sets(pl, lens):
    """the (up to) three list sets of a plan: name, prefix length, cut vectors, rows, ptr"""
    n_stream = int((np.asarray(lens) > BOUNDS[0]).sum())
    sets = [("fine", n_stream, "cut", pl["fine_rows"], pl["fine_ptr"]),
            ("coarse", n_stream, "cut", pl["coarse_rows"], pl["coarse_ptr"])]
    if not pl["nec_is_ne"]:
        sets.append(("nec", pl["q_n_nec"], "nec", pl["nec_rows"], pl["nec_ptr"]))
    return sets


# ---- the cases ---------------------------------------------------------------------------------------------------------
def _shuffled(lens, seed):
    lens = np.asarray(lens, dtype=np.int64)
    return lens[np.random.default_rng(seed).permutation(len(lens))]


def _heavy():
    rng = np.random.default_rng(20240607)
    long_rows = np.minimum(513 + (rng.pareto(1.1, 20000) * 600).astype(np.int64), 400000)   # heavy tail: a few rows beyond 16384
    short_rows = rng.integers(0, 513, 30000)
    return _shuffled(np.concatenate([long_rows, short_rows]), 1)


CASES = {
    "giant": _shuffled([200000] + [600] * 40, 2),
    "round6": _shuffled([2048] + [520] * 100, 3),      # the shape of the round-6 bug: a row whole in one deal, split in the table
    "flat": np.full(5000, 1000, dtype=np.int64),
    "heavy": _heavy(),
    "empty": np.zeros(0, dtype=np.int64),
    "short": np.random.default_rng(5).integers(0, 513, 3000),   # no long row
}
# the model run by hand for fixed = 12: {case: {cus: (segments, split rows, entries, fine lists, coarse lists)}}
TABLE = {
    "giant": {256: (16, 1, 56, 56, 56), 4: (16, 1, 56, 8, 8)},
    "round6": {256: (2, 1, 102, 102, 102), 4: (0, 0, 101, 12, 8)},
    "flat": {256: (0, 0, 5000, 625, 512), 4: (0, 0, 5000, 625, 8)},
}


def test_cases_are_what_they_claim():
    assert (CASES["heavy"] > 512).sum() == 20000 and (CASES["heavy"] > 16384).sum() > 0
    assert CASES["short"].max() <= 512 and (CASES["short"] == 0).sum() > 0


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_order_and_counters(shim, case, cus):
    lens = CASES[case]
    pl = plan(shim, lens, cus)
    n = len(lens)
    order = pl["order"]
    assert sorted(order.tolist()) == list(range(n))                      # a permutation of the rows
    ol = lens[order]
    assert np.all(ol[:-1] >= ol[1:])                                     # lengths non-increasing
    assert np.all((ol[:-1] > ol[1:]) | (order[:-1] < order[1:]))         # ties ascending by row id
    gt = lambda t: int((lens > t).sum())
    want = {"max_len": int(lens.max()) if n else 0, "n_long": gt(32), "nnz_long": int(lens[lens > 32].sum()),
            "n_empty": int((lens == 0).sum()), "q_pair_first": gt(16), "q_team4_first": gt(320), "q_gt32": gt(32), "q_gt48": gt(48),
            "q_lr_first": gt(64), "q_n_lr": int(((lens >= 1) & (lens <= 64)).sum()), "q_n_chol_long": gt(4096), "q_n_nec": gt(16384),
            "q_off0": 0, "q_off6": n}
    for b, t in enumerate(BOUNDS):
        want["q_off%d" % (b + 1)] = gt(t)
    edges = (2 ** 62,) + BOUNDS + (-1,)
    for b in range(6):
        want["q_nnz%d" % b] = int(lens[(lens <= edges[b]) & (lens > edges[b + 1])].sum())
    assert {k: pl[k] for k in want} == want
    n_stream = gt(512)
    assert pl["nec_is_ne"] == (gt(16384) == n_stream)
    if n_stream:
        assert pl["stream_off"].tolist() == np.concatenate([[0], np.cumsum(ol[:n_stream])]).tolist()
    else:
        assert len(pl["stream_off"]) == 0 and len(pl["fine_ptr"]) == 0 and len(pl["coarse_ptr"]) == 0 and len(pl["cut_entry"]) == 0


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_lists_equal_the_model(shim, case, cus):
    lens = CASES[case]
    pl = plan(shim, lens, cus)
    order = pl["order"].tolist()
    ol = lens[pl["order"]].tolist()
    for name, n_prefix, cv, rows, ptr in list_sets(pl, lens):
        items, segs = cut(ol[:n_prefix], FIXED, cus)
        items = [(c, order[e] if e >= 0 else e) for c, e in items]     # (the tables name rows by id, not by position)
        segs = [(order[s[0]],) + tuple(s[1:]) for s in segs]
        dealt = sorted(items, key=lambda t: -t[0])
        assert pl[cv + "_cost"].tolist() == [c for c, _ in dealt], name
        assert pl[cv + "_entry"].tolist() == [e for _, e in dealt], name
        assert pl[cv + "_segs"].tolist() == [v for s in segs for v in s], name
        firsts = [-(i + 1) for i, s in enumerate(segs) if s[3] == 0]
        assert pl[cv + "_split_rows"].tolist() == firsts, name
        assert pl[cv + "_split_ptr"].tolist() == (list(range(len(firsts) + 1)) if segs else []), name
        lists = deal(items, n_prefix, cus, name != "coarse")
        assert rows.tolist() == [e for l in lists for e in l], name
        assert ptr.tolist() == (np.concatenate([[0], np.cumsum([len(l) for l in lists])]).tolist() if lists else []), name
    if case in TABLE and cus in TABLE[case]:
        got = (len(pl["cut_segs"]) // 6, len(pl["cut_split_rows"]), len(pl["cut_entry"]), len(pl["fine_ptr"]) - 1, len(pl["coarse_ptr"]) - 1)
        assert got == TABLE[case][cus]


def check_list_set(lens, prefix_rows, entries, segs, split_rows, split_ptr, rows, ptr):
    """invariants of one list set, stated without the model; prefix_rows: ids of the rows the set covers"""
    segs = np.asarray(segs).reshape(-1, 6)
    assert len(segs) <= MAXTOT
    assert len(rows) == len(entries) and sorted(rows.tolist()) == sorted(entries.tolist())
    if len(rows):
        assert ptr[0] == 0 and ptr[-1] == len(rows) and np.all(np.diff(ptr) > 0)       # no list is empty
    else:
        assert len(ptr) == 0
    whole = [e for e in rows.tolist() if e >= 0]
    seg_ids = sorted(-e - 1 for e in rows.tolist() if e < 0)
    assert seg_ids == list(range(len(segs)))                                           # every segment in exactly one list
    assert len(set(whole)) == len(whole)
    split = {}
    for s, (row, n0, nn, idx, made, slot) in enumerate(segs.tolist()):
        split.setdefault(row, []).append((s, n0, nn, idx, made, slot))
    assert not (set(whole) & set(split))
    assert sorted(whole + list(split)) == sorted(prefix_rows)                          # every row whole or split, once
    for row, ss in split.items():
        assert 2 <= len(ss) <= MAXSEG
        at = 0
        for k, (s, n0, nn, idx, made, slot) in enumerate(ss):
            assert (idx, made, slot) == (k, len(ss), ss[0][0]) and s == ss[0][0] + k     # consecutive in the table
            assert n0 == at and n0 % 16 == 0 and (nn + 15) // 16 >= 64                   # tile [0, len) in order
            at += nn
        assert at == lens[row]
    firsts = [-(ss[0][0] + 1) for ss in split.values()]
    assert sorted(split_rows.tolist()) == sorted(firsts) and len(set(firsts)) == len(firsts)
    assert split_ptr.tolist() == (list(range(len(firsts) + 1)) if len(segs) else [])


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_list_set_invariants(shim, case, cus):
    lens = CASES[case]
    pl = plan(shim, lens, cus)
    for name, n_prefix, cv, rows, ptr in list_sets(pl, lens):
        check_list_set(lens, pl["order"][:n_prefix].tolist(), pl[cv + "_entry"], pl[cv + "_segs"], pl[cv + "_split_rows"],
                       pl[cv + "_split_ptr"], rows, ptr)
    # fine and coarse deals of one cut hold the same entries
    assert sorted(pl["fine_rows"].tolist()) == sorted(pl["coarse_rows"].tolist())
    if len(pl["fine_ptr"]):
        assert len(pl["coarse_ptr"]) - 1 <= 2 * cus and len(pl["fine_ptr"]) >= len(pl["coarse_ptr"])


def test_decreasing_col_ptrs_are_refused(shim):
    p = np.array([0, 5, 3, 9], dtype=np.int32)
    assert not shim.sched_plan(p.ctypes.data, 3, 256)
