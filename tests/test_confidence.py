"""The kernels of wrmf_confidence.hip (segment moments, tables, apply) against numpy, and `WRMF(preprocess=Confidence(kind))` on the
device against the plain model run on the device-weighted matrix.

Bounds, in units of u = 2^-53 (nothing here is fitted to what the kernels return):
  moments   integer values 1..5: every partial sum is an integer below 2^53, so any summation order is exact: ==.  Random
            doubles: |dev - fsum| <= len u sum|terms|, the a-priori bound of recursive summation in ANY order (Higham 4.2:
            (len - 1) u + O(u^2)); the terms |v| and fl(v v) are the same doubles on both sides (no contraction).
  idf       log(N) - log1p(df): device log / log1p at the OpenCL-C bounds of 3 and 2 ulp, numpy at 1 ulp, one subtraction:
            |d| <= (3 + 1) u log(N) + (2 + 1) u log(N + 1) + u |idf| < 16 u log(N + 1).
  K1 L_u    K1 ((1 - B) + (B s_u) / sbar) on the exact s_u and sbar (fsum) has four roundings on either side: rtol 8 u; the
            device's s_u and sbar = total / N carry the moment bound, relative len_u u and nnz u (positive values), which
            reaches the result through the term K1 (B s_u) / sbar: + K1 B (s_u / sbar) (len_u + nnz + 2) u.
  norm      n^(scale - 1) on the DEVICE's moments: sqrt exact, pow at 16 ulp on the device and 1 in numpy; the rounding of the
            exponent and of sqrt's result moves pow by a few ulp more: rtol 48 u.
  apply     against the numpy formula on the device's own tables: +, x, /, sqrt are correctly rounded on both sides, at most
            four in a chain (bm25), whatever is contracted: rtol 8 u.  "log": one log1p per element (2 ulp device, 1 numpy), its
            argument rounded once, then a product and a sum: rtol 16 u.
The observed maxima are in profiles/confidence/README.md."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SPAN = 1024            # kConfSpan of wrmf_confidence.hip
N_COL, HOT = 5000, 7
KINDS = (("linear", {"alpha": 40.0}), ("log", {"alpha": 40.0, "eps": 0.5}), ("tfidf", {}), ("bm25", {}), ("bm25", {"K1": 1.2, "B": 0.75}),
         ("normalize", {"norm": 1, "target": "rows"}), ("normalize", {"norm": 2, "target": "rows"}),
         ("normalize", {"norm": 1, "target": "columns", "scale": 0.25}), ("normalize", {"norm": 2, "target": "columns"}))


def _pattern():
    """~330 rows over 5000 columns: row lengths on both sides of every class break (a thread's four entries, a wave's 256, the
    span), one row longer than three spans, the first and last rows empty, runs of empty rows, one hot column in most rows"""
    rng = np.random.default_rng(17)
    lens = [0, 1, 63, 64, 65, 3, 4, 5, 255, 256, 257, SPAN - 1, SPAN, SPAN + 1, 0, 0, 2 * SPAN + 1, 3 * SPAN + 400, 2, 0, SPAN, SPAN]
    lens += list(rng.integers(0, 40, size=330 - len(lens) - 1)) + [0]
    indptr, indices = [0], []
    for r, n in enumerate(lens):
        cols = rng.choice(N_COL, size=n, replace=False)
        if n and r % 5 and HOT not in cols:
            cols[0] = HOT
        indices.append(np.sort(cols))
        indptr.append(indptr[-1] + n)
    return np.array(indptr, np.int32), np.concatenate(indices).astype(np.int32), len(lens)


@pytest.fixture(scope="module")
def be():
    from rsparse_amd.engine import HipBackend
    return HipBackend()


@pytest.fixture(scope="module")
def mats(be):
    """the shared matrix with integer and with random values, in both orientations, on the host and on the device"""
    indptr, indices, n = _pattern()
    nnz = int(indptr[-1])
    rng = np.random.default_rng(5)
    out = {}
    for name, vals in (("int", rng.integers(1, 6, size=nnz).astype(np.float64)), ("rnd", 0.05 + rng.random(nnz) * 5.0)):
        um = sp.csr_matrix((vals, indices, indptr), shape=(n, N_COL))
        pos = sp.csr_matrix((np.arange(1, nnz + 1, dtype=np.float64), indices, indptr), shape=(n, N_COL)).tocsc()
        pos.sort_indices()
        perm = pos.data.astype(np.int64) - 1          # item-major entry e is user-major entry perm[e]
        im = (pos.indptr.astype(np.int32), pos.indices.astype(np.int32), vals[perm])
        host = {"um": (indptr, indices, vals), "im": im, "perm": perm}
        dev = {k: (be.to_device(host[k][0], torch.int32), be.to_device(host[k][1], torch.int32), be.to_device(host[k][2], torch.float64))
               for k in ("um", "im")}
        out[name] = (host, dev)
    return out


def _segments(p, x):
    return [x[p[r]:p[r + 1]] for r in range(len(p) - 1)]


@pytest.mark.parametrize("side", ["um", "im"])
@pytest.mark.parametrize("power", [1, 2])
def test_moments_of_integers_are_exact(be, mats, side, power):
    host, dev = mats["int"]
    p, _, x = host[side]
    out, total = be.confidence_moments(dev[side][0], dev[side][2], power)
    expect = np.array([float((np.abs(s) ** power).sum()) for s in _segments(p, x)])
    assert np.array_equal(out.cpu().numpy(), expect)
    assert float(total.cpu()[0]) == float((np.abs(x) ** power).sum())


@pytest.mark.parametrize("side", ["um", "im"])
@pytest.mark.parametrize("power", [1, 2])
def test_moments_of_doubles_within_the_summation_bound(be, mats, side, power):
    host, dev = mats["rnd"]
    p, _, x = host[side]
    out, total = be.confidence_moments(dev[side][0], dev[side][2], power)
    again, total2 = be.confidence_moments(dev[side][0], dev[side][2], power)
    got = out.cpu().numpy()
    assert np.array_equal(got, again.cpu().numpy()) and np.array_equal(total.cpu().numpy(), total2.cpu().numpy())   # every bit
    terms = np.abs(x) if power == 1 else x * x
    worst = 0.0
    for r, s in enumerate(_segments(p, terms)):
        exact = math.fsum(s)
        bound = len(s) * U * exact
        worst = max(worst, abs(got[r] - exact) / bound if bound else abs(got[r]))
        assert abs(got[r] - exact) <= bound, (r, len(s), got[r], exact)
    exact = math.fsum(terms)
    print("moments %s power %d: worst error / bound %.3g; total error %.3g u of the sum" % (side, power, worst, abs(float(total.cpu()[0]) - exact) / exact / U))
    assert abs(float(total.cpu()[0]) - exact) <= len(terms) * U * exact


def test_no_entries(be):
    p = be.to_device(np.zeros(6, np.int32), torch.int32)
    i = be.to_device(np.zeros(0, np.int32), torch.int32)
    x = be.to_device(np.zeros(0), torch.float64)
    out, total = be.confidence_moments(p, x, 2)
    assert out.cpu().tolist() == [0.0] * 5 and float(total.cpu()[0]) == 0.0
    assert be.confidence_apply("linear", p, i, x, a=2.0).numel() == 0
    from rsparse_amd import Confidence
    for kind in ("bm25", "tfidf", "normalize", "log"):
        w = Confidence(kind, backend=be).fit_transform(sp.csr_matrix((5, 9)))
        assert w.shape == (5, 9) and w.nnz == 0


def test_tables_against_numpy(be, mats):
    from rsparse_amd.confidence import norm_table
    host, dev = mats["rnd"]
    p, _, x = host["um"]
    pt = host["im"][0]
    n, nnz = len(p) - 1, len(x)
    idf = be.confidence_table("idf", N_COL, p=dev["im"][0], a=float(n)).cpu().numpy()
    df = np.diff(pt).astype(np.float64)
    d = np.abs(idf - (np.log(float(n)) - np.log1p(df)))
    print("idf: max error %.3g u log(N + 1)" % (d.max() / (U * np.log(n + 1.0))))
    assert d.max() <= 16 * U * np.log(n + 1.0)
    assert idf.argmin() == HOT and idf[HOT] < 1.0          # the hot column

    mom, total = be.confidence_moments(dev["um"][0], dev["um"][2], 1)
    for K1, B in ((100.0, 0.8), (1.2, 0.75)):
        got = be.confidence_table("bm25", n, moment=mom, total=total, a=K1, b=B, c=float(n)).cpu().numpy()
        s_u = np.array([math.fsum(s) for s in _segments(p, x)])
        sbar = math.fsum(x) / n
        expect = K1 * ((1.0 - B) + (B * s_u) / sbar)
        bound = 8 * U * np.abs(expect) + K1 * B * (s_u / sbar) * (np.diff(p) + nnz + 2) * U
        print("K1 L_u (K1 = %g): max error / bound %.3g" % (K1, (np.abs(got - expect) / bound).max()))
        assert (np.abs(got - expect) <= bound).all()

    for side in ("um", "im"):
        for norm in (1, 2):
            m, _ = be.confidence_moments(dev[side][0], dev[side][2], norm)
            for scale in (0.5, 0.25, 0.0):
                got = be.confidence_table("norm", int(m.numel()), moment=m, a=scale, b=float(norm)).cpu().numpy()
                expect = norm_table(m.cpu().numpy(), scale, norm)
                assert np.array_equal(got == 0, expect == 0) and (got == 0).any()          # the zero rule: empty segments
                nz = expect != 0
                rel = np.abs(got[nz] - expect[nz]) / np.abs(expect[nz])
                print("norm table %s norm %d scale %g: max %.3g u" % (side, norm, scale, rel.max() / U))
                assert rel.max() <= 48 * U


def _numpy_formula(kind, par, v, ut, it):
    if kind == "linear":
        return 1.0 + par["alpha"] * v
    if kind == "log":
        return 1.0 + par["alpha"] * np.log1p(v / par["eps"])
    if kind == "tfidf":
        return np.sqrt(v) * it
    if kind == "bm25":
        return ((v * (par["K1"] + 1.0)) / (ut + v)) * it
    return v * (ut if par["target"] == "rows" else it)


@pytest.mark.parametrize("kind,par", KINDS)
def test_apply_against_numpy_on_the_device_tables(be, mats, kind, par):
    """fit on the resident arrays of both orientations, weight both, and compare: the numpy formula on the device's own tables
    (copied back); float output == the double output rounded; in place == out of place; a cell gets the same bits from the
    user-major and from the item-major arrays"""
    from rsparse_amd import Confidence
    host, dev = mats["rnd"]
    (p, j, x), (pt, it_idx, xt), perm = host["um"], host["im"], host["perm"]
    n = len(p) - 1
    c = Confidence(kind, **par)
    mom = c.device_fit(be, n, N_COL, dev["um"], dev["im"])
    user_t = c.device_user_table(be, dev["um"], mom)
    w_um = c.device_apply(be, dev["um"], user_t)
    w_im = c.device_apply(be, dev["im"], user_t, item_major=True)
    got = w_um.cpu().numpy()
    par = c.params
    rows = np.repeat(np.arange(n), np.diff(p))
    ut = None if user_t is None else user_t.cpu().numpy()[rows]
    it = None if c.item_table is None else c.item_table[j]
    expect = _numpy_formula(kind, par, x, ut, it)
    rel = np.abs(got - expect) / np.abs(expect)
    tol = 16 if kind == "log" else 8
    print("apply %s %s: max %.3g u" % (kind, par, rel.max() / U))
    assert rel.max() <= tol * U
    # the same bits from the other orientation
    assert np.array_equal(w_im.cpu().numpy(), got[perm])
    # float output, rounded once from the double result
    for arrays, w, item_major in ((dev["um"], w_um, False), (dev["im"], w_im, True)):
        f32 = c.device_apply(be, arrays, user_t, item_major=item_major, out=torch.float32)
        assert f32.dtype == torch.float32 and np.array_equal(f32.cpu().numpy(), w.cpu().numpy().astype(np.float32))
        copy = (arrays[0], arrays[1], arrays[2].clone())
        same = c.device_apply(be, copy, user_t, item_major=item_major, out="inplace")
        assert same.data_ptr() == copy[2].data_ptr() and np.array_equal(same.cpu().numpy(), w.cpu().numpy())
    assert np.array_equal(dev["um"][2].cpu().numpy(), x) and np.array_equal(dev["im"][2].cpu().numpy(), xt)   # the inputs stand


def test_class_equals_the_reference(be, mats):
    """scipy in, scipy out: the public class on the device within the sum of the bounds above of confidence_reference (1e-13 covers
    every one of them at these sizes), new rows weighted with the statistics of the fit"""
    from rsparse_amd import Confidence, ScaleNormalize
    from rsparse_amd.confidence import confidence_reference
    host, _ = mats["rnd"]
    p, j, x = host["um"]
    m = sp.csr_matrix((x, j, p), shape=(len(p) - 1, N_COL))
    train, new = m[:200], m[200:]
    for kind, par in KINDS:
        c = Confidence(kind, backend=be, **par)
        w = c.fit_transform(train)
        ref = Confidence(kind, backend=object(), **par)      # (a backend without the kernels: the numpy reference)
        w_ref = ref.fit_transform(train)
        assert np.array_equal(w.indices, train.indices) and np.array_equal(w.indptr, train.indptr)
        np.testing.assert_allclose(w.data, w_ref.data, rtol=1e-13)
        np.testing.assert_allclose(c.transform(new).data, ref.transform(new).data, rtol=1e-13)
        assert np.array_equal(c.transform(train).data, w.data)
        assert c.n_fit == 200
    for target in ("rows", "columns"):
        sn, sn_ref = ScaleNormalize(target=target, backend=be), ScaleNormalize(target=target, backend=object())
        np.testing.assert_allclose(sn.fit_transform(train).data, sn_ref.fit_transform(train).data, rtol=1e-13)
        np.testing.assert_allclose(sn.scaling, sn_ref.scaling, rtol=1e-13)
    from rsparse_amd import _lib
    with pytest.raises(_lib.UnsupportedOnDevice):
        ScaleNormalize(norm=3, backend=be).fit(train)
    with pytest.raises(_lib.UnsupportedOnDevice):
        Confidence("normalize", norm=3, backend=be).fit(train)
    assert confidence_reference(train, "normalize", norm=3).nnz == train.nnz       # the numpy reference takes any norm > 0


@pytest.fixture(scope="module")
def ml():
    from conftest import load_movielens
    n_user, n_item, p, i, x = load_movielens()
    m = sp.csc_matrix((x, i, p), shape=(n_user, n_item)).tocsr()
    m.sort_indices()
    return m[:900], m[900:]


@pytest.mark.parametrize("precision", ["float", "double"])
@pytest.mark.parametrize("kind,par", [("bm25", {}), ("log", {"alpha": 40.0})])
def test_wrmf_equals_the_plain_model_on_the_device_weighted_matrix(be, ml, kind, par, precision):
    from rsparse_amd import WRMF, Confidence
    train, new = ml
    kw = dict(rank=16, lambda_=0.1, precision=precision)
    c = Confidence(kind, **par)
    a = WRMF(preprocess=c, rng=1, **kw)
    emb_a = a.fit_transform(train, n_iter=2, convergence_tol=-1)
    c2 = Confidence(kind, backend=be, **par)
    xw = c2.fit_transform(train)                     # the device-weighted values, copied back
    b = WRMF(rng=1, **kw)
    emb_b = b.fit_transform(xw, n_iter=2, convergence_tol=-1)
    assert np.array_equal(emb_a, emb_b) and np.array_equal(a.components, b.components) and a.losses == b.losses
    assert c.n_fit == 900 and np.array_equal(c.item_count, np.diff(train.tocsc().indptr))
    if kind == "bm25":
        assert np.array_equal(c.item_table, c2.item_table) and c.mean_row_sum == c2.mean_row_sum
    new_w = c2.transform(new)
    assert np.array_equal(a.transform(new), b.transform(new_w))
    pa, pb = a.predict(new, 10), b.predict(new_w, 10)
    assert np.array_equal(np.asarray(pa), np.asarray(pb)) and np.array_equal(pa.scores, pb.scores)
    # the implicit global bias: the sum of the weighted values, taken on the device in another order
    ga = WRMF(preprocess=Confidence(kind, **par), rng=1, with_global_bias=True, **kw)
    ga.fit_transform(train, n_iter=1, convergence_tol=-1)
    gb = WRMF(rng=1, with_global_bias=True, **kw)
    gb.fit_transform(xw, n_iter=1, convergence_tol=-1)
    print("global bias %s %s: %.17g vs %.17g" % (kind, precision, ga.global_bias, gb.global_bias))
    assert ga.global_bias > 0 and abs(ga.global_bias - gb.global_bias) <= train.nnz * U * gb.global_bias


@pytest.mark.parametrize("solver", ["conjugate_gradient", "nnls"])
def test_negative_weighted_values_are_refused_on_the_device(solver):
    """idf_i < 0 for an item that every user has: kept by the weighting, refused by the fit with the text it has always had"""
    from rsparse_amd import WRMF, Confidence
    rng = np.random.default_rng(2)
    d = (rng.random((20, 30)) < 0.2) * 1.0
    d[:, 4] = 2.0
    c = Confidence("tfidf")
    with pytest.raises(ValueError, match=r"all\(c_ui@x >= 0\) is not TRUE"):
        WRMF(rank=4, preprocess=c, solver=solver, feedback="implicit" if solver != "nnls" else "explicit", precision="float").fit_transform(sp.csr_matrix(d))
    assert c.item_table[4] < 0
