"""BPR / WARP through item features on the device (the compose, item-totals and backward kernels of wrmf_bpr_features.hip
behind rsparse_hip_*_feat_*) against the numpy definition of rsparse_amd/bpr.py and warp.py, bit for bit: exact equality is derived, not
measured -- every operation of the definition is one rounded float64 operation, in a fixed order."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rsparse_amd import BPR, WARP
from rsparse_amd.bpr import bpr_feat_fit_reference, bpr_triples, canonical_features, compose_reference, n_steps_of
from rsparse_amd.warp import rank_weights, warp_feat_fit_reference
from test_bpr import DTYPES, TORCH, backend, bits_equal, upload

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS, N_FEAT, SEED, BATCH = 150, 201, 121, 77, 512
LONELY = 180   # the one item of feature 103; no user holds it, so only a drawn negative touches it


@functools.lru_cache(maxsize=None)
def interactions():
    d = np.random.default_rng(4).random((N_USERS, N_ITEMS)) < 0.1
    d[:, LONELY] = False
    x = sp.csr_matrix(d.astype(np.float64))
    x.sort_indices()
    return x


@functools.lru_cache(maxsize=None)
def features():
    """201 items x 121 features with every edge of the backward kernel: features 0..99 an identity block on the items 0..99;
    100 held by the items 0..199 (4 chunk slots, the last of 8 positions); 101 by exactly 64 items, 102 by exactly 65; 103 by the
    LONELY item alone (untouched in some steps); 104 by nobody; 105..120 by item 199 (17 features with its 100); item 200 has no
    feature; the other items have 1, 2 or 3.  The values outside the identity block are normal draws, negative ones included."""
    rng = np.random.default_rng(8)
    F = sp.lil_matrix((N_ITEMS, N_FEAT))
    for i in range(100):
        F[i, i] = 1.0
    for f, items in ((100, range(200)), (101, range(64)), (102, range(100, 165)), (103, [LONELY]), *((f, [199]) for f in range(105, 121))):
        for i in items:
            F[i, f] = rng.standard_normal()
    F = canonical_features(F, N_ITEMS, np.float64)
    per_item, per_feat = np.diff(F.indptr), np.diff(F.tocsc().indptr)
    assert per_feat[[100, 101, 102, 103, 104]].tolist() == [200, 64, 65, 1, 0] and per_item[200] == 0 and per_item[199] == 17
    assert {1, 2, 3} <= set(per_item.tolist()) and (F.data < 0).any() and F.nnz == 100 + 200 + 64 + 65 + 1 + 16
    # the triples of BPR do not depend on the model: some step of the fit below leaves the lonely item alone, another one not
    x, steps = interactions(), n_steps_of(interactions().nnz, BATCH)
    touched = [LONELY in bpr_triples(SEED, 0, e, 0, x.indptr, x.indices, N_ITEMS, s, steps)[2] for e in range(2) for s in range(steps)]
    assert steps >= 5 and x.nnz % steps != 0 and any(touched) and not all(touched)
    return F


@pytest.mark.parametrize("precision", ["float", "double"])
@pytest.mark.parametrize("loss", ["bpr", "warp"])
@pytest.mark.parametrize("rank", [18, 20, 64, 128])     # 18: the compose kernel's 4-byte form (rank % 4 != 0)
def test_fit_through_features_equals_the_definition(rank, loss, precision):
    dtype, be, x, rng = DTYPES[precision], backend(), interactions(), np.random.default_rng(rank)
    F = canonical_features(features(), N_ITEMS, dtype)
    U0, H0 = ((0.3 * rng.standard_normal((n, rank))).astype(dtype) for n in (N_USERS, N_FEAT))
    w = rank_weights(N_ITEMS, 8)
    if loss == "bpr":
        ref = bpr_feat_fit_reference(x.indptr, x.indices, F, U0, H0, 2, SEED, 0.05, 0.01, BATCH)
    else:
        ref = warp_feat_fit_reference(x.indptr, x.indices, F, U0, H0, 2, SEED, 8, 0.1, w, 0.05, 0.01, BATCH)
    feat = be.item_features(F, TORCH[dtype])

    def run():
        dev = [be.to_device(a, t) for a, t in ((U0, TORCH[dtype]), (H0, TORCH[dtype]), (np.zeros(N_USERS), torch.float64),
                                               (np.zeros(N_FEAT), torch.float64))]
        if loss == "bpr":
            counts, V = be.bpr_feat_epochs(*upload(x), x.nnz, 0, SEED, 0, 0, 2, BATCH, feat, *dev, 0.05, 0.01)
        else:
            counts, V = be.warp_feat_epochs(*upload(x), x.nnz, 0, SEED, 0, 0, 2, BATCH, 8, 0.1, w, feat, *dev, 0.05, 0.01)
        return [t.cpu().numpy() for t in dev] + [V.cpu().numpy()], [tuple(r) for r in counts.cpu().tolist()]

    (got, trace), (again, trace2) = run(), run()
    for name, a, b in zip(("U", "H", "aU", "aH", "V"), got, ref[:4] + (compose_reference(F, ref[1]),)):
        assert bits_equal(a, b), (name, int((a != b).sum()))
    assert trace == ref[4] == trace2 and all(bits_equal(a, b) for a, b in zip(got, again))
    H = got[1]
    assert bits_equal(H[104], H0[104]) and not (H[:104] == H0[:104]).all(axis=1).any() and not got[4][200].any()


@pytest.mark.parametrize("precision", ["float", "double"])
@pytest.mark.parametrize("model", [BPR, WARP])
def test_identity_features_are_the_plain_fit(model, precision):
    x = interactions()
    plain, hybrid = (model(rank=20, batch=BATCH, precision=precision, rng=5) for _ in range(2))
    U = plain.fit_transform(x, 2)
    U2 = hybrid.fit_transform(x, 2, item_features=sp.identity(N_ITEMS, format="csr"))
    assert bits_equal(U, U2) and bits_equal(plain.components, hybrid.components) and plain.trace == hybrid.trace
    assert bits_equal(hybrid.feature_embeddings.T, plain.components) and bits_equal(hybrid.feature_adagrad, plain.item_adagrad)
    assert bits_equal(hybrid.user_adagrad, plain.user_adagrad) and (plain.components != 0).all() and hybrid.item_adagrad is None


def test_unseen_items_are_composed_and_ranked():
    x, F = interactions(), features()
    m = WARP(rank=20, batch=BATCH, precision="double", rng=5)
    m.fit_transform(x, 2, item_features=F)
    assert bits_equal(m.components.T, compose_reference(F, m.feature_embeddings))
    new = sp.random(5, N_FEAT, density=0.1, random_state=2, data_rvs=np.random.default_rng(2).standard_normal).tolil()
    new[0, 100] = 0.5
    new = new.tocsr()
    emb = m.compose_items(new)
    assert bits_equal(emb, compose_reference(canonical_features(new, 5, np.float64), m.feature_embeddings)) and emb[0].any()
    both = m.with_items(sp.vstack([F, new]))
    hist = sp.hstack([x, sp.csr_matrix((N_USERS, 5))]).tocsr()
    assert bits_equal(both.components.T, np.vstack([m.components.T, emb])) and m.components.shape[1] == N_ITEMS
    lists = both.predict(hist, 5, items_exclude=range(N_ITEMS))                # only the cold-start items are admissible
    scores = both.transform(hist) @ emb.T
    assert np.array_equal(np.asarray(lists), N_ITEMS + np.argsort(-scores, axis=1, kind="stable"))
