"""rsparse_amd -- MI355X-native WRMF / ALS solver behind rsparse's WRMF operator boundary.

Only the hot path of the reference (R/model_WRMF.R + inst/include/wrmf_{implicit,explicit}.hpp):
  rsparse_amd.WRMF            host-side mirror of the R6 class
  rsparse_amd.metrics         ap_k() / ndcg_k(), the reference's ranking metrics, and precision / recall / hit rate / MRR /
                              coverage at several cutoffs, on the device
  rsparse_amd.train_test_split  the reference's train_test_split (and leave-n-out), drawn on the device
  rsparse_amd.from_events     the interaction matrix from an event log (sum / count / max / last, decay, latest timestamps), on the device
  rsparse_amd.Confidence      the confidence transformation of WRMF(preprocess=): BM25, TF-IDF, log, linear, on the device
  rsparse_amd.ScaleNormalize  the reference's ScaleNormalize: p-norm scaling of rows or columns
  rsparse_amd.PureSVD         the reference's PureSVD recommender (R/model_PureSVD.R) with WRMF's inference surface
  rsparse_amd.soft_svd        soft_svd / soft_impute (R/SoftALS.R): soft-thresholded SVD of a sparse matrix by alternating least
                              squares, on a fused residual-SpMM kernel
  rsparse_amd.ItemKNN         item-based k-nearest-neighbours on the co-occurrence of items (cosine, Jaccard, count), integer
                              from end to end: neighbour table and top-k lists on the device, equal to the numpy definition;
                              with weighting= on quantised values: BM25 / TF-IDF cosine, dot, asymmetric cosine, P3alpha / RP3beta
  rsparse_amd.EASE            the closed-form item-item model of Steck 2019: Gram rows and top-k lists under a dense items x items
                              weight matrix on the device, equal to the numpy definition
  rsparse_amd.SLIM            the sparse linear method of Ning and Karypis 2011: a non-negative elastic net per item column by
                              coordinate descent on the device, equal to the numpy definition; EASE's inference surface
  rsparse_amd.BPR             matrix factorisation on the pairwise ranking loss of Rendle et al. 2009 by deterministic mini-batch SGD
                              on the device, equal to the numpy definition; WRMF's inference surface with an SGD fold-in
  rsparse_amd.als             als_implicit()/als_explicit() wrappers over the stateless C ABI
  rsparse_amd.engine          device-resident, row-sharded driver (one process per GPU)
  rsparse_amd.synth           synthetic interaction matrices for the BASELINE configs
The numerics live in csrc/ (HIP, gfx950) and are reached through include/rsparse_wrmf_hip.h.
"""
from . import _lib  # noqa: F401


def __getattr__(name):
    if name == "WRMF":
        from .wrmf import WRMF
        return WRMF
    if name == "train_test_split":
        from .split import train_test_split
        return train_test_split
    if name in ("Confidence", "ScaleNormalize", "confidence_reference"):
        from . import confidence
        return getattr(confidence, name)
    if name in ("from_events", "events_reference"):
        from . import events
        return getattr(events, name)
    if name in ("soft_svd", "soft_impute", "soft_als_reference", "softals_half_reference"):
        from . import softals
        return getattr(softals, name)
    if name == "PureSVD":
        from .puresvd import PureSVD
        return PureSVD
    if name in ("ItemKNN", "cooccurrence_reference", "knn_recommend_reference", "quantize_values", "weighted_operands",
                "weighted_cooccurrence_reference", "knn_score_pairs_reference", "knn_candidates_reference", "knn_ranks_reference"):
        from . import itemknn
        return getattr(itemknn, name)
    if name in ("EASE", "ease_gram_reference", "ease_weights_reference", "ease_scores_reference", "ease_recommend_reference",
                "ease_score_pairs_reference", "ease_candidates_reference", "ease_ranks_reference"):
        from . import ease
        return getattr(ease, name)
    if name in ("SLIM", "slim_columns_reference", "slim_weights_reference"):
        from . import slim
        return getattr(slim, name)
    if name in ("BPR", "bpr_triples", "bpr_step_reference", "bpr_fit_reference"):
        from . import bpr
        return getattr(bpr, name)
    if name == "metrics":
        import importlib
        return importlib.import_module(".metrics", __name__)
    raise AttributeError(name)
