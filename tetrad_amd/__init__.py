"""tetrad_amd -- MI355X-native quartet-invariant engine behind tetrad's worker API.

Only the per-quartet hot path of eaton-lab/tetrad and the callers / consumers either side of it live here
(SURVEY.md section 8): HIP kernels + C ABI in ``csrc/``, the ctypes binding (``_lib``, ``engine``) and host-side
mirrors of the reference's interfaces -- ``resolve_quartets`` (worker), ``distributor`` (dispatch + result gather
over the GPUs of a node), ``replicates`` (bootstrap-replicate loop), ``bootstrap`` (resampler draws),
``combinations`` (quartet producers), ``qmc_format`` / ``qmc`` (wQMC text and the quartet supertree), ``concordance``
(quartet concordance on a fixed tree), ``consensus`` (split counts over many trees, majority-rule consensus),
``scf`` (site concordance factors per branch of a fixed tree), ``tbe`` (transfer bootstrap supports of a tree's
branches over replicate trees), ``treedist`` (all-pairs Robinson-Foulds distances of a set of trees),
``qdist`` (all-pairs quartet distances of a set of trees), ``stability`` (quartet frequencies of a set of trees and the
leaf stability of its taxa), ``distance`` (pairwise taxon counts and distances from the SNP matrix, neighbour-joining
trees and their supports).
Importing the package does not load the HIP library; the first compute call does, and fails loudly if it is missing.
"""
__version__ = "0.2.0"

_SCF_EXPORTS = ("SiteConcordance", "sample_edge_quartets", "run_scf")
_TBE_EXPORTS = ("TransferSupport", "transfer_supports")
_TREEDIST_EXPORTS = ("TreeDistances", "rf_matrix")
_QDIST_EXPORTS = ("QuartetDistances", "quartet_distance_matrix")
_STABILITY_EXPORTS = ("LeafStability", "quartet_frequencies", "dominant_splits")
_DISTANCE_EXPORTS = ("taxon_counts_host", "distances", "sharing", "fill_undefined", "pool_counts", "nj_tree", "nj_parents",
                     "jackknife_nj_trees", "bootstrap_nj_trees", "run_distance_tree")
__all__ = list(_SCF_EXPORTS + _TBE_EXPORTS + _TREEDIST_EXPORTS + _QDIST_EXPORTS + _STABILITY_EXPORTS + _DISTANCE_EXPORTS)


def __getattr__(name):
    # resolved on first use, so that importing the package stays free of NumPy and of the binding
    if name in _SCF_EXPORTS:
        from . import scf
        return getattr(scf, name)
    if name in _TBE_EXPORTS:
        from . import tbe
        return getattr(tbe, name)
    if name in _TREEDIST_EXPORTS:
        from . import treedist
        return getattr(treedist, name)
    if name in _QDIST_EXPORTS:
        from . import qdist
        return getattr(qdist, name)
    if name in _STABILITY_EXPORTS:
        from . import stability
        return getattr(stability, name)
    if name in _DISTANCE_EXPORTS:
        from . import distance
        return getattr(distance, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
