"""densityflows.jl_amd — MI355X-native (gfx950) hot path of DensityFlows.jl.

The Python host side mirrors the reference's Julia API (FlowChain,
CouplingLayer, CouplingBlock, NormalizationLayer, Flow, forward / backward /
forward!, logpdf, sample); every evaluation runs in the fused HIP kernels of
``libdensityflows_hip.so`` through its C ABI (include/densityflows_hip.h).

Import as ``densityflows_amd`` (a symlink to this directory at the repo root).
"""
from . import _lib
from ._lib import (ArgumentError, DimensionMismatch, HIPError, HIPLibraryError, UnsupportedError)
from .axes import CouplingAxes, is_reverse, reverse
from .chains import FlowChain, backward, concatenate, forward, forward_, forward_inplace
from .data import (DataArrays, DataPartition, MetaData, dflt_theta, maximum_theta, minimum_theta,
                   normalize_input, resize_output)
from .flows import (HIST_MAX_BINS, HIST_MAX_TABLES, HIST_SPLIT_DRAWS, QUANT_MAX_ORDERS, Box, Flow, HalfSpaces,
                    ImportanceWeights, MvNormal, PointHistograms, PointStats, Region, ScoreMoments,
                    WeightedPointStats, credible_intervals, importance_posterior_stats, importance_weights,
                    posterior_draws, weighted_moments_from_sums, weighted_stats,
                    RESAMPLE_LDS_DRAWS, RESAMPLE_METHODS, importance_resample, resample, resample_indices,
                    WHIST_MAX_TABLE_BINS, WQUANT_MAX_PROBS, WeightedPointHistograms, importance_credible_intervals,
                    importance_posterior_histograms, importance_posterior_quantiles, quantile_numerators,
                    weight_scale, weighted_credible_intervals, weighted_histograms, weighted_quantiles,
                    draw_histograms, entropy, expected_coverage, fisher_information, histogram_edges, hpd_levels,
                    logpdf,
                    logpdf_grad, logpdf_grid, nll_partial_sum, order_statistics, pdf, pdf_marginals,
                    posterior_histograms, posterior_quantiles, posterior_stats, predict, quantile_orders, sample, sample_logpdf,
                    sample_with_rejection, sbc_histogram, sbc_ranks, score_moments, training_loss,
                    trapezoid_weights, validation_loss)
from .layers import (Chain, CouplingBlock, CouplingLayer, Dense, FlowElement, NICECouplingLayer,
                     NormalizationLayer, RNVPCouplingLayer, default_net)
from .train import (Adam, AdamW, ClipGrad, ClipNorm, Descent, OptimiserChain, TrainState, WeightDecay, adjust_,
                    check_weights, load_trainables, setup, train_, trainables, weighted_nll)

__version__ = "0.1.0"


def summarize(obj) -> str:
    """``summarize`` / ``@summary`` — returns the text the reference prints."""
    return obj.summarize()


def library_path() -> str:
    return _lib.LIB_PATH


def load_library():
    """Load the native library (raises HIPLibraryError if it was not built)."""
    return _lib.load()
