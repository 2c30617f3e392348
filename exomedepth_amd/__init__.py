"""exomedepth_amd -- MI355X (gfx950) CNV-calling core: beta-binomial emissions + 3-state Viterbi.

Only what the hot path needs lives here: csrc/ (HIP kernels + the C-ABI of include/exomedepth_amd.h)
and the host-side mirror of the reference's interface for this path (api.py).
"""
from ._lib import EdError, LIB_PATH  # noqa: F401
from .api import (Batch, Cohort, MultiDevice, DeviceArray, device_count, PinnedArray, ExomeDepth, Plan, Posterior, fit_transitions, fit_prop_tumor, mixture_geometry, chromosome_order, cohort_select_reference_sets, refcohort_last_path, fit_betabin, fit_betabin_bins,  # noqa: F401
                  get_loglike_matrix, get_power_betabinom, refset_finalize, select_reference_set, somatic_CNV_call, viterbi_hmm,
                  correct_counts_using_PCA, pca_gram, pca_last_info,
                  Annotation, annotate_calls, cohort_call_recurrence, annot_geometry,
                  ReadCounter, getBamCounts, count_everted_reads, bed_targets, readcount_geometry,
                  GcCounter, gc_content, gc_geometry,
                  CALL_BOUNDS_DTYPE,
                  PowerMap, detection_power, region_runs, power_geometry, power_from_moments, POWER_DTYPE,
                  QuantileMap, normal_range, qbetabinom, qbetabinom_ab, quantile_geometry,
                  runif53, rbetabinom, rbetabinom_ab, rbetabinom_ab_u, sim_geometry, planted_prob, SimulatedCounts, null_call_table,
                  false_calls_per_sample, NULL_CALL_DTYPE,
                  call_copy_number, copy_number_from_profile, ratio_geometry, CALL_DTYPE, COPY_RATIO_GRID)

__all__ = ["Batch", "Cohort", "MultiDevice", "DeviceArray", "device_count", "PinnedArray", "ExomeDepth", "Plan", "Posterior", "fit_transitions", "fit_prop_tumor", "mixture_geometry", "EdError", "chromosome_order", "cohort_select_reference_sets", "refcohort_last_path", "fit_betabin", "fit_betabin_bins",
           "get_loglike_matrix", "get_power_betabinom", "refset_finalize", "select_reference_set", "somatic_CNV_call", "viterbi_hmm", "LIB_PATH",
           "correct_counts_using_PCA", "pca_gram", "pca_last_info",
           "Annotation", "annotate_calls", "cohort_call_recurrence", "annot_geometry",
           "ReadCounter", "getBamCounts", "count_everted_reads", "bed_targets", "readcount_geometry",
           "GcCounter", "gc_content", "gc_geometry",
           "CALL_BOUNDS_DTYPE",
           "PowerMap", "detection_power", "region_runs", "power_geometry", "power_from_moments", "POWER_DTYPE",
           "QuantileMap", "normal_range", "qbetabinom", "qbetabinom_ab", "quantile_geometry",
           "runif53", "rbetabinom", "rbetabinom_ab", "rbetabinom_ab_u", "sim_geometry", "planted_prob", "SimulatedCounts", "null_call_table",
           "false_calls_per_sample", "NULL_CALL_DTYPE",
           "call_copy_number", "copy_number_from_profile", "ratio_geometry", "CALL_DTYPE", "COPY_RATIO_GRID"]
