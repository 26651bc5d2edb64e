"""ctypes declarations for include/vb2_abi.h (the C-ABI of libvb2.so).

This is the same binding a maintainer of another host language would write (see
INTEGRATION.md); the Python layer adds nothing but marshalling.  If libvb2.so is
missing the import fails loudly -- there is no Python or CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VB2_LIB_PATH") or os.path.join(_PKG, "libvb2.so")      # (VB2_LIB_PATH: A/B builds)

VB2_MAX_PC = 64
VB2_OK = 0
VB2_ERR_INVALID, VB2_ERR_NO_DEVICE, VB2_ERR_HIP, VB2_ERR_IO, VB2_ERR_NOMEM, VB2_ERR_SANITY = \
    -1, -2, -3, -4, -5, -6


class Input(C.Structure):
    _fields_ = [
        ("num_marker", C.c_int32), ("num_pc", C.c_int32),
        ("ud", C.c_void_p), ("means", C.c_void_p), ("read_off", C.c_void_p),
        ("bases", C.c_void_p), ("quals", C.c_void_p), ("alt_base", C.c_void_p),
        ("known_af", C.c_void_p),
        ("avg_depth", C.c_double), ("sd_depth", C.c_double),
        ("sanity_disabled", C.c_int32), ("reserved", C.c_int32),
    ]


class Options(C.Structure):
    _fields_ = [("device", C.c_int32), ("flags", C.c_int32), ("stream", C.c_void_p)]


class Info(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("device", C.c_int32), ("num_marker", C.c_int32),
        ("num_pc", C.c_int32), ("num_active_marker", C.c_int64), ("num_read", C.c_int64),
        ("num_read_other", C.c_int64), ("num_code", C.c_int32), ("num_tile", C.c_int32),
        ("device_bytes", C.c_int64), ("algorithmic_bytes_per_eval", C.c_int64),
        ("device_name", C.c_char * 64), ("arch", C.c_char * 32), ("cohort_step_bytes", C.c_int64),
        ("layout", C.c_int32), ("num_table_row", C.c_int32), ("num_step", C.c_int64),
    ]


class Model(C.Structure):
    _fields_ = [
        ("is_heter", C.c_int32), ("is_pc_fixed", C.c_int32), ("is_alpha_fixed", C.c_int32),
        ("is_af_known", C.c_int32), ("fix_alpha", C.c_double), ("fix_pc", C.c_void_p),
        ("epsilon", C.c_double), ("verbose", C.c_int32), ("notices", C.c_int32),
    ]


class SearchOpts(C.Structure):
    _fields_ = [
        ("num_start", C.c_int32), ("seed", C.c_uint32), ("start_sd", C.c_double),
        ("line_search", C.c_int32), ("reserved", C.c_int32),
    ]


class Estimate(C.Structure):
    _fields_ = [
        ("alpha", C.c_double), ("llk1", C.c_double), ("llk0", C.c_double),
        ("pc", C.c_double * VB2_MAX_PC), ("pc2", C.c_double * VB2_MAX_PC),
        ("num_eval", C.c_int64), ("num_launch_point", C.c_int64),
        ("converged", C.c_int32), ("reserved", C.c_int32),
    ]


VB2_CI_MAX_ROW = 2 * VB2_MAX_PC + 1


class Interval(C.Structure):
    _fields_ = [
        ("freemix", C.c_double), ("freemix_se", C.c_double), ("lo", C.c_double), ("hi", C.c_double),
        ("llk_max", C.c_double), ("llk_lo", C.c_double), ("llk_hi", C.c_double),
        ("alpha_free", C.c_int32), ("num_free", C.c_int32), ("pos_def", C.c_int32), ("num_row", C.c_int32),
        ("row_kind", C.c_int32 * VB2_CI_MAX_ROW), ("row_pc", C.c_int32 * VB2_CI_MAX_ROW),
        ("row_est", C.c_double * VB2_CI_MAX_ROW), ("row_se", C.c_double * VB2_CI_MAX_ROW),
        ("row_lo", C.c_double * VB2_CI_MAX_ROW), ("row_hi", C.c_double * VB2_CI_MAX_ROW),
        ("num_launch", C.c_int64), ("num_profile", C.c_int64),
    ]


class Trace(C.Structure):
    _fields_ = [
        ("capacity", C.c_int64), ("count", C.c_int64),
        ("alpha", C.c_void_p), ("pc1", C.c_void_p), ("pc2", C.c_void_p), ("llk", C.c_void_p),
    ]


class MpileupOpts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("given", "min_bq", "min_mq", "adjust_mq", "max_depth", "no_orphans",
                                          "incl_flags", "excl_flags")]


class RunArgs(C.Structure):
    _fields_ = [
        ("ud_path", C.c_char_p), ("mean_path", C.c_char_p), ("bed_path", C.c_char_p),
        ("pileup_path", C.c_char_p), ("known_af_path", C.c_char_p), ("output_prefix", C.c_char_p),
        ("num_pc", C.c_int32), ("disable_sanity", C.c_int32), ("output_pileup", C.c_int32),
        ("device", C.c_int32), ("model", Model),
        ("devices", C.POINTER(C.c_int32)), ("num_device", C.c_int32), ("bam_adjust", C.c_int32),
        ("bam_path", C.c_char_p), ("reference_path", C.c_char_p), ("search", SearchOpts),
        ("mpileup", MpileupOpts),
    ]


class RunResult(C.Structure):
    _fields_ = [
        ("est", Estimate), ("num_marker", C.c_int32), ("num_site", C.c_int32),
        ("num_bases", C.c_int64), ("avg_depth", C.c_double), ("sd_depth", C.c_double),
        ("seconds_load", C.c_double), ("seconds_optimize", C.c_double),
    ]


class BaqStats(C.Structure):
    """vb2_baq_stats: what --ApplyBAQ did to the records of one load (or of one vb2_baq_records call)."""
    _fields_ = [(n, C.c_int64) for n in ("records", "realigned", "left_alone", "tag_applied", "no_reference", "dropped_outside",
                                          "dropped_cap", "not_asked", "records_lds", "records_global", "undefined_rows",
                                          "fasta_bytes")] + \
               [(n, C.c_double) for n in ("seconds_fasta", "seconds_lds", "seconds_global", "seconds_cap", "seconds_stage")]


class BamStats(C.Structure):
    """vb2_bam_stats: what one --BamFile load through the built-in reader did."""
    _fields_ = [(n, C.c_int64) for n in ("blocks", "bytes_inflated", "chunks", "records_seen", "records_kept",
                                          "long_cigar_skipped", "batches", "entries", "sites", "empty_sites",
                                          "pairs_resolved", "capped_sites")] + \
               [(n, C.c_double) for n in ("seconds_index", "seconds_inflate", "seconds_device", "seconds_copyback")]


class BgzfStats(C.Structure):
    """vb2_bgzf_stats: what the device inflate of this process has done since the last reset."""
    _fields_ = [(n, C.c_int64) for n in ("blocks", "refused", "batches", "bytes_raw", "bytes_inflated")] + \
               [(n, C.c_double) for n in ("seconds_upload", "seconds_kernel", "seconds_copyback", "seconds_stage")]


VB2_BAM_SCAN_GROUPS = 1
VB2_BAM_NO_GROUP = 0xFFFF
VB2_GROUP_NO_BASE = 1


class GroupResult(C.Structure):
    """vb2_group_result: one read group of vb2_run_read_groups."""
    _fields_ = [("run", RunResult), ("status", C.c_int32), ("header_index", C.c_int32), ("records", C.c_int64)]


class CohortArgs(C.Structure):
    _fields_ = [
        ("base", RunArgs), ("num_sample", C.c_int32), ("pileup_paths", C.POINTER(C.c_char_p)),
        ("output_prefixes", C.POINTER(C.c_char_p)), ("group_size", C.c_int32), ("num_host_thread", C.c_int32),
    ]


class ShardInfo(C.Structure):
    _fields_ = [
        ("num_shard", C.c_int32), ("nranks", C.c_int32), ("rank", C.c_int32), ("uses_rccl", C.c_int32),
        ("num_allreduce", C.c_int64), ("marker_lo", C.c_int32 * 64), ("marker_hi", C.c_int32 * 64),
        ("num_read", C.c_int64 * 64), ("partial_sums", C.c_int32), ("rccl_stub", C.c_int32),
    ]


class PanelArgs(C.Structure):
    _fields_ = [
        ("vcf_path", C.c_char_p), ("include_chr", C.c_char_p), ("num_svd_pcs", C.c_int32),
        ("skip_min_sample_count_check", C.c_int32), ("check_minimums", C.c_int32), ("num_thread", C.c_int32),
        ("device", C.c_int32), ("notices", C.c_int32), ("chunk_markers", C.c_int32), ("reserved", C.c_int32),
    ]


class VcfView(C.Structure):
    _fields_ = [
        ("num_marker", C.c_int64), ("num_sample", C.c_int32), ("num_chr", C.c_int32),
        ("genotypes", C.c_void_p), ("pos", C.c_void_p), ("chr_index", C.c_void_p), ("ref", C.c_void_p),
        ("alt", C.c_void_p), ("chr_names", C.POINTER(C.c_char_p)), ("sample_ids", C.POINTER(C.c_char_p)),
    ]


class PanelView(C.Structure):
    _fields_ = [
        ("num_marker", C.c_int64), ("num_sample", C.c_int32), ("num_pc", C.c_int32),
        ("ud", C.c_void_p), ("v", C.c_void_p), ("mu", C.c_void_p), ("sigma", C.c_void_p), ("gram", C.c_void_p),
        ("row_sum", C.c_void_p), ("seconds", C.c_double * 7), ("seconds_total", C.c_double),
    ]


EVAL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                      C.POINTER(C.c_double), C.POINTER(C.c_double))

# vb2_batch_derivs_fn: (user, num_sample, num_point, pc1, pc2, alpha, llk, grad, hess)
BATCH_DERIVS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double),
                              C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                              C.POINTER(C.c_double))

# vb2_replicates_eval_fn: (user, num_rep, num_point, pc1, pc2, alpha, llk)
REPLICATES_EVAL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                 C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))
# vb2_conditioned_eval_fn: (user, num_hyp, num_point, pc1, pc2, alpha, llk)
CONDITIONED_EVAL_FN = REPLICATES_EVAL_FN
# vb2_paired_eval_fn: the same
PAIRED_EVAL_FN = REPLICATES_EVAL_FN
VB2_BATCH_SLOTS = 8
VB2_CHROM_NAME_LEN = 32


class ReplicatesInfo(C.Structure):
    _fields_ = [("num_rep", C.c_int32), ("num_marker", C.c_int32), ("device_bytes", C.c_int64), ("num_step", C.c_int64),
                ("num_launch", C.c_int64)]


VB2_SOURCE_FIT_NONE = 1
VB2_SET_SOURCE, VB2_SET_RELATED = 1, 2
VB2_NUM_RELATION = 4
VB2_REL_DUP, VB2_REL_PO, VB2_REL_FS, VB2_REL_D2 = 0, 1, 2, 3


class SourceFit(C.Structure):
    _fields_ = [("candidate", C.c_int32), ("markers", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, C.c_double) for n in ("llr", "freemix", "freelk1", "alpha_given", "lk1_given", "lk0_given", "delta_lk")]


class ConditionedInfo(C.Structure):
    _fields_ = [("num_hyp", C.c_int32), ("num_marker", C.c_int32), ("device_bytes", C.c_int64), ("num_step", C.c_int64),
                ("num_launch", C.c_int64)]


VB2_PAIR_FIT_NONE = 1


class PairFit(C.Structure):
    _fields_ = [("tumour", C.c_int32), ("normal", C.c_int32), ("markers", C.c_int32), ("status", C.c_int32)] + \
               [(n, C.c_double) for n in ("normal_freemix", "freemix", "freelk1", "alpha_paired", "lk1_paired", "lk0_paired")]


class PairedInfo(C.Structure):
    _fields_ = [("num_hyp", C.c_int32), ("num_marker", C.c_int32), ("device_bytes", C.c_int64), ("num_step", C.c_int64),
                ("num_launch", C.c_int64)]


VB2_REFBIAS_MIN, VB2_REFBIAS_MAX, VB2_REFBIAS_NUM_PAIR = 0.25, 0.75, 28
# vb2_refbias_eval_fn: (user, num_row, num_point, beta, pc1, pc2, alpha, llk)
REFBIAS_EVAL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                              C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))


class RefBiasInfo(C.Structure):
    _fields_ = [("num_row", C.c_int32), ("num_marker", C.c_int32), ("device_bytes", C.c_int64), ("num_step", C.c_int64),
                ("num_launch", C.c_int64)]


class RefBiasFit(C.Structure):
    """vb2_refbias_fit: every llk1 is a log-likelihood (.selfSM's FREELK1)."""
    _fields_ = [(n, C.c_double) for n in ("beta", "beta_se", "alpha_bias", "llk1_bias")] + \
               [("pc", C.c_double * VB2_MAX_PC), ("pc2", C.c_double * VB2_MAX_PC)] + \
               [(n, C.c_double) for n in ("llk1_at_half", "alpha_at_half", "lrt")] + \
               [("pair_beta", C.c_double * VB2_REFBIAS_NUM_PAIR), ("pair_llk1", C.c_double * VB2_REFBIAS_NUM_PAIR),
                ("num_step", C.c_int64)] + \
               [(n, C.c_int32) for n in ("at_bound", "num_round", "num_refit", "num_pair", "status", "reserved")]


VB2_ERR_NUM_QUAL, VB2_ERRFIT_MAX_ITER = 94, 24
# vb2_errfit_fns.eval: (user, err_table, num_point, pc1, pc2, alpha, llk); .stats: (user, err_table, pc1, pc2, alpha, n, s)
ERRFIT_EVAL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                             C.POINTER(C.c_double), C.POINTER(C.c_double))
ERRFIT_STATS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double,
                              C.POINTER(C.c_int64), C.POINTER(C.c_double))


class ErrFitFns(C.Structure):
    _fields_ = [("eval", ERRFIT_EVAL_FN), ("stats", ERRFIT_STATS_FN)]


class ErrStatInfo(C.Structure):
    _fields_ = [("num_marker", C.c_int32), ("num_pc", C.c_int32), ("num_read", C.c_int64), ("device_bytes", C.c_int64),
                ("num_launch", C.c_int64)]


class ErrStatBatchInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_sample", "num_pc", "num_panel", "last_grid")] + \
               [(n, C.c_int64) for n in ("num_marker", "num_read", "device_bytes", "num_launch", "num_eval")]


VB2_ERRSTAT_BATCH_MAX = 64


class ErrFitOpts(C.Structure):
    _fields_ = [("prior_reads", C.c_double), ("tol", C.c_double), ("max_iter", C.c_int32), ("reserved", C.c_int32)]


class ErrFit(C.Structure):
    """vb2_errfit: every llk is a log-likelihood (.selfSM's FREELK1)."""
    _fields_ = [("err", C.c_double * VB2_ERR_NUM_QUAL), ("n", C.c_int64 * VB2_ERR_NUM_QUAL), ("s", C.c_double * VB2_ERR_NUM_QUAL),
                ("est", Estimate)] + \
               [(n, C.c_double) for n in ("llk_fit", "llk_nominal", "alpha_nominal", "lrt")] + \
               [(n, C.c_double * VB2_ERRFIT_MAX_ITER) for n in ("iter_llk", "iter_change", "iter_alpha")] + \
               [("iter_err", (C.c_float * VB2_ERR_NUM_QUAL) * VB2_ERRFIT_MAX_ITER), ("num_step", C.c_int64)] + \
               [(n, C.c_int32) for n in ("num_bin", "num_iter", "converged", "status")]


class ErrFitPool(C.Structure):
    """vb2_errfit_pool: the pooled summary of a cohort's error-rate fit."""
    _fields_ = [("err", C.c_double * VB2_ERR_NUM_QUAL), ("n", C.c_int64 * VB2_ERR_NUM_QUAL), ("s", C.c_double * VB2_ERR_NUM_QUAL),
                ("iter_change", C.c_double * VB2_ERRFIT_MAX_ITER), ("iter_err", (C.c_float * VB2_ERR_NUM_QUAL) * VB2_ERRFIT_MAX_ITER)] + \
               [(n, C.c_double) for n in ("lrt_sum", "seconds_stats", "seconds_context", "seconds_search")] + \
               [("num_step", C.c_int64), ("device_bytes", C.c_int64)] + \
               [(n, C.c_int32) for n in ("num_bin", "num_iter", "converged", "pooled", "num_sample", "num_entered", "num_fitted",
                                         "num_estep")]


# vb2_errfit_cohort_fns.eval: (user, sample, err_table, num_point, pc1, pc2, alpha, llk);
# .stats: (user, num_sample, live, err_tables, pc1, pc2, alpha, n, s)
ERRFIT_COHORT_EVAL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))
ERRFIT_COHORT_STATS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_double))


class ErrFitCohortFns(C.Structure):
    _fields_ = [("eval", ERRFIT_COHORT_EVAL_FN), ("stats", ERRFIT_COHORT_STATS_FN)]


class ReplicateSummary(C.Structure):
    _fields_ = [("num_chrom", C.c_int32), ("num_boot", C.c_int32)] + \
               [(n, C.c_double) for n in ("jack_estimate", "jack_se", "jack_lo", "jack_hi", "boot_mean", "boot_sd",
                                          "boot_p025", "boot_p975")] + \
               [("num_step", C.c_int64), ("seconds", C.c_double)]


# every symbol include/vb2_abi.h declares
SYMBOLS = [
    "vb2_ctx_create", "vb2_ctx_destroy", "vb2_ctx_info", "vb2_llk_eval_batch", "vb2_llk_derivs_batch", "vb2_ctx_interval", "vb2_run_interval",
    "vb2_llk_eval_batch_device", "vb2_ctx_search_begin", "vb2_ctx_search_end", "vb2_optimize_llk", "vb2_ctx_optimize_llk", "vb2_ctx_optimize_llk_ex", "vb2_run", "vb2_cohort_run",
    "vb2_flat_load", "vb2_flat_input", "vb2_flat_stats", "vb2_flat_free", "vb2_last_error",
    "vb2_abi_version", "vb2_device_count",
    "vb2_batch_create", "vb2_batch_destroy", "vb2_batch_eval", "vb2_batch_optimize_llk",
    "vb2_shard_group_create", "vb2_rccl_unique_id", "vb2_shard_group_create_rank", "vb2_shard_group_eval",
    "vb2_shard_group_optimize_llk", "vb2_shard_group_info", "vb2_shard_group_destroy", "vb2_shard_range",
    "vb2_vcf_read", "vb2_vcf_get_view", "vb2_vcf_free", "vb2_panel_build", "vb2_panel_build_genotypes",
    "vb2_panel_get_view", "vb2_panel_write", "vb2_panel_destroy",
    "vb2_ctx_marginals", "vb2_source_set_create", "vb2_source_set_add", "vb2_source_set_scores",
    "vb2_source_set_destroy", "vb2_source_set_size", "vb2_cohort_run_sources",
    "vb2_source_set_create_ex", "vb2_source_set_relations", "vb2_ctx_marginals_related", "vb2_cohort_run_related",
    "vb2_batch_derivs", "vb2_batch_interval", "vb2_intervals_lockstep", "vb2_cohort_run_intervals",
    "vb2_replicates_create", "vb2_replicates_destroy", "vb2_replicates_eval", "vb2_replicates_optimize_llk",
    "vb2_replicates_info_get", "vb2_replicates_lockstep", "vb2_chromosome_weights", "vb2_bootstrap_weights", "vb2_jackknife",
    "vb2_run_replicates",
    "vb2_conditioned_create", "vb2_conditioned_create_from_set", "vb2_conditioned_destroy", "vb2_conditioned_eval",
    "vb2_conditioned_optimize_llk", "vb2_conditioned_info_get", "vb2_conditioned_lockstep", "vb2_cohort_run_source_fits",
    "vb2_paired_create", "vb2_paired_create_from_set", "vb2_paired_destroy", "vb2_paired_eval", "vb2_paired_optimize_llk",
    "vb2_paired_info_get", "vb2_paired_lockstep", "vb2_cohort_run_paired", "vb2_matched_normal_read",
    "vb2_cohort_run_paired_intervals", "vb2_paired_derivs", "vb2_paired_derivs_sets", "vb2_paired_interval", "vb2_paired_intervals_lockstep",
    "vb2_flat_baq_stats", "vb2_baq_records", "vb2_baq_result_num", "vb2_baq_result_qual_bytes", "vb2_baq_result_copy",
    "vb2_baq_result_stats", "vb2_baq_result_free", "vb2_baq_case", "vb2_baq_quantise", "vb2_baq_work_bytes", "vb2_fasta_fetch",
    "vb2_flat_bam_stats", "vb2_bam_scan", "vb2_bam_scan_stats", "vb2_bam_scan_records", "vb2_bam_scan_sample", "vb2_bam_scan_free",
    "vb2_bam_scan_ex", "vb2_bam_scan_num_group", "vb2_bam_scan_group_id", "vb2_bam_scan_record_groups",
    "vb2_flat_load_groups", "vb2_flat_groups_count", "vb2_flat_groups_id", "vb2_flat_groups_records", "vb2_flat_groups_status",
    "vb2_flat_groups_flat", "vb2_flat_groups_unassigned", "vb2_flat_groups_seconds", "vb2_flat_groups_free", "vb2_run_read_groups",
    "vb2_refbias_create", "vb2_refbias_destroy", "vb2_refbias_eval", "vb2_refbias_optimize_llk", "vb2_refbias_info_get",
    "vb2_refbias_fit_ctx", "vb2_refbias_lockstep", "vb2_run_refbias",
    "vb2_bgzf_inflate", "vb2_bgzf_inflate_stats", "vb2_cohort_bam_stats",
    "vb2_ctx_create_ex", "vb2_errstat_create", "vb2_errstat_destroy", "vb2_errstat_eval", "vb2_errstat_info_get",
    "vb2_errfit_input", "vb2_errfit_lockstep", "vb2_run_errfit",
    "vb2_errstat_batch_create", "vb2_errstat_batch_destroy", "vb2_errstat_batch_eval", "vb2_errstat_batch_info_get",
    "vb2_errfit_cohort_inputs", "vb2_errfit_cohort_lockstep", "vb2_cohort_run_errfit",
    "vb2_err_table_read", "vb2_run_under_table", "vb2_cohort_run_under_table",
]

_lib = None


def lib():
    """Load libvb2.so (once).  Raises if it has not been built -- by design."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "verifybamid_amd: %s is missing; build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C verifybamid_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    # PyTorch-ROCm wheels bundle their own libamdhip64/libhsa-runtime64.  Two HIP runtimes
    # in one process cannot both own the device, so when torch is installed it must be
    # loaded FIRST: libvb2.so's NEEDED libamdhip64.so.7 then binds to the copy that is
    # already mapped, and torch streams/events/tensors interoperate with our launches.
    # (The C++ command line never loads torch and uses /opt/rocm's runtime.)
    if os.environ.get("VB2_NO_TORCH", "") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(LIB_PATH)
    L.vb2_last_error.restype = C.c_char_p
    L.vb2_abi_version.restype = C.c_int
    L.vb2_device_count.restype = C.c_int
    L.vb2_ctx_create.argtypes = [C.POINTER(Input), C.POINTER(Options), C.POINTER(C.c_void_p)]
    L.vb2_ctx_destroy.argtypes = [C.c_void_p]
    L.vb2_ctx_destroy.restype = None
    L.vb2_ctx_info.argtypes = [C.c_void_p, C.POINTER(Info)]
    L.vb2_llk_eval_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]
    L.vb2_llk_derivs_batch.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6
    L.vb2_ctx_interval.argtypes = [C.c_void_p, C.POINTER(Model), C.POINTER(Estimate), C.POINTER(Interval)]
    L.vb2_llk_eval_batch_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_void_p]
    L.vb2_cohort_run.argtypes = [C.POINTER(CohortArgs), C.POINTER(RunResult), C.POINTER(C.c_int32)]
    L.vb2_ctx_search_begin.argtypes = [C.c_void_p]
    L.vb2_ctx_search_end.argtypes = [C.c_void_p]
    L.vb2_ctx_search_end.restype = None
    L.vb2_optimize_llk.argtypes = [EVAL_FN, C.c_void_p, C.c_int32, C.POINTER(Model),
                                   C.POINTER(Estimate), C.POINTER(Trace)]
    L.vb2_ctx_optimize_llk_ex.argtypes = [C.c_void_p, C.POINTER(Model), C.POINTER(SearchOpts), C.POINTER(Estimate),
                                          C.c_void_p]
    L.vb2_ctx_optimize_llk.argtypes = [C.c_void_p, C.POINTER(Model), C.POINTER(Estimate),
                                       C.POINTER(Trace)]
    L.vb2_run.argtypes = [C.POINTER(RunArgs), C.POINTER(RunResult)]
    L.vb2_run_interval.argtypes = [C.POINTER(RunArgs), C.POINTER(RunResult), C.POINTER(Interval)]
    L.vb2_flat_load.argtypes = [C.POINTER(RunArgs), C.POINTER(C.c_void_p)]
    L.vb2_flat_input.argtypes = [C.c_void_p]
    L.vb2_flat_input.restype = C.POINTER(Input)
    L.vb2_flat_stats.argtypes = [C.c_void_p, C.POINTER(RunResult)]
    L.vb2_flat_free.argtypes = [C.c_void_p]
    L.vb2_flat_free.restype = None
    L.vb2_flat_bam_stats.argtypes = [C.c_void_p, C.POINTER(BamStats)]
    L.vb2_flat_baq_stats.argtypes = [C.c_void_p, C.POINTER(BaqStats)]
    L.vb2_baq_records.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(MpileupOpts), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.vb2_baq_result_num.argtypes = [C.c_void_p]
    L.vb2_baq_result_num.restype = C.c_int64
    L.vb2_baq_result_qual_bytes.argtypes = [C.c_void_p]
    L.vb2_baq_result_qual_bytes.restype = C.c_int64
    L.vb2_baq_result_copy.argtypes = [C.c_void_p] * 6
    L.vb2_baq_result_stats.argtypes = [C.c_void_p, C.POINTER(BaqStats)]
    L.vb2_baq_result_free.argtypes = [C.c_void_p]
    L.vb2_baq_result_free.restype = None
    L.vb2_baq_case.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                               C.POINTER(C.c_int32)]
    L.vb2_baq_quantise.argtypes = [C.c_double]
    L.vb2_baq_quantise.restype = C.c_int32
    L.vb2_baq_work_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.vb2_baq_work_bytes.restype = C.c_uint64
    L.vb2_fasta_fetch.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]
    L.vb2_bam_scan.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
    L.vb2_bam_scan_stats.argtypes = [C.c_void_p, C.POINTER(BamStats)]
    L.vb2_bam_scan_records.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.vb2_bam_scan_records.restype = C.c_int64
    L.vb2_bam_scan_sample.argtypes = [C.c_void_p]
    L.vb2_bam_scan_sample.restype = C.c_char_p
    L.vb2_bam_scan_free.argtypes = [C.c_void_p]
    L.vb2_bam_scan_free.restype = None
    L.vb2_bam_scan_ex.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.vb2_bam_scan_num_group.argtypes = [C.c_void_p]
    L.vb2_bam_scan_num_group.restype = C.c_int32
    L.vb2_bam_scan_group_id.argtypes = [C.c_void_p, C.c_int32]
    L.vb2_bam_scan_group_id.restype = C.c_char_p
    L.vb2_bam_scan_record_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.vb2_bam_scan_record_groups.restype = C.c_int64
    L.vb2_bgzf_inflate.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_int32,
                                   C.POINTER(C.c_int32)]
    L.vb2_bgzf_inflate_stats.argtypes = [C.POINTER(BgzfStats), C.c_int32]
    L.vb2_cohort_bam_stats.argtypes = [C.c_int32, C.POINTER(BamStats)]
    L.vb2_flat_load_groups.argtypes = [C.POINTER(RunArgs), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.vb2_flat_groups_count.argtypes = [C.c_void_p]
    L.vb2_flat_groups_count.restype = C.c_int32
    L.vb2_flat_groups_id.argtypes = [C.c_void_p, C.c_int32]
    L.vb2_flat_groups_id.restype = C.c_char_p
    L.vb2_flat_groups_records.argtypes = [C.c_void_p, C.c_int32]
    L.vb2_flat_groups_records.restype = C.c_int64
    L.vb2_flat_groups_status.argtypes = [C.c_void_p, C.c_int32]
    L.vb2_flat_groups_status.restype = C.c_int32
    L.vb2_flat_groups_flat.argtypes = [C.c_void_p, C.c_int32]
    L.vb2_flat_groups_flat.restype = C.c_void_p
    L.vb2_flat_groups_unassigned.argtypes = [C.c_void_p]
    L.vb2_flat_groups_unassigned.restype = C.c_int64
    L.vb2_flat_groups_seconds.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.vb2_flat_groups_free.argtypes = [C.c_void_p]
    L.vb2_flat_groups_free.restype = None
    L.vb2_run_read_groups.argtypes = [C.POINTER(RunArgs), C.POINTER(RunResult), C.c_int32, C.POINTER(GroupResult), C.POINTER(C.c_int32)]
    L.vb2_batch_create.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p)]
    L.vb2_batch_destroy.argtypes = [C.c_void_p]
    L.vb2_batch_destroy.restype = None
    L.vb2_batch_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vb2_batch_optimize_llk.argtypes = [C.c_void_p, C.POINTER(Model), C.c_int32, C.POINTER(Estimate)]
    L.vb2_shard_group_create.argtypes = [C.POINTER(Input), C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_void_p)]
    L.vb2_rccl_unique_id.argtypes = [C.c_void_p]
    L.vb2_shard_group_create_rank.argtypes = [C.POINTER(Input), C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                              C.POINTER(C.c_void_p)]
    L.vb2_shard_group_eval.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vb2_shard_group_optimize_llk.argtypes = [C.c_void_p, C.POINTER(Model), C.POINTER(Estimate), C.POINTER(Trace)]
    L.vb2_shard_group_info.argtypes = [C.c_void_p, C.POINTER(ShardInfo)]
    L.vb2_shard_range.argtypes = [C.POINTER(Input), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.vb2_shard_group_destroy.argtypes = [C.c_void_p]
    L.vb2_shard_group_destroy.restype = None
    L.vb2_vcf_read.argtypes = [C.POINTER(PanelArgs), C.POINTER(C.c_void_p)]
    L.vb2_vcf_get_view.argtypes = [C.c_void_p, C.POINTER(VcfView)]
    L.vb2_vcf_free.argtypes = [C.c_void_p]
    L.vb2_vcf_free.restype = None
    L.vb2_panel_build.argtypes = [C.POINTER(PanelArgs), C.POINTER(C.c_void_p)]
    L.vb2_panel_build_genotypes.argtypes = [C.POINTER(PanelArgs), C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]
    L.vb2_panel_get_view.argtypes = [C.c_void_p, C.POINTER(PanelView)]
    L.vb2_panel_write.argtypes = [C.c_void_p, C.c_char_p]
    L.vb2_panel_destroy.argtypes = [C.c_void_p]
    L.vb2_panel_destroy.restype = None
    L.vb2_ctx_marginals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vb2_source_set_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.vb2_source_set_create_ex.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.vb2_source_set_relations.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.vb2_ctx_marginals_related.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    L.vb2_cohort_run_related.argtypes = [C.POINTER(CohortArgs), C.c_int32, C.c_int32, C.POINTER(RunResult), C.POINTER(C.c_int32),
                                         C.c_void_p, C.c_void_p]
    L.vb2_source_set_add.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Model), C.POINTER(Estimate), C.POINTER(C.c_int32)]
    L.vb2_source_set_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.vb2_source_set_size.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.vb2_source_set_destroy.argtypes = [C.c_void_p]
    L.vb2_source_set_destroy.restype = None
    L.vb2_cohort_run_sources.argtypes = [C.POINTER(CohortArgs), C.c_int32, C.POINTER(RunResult), C.POINTER(C.c_int32),
                                         C.c_void_p, C.c_void_p]
    L.vb2_batch_derivs.argtypes = [C.c_void_p] + [C.c_void_p] * 7
    L.vb2_batch_interval.argtypes = [C.c_void_p, C.POINTER(Model), C.c_int32, C.POINTER(Estimate), C.POINTER(Interval),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.vb2_intervals_lockstep.argtypes = [BATCH_DERIVS_FN, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                         C.POINTER(Model), C.c_int32, C.POINTER(Estimate), C.POINTER(Interval),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.vb2_cohort_run_intervals.argtypes = [C.POINTER(CohortArgs), C.c_int32, C.POINTER(RunResult), C.POINTER(C.c_int32),
                                           C.POINTER(Interval)]
    L.vb2_replicates_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
    L.vb2_replicates_destroy.argtypes = [C.c_void_p]
    L.vb2_replicates_destroy.restype = None
    L.vb2_replicates_eval.argtypes = [C.c_void_p] * 6
    L.vb2_replicates_optimize_llk.argtypes = [C.c_void_p, C.POINTER(Model), C.POINTER(Estimate), C.POINTER(C.c_int32)]
    L.vb2_replicates_info_get.argtypes = [C.c_void_p, C.POINTER(ReplicatesInfo), C.c_void_p]
    L.vb2_replicates_lockstep.argtypes = [REPLICATES_EVAL_FN, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(Model),
                                          C.POINTER(Estimate), C.POINTER(C.c_int32)]
    L.vb2_chromosome_weights.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32)] + [C.c_void_p] * 5
    L.vb2_bootstrap_weights.argtypes = [C.c_int32, C.c_int32, C.c_uint32, C.c_void_p]
    L.vb2_jackknife.argtypes = [C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.vb2_run_replicates.argtypes = [C.POINTER(RunArgs), C.c_int32, C.c_int32, C.POINTER(RunResult),
                                     C.POINTER(ReplicateSummary)]
    L.vb2_cohort_run_source_fits.argtypes = [C.POINTER(CohortArgs), C.c_int32, C.POINTER(RunResult), C.POINTER(C.c_int32),
                                             C.c_void_p, C.c_void_p, C.POINTER(SourceFit)]
    L.vb2_conditioned_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
    L.vb2_conditioned_create_from_set.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
    L.vb2_conditioned_destroy.argtypes = [C.c_void_p]
    L.vb2_conditioned_destroy.restype = None
    L.vb2_conditioned_eval.argtypes = [C.c_void_p] * 6
    L.vb2_conditioned_optimize_llk.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(Model), C.c_void_p,
                                               C.POINTER(Estimate), C.POINTER(C.c_int32)]
    L.vb2_conditioned_info_get.argtypes = [C.c_void_p, C.POINTER(ConditionedInfo)]
    L.vb2_conditioned_lockstep.argtypes = [CONDITIONED_EVAL_FN, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(Model), C.c_void_p,
                                           C.POINTER(Estimate), C.POINTER(C.c_int32)]
    L.vb2_debug_conditioned_time.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    L.vb2_paired_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
    L.vb2_paired_create_from_set.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.POINTER(C.c_void_p)]
    L.vb2_paired_destroy.argtypes = [C.c_void_p]
    L.vb2_paired_destroy.restype = None
    L.vb2_paired_eval.argtypes = [C.c_void_p] * 6
    L.vb2_paired_optimize_llk.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(Model), C.c_void_p,
                                          C.POINTER(Estimate), C.POINTER(C.c_int32)]
    L.vb2_paired_info_get.argtypes = [C.c_void_p, C.POINTER(PairedInfo), C.c_void_p]
    L.vb2_paired_lockstep.argtypes = [PAIRED_EVAL_FN, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(Model), C.c_void_p,
                                      C.POINTER(Estimate), C.POINTER(C.c_int32)]
    L.vb2_paired_derivs.argtypes = [C.c_void_p] * 8
    L.vb2_paired_derivs_sets.argtypes = [C.POINTER(C.c_void_p), C.c_int32] + [C.c_void_p] * 7
    L.vb2_paired_interval.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(Model), C.c_void_p, C.POINTER(Estimate),
                                      C.POINTER(Interval), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.vb2_paired_intervals_lockstep.argtypes = [BATCH_DERIVS_FN, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                                C.POINTER(Model), C.c_int32, C.c_void_p, C.POINTER(Estimate),
                                                C.POINTER(Interval), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.vb2_cohort_run_paired.argtypes = [C.POINTER(CohortArgs), C.c_int32, C.c_void_p, C.c_void_p, C.c_double,
                                        C.POINTER(RunResult), C.POINTER(C.c_int32), C.POINTER(PairFit)]
    L.vb2_cohort_run_paired_intervals.argtypes = [C.POINTER(CohortArgs), C.c_int32, C.c_void_p, C.c_void_p, C.c_double,
                                                  C.POINTER(RunResult), C.POINTER(C.c_int32), C.POINTER(PairFit),
                                                  C.POINTER(Interval)]
    L.vb2_matched_normal_read.argtypes = [C.c_char_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_void_p,
                                          C.c_void_p]
    L.vb2_refbias_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
    L.vb2_refbias_destroy.argtypes = [C.c_void_p]
    L.vb2_refbias_destroy.restype = None
    L.vb2_refbias_eval.argtypes = [C.c_void_p] * 6
    L.vb2_refbias_optimize_llk.argtypes = [C.c_void_p, C.POINTER(Model), C.POINTER(Estimate), C.POINTER(C.c_int32)]
    L.vb2_refbias_info_get.argtypes = [C.c_void_p, C.POINTER(RefBiasInfo)]
    L.vb2_refbias_fit_ctx.argtypes = [C.c_void_p, C.POINTER(Model), C.POINTER(RefBiasFit)]
    L.vb2_refbias_lockstep.argtypes = [REFBIAS_EVAL_FN, C.c_void_p, C.c_int32, C.POINTER(Model), C.c_int32, C.POINTER(RefBiasFit)]
    L.vb2_run_refbias.argtypes = [C.POINTER(RunArgs), C.POINTER(RunResult), C.POINTER(RefBiasFit)]
    L.vb2_debug_refbias_time.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    L.vb2_ctx_create_ex.argtypes = [C.POINTER(Input), C.POINTER(Options), C.c_void_p, C.POINTER(C.c_void_p)]
    L.vb2_errstat_create.argtypes = [C.POINTER(Input), C.POINTER(Options), C.POINTER(C.c_void_p)]
    L.vb2_errstat_destroy.argtypes = [C.c_void_p]
    L.vb2_errstat_destroy.restype = None
    L.vb2_errstat_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vb2_errstat_info_get.argtypes = [C.c_void_p, C.POINTER(ErrStatInfo)]
    L.vb2_errstat_batch_create.argtypes = [C.POINTER(C.POINTER(Input)), C.c_int32, C.POINTER(Options), C.POINTER(C.c_void_p)]
    L.vb2_errstat_batch_destroy.argtypes = [C.c_void_p]
    L.vb2_errstat_batch_destroy.restype = None
    L.vb2_errstat_batch_eval.argtypes = [C.c_void_p] * 9
    L.vb2_errstat_batch_info_get.argtypes = [C.c_void_p, C.POINTER(ErrStatBatchInfo)]
    L.vb2_err_table_read.argtypes = [C.c_char_p, C.c_void_p, C.POINTER(C.c_int32)]
    L.vb2_run_under_table.argtypes = [C.POINTER(RunArgs), C.c_void_p, C.POINTER(RunResult)]
    L.vb2_cohort_run_under_table.argtypes = [C.POINTER(CohortArgs), C.c_void_p, C.POINTER(RunResult), C.POINTER(C.c_int32)]
    L.vb2_cohort_run_errfit.argtypes = [C.POINTER(CohortArgs), C.POINTER(ErrFitOpts), C.c_int32, C.POINTER(RunResult),
                                        C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]
    L.vb2_errfit_cohort_inputs.argtypes = [C.POINTER(C.POINTER(Input)), C.c_int32, C.POINTER(Options), C.POINTER(Model), C.c_void_p,
                                           C.c_void_p, C.POINTER(ErrFitOpts), C.c_int32, C.c_void_p, C.POINTER(ErrFitPool)]
    L.vb2_errfit_cohort_lockstep.argtypes = [C.POINTER(ErrFitCohortFns), C.c_void_p, C.c_int32, C.c_int32, C.POINTER(Model), C.c_int32,
                                             C.c_void_p, C.c_void_p, C.POINTER(ErrFitOpts), C.c_int32, C.c_void_p,
                                             C.POINTER(ErrFitPool)]
    L.vb2_errfit_input.argtypes = [C.POINTER(Input), C.POINTER(Options), C.POINTER(Model), C.POINTER(Estimate), C.POINTER(ErrFitOpts),
                                   C.POINTER(ErrFit)]
    L.vb2_errfit_lockstep.argtypes = [C.POINTER(ErrFitFns), C.c_void_p, C.c_int32, C.POINTER(Model), C.c_int32, C.POINTER(Estimate),
                                      C.POINTER(ErrFitOpts), C.POINTER(ErrFit)]
    L.vb2_run_errfit.argtypes = [C.POINTER(RunArgs), C.POINTER(ErrFitOpts), C.POINTER(RunResult), C.POINTER(ErrFit)]
    L.vb2_debug_paired_time.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    L.vb2_debug_paired_derivs_time.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    L.vb2_debug_replicates_time.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    L.vb2_debug_set_tunable.argtypes = [C.c_char_p, C.c_int]
    L.vb2_debug_get_tunable.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    _lib = L
    return L


def set_tunable(name, value):
    """A run-time switch of the library by name (csrc/tunables.h): tests and measurement scripts only."""
    if lib().vb2_debug_set_tunable(name.encode(), int(value)) != VB2_OK:
        raise KeyError("libvb2 has no tunable %r" % name)


def get_tunable(name):
    v = C.c_int(0)
    if lib().vb2_debug_get_tunable(name.encode(), C.byref(v)) != VB2_OK:
        raise KeyError("libvb2 has no tunable %r" % name)
    return v.value


class Vb2Error(RuntimeError):
    def __init__(self, code, where):
        msg = lib().vb2_last_error()
        super().__init__("%s failed (%d): %s" % (where, code, msg.decode() if msg else ""))
        self.code = code


def check(code, where):
    if code != VB2_OK:
        raise Vb2Error(code, where)


def kernel_source_hash():
    """sha256 (16 hex digits) over the sources of the evaluation kernels: what ties a PMC-derived figure kept under profiles/
    (instruction counts, HBM-side bytes) to the code it was measured on -- bench.py drops figures whose hash is another."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    for name in ("eval_body.h", "llk_kernels.hip", "llk_passes.hip", "resident_kernel.inc", "llk_kernels.h", "kernel_debug.h", "log_table.inc", "Makefile"):
        with open(os.path.join(d, name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]
