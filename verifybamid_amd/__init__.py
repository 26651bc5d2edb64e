"""verifybamid_amd -- MI355X-native contamination-likelihood core for VerifyBamID2.

The product is libvb2.so (HIP kernels + C++ host, C-ABI in include/vb2_abi.h) and the
`bin/VerifyBamID` command line; this package is the ctypes marshalling used by the
tests, the bench and multi-GPU (torch.distributed) drivers.
"""
from .api import (CohortBatch, LikelihoodContext, PileupData, ShardGroup, SourceSet, intervals_with_evaluator,  # noqa: F401
                  optimize_with_evaluator, Replicates, replicates_with_evaluator, Conditioned, conditioned_with_evaluator, RefBias, refbias_with_evaluator, Paired, paired_with_evaluator, paired_intervals_with_evaluator, chromosome_weights, bootstrap_weights,
                  jackknife, ErrStat, ErrStatBatch, errfit, errfit_cohort, errfit_cohort_with_evaluator, SearchFailed, errfit_with_evaluator, nominal_err_table, read_err_table,
                  run_cohort_files, run_files, read_vcf, build_panel, build_panel_from_genotypes)
from . import synth  # noqa: F401

__all__ = ["CohortBatch", "LikelihoodContext", "PileupData", "ShardGroup", "SourceSet", "intervals_with_evaluator", "optimize_with_evaluator", "run_cohort_files",
           "run_files", "synth", "Replicates", "replicates_with_evaluator", "Conditioned", "conditioned_with_evaluator", "RefBias", "refbias_with_evaluator", "Paired", "paired_with_evaluator", "paired_intervals_with_evaluator", "chromosome_weights", "bootstrap_weights", "jackknife", "ErrStat", "ErrStatBatch", "errfit", "errfit_cohort", "errfit_cohort_with_evaluator", "SearchFailed", "errfit_with_evaluator", "nominal_err_table", "read_err_table", "read_vcf", "build_panel", "build_panel_from_genotypes"]
