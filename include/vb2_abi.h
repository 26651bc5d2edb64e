/*
 * vb2_abi.h -- C-ABI of the MI355X-native contamination-likelihood core.
 *
 * This is the drop-in boundary for the one hot path of VerifyBamID2
 * (Griffan/VerifyBamID): the genotype-mixture log-likelihood
 * FullLLKFunc::ComputeMixLLKs and the Nelder-Mead search that drives it.
 * The reference has no FFI layer; its seam for this path is the libStatGen
 * functor  VectorFunc::Evaluate(Vector&)  (statgen/MathVector.h:281-308),
 * installed with  myMinimizer.func = &fn  (ContaminationEstimator.cpp:212,246,
 * 279,304,325), and one level below it the pure-compute member
 *   double ComputeMixLLKs(const std::vector<double>& pc1,
 *                         const std::vector<double>& pc2, double alpha)
 * (ContaminationEstimator.h:194-195).  Each entry point below names the
 * reference interface it replaces (file:line relative to the reference root).
 *
 * Conventions: plain pointers and sizes, no C++ or torch types; every function
 * returns 0 on success and a negative vb2_status otherwise and never throws;
 * vb2_last_error() gives the message for the calling thread.  A context is
 * thread-compatible (one thread at a time), like the reference's estimator.
 * All arithmetic on the path is IEEE-754 binary64.
 *
 * There is NO CPU fallback: every compute entry point fails with
 * VB2_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef VB2_ABI_H_
#define VB2_ABI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VB2_ABI_VERSION 7

typedef enum vb2_status {
    VB2_OK = 0,
    VB2_ERR_INVALID = -1,    /* bad argument                                     */
    VB2_ERR_NO_DEVICE = -2,  /* no usable HIP device / kernel image not loadable */
    VB2_ERR_HIP = -3,        /* a HIP runtime call failed                        */
    VB2_ERR_IO = -4,         /* file could not be read / written                 */
    VB2_ERR_NOMEM = -5,
    VB2_ERR_SANITY = -6      /* marker sanity check failed (main.cpp:371-379)    */
} vb2_status;

typedef struct vb2_ctx vb2_ctx;

/* ------------------------------------------------------------------------- *
 * 1. Likelihood context: the data ComputeMixLLKs reaches through `ptr`
 *    (ContaminationEstimator.h:82, 236-276), handed over ONCE.
 *
 *    Markers are in panel order (= row order of .UD/.mu/.bed).  read_off has
 *    num_marker+1 entries; marker i owns bases/quals[read_off[i]..read_off[i+1]).
 *    An empty range means "marker absent from the pileup" (baseInfoIndex < 0,
 *    h:239) or depth 0 (h:244).  bases are the pileup characters
 *    ". , A C G T N a c g t n" and quals are ASCII Phred+33, exactly as
 *    SimplePileupViewer stores them (SimplePileupViewer.h:60-61,94-95).
 *    All arrays are caller-owned host memory and may be freed after
 *    vb2_ctx_create returns.
 * ------------------------------------------------------------------------- */
typedef struct vb2_input {
    int32_t num_marker;        /* NumMarker                         (h:446)        */
    int32_t num_pc;            /* numPC                             (h:49)         */
    const double *ud;          /* UD[i][k], row-major M x num_pc    (h:452)        */
    const double *means;       /* means[i]                          (h:454)        */
    const int64_t *read_off;   /* [M+1]                                            */
    const char *bases;         /* viewer.baseInfo, concatenated in panel order     */
    const char *quals;         /* viewer.qualInfo                                  */
    const char *alt_base;      /* resolvedMarkers[i].altBase        (h:472)        */
    const double *known_af;    /* resolvedMarkers[i].knownAFValue or NULL (h:473)  */
    double avg_depth;          /* viewer.avgDepth                                  */
    double sd_depth;           /* viewer.sdDepth                                   */
    int32_t sanity_disabled;   /* isSanityCheckDisabled: skips the +-3sd filter of h:246-249 */
    int32_t reserved;
} vb2_input;

typedef struct vb2_options {
    int32_t device;            /* HIP device ordinal, -1 = current device          */
    int32_t flags;             /* VB2_OPT_* bits                                   */
#define VB2_OPT_COHORT_LAYOUT 1   /* also keep the 16-bit run lists that vb2_batch_* steps stream (half the bytes
                                   * per sample and step; +28 % device memory).  Without it vb2_batch_create
                                   * builds them on first use. */
/* (ABI 6) how vb2_ctx_optimize_llk runs on this context -- the defaults are the fast way; results are the same bits:   */
#define VB2_OPT_PLAIN_LAUNCH 2    /* the resident search kernel goes up with a plain launch instead of a cooperative one (the
                                   * library does this by itself under rocprofv3, whose exit handler does not survive a
                                   * cooperative launch in ROCm 7.2)                                                     */
#define VB2_OPT_HOST_SEARCH 4     /* the simplex decisions stay on the host (the resident kernel only evaluates)        */
#define VB2_OPT_LAUNCH_PER_STEP 8 /* no resident kernel at all: one launch per search step                               */
    void *stream;              /* hipStream_t to run on; NULL = context-owned      */
} vb2_options;

typedef struct vb2_info {
    int32_t abi_version;
    int32_t device;
    int32_t num_marker;        /* panel markers                                    */
    int32_t num_pc;
    int64_t num_active_marker; /* markers that survive h:239-249                   */
    int64_t num_read;          /* bases of the active markers                      */
    int64_t num_read_other;    /* of those, class "other" (folded into a constant) */
    int32_t num_code;          /* distinct (class, quality) pairs in the data      */
    int32_t num_tile;          /* 16-marker micro-tiles                            */
    int64_t device_bytes;      /* HBM held by the context                          */
    /* SURVEY 8(d) algorithmic bytes of ONE evaluation: 2*R + M_active*(8k+12) */
    int64_t algorithmic_bytes_per_eval;
    char device_name[64];
    char arch[32];
    /* (ABI 4) HBM bytes ONE lock-step cohort step (vb2_batch_*) reads of this sample: run lists (16-bit
     * once built, see VB2_OPT_COHORT_LAYOUT) + tile records + panel rows + per-marker constants */
    int64_t cohort_step_bytes;
    /* (ABI 7) how the sample is laid out in HBM: 1 = probability domain -- the per-alpha table holds the powers P^n of
     * P(read | genotype pair, alpha) per quality and a marker's likelihoods are PRODUCTS of table rows, one step per row: no
     * exp() per genotype pair (ContaminationEstimator.h:288-311 sums logarithms and exponentiates) -- taken when no marker's
     * products can leave the normal double range; 0 = run words and sums of logarithms (any depth, quality 0).  The
     * values agree to rounding either way.  num_table_row: rows of the per-alpha table. */
    int32_t layout;
    int32_t num_table_row;
    /* read-loop steps per evaluation point, summed over the markers, the tiles' padding included: each reads one 48-byte
     * table row from LDS (the LDS side of bench.py's roofline) */
    int64_t num_step;
} vb2_info;

/* Builds the device-resident SoA form of the input (classification, quality
 * clamping, marker filtering and the alpha-independent partial sums happen
 * here, once -- on the device: the arrays of `in` go up as they are, through
 * one pinned staging copy and hipMemcpyAsync on the context's stream, and
 * kernels classify, run-length code and pack them; the host keeps the
 * dictionary and the sort of the markers).  Replaces BuildResolvedMarkers + the
 * per-call prologue of ComputeMixLLKs (ContaminationEstimator.cpp:67-86;
 * h:236-249, 285-299).  `in` is not referenced after the call returns.
 * Limits (VB2_ERR_INVALID beyond them; the reference has none short of memory): 2^29 - 1024 markers and 2^25 rows of
 * run words -- a row is the k-th and (k+1)-th distinct (class, quality) pairs of 16 depth-sorted markers, so the second
 * is about a billion reads of one sample: the kernels address both by 32-bit byte offsets. */
int vb2_ctx_create(const vb2_input *in, const vb2_options *opt, vb2_ctx **out);
void vb2_ctx_destroy(vb2_ctx *ctx);
int vb2_ctx_info(const vb2_ctx *ctx, vb2_info *info);

/* Replaces  ComputeMixLLKs(pc1, pc2, alpha)  (ContaminationEstimator.h:194-314)
 * for B parameter points at once.  pc1/pc2 are B x num_pc row-major, alpha has
 * B entries, llk_out receives B values of +LLK (not negated, like the
 * reference's return value).  Synchronous; host pointers. */
int vb2_llk_eval_batch(vb2_ctx *ctx, int32_t num_point, const double *pc1,
                       const double *pc2, const double *alpha, double *llk_out);

/* Derivatives of  ComputeMixLLKs(pc1, pc2, alpha)  (ContaminationEstimator.h:194-314) at B points: llk_out[B] as
 * vb2_llk_eval_batch returns it, grad_out[B][2k+1] and hess_out[B][2k+1][2k+1] (row-major, symmetric) with respect to
 * (pc1[0..k), pc2[0..k), alpha).  It differentiates the table entries (h:223-224) in alpha, the genotype priors (h:186-192;
 * 0 where the reference clamps the allele frequency) and the projection AF = (UD pc + mean) / 2 (h:251-267); a marker counts
 * where its likelihood is > 0 (h:310).  --KnownAF: the PC entries are 0.  At alpha = 0 or 1 the LLK and the PC entries are
 * exact; the alpha entries there are not defined (they may be NaN).  Synchronous; host pointers; not between
 * vb2_ctx_search_begin and vb2_ctx_search_end. */
int vb2_llk_derivs_batch(vb2_ctx *ctx, int32_t num_point, const double *pc1, const double *pc2,
                         const double *alpha, double *llk_out, double *grad_out, double *hess_out);

/* Same evaluation with DEVICE pointers, enqueued on `stream` (NULL = the
 * context's stream) without any host synchronisation:
 *   d_points : num_point x (2*num_pc+1) doubles, each row = pc1[0..k) pc2[0..k) alpha
 *   d_llk_out: num_point doubles
 * Used by the multi-GPU path (the caller all-reduces d_llk_out over RCCL) and by
 * the bench. */
int vb2_llk_eval_batch_device(vb2_ctx *ctx, int32_t num_point, const double *d_points,
                              double *d_llk_out, void *stream);

/* Brackets a series of dependent vb2_llk_eval_batch calls on one context -- a search driven by
 * the caller's own optimiser, e.g. the reference's AmoebaMinimizer calling Evaluate once per
 * point (MathGenMin.cpp:389-421).  Between begin and end the evaluations are served by a kernel
 * that stays resident on the device and is fed through pinned host memory, which
 * saves the launch latency of every call (~7 us of ~22 us for one point at 100 k markers).
 * Results are identical to unbracketed calls.  begin never fails the search: when the mode is
 * unavailable it returns VB2_OK and the calls simply launch kernels as usual.  Only
 * vb2_llk_eval_batch may be called on the context between the two; vb2_ctx_optimize_llk does this
 * bracketing itself. */
int vb2_ctx_search_begin(vb2_ctx *ctx);
void vb2_ctx_search_end(vb2_ctx *ctx);

/* ------------------------------------------------------------------------- *
 * 2. Estimator: FullLLKFunc::Initialize/Evaluate/CalculateLLK0 and
 *    ContaminationEstimator::OptimizeLLK with its six Optimize* wrappers
 *    (ContaminationEstimator.h:316-442, ContaminationEstimator.cpp:88-332),
 *    driving AmoebaMinimizer (MathGenMin.cpp:313-443).
 * ------------------------------------------------------------------------- */
typedef struct vb2_model {
    int32_t is_heter;          /* !--WithinAncestry            (main.cpp:287)      */
    int32_t is_pc_fixed;       /* --FixPC                      (main.cpp:291-308)  */
    int32_t is_alpha_fixed;    /* --FixAlpha                   (main.cpp:309-313)  */
    int32_t is_af_known;       /* --KnownAF                    (main.cpp:314-319)  */
    double fix_alpha;          /* --FixAlpha value                                 */
    const double *fix_pc;      /* --FixPC values (num_pc) or NULL                  */
    double epsilon;            /* --Epsilon, 1e-8 by default   (main.cpp:76); a value that is not positive
                                * (0 of a zero-initialised struct, negative, NaN) means that default */
    int32_t verbose;           /* --Verbose: per-evaluation notice (h:435-440)     */
    int32_t notices;           /* print the reference's stderr lines: PhaseTimer "Starting/Finished
                                * phase" (ContaminationEstimator.cpp:10-24, 93-155) and the
                                * non-convergence warning (MathGenMin.cpp:381); vb2_run sets it */
} vb2_model;

#define VB2_MAX_PC 64

typedef struct vb2_estimate {
    double alpha;              /* fn.globalAlpha                                   */
    double llk1;               /* fn.llk1 (= -LLK at the best evaluated point)     */
    double llk0;               /* fn.llk0                                          */
    double pc[VB2_MAX_PC];     /* fn.globalPC   (contaminating sample)             */
    double pc2[VB2_MAX_PC];    /* fn.globalPC2  (intended sample)                  */
    int64_t num_eval;          /* likelihood evaluations the reference would make  */
    int64_t num_launch_point;  /* points actually evaluated (speculation included) */
    int32_t converged;         /* 0 if a Minimize() ran out of cycles              */
    int32_t reserved;          /* vb2_ctx_optimize_llk_ex: index of the winning start, else 0 */
} vb2_estimate;

/* The objective seam, batched: the analogue of VectorFunc::Evaluate
 * (statgen/MathVector.h:281-308).  Must write +LLK for each point. */
typedef int (*vb2_eval_fn)(void *user, int32_t num_point, const double *pc1,
                           const double *pc2, const double *alpha, double *llk_out);

/* Optional per-evaluation trace: one record per evaluation the REFERENCE would
 * have made, in its order. */
typedef struct vb2_trace {
    int64_t capacity;
    int64_t count;
    double *alpha;             /* [capacity]            */
    double *pc1;               /* [capacity * num_pc]   */
    double *pc2;               /* [capacity * num_pc]   */
    double *llk;               /* [capacity]            */
} vb2_trace;

/* OptimizeLLK over an arbitrary evaluator (e.g. marker shards + all-reduce). */
int vb2_optimize_llk(vb2_eval_fn eval, void *user, int32_t num_pc, const vb2_model *model,
                     vb2_estimate *out, vb2_trace *trace);
/* OptimizeLLK on a context (evaluator = vb2_llk_eval_batch on ctx).  The search runs against ONE
 * kernel that stays resident on the device and receives each iteration's points through a mailbox
 * in pinned host memory; the calling thread spins until the search is over and
 * the context's stream is busy for that time.  Falls back to one launch per iteration on its own
 * when the mode is unavailable (VB2_RESIDENT=0 forces that).  Same results either way. */
int vb2_ctx_optimize_llk(vb2_ctx *ctx, const vb2_model *model, vb2_estimate *out,
                         vb2_trace *trace);

/* Optimiser variants beyond the reference's single Nelder-Mead run; with
 * num_start <= 1 and line_search == 0 this IS vb2_ctx_optimize_llk.
 *  - Multi-start: num_start searches from different starting points advance in lock-step on the
 *    context, the evaluations of one step leaving as ONE launch (north_star: "objective
 *    evaluations batch across restarts").  Start 0 is the reference's (h:321-331: PCs 0.01, alpha
 *    0.03); starts 1.. add seeded Gaussian noise to the free parameters -- what the reference's
 *    commented-out rand() starts (h:322, 326) and its otherwise unused --Seed were for.  *best is
 *    the run with the smallest llk1; all (optional) receives every run, all[0] = the reference's.
 *  - Line search: a model with ONE free parameter (--FixPC / --KnownAF: alpha alone) is minimised
 *    by golden-ratio bracketing + Brent's method (ScalarMinimizer, MathGold.cpp:27-195, which the
 *    reference links but never calls) instead of the two-vertex simplex. */
typedef struct vb2_search_opts {
    int32_t num_start;         /* >= 1 (0 counts as 1); at most 64                 */
    uint32_t seed;             /* --Seed                                           */
    double start_sd;           /* noise on the PC starts; logit(alpha) gets 50 x; 0 = 0.02 */
    int32_t line_search;       /* Brent for one-parameter models                   */
    int32_t reserved;
} vb2_search_opts;
int vb2_ctx_optimize_llk_ex(vb2_ctx *ctx, const vb2_model *model, const vb2_search_opts *opts,
                            vb2_estimate *best, vb2_estimate *all /* [num_start] or NULL */);

/* A 95% confidence interval for FREEMIX and standard errors of the model's free parameters at an estimate
 * (vb2_ctx_interval).  Rows are those of <Output>.CI: FREEMIX first, then one row per free PC; values and SEs as
 * .selfSM / .Ancestry print them -- FREEMIX = alpha or 1 - alpha, the PCs with the reference's swap of indices 0 and 1
 * between the two samples when alpha >= 0.5 (ContaminationEstimator.cpp:146-149), each SE following its value.
 * NAN where a value does not exist. */
#define VB2_CI_MAX_ROW (2 * VB2_MAX_PC + 1)
typedef struct vb2_interval {
    double freemix;            /* FREEMIX as .selfSM prints it                                            */
    double freemix_se;         /* alpha(1-alpha) SE(logit alpha); NAN: alpha fixed or -H not pos. definite */
    double lo, hi;             /* profile-likelihood interval (chi2_1(0.95)/2 below llk_max); NAN: fixed   */
    double llk_max;            /* max(-llk1, every profile value)                                         */
    double llk_lo, llk_hi;     /* profile LLK at lo and hi                                                */
    int32_t alpha_free;        /* 0: --FixAlpha (no interval: METHOD fixed)                                */
    int32_t num_free;          /* free parameters: the components of the model's simplex vector (h:339-433) */
    int32_t pos_def;           /* 1: -H at the estimate is positive definite                              */
    int32_t num_row;
    int32_t row_kind[VB2_CI_MAX_ROW];   /* 0 FREEMIX, 1 ContaminatingSample.PC, 2 IntendedSample.PC, 3 PC (shared) */
    int32_t row_pc[VB2_CI_MAX_ROW];     /* PC number (1-based); 0 for FREEMIX                                  */
    double row_est[VB2_CI_MAX_ROW];
    double row_se[VB2_CI_MAX_ROW];
    double row_lo[VB2_CI_MAX_ROW];      /* FREEMIX: the profile interval; PCs: Wald, estimate -+ 1.96 SE       */
    double row_hi[VB2_CI_MAX_ROW];
    int64_t num_launch;        /* derivative launches (vb2_llk_derivs_batch calls) the interval used      */
    int64_t num_profile;       /* profile points maximised                                                */
} vb2_interval;

/* The interval at `est` (the result of vb2_ctx_optimize_llk / _ex under `model`).  Standard errors from -H of the LLK in
 * the free parameters of FullLLKFunc::Evaluate's packing (h:339-433; alpha as logit), from vb2_llk_derivs_batch at the
 * reported point.  FREEMIX: the profile likelihood -- the LLK maximised over the other free parameters at alpha = f
 * (1 - f when alpha >= 0.5: L(pc1, pc2, a) = L(pc2, pc1, 1 - a)) by damped Newton steps on the derivatives -- cut at
 * llk_max - 1.9207294103470620; lo = 0 / hi = 0.5 where the profile stays above the cut there.  model->notices: NOTICE
 * lines on stderr (a non-positive-definite Hessian, a profile value above -llk1, a search that did not converge). */
int vb2_ctx_interval(vb2_ctx *ctx, const vb2_model *model, const vb2_estimate *est, vb2_interval *out);

/* ------------------------------------------------------------------------- *
 * 2b. Cohorts: several samples (contexts on one device, same --NumPC) advancing in
 *     lock-step -- every Nelder-Mead step of every sample goes into ONE kernel launch
 *     (BASELINE.json configs[4]; the reference would run them as separate processes).
 * ------------------------------------------------------------------------- */
typedef struct vb2_batch vb2_batch;
#define VB2_BATCH_SLOTS 8      /* parameter points per sample and step */

int vb2_batch_create(vb2_ctx *const *ctxs, int32_t num_sample, vb2_batch **out);
void vb2_batch_destroy(vb2_batch *b);
/* One step: sample s evaluates num_point[s] (0..8) points.  pc1/pc2 are
 * [num_sample][8][num_pc], alpha and llk_out [num_sample][8]; unused slots are ignored. */
int vb2_batch_eval(vb2_batch *b, const int32_t *num_point, const double *pc1, const double *pc2,
                   const double *alpha, double *llk_out);
/* OptimizeLLK for every sample; models has 1 entry (shared) or num_sample entries. */
int vb2_batch_optimize_llk(vb2_batch *b, const vb2_model *models, int32_t num_model,
                           vb2_estimate *out);

/* Gradient and Hessian of several samples' LLK in one launch pair: sample s has num_point[s] >= 0 points, the rows of all
 * samples concatenated in sample order -- pc1 / pc2 [sum][num_pc], alpha [sum] -> llk [sum], grad [sum][2k+1],
 * hess [sum][2k+1][2k+1].  Every point's results are the bits vb2_llk_derivs_batch returns on that sample's context alone,
 * whatever else the call holds.  Synchronous; not while a sample is inside vb2_ctx_search_begin / vb2_ctx_search_end. */
int vb2_batch_derivs(vb2_batch *b, const int32_t *num_point, const double *pc1, const double *pc2, const double *alpha,
                     double *llk_out, double *grad_out, double *hess_out);
/* vb2_ctx_interval for every sample of the batch at est[s] (models: 1 entry or num_sample), the intervals advancing in
 * lock-step: every step's one derivative point per unfinished sample goes into one vb2_batch_derivs call.  out[s] is what
 * vb2_ctx_interval gives for the sample alone, bit for bit; status[s] the sample's own code; *num_step (may be NULL) the
 * batched derivative steps taken: the largest num_launch among the samples, not their sum. */
int vb2_batch_interval(vb2_batch *b, const vb2_model *models, int32_t num_model, const vb2_estimate *est,
                       vb2_interval *out /* [num_sample] */, int32_t *status /* [num_sample] */, int64_t *num_step);
/* The same driver over a caller's evaluator (the seam vb2_optimize_llk is for the search): no device needed.  A step calls
 * fn once, on the calling thread's own stack, with num_point[s] = 1 for every sample whose interval is still running and 0
 * for the others; rows and results concatenated in sample order as for vb2_batch_derivs.  Non-zero from fn ends every
 * interval and is returned.  data_has_known_af: [num_sample] or NULL (none). */
typedef int (*vb2_batch_derivs_fn)(void *user, int32_t num_sample, const int32_t *num_point, const double *pc1,
                                   const double *pc2, const double *alpha, double *llk, double *grad, double *hess);
int vb2_intervals_lockstep(vb2_batch_derivs_fn fn, void *user, int32_t num_sample, int32_t num_pc,
                           const int32_t *data_has_known_af, const vb2_model *models, int32_t num_model,
                           const vb2_estimate *est, vb2_interval *out, int32_t *status, int64_t *num_step);

/* ------------------------------------------------------------------------- *
 * 2c. Marker shards: ONE sample's markers spread over several GPUs (BASELINE.json configs[3]).
 *     LLK is a sum of independent per-marker terms -- the reference's OpenMP
 *     `reduction(+:sumLLK)` over markers (ContaminationEstimator.h:232-235) -- so each device
 *     evaluates a contiguous, read-balanced marker range and the B partial sums of a batch meet
 *     in ONE ncclAllReduce of B doubles over RCCL/xGMI.  librccl is bound at run time when a
 *     group spans more than one device.
 * ------------------------------------------------------------------------- */
typedef struct vb2_shard_group vb2_shard_group;

/* One process drives every device (VerifyBamID --Devices a,b,...).  `in` is the WHOLE sample;
 * shard d lives on devices[d].  Evaluations: one launch per device + a grouped ncclAllReduce;
 * vb2_shard_group_optimize_llk runs the search against one resident kernel per device and adds
 * the (<= 4) partial sums per device on the host.  A device listed twice gets two shards that
 * are added on the host (no RCCL): that is how a single-GPU machine exercises the code. */
int vb2_shard_group_create(const vb2_input *in, const int32_t *devices, int32_t num_device,
                           vb2_shard_group **out);
/* One process per GPU (python -m torch.distributed.run, mpirun): rank 0 calls vb2_rccl_unique_id,
 * the caller broadcasts the 128 bytes by its own means, then every rank builds the group with the
 * WHOLE sample, its device, its rank.  Every evaluation is launch + ncclAllReduce on the
 * context's stream; all ranks receive identical sums and take identical search decisions.
 * id128 == VB2_SHARD_PARTIAL_SUMS asks for a group WITHOUT a communicator: vb2_shard_group_eval then
 * returns this rank's PARTIAL sums and the caller reduces them over its own transport
 * (torch.distributed, MPI); vb2_shard_group_optimize_llk needs whole sums and refuses such a group.
 * id128 == NULL is accepted with nranks == 1 only (one rank needs no communicator); with more ranks it
 * is VB2_ERR_INVALID -- since ABI 5: a forgotten id used to yield plausible but partial LLKs silently.
 * vb2_shard_info.partial_sums says which kind a group is. */
#define VB2_SHARD_PARTIAL_SUMS ((const void *)(uintptr_t)1)
int vb2_rccl_unique_id(void *id128 /* 128 bytes out */);
int vb2_shard_group_create_rank(const vb2_input *in, int32_t device, int32_t rank, int32_t nranks,
                                const void *id128, vb2_shard_group **out);
/* ComputeMixLLKs over all shards for B points (host pointers, synchronous). */
int vb2_shard_group_eval(vb2_shard_group *g, int32_t num_point, const double *pc1, const double *pc2,
                         const double *alpha, double *llk_out);
int vb2_shard_group_optimize_llk(vb2_shard_group *g, const vb2_model *model, vb2_estimate *out,
                                 vb2_trace *trace);
typedef struct vb2_shard_info {
    int32_t num_shard;         /* shards owned by THIS process                     */
    int32_t nranks;            /* processes in the group (1 = single process)      */
    int32_t rank;
    int32_t uses_rccl;         /* partial sums meet in ncclAllReduce (else: host)  */
    int64_t num_allreduce;     /* collectives issued so far                        */
    int32_t marker_lo[64];     /* marker range of each owned shard                 */
    int32_t marker_hi[64];
    int64_t num_read[64];      /* reads of each owned shard                        */
    int32_t partial_sums;      /* 1: no communicator by request (VB2_SHARD_PARTIAL_SUMS): eval = this rank's part */
    int32_t rccl_stub;         /* 1: the collective library bound at run time is the test stand-in
                                * (VB2_RCCL_LIB=tests/stub_rccl/librccl_stub.so), not librccl                */
} vb2_shard_info;
int vb2_shard_group_info(const vb2_shard_group *g, vb2_shard_info *info);
/* The partition itself (no device needed): shard `rank` of `nranks` owns markers [*lo, *hi), cut so
 * that every shard holds about the same number of READS (balance on R, not M). */
int vb2_shard_range(const vb2_input *in, int32_t rank, int32_t nranks, int32_t *lo, int32_t *hi);
void vb2_shard_group_destroy(vb2_shard_group *g);

/* ------------------------------------------------------------------------- *
 * 3. File level: the --SVDPrefix/--PileupFile flow of execute()
 *    (main.cpp:283-411): panel + pileup readers, sanity check, OptimizeLLK,
 *    <out>.Ancestry and <out>.selfSM writers.
 * ------------------------------------------------------------------------- */
typedef struct vb2_mpileup_opts {
    int32_t given;             /* 0: every field below is ignored, the defaults of main.cpp:81-96 apply */
    int32_t min_bq;            /* --min-BQ      skip bases with baseQ/BAQ below it         (13)   */
    int32_t min_mq;            /* --min-MQ      skip alignments with mapQ below it         (2)    */
    int32_t adjust_mq;         /* --adjust-MQ   mapQ cap coefficient, 0 disables           (40)   */
    int32_t max_depth;         /* --max-depth   per-file depth cap                         (8000) */
    int32_t no_orphans;        /* --no-orphans  drop anomalous read pairs                  (0)    */
    int32_t incl_flags;        /* --incl-flags  the reference stores this in mplp.flag     (REALN | SMART_OVERLAPS) */
    int32_t excl_flags;        /* --excl-flags  skip reads with any of these bits set      (UNMAP|SECONDARY|QCFAIL|DUP) */
} vb2_mpileup_opts;

typedef struct vb2_run_args {
    const char *ud_path;       /* <SVDPrefix>.UD   (main.cpp:229)                  */
    const char *mean_path;     /* <SVDPrefix>.mu                                   */
    const char *bed_path;      /* <SVDPrefix>.bed                                  */
    const char *pileup_path;   /* --PileupFile                                     */
    const char *known_af_path; /* --KnownAF or NULL                                */
    const char *output_prefix; /* --Output (default "result"); NULL = write nothing*/
    int32_t num_pc;            /* --NumPC (default 2)                              */
    int32_t disable_sanity;    /* --DisableSanityCheck                             */
    int32_t output_pileup;     /* --OutputPileup                                   */
    int32_t device;            /* HIP device ordinal, -1 = current                 */
    vb2_model model;
    /* --Devices a,b,...: more than one entry spreads the work over those GPUs -- vb2_run shards
     * the sample's markers (2c), vb2_cohort_run deals whole groups of samples to the devices
     * (no collective).  NULL / 0 = `device` alone. */
    const int32_t *devices;
    int32_t num_device;
    /* --ApplyBAQ (the field was `reserved`: same offset and size, ABI 7 stays).  0: BAM input is piled up as it is.  1: the
     * built-in reader applies to every record what the effective mpileup options ask of the FASTA at reference_path, in
     * mplp_func's order (vb2_baq_stats below): the Illumina-1.3 shift (incl_flags & 128), base alignment quality
     * (incl_flags & 16; & 64 ignores an existing BQ tag), the mapping-quality cap (adjust_mq > 10).  Any other value is
     * VB2_ERR_INVALID.  No effect on pileup_path input. */
    int32_t bam_adjust;
    /* --BamFile / --Reference: BAM input (SimplePileupViewer.cpp:172-557), used when pileup_path is NULL: the built-in
     * reader (vb2_bam_stats below), or htslib's where the library was configured with it.  reference_path is read by
     * the built-in reader under bam_adjust = 1 alone; the reference base of a site is the panel's REF allele either way. */
    const char *bam_path;
    const char *reference_path;
    /* --NumStart / --Seed / --LineSearch: optimiser variants (vb2_search_opts); all zero = the
     * reference's single Nelder-Mead run.  One sample on one device only. */
    vb2_search_opts search;
    /* (ABI 6) The reference's "Pileup Options" (main.cpp:176-187; defaults main.cpp:81-96): they shape what
     * --BamFile input turns into pileup columns (SimplePileupViewer.cpp:172-237, 457-476) and have no effect on
     * --PileupFile input, exactly as in the reference.  given == 0: the defaults. */
    vb2_mpileup_opts mpileup;
} vb2_run_args;

typedef struct vb2_run_result {
    vb2_estimate est;
    int32_t num_marker;        /* #SNPS                                            */
    int32_t num_site;          /* sites shared with the pileup                     */
    int64_t num_bases;         /* viewer.numBases                                  */
    double avg_depth;          /* AVG_DP                                           */
    double sd_depth;
    double seconds_load;       /* wall-clock: readers                              */
    double seconds_optimize;   /* wall-clock: OptimizeLLK (the "converged alpha" time) */
} vb2_run_result;

int vb2_run(const vb2_run_args *args, vb2_run_result *out);
/* vb2_run, then vb2_ctx_interval on the winning estimate, then <output_prefix>.CI (tab-separated: #PARAM ESTIMATE STDERR
 * CI_LOW CI_HIGH METHOD) and one NOTICE line with the FREEMIX interval on stderr.  stdout, .selfSM and .Ancestry are what
 * vb2_run writes.  One device only (VB2_ERR_INVALID for marker shards over several devices, before any file is read). */
int vb2_run_interval(const vb2_run_args *args, vb2_run_result *out, vb2_interval *ci);

/* Cohort form of vb2_run (BASELINE configs[4]: many samples against one panel).  The reference
 * runs one process per sample; here the panel (.UD/.mu/.bed, optional AF file) is read once, the
 * pileups are read by host threads (and flattened on the device) while the device searches the previous group of
 * samples in lock-step (one kernel launch per search step for the whole group, vb2_batch_*), and
 * every sample gets the outputs vb2_run would write (<prefix>.Ancestry, <prefix>.selfSM, optional
 * <prefix>.Pileup).  args->pileup_path / output_prefix of `base` are ignored.
 * status[s] receives the sample's own VB2_* code (e.g. VB2_ERR_SANITY); the call itself fails only
 * for errors that concern all samples (panel, device). */
typedef struct vb2_cohort_args {
    vb2_run_args base;                   /* panel paths, num_pc, flags, model, device          */
    int32_t num_sample;
    const char *const *pileup_paths;     /* [num_sample]                                      */
    const char *const *output_prefixes;  /* [num_sample], or NULL = write nothing             */
    int32_t group_size;                  /* samples on a device at a time (<= 64); 0 = 32: slots
                                          * that a converged sample hands to the next ready one;
                                          * < 0: |group_size|.  (VB2_COHORT_STREAM=0: groups of that
                                          * size searched one after the other, the first of 16)   */
    int32_t num_host_thread;             /* pileup readers/flatteners; 0 = the CPUs the process may
                                          * use (cgroup quota / affinity) less one, at most 64 per
                                          * device                                                */
} vb2_cohort_args;
int vb2_cohort_run(const vb2_cohort_args *args, vb2_run_result *out /* [num_sample] */,
                   int32_t *status /* [num_sample] */);

/* ------------------------------------------------------------------------- *
 * 3b. The source of a contamination within a cohort (--FindSource).  Not in the reference: it
 *     follows its model (ContaminationEstimator.h:186-192, 285-311).  With W[g1][g2] = prod_reads P(read | g1, g2, alpha)
 *     of a marker (g1 the alpha-fraction, contaminating genotype, g2 the intended one) and GF1, GF2 the genotype priors
 *     at the two samples' allele frequencies:
 *         L     = sum GF1[g1] GF2[g2] W[g1][g2]                 (h:307-309; the marker counts where L > 0, h:310)
 *         c[g1] = (sum_g2 W[g1][g2] GF2[g2]) / L                contaminant-genotype likelihood relative to a random one
 *         q[g2] = GF2[g2] (sum_g1 GF1[g1] W[g1][g2]) / L        posterior of the sample's own genotype
 *     and for target i, candidate j:  S(i, j) = sum_m log max(c_i[m] . q_j[m], VB2_SOURCE_DOT_FLOOR)  over the markers
 *     both count: the log-likelihood ratio of "i's contaminant carries j's genotypes" against "a random individual of
 *     i's fitted contaminant ancestry".  S -> 0 as alpha_i -> 0 (c -> 1): a clean sample has no source.
 * ------------------------------------------------------------------------- */
#define VB2_SOURCE_DOT_FLOOR 1e-30     /* bounds what one marker can veto at -69 nats; part of the definition (the device
                                        * compares float32 dots against its float32 rounding) */

/* c, q and log L at ONE point, per marker in panel order: contam_lik [M][3], geno_post [M][3], log_l [M]; host pointers,
 * any may be NULL; zeros for the markers the sample does not count.  sum_m log_l = vb2_llk_eval_batch at the point.
 * Synchronous; not between vb2_ctx_search_begin and vb2_ctx_search_end. */
int vb2_ctx_marginals(vb2_ctx *ctx, const double *pc1, const double *pc2, double alpha, double *contam_lik,
                      double *geno_post, double *log_l);

/* A set of samples of ONE panel on ONE device: per sample its c and q as float32, 24 bytes per marker, in device memory
 * (capacity x num_marker x 24 bytes, reserved at creation: VB2_ERR_NOMEM with the bytes needed when they do not fit). */
typedef struct vb2_source_set vb2_source_set;
int vb2_source_set_create(int32_t num_marker, int32_t capacity, int32_t device, vb2_source_set **out);
/* Adds the sample of `ctx` at the search's own point of `est` (the result of vb2_ctx_optimize_llk under `model`): the
 * reported PCs with the swap of indices 0 and 1 undone, and -- when alpha >= 0.5 -- mirrored, pc1 <-> pc2 and alpha ->
 * 1 - alpha (L(pc1, pc2, a) = L(pc2, pc1, 1 - a)), so that g1 is always the minor component.  The context may be destroyed
 * afterwards.  *index: the sample's row and column in the score matrix.  Thread-safe. */
int vb2_source_set_add(vb2_source_set *set, vb2_ctx *ctx, const vb2_model *model, const vb2_estimate *est, int32_t *index);
/* score [n][n] (row = target, column = candidate; NAN on the diagonal) and shared [n][n] (markers both count), n = samples
 * added; either may be NULL.  A pair's score is the same bits from call to call and whatever else the set holds. */
int vb2_source_set_scores(vb2_source_set *set, double *score, int32_t *shared);
/* n: the slots taken so far (a sample whose add failed after it took its slot keeps it, as a row and column of NAN). */
int vb2_source_set_size(vb2_source_set *set, int32_t *n);
void vb2_source_set_destroy(vb2_source_set *set);

/* vb2_cohort_run that also adds every searched sample to a source set before its context is released (one device only:
 * VB2_ERR_INVALID otherwise, before any file is read).  score / shared: [num_sample][num_sample] in the order of the
 * samples, or NULL; a sample that failed has a row and a column of NAN.  With output prefixes it writes
 * <output_prefix of base>.Sources -- tab-separated "#SAMPLE FREEMIX RANK CANDIDATE LLR MARKERS", per sample its `top`
 * best candidates by descending LLR, samples and candidates named by their output prefixes.  Everything else is what
 * vb2_cohort_run does and writes. */
int vb2_cohort_run_sources(const vb2_cohort_args *args, int32_t top, vb2_run_result *out /* [num_sample] */,
                           int32_t *status /* [num_sample] */, double *score, int32_t *shared);

/* vb2_cohort_run_sources plus a stage after the score matrix (--FindSource --RefitSource; section 3d):
 * the contexts of the samples that got a row in the source set are not destroyed when their files are written but parked --
 * the one cost of the call, their device bytes go into a NOTICE -- and after the matrix every sample is refitted GIVEN its best
 * candidate, where that candidate's score is finite and > 0: a one-hypothesis vb2_conditioned set on the sample's own
 * context, pc1 held at the sample's search point (vb2_source_set_add), all refits in ONE vb2_conditioned_optimize_llk.
 * fit: [num_sample] or NULL.  With output prefixes it writes <output_prefix of base>.SourceFit, tab-separated with %g:
 *     #SAMPLE CANDIDATE LLR MARKERS FREEMIX FREELK1 ALPHA_GIVEN LK1_GIVEN LK0_GIVEN DELTA_LK
 * one row per searched sample with a first candidate in .Sources (a sample that failed is absent), NA in the last four
 * columns where no refit ran.  FREELK1, LK1_GIVEN and LK0_GIVEN are minus log-likelihoods as the cohort's stdout table
 * prints FREELK1 (vb2_estimate.llk1 / llk0); DELTA_LK = (-LK1_GIVEN) - (-FREELK1): positive = the likelihood at the
 * conditioned maximum exceeds the anonymous model's at its own maximum -- with num_pc fewer free parameters.  LLR is the
 * floored score of .Sources; DELTA_LK has no floor.  A refit that fails leaves its row NA, gives a NOTICE and does not fail
 * the run.  is_alpha_fixed and more than one device are VB2_ERR_INVALID before any file is read.  stdout, .selfSM, .Ancestry
 * and .Sources are what vb2_cohort_run_sources writes. */
#define VB2_SOURCE_FIT_NONE 1          /* vb2_source_fit.status: no refit was asked of this sample */
typedef struct vb2_source_fit {
    int32_t candidate;         /* the best candidate's sample index; -1: none (the sample failed, or stands alone)   */
    int32_t markers;           /* markers both count                                                                  */
    int32_t status;            /* VB2_OK: refitted; VB2_SOURCE_FIT_NONE; or the refit's error                         */
    int32_t reserved;
    double llr;                /* the candidate's score in the matrix                                                 */
    double freemix, freelk1;   /* the anonymous fit: min(alpha, 1 - alpha), llk1                                      */
    double alpha_given, lk1_given, lk0_given, delta_lk;    /* NAN where no refit ran                                  */
} vb2_source_fit;
int vb2_cohort_run_source_fits(const vb2_cohort_args *args, int32_t top, vb2_run_result *out /* [num_sample] */,
                               int32_t *status /* [num_sample] */, double *score, int32_t *shared,
                               vb2_source_fit *fit /* [num_sample] or NULL */);

/* vb2_cohort_run, then FREEMIX of every listed tumour given its matched normal (--MatchedNormal; 3e).
 * Pair p is (tumour[p], normal[p]), sample indices of the cohort.  The normals get a q row in a source set; only the
 * tumours' contexts stay on the device after their search (a NOTICE names the bytes); after the last sample every pair is
 * refitted in ONE vb2_paired_optimize_llk -- pi2 = the normal's q where max(q[0], q[2]) >= hom_min, every other marker left
 * out, pc2 held at the normal's intended PCs at its search point, alpha and pc1 searched -- and <output_prefix>.PairFit is
 * written (tab-separated, %g, minus log-likelihoods as in .SourceFit):
 *     #TUMOUR NORMAL NORMAL_FREEMIX MARKERS FREEMIX FREELK1 ALPHA_PAIRED LK1_PAIRED LK0_PAIRED
 * A pair whose tumour or normal failed its own run is a row of NA (status VB2_PAIR_FIT_NONE) and changes no other row; a
 * refit that fails leaves NA in the last three columns, gives a NOTICE and does not fail the run.  stdout, .selfSM and
 * .Ancestry are what vb2_cohort_run writes.  VB2_ERR_INVALID before any file is read: an index out of range, a tumour listed
 * twice, a sample paired with itself, hom_min outside [0, 1], is_alpha_fixed, more than one device. */
#define VB2_PAIR_FIT_NONE 1            /* vb2_pair_fit.status: the tumour or the normal failed its own run */
typedef struct vb2_pair_fit {
    int32_t tumour, normal;    /* sample indices                                                                      */
    int32_t markers;           /* markers of the tumour the refit walks (vb2_paired_info_get's given)                 */
    int32_t status;            /* VB2_OK: refitted; VB2_PAIR_FIT_NONE; or the refit's error                           */
    double normal_freemix;     /* the normal's anonymous fit: min(alpha, 1 - alpha)                                   */
    double freemix, freelk1;   /* the tumour's anonymous fit                                                          */
    double alpha_paired, lk1_paired, lk0_paired;           /* NAN where no refit ran                                  */
} vb2_pair_fit;
int vb2_cohort_run_paired(const vb2_cohort_args *args, int32_t num_pair, const int32_t *tumour, const int32_t *normal,
                          double hom_min, vb2_run_result *out /* [num_sample] */, int32_t *status /* [num_sample] */,
                          vb2_pair_fit *fits /* [num_pair] or NULL */);
/* vb2_cohort_run_paired followed by ONE vb2_paired_interval (3f) over every refitted pair, on the
 * parked tumour contexts before they are released (--MatchedNormal --PairInterval): ci [num_pair] or NULL, zeroed for a pair
 * without a refit or whose interval failed (a NOTICE; the run goes on).  <output_prefix>.PairCI is written (tab-separated,
 * %g, names as in the pair file, NA for such a pair and for an SE that does not exist):
 *     #TUMOUR NORMAL MARKERS ALPHA_PAIRED SE LO95 HI95 LLK_MAX LLK_LO LLK_HI POS_DEF PROFILE_POINTS
 * ALPHA_PAIRED is unfolded and LO95 / HI95 lie within [0, 1].  stdout, .selfSM, .Ancestry and .PairFit are what
 * vb2_cohort_run_paired writes, byte for byte. */
int vb2_cohort_run_paired_intervals(const vb2_cohort_args *args, int32_t num_pair, const int32_t *tumour, const int32_t *normal,
                                    double hom_min, vb2_run_result *out /* [num_sample] */, int32_t *status /* [num_sample] */,
                                    vb2_pair_fit *fits /* [num_pair] or NULL */, vb2_interval *ci /* [num_pair] or NULL */);
/* The --MatchedNormal file: lines "TUMOUR<TAB>NORMAL", each a pileup path exactly as in pileup_paths.  tumour / normal:
 * [num_sample] (a tumour is listed once).  VB2_ERR_IO: the file cannot be read; VB2_ERR_INVALID with a message that names
 * the line: a name that is not in the list, a tumour listed twice, a sample paired with itself, no pair at all.  Host only. */
int vb2_matched_normal_read(const char *path, int32_t num_sample, const char *const *pileup_paths, int32_t *num_pair,
                            int32_t *tumour, int32_t *normal);

/* vb2_cohort_run that also computes every searched sample's interval (vb2_batch_interval: in lock-step, on a stage of its own
 * next to the search) and writes <prefix>.CI per sample; ci: [num_sample] or NULL.  A sample that failed its search or its
 * sanity check has no .CI (and a zeroed ci entry).  source_top > 0: --FindSource as well, what vb2_cohort_run_sources does
 * with top = source_top (score and shared NULL).  One device only: VB2_ERR_INVALID otherwise, before any file is read. */
int vb2_cohort_run_intervals(const vb2_cohort_args *args, int32_t source_top, vb2_run_result *out /* [num_sample] */,
                             int32_t *status /* [num_sample] */, vb2_interval *ci);

/* ------------------------------------------------------------------------- *
 * 3e. Duplicates and relatives within a cohort (--FindRelated).  Not in the reference: its model
 *     again.  Per counted marker, at the point vb2_source_set_add takes (3b), with p the clamped allele frequency GF2 is
 *     formed from:
 *         h[g]  = (sum_g1 GF1[g1] W[g1][g]) / L      own-genotype likelihood relative to a random individual; q = GF2 h
 *         t[g'] = sum_g q[g] T_p[g][g']              genotype distribution of a relative sharing one allele by descent,
 *         T_p   = [(1-p, p, 0), ((1-p)/2, 1/2, p/2), (0, 1-p, p)]
 *     and for target i, partner j over the markers both count, d2 = q_i . h_j, d1 = t_i . h_j,
 *         K_r(i, j) = sum_m log max(k0_r + k1_r d1 + k2_r d2, VB2_SOURCE_DOT_FLOOR)
 *     with (k0, k1, k2) = DUP (0, 0, 1), PO (0, 1, 0), FS (1/4, 1/2, 1/4), D2 (1/2, 1/2, 0): the log-likelihood ratio of "j's
 *     reads come from a relative r of i's individual, genotype prior at i's fitted ancestry" against "two unrelated
 *     individuals, each at its own fitted ancestry".  The matrix is ordered; K(i, i) is NAN.
 * ------------------------------------------------------------------------- */
#define VB2_SET_SOURCE 1               /* planes of a set: c and q -- vb2_source_set_scores                     */
#define VB2_SET_RELATED 2              /*                  q, h and t -- vb2_source_set_relations               */
#define VB2_NUM_RELATION 4
#define VB2_REL_DUP 0                  /* the same individual (a second library, a swap)                        */
#define VB2_REL_PO 1                   /* parent and child                                                      */
#define VB2_REL_FS 2                   /* full siblings                                                         */
#define VB2_REL_D2 3                   /* second degree: grandparent, half sibling, uncle or aunt               */

/* vb2_source_set_create with the planes to keep, VB2_SET_SOURCE | VB2_SET_RELATED in any combination: 12 bytes per marker
 * and sample for each of c, q, h, t the set holds (source: c q; related: q h t; both: c q h t).  vb2_source_set_create is
 * planes = VB2_SET_SOURCE.  vb2_source_set_add fills whatever planes the set has from ONE launch.  An entry asked of a set
 * without its planes returns VB2_ERR_INVALID. */
int vb2_source_set_create_ex(int32_t num_marker, int32_t capacity, int32_t device, int32_t planes, vb2_source_set **out);
/* llr [n][n][VB2_NUM_RELATION] (row = target, column = partner; NAN on the diagonal and for an empty slot's row and column)
 * and shared [n][n]; either may be NULL.  A pair's four values are the same bits from call to call and whatever else the
 * set holds. */
int vb2_source_set_relations(vb2_source_set *set, double *llr, int32_t *shared);
/* h and t at ONE point, per marker in panel order: own_lik [M][3], kin_post [M][3]; host pointers, either may be NULL; zeros
 * for the markers the sample does not count.  Synchronous, like vb2_ctx_marginals. */
int vb2_ctx_marginals_related(vb2_ctx *ctx, const double *pc1, const double *pc2, double alpha, double *own_lik,
                              double *kin_post);
/* vb2_cohort_run that also adds every searched sample to a set with the related planes before its context is released, in
 * both cohort modes (one device only: VB2_ERR_INVALID otherwise, before any file is read).  llr [num_sample][num_sample][4]
 * and shared [num_sample][num_sample] in the order of the samples, or NULL.  With output prefixes it writes <output_prefix of
 * base>.Related, tab-separated with %g:
 *     #SAMPLE PARTNER RANK RELATION LLR LLR_DUP LLR_PO LLR_FS LLR_D2 MARKERS
 * per sample its `related_top` partners by descending LLR = max_r K_r; RELATION names the arg-max (DUP, PO, FS, D2), or UN
 * when that LLR <= 0.  A sample that failed its search or sanity check keeps its files and status and is absent from the
 * file.  source_top > 0: what vb2_cohort_run_sources does with top = source_top as well (score and shared NULL), from the
 * same set and the same launch per sample.  Everything else is what vb2_cohort_run does and writes. */
int vb2_cohort_run_related(const vb2_cohort_args *args, int32_t related_top, int32_t source_top,
                           vb2_run_result *out /* [num_sample] */, int32_t *status /* [num_sample] */, double *llr,
                           int32_t *shared);

/* ------------------------------------------------------------------------- *
 * 3c. Weighted-marker replicates (--PerChromosome, --Bootstrap).  Not in the reference: its model
 *     with integer marker weights,  LLK_w(theta) = sum_i w_i log L_i(theta)  (L_i as in h:285-311; a marker counts where
 *     L_i > 0, h:310), for many weight vectors ("replicates") over the ONE resident copy of a sample.  LLK_w is what
 *     ComputeMixLLKs returns on the input with marker i repeated w_i times (depth statistics unchanged).
 * ------------------------------------------------------------------------- */
typedef struct vb2_replicates vb2_replicates;

/* weight: [num_rep][num_marker] counts 0..255 in panel order (num_marker = the context's).  The rows are uploaded once and
 * permuted on the device into the context's marker order; device memory comes from the library's slab cache.  The context
 * must outlive the set and must not be inside vb2_ctx_search_begin / vb2_ctx_search_end when the set is used. */
int vb2_replicates_create(vb2_ctx *ctx, int32_t num_rep, const uint8_t *weight, vb2_replicates **out);
void vb2_replicates_destroy(vb2_replicates *rep);
/* One step: replicate r evaluates num_point[r] (0..VB2_BATCH_SLOTS) points under its weights; the rows of all replicates
 * are concatenated in replicate order -- pc1 / pc2 [sum][num_pc], alpha [sum] -> llk_out [sum] -- as in vb2_batch_derivs.
 * A point's value is the same bits whatever else the step holds and from call to call; a replicate whose weights select no
 * counted marker evaluates to 0.0; an alpha outside [0, 1] leaves every marker out, as in vb2_llk_eval_batch. */
int vb2_replicates_eval(vb2_replicates *rep, const int32_t *num_point, const double *pc1, const double *pc2,
                        const double *alpha, double *llk_out);
/* OptimizeLLK for every replicate under `model` (the reference-exact simplex from the reference's start), all advancing in
 * lock-step, each step one vb2_replicates_eval.  status[r]: VB2_OK, or VB2_ERR_INVALID for a replicate with no counted
 * marker (the others finish); the return value: an error that concerns all. */
int vb2_replicates_optimize_llk(vb2_replicates *rep, const vb2_model *model, vb2_estimate *est_out /* [num_rep] */,
                                int32_t *status /* [num_rep] */);
typedef struct vb2_replicates_info {
    int32_t num_rep;
    int32_t num_marker;
    int64_t device_bytes;      /* device memory the set holds beyond the context's                   */
    int64_t num_step;          /* vb2_replicates_eval calls so far (the searches' steps included)     */
    int64_t num_launch;        /* marker-kernel launches of those steps                               */
} vb2_replicates_info;
int vb2_replicates_info_get(const vb2_replicates *rep, vb2_replicates_info *info, int64_t *counted /* [num_rep] or NULL */);
/* The same driver over a caller's evaluator (the seam vb2_optimize_llk is for one search): no device needed.  A step calls
 * fn once, on the calling thread's own stack; num_point[r] = 0 for a replicate that has finished.  A replicate whose first
 * evaluation is exactly 0.0 at every point has no counted marker.  Non-zero from fn ends every search and is returned. */
typedef int (*vb2_replicates_eval_fn)(void *user, int32_t num_rep, const int32_t *num_point, const double *pc1,
                                      const double *pc2, const double *alpha, double *llk);
int vb2_replicates_lockstep(vb2_replicates_eval_fn fn, void *user, int32_t num_rep, int32_t num_pc, const vb2_model *model,
                            vb2_estimate *est_out, int32_t *status);

/* Host-only helpers.
 * vb2_chromosome_weights: the blocks of a panel's .bed are its chromosomes in order of first appearance.  *num_block: their
 * number; block_of [num_marker]: the block of each of the first num_marker rows; block_size [max_block]: DISTINCT positions
 * of the block among those rows (a position listed twice is one); names [max_block][VB2_CHROM_NAME_LEN]; only / without
 * [num_block][num_marker]: the 0/1 indicator of the block's rows and its complement.  Any output may be NULL; more than
 * max_block blocks with a non-NULL per-block output, or fewer rows than num_marker, is VB2_ERR_INVALID (*num_block is set). */
#define VB2_CHROM_NAME_LEN 32
int vb2_chromosome_weights(const char *bed_path, int32_t num_marker, int32_t max_block, int32_t *num_block, int32_t *block_of,
                           int32_t *block_size, char *names, uint8_t *only, uint8_t *without);
/* out [num_rep][num_marker]: replicate r counts num_marker uniform draws of a marker index,
 * index = floor(x * num_marker / 2^64) for the 64-bit outputs x of splitmix64 started at
 * ((uint64_t)seed << 32) ^ (0x5851f42d4c957f2d * (r + 1)) -- the stream of the multi-start searches; counts saturate at 255. */
int vb2_bootstrap_weights(int32_t num_marker, int32_t num_rep, uint32_t seed, uint8_t *out);
/* Delete-m_j jackknife (Busing, Meijer and van der Leeden 1999): block j has m[j] counted markers and the estimate
 * theta_without[j] with it left out; n = sum m_j over the g blocks with m_j > 0 (the others are skipped), h_j = n / m_j,
 *   estimate = g theta_hat - sum_j (1 - m_j / n) theta_without[j],  tau_j = h_j theta_hat - (h_j - 1) theta_without[j],
 *   se^2 = (1 / g) sum_j (tau_j - estimate)^2 / (h_j - 1).   Fewer than two blocks with markers: VB2_ERR_INVALID. */
int vb2_jackknife(int32_t num_block, const int64_t *m, double theta_hat, const double *theta_without, double *estimate,
                  double *se);

/* vb2_run, then on the same context: per_chromosome != 0 -- every chromosome of the .bed alone and left out, refitted under
 * the run's model, <output_prefix>.Chrom (tab-separated: #CHROM MARKERS FREEMIX_ONLY FREELK1_ONLY FREELK0_ONLY
 * FREEMIX_WITHOUT DELTA, NA for a chromosome without counted markers, then "#JACKKNIFE FREEMIX <est> SE <se> LO <lo> HI
 * <hi>", the bounds FREEMIX -+ 1.96 se clipped to [0, 0.5]); bootstrap = N in 1..1000 -- N marker resamples seeded by
 * args->search.seed, <output_prefix>.Boot (#REPLICATE FREEMIX FREELK1, then "#BOOTSTRAP MEAN .. SD .. P2.5 .. P97.5 ..",
 * percentile q = the sorted value of index floor(q (N - 1) + 0.5)).  All searches form ONE replicate set.  stdout, .selfSM
 * and .Ancestry are what vb2_run writes.  One device only (VB2_ERR_INVALID otherwise, before any file is read). */
typedef struct vb2_replicate_summary {
    int32_t num_chrom;         /* rows of .Chrom (0: not asked for)                                  */
    int32_t num_boot;          /* bootstrap replicates that finished                                 */
    double jack_estimate, jack_se, jack_lo, jack_hi;
    double boot_mean, boot_sd, boot_p025, boot_p975;
    int64_t num_step;          /* lock-step steps of the replicate set                               */
    double seconds;            /* wall-clock of the replicate stage                                  */
} vb2_replicate_summary;
int vb2_run_replicates(const vb2_run_args *args, int32_t per_chromosome, int32_t bootstrap, vb2_run_result *out,
                       vb2_replicate_summary *summary /* or NULL */);

/* ------------------------------------------------------------------------- *
 * 3d. The likelihood given a hypothesised contaminant.  Not in the reference: its model with a
 *     per-marker genotype prior on the alpha-fraction component in place of the Hardy-Weinberg prior GF1.  In the notation
 *     of 3b, a hypothesis h carries one triple pi_h[m][3] per panel marker (float32, panel order):
 *         L_m(pc1, pc2, alpha | h) = sum_g1 P[g1] sum_g2 GF2[g2] W[g1][g2]
 *             P = pi_h[m]          where the triple is not all zero
 *             P = GF1(pc1)[m]      where it is (no information: the anonymous model's term)
 *         LLK(. | h) = sum_m log L_m  over the markers with L_m > 0  (h:310)
 *     An all-zero hypothesis is vb2_llk_eval_batch; at alpha = 0 a normalised prior drops out; with pi = q_j (3b) on the
 *     markers j counts, LLK(theta | j) - LLK(theta) = sum_shared log(c_i . q_j): 3b's score without its floor -- ONE
 *     discordant marker can cost more than 3b's -69 nats.  There is no mirror symmetry: alpha is the share of the
 *     hypothesised individual and is reported as fitted, never folded at 0.5.
 *     The refit (vb2_conditioned_optimize_llk) holds pc1 -- it only feeds the fallback markers -- and searches alpha and
 *     the intended sample's PCs: the conditioned model has num_pc FEWER free parameters than the default two-ancestry
 *     model, which a comparison of the two maxima has to bear in mind.
 * ------------------------------------------------------------------------- */
typedef struct vb2_conditioned vb2_conditioned;

/* prior: [num_hyp][num_marker][3] float32 in panel order (num_marker = the context's), host memory.  The rows are uploaded
 * once and permuted on the device into the context's marker order (three planes per hypothesis); device memory comes from
 * the library's slab cache.  The context must outlive the set and must not be inside vb2_ctx_search_begin /
 * vb2_ctx_search_end when the set is used. */
int vb2_conditioned_create(vb2_ctx *ctx, int32_t num_hyp, const float *prior, vb2_conditioned **out);
/* The same with hypothesis h = the genotype posterior q of sample candidate[h] of a source set (3b), copied device to
 * device.  The set must be of the context's panel size and on the context's device, and the candidate must have a row:
 * VB2_ERR_INVALID otherwise. */
int vb2_conditioned_create_from_set(vb2_ctx *ctx, vb2_source_set *set, int32_t num_hyp, const int32_t *candidate,
                                    vb2_conditioned **out);
void vb2_conditioned_destroy(vb2_conditioned *cond);
/* One step: hypothesis h evaluates num_point[h] (0..VB2_BATCH_SLOTS) points; the rows of all hypotheses are concatenated in
 * hypothesis order -- pc1 / pc2 [sum][num_pc], alpha [sum] -> llk_out [sum] -- as in vb2_replicates_eval.  A point's value
 * is the same bits whatever else the step holds and from call to call; an alpha outside [0, 1] leaves every marker out. */
int vb2_conditioned_eval(vb2_conditioned *cond, const int32_t *num_point, const double *pc1, const double *pc2,
                         const double *alpha, double *llk_out);
/* The refit of every hypothesis of every set, all in lock-step: the reference-exact OptimizeLLK under a copy of `model` with
 * is_heter = 0 (it packs pc1 = pc2 = v, starts where the reference starts and takes llk0 at alpha = 0), whose pc1 rows are
 * overwritten with pc1_fixed on their way to the device -- alpha and the intended sample's PCs are searched (alpha alone
 * with is_pc_fixed or known allele frequencies); is_alpha_fixed is VB2_ERR_INVALID.  pc1_fixed: [num_set][num_pc], one row
 * per set (the target's search point).  A step begins the evaluation of every set with live points, then collects them:
 * sets on different contexts overlap on the device.  est_out / status: [sum of num_hyp] in set order; est_out has alpha,
 * pc2 (also in pc), llk1 and llk0.  status: VB2_OK, or VB2_ERR_INVALID for a hypothesis whose first evaluation is exactly
 * 0.0 everywhere (no counted marker; the others finish).  All sets must share num_pc.  The return value: an error that
 * concerns all. */
int vb2_conditioned_optimize_llk(vb2_conditioned *const *sets, int32_t num_set, const vb2_model *model,
                                 const double *pc1_fixed, vb2_estimate *est_out, int32_t *status);
typedef struct vb2_conditioned_info {
    int32_t num_hyp;
    int32_t num_marker;
    int64_t device_bytes;      /* device memory the set holds beyond the context's                   */
    int64_t num_step;          /* evaluations that reached the device (the searches' steps included)  */
    int64_t num_launch;        /* marker-kernel launches of those steps                               */
} vb2_conditioned_info;
int vb2_conditioned_info_get(const vb2_conditioned *cond, vb2_conditioned_info *info);
/* The same driver over a caller's evaluator (the seam vb2_replicates_lockstep is for the replicates): no device needed.  A
 * step calls fn once, on the calling thread's own stack; num_point[h] = 0 for a hypothesis that has finished.  The pc1 rows
 * fn sees are pc1_fixed [num_hyp][num_pc] at every call, the llk0 call included.  Non-zero from fn ends every search and is
 * returned. */
typedef int (*vb2_conditioned_eval_fn)(void *user, int32_t num_hyp, const int32_t *num_point, const double *pc1,
                                       const double *pc2, const double *alpha, double *llk);
int vb2_conditioned_lockstep(vb2_conditioned_eval_fn fn, void *user, int32_t num_hyp, int32_t num_pc, const vb2_model *model,
                             const double *pc1_fixed, vb2_estimate *est_out, int32_t *status);

/* ------------------------------------------------------------------------- *
 * 3e. The likelihood given genotype priors on BOTH components, with markers left out (DESIGN.md section 16;
 *     --MatchedNormal).  Not in the reference.  In the notation of 3d, a pair hypothesis h carries two float32 triples per
 *     panel marker, pi1_h[m] for the contaminant (g1) and pi2_h[m] for the intended sample (g2):
 *         L_m(pc1, pc2, alpha | h) = sum_g1 P1[g1] sum_g2 P2[g2] W[g1][g2]
 *             P1 = pi1_h[m] where that triple is not all zero, else GF1(pc1)[m]      (3d's rule)
 *             P2 = pi2_h[m] where that triple is not all zero, else GF2(pc2)[m]
 *             a marker whose pi2_h[m][0] is negative is LEFT OUT: not walked, adds nothing
 *         LLK(. | h) = sum_m log L_m  over the walked markers with L_m > 0  (h:310)
 *     With pi2 all zero and no marker left out this is vb2_conditioned_eval; with both all zero vb2_llk_eval_batch; with
 *     both all zero on a set S and the rest left out vb2_replicates_eval under the 0/1 weights of S; LLK(pc1, pc2, alpha |
 *     pi1 = a, pi2 = b) = LLK(pc2, pc1, 1 - alpha | pi1 = b, pi2 = a).  alpha is the share of the non-intended component,
 *     reported as fitted and never folded at 0.5.
 *     The paired refit of a tumour given its matched normal: pi1 all zero (an anonymous contaminant at a searched
 *     ancestry), pi2 = the normal's genotype posterior q (3b) where the normal counts the marker and max(q[0], q[2]) >=
 *     hom_min, every other marker left out -- a tumour's allelic imbalance at its heterozygous sites cannot pass for
 *     contamination.  A wrong normal yields a meaningless alpha: identity is vb2_cohort_run_related's to check.
 * ------------------------------------------------------------------------- */
typedef struct vb2_paired vb2_paired;

/* prior: [num_hyp][num_marker][6] float32 in panel order (num_marker = the context's), host memory: pi1[3] then pi2[3] per
 * marker.  Uploaded once and permuted on the device into the context's marker order (six planes per hypothesis); device
 * memory comes from the library's slab cache.  The context must outlive the set and must not be inside
 * vb2_ctx_search_begin / vb2_ctx_search_end when the set is used. */
int vb2_paired_create(vb2_ctx *ctx, int32_t num_hyp, const float *prior, vb2_paired **out);
/* Hypothesis h = the paired rule on the q row of sample normal[h] of a source set (3b), device to device; hom_min within
 * [0, 1] (0 keeps every marker the normal counts).  The set must be of the context's panel size and on the context's
 * device, and the normal must have a row: VB2_ERR_INVALID otherwise. */
int vb2_paired_create_from_set(vb2_ctx *ctx, vb2_source_set *set, int32_t num_hyp, const int32_t *normal, double hom_min,
                               vb2_paired **out);
void vb2_paired_destroy(vb2_paired *pair);
/* One step: hypothesis h evaluates num_point[h] (0..VB2_BATCH_SLOTS) points; rows concatenated in hypothesis order as in
 * vb2_conditioned_eval.  A point's value is the same bits whatever else the step holds and from call to call; a hypothesis
 * that leaves every marker out evaluates to 0.0; an alpha outside [0, 1] leaves every marker out. */
int vb2_paired_eval(vb2_paired *pair, const int32_t *num_point, const double *pc1, const double *pc2, const double *alpha,
                    double *llk_out);
/* The refit of every hypothesis of every set, all in ONE lock-step gang: the reference-exact OptimizeLLK under a copy of
 * `model` with is_heter = 0, whose pc2 rows are overwritten with pc2_fixed on their way to the device, the llk0 call
 * included -- alpha and the contaminant's PCs are searched (alpha alone with is_pc_fixed or known allele frequencies);
 * is_alpha_fixed is VB2_ERR_INVALID.  pc2_fixed: [num_set][num_pc], one row per set.  Sets on different contexts overlap
 * on the device.  est_out / status: [sum of num_hyp] in set order; est_out has alpha, pc1 (in pc and pc2), llk1 and llk0.
 * status: VB2_OK, or VB2_ERR_INVALID for a hypothesis whose first evaluation is exactly 0.0 everywhere (no walked marker;
 * the others finish).  All sets must share num_pc.  The return value: an error that concerns all. */
int vb2_paired_optimize_llk(vb2_paired *const *sets, int32_t num_set, const vb2_model *model, const double *pc2_fixed,
                            vb2_estimate *est_out, int32_t *status);
typedef struct vb2_paired_info {
    int32_t num_hyp;
    int32_t num_marker;
    int64_t device_bytes;      /* device memory the set holds beyond the context's                   */
    int64_t num_step;          /* evaluations that reached the device (the searches' steps included)  */
    int64_t num_launch;        /* marker-kernel launches of those steps                               */
} vb2_paired_info;
/* given [num_hyp] or NULL: the context's counted markers that hypothesis h does not leave out */
int vb2_paired_info_get(const vb2_paired *pair, vb2_paired_info *info, int64_t *given);
/* The same driver over a caller's evaluator: no device needed.  The pc2 rows fn sees are pc2_fixed [num_hyp][num_pc] at
 * every call, the llk0 call included.  Non-zero from fn ends every search and is returned. */
typedef int (*vb2_paired_eval_fn)(void *user, int32_t num_hyp, const int32_t *num_point, const double *pc1,
                                  const double *pc2, const double *alpha, double *llk);
int vb2_paired_lockstep(vb2_paired_eval_fn fn, void *user, int32_t num_hyp, int32_t num_pc, const vb2_model *model,
                        const double *pc2_fixed, vb2_estimate *est_out, int32_t *status);

/* 3f. Derivatives of LLK(. | h) and the interval of a paired refit.  Section 10's math with 3e's
 *     rule per marker and per side: where a side's triple is given, its prior is that triple and nothing at the marker
 *     depends on that side's PCs (P' = P'' = 0 there); a left-out marker adds nothing; a marker counts where L > 0.
 *
 * vb2_paired_derivs: hypothesis h evaluates num_point[h] >= 0 points (any number; chunks inside), rows concatenated in
 * hypothesis order as in vb2_paired_eval: llk [sum], grad [sum][2k+1], hess [sum][2k+1][2k+1] in the order pc1 pc2 alpha, as
 * vb2_llk_derivs_batch returns them.  Every chunk is ONE launch pair over all hypotheses that still have points.  A point's
 * results are the same bits whatever else the call holds and from call to call; with both sides all zero and no marker
 * left out they are vb2_llk_derivs_batch's bits; the blocks of a side whose prior is given at every walked marker are
 * exactly 0; a hypothesis that leaves every marker out gives zeros.  The per-hypothesis marker scratch comes from the slab
 * cache on the first call and is counted in vb2_paired_info.device_bytes from then on. */
int vb2_paired_derivs(vb2_paired *pair, const int32_t *num_point, const double *pc1, const double *pc2, const double *alpha,
                      double *llk, double *grad, double *hess);
/* The same for every hypothesis of every set -- the sets may be on different contexts of one device and must share num_pc --
 * every chunk still ONE launch pair: num_point [sum of num_hyp] in set order, rows and results concatenated in that order.
 * A point's results are vb2_paired_derivs' bits on its own set. */
int vb2_paired_derivs_sets(vb2_paired *const *sets, int32_t num_set, const int32_t *num_point, const double *pc1,
                           const double *pc2, const double *alpha, double *llk, double *grad, double *hess);
/* The interval of every hypothesis of every set at est[] (the results of vb2_paired_optimize_llk under `model` with the same
 * pc2_fixed [num_set][num_pc]), all in ONE lock-step gang: every step is ONE launch pair with the point of every interval
 * still running, whatever set or context it is on (all on one device).  alpha is reported as fitted, never folded: the
 * profile runs over alpha in [0, 1], lo = 0 where the profile at 0 is above the cut and hi = 1 where the profile at 1 is.
 * Free parameters: the contaminant's PCs, then logit alpha; alpha alone with is_pc_fixed or known allele frequencies;
 * is_alpha_fixed is VB2_ERR_INVALID.  Rows of vb2_interval: row 0 is alpha (in `freemix`, row_kind 0), then the
 * ContaminatingSample.PC rows (row_kind 1) as fitted.  out / status: [sum of num_hyp] in set order; out[i] is bit for bit
 * what the hypothesis gives alone; status VB2_ERR_INVALID for a hypothesis that walks no marker (the others finish).
 * *num_step (may be NULL): the launch pairs taken = the largest num_launch. */
int vb2_paired_interval(vb2_paired *const *sets, int32_t num_set, const vb2_model *model, const double *pc2_fixed,
                        const vb2_estimate *est, vb2_interval *out, int32_t *status, int64_t *num_step);
/* The same driver over a caller's derivative evaluator (vb2_batch_derivs_fn, one slot per hypothesis): no device needed.
 * held: 0 none -- vb2_intervals_lockstep's intervals bit for bit, fold included --, 1 pc1, 2 pc2; fixed [num_hyp][num_pc]
 * the held side's PCs (NULL with held = 0), which are what fn sees on that side at every call.  held = 1 is the interval
 * of a refit given the contaminant (3d): its rows after row 0 are the IntendedSample.PC rows. */
int vb2_paired_intervals_lockstep(vb2_batch_derivs_fn fn, void *user, int32_t num_hyp, int32_t num_pc,
                                  const int32_t *data_has_known_af, const vb2_model *model, int32_t held, const double *fixed,
                                  const vb2_estimate *est, vb2_interval *out, int32_t *status, int64_t *num_step);

/* ------------------------------------------------------------------------- *
 * 3g. Reference bias (--RefBias).  Not in the reference (VerifyBamID 1 had --free-refBias): its
 *     model with beta = P(an error-free read of a heterozygous genotype shows REF) in place of the constant 0.5 of
 *     h:164-177.  g counts ALT alleles, e = 10^(-q/10):
 *         class ref:  u(g; e, beta) = (g/6) e     + n_beta(g) (1 - e),          n_beta = {1, beta, 0}[g]
 *         class alt:  u(g; e, beta) = ((2-g)/6) e + n_(1-beta)(2 - g) (1 - e)   -- the ref entry at 1 - beta, read mirrored
 *         p(read | g1, g2, alpha, beta) = (alpha e1 + (1 - alpha) e2) p_err + (alpha n1 + (1 - alpha) n2) p_ok   (h:223-225)
 *     W, GF1, GF2 and L = sum GF1[g1] GF2[g2] W[g1][g2] stay as they are; a marker counts where L > 0; LLK = sum log L.
 *     At beta = 0.5 the entries are the reference's.  Only the entries of the four off-diagonal pairs with a heterozygous
 *     genotype and of (het, het) depend on beta.  LLK(.; beta) of a sample is LLK(.; 1 - beta) of the sample with REF and
 *     ALT exchanged (classes swapped, every allele frequency AF -> 1 - AF).  The domain of beta is [VB2_REFBIAS_MIN, VB2_REFBIAS_MAX] = [0.25, 0.75];
 *     outside it the entries of this section return VB2_ERR_INVALID.
 *     Every llk1 of this section is a LOG-LIKELIHOOD (what .selfSM prints as FREELK1: minus vb2_estimate.llk1).
 * ------------------------------------------------------------------------- */
#define VB2_REFBIAS_MIN 0.25
#define VB2_REFBIAS_MAX 0.75
#define VB2_REFBIAS_NUM_PAIR 28
typedef struct vb2_refbias vb2_refbias;

/* A set of num_row (1..65535) values of beta over the ONE resident sample of the context: one double per row, host memory.
 * On a probability-domain context (vb2_info.layout 1) whose deepest marker's (het, het) term may fall below 2^-450 at beta =
 * 0.5 the set is refused with VB2_ERR_INVALID -- a het factor at beta >= 0.25 is at least half its value at 0.5, so the
 * bound of the layout (2^-900) would no longer hold; the message names the tunable pd, whose value 0 gives run words, which
 * take any depth.  The context must outlive the set and must not be inside vb2_ctx_search_begin / vb2_ctx_search_end when
 * the set is used. */
int vb2_refbias_create(vb2_ctx *ctx, int32_t num_row, const double *beta, vb2_refbias **out);
void vb2_refbias_destroy(vb2_refbias *set);
/* One step: row r evaluates num_point[r] (0..VB2_BATCH_SLOTS) points at its beta; rows concatenated in row order as in
 * vb2_conditioned_eval.  A point's value is the same bits whatever else the step holds and from call to call; an alpha
 * outside [0, 1] leaves every marker out. */
int vb2_refbias_eval(vb2_refbias *set, const int32_t *num_point, const double *pc1, const double *pc2, const double *alpha,
                     double *llk_out);
/* The profile refit of every row in lock-step: the reference-exact OptimizeLLK under `model` as it is (Heter, Homo,
 * is_pc_fixed, known allele frequencies; no side is held), every evaluation at the row's beta.  is_alpha_fixed is
 * VB2_ERR_INVALID.  est_out / status: [num_row]. */
int vb2_refbias_optimize_llk(vb2_refbias *set, const vb2_model *model, vb2_estimate *est_out, int32_t *status);
typedef struct vb2_refbias_info {
    int32_t num_row;
    int32_t num_marker;
    int64_t device_bytes;      /* device memory the set holds beyond the context's                   */
    int64_t num_step;          /* evaluations that reached the device (the searches' steps included)  */
    int64_t num_launch;        /* marker-kernel launches of those steps                               */
} vb2_refbias_info;
int vb2_refbias_info_get(const vb2_refbias *set, vb2_refbias_info *info);

/* The estimate of beta: the maximum of the profile likelihood l(beta) = max over the model's parameters of LLK(.; beta),
 * every value of l one search of vb2_refbias_optimize_llk, found by a fixed procedure in lock-step rounds:
 *   round 0        the nine values 0.25 + j / 16, j = 0..8 (beta = 0.5 is value 4);
 *   rounds 1..3    the interval between the two neighbours of the best value (the lowest index on ties; a best value at
 *                  an end of its round takes the end's neighbour as the centre, so the interval never leaves the round's
 *                  values nor the domain); nine equally spaced values on it, of which the ends and the centre are known:
 *                  six new searches per round, the last spacing 2^-10;
 *   beta           the vertex of the parabola through the last round's best value and its two neighbours; that value
 *                  itself where it is the first or last of its round (at_bound: and 0.25 or 0.75) or where the three lie
 *                  on no concave parabola;
 *   beta_se        sqrt(-1 / l'') from the parabola through the last round's two ends and its centre (spacing 2^-8: the
 *                  searches' own tolerance leaves about 1e-3 nats of noise on every l); NAN where l'' is not negative;
 *   final          one more search at beta: alpha_bias, pc, pc2, llk1_bias;  lrt = 2 (llk1_bias - l(0.5)).
 * 27 + 1 searches in 4 + 1 lock-step calls.  A search that fails puts its status into `status` and ends the fit with
 * VB2_ERR_INVALID. */
typedef struct vb2_refbias_fit {
    double beta, beta_se;
    double alpha_bias, llk1_bias;      /* the final search; alpha as fitted (FREEMIX_BIAS = min(alpha, 1 - alpha))    */
    double pc[VB2_MAX_PC], pc2[VB2_MAX_PC];
    double llk1_at_half, alpha_at_half, lrt;
    double pair_beta[VB2_REFBIAS_NUM_PAIR], pair_llk1[VB2_REFBIAS_NUM_PAIR];   /* in the order evaluated; the last: the final */
    int64_t num_step;                  /* lock-step steps of all calls                                                */
    int32_t at_bound;
    int32_t num_round;                 /* 4                                                                           */
    int32_t num_refit;                 /* searches: 28                                                                */
    int32_t num_pair;                  /* pairs filled in                                                             */
    int32_t status;                    /* VB2_OK, or the status of the search that failed                             */
    int32_t reserved;
} vb2_refbias_fit;
/* the whole procedure on a context (one vb2_refbias set per call) */
int vb2_refbias_fit_ctx(vb2_ctx *ctx, const vb2_model *model, vb2_refbias_fit *out);
/* The same procedure over a caller's evaluator: no device needed.  A step calls fn once, on the calling thread's own stack,
 * with the call's rows beta [num_row]; num_point[r] = 0 for a row that has finished.  Non-zero from fn ends the fit and is
 * returned. */
typedef int (*vb2_refbias_eval_fn)(void *user, int32_t num_row, const int32_t *num_point, const double *beta, const double *pc1,
                                   const double *pc2, const double *alpha, double *llk);
int vb2_refbias_lockstep(vb2_refbias_eval_fn fn, void *user, int32_t num_pc, const vb2_model *model, int32_t data_has_known_af,
                         vb2_refbias_fit *out);
/* vb2_run, then vb2_refbias_fit_ctx on the run's context under the run's model, then <output_prefix>.RefBias
 * (tab-separated, default ostream formatting):
 *     #SEQ_ID FREEMIX FREEMIX_BIAS REF_BIAS REF_BIAS_SE LRT FREELK1_BIAS FREELK1_HALF AT_BOUND
 * FREEMIX is the run's own, as in .selfSM.  stdout, .selfSM and .Ancestry are what vb2_run writes, byte for byte.  One
 * device and a searched alpha only: VB2_ERR_INVALID otherwise, before any file is read. */
int vb2_run_refbias(const vb2_run_args *args, vb2_run_result *out, vb2_refbias_fit *fit);

/* ------------------------------------------------------------------------- *
 * 3h. Empirical base-error rates (--FitError).  Not in the reference: its model with an error rate
 *     eps[q] per clamped quality q = 0..93 in place of pErr(q) = 10^(-q/10) (ContaminationEstimator.h:65-74), the nominal
 *     table eps0[q] = pow(10.0, q / -10.0):
 *         p(read | g1, g2) = (alpha E[g1][c] + (1 - alpha) E[g2][c]) eps_q + (alpha N[g1][c] + (1 - alpha) N[g2][c]) (1 - eps_q)
 *     (h:223-225; E, N = COND_LK[1], COND_LK[0], c = ref, alt, other).  W, GF1, GF2, L = sum GF1[g1] GF2[g2] W[g1][g2], "a
 *     marker counts where L > 0" and LLK = sum log L stay as they are.  Every llk of this section is a LOG-LIKELIHOOD.
 * ------------------------------------------------------------------------- */
#define VB2_ERR_NUM_QUAL 94
#define VB2_ERRFIT_MAX_ITER 24

/* vb2_ctx_create under an error table: err_table [VB2_ERR_NUM_QUAL] replaces pErr(q) in every table the context builds and
 * nothing else; NULL is vb2_ctx_create, and so are the nominal values, byte for byte.  An entry outside [0, 1] or a NaN is
 * VB2_ERR_INVALID. */
int vb2_ctx_create_ex(const vb2_input *in, const vb2_options *opt, const double *err_table, vb2_ctx **out);

/* The E-step.  A set holds a device copy of the RAW input (bases, qualities, offsets, alt alleles, panel rows or known
 * allele frequencies, the depth filter's constants): `in` is not referenced after the call returns.  opt: the device (and
 * stream) as for vb2_ctx_create; flags are ignored. */
typedef struct vb2_errstat vb2_errstat;
int vb2_errstat_create(const vb2_input *in, const vb2_options *opt, vb2_errstat **out);
void vb2_errstat_destroy(vb2_errstat *set);
/* At (pc1, pc2, alpha) under err_table, over the markers that count there (the context's rules: a non-empty range, the
 * +-3 sd depth filter unless disabled, L > 0 as the reference forms it): per quality n_out = their reads, all three classes,
 * and s_out = the sum of P(the read is an error | all reads of its marker) -- a class-other read counts 1 --; *llk_out =
 * sum log L (vb2_llk_eval_batch on a context of the same table, to rounding).  Any of the three may be NULL.  All are the
 * same bits from call to call and whatever the launch's grid: s is summed in 64-bit fixed point (what a read loses is below
 * 2^-64) and rounded once.  alpha outside [0, 1] (or NaN) and a bad table are VB2_ERR_INVALID.  Synchronous; host pointers. */
int vb2_errstat_eval(vb2_errstat *set, const double *err_table, const double *pc1, const double *pc2, double alpha,
                     int64_t *n_out, double *s_out, double *llk_out);
typedef struct vb2_errstat_info {
    int32_t num_marker;
    int32_t num_pc;
    int64_t num_read;
    int64_t device_bytes;      /* device memory the set holds                                        */
    int64_t num_launch;        /* kernel launches so far (two per evaluation)                        */
} vb2_errstat_info;
int vb2_errstat_info_get(const vb2_errstat *set, vb2_errstat_info *info);

/* The E-step of up to VB2_ERRSTAT_BATCH_MAX samples in one launch pair: a set holds the RAW inputs
 * of all of them on one device.  in [num_sample]; a NULL in[s] is a sample that holds nothing (one that failed its own run).
 * Inputs whose ud and means pointers -- or known_af pointers -- are equal, with equal num_marker and num_pc, share one
 * device copy: the samples of a cohort share the panel.  The inputs are not referenced after the call returns. */
#define VB2_ERRSTAT_BATCH_MAX 64
typedef struct vb2_errstat_batch vb2_errstat_batch;
int vb2_errstat_batch_create(const vb2_input *const *in, int32_t num_sample, const vb2_options *opt, vb2_errstat_batch **out);
void vb2_errstat_batch_destroy(vb2_errstat_batch *set);
/* Every live sample at its own point under its own table: live [S] (NULL: all), err_tables [S][94] (a pooled fit passes the
 * same table S times), pc1 / pc2 [S][num_pc] with num_pc the set's (vb2_errstat_batch_info: the largest of the samples'; a
 * sample reads its own first entries; NULL where every live sample has known allele frequencies), alpha [S]; n_out [S][94],
 * s_out [S][94], llk_out [S], any of which may be NULL.  For every live sample the three are BIT FOR BIT what
 * vb2_errstat_eval returns for that sample alone at the same point and table, whatever the other samples of the call.  A
 * sample that is not live, was NULL, or has num_marker == 0 takes no workgroup and reads zeros and llk 0.  A bad table, or
 * an alpha outside [0, 1], of a live sample is VB2_ERR_INVALID; what belongs to a sample that is not live is not read.
 * Synchronous; host pointers. */
int vb2_errstat_batch_eval(vb2_errstat_batch *set, const int32_t *live, const double *err_tables, const double *pc1,
                           const double *pc2, const double *alpha, int64_t *n_out, double *s_out, double *llk_out);
typedef struct vb2_errstat_batch_info {
    int32_t num_sample;
    int32_t num_pc;            /* the largest num_pc of the samples: the row stride of pc1 / pc2        */
    int32_t num_panel;         /* device copies of (ud, means) or known_af the samples share            */
    int32_t last_grid;         /* workgroups of the last evaluation's marker kernel                     */
    int64_t num_marker;        /* summed over the samples                                               */
    int64_t num_read;
    int64_t device_bytes;      /* device memory the set holds                                           */
    int64_t num_launch;        /* kernel launches so far (two per evaluation with a live sample)        */
    int64_t num_eval;          /* evaluations so far                                                    */
} vb2_errstat_batch_info;
int vb2_errstat_batch_info_get(const vb2_errstat_batch *set, vb2_errstat_batch_info *info);

/* The fit: alternating maximisation of the likelihood penalised by a Beta prior of prior_reads pseudo-reads centred on
 * the nominal rate of every quality.
 *   start      eps_0 = eps0, est_0 = `nominal` (the run's own estimate);
 *   iteration  (n, s) at (est_t, eps_t); eps_{t+1}[q] = (s[q] + kappa eps0[q]) / (n[q] + kappa) where n[q] > 0, eps0[q]
 *              elsewhere, ROUNDED TO THE NEAREST float32 and stored as that double; then the reference-exact OptimizeLLK
 *              under the caller's model from the reference's start, every evaluation under eps_{t+1} -> est_{t+1};
 *   stop       after the iteration in which max over n[q] > 0 of |eps_{t+1}[q] - eps_t[q]| / eps_t[q] <= tol (a bin whose
 *              eps_t is 0 counts as changed unless eps_{t+1} is 0 too), else after max_iter iterations with converged = 0;
 *   report     one more (n, s) at the final (est, eps); lrt = 2 (llk_fit - llk_nominal), num_bin = qualities with reads.
 * The points handed to the statistics are the search's own: the reported PCs with the reference's swap of indices 0 and 1
 * for alpha >= 0.5 (ContaminationEstimator.cpp:146-149) undone.  is_alpha_fixed is VB2_ERR_INVALID.  A search that fails
 * puts its code into status and ends the fit with that code. */
typedef struct vb2_errfit_opts {
    double prior_reads;        /* kappa; 0 = 100; negative or NaN: VB2_ERR_INVALID                    */
    double tol;                /* 0 = 1e-4                                                            */
    int32_t max_iter;          /* 0 = 24; at most VB2_ERRFIT_MAX_ITER                                 */
    int32_t reserved;
} vb2_errfit_opts;
typedef struct vb2_errfit {
    double err[VB2_ERR_NUM_QUAL];
    int64_t n[VB2_ERR_NUM_QUAL];
    double s[VB2_ERR_NUM_QUAL];
    vb2_estimate est;          /* the final search under err                                          */
    double llk_fit, llk_nominal, alpha_nominal, lrt;
    double iter_llk[VB2_ERRFIT_MAX_ITER];      /* the iteration's search: its log-likelihood,       */
    double iter_change[VB2_ERRFIT_MAX_ITER];   /* the stop rule's maximum,                           */
    double iter_alpha[VB2_ERRFIT_MAX_ITER];    /* and alpha as fitted                                */
    float iter_err[VB2_ERRFIT_MAX_ITER][VB2_ERR_NUM_QUAL];      /* eps_{t+1}: every entry is a float32 */
    int64_t num_step;          /* likelihood evaluations of all searches (the reference's count)      */
    int32_t num_bin, num_iter, converged;
    int32_t status;            /* VB2_OK, or the code of the search that failed                       */
} vb2_errfit;
/* the procedure on the device: one vb2_errstat, one fresh context per iteration (vb2_ctx_create_ex, vb2_ctx_optimize_llk) */
int vb2_errfit_input(const vb2_input *in, const vb2_options *opt, const vb2_model *model, const vb2_estimate *nominal,
                     const vb2_errfit_opts *fit_opts, vb2_errfit *out);
/* The same procedure over a caller's two callbacks: no device needed.  eval answers the searches (the seam of
 * vb2_optimize_llk with the table in front); stats is the E-step.  Non-zero from either ends the fit and is returned. */
typedef struct vb2_errfit_fns {
    int (*eval)(void *user, const double *err_table, int32_t num_point, const double *pc1, const double *pc2,
                const double *alpha, double *llk_out);
    int (*stats)(void *user, const double *err_table, const double *pc1, const double *pc2, double alpha, int64_t *n_out,
                 double *s_out);
} vb2_errfit_fns;
int vb2_errfit_lockstep(const vb2_errfit_fns *fns, void *user, int32_t num_pc, const vb2_model *model, int32_t data_has_known_af,
                        const vb2_estimate *nominal, const vb2_errfit_opts *fit_opts, vb2_errfit *out);
/* The fit of a cohort: the procedure above for up to VB2_ERRSTAT_BATCH_MAX samples in lock-step.
 * Each step is one batched E-step of the samples still fitting (vb2_errstat_batch_eval), fresh contexts under the new tables
 * (vb2_ctx_create_ex) and one vb2_batch_optimize_llk over them.
 *   per sample (pooled = 0)  every sample runs the procedure unchanged on its own table and leaves when it converges or
 *              reaches max_iter: fits[s] is what vb2_errfit_input gives on the sample alone (tables, n, iterations and
 *              convergence equal; what comes out of a search to the searches' own agreement);
 *   pooled     ONE table for all.  start: eps_0 = eps0, every sample at its own nominal estimate; iteration: (n_s, s_s)
 *              of every sample still in at (est_s,t, eps_t); N[q] = sum n_s[q] in integers, SUM[q] = the s_s[q] added in
 *              list order; eps_{t+1}[q] = (float)((SUM[q] + kappa eps0[q]) / (N[q] + kappa)) where N[q] > 0, eps0[q]
 *              elsewhere -- kappa is NOT scaled by the number of samples --; then the search of every sample under
 *              eps_{t+1}; stop: the rule above on the pooled table; report: one more E-step.  fits[s]: err the pooled
 *              table, n / s the sample's own at the end, iter_err / iter_change the pool's, iter_alpha / iter_llk its own.
 * A sample whose enter_status is not VB2_OK (its own run failed) never enters and keeps that code as fits[s].status, the
 * rest of fits[s] zeros and NaNs.  A sample whose context or search fails under a table gets that code as its status, is in
 * no later sum, and the others go on.  With one sample, pooled is the single-sample fit exactly. */
typedef struct vb2_errfit_pool {
    double err[VB2_ERR_NUM_QUAL];      /* pooled: the fitted table; per sample: the nominal one                         */
    int64_t n[VB2_ERR_NUM_QUAL];       /* the reported samples' final n summed,                                         */
    double s[VB2_ERR_NUM_QUAL];        /* ... and their s, added in list order                                          */
    double iter_change[VB2_ERRFIT_MAX_ITER];                     /* pooled only: the stop rule's maximum, and           */
    float iter_err[VB2_ERRFIT_MAX_ITER][VB2_ERR_NUM_QUAL];       /* eps_{t+1}                                            */
    double lrt_sum;                    /* the reported samples' lrt summed                                              */
    double seconds_stats, seconds_context, seconds_search;       /* vb2_errfit_cohort_inputs: where the time went       */
    int64_t num_step;                  /* likelihood evaluations of all searches                                        */
    int64_t device_bytes;              /* vb2_errfit_cohort_inputs: what the batched E-step's set held                  */
    int32_t num_bin;                   /* qualities with reads in n                                                     */
    int32_t num_iter;                  /* iterations run (per sample: the longest fit's)                                */
    int32_t converged;                 /* pooled: the pooled table's; per sample: every reported sample converged       */
    int32_t pooled;
    int32_t num_sample, num_entered, num_fitted;                 /* given; enter_status VB2_OK; reported                 */
    int32_t num_estep;                 /* batched E-steps                                                               */
} vb2_errfit_pool;
/* on the device `opt` names; the samples that enter have one num_pc and known allele frequencies all or none; nominal,
 * enter_status (or NULL: all enter), fits: [num_sample] */
int vb2_errfit_cohort_inputs(const vb2_input *const *in, int32_t num_sample, const vb2_options *opt, const vb2_model *model,
                             const vb2_estimate *nominal, const int32_t *enter_status, const vb2_errfit_opts *fit_opts,
                             int32_t pooled, vb2_errfit *fits, vb2_errfit_pool *pool);
/* The same procedure over a caller's two callbacks: no device needed.  eval answers the searches of sample `sample` (the
 * seam of vb2_optimize_llk with the sample and its table in front; non-zero fails that sample's search); stats is the
 * batched E-step with vb2_errstat_batch_eval's arrays (pc1 / pc2 [num_sample][num_pc]); non-zero from it ends the fit. */
typedef struct vb2_errfit_cohort_fns {
    int (*eval)(void *user, int32_t sample, const double *err_table, int32_t num_point, const double *pc1, const double *pc2,
                const double *alpha, double *llk_out);
    int (*stats)(void *user, int32_t num_sample, const int32_t *live, const double *err_tables, const double *pc1,
                 const double *pc2, const double *alpha, int64_t *n_out, double *s_out);
} vb2_errfit_cohort_fns;
int vb2_errfit_cohort_lockstep(const vb2_errfit_cohort_fns *fns, void *user, int32_t num_sample, int32_t num_pc,
                               const vb2_model *model, int32_t data_has_known_af, const vb2_estimate *nominal,
                               const int32_t *enter_status, const vb2_errfit_opts *fit_opts, int32_t pooled, vb2_errfit *fits,
                               vb2_errfit_pool *pool);

/* vb2_cohort_run, then the fit of the cohort (--PileupList L --CohortFitError [--PooledError]): an after-run stage that takes
 * every searched sample's flattened input as it retires (the readers leave the raw arrays in it) and then runs
 * vb2_errfit_cohort_inputs in chunks of at most VB2_ERRSTAT_BATCH_MAX samples, the run's own estimates the nominal ones, a
 * sample's own status its enter_status.  Per sample (pooled = 0): <prefix>.ErrorFit and <prefix>.ErrorRates of every fitted
 * sample, in vb2_run_errfit's formats.  Pooled: <output_prefix>.ErrorRates in the same format (READS = N, SE_BINOM from N)
 * and <output_prefix>.PooledFit, a header and one row per sample of the list:
 *     #SEQ_ID FREEMIX FREEMIX_FIT LRT FREELK1_FIT FREELK1_NOMINAL STATUS
 * ("NA" where a sample was not fitted; STATUS: the code it left with; SEQ_ID of a sample that failed its own run: its pileup
 * path).  One NOTICE line on stderr.  stdout, .selfSM and .Ancestry are what vb2_cohort_run writes, byte for byte; out and
 * status are its own.  fits [num_sample] and pooled_out may be NULL (pooled_out: the last chunk's).  VB2_ERR_INVALID before
 * any file is read: more than one device, is_alpha_fixed, --NumStart / --LineSearch, bad fit options, pooled with more than
 * VB2_ERRSTAT_BATCH_MAX samples.  Raw inputs that do not fit the device fail the stage (VB2_ERR_NOMEM, the byte counts in
 * the message) before any of them goes up. */
int vb2_cohort_run_errfit(const vb2_cohort_args *args, const vb2_errfit_opts *fit_opts, int32_t pooled, vb2_run_result *out,
                          int32_t *status, vb2_errfit *fits, vb2_errfit_pool *pooled_out);

/* --ErrorTable F: a fitted table applied to other runs.  vb2_err_table_read reads a file in the format of .ErrorRates --
 * a tab-separated header that names at least the columns #Q_REPORTED and ERROR_RATE, then a row per quality -- into
 * err_table [VB2_ERR_NUM_QUAL]: the file's rate of every quality it lists (*num_taken of them; may be NULL), the nominal
 * pow(10.0, q / -10.0) of the others.  VB2_ERR_INVALID, the message naming the line (1 = the header): a file that cannot be
 * opened, a missing column, too few fields, a quality that is no whole number within 0..93 or listed twice, a rate that
 * is no number, a NaN or outside [0, 1].  No device is touched.
 * vb2_run_under_table is vb2_run, and vb2_cohort_run_under_table is vb2_cohort_run, with every context made by
 * vb2_ctx_create_ex under err_table and nothing else changed: the same files, the same stdout; with the nominal table the
 * same bytes.  A bad table is VB2_ERR_INVALID before any file is read; vb2_run_under_table takes one device (no marker
 * shards). */
int vb2_err_table_read(const char *path, double *err_table, int32_t *num_taken);
int vb2_run_under_table(const vb2_run_args *args, const double *err_table, vb2_run_result *out);
int vb2_cohort_run_under_table(const vb2_cohort_args *args, const double *err_table, vb2_run_result *out, int32_t *status);

/* vb2_run, then the fit on the run's input under the run's model, the run's estimate the nominal one; then
 * <output_prefix>.ErrorFit (tab-separated, default ostream formatting):
 *     #SEQ_ID FREEMIX FREEMIX_FIT LRT NUM_BIN FREELK1_FIT FREELK1_NOMINAL ITERATIONS CONVERGED
 * and <output_prefix>.ErrorRates, one row per quality with reads:
 *     #Q_REPORTED READS EXPECTED_ERRORS ERROR_RATE Q_EMPIRICAL SE_BINOM
 * Q_EMPIRICAL = -10 log10 ERROR_RATE; SE_BINOM = sqrt(eps (1 - eps) / READS), a LOWER bound of the rate's standard error:
 * it takes every read's error indicator as observed.  One NOTICE line on stderr.  stdout, .selfSM and .Ancestry are what
 * vb2_run writes, byte for byte.  VB2_ERR_INVALID before any file is read: more than one device, is_alpha_fixed, --NumStart /
 * --LineSearch. */
int vb2_run_errfit(const vb2_run_args *args, const vb2_errfit_opts *fit_opts, vb2_run_result *out, vb2_errfit *fit);

/* Host-side flattening only (no device): reads panel + pileup, resolves markers
 * and returns the arrays of vb2_input in library-owned memory; free with
 * vb2_flat_free.  Lets callers (tests, shard planners) inspect or slice them. */
typedef struct vb2_flat vb2_flat;
int vb2_flat_load(const vb2_run_args *args, vb2_flat **out);
const vb2_input *vb2_flat_input(const vb2_flat *f);
int vb2_flat_stats(const vb2_flat *f, vb2_run_result *out);
void vb2_flat_free(vb2_flat *f);

/* --BamFile through the built-in reader (no htslib): BGZF, the header, the .bai index and the
 * record chain on the host, the per-marker pileup on args->device.  vb2_flat_load opens the file and its index before it
 * touches a device: an unreadable BAM is VB2_ERR_IO, a valid one without a GPU VB2_ERR_NO_DEVICE (no CPU fallback).
 * What one load did: */
typedef struct vb2_bam_stats {
    int64_t blocks;             /* BGZF blocks inflated (the header's included)                          */
    int64_t bytes_inflated;     /* ... and the bytes they held, the header's not included               */
    int64_t chunks;             /* merged chunks of the index that were read                            */
    int64_t records_seen;       /* records walked in them                                               */
    int64_t records_kept;       /* ... of which on a panel sequence and reaching a marker: sent up      */
    int64_t long_cigar_skipped; /* records whose CIGAR is in a CG tag (more than 65 535 operations)     */
    int64_t batches;            /* uploads (tunable bam_batch_kb)                                       */
    int64_t entries;            /* (record, marker) pairs that passed the read filters                  */
    int64_t sites;              /* markers some record spans: indexed sites                             */
    int64_t empty_sites;        /* ... of which without a base (every read below --min-BQ, or deleted)  */
    int64_t pairs_resolved;     /* overlapping mates met at a site                                      */
    int64_t capped_sites;       /* sites deeper than --max-depth                                        */
    double seconds_index;       /* open, header, index, plan                                            */
    double seconds_inflate;     /* inflate and walk                                                     */
    double seconds_device;      /* upload, kernels, sort                                                */
    double seconds_copyback;    /* pools back and the sites added                                       */
} vb2_bam_stats;
/* VB2_ERR_INVALID for a vb2_flat that was not loaded from a BAM by the built-in reader. */
int vb2_flat_bam_stats(const vb2_flat *f, vb2_bam_stats *out);

/* The host stage alone -- no device: the records the reader would send up for the markers of bed_path. */
/* (the handle cannot share the function's name: one namespace in C) */
typedef struct vb2_bam_scan_result vb2_bam_scan_result;
int vb2_bam_scan(const char *bam_path, const char *bed_path, vb2_bam_scan_result **out);
int vb2_bam_scan_stats(const vb2_bam_scan_result *scan, vb2_bam_stats *out);     /* the host fields; the others 0 */
/* Virtual offsets of the fetched records, ascending: returns their number, writes the first `capacity` (voffset may be
 * NULL with capacity 0). */
int64_t vb2_bam_scan_records(const vb2_bam_scan_result *scan, uint64_t *voffset, int64_t capacity);
/* @RG SM: of the header, "DefaultSampleName" without one (two different ones fail vb2_bam_scan itself) */
const char *vb2_bam_scan_sample(const vb2_bam_scan_result *scan);
void vb2_bam_scan_free(vb2_bam_scan_result *scan);

/* ---- per read group (--PerReadGroup) ----
 * The header's @RG lines, in header order and identified by ID:, are the groups of a BAM; a record belongs to the group its
 * RG field of type Z names, and to none without one, with an RG of another type or with an ID the header lacks.  Two
 * lines with one ID, a line without ID:, more than 65 535 lines, and groups x panel positions beyond 2^31 - 2 are
 * VB2_ERR_INVALID; so is an auxiliary field that does not fit its record, with the record's virtual offset in the message.
 * A group's pileup: the whole sample's site after the read filters, --max-depth and the mate-overlap rule, restricted to
 * the group's reads, then --min-BQ, the characters and the deletion quirk as for any site.
 *
 * vb2_bam_scan with flags: VB2_BAM_SCAN_GROUPS also parses the @RG lines and walks every kept record's auxiliary fields
 * (without it they are not looked at, and the three accessors below report no group).  No device. */
#define VB2_BAM_SCAN_GROUPS 1u
#define VB2_BAM_NO_GROUP 0xFFFFu
int vb2_bam_scan_ex(const char *bam_path, const char *bed_path, uint32_t flags, vb2_bam_scan_result **out);
int32_t vb2_bam_scan_num_group(const vb2_bam_scan_result *scan);
const char *vb2_bam_scan_group_id(const vb2_bam_scan_result *scan, int32_t group);       /* NULL out of range */
/* The kept records' group numbers (VB2_BAM_NO_GROUP = none), parallel to vb2_bam_scan_records: returns their number (0
 * for a scan without VB2_BAM_SCAN_GROUPS), writes the first `capacity`. */
int64_t vb2_bam_scan_record_groups(const vb2_bam_scan_result *scan, uint16_t *group, int64_t capacity);

/* vb2_flat_load of args->bam_path (built-in reader; a pileup_path is VB2_ERR_INVALID) and, beside the whole sample's
 * vb2_flat -- byte for byte what vb2_flat_load gives --, one vb2_flat per group over the same panel.  A group's status:
 * VB2_OK, VB2_ERR_SANITY (its own marker sanity check failed; not run with disable_sanity) or VB2_GROUP_NO_BASE (no base at
 * any marker).  Return codes as vb2_flat_load's: with VB2_ERR_SANITY for the whole sample both handles are still set; a
 * valid BAM without a GPU is VB2_ERR_NO_DEVICE after the file and its index were opened. */
#define VB2_GROUP_NO_BASE 1
typedef struct vb2_flat_groups vb2_flat_groups;
int vb2_flat_load_groups(const vb2_run_args *args, vb2_flat **whole, vb2_flat_groups **groups);
int32_t vb2_flat_groups_count(const vb2_flat_groups *g);
const char *vb2_flat_groups_id(const vb2_flat_groups *g, int32_t group);                 /* NULL out of range */
int64_t vb2_flat_groups_records(const vb2_flat_groups *g, int32_t group);                /* kept records naming it */
int32_t vb2_flat_groups_status(const vb2_flat_groups *g, int32_t group);
/* usable with vb2_flat_input and vb2_flat_stats; owned by the handle */
const vb2_flat *vb2_flat_groups_flat(const vb2_flat_groups *g, int32_t group);
int64_t vb2_flat_groups_unassigned(const vb2_flat_groups *g);                            /* kept records of no group */
/* what the groups' part of the load took beside the whole sample's vb2_bam_stats: second keys, second sort and sites on the
 * device; pools back and sites added on the host */
int vb2_flat_groups_seconds(const vb2_flat_groups *g, double *seconds_device, double *seconds_copyback);
void vb2_flat_groups_free(vb2_flat_groups *g);

/* vb2_run for the whole sample -- the same stdout, .selfSM, .Ancestry and .Pileup -- and then FREEMIX of every group under
 * the same model, the groups searched in lock-step in batches of at most 64 (vb2_batch_optimize_llk).  A group whose
 * status is not VB2_OK is not searched.  Writes <output_prefix>.selfRG (.selfSM's header; per group SEQ_ID = its SM: or the
 * sample, RG = its ID, #READS = its bases, FREEMIX / FREELK1 / FREELK0 "NA" when not searched) and, with output_pileup,
 * <output_prefix>.RG<header index>.Pileup per group.  group_results: the first `capacity` groups; *num_group: how many
 * the header has.  One device, no vb2_search_opts variants: VB2_ERR_INVALID otherwise, before any file is read. */
typedef struct vb2_group_result {
    vb2_run_result run;         /* est is zero for a group that was not searched */
    int32_t status;             /* as vb2_flat_groups_status */
    int32_t header_index;       /* 0-based @RG line */
    int64_t records;
} vb2_group_result;
int vb2_run_read_groups(const vb2_run_args *args, vb2_run_result *whole, int32_t capacity, vb2_group_result *group_results,
                        int32_t *num_group);

/* ---- BGZF blocks inflated on the device ----
 * The BGZF blocks of a buffer -- a whole file, or any run of whole blocks -- inflated on `device` (< 0: the current one):
 * the block headers are walked with the reader's own checks (a buffer that is not BGZF is VB2_ERR_INVALID or VB2_ERR_IO
 * with a message, before any device is touched), every block's deflate payload is inflated by one wave, in batches of
 * tunable bam_batch_kb.  NO zlib fallback and NO CRC32 here: block_status[b] is the device decoder's verdict (0 = the
 * block's ISIZE bytes are in `out`; 1 input exhausted, 2 output would pass ISIZE, 3 reserved block type, 4 stored LEN/NLEN,
 * 5 code lengths, 6 repeat, 7 symbol, 8 distance, 9 stream ends before ISIZE bytes, 10 step budget), and the bytes of a
 * block with another status are zero.  out holds the blocks' bytes back to back, *out_bytes of them (the sum of the
 * ISIZEs; VB2_ERR_INVALID when that passes out_capacity or the blocks pass status_capacity: *out_bytes and *num_block say
 * what is needed).  The built-in reader uses the same kernel with tunable bam_inflate = 1, and there inflates a block the
 * device refused again with zlib and checks every block's CRC32 on the host. */
int vb2_bgzf_inflate(const uint8_t *file_bytes, int64_t n_bytes, int32_t device, uint8_t *out, int64_t out_capacity,
                     int64_t *out_bytes, int32_t *block_status, int32_t status_capacity, int32_t *num_block);
/* What the device inflate of this process has done since the last reset, every caller counted (vb2_bgzf_inflate, and
 * the loads of the built-in reader under bam_inflate = 1): the stages of its batches, timed with events on its stream. */
typedef struct vb2_bgzf_stats {
    int64_t blocks;             /* blocks given to the kernel                                            */
    int64_t refused;            /* ... of which with a status other than 0                              */
    int64_t batches;            /* launches                                                             */
    int64_t bytes_raw;          /* deflate payload uploaded                                             */
    int64_t bytes_inflated;     /* bytes of the accepted blocks                                         */
    double seconds_upload;      /* payloads and job table up                                            */
    double seconds_kernel;
    double seconds_copyback;    /* inflated bytes and statuses down                                     */
    double seconds_stage;       /* host: inflated bytes out of the staging buffer                       */
} vb2_bgzf_stats;
int vb2_bgzf_inflate_stats(vb2_bgzf_stats *out, int32_t reset);

/* ---- --ApplyBAQ: base alignment quality and the mapping-quality cap on BAM input (vb2_run_args.bam_adjust) ----
 * The HMM is the reference's bundled samtools/kprobaln.c (kpa_glocal), the wrapper and the cap its samtools/bam_md.c
 * (bam_prob_realn_core with flag 3 or 7, bam_cap_mapQ), restated once for host and device (csrc/baq_core.h); the device
 * stage runs between a batch's upload and its cover pass.  Agreement with htslib 1.11's sam_prob_realn / sam_cap_mapq,
 * which the reference binary links, is UNPINNED. */
typedef struct vb2_baq_stats {
    int64_t records;            /* records the stage saw (vb2_bam_stats.records_kept)                     */
    int64_t realigned;          /* the HMM ran                                                            */
    int64_t left_alone;         /* by rule: unmapped, no bases, qualities 0xFF, an N operation, a ZQ tag  */
    int64_t tag_applied;        /* a BQ tag was there and applied (no redo)                               */
    int64_t no_reference;       /* the FASTA lacks the record's sequence: neither BAQ nor the cap         */
    int64_t dropped_outside;    /* pos >= the sequence's length in the .fai                               */
    int64_t dropped_cap;        /* the cap dropped the read                                               */
    int64_t not_asked;          /* BAQ off in the options (the cap may have run)                          */
    int64_t records_lds;        /* realigned with the matrix in LDS ...                                   */
    int64_t records_global;     /* ... and in global memory                                               */
    int64_t undefined_rows;     /* rows where the reference converts a NaN or an infinity to int: quality 0 */
    int64_t fasta_bytes;        /* bases read from the FASTA                                              */
    double seconds_fasta;       /* index, spans                                                           */
    double seconds_lds;         /* the kernel over the LDS tier (events)                                  */
    double seconds_global;      /* ... over the global tier                                               */
    double seconds_cap;         /* the cap's end on the host and its byte per record back up              */
    double seconds_stage;       /* the whole stage, host clock                                            */
} vb2_baq_stats;
/* VB2_ERR_INVALID for a vb2_flat that was not loaded with bam_adjust = 1 */
int vb2_flat_baq_stats(const vb2_flat *f, vb2_baq_stats *out);

/* Diagnostic: for the records vb2_bam_scan would send up, in its order, what the stage makes of them under `opts` (NULL or
 * given == 0: the defaults).  where = 0: baq_core.h's sequential host driver, no device (a diagnostic and the tests'
 * yardstick, NOT a fallback of the product); where = 1: the device stage, in upload batches of tunable bam_batch_kb. */
typedef struct vb2_baq_result vb2_baq_result;
int vb2_baq_records(const char *bam_path, const char *bed_path, const char *reference_path, const vb2_mpileup_opts *opts,
                    int where, int device, vb2_baq_result **out);
int64_t vb2_baq_result_num(const vb2_baq_result *r);
int64_t vb2_baq_result_qual_bytes(const vb2_baq_result *r);
/* qual_off [num + 1]: record i's adjusted qualities are qual[qual_off[i] .. qual_off[i + 1]); mapq [num]: after the cap, -1
 * = dropped; outcome [num]: 0 realigned, 1 left alone, 2 BQ tag applied, 3 no reference sequence, 4 outside the sequence,
 * 5 dropped by the cap, 6 BAQ not asked for; cap4 [4 * num]: mm, q, len, clip_q of the cap's walk.  Any may be NULL. */
int vb2_baq_result_copy(const vb2_baq_result *r, uint64_t *qual_off, uint8_t *qual, int16_t *mapq, uint8_t *outcome, int32_t *cap4);
int vb2_baq_result_stats(const vb2_baq_result *r, vb2_baq_stats *out);      /* where = 0: the counts; tiers and times 0 */
void vb2_baq_result_free(vb2_baq_result *r);
/* The HMM alone on the host: ref and query are codes 0..4, qual the base qualities, bw the band's configured width; state
 * and q as kpa_glocal fills them.  *undefined (may be NULL): the undefined rows. */
int vb2_baq_case(const uint8_t *ref, int32_t l_ref, const uint8_t *query, const uint8_t *qual, int32_t l_query, int32_t bw,
                 int32_t *state, uint8_t *q, int32_t *undefined);
/* (int)(-4.343*log(z) + .499) for 0 < z by the threshold table the device searches (above 100: 101) */
int32_t vb2_baq_quantise(double z);
/* bytes of a record's workspace: what sorts it into the LDS tier (<= tunable baq_lds_kb KiB / 4) or the global one */
uint64_t vb2_baq_work_bytes(int32_t l_ref, int32_t l_query, int32_t bw);
/* The FASTA reader alone: *length = the sequence's length in the .fai (VB2_ERR_INVALID when the FASTA lacks it); out (may
 * be NULL) gets the nt16 codes of [beg, end). */
int vb2_fasta_fetch(const char *fasta_path, const char *name, int64_t beg, int64_t end, uint8_t *out, int64_t *length);

/* ---- .bam lines in a cohort's list ----
 * A line of vb2_cohort_args.pileup_paths whose name ends in ".bam" is read by the built-in BAM reader (with base.mpileup,
 * on the sample's device), every other line as a text pileup; lists may mix the two.  A ".cram" name, or a file that
 * starts with the CRAM magic, is that sample's VB2_ERR_INVALID; an unreadable or corrupt BAM, or one without its index,
 * is that sample's status too (what went wrong is printed to stderr, the other samples run on).  A BAM sample's .selfSM
 * has the header's @RG SM: as SEQ_ID and its bases as #READS.  The host pool of one BAM load is 16 / reader threads,
 * and at most tunable cohort_bam_inflight (4) BAM samples per device are between "file opened" and "context created".
 * What the load of sample `sample` of this process's most recent cohort run did; VB2_ERR_INVALID for a sample that was
 * not read from a BAM (or whose load failed). */
int vb2_cohort_bam_stats(int32_t sample, vb2_bam_stats *out);

/* ------------------------------------------------------------------------- *
 * 4. Reference-panel builder: --RefVCF (main.cpp:233-257, SVDcalculator::
 *    ProcessRefVCF, SVDcalculator.cpp:363-400).  The kept markers' genotypes
 *    (0/1/2, -1 = missing or no likelihood below 255) become an int8 slab on the
 *    device; S = G^T G is exact (int8 MFMA, int32); mu, the centred Gram, its
 *    eigenbasis (rocSOLVER dsyevd, bound at run time) and UD = (G - mu 1^T) V are
 *    FP64.  Sign convention: each column of V is flipped so that its entry of
 *    largest magnitude is positive (the lowest index on ties); UD follows.
 * ------------------------------------------------------------------------- */
typedef struct vb2_panel_args {
    const char *vcf_path;      /* --RefVCF (vcf or vcf.gz); files go to <vcf_path>.UD/.mu/.bed/.V  */
    const char *include_chr;   /* --IncludeChr a,b,...; NULL = the 44 autosome names (main.cpp:69-73);
                                * "" = no chromosome filter                                      */
    int32_t num_svd_pcs;       /* --NumSVDPCs (10); <= 0 = all min(M, N)                          */
    int32_t skip_min_sample_count_check; /* --SkipMinSampleCountCheck                            */
    int32_t check_minimums;    /* vb2_panel_build_genotypes only: enforce >= 5000 markers and
                                * >= 1000 samples (unless skipped); the VCF entry always does   */
    int32_t num_thread;        /* --NumThread: VCF parser threads; 0 = 4                          */
    int32_t device;            /* HIP device ordinal, -1 = current                                */
    int32_t notices;           /* print the reference's NOTICE / WARNING lines to stderr          */
    int32_t chunk_markers;     /* markers per device chunk (a multiple of 128); 0 = 16384         */
    int32_t reserved;
} vb2_panel_args;

/* The kept markers of a VCF, read on the host only (SVDcalculator::ReadVcf).  Library-owned. */
typedef struct vb2_vcf vb2_vcf;
typedef struct vb2_vcf_view {
    int64_t num_marker;
    int32_t num_sample;
    int32_t num_chr;
    const int8_t *genotypes;       /* marker-major [num_marker][num_sample]                     */
    const int32_t *pos;            /* [num_marker] 1-based                                        */
    const int32_t *chr_index;      /* [num_marker] into chr_names                                 */
    const char *ref;               /* [num_marker] one base each                                  */
    const char *alt;               /* [num_marker]                                                */
    const char *const *chr_names;  /* [num_chr]                                                   */
    const char *const *sample_ids; /* [num_sample]                                                */
} vb2_vcf_view;
int vb2_vcf_read(const vb2_panel_args *args, vb2_vcf **out);
int vb2_vcf_get_view(const vb2_vcf *v, vb2_vcf_view *out);
void vb2_vcf_free(vb2_vcf *v);

typedef struct vb2_panel vb2_panel;
typedef struct vb2_panel_view {
    int64_t num_marker;            /* M                                                           */
    int32_t num_sample;            /* N                                                           */
    int32_t num_pc;                /* k: columns of ud and v                                      */
    const double *ud;              /* [M][k]                                                      */
    const double *v;               /* [N][k]                                                      */
    const double *mu;              /* [M] binary32 means, widened                                 */
    const double *sigma;           /* [N] descending: sqrt(max(lambda, 0)) of the centred Gram    */
    const int32_t *gram;           /* [N][N] S = G^T G of the raw genotypes                       */
    const int32_t *row_sum;        /* [M] sum_j g_mj                                              */
    /* wall-clock seconds: parse (reading, with the device work it overlaps), upload, gram,
     * centring, eigensolve, projection, write; device stages are event-timed */
    double seconds[7];
    double seconds_total;
} vb2_panel_view;
int vb2_panel_build(const vb2_panel_args *args, vb2_panel **out);
int vb2_panel_build_genotypes(const vb2_panel_args *args, const int8_t *genotypes /* [M][N] marker-major */,
                              int64_t num_marker, int32_t num_sample, vb2_panel **out);
int vb2_panel_get_view(const vb2_panel *p, vb2_panel_view *out);
/* <prefix>.UD, .mu, .bed, .V in the reference's format (WriteSVD, SVDcalculator.cpp:471-513);
 * a panel built from genotypes has no marker names and is VB2_ERR_INVALID here. */
int vb2_panel_write(vb2_panel *p, const char *prefix);
void vb2_panel_destroy(vb2_panel *p);

const char *vb2_last_error(void);
int vb2_abi_version(void);
/* Number of usable gfx950 devices (0 = none; compute calls will fail loudly). */
int vb2_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* VB2_ABI_H_ */
