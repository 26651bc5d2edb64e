// cli_main.cpp -- command line with the reference's flag names, defaults and
// output files for the contamination path (main.cpp:56-414), on top of the C-ABI.
//
//   VerifyBamID --SVDPrefix P --PileupFile F --Reference R [--NumPC k] [--Output o]
//               [--WithinAncestry] [--FixPC a:b:..] [--FixAlpha x] [--KnownAF f]
//               [--Epsilon e] [--DisableSanityCheck] [--OutputPileup] [--Verbose]
//               [--NumThread n] [--Seed s]      (+ deprecated --UDPath/--MeanPath/--BedPath)
//               [--min-BQ n] [--min-MQ n] [--adjust-MQ n] [--max-depth n] [--no-orphans]
//               [--incl-flags n] [--excl-flags n]      (the reference's "Pileup Options", main.cpp:176-187: --BamFile only)
//
// --Epsilon e is the simplex's relative tolerance; a value that is not positive (0, negative, NaN) means the default 1e-8.
// --BamFile B reads a coordinate-sorted BAM with its .bai through the built-in reader (no htslib):
// BGZF, index and records on the host (--NumThread above its default of 4 sizes that pool), the per-marker pileup on the
// GPU.  Without --ApplyBAQ, BAQ and the mapQ cap are not applied -- a NOTICE says so when the options ask for them, and
// names the reference command that matches what was computed (--incl-flags 1024 --adjust-MQ 0) -- and --Reference stays
// required and unread.  --ApplyBAQ (with --BamFile, or a --PileupList that has a .bam line) applies to every record what
// the effective pileup options ask of the FASTA at --Reference (plain, with its .fai), in the reference's order: the
// Illumina-1.3 shift, base alignment quality, the mapping-quality cap; one NOTICE says what was
// applied and from which file.  The reference base of a site is the panel's REF allele either way.  CRAM and .csi are
// not read.
// --RefVCF V [--NumSVDPCs k] [--SkipMinSampleCountCheck] [--IncludeChr a,b,..] [--GramSVD] builds a reference panel
// (main.cpp:233-257): V.UD, V.mu, V.bed, V.V, decomposed on the GPU (vb2_panel_build), and returns before --Reference
// is looked at.  --NumThread sizes the VCF parser pool there.
// Extensions: --Device n selects the GPU; --Devices a,b,.. uses several -- one sample's markers
// are sharded over them (partial log-likelihoods met in one RCCL all-reduce), a --PileupList
// cohort is dealt to them group by group; --PileupList F runs many samples against one panel.
// --ConfidenceInterval writes <Output>.CI for the sample of a --PileupFile / --BamFile run; --PileupList F --CohortInterval
// writes <output prefix>.CI for every sample of the cohort, the intervals computed in lock-step next to the search (one
// device; may be combined with --FindSource).
// --PerChromosome writes <Output>.Chrom -- FREEMIX refitted on every chromosome of the .bed alone and with it left out, and a
// delete-one-chromosome jackknife --, --Bootstrap N (1..1000, seeded by --Seed) <Output>.Boot: weighted-marker replicates of
// the one resident sample searched in lock-step (vb2_run_replicates; one sample, one device).
// --FindSource --RefitSource also writes <Output>.SourceFit: every sample's FREEMIX refitted GIVEN the genotypes of its best
// candidate, and the likelihood difference to the anonymous fit (vb2_cohort_run_source_fits; not with --FixAlpha,
// --CohortInterval or several --Devices).
// --RefBias estimates the reference bias beta -- the share of REF among the error-free reads of a heterozygous genotype,
// 0.5 in the model -- jointly with FREEMIX and writes <Output>.RefBias (vb2_run_refbias; one sample,
// one device, a searched alpha).
// --FitError [--ErrorPrior k] fits the error rate of every reported base quality jointly with FREEMIX, in place of the
// model's 10^(-q/10), and writes <Output>.ErrorFit and <Output>.ErrorRates (vb2_run_errfit); k is the
// weight of the nominal rate in pseudo-reads per quality (default 100).  With --PileupFile or --BamFile; one sample, one
// device, a searched alpha, the reference's own search: not with --PileupList, --PerReadGroup, --FixAlpha,
// --ConfidenceInterval, --PerChromosome, --Bootstrap, --RefBias, --NumStart, --LineSearch or several --Devices.
// --PileupList F --CohortFitError [--PooledError] [--ErrorPrior k] fits them for every sample of a cohort in lock-step after
// the run (vb2_cohort_run_errfit): each sample on its own table, to <prefix>.ErrorFit / .ErrorRates, or
// with --PooledError all on one, to <Output>.ErrorRates and <Output>.PooledFit.  One device, a searched alpha, the
// reference's own search, no other after-run stage (--FindSource, --FindRelated, --MatchedNormal, --CohortInterval).
// --ErrorTable F runs a plain --PileupFile / --BamFile / --PileupList run under the rates of F, a file in .ErrorRates format
// (columns #Q_REPORTED and ERROR_RATE; a quality it does not list stays nominal): what makes a pooled fit usable elsewhere.
// Not with any flag above that adds a stage, nor with --FitError / --CohortFitError.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/vb2_abi.h"

extern "C" int vb2_debug_set_tunable(const char* name, int value);      // (abi.cpp; csrc/tunables.h)

namespace {

struct Flag {
    enum Kind { kBool, kInt, kDouble, kString } kind;
    void* dst;
    bool seen;
};

void fatal(const char* msg)
{
    std::fprintf(stderr, "\nFATAL ERROR - \n%s\n\n", msg);
    std::exit(EXIT_FAILURE);
}

// One sample of a --PileupList cohort: the stdout block the reference prints for its sample (ContaminationEstimator.cpp:98-166,
// the "Estimation from Optimize..." title its model selects, then the PCs and FREEMIX in default ostream formatting) -- what
// vb2_run prints for the sample of a --PileupFile run.
void print_sample_summary(const vb2_model& m, int k, const vb2_estimate& est)
{
    const bool heter = m.is_heter && !m.is_af_known;
    const bool pcfix = (m.is_pc_fixed && m.fix_pc) || m.is_af_known;
    const bool afix = !pcfix && m.is_alpha_fixed;
    const char* title = !heter ? (pcfix ? "Estimation from OptimizeHomoFixedPC:" : afix ? nullptr : "Estimation from OptimizeHomo:")
                               : (pcfix ? "Estimation from OptimizeHeterFixedPC:"
                                        : afix ? "Estimation from OptimizeHeterFixedAlpha:" : "Estimation from OptimizeHeter:");
    if (title) std::printf("%s\n", title);
    std::printf("Contaminating Sample ");
    for (int i = 0; i < k; ++i) std::printf("PC%d:%g\t", i + 1, est.pc[i]);
    std::printf("\nIntended Sample ");
    for (int i = 0; i < k; ++i) std::printf("PC%d:%g\t", i + 1, est.pc2[i]);
    std::printf("\nFREEMIX(Alpha):%g\n", est.alpha < 0.5 ? est.alpha : 1 - est.alpha);
}

}  // namespace

int main(int argc, char** argv)
{
    std::fprintf(stderr,
                 "VerifyBamID2 (MI355X-native likelihood core): DNA contamination estimation from "
                 "sequence reads using ancestry-agnostic method.\n\n");

    // defaults: main.cpp:58-79
    std::string UDPath("Empty"), MeanPath("Empty"), BedPath("Empty"), BamFile("Empty"),
        RefPath("Empty"), outputPrefix("result"), PileupFile("Empty"), SVDPrefix("Empty"),
        knownAF("Empty"), fixPC("Empty"), PileupList("Empty"), Devices("Empty"), RefVCF("Empty");
    // --RefVCF mode (main.cpp:66-73): the default chromosome set is the 44 human autosome names
    int numSVDPCs = 10;
    bool skipMinSampleCountCheck = false, gramSVD = false;
    std::string includeChrStr("1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20,21,22,"
                              "chr1,chr2,chr3,chr4,chr5,chr6,chr7,chr8,chr9,chr10,"
                              "chr11,chr12,chr13,chr14,chr15,chr16,chr17,chr18,chr19,"
                              "chr20,chr21,chr22");
    double fixAlpha = -1., epsilon = 1e-8;
    bool withinAncestry = false, outputPileup = false, verbose = false, disableSanityCheck = false;
    int seed = 12345, nPC = 2, nthread = 4, device = -1, numStart = 1;
    bool lineSearch = false;
    bool confidenceInterval = false;
    bool cohortInterval = false;
    bool findSource = false;
    int sourceTop = 3;
    bool refitSource = false;
    bool findRelated = false;
    int relatedTop = 3;
    bool perChromosome = false;
    int bootstrap = 0;
    std::string MatchedNormal("Empty");
    double normalHomMin = 0.99;
    bool pairInterval = false;
    bool perReadGroup = false;
    bool applyBAQ = false;
    bool refBias = false;
    bool fitError = false;
    bool cohortFitError = false, pooledError = false;
    double errorPrior = 100.0;
    std::string ErrorTable("Empty");
    // "Pileup Options" (main.cpp:176-187), defaults main.cpp:81-96 (MPLP_REALN | MPLP_SMART_OVERLAPS; UNMAP | SECONDARY |
    // QCFAIL | DUP): they shape what --BamFile input becomes and, as in the reference, do nothing to --PileupFile input
    int minBQ = 13, minMQ = 2, adjustMQ = 40, maxDepth = 8000, inclFlags = (1 << 4) | (1 << 10), exclFlags = 0x4 | 0x100 | 0x200 | 0x400;
    bool noOrphans = false;

    std::map<std::string, Flag> flags = {
        {"BamFile", {Flag::kString, &BamFile, false}},
        {"PileupFile", {Flag::kString, &PileupFile, false}},
        {"Reference", {Flag::kString, &RefPath, false}},
        {"SVDPrefix", {Flag::kString, &SVDPrefix, false}},
        {"Output", {Flag::kString, &outputPrefix, false}},
        {"WithinAncestry", {Flag::kBool, &withinAncestry, false}},
        {"DisableSanityCheck", {Flag::kBool, &disableSanityCheck, false}},
        {"NumPC", {Flag::kInt, &nPC, false}},
        {"FixPC", {Flag::kString, &fixPC, false}},
        {"FixAlpha", {Flag::kDouble, &fixAlpha, false}},
        {"KnownAF", {Flag::kString, &knownAF, false}},
        {"NumThread", {Flag::kInt, &nthread, false}},
        {"Seed", {Flag::kInt, &seed, false}},
        {"Epsilon", {Flag::kDouble, &epsilon, false}},
        {"OutputPileup", {Flag::kBool, &outputPileup, false}},
        {"Verbose", {Flag::kBool, &verbose, false}},
        {"UDPath", {Flag::kString, &UDPath, false}},
        {"MeanPath", {Flag::kString, &MeanPath, false}},
        {"BedPath", {Flag::kString, &BedPath, false}},
        {"min-BQ", {Flag::kInt, &minBQ, false}},
        {"min-MQ", {Flag::kInt, &minMQ, false}},
        {"adjust-MQ", {Flag::kInt, &adjustMQ, false}},
        {"max-depth", {Flag::kInt, &maxDepth, false}},
        {"no-orphans", {Flag::kBool, &noOrphans, false}},
        {"incl-flags", {Flag::kInt, &inclFlags, false}},
        {"excl-flags", {Flag::kInt, &exclFlags, false}},
        {"RefVCF", {Flag::kString, &RefVCF, false}},
        {"NumSVDPCs", {Flag::kInt, &numSVDPCs, false}},
        {"SkipMinSampleCountCheck", {Flag::kBool, &skipMinSampleCountCheck, false}},
        {"IncludeChr", {Flag::kString, &includeChrStr, false}},
        {"GramSVD", {Flag::kBool, &gramSVD, false}},
        {"Device", {Flag::kInt, &device, false}},
        {"Devices", {Flag::kString, &Devices, false}},
        // not in the reference: a cohort against one panel.  File of lines "<pileup>\t<output prefix>";
        // the panel is read once and the samples are searched in lock-step groups (vb2_cohort_run).
        {"PileupList", {Flag::kString, &PileupList, false}},
        // not in the reference: optimiser variants (vb2_search_opts).  --NumStart n searches from n
        // starting points in lock-step (start 0 = the reference's; the others add noise drawn from
        // --Seed) and reports the best; --LineSearch uses Brent's method (the reference's unused
        // MathGold) for the one-parameter models (--FixPC / --KnownAF).
        {"NumStart", {Flag::kInt, &numStart, false}},
        {"LineSearch", {Flag::kBool, &lineSearch, false}},
        // not in the reference: a 95% confidence interval for FREEMIX (profile likelihood) and standard errors of the free
        // parameters, written to <Output>.CI (vb2_run_interval)
        {"ConfidenceInterval", {Flag::kBool, &confidenceInterval, false}},
        // not in the reference: the same interval for every sample of a --PileupList cohort, <output prefix>.CI each, computed
        // in lock-step (vb2_cohort_run_intervals)
        {"CohortInterval", {Flag::kBool, &cohortInterval, false}},
        // not in the reference: which sample of the --PileupList cohort does each sample's contamination come from?  Every
        // pair's log-likelihood ratio (vb2_cohort_run_sources); the --SourceTop best candidates per sample go to <Output>.Sources
        {"FindSource", {Flag::kBool, &findSource, false}},
        {"SourceTop", {Flag::kInt, &sourceTop, false}},
        // not in the reference: after --FindSource, every sample's FREEMIX refitted given its best candidate's genotypes
        // (vb2_cohort_run_source_fits), to <Output>.SourceFit
        {"RefitSource", {Flag::kBool, &refitSource, false}},
        // not in the reference: which samples of the --PileupList cohort are the same individual, parent and child, full
        // siblings or second-degree relatives?  Every ordered pair's four log-likelihood ratios (vb2_cohort_run_related); the
        // --RelatedTop best partners per sample go to <Output>.Related
        {"FindRelated", {Flag::kBool, &findRelated, false}},
        {"RelatedTop", {Flag::kInt, &relatedTop, false}},
        // not in the reference: FREEMIX refitted on every chromosome alone and with every chromosome left out, with a
        // delete-one-chromosome jackknife (<Output>.Chrom), and over --Bootstrap N marker resamples seeded by --Seed
        // (<Output>.Boot): weighted-marker replicates of the one resident sample, searched in lock-step (vb2_run_replicates)
        {"PerChromosome", {Flag::kBool, &perChromosome, false}},
        {"Bootstrap", {Flag::kInt, &bootstrap, false}},
        // not in the reference: FREEMIX of the tumours of a --PileupList cohort given their matched normals' genotypes
        // (vb2_cohort_run_paired), to <Output>.PairFit.  File of lines "<tumour pileup>\t<normal pileup>", names as in the
        // list; only the markers where the normal is homozygous with a posterior of at least --NormalHomMin are used
        {"MatchedNormal", {Flag::kString, &MatchedNormal, false}},
        {"NormalHomMin", {Flag::kDouble, &normalHomMin, false}},
        // not in the reference: with --MatchedNormal, a 95% confidence interval (profile likelihood, unfolded) and a
        // standard error for every ALPHA_PAIRED, computed in lock-step (vb2_cohort_run_paired_intervals), to <Output>.PairCI
        {"PairInterval", {Flag::kBool, &pairInterval, false}},
        // not in the reference (VerifyBamID 1 had it): FREEMIX of every read group of the --BamFile header beside the whole
        // sample's, each from the group's own pileup, the groups searched in lock-step (vb2_run_read_groups), to <Output>.selfRG
        {"PerReadGroup", {Flag::kBool, &perReadGroup, false}},
        // the built-in BAM reader applies base alignment quality and the mapping-quality cap from --Reference (vb2_run_args.bam_adjust)
        {"ApplyBAQ", {Flag::kBool, &applyBAQ, false}},
        // not in the reference (VerifyBamID 1 had --free-refBias): the reference bias of the read model estimated jointly with
        // FREEMIX by profile likelihood, 28 refits of the one resident sample in lock-step (vb2_run_refbias), to <Output>.RefBias
        {"RefBias", {Flag::kBool, &refBias, false}},
        // not in the reference: the error rate per reported base quality fitted jointly with FREEMIX (vb2_run_errfit), to
        // <Output>.ErrorFit and <Output>.ErrorRates; --ErrorPrior: pseudo-reads at the nominal rate per quality
        {"FitError", {Flag::kBool, &fitError, false}},
        {"ErrorPrior", {Flag::kDouble, &errorPrior, false}},
        // ... of every sample of a --PileupList cohort in lock-step (vb2_cohort_run_errfit): each on its own table, or with
        // --PooledError all on one, to <Output>.ErrorRates and <Output>.PooledFit
        {"CohortFitError", {Flag::kBool, &cohortFitError, false}},
        {"PooledError", {Flag::kBool, &pooledError, false}},
        // a plain --PileupFile / --BamFile / --PileupList run under the error rates of a file in .ErrorRates format
        // (vb2_err_table_read, vb2_run_under_table, vb2_cohort_run_under_table)
        {"ErrorTable", {Flag::kString, &ErrorTable, false}},
    };
    for (int i = 1; i < argc; ++i) {
        const char* a = argv[i];
        if (std::strncmp(a, "--", 2) != 0) {
            std::fprintf(stderr, "WARNING - ignoring stray argument %s\n", a);
            continue;
        }
        auto it = flags.find(a + 2);
        if (it == flags.end()) {
            std::fprintf(stderr, "WARNING - unknown option %s ignored\n", a);
            continue;
        }
        Flag& f = it->second;
        if (f.seen) {   // params.cpp:114-185: an option may be given once
            std::string m = std::string("Option ") + a + " specified more than once";
            fatal(m.c_str());
        }
        f.seen = true;
        if (f.kind == Flag::kBool) {
            *static_cast<bool*>(f.dst) = true;
            continue;
        }
        if (i + 1 >= argc) {
            std::string m = std::string("Option ") + a + " needs a value";
            fatal(m.c_str());
        }
        const char* v = argv[++i];
        if (f.kind == Flag::kInt) *static_cast<int*>(f.dst) = std::atoi(v);
        else if (f.kind == Flag::kDouble) *static_cast<double*>(f.dst) = std::atof(v);
        else *static_cast<std::string*>(f.dst) = v;
    }
    if (ErrorTable != "Empty") {                                        // a plain run, every context under the file's table
        if (fitError) fatal("--ErrorTable cannot be combined with --FitError: a run either fits the error rates or is given them");
        if (cohortFitError) fatal("--ErrorTable cannot be combined with --CohortFitError: a run either fits the error rates or is given them");
        if (confidenceInterval) fatal("--ErrorTable cannot be combined with --ConfidenceInterval: the interval is computed under the nominal rates");
        if (cohortInterval) fatal("--ErrorTable cannot be combined with --CohortInterval: the intervals are computed under the nominal rates");
        if (findSource) fatal("--ErrorTable cannot be combined with --FindSource: the source scores are computed under the nominal rates");
        if (findRelated) fatal("--ErrorTable cannot be combined with --FindRelated: the relatedness is computed under the nominal rates");
        if (MatchedNormal != "Empty") fatal("--ErrorTable cannot be combined with --MatchedNormal: the paired refits are computed under the nominal rates");
        if (perReadGroup) fatal("--ErrorTable cannot be combined with --PerReadGroup: the groups are searched under the nominal rates");
        if (perChromosome) fatal("--ErrorTable cannot be combined with --PerChromosome: the replicates are searched under the nominal rates");
        if (flags["Bootstrap"].seen) fatal("--ErrorTable cannot be combined with --Bootstrap: the replicates are searched under the nominal rates");
        if (refBias) fatal("--ErrorTable cannot be combined with --RefBias: the bias is fitted under the nominal rates");
        if (PileupList == "Empty" && Devices != "Empty" && Devices.find(',') != std::string::npos)
            fatal("--ErrorTable cannot be combined with more than one --Devices for one sample: marker shards are built under the nominal rates");
    }
    double errTable[VB2_ERR_NUM_QUAL];                                  // (read before any other file of the run)
    int32_t errTableTaken = 0;
    if (ErrorTable != "Empty" && vb2_err_table_read(ErrorTable.c_str(), errTable, &errTableTaken) != VB2_OK) fatal(vb2_last_error());
    if (fitError) {                                                     // one sample, one device, a searched alpha, the plain search
        if (PileupList != "Empty")
            fatal("--FitError cannot be combined with --PileupList: the error rates are fitted for one sample per run");
        if (perReadGroup) fatal("--FitError cannot be combined with --PerReadGroup: run them separately");
        if (flags["FixAlpha"].seen)
            fatal("--FitError cannot be combined with --FixAlpha: a fixed alpha leaves the fit nothing to tell errors from");
        if (confidenceInterval) fatal("--FitError cannot be combined with --ConfidenceInterval: run them separately");
        if (perChromosome) fatal("--FitError cannot be combined with --PerChromosome: run them separately");
        if (flags["Bootstrap"].seen) fatal("--FitError cannot be combined with --Bootstrap: run them separately");
        if (refBias) fatal("--FitError cannot be combined with --RefBias: the two fits are not estimated jointly; run them separately");
        if (flags["NumStart"].seen) fatal("--FitError cannot be combined with --NumStart: every iteration's search is the reference's own");
        if (lineSearch) fatal("--FitError cannot be combined with --LineSearch: every iteration's search is the reference's own");
        if (Devices != "Empty" && Devices.find(',') != std::string::npos)
            fatal("--FitError cannot be combined with more than one --Devices: the fit reads one resident sample on one device");
        if (!(errorPrior > 0.0)) fatal("--ErrorPrior takes a positive number of pseudo-reads");
    } else if (cohortFitError) {                                        // a cohort on one device, the plain searches, no other stage
        if (PileupList == "Empty")
            fatal("--CohortFitError needs --PileupList: it fits the error rates of every sample of a cohort run (--FitError is the "
                  "flag for one sample)");
        if (flags["FixAlpha"].seen)
            fatal("--CohortFitError cannot be combined with --FixAlpha: a fixed alpha leaves the fit nothing to tell errors from");
        if (flags["NumStart"].seen) fatal("--CohortFitError cannot be combined with --NumStart: every iteration's search is the reference's own");
        if (lineSearch) fatal("--CohortFitError cannot be combined with --LineSearch: every iteration's search is the reference's own");
        if (Devices != "Empty" && Devices.find(',') != std::string::npos)
            fatal("--CohortFitError cannot be combined with more than one --Devices: the samples' raw inputs are fitted together on one device");
        if (findSource) fatal("--CohortFitError cannot be combined with --FindSource: run the source scores and the fits separately");
        if (findRelated) fatal("--CohortFitError cannot be combined with --FindRelated: run the relatedness and the fits separately");
        if (MatchedNormal != "Empty") fatal("--CohortFitError cannot be combined with --MatchedNormal: run the paired refits and the fits separately");
        if (cohortInterval) fatal("--CohortFitError cannot be combined with --CohortInterval: run the intervals and the fits separately");
        if (!(errorPrior > 0.0)) fatal("--ErrorPrior takes a positive number of pseudo-reads");
    } else if (pooledError) {
        fatal("--PooledError needs --CohortFitError");
    } else if (flags["ErrorPrior"].seen) {
        fatal("--ErrorPrior needs --FitError or --CohortFitError");
    }
    if (refBias) {                                                      // one sample, one device, a searched alpha
        if (PileupList != "Empty")
            fatal("--RefBias cannot be combined with --PileupList: the reference bias is estimated for one sample per run");
        if (perReadGroup) fatal("--RefBias cannot be combined with --PerReadGroup: run them separately");
        if (flags["FixAlpha"].seen)
            fatal("--RefBias cannot be combined with --FixAlpha: a fixed alpha leaves the refits nothing to estimate");
        if (confidenceInterval) fatal("--RefBias cannot be combined with --ConfidenceInterval: run them separately");
        if (perChromosome || flags["Bootstrap"].seen)
            fatal("--RefBias cannot be combined with --PerChromosome / --Bootstrap: run them separately");
        if (Devices != "Empty" && Devices.find(',') != std::string::npos)
            fatal("--RefBias cannot be combined with more than one --Devices: the refits read one resident sample on one device");
    }
    if (confidenceInterval) {                                           // single-sample, single-device runs only
        if (PileupList != "Empty")
            fatal("--ConfidenceInterval cannot be combined with --PileupList: intervals are computed for one sample per run "
                  "(--CohortInterval computes them for every sample of a --PileupList cohort)");
        if (Devices != "Empty" && Devices.find(',') != std::string::npos)
            fatal("--ConfidenceInterval cannot be combined with more than one --Devices: intervals are computed on one device");
    }
    if (cohortInterval) {                                               // a cohort on one device
        if (PileupList == "Empty")
            fatal("--CohortInterval needs --PileupList: it computes the interval of every sample of a cohort run "
                  "(--ConfidenceInterval is the flag for one sample)");
        if (Devices != "Empty" && Devices.find(',') != std::string::npos)
            fatal("--CohortInterval cannot be combined with more than one --Devices: the intervals of a cohort are computed on one device");
    }
    if (refitSource) {                                                  // a --FindSource cohort on one device
        if (!findSource)
            fatal("--RefitSource needs --FindSource: the refit is given the best candidate of the cohort's source scores");
        if (flags["FixAlpha"].seen)
            fatal("--RefitSource cannot be combined with --FixAlpha: a fixed alpha leaves the refit nothing to estimate");
        if (cohortInterval)
            fatal("--RefitSource cannot be combined with --CohortInterval: run the intervals and the refits separately");
        if (Devices != "Empty" && Devices.find(',') != std::string::npos)
            fatal("--RefitSource cannot be combined with more than one --Devices: the refits read a source set on one device");
    }
    if (findRelated) {                                                  // a cohort on one device
        if (PileupList == "Empty")
            fatal("--FindRelated needs --PileupList: duplicates and relatives are looked for among the samples of one cohort run");
        if (refitSource)
            fatal("--FindRelated cannot be combined with --RefitSource: run the refits and the relatedness separately");
        if (cohortInterval)
            fatal("--FindRelated cannot be combined with --CohortInterval: run the intervals and the relatedness separately");
        if (Devices != "Empty" && Devices.find(',') != std::string::npos)
            fatal("--FindRelated cannot be combined with more than one --Devices: a set of samples lives on one device");
        if (relatedTop < 1) fatal("--RelatedTop takes a positive number of partners");
    }
    if (MatchedNormal != "Empty") {                                     // a cohort on one device, a stage of its own
        if (PileupList == "Empty")
            fatal("--MatchedNormal needs --PileupList: tumours and normals are samples of one cohort run");
        if (flags["FixAlpha"].seen)
            fatal("--MatchedNormal cannot be combined with --FixAlpha: a fixed alpha leaves the refit nothing to estimate");
        if (cohortInterval)
            fatal("--MatchedNormal cannot be combined with --CohortInterval: run the intervals and the paired refits separately");
        if (refitSource)
            fatal("--MatchedNormal cannot be combined with --RefitSource: run the two refits separately");
        if (findSource)
            fatal("--MatchedNormal cannot be combined with --FindSource: run the source scores and the paired refits separately");
        if (findRelated)
            fatal("--MatchedNormal cannot be combined with --FindRelated: run the relatedness and the paired refits separately");
        if (Devices != "Empty" && Devices.find(',') != std::string::npos)
            fatal("--MatchedNormal cannot be combined with more than one --Devices: the normals' rows live on one device");
        if (!(normalHomMin >= 0.0 && normalHomMin <= 1.0)) fatal("--NormalHomMin takes a probability within [0, 1]");
    } else if (flags["NormalHomMin"].seen) {
        fatal("--NormalHomMin needs --MatchedNormal");
    } else if (pairInterval) {
        fatal("--PairInterval needs --MatchedNormal: it computes the interval of every tumour's FREEMIX given its matched normal");
    }
    if (findSource) {                                                   // a cohort on one device
        if (PileupList == "Empty")
            fatal("--FindSource needs --PileupList: the source of a contamination is looked for among the samples of one cohort run");
        if (Devices != "Empty" && Devices.find(',') != std::string::npos)
            fatal("--FindSource cannot be combined with more than one --Devices: a source set lives on one device");
        if (sourceTop < 1) fatal("--SourceTop takes a positive number of candidates");
    }
    if (perChromosome || flags["Bootstrap"].seen) {                     // single-sample, single-device runs only
        const char* which = perChromosome ? "--PerChromosome" : "--Bootstrap";
        if (PileupList != "Empty") {
            const std::string m = std::string(which) + " cannot be combined with --PileupList: replicates are refitted for one sample per run";
            fatal(m.c_str());
        }
        if (Devices != "Empty" && Devices.find(',') != std::string::npos) {
            const std::string m = std::string(which) + " cannot be combined with more than one --Devices: replicates read one resident sample on one device";
            fatal(m.c_str());
        }
        if (flags["Bootstrap"].seen && (bootstrap < 1 || bootstrap > 1000)) fatal("--Bootstrap takes 1 to 1000 replicates");
        if (confidenceInterval) fatal("--PerChromosome / --Bootstrap cannot be combined with --ConfidenceInterval: run them separately");
    }
    if (perReadGroup) {                                                 // one BAM, one device, the plain search
        if (PileupFile != "Empty" || PileupList != "Empty")
            fatal("--PerReadGroup cannot be combined with --PileupFile or --PileupList: a text pileup does not say which read group "
                  "a base came from");
        if (BamFile == "Empty") fatal("--PerReadGroup needs --BamFile: read groups are read from a BAM's header and RG:Z fields");
        if (Devices != "Empty" && Devices.find(',') != std::string::npos)
            fatal("--PerReadGroup cannot be combined with more than one --Devices: the groups are searched in lock-step on one device");
        if (confidenceInterval) fatal("--PerReadGroup cannot be combined with --ConfidenceInterval: run them separately");
        if (perChromosome || flags["Bootstrap"].seen)
            fatal("--PerReadGroup cannot be combined with --PerChromosome / --Bootstrap: run them separately");
        if (flags["NumStart"].seen || lineSearch)
            fatal("--PerReadGroup cannot be combined with --NumStart / --LineSearch: the groups are searched in lock-step by the "
                  "reference's optimiser");
    }
    // --Seed: parsed and never used by the reference (main.cpp:137,286); here it seeds --NumStart's starting points
    // --NumThread: the likelihood runs on the GPU; the VCF parser pool of --RefVCF and the reader threads of --PileupList use it

    if (RefVCF != "Empty") {                                            // main.cpp:233-257: SVD on the fly
        std::fprintf(stderr, "NOTICE - Specified --RefVCF reference panel VCF file, doing SVD on the fly...\n");
        std::fprintf(stderr, "NOTICE - This procedure will generate SVD matrices as [RefVCF path].UD and [RefVCF path].mu\n");
        std::fprintf(stderr, "NOTICE - You may specify --SVDPrefix [RefVCF path](or --UDPath [RefVCF path].UD and "
                             "--MeanPath [RefVCF path].mu) in future use\n");
        if (gramSVD)
            std::fprintf(stderr, "NOTICE - --GramSVD has no effect here: the one decomposition path is the exact Gram "
                                 "matrix on the GPU with an FP64 eigensolver\n");
        vb2_panel_args pa;
        std::memset(&pa, 0, sizeof(pa));
        pa.vcf_path = RefVCF.c_str();
        pa.include_chr = includeChrStr.c_str();
        pa.num_svd_pcs = numSVDPCs;
        pa.skip_min_sample_count_check = skipMinSampleCountCheck ? 1 : 0;
        pa.num_thread = nthread;
        pa.device = device;
        pa.notices = 1;
        vb2_panel* panel = nullptr;
        int rcp = vb2_panel_build(&pa, &panel);
        if (rcp == VB2_OK) rcp = vb2_panel_write(panel, RefVCF.c_str());
        vb2_panel_destroy(panel);
        if (rcp != VB2_OK) fatal(vb2_last_error());
        std::fprintf(stderr, "NOTICE - SVD output files written: %s.UD, %s.mu, %s.bed, %s.V\n", RefVCF.c_str(),
                     RefVCF.c_str(), RefVCF.c_str(), RefVCF.c_str());
        std::fprintf(stderr, "NOTICE - Success!\n");
        return 0;
    }

    // main.cpp:214-232
    if (SVDPrefix == "Empty") {
        if (UDPath == "Empty") fatal("--UDPath is required when --RefVCF is absent");
        if (MeanPath == "Empty") fatal("--MeanPath is required when --RefVCF is absent");
        if (BedPath == "Empty") fatal("--BedPath is required when --RefVCF is absent");
    } else {
        UDPath = SVDPrefix + ".UD";
        MeanPath = SVDPrefix + ".mu";
        BedPath = SVDPrefix + ".bed";
    }
    if (RefPath == "Empty") fatal("--Reference is required");          // main.cpp:263-266
    if (PileupFile == "Empty" && PileupList == "Empty" && BamFile == "Empty")
        fatal("--BamFile or --PileupFile is required");                // main.cpp:278-281

    vb2_run_args args;
    std::memset(&args, 0, sizeof(args));
    args.ud_path = UDPath.c_str();
    args.mean_path = MeanPath.c_str();
    args.bed_path = BedPath.c_str();
    args.pileup_path = PileupFile == "Empty" ? nullptr : PileupFile.c_str();
    args.bam_path = BamFile == "Empty" ? nullptr : BamFile.c_str();       // the built-in reader (bam_flatten.cpp)
    args.reference_path = RefPath.c_str();
    args.known_af_path = knownAF == "Empty" ? nullptr : knownAF.c_str();
    args.output_prefix = outputPrefix.c_str();
    args.num_pc = nPC;
    args.disable_sanity = disableSanityCheck;
    args.output_pileup = outputPileup;
    args.search.num_start = numStart;
    args.search.seed = (uint32_t)seed;
    args.search.line_search = lineSearch ? 1 : 0;
    args.device = device;
    std::vector<int32_t> devs;
    if (Devices != "Empty") {
        std::stringstream ds(Devices);
        std::string tok;
        while (std::getline(ds, tok, ',')) {
            if (tok.empty() || tok.find_first_not_of("0123456789") != std::string::npos)
                fatal("--Devices takes a comma-separated list of device ordinals, e.g. 0,1,2,3");
            devs.push_back(std::atoi(tok.c_str()));
        }
        if (devs.empty() || devs.size() > 64) fatal("--Devices names no device (or more than 64)");
        args.devices = devs.data();
        args.num_device = (int32_t)devs.size();
        args.device = devs[0];
    }
    // the lines of --PileupList: a name that ends in ".bam" is read by the built-in BAM reader, any other as a text pileup
    std::vector<std::string> pile, pref;
    bool listHasBam = false;
    if (PileupList != "Empty") {
        std::ifstream fl(PileupList);
        if (!fl.is_open()) fatal("cannot open --PileupList file");
        std::string line;
        while (std::getline(fl, line)) {
            if (line.empty()) continue;
            const size_t tab = line.find('\t');
            pile.push_back(line.substr(0, tab));
            pref.push_back(tab == std::string::npos ? line + ".vb2" : line.substr(tab + 1));
            const std::string& name = pile.back();
            if (name.size() > 4 && name.compare(name.size() - 4, 4, ".bam") == 0) listHasBam = true;
        }
        if (pile.empty()) fatal("--PileupList file names no sample");
    }
    static const char* const kPileupOpts[] = {"min-BQ", "min-MQ", "adjust-MQ", "max-depth", "no-orphans", "incl-flags", "excl-flags"};
    for (const char* name : kPileupOpts) args.mpileup.given |= flags[name].seen ? 1 : 0;
    args.mpileup.min_bq = minBQ;
    args.mpileup.min_mq = minMQ;
    args.mpileup.adjust_mq = adjustMQ;
    args.mpileup.max_depth = maxDepth;
    args.mpileup.no_orphans = noOrphans ? 1 : 0;
    args.mpileup.incl_flags = inclFlags;
    args.mpileup.excl_flags = exclFlags;
    if (args.mpileup.given && BamFile == "Empty" && !listHasBam)
        std::fprintf(stderr, "NOTICE - pileup options (--min-BQ, --min-MQ, ...) apply to --BamFile input only; "
                             "the text pileup is taken as it is (as in the reference)\n");
    // (once per run, also for the .bam lines of a --PileupList, however many there are)
    if (applyBAQ && !((BamFile != "Empty" && PileupFile == "Empty") || listHasBam))
        fatal("--ApplyBAQ needs --BamFile, or a --PileupList with a .bam line: a text pileup carries no alignments to realign");
    args.bam_adjust = applyBAQ ? 1 : 0;
    if (applyBAQ) {
        const int effFlags = args.mpileup.given ? inclFlags : (16 | 1024), effCap = args.mpileup.given ? adjustMQ : 40;
        std::string what;
        if (effFlags & 128) what += "the Illumina-1.3 quality shift";
        if (effFlags & 16) what += std::string(what.empty() ? "" : ", ") + "base alignment quality" + ((effFlags & 64) ? " (recomputed: BQ tags ignored)" : "");
        if (effCap > 10) what += std::string(what.empty() ? "" : ", ") + "the mapping quality cap (--adjust-MQ " + std::to_string(effCap) + ")";
        if (what.empty()) what = "nothing (the pileup options ask for neither BAQ nor the cap; the FASTA is not opened)";
        std::fprintf(stderr, "NOTICE - --ApplyBAQ: applied to BAM input from %s: %s; the reference base of a site stays the panel's "
                             "REF allele (.bed)\n", RefPath.c_str(), what.c_str());
        if (nthread > 4 && !listHasBam) vb2_debug_set_tunable("bam_threads", nthread);
    } else if ((BamFile != "Empty" && PileupFile == "Empty") || listHasBam) {
        // what the built-in reader leaves out of the reference's pileup without --ApplyBAQ
        const int effFlags = args.mpileup.given ? inclFlags : (16 | 1024), effCap = args.mpileup.given ? adjustMQ : 40;
        if (effFlags & 16)
            std::fprintf(stderr, "NOTICE - --BamFile: base alignment quality (BAQ, --incl-flags bit 16) is not applied by the built-in "
                                 "BAM reader; the reference computes the same with --incl-flags 1024 --adjust-MQ 0\n");
        if (effCap > 10)
            std::fprintf(stderr, "NOTICE - --BamFile: the mapping quality cap (--adjust-MQ %d) is not applied by the built-in BAM "
                                 "reader; the reference computes the same with --incl-flags 1024 --adjust-MQ 0\n", effCap);
        std::fprintf(stderr, "NOTICE - --BamFile: the reference base of a site is the panel's REF allele (.bed); --Reference is not read\n");
        // --NumThread above its default: the reader's pool (of a cohort it stays the number of reader threads, and a BAM
        // line's pool is 16 / that)
        if (nthread > 4 && !listHasBam) vb2_debug_set_tunable("bam_threads", nthread);
    }
    args.model.is_heter = !withinAncestry;
    args.model.epsilon = epsilon;
    args.model.verbose = verbose;
    args.model.notices = 1;

    std::vector<double> tmpPC;
    if (fixPC != "Empty") {                                            // main.cpp:291-308
        std::fprintf(stderr, "NOTICE - you specified --fixPC, this will overide dynamic estimation of PCs\n");
        std::stringstream ss(fixPC);
        std::string token;
        while (std::getline(ss, token, ':')) tmpPC.push_back(std::atof(token.c_str()));
        if ((int)tmpPC.size() > nPC)
            std::fprintf(stderr, "WARNING - parameter --fixPC provided larger dimension than parameter "
                                 "--numPC(default value 2) and hence will be truncated\n");
        if ((int)tmpPC.size() < nPC)
            fatal("parameter --fixPC provided smaller dimension than parameter --numPC(default value 2)");
        args.model.is_pc_fixed = 1;
        args.model.fix_pc = tmpPC.data();
    } else if (std::fabs(fixAlpha + 1.) > std::numeric_limits<double>::epsilon()) {   // main.cpp:309-313
        std::fprintf(stderr, "NOTICE - you specified --fixAlpha, this will overide dynamic estimation of alpha\n");
        args.model.is_alpha_fixed = 1;
        args.model.fix_alpha = fixAlpha;
    }
    if (args.known_af_path) args.model.is_af_known = 1;               // main.cpp:314-319

    if (ErrorTable != "Empty")
        std::fprintf(stderr, "NOTICE - --ErrorTable: the error rates of %d qualities taken from %s, the others nominal\n",
                     (int)errTableTaken, ErrorTable.c_str());
    if (PileupList != "Empty") {
        std::vector<const char*> cpile, cpref;
        for (size_t i = 0; i < pile.size(); ++i) { cpile.push_back(pile[i].c_str()); cpref.push_back(pref[i].c_str()); }
        vb2_cohort_args ca;
        std::memset(&ca, 0, sizeof(ca));
        ca.base = args;
        ca.num_sample = (int32_t)pile.size();
        ca.pileup_paths = cpile.data();
        ca.output_prefixes = cpref.data();
        ca.num_host_thread = nthread > 4 ? nthread : 0;               // --NumThread above its default: reader threads
        std::vector<vb2_run_result> cres(pile.size());
        std::vector<int32_t> cst(pile.size());
        std::vector<int32_t> tumour(pile.size()), normal(pile.size());
        int32_t numPair = 0;
        if (MatchedNormal != "Empty" &&         // (before the panel is read and any device is touched)
            vb2_matched_normal_read(MatchedNormal.c_str(), ca.num_sample, cpile.data(), &numPair, tumour.data(), normal.data()) != VB2_OK)
            fatal(vb2_last_error());
        vb2_errfit_opts cohortFitOpts;
        std::memset(&cohortFitOpts, 0, sizeof(cohortFitOpts));
        cohortFitOpts.prior_reads = errorPrior;
        const int rcc = ErrorTable != "Empty" ? vb2_cohort_run_under_table(&ca, errTable, cres.data(), cst.data())
                        : cohortFitError ? vb2_cohort_run_errfit(&ca, &cohortFitOpts, pooledError ? 1 : 0, cres.data(), cst.data(), nullptr, nullptr)
                        : numPair > 0 && pairInterval
                            ? vb2_cohort_run_paired_intervals(&ca, numPair, tumour.data(), normal.data(), normalHomMin, cres.data(),
                                                              cst.data(), nullptr, nullptr)
                        : numPair > 0 ? vb2_cohort_run_paired(&ca, numPair, tumour.data(), normal.data(), normalHomMin, cres.data(), cst.data(), nullptr)
                        : findRelated ? vb2_cohort_run_related(&ca, relatedTop, findSource ? sourceTop : 0, cres.data(), cst.data(), nullptr, nullptr)
                        : cohortInterval ? vb2_cohort_run_intervals(&ca, findSource ? sourceTop : 0, cres.data(), cst.data(), nullptr)
                        : refitSource ? vb2_cohort_run_source_fits(&ca, sourceTop, cres.data(), cst.data(), nullptr, nullptr, nullptr)
                        : findSource ? vb2_cohort_run_sources(&ca, sourceTop, cres.data(), cst.data(), nullptr, nullptr)
                                     : vb2_cohort_run(&ca, cres.data(), cst.data());
        if (rcc != VB2_OK) {
            std::fprintf(stderr, "\nFATAL ERROR - \n%s\n\n", vb2_last_error());
            return EXIT_FAILURE;
        }
        int bad = 0;
        for (size_t i = 0; i < pile.size(); ++i)
            if (cst[i] == VB2_OK) print_sample_summary(args.model, args.num_pc, cres[i].est);
        std::printf("#PILEUP\tOUTPUT\tSTATUS\tFREEMIX\tFREELK1\tFREELK0\tAVG_DP\n");
        for (size_t i = 0; i < pile.size(); ++i) {
            const double al = cres[i].est.alpha;
            std::printf("%s\t%s\t%d\t%g\t%g\t%g\t%g\n", pile[i].c_str(), pref[i].c_str(), (int)cst[i],
                        al < 0.5 ? al : 1 - al, cres[i].est.llk1, cres[i].est.llk0, cres[i].avg_depth);
            if (cst[i] != VB2_OK) ++bad;
        }
        std::fprintf(stderr, "NOTICE - cohort of %zu samples done, %d failed their own checks\n", pile.size(), bad);
        return bad ? EXIT_FAILURE : 0;
    }

    vb2_run_result res;
    vb2_interval ci;
    int32_t numGroup = 0;
    vb2_errfit_opts fitOpts;
    std::memset(&fitOpts, 0, sizeof(fitOpts));
    fitOpts.prior_reads = errorPrior;
    const int rc = ErrorTable != "Empty"            ? vb2_run_under_table(&args, errTable, &res)
                   : fitError                       ? vb2_run_errfit(&args, &fitOpts, &res, nullptr)
                   : refBias                        ? vb2_run_refbias(&args, &res, nullptr)
                   : perReadGroup                   ? vb2_run_read_groups(&args, &res, 0, nullptr, &numGroup)
                   : (perChromosome || bootstrap > 0) ? vb2_run_replicates(&args, perChromosome ? 1 : 0, bootstrap, &res, nullptr)
                   : confidenceInterval             ? vb2_run_interval(&args, &res, &ci)
                                                    : vb2_run(&args, &res);
    if (rc != VB2_OK) {
        if (rc == VB2_ERR_SANITY) std::fprintf(stderr, "WARNING - %s\n", vb2_last_error());
        else std::fprintf(stderr, "\nFATAL ERROR - \n%s\n\n", vb2_last_error());
        return EXIT_FAILURE;
    }
    std::fprintf(stderr, "NOTICE - %lld likelihood evaluations, %lld points launched on the device\n",
                 (long long)res.est.num_eval, (long long)res.est.num_launch_point);
    if (perReadGroup) std::fprintf(stderr, "NOTICE - %d read groups written to %s.selfRG\n", (int)numGroup, outputPrefix.c_str());
    std::fprintf(stderr, "NOTICE - Success!\n");
    return 0;
}
