// cohort.cpp -- vb2_cohort_run: many samples against one panel (BASELINE.json configs[4]).
//
// The reference runs one process per sample (main.cpp:56-414).  Here the panel is read once, a
// pool of host threads reads + flattens + uploads pileups, and every DEVICE of the run has its
// own pipeline thread that searches the samples in lock-step (one kernel launch per Nelder-Mead
// step for all the samples on the device).  Round 4: the device keeps `group_size` slots and a
// sample that has converged hands its slot to the next one that is ready (stream_search.h) --
// before, a device took the next ready GROUP of samples and searched it to its last sample
// (vb2_batch_*; still there as VB2_COHORT_STREAM=0).  Samples are independent, so several devices
// need no collective: sample s runs on devices[s % n] (--Devices a,b,...; groups: group g on
// devices[g % n]), which is the sample-parallel sharding of SURVEY.md 8e(2) inside one process.
// vb2_cohort_run_intervals (--CohortInterval; one device): every searched sample's confidence interval as well, computed in
// lock-step (interval.h) -- on the group's batch after its search, or, streaming, on an interval stage with a thread and a
// stream of its own that takes the samples the search is done with.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <deque>
#include <limits>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "batch.h"
#include "conditioned.h"
#include "context.h"
#include "estimator.h"
#include "guard.h"
#include "hostio.h"
#include "interval.h"
#include "paired.h"
#include "source.h"
#include "stream_search.h"
#include "tunables.h"

using vb2::set_error;

namespace {

double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct Slot {
    std::unique_ptr<vb2_flat> flat;
    vb2_ctx* ctx = nullptr;
    int rc = VB2_OK;
    bool ready = false;
};

class CohortRunner {
public:
    // find_source: every searched sample also goes into a source set (vb2_cohort_run_sources) -- on the releaser thread,
    // before its context is destroyed; score / shared ([S][S], may be null) and <Output>.Sources after the last sample
    // intervals: every searched sample's vb2_interval as well (vb2_cohort_run_intervals; one device) -- <prefix>.CI, and
    // ci[s] when ci is not null -- before the sample goes to the releaser
    // refit (with find_source; vb2_cohort_run_source_fits): the contexts of the samples that got a row in the source set are
    // parked instead of destroyed, and after the score matrix every sample's FREEMIX is refitted given its best candidate
    // (conditioned.h) -- <Output>.SourceFit, and fit[s] when fit is not null
    CohortRunner(const vb2_cohort_args* a, vb2_run_result* out, int32_t* status, bool find_source = false, int top = 0,
                 double* score = nullptr, int32_t* shared = nullptr, bool intervals = false, vb2_interval* ci = nullptr,
                 bool refit = false, vb2_source_fit* fit = nullptr)
        : a_(a), out_(out), status_(status), S_(a->num_sample), find_source_(find_source), top_(top), score_(score),
          shared_(shared), intervals_(intervals), ci_(ci), refit_(refit && find_source), fit_(fit)
    {
        if (a->base.devices && a->base.num_device > 0) devices_.assign(a->base.devices, a->base.devices + a->base.num_device);
        else devices_.push_back(a->base.device);
        ndev_ = (int)devices_.size();
        // (round 4: 32, not 64 -- with the finished samples regrouped (Batch::optimize) a group of 32 costs 1.55 ms per C3
        // sample and one of 64 1.5, and the smaller group starts earlier and leaves a shorter tail nothing overlaps:
        // 256 files 479 -> 546 samples/s)
        G_ = std::max(1, std::min(a->group_size != 0 ? std::abs(a->group_size) : 32, 64));
        const int hw = vb2::usable_cpu_count();
        // readers: reading + resolving + creating the context is ~7 ms of one CPU per C3-sized sample (the flatten runs on the
        // device), the device needs ~1.65 ms per sample -> a device keeps 4-5 readers busy.  The default is SIX per device,
        // within the process's allowance (cgroup quota / affinity, not the host's core count) less one CPU per pipeline
        // thread and one for the rest: the thread of a lock-step search spins on its device's flag between steps, and when it
        // has to queue for a CPU -- or the whole cgroup is throttled because fifteen readers woke up at once -- the device
        // idles (16 CPUs, 256 files: 15 readers 562-587 samples/s with runs at 390; 5 to 10 readers 600-633)
        // (round 6: the device needs 1.2 ms per sample, the host 9 ms of one CPU -> EIGHT per device: 4 / 6 / 8 / 10 / 12
        // readers 500 / 705 / 740 / 750 / 750 samples/s on 16 CPUs)
        const int dflt = std::max(2, std::min(hw - 1 - ndev_, 8 * ndev_));
        T_ = std::max(1, std::min({a->num_host_thread > 0 ? a->num_host_thread : dflt, std::max(hw, 1) * 4, S_}));
        slots_.resize(S_);
        cnt_.assign(ndev_, 0);
        stream_ = vb2::tunables().cohort_stream != 0;
        inflight_.assign(ndev_, 0);
        remaining_.assign(ndev_, 0);
        for (int s = 0; s < S_; ++s) ++remaining_[s % ndev_];
        ready_q_.resize(ndev_);
        // Group boundaries, a function of (S, G, devices) only -- never of timing, so a run is
        // reproducible.  A device's first groups are small (16, then 32 samples): it starts searching
        // after a fraction of the reading a full group needs; the later ones have the full size (a
        // bigger group costs less per sample: 3.6 / 3.25 / 3.0 ms at 16 / 32 / 48 C3-sized samples).
        // A remainder of up to half a group joins the last group instead of running alone.
        for (int begin = 0, gi = 0; begin < S_; ++gi) {
            const int nth = gi / ndev_;                       // this group's index on its device
            int want = std::min(G_, nth == 0 ? 16 : nth == 1 ? 32 : G_);     // (G_ > 32: 16, 32, then full groups)
            if (a->group_size < 0) want = G_;                 // (negative group_size: plain equal groups of |group_size|)
            const int left = S_ - begin;
            if (left <= want + want / 2) want = left;
            group_begin_.push_back(begin);
            for (int s = begin; s < begin + want; ++s) group_of_.push_back(gi);
            begin += want;
        }
        group_begin_.push_back(S_);
        ngroup_ = (int)group_begin_.size() - 1;
    }

    // related (vb2_cohort_run_related): the set also keeps the related planes -- one marginal launch per sample all the same --,
    // llr ([S][S][4]) / shared ([S][S]; may be null) and <Output>.Related after the last sample
    void enable_related(int top, double* llr, int32_t* shared)
    {
        related_ = true;
        related_top_ = top;
        llr_ = llr;
        rel_shared_ = shared;
    }

    // paired (vb2_cohort_run_paired; --MatchedNormal): the listed normals get a q row in a source set, the listed tumours'
    // contexts are parked instead of destroyed, and after the last sample every pair is refitted (paired.h) --
    // <Output>.PairFit, and fits[p] when fits is not null.  interval (vb2_cohort_run_paired_intervals; --PairInterval): and
    // then ONE vb2_paired_interval over the refitted pairs, before the contexts go -- <Output>.PairCI, and ci[p]
    void enable_paired(int num_pair, const int32_t* tumour, const int32_t* normal, double hom_min, vb2_pair_fit* fits,
                       bool interval = false, vb2_interval* ci = nullptr)
    {
        paired_ = true;
        pair_interval_ = interval;
        pair_ci_ = ci;
        pair_t_.assign(tumour, tumour + num_pair);
        pair_n_.assign(normal, normal + num_pair);
        hom_min_ = hom_min;
        pair_fit_ = fits;
        is_tumour_.assign((size_t)S_, 0);
        is_normal_.assign((size_t)S_, 0);
        for (int p = 0; p < num_pair; ++p) {
            is_tumour_[(size_t)tumour[p]] = 1;
            is_normal_[(size_t)normal[p]] = 1;
        }
    }

    ~CohortRunner()
    {
        shutdown();
        release_parked();
        drop_streams();
    }

    int run()
    {
        for (int s = 0; s < S_; ++s) {
            std::memset(&out_[s], 0, sizeof(out_[s]));
            status_[s] = VB2_ERR_INVALID;
            if (ci_) std::memset(&ci_[s], 0, sizeof(ci_[s]));
        }
        const bool timing = vb2::tunables().debug_timing != 0;
        const double t_run0 = now_s();
        // HIP runtime start-up (per device) behind the panel reading
        std::vector<std::thread> warm;
        for (int d : devices_)
            warm.emplace_back([d] {
                if (d >= 0) (void)hipSetDevice(d);
                (void)hipFree(nullptr);
                (void)hipGetLastError();
            });
        panel_ = std::make_shared<vb2::Panel>();
        panel_->numPC = a_->base.num_pc;
        int rc = VB2_OK;
        try {
            rc = vb2::load_panel(&a_->base, panel_.get());
        } catch (...) {
            for (auto& t : warm) t.join();
            throw;
        }
        const double t_panel = now_s();
        for (auto& t : warm) t.join();
        if (rc) return rc;
        const double t_warm = now_s();
        model_ = a_->base.model;
        if (panel_->isAFknown) model_.is_af_known = 1;
        if (find_source_ || related_ || paired_) {
            vb2::SourceSet* set = nullptr;
            const int planes = (find_source_ || paired_ ? VB2_SET_SOURCE : 0) | (related_ ? VB2_SET_RELATED : 0);
            if (const int rcs = vb2::SourceSet::create((int)panel_->NumMarker, S_, devices_[0], &set, planes)) {
                err_all_ = vb2::g_last_error;
                return rcs;
            }
            sources_.reset(set);
        }
        vb2::g_flatten_thread_cap.store(std::max(1, 16 / T_));

        // HIP maps a process's streams onto FOUR hardware queues per device, each in order.  A context's creation (uploads, the
        // flatten's kernels, and a barrier that waits for the 10-MB upload) on a stream that shares its hardware queue with a lane
        // of the search holds that lane's next step back for as long -- a few hundred microseconds, for half of the samples when
        // every context and every lane takes whatever stream the cache has (kernel trace of tools/cohort_from_text.py: steps
        // on two queues, the flatten's kernels on all four).  So: per device four streams made back to back, after the idle cached
        // ones are gone (the runtime gives a new stream the least used queue: four queues), two for the lanes and two that every
        // context of this run is created on.
        if (stream_ && vb2::tunables().cohort_own_queues) {
            own_streams_.assign((size_t)ndev_ * 4, nullptr);
            for (int d = 0; d < ndev_; ++d) {
                int dev = devices_[d];
                if (dev < 0) (void)hipGetDevice(&dev);
                if (hipSetDevice(dev) != hipSuccess) { (void)hipGetLastError(); continue; }
                vb2::drop_cached_streams(dev);
                for (int q = 0; q < 4; ++q)
                    if (hipStreamCreateWithFlags(&own_streams_[(size_t)d * 4 + q], hipStreamNonBlocking) != hipSuccess) {
                        (void)hipGetLastError();
                        own_streams_[(size_t)d * 4 + q] = nullptr;
                    }
            }
        }
        releaser_ = std::thread([this] { release_loop(); });
        for (int t = 0; t < T_; ++t) pool_.emplace_back([this] { reader_loop(); });
        for (int d = 0; d < ndev_; ++d) dev_threads_.emplace_back([this, d] { if (stream_) stream_loop(d); else device_loop(d); });
        for (auto& t : dev_threads_) t.join();
        dev_threads_.clear();
        const double t_dev = now_s();
        shutdown();
        if (sources_ && find_source_ && !rc_all_) rc_all_ = finish_sources();
        if (sources_ && related_ && !rc_all_) rc_all_ = finish_related();
        if (refit_ || paired_) {
            if (refit_ && !rc_all_) rc_all_ = refit_sources();
            if (paired_ && !rc_all_) rc_all_ = refit_pairs();
            release_parked();
            drop_streams();
        }
        if (timing)
            std::fprintf(stderr, "vb2_cohort_run: panel %.1f ms, HIP start-up beyond that %.1f ms, pipelines %.1f ms, "
                                 "shutdown (release contexts, join) %.1f ms; releaser: %.2f ms per context, %.2f ms per sample's host arrays\n",
                         1e3 * (t_panel - t_run0), 1e3 * (t_warm - t_panel), 1e3 * (t_dev - t_warm), 1e3 * (now_s() - t_dev),
                         1e3 * rel_s_[0] / S_, 1e3 * rel_s_[1] / S_);
        if (timing)
            std::fprintf(stderr, "vb2_cohort_run: %d reader threads, per sample: read_pileup %.1f ms, sanity + resolve %.1f ms, "
                                 "vb2_ctx_create %.1f ms (wall-clock inside the reader threads)\n", T_,
                         1e3 * phase_s_[0] / S_, 1e3 * phase_s_[1] / S_, 1e3 * phase_s_[2] / S_);
        return rc_all_;
    }

private:
    const vb2_cohort_args* a_;
    vb2_run_result* out_;
    int32_t* status_;
    int S_, G_ = 64, T_ = 1, ndev_ = 1, ngroup_ = 0;
    std::vector<int> group_begin_, group_of_;       // [group] first sample (+ S_ at the end); [sample] group
    std::vector<int> devices_;
    std::shared_ptr<vb2::Panel> panel_;
    vb2_model model_{};
    std::vector<Slot> slots_;
    std::mutex mu_;
    std::condition_variable cv_;
    int next_ = 0;
    std::vector<int> cnt_;                 // groups completed per device
    bool stop_ = false;
    int rc_all_ = VB2_OK;
    std::string err_all_;
    std::vector<hipStream_t> own_streams_;      // [device][4]: two lanes' streams, two creation streams (or empty)
    std::vector<std::thread> pool_, dev_threads_;
    std::thread releaser_;
    std::mutex rel_mu_;
    std::condition_variable rel_cv_;
    std::deque<std::pair<vb2_ctx*, std::unique_ptr<vb2_flat>>> rel_queue_;
    bool rel_stop_ = false;
    bool down_ = false;

    double rel_s_[2] = {0, 0};             // releaser thread: vb2_ctx_destroy, freeing the host arrays
    double phase_s_[3] = {0, 0, 0};        // reader threads' wall-clock: read_pileup, sanity + resolve, vb2_ctx_create

    // streaming (stream_search.h): sample s belongs to device s % ndev_
    bool stream_ = true;
    std::vector<int> inflight_;            // [device] samples handed to a reader and not yet done
    std::vector<int> remaining_;           // [device] samples not yet delivered to the search (or failed before it)
    std::vector<std::deque<int>> ready_q_; // [device] prepared samples, in the order they became ready
    struct Done { int s; vb2_ctx* ctx; std::unique_ptr<vb2_flat> flat; bool write; vb2_estimate est; bool add = false; };
    // --FindSource (null without it: nothing below then differs from a plain run)
    bool find_source_ = false;
    int top_ = 0;
    double* score_ = nullptr;
    int32_t* shared_ = nullptr;
    std::unique_ptr<vb2::SourceSet> sources_;
    // --CohortInterval (false without it: nothing below then differs from a plain run).  Streaming: a searched sample waits
    // in iv_queue_ for a fiber of the interval stage (interval_loop), which has a thread and a stream of its own.
    bool intervals_ = false;
    vb2_interval* ci_ = nullptr;
    struct IvItem { int s = -1; vb2_estimate est{}; };
    std::mutex iv_mu_;
    std::condition_variable iv_cv_;
    std::deque<IvItem> iv_queue_;
    bool iv_closed_ = false;

    // --RefitSource (false without it: nothing else then differs from a --FindSource run)
    bool refit_ = false;
    vb2_source_fit* fit_ = nullptr;
    std::vector<vb2_ctx*> parked_;         // [sample] the context of a sample with a row in the source set (releaser thread)
    int64_t parked_bytes_ = 0;
    std::vector<double> sc_;               // the matrix, where the caller gave no room for it
    std::vector<int32_t> sh_;
    const double* fit_score_ = nullptr;
    const int32_t* fit_shared_ = nullptr;

    // after the last context is gone: the matrix, and <Output>.Sources next to the samples' own files
    int finish_sources()
    {
        sources_->set_count(S_);
        const size_t nn = (size_t)S_ * (size_t)S_;
        std::vector<double>& sc = sc_;
        std::vector<int32_t>& sh = sh_;
        const bool file = a_->output_prefixes && a_->base.output_prefix;
        double* score = score_;
        int32_t* shared = shared_;
        if ((file || refit_) && !score) { sc.resize(nn); score = sc.data(); }
        if ((file || refit_) && !shared) { sh.resize(nn); shared = sh.data(); }
        fit_score_ = score;
        fit_shared_ = shared;
        if (!score && !shared) return VB2_OK;
        int rc = sources_->scores(score, shared);
        if (!rc && file) rc = vb2::write_sources(a_->base.output_prefix, S_, top_, a_->output_prefixes, out_, status_, score, shared);
        if (rc) err_all_ = vb2::g_last_error;
        return rc;
    }
    // --FindRelated (false without it: nothing else then differs)
    bool related_ = false;
    int related_top_ = 0;
    double* llr_ = nullptr;
    int32_t* rel_shared_ = nullptr;

    // after the last context is gone: K, and <Output>.Related next to the samples' own files
    int finish_related()
    {
        sources_->set_count(S_);
        for (int s = 0; s < S_; ++s)
            if (status_[s] != VB2_OK)
                std::fprintf(stderr, "NOTICE - --FindRelated: sample %d failed (status %d) and is left out of the relatedness matrix\n",
                             s, (int)status_[s]);
        const size_t nn = (size_t)S_ * (size_t)S_;
        std::vector<double> kk;
        std::vector<int32_t> sh;
        const bool file = a_->output_prefixes && a_->base.output_prefix;
        double* llr = llr_;
        int32_t* shared = rel_shared_;
        if (file && !llr) { kk.resize(nn * VB2_NUM_RELATION); llr = kk.data(); }
        if (file && !shared) { sh.resize(nn); shared = sh.data(); }
        if (!llr && !shared) return VB2_OK;
        int rc = sources_->relations(llr, shared);
        if (!rc && file) rc = vb2::write_related(a_->base.output_prefix, S_, related_top_, a_->output_prefixes, status_, llr, shared);
        if (rc) err_all_ = vb2::g_last_error;
        return rc;
    }
    std::deque<Done> done_queue_;          // (rel_mu_) searched samples: outputs to write, context and arrays to free

    int device_of_group(int gi) const { return gi % ndev_; }
    int device_of_sample(int s) const { return stream_ ? s % ndev_ : device_of_group(group_of_[s]); }

    // every way out (normal end, error, exception in run()) stops and joins all threads and
    // gives back the contexts that were never handed to a device pipeline
    void shutdown()
    {
        if (down_) return;
        down_ = true;
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : dev_threads_)
            if (t.joinable()) t.join();
        for (auto& t : pool_)
            if (t.joinable()) t.join();
        {
            std::lock_guard<std::mutex> lk(rel_mu_);
            rel_stop_ = true;
        }
        rel_cv_.notify_all();
        if (releaser_.joinable()) releaser_.join();
        for (auto& sl : slots_)
            if (sl.ctx) {
                vb2_ctx_destroy(sl.ctx);
                sl.ctx = nullptr;
            }
        vb2::g_flatten_thread_cap.store(0);
        if (!refit_ && !paired_) drop_streams();         // (--RefitSource, --MatchedNormal: the parked contexts still run on them)
    }

    void drop_streams()
    {
        for (hipStream_t& st : own_streams_)             // (every context and batch that used them is gone)
            if (st) {
                (void)hipStreamSynchronize(st);
                (void)hipStreamDestroy(st);
                st = nullptr;
            }
    }

    void release_parked()
    {
        for (vb2_ctx*& c : parked_)
            if (c) {
                vb2_ctx_destroy(c);
                c = nullptr;
            }
    }

    // The tail both refits share: the one-row sets on the parked contexts, ALL in one lock-step call of `optimize` between
    // the phase's notices.  fit[who[n]].status becomes set n's (the call's own failure is everybody's), a failure gives
    // "NOTICE - <failed> <who[n] + first>" with the last error, and the sets go before their contexts do.  The estimates, by set.
    // keep: the sets stay (the caller has more to do on them, and clears them itself).
    template <class Set, class Optimize, class Fit>
    std::vector<vb2_estimate> refit_sets(const char* phase, const char* failed, int first, Optimize optimize,
                                         std::vector<std::unique_ptr<Set>>& sets, const std::vector<double>& fixed,
                                         const std::vector<int>& who, std::vector<Fit>& fit, bool keep = false)
    {
        std::vector<vb2_estimate> est(sets.size());
        if (sets.empty()) return est;
        std::vector<Set*> raw;
        for (auto& p : sets) raw.push_back(p.get());
        std::vector<int32_t> st(sets.size(), VB2_ERR_INVALID);
        const double t0 = now_s();
        if (model_.notices) std::fprintf(stderr, "NOTICE - Starting phase: %s (%d searches in lock-step)\n", phase, (int)sets.size());
        const int rc = optimize(raw.data(), (int)raw.size(), model_, fixed.data(), est.data(), st.data());
        if (model_.notices) std::fprintf(stderr, "NOTICE - Finished phase: %s  [%.3f seconds]\n", phase, now_s() - t0);
        for (size_t n = 0; n < who.size(); ++n) {
            Fit& f = fit[(size_t)who[n]];
            f.status = rc ? rc : st[n];
            if (f.status != VB2_OK)
                std::fprintf(stderr, "NOTICE - %s %d failed: %s\n", failed, who[n] + first, vb2::g_last_error.c_str());
        }
        if (!keep) sets.clear();
        return est;
    }

    // --RefitSource, after the matrix: one refit per sample -- its best candidate, where that candidate's score is finite
    // and > 0 --, each a one-hypothesis set on the sample's parked context, ALL in one lock-step call; fit[] and
    // <Output>.SourceFit.  A refit that fails leaves its row NA, gives a NOTICE and does not fail the run.
    int refit_sources()
    {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        std::vector<vb2_source_fit> fit((size_t)S_);
        std::vector<std::unique_ptr<vb2::Conditioned>> sets;
        std::vector<int> who;
        std::vector<double> fixed;
        if (parked_bytes_ > 0)
            std::fprintf(stderr, "NOTICE - --RefitSource: the contexts of %d samples stayed on the device for the refit (%lld bytes)\n",
                         (int)std::count_if(parked_.begin(), parked_.end(), [](vb2_ctx* c) { return c != nullptr; }),
                         (long long)parked_bytes_);
        for (int i = 0; i < S_; ++i) {
            vb2_source_fit& f = fit[(size_t)i];
            std::memset(&f, 0, sizeof(f));
            f.candidate = -1;
            f.status = VB2_SOURCE_FIT_NONE;
            f.llr = f.freemix = f.freelk1 = f.alpha_given = f.lk1_given = f.lk0_given = f.delta_lk = nan;
            if (status_[i] != VB2_OK || !fit_score_ || top_ < 1) continue;
            const vb2_estimate& e = out_[i].est;
            f.freemix = e.alpha < 0.5 ? e.alpha : 1 - e.alpha;
            f.freelk1 = e.llk1;
            // the first row of the sample in .Sources: the first of the largest scores (write_sources: a stable sort)
            int best = -1;
            for (int j = 0; j < S_; ++j) {
                const double v = fit_score_[(size_t)i * S_ + j];
                if (j == i || std::isnan(v)) continue;
                if (best < 0 || v > fit_score_[(size_t)i * S_ + best]) best = j;
            }
            if (best < 0) continue;
            f.candidate = best;
            f.llr = fit_score_[(size_t)i * S_ + best];
            f.markers = fit_shared_ ? fit_shared_[(size_t)i * S_ + best] : 0;
            if (!(std::isfinite(f.llr) && f.llr > 0) || (size_t)i >= parked_.size() || !parked_[(size_t)i]) continue;
            // the target's search point, as the source set took it: its pc1 is what the refit holds
            vb2::Context* c = parked_[(size_t)i]->impl;
            std::vector<double> p1, p2;
            vb2::search_point(*c, model_, e, &p1, &p2, nullptr);
            vb2::Conditioned* set = nullptr;
            const int32_t cand = best;
            if (const int rc = vb2::Conditioned::create_from_set(c, sources_.get(), 1, &cand, &set)) {
                f.status = rc;
                std::fprintf(stderr, "NOTICE - --RefitSource: sample %d is not refitted: %s\n", i, vb2::g_last_error.c_str());
                continue;
            }
            sets.emplace_back(set);
            who.push_back(i);
            fixed.insert(fixed.end(), p1.begin(), p1.end());
        }
        const std::vector<vb2_estimate> est =
            refit_sets("Refit given the source", "--RefitSource: the refit of sample", 0, vb2::conditioned_optimize, sets, fixed, who, fit);
        for (size_t n = 0; n < who.size(); ++n) {
            vb2_source_fit& f = fit[(size_t)who[n]];
            if (f.status != VB2_OK) continue;
            f.alpha_given = est[n].alpha;
            f.lk1_given = est[n].llk1;
            f.lk0_given = est[n].llk0;
            f.delta_lk = (-f.lk1_given) - (-f.freelk1);
        }
        if (fit_) std::memcpy(fit_, fit.data(), sizeof(vb2_source_fit) * (size_t)S_);
        if (a_->output_prefixes && a_->base.output_prefix) {
            const int rc = vb2::write_source_fit(a_->base.output_prefix, S_, a_->output_prefixes, fit.data());
            if (rc) {
                err_all_ = vb2::g_last_error;
                return rc;
            }
        }
        return VB2_OK;
    }

    // --MatchedNormal (false without it: nothing else then differs from a plain run)
    bool paired_ = false;
    std::vector<int32_t> pair_t_, pair_n_;     // [pair] sample indices
    std::vector<char> is_tumour_, is_normal_;  // [sample]
    double hom_min_ = 0.99;
    vb2_pair_fit* pair_fit_ = nullptr;
    bool pair_interval_ = false;               // --PairInterval
    vb2_interval* pair_ci_ = nullptr;

    // --MatchedNormal, after the last sample: one refit per pair whose tumour and normal were both searched -- a
    // one-hypothesis set on the tumour's parked context, built on the device from the normal's q row --, ALL in one lock-step
    // call; fits[] and <Output>.PairFit.  A refit that fails leaves NA, gives a NOTICE and does not fail the run.
    int refit_pairs()
    {
        const int P = (int)pair_t_.size();
        const double nan = std::numeric_limits<double>::quiet_NaN();
        std::vector<vb2_pair_fit> fit((size_t)P);
        std::vector<std::unique_ptr<vb2::Paired>> sets;
        std::vector<int> who;
        std::vector<double> fixed;
        if (parked_bytes_ > 0)
            std::fprintf(stderr, "NOTICE - --MatchedNormal: the contexts of %d tumours stayed on the device for the refit (%lld bytes)\n",
                         (int)std::count_if(parked_.begin(), parked_.end(), [](vb2_ctx* c) { return c != nullptr; }),
                         (long long)parked_bytes_);
        auto folded = [](double a) { return a < 0.5 ? a : 1 - a; };
        for (int p = 0; p < P; ++p) {
            const int t = pair_t_[(size_t)p], n = pair_n_[(size_t)p];
            vb2_pair_fit& f = fit[(size_t)p];
            std::memset(&f, 0, sizeof(f));
            f.tumour = t;
            f.normal = n;
            f.status = VB2_PAIR_FIT_NONE;
            f.normal_freemix = f.freemix = f.freelk1 = f.alpha_paired = f.lk1_paired = f.lk0_paired = nan;
            if (status_[t] != VB2_OK || status_[n] != VB2_OK) {
                std::fprintf(stderr, "NOTICE - --MatchedNormal: pair %d is not refitted: its %s failed (status %d)\n", p + 1,
                             status_[t] != VB2_OK ? "tumour" : "normal", (int)(status_[t] != VB2_OK ? status_[t] : status_[n]));
                continue;
            }
            const vb2_estimate& e = out_[n].est;
            f.normal_freemix = folded(e.alpha);
            f.freemix = folded(out_[t].est.alpha);
            f.freelk1 = out_[t].est.llk1;
            f.status = VB2_ERR_INVALID;
            if ((size_t)t >= parked_.size() || !parked_[(size_t)t]) {
                std::fprintf(stderr, "NOTICE - --MatchedNormal: pair %d is not refitted: the tumour's context is gone\n", p + 1);
                continue;
            }
            // the normal's search point, as the source set took it: its pc2 -- the intended sample's -- is what the refit holds
            vb2::Context* c = parked_[(size_t)t]->impl;
            std::vector<double> p1, p2;
            vb2::search_point(*c, model_, e, &p1, &p2, nullptr);
            vb2::Paired* set = nullptr;
            const int32_t nrm = n;
            if (const int rc = vb2::Paired::create_from_set(c, sources_.get(), 1, &nrm, hom_min_, &set)) {
                f.status = rc;
                std::fprintf(stderr, "NOTICE - --MatchedNormal: pair %d is not refitted: %s\n", p + 1, vb2::g_last_error.c_str());
                continue;
            }
            f.markers = (int32_t)set->given[0];
            sets.emplace_back(set);
            who.push_back(p);
            fixed.insert(fixed.end(), p2.begin(), p2.end());
        }
        const std::vector<vb2_estimate> est = refit_sets("Refit given the matched normal", "--MatchedNormal: the refit of pair", 1,
                                                         vb2::paired_optimize, sets, fixed, who, fit, pair_interval_);
        for (size_t i = 0; i < who.size(); ++i) {
            vb2_pair_fit& f = fit[(size_t)who[i]];
            if (f.status != VB2_OK) continue;
            f.alpha_paired = est[i].alpha;
            f.lk1_paired = est[i].llk1;
            f.lk0_paired = est[i].llk0;
        }
        // --PairInterval: the intervals of the refitted pairs, ALL in one lock-step gang on the parked contexts
        std::vector<vb2_interval> ci((size_t)P);
        std::vector<int32_t> ci_status((size_t)P, VB2_PAIR_FIT_NONE);
        if (P > 0) std::memset(ci.data(), 0, sizeof(vb2_interval) * (size_t)P);
        if (pair_interval_) {
            std::vector<vb2::Paired*> raw;
            std::vector<int> pair_of;
            std::vector<double> fixed_l;
            std::vector<vb2_estimate> est_l;
            const int k = a_->base.num_pc;
            for (size_t i = 0; i < who.size(); ++i) {
                if (fit[(size_t)who[i]].status != VB2_OK) continue;
                raw.push_back(sets[i].get());
                pair_of.push_back(who[i]);
                fixed_l.insert(fixed_l.end(), fixed.begin() + (long)i * k, fixed.begin() + (long)(i + 1) * k);
                est_l.push_back(est[i]);
            }
            if (!raw.empty()) {
                std::vector<vb2_interval> ci_l(raw.size());
                std::vector<int32_t> st_l(raw.size(), VB2_ERR_INVALID);
                int64_t steps = 0;
                const double t0 = now_s();
                if (model_.notices)
                    std::fprintf(stderr, "NOTICE - Starting phase: Intervals given the matched normal (%d intervals in lock-step)\n",
                                 (int)raw.size());
                const int rc = vb2::paired_interval(raw.data(), (int)raw.size(), model_, fixed_l.data(), est_l.data(), ci_l.data(),
                                                    st_l.data(), &steps);
                if (model_.notices)
                    std::fprintf(stderr, "NOTICE - Finished phase: Intervals given the matched normal (%lld launch pairs)  [%.3f seconds]\n",
                                 (long long)steps, now_s() - t0);
                for (size_t i = 0; i < raw.size(); ++i) {
                    const int p = pair_of[i];
                    ci_status[(size_t)p] = rc ? rc : st_l[i];
                    if (ci_status[(size_t)p] == VB2_OK) ci[(size_t)p] = ci_l[i];
                    else std::fprintf(stderr, "NOTICE - --PairInterval: the interval of pair %d failed: %s\n", p + 1, vb2::g_last_error.c_str());
                }
            }
            sets.clear();                              // (before their contexts go)
            if (pair_ci_) std::memcpy(pair_ci_, ci.data(), sizeof(vb2_interval) * (size_t)P);
        }
        if (pair_fit_) std::memcpy(pair_fit_, fit.data(), sizeof(vb2_pair_fit) * (size_t)P);
        if (a_->output_prefixes && a_->base.output_prefix) {
            int rc = vb2::write_pair_fit(a_->base.output_prefix, P, a_->pileup_paths, fit.data());
            if (!rc && pair_interval_)
                rc = vb2::write_pair_ci(a_->base.output_prefix, P, a_->pileup_paths, fit.data(), ci.data(), ci_status.data());
            if (rc) {
                err_all_ = vb2::g_last_error;
                return rc;
            }
        }
        return VB2_OK;
    }

    void prepare(int s)
    {
        Slot& sl = slots_[s];
        const double t0 = now_s();
        sl.flat.reset(new vb2_flat(panel_));
        vb2_flat& f = *sl.flat;
        sl.rc = vb2::read_pileup(a_->pileup_paths[s], *panel_, &f.viewer);
        if (sl.rc) return;
        const double t_read = now_s();
        const bool sanity_off = a_->base.disable_sanity != 0;
        f.sanity_disabled = sanity_off;
        const bool sane = sanity_off || vb2::sanity_check(*panel_, &f.viewer);
        f.resolve();
        vb2_flat_stats(&f, &out_[s]);
        const double t_res = now_s();
        const char* prefix = a_->output_prefixes ? a_->output_prefixes[s] : nullptr;
        if (a_->base.output_pileup && prefix) (void)vb2::write_pileup(prefix, f);
        if (!sane) {
            sl.rc = VB2_ERR_SANITY;
            return;
        }
        vb2_options opt{};
        opt.device = devices_[device_of_sample(s)];
        opt.flags = VB2_OPT_COHORT_LAYOUT;       // the lock-step search streams the 16-bit run lists
        if (!own_streams_.empty())               // (one of the device's two creation streams: see run())
            opt.stream = own_streams_[(size_t)device_of_sample(s) * 4 + 2 + (size_t)(s / ndev_) % 2];
        sl.rc = vb2_ctx_create(&f.input, &opt, &sl.ctx);
        if (sl.rc == VB2_OK && sl.ctx && sl.ctx->impl) {
            // the static schedules of the sample's group (and of the batches its lane is regrouped into): here, on one of many
            // reader threads, not on the one thread that feeds the device (a failure only means they are built there)
            const int gi = group_of_[s];
            if (stream_) (void)vb2::prepare_for_stream(sl.ctx->impl, G_);
            else (void)vb2::Batch::prepare_for_cohort(sl.ctx->impl, group_begin_[gi + 1] - group_begin_[gi]);
        }
        // the context holds its own (flattened) copy: the sample's text-sized arrays go back now, on
        // this reader thread, instead of piling up in front of the single releaser (the writers need
        // only the viewer's counters and the panel)
        std::string().swap(f.bases);
        std::string().swap(f.quals);
        std::string().swap(f.viewer.basePool);
        std::string().swap(f.viewer.qualPool);
        std::vector<int64_t>().swap(f.read_off);
        f.input = vb2_input{};
        const double t_end = now_s();
        out_[s].seconds_load = t_end - t0;
        {
            std::lock_guard<std::mutex> lk(mu_);
            phase_s_[0] += t_read - t0;
            phase_s_[1] += t_res - t_read;
            phase_s_[2] += t_end - t_res;
        }
    }

    void reader_loop()
    {
        for (;;) {
            int s;
            {
                std::unique_lock<std::mutex> lk(mu_);
                // stay at most two groups ahead of the group's device (bounds host and device memory)
                cv_.wait(lk, [&] {
                    if (stop_ || next_ >= S_) return true;
                    if (stream_) return inflight_[next_ % ndev_] < 2 * G_ + T_;       // (two slot sets ahead of the device)
                    const int gi = group_of_[next_];
                    return gi / ndev_ < cnt_[device_of_group(gi)] + 2;
                });
                if (stop_ || next_ >= S_) return;
                s = next_++;
                if (stream_) ++inflight_[s % ndev_];
            }
            try {
                prepare(s);
            } catch (const std::bad_alloc&) {
                slots_[s].rc = VB2_ERR_NOMEM;
            } catch (const std::exception&) {
                slots_[s].rc = VB2_ERR_INVALID;
            }
            if (stream_ && !(slots_[s].rc == VB2_OK && slots_[s].ctx)) {
                // never reaches the search: reported here (the pipeline thread may be waiting for this device's last sample)
                status_[s] = slots_[s].rc ? slots_[s].rc : VB2_ERR_INVALID;
                finish_sample(s, false, nullptr, /*delivered=*/false);
                continue;
            }
            {
                std::lock_guard<std::mutex> lk(mu_);
                slots_[s].ready = true;
                if (stream_) ready_q_[s % ndev_].push_back(s);
            }
            cv_.notify_all();
        }
    }

    // sample s leaves the pipeline: outputs (write) + context + host arrays go to the releaser thread, its place in the
    // readers' window is free again.  delivered: the search took the sample (DeviceSource::next counted it out of
    // remaining_ then) -- whether or not the search then succeeded; a sample that fails on a reader thread never
    // gets that far and is counted out here.
    void finish_sample(int s, bool write, const vb2_estimate* est, bool delivered)
    {
        {
            std::lock_guard<std::mutex> lk(rel_mu_);
            Done d{s, slots_[s].ctx, std::move(slots_[s].flat), write, vb2_estimate{}};
            if (est) d.est = *est;
            d.add = write && est;
            slots_[s].ctx = nullptr;
            done_queue_.push_back(std::move(d));
        }
        rel_cv_.notify_one();
        {
            std::lock_guard<std::mutex> lk(mu_);
            const int d = s % ndev_;
            --inflight_[d];
            if (!delivered) --remaining_[d];
        }
        cv_.notify_all();
    }

    // the pipeline thread's view of its device's samples (stream_search.h)
    struct DeviceSource : vb2::StreamSource {
        CohortRunner* r;
        int d;
        DeviceSource(CohortRunner* runner, int dev) : r(runner), d(dev) {}
        int next(bool block, vb2::Context** ctx) override
        {
            std::unique_lock<std::mutex> lk(r->mu_);
            for (;;) {
                if (r->stop_) return kEnd;
                if (!r->ready_q_[d].empty()) {
                    const int s = r->ready_q_[d].front();
                    r->ready_q_[d].pop_front();
                    --r->remaining_[d];
                    *ctx = r->slots_[s].ctx->impl;
                    return s;
                }
                if (r->remaining_[d] <= 0) return kEnd;
                if (!block) return kNone;
                r->cv_.wait(lk);
            }
        }
        const vb2_model& model(int) override { return r->model_; }
        void done(int s, int rc, const vb2_estimate& est, double seconds) override
        {
            r->status_[s] = rc;
            if (!rc) {
                r->out_[s].est = est;
                r->out_[s].seconds_optimize = seconds;
            }
            if (r->intervals_ && rc == VB2_OK) {             // its interval first: the stage finishes the sample
                {
                    std::lock_guard<std::mutex> lk(r->iv_mu_);
                    IvItem it;
                    it.s = s;
                    it.est = est;
                    r->iv_queue_.push_back(it);
                }
                r->iv_cv_.notify_one();
                return;
            }
            r->finish_sample(s, rc == VB2_OK, &est, /*delivered=*/true);
        }
    };

    // 1: *it is the next searched sample; 0: none right now (only when block is false); -1: none will come any more
    int take_searched(bool block, IvItem* it)
    {
        std::unique_lock<std::mutex> lk(iv_mu_);
        for (;;) {
            if (!iv_queue_.empty()) {
                *it = iv_queue_.front();
                iv_queue_.pop_front();
                return 1;
            }
            if (iv_closed_) return -1;
            if (!block) return 0;
            iv_cv_.wait(lk);
        }
    }

    // sample s's interval is over (rc != 0: it has none): <prefix>.CI, the caller's array, then the sample leaves as it does
    // without intervals -- its other files are the search's
    void complete_interval(int s, int rc, const vb2_estimate& est, const vb2_interval& ci)
    {
        const char* prefix = a_->output_prefixes ? a_->output_prefixes[s] : nullptr;
        if (!rc && prefix) rc = vb2::write_ci(prefix, ci);
        if (!rc && ci_) ci_[s] = ci;
        if (rc) status_[s] = rc;
        finish_sample(s, true, &est, /*delivered=*/true);
    }

    // The interval stage of a streaming run: as many fibers as the search has slots, each running one sample's interval
    // (interval.h).  At a step boundary an idle fiber takes the next searched sample; a step -- one Batch::derivs call for
    // every live fiber's point -- goes out as soon as all live fibers have parked, however few they are.  The search of later
    // samples goes on meanwhile on its own thread and streams.
    void interval_loop(int d)
    {
        int dev = devices_[d];
        if (dev < 0) (void)hipGetDevice(&dev);
        int fail = hipSetDevice(dev) == hipSuccess ? VB2_OK : VB2_ERR_HIP;
        if (fail) set_error("--CohortInterval: hipSetDevice failed");
        int num_cu = 256;
        {
            hipDeviceProp_t prop;
            if (!fail && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) num_cu = prop.multiProcessorCount;
        }
        const int k = a_->base.num_pc;
        std::unique_ptr<vb2::Batch> batch;
        if (!fail) {
            vb2::Batch* bp = nullptr;
            fail = vb2::Batch::create_slots(G_, dev, k, num_cu, &bp);
            batch.reset(bp);
        }
        auto device_failure = [&](int rc) {          // concerns every sample: the run stops, what is queued leaves with rc
            fail = rc;
            std::lock_guard<std::mutex> lk(mu_);
            if (!rc_all_) {
                rc_all_ = rc;
                err_all_ = vb2::g_last_error;
            }
            stop_ = true;
        };
        if (fail) device_failure(fail);
        vb2::IntervalGang gang(G_, k);
        std::vector<IvItem> cur(G_);
        std::vector<vb2_interval> civ(G_);
        std::vector<char> live(G_, 0);
        int nlive = 0;
        const vb2::BatchDerivsFn fn = [&](int32_t, const int32_t* np, const double* p1, const double* p2, const double* al,
                                          double* llk, double* grad, double* hess) {
            return batch->derivs(np, p1, p2, al, llk, grad, hess);
        };
        auto retire = [&](int i) {
            live[i] = 0;
            --nlive;
            if (batch) (void)batch->set_slot(i, nullptr);
            complete_interval(cur[i].s, fail ? fail : gang.result(i), cur[i].est, civ[i]);
        };
        for (;;) {
            bool end = false;
            for (int i = 0; i < G_; ++i) {
                if (live[i]) continue;
                IvItem it;
                const int got = take_searched(nlive == 0, &it);
                if (got < 0) end = true;
                if (got <= 0) break;
                cur[i] = it;
                vb2::Context* c = slots_[it.s].ctx->impl;
                int rcs = fail;
                if (!rcs) rcs = batch->set_slot(i, c);
                // (the sample's scratch and the batch's staging here, on this thread's own stack: the fibers only park)
                if (!rcs) rcs = batch->ensure_deriv_resources();
                if (rcs) {
                    if (batch) (void)batch->set_slot(i, nullptr);
                    complete_interval(it.s, rcs, it.est, civ[i]);
                    continue;
                }
                vb2::IntervalGang::Task t;
                t.model = &model_;
                t.est = &cur[i].est;
                t.out = &civ[i];
                t.data_has_known_af = c->L.known_af != nullptr;
                t.label = a_->output_prefixes ? a_->output_prefixes[it.s] : nullptr;
                live[i] = 1;
                ++nlive;
                (void)gang.spawn(i, t);
                if (gang.idle(i)) retire(i);
            }
            if (nlive == 0) {
                if (end) break;
                continue;
            }
            if (const int rc = gang.step(fn))
                if (!fail) device_failure(rc);
            for (int i = 0; i < G_; ++i)
                if (live[i] && gang.idle(i)) retire(i);
        }
        cv_.notify_all();
    }

    void stream_loop(int d)
    {
        const bool timing = vb2::tunables().debug_timing != 0;
        const double t0 = now_s();
        DeviceSource src(this, d);
        int rc = VB2_OK;
        int num_cu = 256;
        {
            hipDeviceProp_t prop;
            const int dev = devices_[d];
            int cur = dev;
            if (dev < 0) (void)hipGetDevice(&cur);
            if (hipGetDeviceProperties(&prop, cur) == hipSuccess && prop.multiProcessorCount > 0) num_cu = prop.multiProcessorCount;
        }
        std::thread iv;
        if (intervals_) iv = std::thread([this, d] { interval_loop(d); });
        struct IvJoin {                              // the stage ends when the search has handed over its last sample
            CohortRunner* r;
            std::thread* t;
            ~IvJoin()
            {
                if (!t->joinable()) return;
                {
                    std::lock_guard<std::mutex> lk(r->iv_mu_);
                    r->iv_closed_ = true;
                }
                r->iv_cv_.notify_all();
                t->join();
            }
        };
        try {
            IvJoin join{this, &iv};
            int dev = devices_[d];
            if (dev < 0) (void)hipGetDevice(&dev);
            rc = vb2::stream_search(dev, a_->base.num_pc, num_cu, G_, src, own_streams_.empty() ? nullptr : &own_streams_[(size_t)d * 4]);
        } catch (const std::exception& e) {
            set_error(e.what());
            rc = VB2_ERR_INVALID;
        }
        if (timing)
            std::fprintf(stderr, "vb2_cohort_run: device %d: %d slots, stream over after %.1f ms\n", devices_[d], G_, 1e3 * (now_s() - t0));
        if (rc) {                                // device-level failure: concerns every sample
            std::lock_guard<std::mutex> lk(mu_);
            if (!rc_all_) {
                rc_all_ = rc;
                err_all_ = vb2::g_last_error;
            }
            stop_ = true;
        }
        cv_.notify_all();
    }

    void release_loop()
    {
        for (;;) {
            std::pair<vb2_ctx*, std::unique_ptr<vb2_flat>> item;
            {
                std::unique_lock<std::mutex> lk(rel_mu_);
                rel_cv_.wait(lk, [&] { return rel_stop_ || !rel_queue_.empty() || !done_queue_.empty(); });
                if (!done_queue_.empty()) {
                    Done d = std::move(done_queue_.front());
                    done_queue_.pop_front();
                    lk.unlock();
                    // a searched sample: its output files first (they need the flattened sample's counters)
                    const char* prefix = a_->output_prefixes ? a_->output_prefixes[d.s] : nullptr;
                    if (d.write && prefix && d.flat) {
                        int rw = vb2::write_ancestry(prefix, a_->base.num_pc, d.est.pc, d.est.pc2);
                        if (!rw) rw = vb2::write_selfsm(prefix, *d.flat, d.est, true);   // (cohort input is text pileups: #READS = NA)
                        if (rw) status_[d.s] = rw;
                    }
                    if (paired_) {
                        // a searched normal gets its row; a searched tumour stays for the refit; the rest go as ever
                        if (d.add && d.ctx && d.ctx->impl && status_[d.s] == VB2_OK) {
                            if (is_normal_[(size_t)d.s] && sources_->put(d.s, d.ctx->impl, model_, d.est))
                                std::fprintf(stderr, "NOTICE - --MatchedNormal: sample %d has no row in the source set: %s\n", d.s,
                                             vb2::g_last_error.c_str());
                            if (is_tumour_[(size_t)d.s]) {
                                if (parked_.empty()) parked_.assign((size_t)S_, nullptr);
                                parked_[(size_t)d.s] = d.ctx;
                                parked_bytes_ += d.ctx->impl->device_bytes;
                                d.ctx = nullptr;
                            }
                        }
                    } else if (sources_ && d.add && d.ctx && d.ctx->impl && status_[d.s] == VB2_OK) {
                        // (a sample whose row cannot be made keeps its files and its status -- it was searched and written as
                        // the plain run does it --; its row and column of the matrix are NaN and a NOTICE says why)
                        if (sources_->put(d.s, d.ctx->impl, model_, d.est))
                            std::fprintf(stderr, "NOTICE - %s: sample %d has no row in the source set: %s\n",
                                         find_source_ ? "--FindSource" : "--FindRelated", d.s, vb2::g_last_error.c_str());
                        else if (refit_) {               // searched, written, in the set: parked for the refit, not destroyed
                            if (parked_.empty()) parked_.assign((size_t)S_, nullptr);
                            parked_[(size_t)d.s] = d.ctx;
                            parked_bytes_ += d.ctx->impl->device_bytes;
                            d.ctx = nullptr;
                        }
                    }
                    item.first = d.ctx;
                    item.second = std::move(d.flat);
                } else {
                    if (rel_queue_.empty()) return;
                    item = std::move(rel_queue_.front());
                    rel_queue_.pop_front();
                }
            }
            const double t0 = now_s();
            if (item.first) vb2_ctx_destroy(item.first);
            const double t1 = now_s();
            item.second.reset();
            rel_s_[0] += t1 - t0;
            rel_s_[1] += now_s() - t1;
        }
    }

    void device_loop(int d)
    {
        const bool timing = vb2::tunables().debug_timing != 0;
        for (int gi = d; gi < ngroup_; gi += ndev_) {
            const int g0 = group_begin_[gi], g1 = group_begin_[gi + 1];
            const double tg0 = now_s();
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] {
                    if (stop_) return true;
                    for (int s = g0; s < g1; ++s)
                        if (!slots_[s].ready) return false;
                    return true;
                });
                if (stop_) return;
            }
            const double tg_wait = now_s();
            std::vector<vb2_ctx*> ctxs;
            std::vector<int> who;
            for (int s = g0; s < g1; ++s) {
                status_[s] = slots_[s].rc;
                if (slots_[s].rc == VB2_OK && slots_[s].ctx) {
                    ctxs.push_back(slots_[s].ctx);
                    who.push_back(s);
                }
            }
            int rcb = VB2_OK;
            if (!ctxs.empty()) {
                const double t1 = now_s();
                std::vector<vb2_estimate> est(ctxs.size());
                std::vector<vb2_interval> civ;
                std::vector<int32_t> ist;
                vb2_batch* batch = nullptr;
                try {
                    rcb = vb2_batch_create(ctxs.data(), (int32_t)ctxs.size(), &batch);
                    if (!rcb) rcb = vb2_batch_optimize_llk(batch, &model_, 1, est.data());
                    if (!rcb && intervals_) {        // on the same batch, before it goes
                        civ.resize(ctxs.size());
                        ist.assign(ctxs.size(), VB2_ERR_INVALID);
                        std::vector<const char*> labels;
                        for (const int s : who) labels.push_back(a_->output_prefixes ? a_->output_prefixes[s] : nullptr);
                        rcb = vb2::batch_interval(batch->impl, &model_, 1, est.data(), civ.data(), ist.data(), nullptr, labels.data());
                    }
                } catch (const std::exception& e) {
                    set_error(e.what());
                    rcb = VB2_ERR_INVALID;
                }
                if (batch) vb2_batch_destroy(batch);
                const double dt = (now_s() - t1) / (double)ctxs.size();
                if (rcb)                    // the group's search failed: its samples must not keep "ok" with a zeroed estimate
                    for (const int s : who) status_[s] = rcb;
                if (!rcb) {
                    for (size_t i = 0; i < who.size(); ++i) {
                        const int s = who[i];
                        out_[s].est = est[i];
                        out_[s].seconds_optimize = dt;
                        const char* prefix = a_->output_prefixes ? a_->output_prefixes[s] : nullptr;
                        if (prefix) {
                            int rw = vb2::write_ancestry(prefix, a_->base.num_pc, est[i].pc, est[i].pc2);
                            if (!rw) rw = vb2::write_selfsm(prefix, *slots_[s].flat, est[i], true);   // (cohort input is text pileups: #READS = NA)
                            if (rw) status_[s] = rw;
                        }
                        if (intervals_) {
                            int ri = ist[i];
                            if (!ri && prefix) ri = vb2::write_ci(prefix, civ[i]);
                            if (!ri && ci_) ci_[s] = civ[i];
                            if (ri) status_[s] = ri;
                        }
                    }
                }
            }
            const double tg_opt = now_s();
            {   // freeing device and pinned memory synchronises with the device and takes milliseconds
                // per context: hand the group to the releaser thread and move on
                std::lock_guard<std::mutex> lk(rel_mu_);
                for (int s = g0; s < g1; ++s) {
                    if (sources_) {              // (the releaser adds the sample to the source set first; its files are written)
                        Done d{s, slots_[s].ctx, std::move(slots_[s].flat), false, out_[s].est};
                        d.add = !rcb && status_[s] == VB2_OK && slots_[s].ctx != nullptr;
                        done_queue_.push_back(std::move(d));
                    } else {
                        rel_queue_.emplace_back(slots_[s].ctx, std::move(slots_[s].flat));
                    }
                    slots_[s].ctx = nullptr;
                }
            }
            rel_cv_.notify_one();
            if (timing)
                std::fprintf(stderr, "vb2_cohort_run: device %d group %d (samples %d-%d): waited %.1f ms for the "
                                     "readers, search + outputs %.1f ms\n", devices_[d], gi, g0, g1 - 1,
                             1e3 * (tg_wait - tg0), 1e3 * (tg_opt - tg_wait));
            {
                std::lock_guard<std::mutex> lk(mu_);
                ++cnt_[d];
                if (rcb) {                       // device-level failure: concerns every sample
                    if (!rc_all_) {
                        rc_all_ = rcb;
                        err_all_ = vb2::g_last_error;
                    }
                    stop_ = true;
                }
            }
            cv_.notify_all();
            if (rcb) return;
        }
    }

public:
    const std::string& error() const { return err_all_; }
    int num_reader() const { return T_; }
};

}  // namespace

extern "C" int vb2_cohort_run(const vb2_cohort_args* a, vb2_run_result* out, int32_t* status)
{
    if (!a || !out || !status || a->num_sample < 1 || !a->pileup_paths || !a->base.ud_path ||
        !a->base.mean_path || !a->base.bed_path || a->base.num_pc < 1 || a->base.num_pc > VB2_MAX_PC ||
        a->base.num_device < 0 || a->base.num_device > 64) {
        set_error("vb2_cohort_run: invalid argument");
        return VB2_ERR_INVALID;
    }
    // (Tunables::cohort_dup_devices: a test switch -- the pipelines of a several-device run, their group
    // schedule and the readers' per-device look-ahead exercised on a machine with one GPU)
    const bool dup_ok = vb2::tunables().cohort_dup_devices != 0;
    for (int i = 0; i < a->base.num_device && !dup_ok; ++i)
        for (int j = 0; j < i; ++j)
            if (a->base.devices && a->base.devices[i] == a->base.devices[j]) {
                // (two lock-step pipelines on one device would each launch device-filling grids)
                set_error("vb2_cohort_run: a device is listed twice");
                return VB2_ERR_INVALID;
            }
    return vb2::guarded([&] {
        CohortRunner runner(a, out, status);
        const int rc = runner.run();
        if (rc && !runner.error().empty()) set_error(runner.error());
        return rc;
    });
}

extern "C" int vb2_cohort_run_sources(const vb2_cohort_args* a, int32_t top, vb2_run_result* out, int32_t* status, double* score,
                                      int32_t* shared)
{
    if (!a || !out || !status || a->num_sample < 1 || !a->pileup_paths || !a->base.ud_path || !a->base.mean_path ||
        !a->base.bed_path || a->base.num_pc < 1 || a->base.num_pc > VB2_MAX_PC || top < 0) {
        set_error("vb2_cohort_run_sources: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (a->base.num_device > 1 || a->base.num_device < 0) {
        set_error("--FindSource takes one device: a source set is not spread over several --Devices");
        return VB2_ERR_INVALID;
    }
    return vb2::guarded([&] {
        CohortRunner runner(a, out, status, true, top, score, shared);
        const int rc = runner.run();
        if (rc && !runner.error().empty()) set_error(runner.error());
        return rc;
    });
}

extern "C" int vb2_cohort_run_related(const vb2_cohort_args* a, int32_t related_top, int32_t source_top, vb2_run_result* out,
                                      int32_t* status, double* llr, int32_t* shared)
{
    if (!a || !out || !status || a->num_sample < 1 || !a->pileup_paths || !a->base.ud_path || !a->base.mean_path ||
        !a->base.bed_path || a->base.num_pc < 1 || a->base.num_pc > VB2_MAX_PC || related_top < 0 || source_top < 0) {
        set_error("vb2_cohort_run_related: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (a->base.num_device > 1 || a->base.num_device < 0) {
        set_error("--FindRelated takes one device: a set of samples is not spread over several --Devices");
        return VB2_ERR_INVALID;
    }
    return vb2::guarded([&] {
        CohortRunner runner(a, out, status, source_top > 0, source_top);
        runner.enable_related(related_top, llr, shared);
        const int rc = runner.run();
        if (rc && !runner.error().empty()) set_error(runner.error());
        return rc;
    });
}

extern "C" int vb2_cohort_run_source_fits(const vb2_cohort_args* a, int32_t top, vb2_run_result* out, int32_t* status, double* score,
                                          int32_t* shared, vb2_source_fit* fit)
{
    if (!a || !out || !status || a->num_sample < 1 || !a->pileup_paths || !a->base.ud_path || !a->base.mean_path ||
        !a->base.bed_path || a->base.num_pc < 1 || a->base.num_pc > VB2_MAX_PC || top < 0) {
        set_error("vb2_cohort_run_source_fits: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (a->base.num_device > 1 || a->base.num_device < 0) {
        set_error("--RefitSource takes one device: a source set and the refits given it are not spread over several --Devices");
        return VB2_ERR_INVALID;
    }
    if (a->base.model.is_alpha_fixed) {
        set_error("--RefitSource cannot be combined with --FixAlpha: a fixed alpha leaves the refit nothing to estimate");
        return VB2_ERR_INVALID;
    }
    return vb2::guarded([&] {
        CohortRunner runner(a, out, status, true, top, score, shared, false, nullptr, true, fit);
        const int rc = runner.run();
        if (rc && !runner.error().empty()) set_error(runner.error());
        return rc;
    });
}

extern "C" int vb2_cohort_run_intervals(const vb2_cohort_args* a, int32_t source_top, vb2_run_result* out, int32_t* status,
                                        vb2_interval* ci)
{
    if (!a || !out || !status || a->num_sample < 1 || !a->pileup_paths || !a->base.ud_path || !a->base.mean_path ||
        !a->base.bed_path || a->base.num_pc < 1 || a->base.num_pc > VB2_MAX_PC || source_top < 0) {
        set_error("vb2_cohort_run_intervals: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (a->base.num_device > 1 || a->base.num_device < 0) {
        set_error("--CohortInterval takes one device: the intervals of a cohort are not spread over several --Devices");
        return VB2_ERR_INVALID;
    }
    return vb2::guarded([&] {
        CohortRunner runner(a, out, status, source_top > 0, source_top, nullptr, nullptr, true, ci);
        const int rc = runner.run();
        if (rc && !runner.error().empty()) set_error(runner.error());
        return rc;
    });
}

namespace {
int cohort_run_paired(const vb2_cohort_args* a, int32_t num_pair, const int32_t* tumour, const int32_t* normal, double hom_min,
                      vb2_run_result* out, int32_t* status, vb2_pair_fit* fits, bool interval, vb2_interval* ci)
{
    if (!a || !out || !status || a->num_sample < 1 || !a->pileup_paths || !a->base.ud_path || !a->base.mean_path ||
        !a->base.bed_path || a->base.num_pc < 1 || a->base.num_pc > VB2_MAX_PC || num_pair < 1 || !tumour || !normal) {
        set_error("vb2_cohort_run_paired: invalid argument");
        return VB2_ERR_INVALID;
    }
    if (a->base.num_device > 1 || a->base.num_device < 0) {
        set_error("--MatchedNormal takes one device: the normals' rows and the refits given them are not spread over several --Devices");
        return VB2_ERR_INVALID;
    }
    if (a->base.model.is_alpha_fixed) {
        set_error("--MatchedNormal cannot be combined with --FixAlpha: a fixed alpha leaves the refit nothing to estimate");
        return VB2_ERR_INVALID;
    }
    if (!(hom_min >= 0.0 && hom_min <= 1.0)) {
        set_error("--NormalHomMin takes a probability within [0, 1]");
        return VB2_ERR_INVALID;
    }
    if (const int rc = vb2::check_pairs("vb2_cohort_run_paired", a->num_sample, num_pair, tumour, normal)) return rc;
    return vb2::guarded([&] {
        CohortRunner runner(a, out, status);
        runner.enable_paired(num_pair, tumour, normal, hom_min, fits, interval, ci);
        const int rc = runner.run();
        if (rc && !runner.error().empty()) set_error(runner.error());
        return rc;
    });
}
}  // namespace

extern "C" int vb2_cohort_run_paired(const vb2_cohort_args* a, int32_t num_pair, const int32_t* tumour, const int32_t* normal,
                                     double hom_min, vb2_run_result* out, int32_t* status, vb2_pair_fit* fits)
{
    return cohort_run_paired(a, num_pair, tumour, normal, hom_min, out, status, fits, false, nullptr);
}

extern "C" int vb2_cohort_run_paired_intervals(const vb2_cohort_args* a, int32_t num_pair, const int32_t* tumour,
                                               const int32_t* normal, double hom_min, vb2_run_result* out, int32_t* status,
                                               vb2_pair_fit* fits, vb2_interval* ci)
{
    return cohort_run_paired(a, num_pair, tumour, normal, hom_min, out, status, fits, true, ci);
}
