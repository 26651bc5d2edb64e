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
// --CohortInterval (one device): every searched sample's confidence interval as well, computed in lock-step (interval.h)
// -- on the group's batch after its search, or, streaming, on an interval stage with a thread and a stream of its own that
// takes the samples the search is done with.
//
// This unit is the PIPELINE: group schedule, readers, the streamed and the grouped device pipelines, the interval stage
// and the releaser.  What a run does after its last sample is a list of vb2::CohortStage (cohort_stages.h; the stages and
// the entry points that choose them: cohort_stages.cpp), and nothing here knows one by name.  Three rules hold whatever
// the stages are:
//   1. the releaser thread alone puts a sample into the run's set and parks its context, after the sample's files are
//      written (streamed runs write them there, grouped runs on the device thread; a .CI before the sample gets there);
//   2. a run ends in ONE order: every thread joined, the stages' finish() in the order given, the parked contexts
//      destroyed, the run's own streams destroyed -- a set a stage builds on a parked context goes inside its finish();
//   3. a device-level failure is recorded with the last error of the thread it happened on (device_failure).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "batch.h"
#include "cohort_stages.h"
#include "context.h"
#include "device_util.h"
#include "estimator.h"
#include "guard.h"
#include "hostio.h"
#include "interval.h"
#include "run.h"
#include "stream_search.h"
#include "tunables.h"

using vb2::now_s;
using vb2::set_error;

namespace {

struct Slot {
    std::unique_ptr<vb2_flat> flat;
    vb2_ctx* ctx = nullptr;
    int rc = VB2_OK;
    bool ready = false;
};

class CohortRunner {
public:
    // stages.after: what the run does after its last sample (cohort_stages.h); stages.intervals: every searched sample's
    // vb2_interval as well (one device) -- <prefix>.CI, and ci[s] when ci is not null -- before the sample goes to the releaser
    CohortRunner(const vb2_cohort_args* a, vb2_run_result* out, int32_t* status, const vb2::CohortStages& stages)
        : a_(a), out_(out), status_(status), S_(a->num_sample), intervals_(stages.intervals), ci_(stages.ci),
          err_table_(stages.err_table)
    {
        for (vb2::CohortStage* st : stages.after)
            if (st) {
                after_.push_back(st);
                keep_raw_ = keep_raw_ || st->takes_flat();
            }
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
        bam_inflight_.assign(ndev_, 0);
        bam_cap_ = std::max(1, vb2::tunables().cohort_bam_inflight);
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

    ~CohortRunner() { shutdown(); release_parked_and_streams(); }

    int run()
    {
        for (int s = 0; s < S_; ++s) {
            std::memset(&out_[s], 0, sizeof(out_[s]));
            status_[s] = VB2_ERR_INVALID;
            if (ci_) std::memset(&ci_[s], 0, sizeof(ci_[s]));
        }
        vb2::cohort_bam_stats_reset(S_);
#ifdef VB2_WITH_HTSLIB
        // the htslib reader has never been compiled, let alone run from many threads at once: refused before anything is read
        for (int s = 0; s < S_; ++s)
            if (vb2::classify_list_entry(a_->pileup_paths[s]) == vb2::ListEntry::kBam) {
                set_error(std::string("vb2_cohort_run: ") + a_->pileup_paths[s] + ": .bam lines of a cohort are read by the built-in BAM "
                          "reader, which a library configured with VB2_WITH_HTSLIB does not have");
                return VB2_ERR_INVALID;
            }
#endif
        const bool timing = vb2::tunables().debug_timing != 0;
        const double t_run0 = now_s();
        // HIP runtime start-up (per device) behind the panel reading
        std::vector<std::thread> warm;
        for (int d : devices_)
            warm.emplace_back(vb2::warm_device, d);
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
        int planes = 0;                                  // one set with every plane a stage reads: a sample is put once
        for (const vb2::CohortStage* st : after_) planes |= st->planes;
        if (planes) {
            vb2::SourceSet* set = nullptr;
            if (const int rcs = vb2::SourceSet::create((int)panel_->NumMarker, S_, devices_[0], &set, planes)) {
                err_all_ = vb2::g_last_error;
                return rcs;
            }
            set_.reset(set);
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
                const int dev = device_index(d);
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
        shutdown();                                      // (rule 2 of this file's head, for every run)
        const vb2::CohortEnd end{a_, out_, status_, model_, set_.get(), parked_, parked_bytes_};
        for (size_t i = 0; i < after_.size() && !rc_all_; ++i)
            if ((rc_all_ = after_[i]->finish(end)) != VB2_OK) err_all_ = vb2::g_last_error;
        release_parked_and_streams();
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
    bool rel_stop_ = false;
    bool down_ = false;

    double rel_s_[2] = {0, 0};             // releaser thread: vb2_ctx_destroy, freeing the host arrays
    double phase_s_[3] = {0, 0, 0};        // reader threads' wall-clock: read_pileup, sanity + resolve, vb2_ctx_create

    // streaming (stream_search.h): sample s belongs to device s % ndev_
    bool stream_ = true;
    std::vector<int> inflight_;            // [device] samples handed to a reader and not yet done
    std::vector<int> remaining_;           // [device] samples not yet delivered to the search (or failed before it)
    std::vector<std::deque<int>> ready_q_; // [device] prepared samples, in the order they became ready
    // a sample on its way out: files to write (streamed runs); row: it was searched, the stages are asked about it
    struct Done { int s; vb2_ctx* ctx; std::unique_ptr<vb2_flat> flat; bool write; vb2_estimate est; bool row = false; };
    std::deque<Done> done_queue_;          // (rel_mu_)
    // the stages after the run (none: a plain run), their set (null without planes), the contexts they keep (releaser thread)
    std::vector<vb2::CohortStage*> after_;
    bool keep_raw_ = false;                 // a stage takes the samples' flattened inputs: the readers leave the raw arrays
    std::unique_ptr<vb2::SourceSet> set_;
    std::vector<vb2_ctx*> parked_;
    int64_t parked_bytes_ = 0;
    // --CohortInterval (false without it: nothing below then differs from a plain run).  Streaming: a searched sample waits
    // in iv_queue_ for a fiber of the interval stage (interval_loop), which has a thread and a stream of its own.
    bool intervals_ = false;
    const double* err_table_ = nullptr;    // every context under this error table (--ErrorTable), or null
    vb2_interval* ci_ = nullptr;
    struct IvItem { int s = -1; vb2_estimate est{}; };
    std::mutex iv_mu_;
    std::condition_variable iv_cv_;
    std::deque<IvItem> iv_queue_;
    bool iv_closed_ = false;

    // .bam lines between "file opened" and "context created", per device: each holds its inflated chunks on the host and its
    // kept records on the device (tunable cohort_bam_inflight)
    std::mutex bam_mu_;
    std::condition_variable bam_cv_;
    std::vector<int> bam_inflight_;
    int bam_cap_ = 4;
    struct BamGate {
        CohortRunner* r;
        int d;
        BamGate(CohortRunner* runner, int dev) : r(runner), d(dev)
        {
            if (d < 0) return;
            std::unique_lock<std::mutex> lk(r->bam_mu_);
            r->bam_cv_.wait(lk, [&] { return r->bam_inflight_[(size_t)d] < r->bam_cap_; });
            vb2::cohort_bam_peak_note(++r->bam_inflight_[(size_t)d]);
        }
        ~BamGate()
        {
            if (d < 0) return;
            {
                std::lock_guard<std::mutex> lk(r->bam_mu_);
                --r->bam_inflight_[(size_t)d];
            }
            r->bam_cv_.notify_all();
        }
        BamGate(const BamGate&) = delete;
        BamGate& operator=(const BamGate&) = delete;
    };

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
    }

    // the contexts the stages kept, THEN the run's own streams (every context and batch that used them is gone)
    void release_parked_and_streams()
    {
        for (vb2_ctx*& c : parked_)
            if (c) {
                vb2_ctx_destroy(c);
                c = nullptr;
            }
        for (hipStream_t& st : own_streams_)
            if (st) {
                (void)hipStreamSynchronize(st);
                (void)hipStreamDestroy(st);
                st = nullptr;
            }
    }

    // device d of the run as HIP numbers it, and its compute units
    int device_index(int d) const
    {
        int dev = devices_[d];
        if (dev < 0) (void)hipGetDevice(&dev);
        return dev;
    }
    static int cu_count(int dev)
    {
        hipDeviceProp_t prop;
        return hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }

    // a device-level failure concerns every sample: the run stops with the first one's code and text (the last error of
    // the thread it happened on, which is the caller's)
    void device_failure(int rc)
    {
        std::lock_guard<std::mutex> lk(mu_);
        if (!rc_all_) {
            rc_all_ = rc;
            err_all_ = vb2::g_last_error;
        }
        stop_ = true;
    }

    // Sample s's own files, each failure the sample's status: <prefix>.Ancestry and .selfSM of its search (flat: the
    // flattened sample's counters; null: not now), and of its interval (ci; ci_rc: the interval's own outcome) <prefix>.CI
    // and the caller's ci[s].
    void write_sample_files(int s, const vb2_flat* flat, const vb2_estimate& est, const vb2_interval* ci = nullptr, int ci_rc = VB2_OK)
    {
        const char* prefix = a_->output_prefixes ? a_->output_prefixes[s] : nullptr;
        if (flat && prefix) {
            int rw = vb2::write_ancestry(prefix, a_->base.num_pc, est.pc, est.pc2);
            if (!rw) rw = vb2::write_selfsm(prefix, *flat, est, /*pileup_input=*/!flat->from_bam);   // (#READS: NA for a text pileup)
            if (rw) status_[s] = rw;
        }
        if (!ci) return;
        if (!ci_rc && prefix) ci_rc = vb2::write_ci(prefix, *ci);
        if (!ci_rc && ci_) ci_[s] = *ci;
        if (ci_rc) status_[s] = ci_rc;
    }

    void prepare(int s)
    {
        Slot& sl = slots_[s];
        const double t0 = now_s();
        sl.flat.reset(new vb2_flat(panel_));
        vb2_flat& f = *sl.flat;
        // a ".bam" line goes through the built-in BAM reader, every other line is a text pileup; what follows the read is the
        // same for both (the reader fills the same PileupViewer)
        const std::string path = a_->pileup_paths[s];
        vb2::ListEntry kind = vb2::classify_list_entry(path);
        if (kind == vb2::ListEntry::kText && vb2::has_cram_magic(path)) kind = vb2::ListEntry::kCram;
        BamGate gate(this, kind == vb2::ListEntry::kBam ? device_of_sample(s) : -1);      // (held until the context exists)
        if (kind == vb2::ListEntry::kCram) {
            set_error(vb2::cram_message(path));
            sl.rc = VB2_ERR_INVALID;
        } else if (kind == vb2::ListEntry::kBam) {
            vb2::BamReadHow how;
            how.threads = vb2::cohort_bam_pool(T_);
            // the device stage on one of the device's two creation streams, never on a lane's hardware queue (see run())
            if (!own_streams_.empty()) how.stream = own_streams_[(size_t)device_of_sample(s) * 4 + 2 + (size_t)(s / ndev_) % 2];
            how.bam_adjust = a_->base.bam_adjust;      // --ApplyBAQ reaches a cohort's .bam lines as the pileup options do
            vb2_baq_stats baq_stats{};
            how.baq_stats = &baq_stats;
            sl.rc = vb2::read_bam(path, a_->base.reference_path ? a_->base.reference_path : "", *panel_, &f.viewer, &a_->base.mpileup,
                                  devices_[device_of_sample(s)], &f.bam_stats, &how);
            f.from_bam = sl.rc == VB2_OK;
            if (f.from_bam) vb2::cohort_bam_stats_put(s, f.bam_stats);
        } else {
            sl.rc = vb2::read_pileup(path, *panel_, &f.viewer);
        }
        if (sl.rc) {
            // a sample's own failure is its status; what went wrong is said here, once (the caller's last error is the run's)
            if (kind != vb2::ListEntry::kText)
                std::fprintf(stderr, "WARNING - cohort sample %d (%s): %s\n", s, path.c_str(), vb2::g_last_error.c_str());
            return;
        }
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
        sl.rc = err_table_ ? vb2_ctx_create_ex(&f.input, &opt, err_table_, &sl.ctx) : vb2_ctx_create(&f.input, &opt, &sl.ctx);
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
        // (unless a stage takes the flattened input: CohortStage::takes_flat)
        std::string().swap(f.viewer.basePool);
        std::string().swap(f.viewer.qualPool);
        if (!keep_raw_) {
            std::string().swap(f.bases);
            std::string().swap(f.quals);
            std::vector<int64_t>().swap(f.read_off);
            f.input = vb2_input{};
        }
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
            d.row = write && est;
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
                    r->iv_queue_.push_back(IvItem{s, est});
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
        write_sample_files(s, nullptr, est, &ci, rc);
        finish_sample(s, true, &est, /*delivered=*/true);
    }

    // The interval stage of a streaming run: as many fibers as the search has slots, each running one sample's interval
    // (interval.h).  At a step boundary an idle fiber takes the next searched sample; a step -- one Batch::derivs call for
    // every live fiber's point -- goes out as soon as all live fibers have parked, however few they are.  The search of later
    // samples goes on meanwhile on its own thread and streams.
    void interval_loop(int d)
    {
        const int dev = device_index(d);
        int fail = hipSetDevice(dev) == hipSuccess ? VB2_OK : VB2_ERR_HIP;
        if (fail) set_error("--CohortInterval: hipSetDevice failed");
        const int k = a_->base.num_pc;
        std::unique_ptr<vb2::Batch> batch;
        if (!fail) {
            vb2::Batch* bp = nullptr;
            fail = vb2::Batch::create_slots(G_, dev, k, cu_count(dev), &bp);
            batch.reset(bp);
        }
        if (fail) device_failure(fail);              // (the run stops, what is queued leaves with the failure's code)
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
                if (!fail) device_failure(fail = rc);
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
        const int dev = device_index(d);
        const int num_cu = cu_count(dev);
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
            rc = vb2::stream_search(dev, a_->base.num_pc, num_cu, G_, src, own_streams_.empty() ? nullptr : &own_streams_[(size_t)d * 4]);
        } catch (const std::exception& e) {
            set_error(e.what());
            rc = VB2_ERR_INVALID;
        }
        if (timing)
            std::fprintf(stderr, "vb2_cohort_run: device %d: %d slots, stream over after %.1f ms\n", devices_[d], G_, 1e3 * (now_s() - t0));
        if (rc) device_failure(rc);
        cv_.notify_all();
    }

    // The releaser: a sample's files (streamed runs: here; grouped runs wrote them on the device thread), THEN its row in the
    // set and whether its context stays -- the stages' answers, in their order --, then the context and the host arrays go.
    void release_loop()
    {
        for (;;) {
            std::unique_lock<std::mutex> lk(rel_mu_);
            rel_cv_.wait(lk, [&] { return rel_stop_ || !done_queue_.empty(); });
            if (done_queue_.empty()) return;
            Done d = std::move(done_queue_.front());
            done_queue_.pop_front();
            lk.unlock();
            if (d.write && d.flat) write_sample_files(d.s, d.flat.get(), d.est);    // (they need the flattened sample's counters)
            if (d.row && d.ctx && d.ctx->impl && status_[d.s] == VB2_OK) {
                // (a sample whose row cannot be made keeps its files and its status -- it was searched and written as the
                // plain run does it --; its row and column of a matrix are NaN and a NOTICE says why)
                bool made = false, keep = false;
                for (const vb2::CohortStage* st : after_)
                    if (set_ && st->planes && st->wants_row(d.s)) {
                        made = set_->put(d.s, d.ctx->impl, model_, d.est) == VB2_OK;
                        if (!made)
                            std::fprintf(stderr, "NOTICE - %s: sample %d has no row in the source set: %s\n", st->flag, d.s,
                                         vb2::g_last_error.c_str());
                        break;                           // (put once, whatever the number of stages that read the row)
                    }
                for (const vb2::CohortStage* st : after_) keep = keep || st->keeps(d.s, made);
                if (keep) {                              // searched and written: parked for finish(), not destroyed
                    if (parked_.empty()) parked_.assign((size_t)S_, nullptr);
                    parked_[(size_t)d.s] = d.ctx;
                    parked_bytes_ += d.ctx->impl->device_bytes;
                    d.ctx = nullptr;
                }
            }
            if (keep_raw_ && d.row && d.flat && status_[d.s] == VB2_OK)
                for (vb2::CohortStage* st : after_)
                    if (st->takes_flat()) {
                        st->take_flat(d.s, std::move(d.flat), d.est);
                        break;
                    }
            const double t0 = now_s();
            if (d.ctx) vb2_ctx_destroy(d.ctx);
            const double t1 = now_s();
            d.flat.reset();
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
                        write_sample_files(s, slots_[s].flat.get(), est[i], intervals_ ? &civ[i] : nullptr, intervals_ ? ist[i] : VB2_OK);
                    }
                }
            }
            const double tg_opt = now_s();
            {   // freeing device and pinned memory synchronises with the device and takes milliseconds
                // per context: hand the group to the releaser thread and move on
                std::lock_guard<std::mutex> lk(rel_mu_);
                for (int s = g0; s < g1; ++s) {      // (nothing to write: the files are written)
                    Done d{s, slots_[s].ctx, std::move(slots_[s].flat), false, out_[s].est};
                    d.row = !rcb && status_[s] == VB2_OK && slots_[s].ctx != nullptr;
                    done_queue_.push_back(std::move(d));
                    slots_[s].ctx = nullptr;
                }
            }
            rel_cv_.notify_one();
            if (timing)
                std::fprintf(stderr, "vb2_cohort_run: device %d group %d (samples %d-%d): waited %.1f ms for the "
                                     "readers, search + outputs %.1f ms\n", devices_[d], gi, g0, g1 - 1,
                             1e3 * (tg_wait - tg0), 1e3 * (tg_opt - tg_wait));
            if (rcb) device_failure(rcb);
            {
                std::lock_guard<std::mutex> lk(mu_);
                ++cnt_[d];
            }
            cv_.notify_all();
            if (rcb) return;
        }
    }

public:
    const std::string& error() const { return err_all_; }
};

}  // namespace

int vb2::cohort_run_with(const vb2_cohort_args* a, vb2_run_result* out, int32_t* status, const CohortStages& stages)
{
    return vb2::guarded([&] {
        CohortRunner runner(a, out, status, stages);
        const int rc = runner.run();
        if (rc && !runner.error().empty()) set_error(runner.error());
        return rc;
    });
}

