// lockstep.cpp -- see lockstep.h.
#include "lockstep.h"

#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <string>

#include "estimator.h"

namespace vb2 {

void set_error(const std::string& msg);         // (context.h, which this file stays clear of: it brings HIP in)

namespace {
constexpr size_t kFiberStack = 256 * 1024;      // the optimiser's frames are a few KB deep
size_t page_size()
{
    static const size_t p = (size_t)std::max(4096L, sysconf(_SC_PAGESIZE));
    return p;
}
}

FiberGang::FiberGang(int num_fiber, int max_points_per_request)
    : fibers_(num_fiber), cb_(num_fiber), req_(num_fiber), max_points_(std::max(1, max_points_per_request))
{
    for (int i = 0; i < num_fiber; ++i) cb_[i] = Cb{this, i};
}

FiberGang::~FiberGang()
{
    for (Fiber& f : fibers_)
        if (f.map) munmap(f.map, kFiberStack + page_size());
}

void FiberGang::entry(unsigned lo, unsigned hi)
{
    FiberGang* g = reinterpret_cast<FiberGang*>(((uintptr_t)hi << 32) | (uintptr_t)lo);
    const int i = g->cur_;
    g->body_(i);                     // (never throws: the body catches)
    g->fibers_[i].done = true;
    g->req_[i].n = 0;
}                                    // uc_link: back to run()

int FiberGang::eval_cb(void* user, int32_t n, const double* p1, const double* p2, const double* a, double* o)
{
    Cb* cb = static_cast<Cb*>(user);
    FiberGang* g = cb->gang;
    const int k = g->num_pc_;
    for (int done = 0; done < n; done += g->max_points_) {
        Request& r = g->req_[cb->index];
        r.n = std::min(g->max_points_, n - done);
        r.p1 = p1 + (size_t)done * k;
        r.p2 = p2 + (size_t)done * k;
        r.a = a + done;
        r.out = o + done;
        r.grad = r.hess = nullptr;
        swapcontext(&g->fibers_[cb->index].ctx, &g->main_);      // parked until the step has been evaluated
        if (g->error_) return g->error_;
    }
    return 0;
}

int FiberGang::derivs_cb(void* user, const double* p1, const double* p2, double a, double* llk, double* grad, double* hess)
{
    Cb* cb = static_cast<Cb*>(user);
    FiberGang* g = cb->gang;
    Request& r = g->req_[cb->index];
    r.n = 1;
    r.p1 = p1;
    r.p2 = p2;
    r.a = &a;
    r.out = llk;
    r.grad = grad;
    r.hess = hess;
    swapcontext(&g->fibers_[cb->index].ctx, &g->main_);          // parked until the step has been evaluated
    return g->error_;
}

int FiberGang::prepare(int i)
{
    Fiber& f = fibers_[i];
    if (!f.map) {
        // stacks grow downwards: an overflow hits the PROT_NONE page and faults instead of
        // scribbling over the heap
        void* m = mmap(nullptr, kFiberStack + page_size(), PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m == MAP_FAILED) return -1;
        (void)mprotect(m, page_size(), PROT_NONE);
        f.map = m;
    }
    f.done = false;
    req_[i] = Request{};
    if (getcontext(&f.ctx) != 0) return -1;
    f.ctx.uc_stack.ss_sp = static_cast<char*>(f.map) + page_size();
    f.ctx.uc_stack.ss_size = kFiberStack;
    f.ctx.uc_link = &main_;
    const uintptr_t p = reinterpret_cast<uintptr_t>(this);
    makecontext(&f.ctx, reinterpret_cast<void (*)()>(entry), 2, (unsigned)(p & 0xffffffffu), (unsigned)(p >> 32));
    return 0;
}

int FiberGang::start(int num_pc, const std::function<void(int)>& body)
{
    num_pc_ = num_pc;
    body_ = body;
    error_ = 0;
    const int n = (int)fibers_.size();
    for (int i = 0; i < n; ++i)
        if (prepare(i) < 0) return -1;
    for (int i = 0; i < n; ++i) {                                  // up to everybody's first request
        cur_ = i;
        swapcontext(&main_, &fibers_[i].ctx);
    }
    return 0;
}

void FiberGang::open(int num_pc, const std::function<void(int)>& body)
{
    num_pc_ = num_pc;
    body_ = body;
    error_ = 0;
    for (size_t i = 0; i < fibers_.size(); ++i) {
        fibers_[i].done = true;
        req_[i] = Request{};
    }
}

int FiberGang::spawn(int i)
{
    if (prepare(i) < 0) {
        fibers_[i].done = true;
        return -1;
    }
    cur_ = i;
    swapcontext(&main_, &fibers_[i].ctx);                          // up to its first request, or to the end
    return 0;
}

bool FiberGang::pending() const
{
    for (size_t i = 0; i < fibers_.size(); ++i)
        if (!fibers_[i].done && req_[i].n > 0) return true;
    return false;
}

void FiberGang::resume_parked()
{
    const int n = (int)fibers_.size();
    for (int i = 0; i < n; ++i) {
        if (fibers_[i].done || req_[i].n <= 0) continue;
        req_[i].n = 0;
        cur_ = i;
        swapcontext(&main_, &fibers_[i].ctx);                      // up to its next request, or to the end
    }
}

int FiberGang::run(int num_pc, const std::function<void(int)>& body, const StepFn& step)
{
    if (start(num_pc, body) < 0) return -1;
    while (pending()) {
        if (!error_) {
            ++steps;
            const int rc = step(req_);
            if (rc) error_ = rc;                                   // the fibers see it and unwind
        }
        resume_parked();
    }
    return error_;
}

int FiberGang::search(int i, const Search& cfg, const char* caller, vb2_estimate* out) noexcept
{
    try {
        Estimator est(num_pc_, cfg.eval ? cfg.eval : eval_cb, cfg.eval ? cfg.eval_user : user(i));
        apply_model(est, *cfg.model, cfg.data_has_known_af);
        est.speculate = cfg.speculate;
        est.line_search = cfg.line_search;
        est.start_index = cfg.start_index;
        est.start_seed = cfg.start_seed;
        if (cfg.start_sd > 0) est.start_sd = cfg.start_sd;
        const int rc = est.OptimizeLLK();
        fill_estimate(est, out);
        return rc;
    } catch (const std::bad_alloc&) {
        return VB2_ERR_NOMEM;
    } catch (const std::exception& e) {
        set_error(e.what());
        return VB2_ERR_INVALID;
    } catch (...) {                              // nothing may unwind past the fiber's entry frame
        set_error(std::string(caller) + ": unknown exception in a search");
        return VB2_ERR_INVALID;
    }
}

FiberGang::StepFn FiberGang::concat_step(int num_pc, ConcatEval eval)
{
    std::vector<int32_t> npt;
    std::vector<double> p1, p2, al, vals;
    return [=](std::vector<Request>& req) mutable {
        p1.clear(); p2.clear(); al.clear();
        npt.assign(req.size(), 0);
        for (size_t i = 0; i < req.size(); ++i) {
            const Request& r = req[i];
            if (r.n <= 0) continue;
            npt[i] = r.n;
            p1.insert(p1.end(), r.p1, r.p1 + (size_t)r.n * num_pc);
            p2.insert(p2.end(), r.p2, r.p2 + (size_t)r.n * num_pc);
            al.insert(al.end(), r.a, r.a + r.n);
        }
        vals.assign(al.size(), 0.0);
        if (const int rc = eval(npt.data(), al.size(), p1.data(), p2.data(), al.data(), vals.data())) return rc;
        size_t o = 0;
        for (Request& r : req) {
            if (r.n <= 0) continue;
            std::memcpy(r.out, &vals[o], sizeof(double) * r.n);
            o += (size_t)r.n;
        }
        return 0;
    };
}

FiberGang::StepFn FiberGang::concat_step(int num_pc, vb2_eval_fn eval, void* user)
{
    return concat_step(num_pc, [eval, user](const int32_t*, size_t total, const double* p1, const double* p2, const double* a,
                                            double* out) { return eval(user, (int32_t)total, p1, p2, a, out); });
}

}  // namespace vb2
