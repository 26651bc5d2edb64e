// lockstep.h -- several optimiser runs advancing in lock-step on ONE host thread.
//
// Every run (a sample of a cohort, a restart of a multi-start search) executes ordinary blocking
// code -- Estimator::OptimizeLLK with the reference-exact simplex -- as a FIBER: its own small
// stack, switched with swapcontext.  A fiber runs until its optimiser asks for likelihood values,
// parks the request and yields; when every live fiber has parked, the step callback evaluates all
// requests together (one kernel launch), the values are handed back and the fibers run on.  No
// threads, no locks, no wake-ups: a step costs the host ~0.3 us per run where one thread per run
// cost a futex round trip each (9 ms of CPU per sample and search at C3 size, and under a
// container's CPU quota it throttled the readers and the search alike).
//
// Two helpers every user of a gang shares, no device in either: FiberGang::search, the body of a search fiber (one configured
// OptimizeLLK to its rc and vb2_estimate), and FiberGang::concat_step, a step that answers all requests with ONE evaluator call.
#ifndef VB2_LOCKSTEP_H_
#define VB2_LOCKSTEP_H_

#include <ucontext.h>

#include <cstdint>
#include <functional>
#include <memory>
#include <vector>

#include "../../include/vb2_abi.h"

namespace vb2 {

class FiberGang {
public:
    // A parked request: n points (rows of pc1 / pc2 with num_pc columns, alpha) and where the
    // values go.  The pointers are into the fiber's own frames: alive while it is parked.
    struct Request {
        int n = 0;
        const double *p1 = nullptr, *p2 = nullptr, *a = nullptr;
        double* out = nullptr;
        // a derivative request (derivs_cb; n = 1) also wants the gradient [2k+1] and the Hessian [2k+1][2k+1] of its point;
        // null for the searches' requests, whose steps never look at them
        double *grad = nullptr, *hess = nullptr;
    };
    // evaluates every request with n > 0 (writes req[i].out[0..n)); non-zero = error for all
    typedef std::function<int(std::vector<Request>& req)> StepFn;

    explicit FiberGang(int num_fiber, int max_points_per_request);
    ~FiberGang();
    // the evaluator to hand to run i's Estimator (vb2_eval_fn signature) and its user pointer
    static int eval_cb(void* user, int32_t n, const double* p1, const double* p2, const double* a, double* o);
    void* user(int i) { return &cb_[i]; }
    // the same for code that asks for ONE point's LLK, gradient and Hessian (the interval's Profiler, interval.cpp)
    static int derivs_cb(void* user, const double* p1, const double* p2, double a, double* llk, double* grad, double* hess);
    // body(i) runs as fiber i; it must not let an exception escape
    int run(int num_pc, const std::function<void(int)>& body, const StepFn& step);
    int64_t steps = 0;

    // The same in pieces, for a caller that keeps several gangs going (one gang's step on the
    // device while another gang's fibers run on the host):
    int start(int num_pc, const std::function<void(int)>& body);   // every fiber up to its first request; < 0: no contexts
    bool pending() const;                                           // some fiber is parked with a request
    std::vector<Request>& requests() { return req_; }
    void fail(int rc) { if (!error_) error_ = rc; }                 // the fibers see it at resume and unwind
    int error() const { return error_; }
    void resume_parked();                                           // values delivered: every parked fiber runs on
    // A gang whose fibers come and go (the streaming cohort search: a finished sample's fiber is given the next sample):
    // open() starts with every fiber idle; spawn(i) runs body(i) as fiber i up to its first request (or to its end);
    // idle(i): fiber i is not running anything (never spawned, or its body has returned).
    void open(int num_pc, const std::function<void(int)>& body);
    int spawn(int i);                                               // < 0: no context / stack
    bool idle(int i) const { return fibers_[i].done; }
    int size() const { return (int)fibers_.size(); }

    // What the search of one fiber is configured with (estimator.h has the meaning of each field).
    struct Search {
        const vb2_model* model = nullptr;
        bool data_has_known_af = false;     // (Context::L.known_af: apply_model)
        int speculate = 4;
        bool line_search = false;
        int start_index = 0;
        uint32_t start_seed = 0;
        double start_sd = 0;                // <= 0: the Estimator's own
        // what the Estimator calls for its values instead of eval_cb on user(i) (null: that); it must end up in eval_cb on
        // user(i) itself -- a wrapper that holds one side of the points or looks at the values on their way (refit.cpp)
        vb2_eval_fn eval = nullptr;
        void* eval_user = nullptr;
    };
    // For body(i): that search on fiber i's evaluator.  Fills *out when the optimiser returned and gives its code, or
    // VB2_ERR_NOMEM / VB2_ERR_INVALID with the last error set (`caller` goes into the message for an unknown exception).
    int search(int i, const Search& cfg, const char* caller, vb2_estimate* out) noexcept;
    // A StepFn that evaluates the points of all requests with ONE call and hands the values back: the requests' rows one
    // after the other, `total` points, num_point[i] of them fiber i's (0: it asked for none); out[] starts as zeros.
    typedef std::function<int(const int32_t* num_point, size_t total, const double* p1, const double* p2, const double* a,
                              double* out)>
        ConcatEval;
    static StepFn concat_step(int num_pc, ConcatEval eval);
    // the same for an evaluator that does not ask whose the points are: eval(user, total, ...)
    static StepFn concat_step(int num_pc, vb2_eval_fn eval, void* user);

private:
    struct Fiber {
        ucontext_t ctx;
        void* map = nullptr;                // mmap'ed: one inaccessible guard page below the stack
        bool done = false;
    };
    struct Cb {
        FiberGang* gang;
        int index;
    };
    static void entry(unsigned lo, unsigned hi);
    ucontext_t main_;
    std::vector<Fiber> fibers_;
    std::vector<Cb> cb_;
    std::vector<Request> req_;
    std::function<void(int)> body_;
    int cur_ = -1, num_pc_ = 0, max_points_, error_ = 0;
    int prepare(int i);                  // fiber i's stack and context, ready to enter body(i)
};

}  // namespace vb2
#endif
