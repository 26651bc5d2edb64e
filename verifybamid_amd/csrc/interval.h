// interval.h -- the intervals of several samples advancing in lock-step (interval.cpp): one interval_at (context.h) per
// sample as a fiber of a FiberGang (lockstep.h).  A fiber parks at every derivative request; step() answers all parked
// requests with ONE call of a batched evaluator, made on the caller's own stack, and runs the fibers on to their next
// request or to their end.  Fibers come and go: the streaming cohort runner gives an idle fiber the next searched sample.
#ifndef VB2_INTERVAL_H_
#define VB2_INTERVAL_H_

#include <vector>

#include "context.h"
#include "lockstep.h"

namespace vb2 {

class IntervalGang {
public:
    struct Task {
        const vb2_model* model = nullptr;
        const vb2_estimate* est = nullptr;
        vb2_interval* out = nullptr;
        bool data_has_known_af = false;
        const char* label = nullptr;        // starts the sample's NOTICE lines (null: none)
        const IntervalOptions* opt = nullptr;   // null: the defaults
    };
    IntervalGang(int num_fiber, int num_pc);
    // fiber i takes the task and runs up to its first request, or to its end (what t points to outlives the fiber's run)
    int spawn(int i, const Task& t);
    bool idle(int i) const { return gang_.idle(i); }      // not running anything: never spawned, or its interval is over
    bool pending() const { return gang_.pending(); }      // some fiber is parked
    int result(int i) const { return rc_[i]; }            // of the interval fiber i ran last
    int size() const { return gang_.size(); }
    // one call of fn with the point of every parked fiber (slot = fiber index), then those fibers run on.  Non-zero: fn
    // failed -- every interval of the gang ends with that code.
    int step(const BatchDerivsFn& fn);
    int64_t steps = 0;

private:
    FiberGang gang_;
    int k_;
    std::vector<Task> task_;
    std::vector<int> rc_;
    std::vector<int32_t> np_;
    std::vector<double> p1_, p2_, al_, llk_, grad_, hess_;
};

}  // namespace vb2
#endif
