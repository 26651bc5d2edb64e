// host_clock.h -- the host's wall clock in seconds, for the stage times of the stats structs.  Plain C++: no HIP header and
// nothing of context.h, so that bam_io.cpp and baq_host.cpp may include it.
#ifndef VB2_HOST_CLOCK_H_
#define VB2_HOST_CLOCK_H_

#include <chrono>

namespace vb2 {

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace vb2

#endif
