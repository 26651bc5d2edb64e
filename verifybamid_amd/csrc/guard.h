// guard.h -- the body of an extern "C" entry that may throw: no exception crosses the C boundary.
#ifndef VB2_GUARD_H_
#define VB2_GUARD_H_

#include <exception>
#include <new>
#include <string>

#include "../../include/vb2_abi.h"

namespace vb2 {

void set_error(const std::string& msg);         // (context.h)

template <class F>
int guarded(F&& f)
{
    try {
        return f();
    } catch (const std::bad_alloc&) {
        set_error("out of host memory");
        return VB2_ERR_NOMEM;
    } catch (const std::exception& e) {
        set_error(e.what());
        return VB2_ERR_INVALID;
    }
}

}  // namespace vb2
#endif
