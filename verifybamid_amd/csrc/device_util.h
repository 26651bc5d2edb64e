// device_util.h -- what the host files around the per-marker kernels share (internal): the HIP error macro, device slabs
// from the context's cache, the owners of device buffers, pinned buffers, streams and events, and the host clock.
#ifndef VB2_DEVICE_UTIL_H_
#define VB2_DEVICE_UTIL_H_

#include <hip/hip_runtime_api.h>

#include <string>
#include <vector>

#include "context.h"
#include "host_clock.h"

// in a function that returns a VB2_* code: a failed call sets the error text and returns VB2_ERR_HIP
#define VB2_HIP(call)                                                                  \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                        \
            set_error(std::string(#call) + " failed: " + hipGetErrorString(e_));       \
            return VB2_ERR_HIP;                                                        \
        }                                                                              \
    } while (0)

namespace vb2 {

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// The HIP runtime takes ~0.2 s to come up in a fresh process: the body of a helper thread that starts it on `device`
// (< 0: the current one) while the caller reads files.  Errors surface later, where a context is created.
inline void warm_device(int device)
{
    if (device >= 0) (void)hipSetDevice(device);
    (void)hipFree(nullptr);
    (void)hipGetLastError();
}

// A device slab from the cache, or a fresh one.  When hipMalloc fails: VB2_ERR_HIP with the call's text, or, where the
// caller names itself in nomem_who, VB2_ERR_NOMEM with "<who>: N bytes of device memory do not fit".
inline int take_device(size_t bytes, int device, void** p, size_t* got, const char* nomem_who = nullptr)
{
    *p = cached_device_slab(bytes, device, got);
    if (*p) return VB2_OK;
    if (!nomem_who) {
        VB2_HIP(hipMalloc(p, bytes));
    } else if (hipMalloc(p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        set_error(std::string(nomem_who) + ": " + std::to_string(bytes) + " bytes of device memory do not fit");
        return VB2_ERR_NOMEM;
    }
    *got = bytes;
    return VB2_OK;
}
inline void give_device(void* p, size_t bytes, int device)
{
    if (p && !recycle_device_slab(p, bytes, device)) (void)hipFree(p);
}

// device and pinned allocations, a stream, an event: owned by a scope or an object, released on every exit path
struct DeviceBuffer {
    void* p = nullptr;
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { if (p) (void)hipFree(p); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
struct PinnedBuffer {
    void* p = nullptr;
    PinnedBuffer() = default;
    PinnedBuffer(const PinnedBuffer&) = delete;
    PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    ~PinnedBuffer() { if (p) (void)hipHostFree(p); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
struct OwnedStream {
    hipStream_t s = nullptr;
    OwnedStream() = default;
    OwnedStream(const OwnedStream&) = delete;
    OwnedStream& operator=(const OwnedStream&) = delete;
    ~OwnedStream() { if (s) (void)hipStreamDestroy(s); }
};
struct OwnedEvent {
    hipEvent_t e = nullptr;
    OwnedEvent() = default;
    OwnedEvent(const OwnedEvent&) = delete;
    OwnedEvent& operator=(const OwnedEvent&) = delete;
    ~OwnedEvent() { if (e) (void)hipEventDestroy(e); }
};
struct DeviceBufferList {      // freed first to last
    std::vector<void*> v;
    DeviceBufferList() = default;
    DeviceBufferList(const DeviceBufferList&) = delete;
    DeviceBufferList& operator=(const DeviceBufferList&) = delete;
    ~DeviceBufferList() { for (void* p : v) (void)hipFree(p); }
};

struct TimerEvents {
    hipEvent_t a = nullptr, b = nullptr;
    ~TimerEvents()
    {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

}  // namespace vb2
#endif
