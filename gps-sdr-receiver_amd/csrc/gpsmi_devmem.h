// DevBuf<T>: the one owner of a device allocation in libgpsmi ("How a handle owns
// memory").  Every device buffer of a handle is a DevBuf member: it is released when the handle is
// deleted, and its capacity travels with it, in elements of T.
#pragma once
#include "gpsmi_common.h"
#include "gpsmi_event_scope.h"

namespace gpsmi {

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;                        // capacity in elements of T

    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }

    // Room for `count` elements: nothing when there is, else the old block is freed and exactly
    // `count` allocated (the contents are not kept).  A failure leaves the buffer empty and the
    // handle usable: GPSMI_E_NOMEM when the device cannot serve the request, `what` names the
    // buffer in the error text.
    int reserve(size_t count, const char* what) {
        if (count <= n) return GPSMI_OK;
        if (p) GPSMI_HIP(hipFree(p));
        p = nullptr; n = 0;
        const hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {
                (void)hipGetLastError();     // (the error is sticky: the next GPSMI_HIP would see it)
                return fail(GPSMI_E_NOMEM, "%s: no device memory for %zu bytes", what, count * sizeof(T));
            }
            return fail(GPSMI_E_HIP, "hipMalloc: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
        }
        n = count;
        return GPSMI_OK;
    }

    // reserve, then all bytes zero (a blocking memset, at create time)
    int reserve_zeroed(size_t count, const char* what) {
        const int rc = reserve(count, what);
        if (rc) return rc;
        GPSMI_HIP(hipMemset(p, 0, count * sizeof(T)));
        return GPSMI_OK;
    }

    // reserve, then a blocking copy of a host table (at create time)
    int upload(const std::vector<T>& v, const char* what) {
        const int rc = reserve(v.size(), what);
        if (rc) return rc;
        GPSMI_HIP(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return GPSMI_OK;
    }

    void release() {
        if (p) (void)hipFree(p);
        p = nullptr; n = 0;
    }
};

// DevStream / DevEvent: the one owner of a stream / an event of a handle, empty until create().  They
// convert to the runtime's handle, which is what HandleSync, the launch sites and every runtime call
// take (borrowed, never destroyed there).
template <typename H, hipError_t (*Destroy)(H)>
struct DevHandle {
    H h = nullptr;
    DevHandle() = default;
    DevHandle(DevHandle&& o) noexcept : h(o.h) { o.h = nullptr; }
    DevHandle& operator=(DevHandle&& o) noexcept {
        if (this != &o) { release(); h = o.h; o.h = nullptr; }
        return *this;
    }
    DevHandle(const DevHandle&) = delete;
    DevHandle& operator=(const DevHandle&) = delete;
    ~DevHandle() { release(); }
    operator H() const { return h; }
    void release() {
        if (h) (void)Destroy(h);
        h = nullptr;
    }
};
struct DevStream : DevHandle<hipStream_t, hipStreamDestroy> {
    int create() {
        GPSMI_HIP(hipStreamCreate(&h));
        return GPSMI_OK;
    }
};
// An event is created as the row W of the classification (gpsmi_event_scope.h) and names its scope S at
// the call: create<Ev::TrkCopied, EventScope::HostVisible>().  A call that disagrees with the table
// does not compile.  Whether the event records time is the row's.
struct DevEvent : DevHandle<hipEvent_t, hipEventDestroy> {
    template <Ev W, EventScope S>
    int create() {
        constexpr EventClass c = event_class(W);
        static_assert(c.scope == S, "the scope named here is not the one of the event's row in gpsmi_event_scope.h");
        GPSMI_HIP(hipEventCreateWithFlags(&h, (c.stamps ? hipEventDefault : hipEventDisableTiming) |
                                                  (S == EventScope::DeviceOnly ? hipEventDisableSystemFence : 0u)));
        return GPSMI_OK;
    }
};

}  // namespace gpsmi
