// A stand-in for <hip/hip_runtime.h>, for tests/cpp/device_mem_check.cpp alone: the runtime calls madsim_amd/csrc/device_mem.h uses, backed by
// malloc, with counters of live objects and a countdown that makes the k-th creating call fail.  No device, no HIP.
#pragma once
#include <cstddef>
#include <cstdlib>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
typedef struct fake_stream* hipStream_t;
typedef struct fake_event* hipEvent_t;
enum { hipHostMallocDefault = 0, hipStreamNonBlocking = 1 };

struct FakeHip {
    long live_dev = 0, live_pinned = 0, live_events = 0, live_streams = 0;      // objects created and not yet released
    long frees = 0, bad_frees = 0;                                               // releases in all, releases of something not live
    long syncs = 0;                                                              // hipStreamSynchronize calls
    long fail_in = 0;                                                            // k > 0: the k-th creating call from now fails
    long creating_calls = 0;
    bool refuse() { creating_calls++; return fail_in > 0 && --fail_in == 0; }
    long live() const { return live_dev + live_pinned + live_events + live_streams; }
};
inline FakeHip& fake_hip() { static FakeHip f; return f; }

// every object is a malloc'ed block whose first word says what it is, so a release of the wrong kind, or a second one, is counted
// (and the second free is then AddressSanitizer's to report)
namespace fake_hip_detail {
enum Kind : long { DEV = 0x11, PINNED = 0x22, EVENT = 0x33, STREAM = 0x44, DEAD = 0x55 };
inline void* make(Kind k, size_t bytes, long& live) {
    if (fake_hip().refuse()) return nullptr;
    long* b = static_cast<long*>(malloc(2 * sizeof(long) + bytes));
    if (!b) return nullptr;
    b[0] = k; live++;
    return b + 2;
}
inline hipError_t release(void* p, Kind k, long& live) {
    fake_hip().frees++;
    if (!p) { fake_hip().bad_frees++; return 1; }
    long* b = static_cast<long*>(p) - 2;
    if (b[0] != k) { fake_hip().bad_frees++; return 1; }
    b[0] = DEAD; live--;
    free(b);
    return hipSuccess;
}
}  // namespace fake_hip_detail

inline hipError_t hipMalloc(void** p, size_t bytes) {
    *p = fake_hip_detail::make(fake_hip_detail::DEV, bytes, fake_hip().live_dev);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
inline hipError_t hipFree(void* p) { return fake_hip_detail::release(p, fake_hip_detail::DEV, fake_hip().live_dev); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) {
    *p = fake_hip_detail::make(fake_hip_detail::PINNED, bytes, fake_hip().live_pinned);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
inline hipError_t hipHostFree(void* p) { return fake_hip_detail::release(p, fake_hip_detail::PINNED, fake_hip().live_pinned); }
inline hipError_t hipEventCreate(hipEvent_t* e) {
    *e = static_cast<hipEvent_t>(fake_hip_detail::make(fake_hip_detail::EVENT, 8, fake_hip().live_events));
    return *e ? hipSuccess : hipErrorOutOfMemory;
}
inline hipError_t hipEventDestroy(hipEvent_t e) { return fake_hip_detail::release(e, fake_hip_detail::EVENT, fake_hip().live_events); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
    *s = static_cast<hipStream_t>(fake_hip_detail::make(fake_hip_detail::STREAM, 8, fake_hip().live_streams));
    return *s ? hipSuccess : hipErrorOutOfMemory;
}
inline hipError_t hipStreamDestroy(hipStream_t s) { return fake_hip_detail::release(s, fake_hip_detail::STREAM, fake_hip().live_streams); }
inline hipError_t hipStreamSynchronize(hipStream_t) { fake_hip().syncs++; return hipSuccess; }
