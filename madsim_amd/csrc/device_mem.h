// device_mem.h — the owning types of the host runtime (madsim_hip.cpp): a device buffer, a page-locked host buffer, an event and a stream.
// Each is move-only, releases what it holds in reset() (which its destructor runs) and converts to the raw handle, so a launch line reads as
// it would with a bare pointer.  A context releases its members while its device is bound (madsim_hip_ctx::close); the destructors then find
// nothing left.  Nothing here is more general than madsim_hip.cpp needs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace madsim_mem {

// `cap` elements of T in device memory (Pinned: in page-locked host memory).
template <class T, bool Pinned>
struct Buf {
    T* p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { reset(); }
    void reset() {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr; cap = 0;
    }
    // Room for `want` elements: grows only (a smaller request is a no-op) and never keeps the old contents.  A failure leaves {nullptr, 0},
    // so the next call tries again.  The second form is for a buffer that work queued on `drain` may still use: that stream is
    // synchronised before a live buffer is freed (the null stream is a stream like any other here).
    hipError_t room(size_t want) { return grow(want, false, nullptr); }
    hipError_t room(size_t want, hipStream_t drain) { return grow(want, true, drain); }
    operator T*() const { return p; }

private:
    hipError_t grow(size_t want, bool draining, hipStream_t drain) {
        if (want <= cap) return hipSuccess;
        if (p && draining) {
            hipError_t e = hipStreamSynchronize(drain);
            if (e != hipSuccess) return e;                       // (the buffer may still be in use: it stays as it is)
        }
        reset();
        void* q = nullptr;
        hipError_t e = Pinned ? hipHostMalloc(&q, want * sizeof(T), hipHostMallocDefault) : hipMalloc(&q, want * sizeof(T));
        if (e != hipSuccess) return e;
        p = static_cast<T*>(q); cap = want;
        return hipSuccess;
    }
};
template <class T> using DevBuf = Buf<T, false>;
template <class T> using PinnedBuf = Buf<T, true>;

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept {
        if (this != &o) { reset(); e = o.e; o.e = nullptr; }
        return *this;
    }
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { reset(); }
    void reset() {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    hipError_t ensure() {                                        // created on first use
        if (e) return hipSuccess;
        hipEvent_t made = nullptr;
        hipError_t rc = hipEventCreate(&made);
        if (rc == hipSuccess) e = made;
        return rc;
    }
    operator hipEvent_t() const { return e; }
};

// A non-blocking stream (hipStreamNonBlocking: it does not synchronise with the null stream).
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
    Stream& operator=(Stream&& o) noexcept {
        if (this != &o) { reset(); s = o.s; o.s = nullptr; }
        return *this;
    }
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { reset(); }
    void reset() {
        if (s) (void)hipStreamDestroy(s);
        s = nullptr;
    }
    hipError_t ensure() {
        if (s) return hipSuccess;
        hipStream_t made = nullptr;
        hipError_t rc = hipStreamCreateWithFlags(&made, hipStreamNonBlocking);
        if (rc == hipSuccess) s = made;
        return rc;
    }
    operator hipStream_t() const { return s; }
};

}  // namespace madsim_mem
