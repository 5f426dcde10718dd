// The owning types of madsim_amd/csrc/device_mem.h against the fake runtime of tests/cpp/fake_hip (first on the include path): built with
// -fsanitize=address,undefined and run by tests/test_device_mem.py.  Prints one line per check; exits 1 at the first that does not hold.
#include "device_mem.h"

#include <cstdio>
#include <type_traits>
#include <utility>

using madsim_mem::DevBuf;
using madsim_mem::Event;
using madsim_mem::PinnedBuf;
using madsim_mem::Stream;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static FakeHip& H = fake_hip();

template <class B>
static int buffer_checks(long FakeHip::*live) {
    {
        B b;
        H.creating_calls = 0;
        CHECK(!b && b.p == nullptr && b.cap == 0);
        CHECK(b.room(0) == hipSuccess && !b && H.creating_calls == 0);       // nothing asked, nothing made
        H.creating_calls = 0;
        CHECK(b.room(100) == hipSuccess && b.p && b.cap == 100 && H.*live == 1);
        auto* first = b.p;
        b.p[99] = typename std::remove_reference<decltype(*b.p)>::type();   // (all 100 elements are there: AddressSanitizer watches)
        CHECK(b.room(40) == hipSuccess && b.p == first && b.cap == 100);     // a smaller request is a no-op
        CHECK(b.room(100) == hipSuccess && b.p == first && H.creating_calls == 1);
        CHECK(b.room(101) == hipSuccess && b.cap == 101 && H.*live == 1 && H.creating_calls == 2);      // grown: the old one released
        b.p[100] = typename std::remove_reference<decltype(*b.p)>::type();
        // a failed room leaves {nullptr, 0} — the old buffer is gone too —, and a later room succeeds
        H.fail_in = 1;
        CHECK(b.room(500) != hipSuccess && b.p == nullptr && b.cap == 0 && H.*live == 0);
        CHECK(b.room(10) == hipSuccess && b.p && b.cap == 10 && H.*live == 1);
        H.fail_in = 1;
        B fresh;
        CHECK(fresh.room(10) != hipSuccess && !fresh && fresh.cap == 0);
        CHECK(fresh.room(10) == hipSuccess && fresh && fresh.cap == 10 && H.*live == 2);
        // draining: only the form that names a stream synchronises, and only before a live buffer is released
        const long syncs = H.syncs;
        B idle;
        CHECK(idle.room(8, nullptr) == hipSuccess && H.syncs == syncs);       // nothing live: nothing to wait for
        CHECK(idle.room(8, nullptr) == hipSuccess && H.syncs == syncs);       // no growth
        CHECK(idle.room(9) == hipSuccess && H.syncs == syncs);                // no stream named
        CHECK(idle.room(10, nullptr) == hipSuccess && H.syncs == syncs + 1 && idle.cap == 10);
        // move: the source is left empty, the target's old buffer is released
        auto* held = b.p;
        B moved(std::move(b));
        CHECK(moved.p == held && moved.cap == 10 && b.p == nullptr && b.cap == 0);
        const long before = H.*live;
        fresh = std::move(moved);
        CHECK(fresh.p == held && moved.p == nullptr && moved.cap == 0 && H.*live == before - 1);
        B& same = fresh;
        fresh = std::move(same);                                              // (self-assignment keeps it)
        CHECK(fresh.p == held && fresh.cap == 10);
        fresh.reset();
        CHECK(!fresh && fresh.cap == 0 && H.*live == before - 2);
        fresh.reset();                                                        // a second reset releases nothing
        CHECK(H.*live == before - 2 && H.bad_frees == 0);
    }
    CHECK(H.live() == 0 && H.bad_frees == 0);                                 // the destructors released the rest, each once
    return 0;
}

static int handle_checks() {
    {
        Event e;
        Stream s;
        CHECK(!e && !s);
        H.fail_in = 1;
        CHECK(e.ensure() != hipSuccess && !e);
        CHECK(e.ensure() == hipSuccess && e && H.live_events == 1);
        hipEvent_t raw = e;
        CHECK(e.ensure() == hipSuccess && (hipEvent_t)e == raw && H.live_events == 1);      // created once
        H.fail_in = 1;
        CHECK(s.ensure() != hipSuccess && !s);
        CHECK(s.ensure() == hipSuccess && s && s.ensure() == hipSuccess && H.live_streams == 1);
        Event e2(std::move(e));
        Stream s2(std::move(s));
        CHECK(!e && !s && (hipEvent_t)e2 == raw && s2);
        Event e3;
        CHECK(e3.ensure() == hipSuccess && H.live_events == 2);
        e3 = std::move(e2);                                                   // e3's own event is destroyed
        CHECK(H.live_events == 1 && (hipEvent_t)e3 == raw && !e2);
        s2.reset(); s2.reset();
        CHECK(H.live_streams == 0);
    }
    CHECK(H.live() == 0 && H.bad_frees == 0);
    return 0;
}

// A struct shaped like madsim_hip_ctx::Flight and its groups: every resource ensured on its own, the first failure returned.
struct Group {
    static constexpr int RESOURCES = 12;
    Stream stream; Event e0, e1, done;
    DevBuf<unsigned long long> d_rep; PinnedBuf<unsigned long long> h_rep;
    DevBuf<char> d_out; PinnedBuf<char> h_out;
    struct Part {
        DevBuf<unsigned> wcnt; DevBuf<short> rec; PinnedBuf<unsigned> h_cnt; Event r0;
        hipError_t ensure(size_t n, hipStream_t s) {
            hipError_t e;
            if ((e = wcnt.room(64)) || (e = rec.room(n, s)) || (e = h_cnt.room(1)) || (e = r0.ensure())) return e;
            return hipSuccess;
        }
        bool complete(size_t n) const { return wcnt && rec && rec.cap >= n && h_cnt && r0; }
    } part;
    hipError_t ensure(size_t n) {
        hipError_t e;
        if ((e = stream.ensure()) || (e = d_rep.room(675)) || (e = h_rep.room(675)) || (e = e0.ensure()) || (e = e1.ensure()) || (e = done.ensure()) ||
            (e = d_out.room(n, stream)) || (e = h_out.room(n, stream)))
            return e;
        return part.ensure(n, stream);
    }
    bool complete(size_t n) const {
        return stream && e0 && e1 && done && d_rep && h_rep && d_out && d_out.cap >= n && h_out && h_out.cap >= n && part.complete(n);
    }
};

static int group_checks() {
    {
        Group probe;                                                          // the number of creating calls one ensure() makes
        H.creating_calls = 0;
        CHECK(probe.ensure(100) == hipSuccess && H.creating_calls == Group::RESOURCES && probe.complete(100));
        CHECK(probe.ensure(100) == hipSuccess && H.creating_calls == Group::RESOURCES);      // complete: nothing more is made
    }
    for (int k = 1; k <= Group::RESOURCES; k++) {
        {
            Group g;                                                          // the k-th creation of a fresh group fails ...
            H.fail_in = k;
            CHECK(g.ensure(100) != hipSuccess && !g.complete(100) && H.fail_in == 0);
            CHECK(g.ensure(100) == hipSuccess && g.complete(100));            // ... and the next call makes everything that is missing
            CHECK(H.live() == Group::RESOURCES);
            g = Group();                                                      // what a context's close() does
            CHECK(H.live() == 0);
        }
        CHECK(H.live() == 0 && H.bad_frees == 0);
    }
    for (int k = 1; k <= 3; k++) {                                           // the same while a complete group grows (three buffers do)
        Group g;
        CHECK(g.ensure(100) == hipSuccess);
        H.fail_in = k;
        CHECK(g.ensure(1000) != hipSuccess && !g.complete(1000));
        CHECK(g.ensure(1000) == hipSuccess && g.complete(1000) && H.live() == Group::RESOURCES);
    }
    CHECK(H.live() == 0 && H.bad_frees == 0);
    return 0;
}

int main() {
    if (buffer_checks<DevBuf<int>>(&FakeHip::live_dev)) return 1;
    printf("ok DevBuf\n");
    if (buffer_checks<PinnedBuf<double>>(&FakeHip::live_pinned)) return 1;
    printf("ok PinnedBuf\n");
    if (handle_checks()) return 1;
    printf("ok Event Stream\n");
    if (group_checks()) return 1;
    printf("ok group of %d resources, a failure at each\n", Group::RESOURCES);
    CHECK(H.live() == 0 && H.bad_frees == 0 && H.frees > 0);
    printf("ok all released once: %ld releases\n", H.frees);
    return 0;
}
