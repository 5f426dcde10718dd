// examples/latency_shift_test.cpp — "what did my change do to each seed's numbers?": Builder::paired_against (C++ host mirror).
//
// The four-node ping-pong (two pairs, sixteen rounds each) under the default send latency of 1 .. 10 ms (side A) and under 2 .. 10 ms
// (side B), over the same seeds.  Every seed passes on both sides, so a differential campaign can only say "clock_ns differs in nearly
// every seed", and two statistics campaigns give two histograms whose buckets are wider than the shift.  The paired campaign pairs the
// two runs of each seed on the device: per metric how many seeds went up, down or stayed, the exact mean shift of the virtual time at
// which the test ends, and the three seeds that regressed most, each with both sides' values.
//
// Run:  MADSIM_TEST_SEED=1000 MADSIM_TEST_NUM=10000 ./latency_shift_test
#include <cstdio>

#include "../include/madsim_hip.hpp"

namespace {
constexpr uint32_t PING = 0x676E6970, PONG = 0x676E6F70, R = 16;

madsim::Workload body() {
    using namespace std::chrono_literals;
    madsim::WorkloadBuilder wl;
    std::vector<madsim::Task*> tasks;
    for (uint32_t pair = 0; pair < 2; pair++) {
        int n1 = wl.create_node(), n2 = wl.create_node();
        int a1 = wl.addr(n1, 1), a2 = wl.addr(n2, 1);
        madsim::Task& t1 = wl.task(n1);
        madsim::Task& t2 = wl.task(n2);
        t1.bind(a1).sleep(1s).set(0, R);
        int top1 = t1.label();
        t1.send_to(a1, a2, 1, PING).recv_from(a1, 1).assert_val(PONG).djnz(0, top1).done();
        t2.bind(a2).set(0, R);
        int top2 = t2.label();
        t2.recv_from(a2, 1).assert_val(PING).reply(a2, 1, PONG).djnz(0, top2).done();
        tasks.push_back(&t1);
        tasks.push_back(&t2);
    }
    madsim::Task& m = wl.main();
    for (madsim::Task* t : tasks) m.spawn(*t);
    for (madsim::Task* t : tasks) m.join(*t);
    m.done();
    return wl.build();
}
}  // namespace

int main() {
    static const char* const metrics[4] = {"clock_ns", "steps", "msg_count", "rng_calls"};
    try {
        auto a = madsim::runtime::Builder::from_env();
        auto b = a;
        b.config.send_latency_start_ns = 2000000;              // 2 .. 10 ms where side A has 1 .. 10 ms
        b.config.send_latency_end_ns = 10000000;
        auto p = a.paired_against(b, body(), 1u << MADSIM_PASS, 0, 3);
        std::printf("test ping_pong, send latency 1..10 ms against 2..10 ms: %llu seeds from %llu, %llu paired, %llu unpaired, %llu incomparable\n",
                    (unsigned long long)p.a.seeds_run, (unsigned long long)a.seed, (unsigned long long)p.report.n_paired,
                    (unsigned long long)p.report.n_unpaired, (unsigned long long)p.report.n_incomparable);
        for (uint32_t m = 0; m < MADSIM_STAT_METRICS; m++)
            std::printf("  %-9s up %llu, down %llu, equal %llu\n", metrics[m], (unsigned long long)p.report.n[2 * m + MADSIM_PAIRED_UP],
                        (unsigned long long)p.report.n[2 * m + MADSIM_PAIRED_DOWN], (unsigned long long)p.report.n_equal[m]);
        std::printf("  mean shift of clock_ns: %+.1f ns\n", p.mean_delta(MADSIM_STAT_CLOCK));
        for (const madsim_paired_extreme_t& e : p.regressions(MADSIM_STAT_CLOCK))
            std::printf("  seed %llu: %llu ns -> %llu ns (+%llu)\n", (unsigned long long)e.seed, (unsigned long long)e.a, (unsigned long long)e.b,
                        (unsigned long long)(e.b - e.a));
        // every seed must still pass on both sides, and each metric's three counts must account for every paired seed
        bool ok = p.report.n_paired == p.a.seeds_run && p.a.n_failed == 0 && p.b.n_failed == 0;
        for (uint32_t m = 0; m < MADSIM_STAT_METRICS; m++) ok = ok && p.report.n[2 * m] + p.report.n[2 * m + 1] + p.report.n_equal[m] == p.report.n_paired;
        return ok ? 0 : 101;                                   // cargo test's exit code for a failed test
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
}
