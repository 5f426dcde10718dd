// examples/probe_census_test.cpp — DID THE INTERESTING THING EVER HAPPEN?  Builder::census (C++ host mirror).
//
// The lossy two-pair ping-pong of failure_modes_test.cpp with probes: each pair's client traces 0x10 + pair when it starts its loop and
// 0x20 + pair when the loop completes; neither side retries, so a lost packet leaves a pair waiting for ever and the seed deadlocks.  A green
// campaign says nothing about whether the test body ever went where its author feared.  The census runs the range on the trace build and
// reduces what the seeds traced on the device: per probe, how many seeds of each verdict reached it, how often, and the smallest seed that
// did — and, against a list of the probes the author expects, the ones that never fired: FoundationDB's code-probe report, the
// "sometimes" assertion of deterministic simulation testing.  0x30 stands for a branch this body cannot take.
//
// Run:  MADSIM_TEST_SEED=5000000 MADSIM_TEST_NUM=40000 ./probe_census_test
#include <cstdio>

#include "../include/madsim_hip.hpp"

int main() {
    using namespace std::chrono_literals;
    constexpr uint32_t PING = 0x676E6970, PONG = 0x676E6F70, R = 16;
    madsim::WorkloadBuilder wl;
    std::vector<madsim::Task*> tasks;
    for (uint32_t pair = 0; pair < 2; pair++) {
        int n1 = wl.create_node(), n2 = wl.create_node();
        int a1 = wl.addr(n1, 1), a2 = wl.addr(n2, 1);
        madsim::Task& t1 = wl.task(n1);
        t1.bind(a1).sleep(1s).trace(0x10 + pair).set(0, R);
        int top1 = t1.label();
        t1.send_to(a1, a2, 1, PING).recv_from(a1, 1).assert_val(PONG).djnz(0, top1).trace(0x20 + pair).done();
        madsim::Task& t2 = wl.task(n2);
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

    try {
        auto b = madsim::runtime::Builder::from_env();
        b.config.packet_loss_rate = 0.002;
        const std::vector<uint64_t> expected = {0x10, 0x11, 0x20, 0x21, 0x30};
        auto c = b.census(wl.build());
        const madsim_census_t& t = c.totals;
        std::printf("test lossy_ping_pong: %llu seeds from %llu: %llu pass, %llu panic, %llu deadlock, %llu time-limit; %llu silent, %llu probes\n",
                    (unsigned long long)b.count, (unsigned long long)b.seed, (unsigned long long)t.n_counted[0], (unsigned long long)t.n_counted[1],
                    (unsigned long long)t.n_counted[2], (unsigned long long)t.n_counted[3],
                    (unsigned long long)(t.n_silent[0] + t.n_silent[1] + t.n_silent[2] + t.n_silent[3]), (unsigned long long)c.values.size());
        for (const madsim_census_value_t& e : c.values)
            std::printf("  probe 0x%llx: %llu pass, %llu panic, %llu deadlock, %llu time-limit seeds, %llu times, first at MADSIM_TEST_SEED=%llu\n",
                        (unsigned long long)e.value, (unsigned long long)e.n_seeds[0], (unsigned long long)e.n_seeds[1], (unsigned long long)e.n_seeds[2],
                        (unsigned long long)e.n_seeds[3], (unsigned long long)e.n_total, (unsigned long long)e.first_seed);
        for (uint64_t v : c.never(expected)) std::printf("  probe 0x%llx never fired\n", (unsigned long long)v);
        if (t.n_runner) std::printf("  ... and %llu seeds left with a runner verdict\n", (unsigned long long)t.n_runner);
        uint64_t sum = 0;
        for (const madsim_census_value_t& e : c.values) sum += e.n_total;
        if (sum != t.n_observations) { std::fprintf(stderr, "error: the occurrences do not add up to the observations\n"); return 2; }
        return 0;          // (a report, not a verdict)
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
}
