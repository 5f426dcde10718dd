// examples/triage_test.cpp — which seeds of a range fail, and how: Builder::search_failures (C++ host mirror).
//
// The ping-pong test of pingpong_test.cpp on a lossy network (4 nodes: two pairs).  Neither side retries, so a lost packet leaves
// both tasks of a pair waiting: "no events, all tasks will block forever" — the reference's Builder::run would stop at the first
// such seed.  A search over many seeds wants the list instead: the whole range runs at the campaign's rate, the smallest failing
// seeds come back with their results (ready for MADSIM_TEST_SEED=<seed> or madsim_hip_trace_seed), and every seed is counted by
// verdict.
//
// Run:  MADSIM_TEST_SEED=5000000 MADSIM_TEST_NUM=40000 ./triage_test
#include <cstdio>

#include "../include/madsim_hip.hpp"

int main() {
    using namespace std::chrono_literals;
    constexpr uint32_t PING = 0x676E6970, PONG = 0x676E6F70, R = 16;
    static const char* const names[8] = {"pass", "panic", "deadlock", "time-limit", "resource-overflow", "step-limit",
                                         "outside-the-workload-model", "internal-invariant"};
    madsim::WorkloadBuilder wl;
    std::vector<madsim::Task*> tasks;
    for (int pair = 0; pair < 2; pair++) {
        int n1 = wl.create_node(), n2 = wl.create_node();
        int a1 = wl.addr(n1, 1), a2 = wl.addr(n2, 1);
        madsim::Task& t1 = wl.task(n1);
        t1.bind(a1).sleep(1s).set(0, R);
        int top1 = t1.label();
        t1.send_to(a1, a2, 1, PING).recv_from(a1, 1).assert_val(PONG).djnz(0, top1).done();
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
        auto found = b.search_failures(wl.build(), 32);
        std::printf("test lossy_ping_pong: %llu seeds from %llu:", (unsigned long long)found.campaign.seeds_run, (unsigned long long)b.seed);
        for (int v = 0; v < 8; v++)
            if (found.by_verdict[(size_t)v]) std::printf(" %llu %s", (unsigned long long)found.by_verdict[(size_t)v], names[v]);
        std::printf("\n");
        for (const madsim_failure_t& f : found.failures)
            std::printf("  seed %llu: %s after %u steps, %.6f simulated seconds\n", (unsigned long long)f.seed, names[f.result.verdict & 7],
                        f.result.steps, f.result.clock_ns * 1e-9);
        if (found.campaign.n_failed > found.failures.size())
            std::printf("  ... and %llu more\n", (unsigned long long)(found.campaign.n_failed - found.failures.size()));
        return found.campaign.n_failed ? 101 : 0;          // cargo test's exit code for a failed test
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
}
