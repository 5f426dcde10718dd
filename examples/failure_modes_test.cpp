// examples/failure_modes_test.cpp — how many DIFFERENT failures a range holds: Builder::failure_groups (C++ host mirror).
//
// The lossy two-pair ping-pong of triage_test.cpp, with one addition: each pair's client traces its pair number when its loop
// completes.  Neither side retries, so a lost packet leaves a pair waiting for ever and the seed deadlocks — in one of three ways,
// and obs_hash (FNV-1a over the traced values) tells them apart: pair 0 stuck (only 1 was traced), pair 1 stuck (only 0), both stuck
// (nothing was traced: the FNV offset basis).  triage_test lists the 32 smallest failing seeds; this one says there are three
// failures, how many seeds each has, and which seed replays each (MADSIM_TEST_SEED=<seed>).
//
// Run:  MADSIM_TEST_SEED=5000000 MADSIM_TEST_NUM=40000 ./failure_modes_test
#include <cstdio>

#include "../include/madsim_hip.hpp"

namespace {
uint64_t fnv1a(std::initializer_list<uint32_t> traced) {          // obs_hash: one FNV-1a step per traced value, in execution order
    uint64_t h = 0xCBF29CE484222325ull;
    for (uint32_t v : traced) h = (h ^ v) * 0x100000001B3ull;
    return h;
}
}  // namespace

int main() {
    using namespace std::chrono_literals;
    constexpr uint32_t PING = 0x676E6970, PONG = 0x676E6F70, R = 16;
    static const char* const names[8] = {"pass", "panic", "deadlock", "time-limit", "resource-overflow", "step-limit",
                                         "outside-the-workload-model", "internal-invariant"};
    madsim::WorkloadBuilder wl;
    std::vector<madsim::Task*> tasks;
    for (uint32_t pair = 0; pair < 2; pair++) {
        int n1 = wl.create_node(), n2 = wl.create_node();
        int a1 = wl.addr(n1, 1), a2 = wl.addr(n2, 1);
        madsim::Task& t1 = wl.task(n1);
        t1.bind(a1).sleep(1s).set(0, R);
        int top1 = t1.label();
        t1.send_to(a1, a2, 1, PING).recv_from(a1, 1).assert_val(PONG).djnz(0, top1).trace(pair).done();
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
        auto found = b.failure_groups(wl.build(), 8);
        std::printf("test lossy_ping_pong: %llu seeds from %llu: %llu fail in %zu different ways\n", (unsigned long long)found.campaign.seeds_run,
                    (unsigned long long)b.seed, (unsigned long long)found.campaign.n_failed, found.groups.size());
        for (const madsim_group_t& g : found.groups) {
            const char* what = g.key == fnv1a({}) ? "both pairs stuck" : g.key == fnv1a({1}) ? "pair 0 stuck" : g.key == fnv1a({0}) ? "pair 1 stuck" : "?";
            std::printf("  %s, traced %016llx (%s): %llu seeds, first %llu\n", names[g.verdict & 7], (unsigned long long)g.key, what,
                        (unsigned long long)g.count, (unsigned long long)g.first_seed);
        }
        if (found.n_ungrouped) std::printf("  ... and %llu seeds in further groups\n", (unsigned long long)found.n_ungrouped);
        return found.campaign.n_failed ? 101 : 0;          // cargo test's exit code for a failed test
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
}
