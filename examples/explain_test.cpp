// examples/explain_test.cpp — WHAT each failure mode of a range traced: Builder::failure_groups with `observe` (C++ host mirror).
//
// The lossy two-pair ping-pong of failure_modes_test.cpp: each pair's client traces its pair number when its loop completes, neither side
// retries, so a lost packet leaves a pair waiting for ever and the seed deadlocks.  failure_modes_test tells the three ways apart by
// comparing each group's key with obs_hash values it computes for itself; this one asks the library what the seeds traced.  Every
// group's smallest seed is replayed on the trace build — all of them in one launch — and comes back with the values its test body
// handed to trace(), in execution order: the output a failing #[madsim::test] prints, next to the seed that replays it.
//
// Run:  MADSIM_TEST_SEED=5000000 MADSIM_TEST_NUM=40000 ./explain_test
#include <cstdio>

#include "../include/madsim_hip.hpp"

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
        const uint32_t failing = (1u << MADSIM_PANIC) | (1u << MADSIM_DEADLOCK) | (1u << MADSIM_TIME_LIMIT);
        auto found = b.failure_groups(wl.build(), 8, failing, MADSIM_GROUP_KEY_OBS, 8);
        std::printf("test lossy_ping_pong: %llu seeds from %llu: %llu fail in %zu different ways\n", (unsigned long long)found.campaign.seeds_run,
                    (unsigned long long)b.seed, (unsigned long long)found.campaign.n_failed, found.groups.size());
        bool consistent = true;
        for (size_t i = 0; i < found.groups.size(); i++) {
            const madsim_group_t& g = found.groups[i];
            const std::vector<uint64_t>& traced = found.observations[i];
            std::printf("  %s, %llu seeds, replay with MADSIM_TEST_SEED=%llu: traced [", names[g.verdict & 7], (unsigned long long)g.count,
                        (unsigned long long)g.first_seed);
            for (size_t k = 0; k < traced.size(); k++) std::printf("%s%llu", k ? ", " : "", (unsigned long long)traced[k]);
            // the pairs whose number is missing from the list never finished their loop
            bool done[2] = {false, false};
            for (uint64_t v : traced) if (v < 2) done[v] = true;
            std::printf("] (%s)\n", !done[0] && !done[1] ? "both pairs stuck" : !done[0] ? "pair 0 stuck" : !done[1] ? "pair 1 stuck" : "both pairs finished");
            consistent &= madsim::runtime::Builder::fold_observations(traced) == g.key;      // the list IS the key, spelled out
        }
        if (found.n_ungrouped) std::printf("  ... and %llu seeds in further groups\n", (unsigned long long)found.n_ungrouped);
        if (!consistent) { std::fprintf(stderr, "error: a group's observations do not fold to its key\n"); return 2; }
        return 0;          // (a report, not a verdict: failure_modes_test.cpp is the one that exits like a failed cargo test)
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
}
