// examples/stall_test.cpp — which task is waiting, and on what: Builder::stall_census and Builder::post_mortem (C++ host mirror).
//
// The lossy two-pair ping-pong of failure_modes_test.cpp.  Neither side retries, so a lost packet leaves a pair waiting for ever and the
// seed deadlocks.  failure_modes_test tells the modes apart by what the test body traced; this one needs no probe: the trace builds keep
// every task that is still alive when a run ends, stall_census folds those task tables over the whole range on the device — one SHAPE per
// distinct multiset of (state, program, instruction) — and post_mortem replays the seed that stands for a shape, task by task.
//
// Run:  MADSIM_TEST_SEED=5000000 MADSIM_TEST_NUM=20000 ./stall_test
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
        const madsim::Workload w = wl.build();
        const auto sc = b.stall_census(w, 32, 4096, 4096, 1u << MADSIM_DEADLOCK);
        const unsigned long long dead = sc.totals.n_counted[MADSIM_DEADLOCK];
        std::printf("test lossy_ping_pong: %llu of %llu seeds deadlock, in %zu shapes over %zu sites\n", dead, (unsigned long long)b.count,
                    sc.shapes.size(), sc.sites.size());
        for (const madsim_census_value_t& s : sc.shapes_of(MADSIM_DEADLOCK)) {
            std::printf("shape %016llx seeds %llu replay seed %llu\n", (unsigned long long)s.value, (unsigned long long)s.n_seeds[MADSIM_DEADLOCK],
                        (unsigned long long)s.first_seed);
            const auto pm = b.post_mortem(w, {s.first_seed}).front();
            if (pm.shape() != s.value) { std::fprintf(stderr, "error: seed %llu does not replay its shape\n", (unsigned long long)s.first_seed); return 2; }
            for (uint64_t t : pm.tasks)
                std::printf("    %s, loop registers %u / %u\n", madsim::runtime::Builder::describe(w, t).c_str(), MADSIM_TASK_CNT0(t), MADSIM_TASK_CNT1(t));
        }
        return dead ? 101 : 0;          // cargo test's exit code for a failed test
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
}
