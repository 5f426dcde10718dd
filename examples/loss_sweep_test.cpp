// examples/loss_sweep_test.cpp — one test body under four packet-loss rates in ONE campaign: Builder::sweep (C++ host mirror).
//
// The ping-pong test of triage_test.cpp (4 nodes: two pairs, nobody retries) at loss 0, 0.0005, 0.002 and 0.01.  Three differential
// campaigns would run the lossless side three times and still could not say which seeds fail at 0.002 and not at 0.01.  A sweep campaign
// runs the four variants of every batch back to back and classifies each seed across all of them on the device: the failures per rate,
// the seeds per SET of failing rates (bit v of a mask = rate v), whether those sets nest — a threshold bug: a seed that fails at one
// rate fails at every higher one — and the first few seeds the rates disagree on, with their verdict under each rate.
//
// Run:  MADSIM_TEST_SEED=5000000 MADSIM_TEST_NUM=10000 ./loss_sweep_test
#include <cstdio>

#include "../include/madsim_hip.hpp"

int main() {
    using namespace std::chrono_literals;
    constexpr uint32_t PING = 0x676E6970, PONG = 0x676E6F70, R = 16;
    static const char* const names[8] = {"pass", "panic", "deadlock", "time-limit", "resource-overflow", "step-limit",
                                         "outside-the-workload-model", "internal-invariant"};
    static const double rates[4] = {0.0, 0.0005, 0.002, 0.01};
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
        const madsim::Workload body = wl.build();
        const auto b = madsim::runtime::Builder::from_env();
        std::vector<madsim::runtime::Builder> under(4, b);             // the same builder, one loss rate each
        std::vector<std::pair<const madsim::runtime::Builder*, const madsim::Workload*>> variants;
        for (size_t v = 0; v < 4; v++) {
            under[v].config.packet_loss_rate = rates[v];
            variants.push_back({&under[v], &body});
        }
        const auto s = b.sweep(variants, MADSIM_DIFF_VERDICT, MADSIM_SWEEP_LIST_MIXED, 8);
        std::printf("test loss_sweep: %llu seeds from %llu under loss 0 / 0.0005 / 0.002 / 0.01, %llu incomparable\n",
                    (unsigned long long)s.campaigns[0].seeds_run, (unsigned long long)b.seed, (unsigned long long)s.report.n_incomparable);
        std::printf("  failures per rate:");
        for (unsigned v = 0; v < 4; v++) std::printf(" %llu", (unsigned long long)s.fails(v));
        std::printf("\n");
        for (unsigned mask = 0; mask < 16; mask++)
            if (s.report.n_by_mask[mask])
                std::printf("  fails at {%s%s%s%s }: %llu seeds (mask %u)\n", mask & 1 ? " 0" : "", mask & 2 ? " 0.0005" : "", mask & 4 ? " 0.002" : "",
                            mask & 8 ? " 0.01" : "", (unsigned long long)s.report.n_by_mask[mask], mask);
        std::printf("  the failing sets nest: %s\n", s.nested() ? "yes" : "no");
        for (const madsim_sweep_record_t& r : s.records)
            std::printf("  seed %llu: %s / %s / %s / %s\n", (unsigned long long)r.seed, names[r.verdict[0] & 7], names[r.verdict[1] & 7], names[r.verdict[2] & 7],
                        names[r.verdict[3] & 7]);
        if (s.report.n_selected > s.records.size()) std::printf("  ... and %llu more\n", (unsigned long long)(s.report.n_selected - s.records.size()));
        return s.fails(0) ? 101 : 0;                                   // cargo test's exit code for a failed test: the lossless run must pass
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
}
