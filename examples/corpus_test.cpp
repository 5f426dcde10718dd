// examples/corpus_test.cpp — "did the fix fix all of them?" over exactly the seeds that failed: Builder::over_seeds (C++ host mirror).
//
// fix_check_test.cpp diffs the whole range again to look at the seeds that failed.  For a rare failure that is a hundred million passing
// seeds re-run to look at a hundred.  Here the two steps a user takes are kept apart:
//   1. a collecting campaign (search_failures) over the range of the lossy two-pair ping-pong yields its failing seeds;
//   2. diff_against over EXACTLY those seeds — the list campaign, madsim_hip_run_seeds_campaign_diff — against the body with a timeout and
//      a resend.  The list a collecting campaign returns ascends strictly already, which is what a list campaign asks for.
// The same second step is how a regression corpus (every seed that ever failed in CI) is re-run on every commit.
//
// Run:  MADSIM_TEST_SEED=5000000 MADSIM_TEST_NUM=40000 ./corpus_test
#include <cstdio>

#include "../include/madsim_hip.hpp"

namespace {
constexpr uint32_t PING = 0x676E6970, PONG = 0x676E6F70, R = 16;

// the two bodies of fix_check_test.cpp
madsim::Workload body(bool fixed) {
    using namespace std::chrono_literals;
    madsim::WorkloadBuilder wl;
    std::vector<madsim::Task*> tasks;
    for (uint32_t pair = 0; pair < 2; pair++) {
        int n1 = wl.create_node(), n2 = wl.create_node();
        int a1 = wl.addr(n1, 1), a2 = wl.addr(n2, 1);
        madsim::Task& t1 = wl.task(n1);
        madsim::Task& t2 = wl.task(n2);
        t1.bind(a1).sleep(1s).set(0, R);
        t2.bind(a2);
        if (!fixed) {
            int top1 = t1.label();
            t1.send_to(a1, a2, 1, PING).recv_from(a1, 1).assert_val(PONG).djnz(0, top1).done();
            t2.set(0, R);
            int top2 = t2.label();
            t2.recv_from(a2, 1).assert_val(PING).reply(a2, 1, PONG).djnz(0, top2).done();
        } else {
            int top1 = t1.label();                                  // a round: ping until a pong comes back within 100 ms
            t1.send_to(a1, a2, 1, PING).recv_from_timeout(a1, 1, 100ms).jeq(MADSIM_VAL_TIMEOUT, top1).assert_val(PONG).djnz(0, top1).done();
            int top2 = t2.label();                                  // answer every ping (a repeated one too), leave after 5 s of silence
            int out2 = top2 + 5;
            t2.recv_from_timeout(a2, 1, 5s).jeq(MADSIM_VAL_TIMEOUT, out2).assert_val(PING).reply(a2, 1, PONG).jmp(top2).done();
        }
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
    try {
        auto b = madsim::runtime::Builder::from_env();
        b.config.packet_loss_rate = 0.002;
        b.capacities.heap_spill_slots = 128;                       // (the fixed body's timers: see fix_check_test.cpp)
        b.capacities.mbox_regs = 8;
        b.capacities.mbox_msgs = 4;
        // 1. which seeds of the range fail with the body as it is
        auto found = b.search_failures(body(false), (size_t)b.count);
        std::vector<uint64_t> corpus;
        for (const madsim_failure_t& f : found.failures) corpus.push_back(f.seed);
        std::printf("test lossy_ping_pong: %llu seeds from %llu, %zu fail\n", (unsigned long long)found.campaign.seeds_run, (unsigned long long)b.seed,
                    corpus.size());
        // 2. the fix, over exactly those seeds
        b.over_seeds(corpus);
        auto d = b.diff_against(b, body(false), body(true), MADSIM_DIFF_VERDICT, 8);
        uint64_t still = 0;                                        // failed before, and does not pass now
        for (int va = 1; va < 8; va++)
            for (int vb = 1; vb < 8; vb++) still += d.report.transitions[va][vb];
        uint64_t fixed = 0;
        for (int va = 1; va < 8; va++) fixed += d.report.transitions[va][MADSIM_PASS];
        const uint64_t broken = d.regressions();                   // passed before (none of the corpus did), fails now
        std::printf("  %llu of %zu fixed, %llu broken\n", (unsigned long long)fixed, corpus.size(), (unsigned long long)broken);
        std::printf("  seeds run: %llu to find them, %llu per side to check the fix\n", (unsigned long long)found.campaign.seeds_run,
                    (unsigned long long)d.a.seeds_run);
        for (const madsim_diff_record_t& r : d.records)
            std::printf("  seed %llu: verdict %u -> %u\n", (unsigned long long)r.seed, r.a.verdict, r.b.verdict);
        if (d.a.seeds_run != corpus.size() || d.a.n_failed != corpus.size()) {
            std::printf("  the list campaign did not run the corpus: %llu seeds, %llu failing on the old body\n", (unsigned long long)d.a.seeds_run,
                        (unsigned long long)d.a.n_failed);
            return 101;
        }
        return (still || broken) ? 101 : 0;                        // cargo test's exit code for a failed test
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
}
