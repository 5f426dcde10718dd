// examples/fix_check_test.cpp — "did my fix work, and did it break anything?": Builder::diff_against (C++ host mirror).
//
// Side A is the lossy two-pair ping-pong of triage_test.cpp: neither side retries, so a lost packet leaves a pair waiting for ever and
// the seed deadlocks.  Side B is the same body with the fix: the client wraps its recv in a timeout and sends the ping again when it
// expires; the server answers every ping it gets and leaves after five seconds of silence instead of counting rounds.
// Both run over the same seeds at the campaign's rate and are compared on the device on the verdict alone (the fix changes every
// other number of a seed that lost a packet).  What comes back is the 8 x 8 matrix of verdict transitions: "deadlock -> pass: N" seeds
// were fixed, "pass -> pass: M" stayed, and no seed that passed may fail now: every other cell of the PASS row must be zero.
//
// Run:  MADSIM_TEST_SEED=5000000 MADSIM_TEST_NUM=40000 ./fix_check_test
#include <cstdio>

#include "../include/madsim_hip.hpp"

namespace {
constexpr uint32_t PING = 0x676E6970, PONG = 0x676E6F70, R = 16;

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
    static const char* const names[8] = {"pass", "panic", "deadlock", "time-limit", "resource-overflow", "step-limit",
                                         "outside-the-workload-model", "internal-invariant"};
    try {
        auto b = madsim::runtime::Builder::from_env();
        b.config.packet_loss_rate = 0.002;
        // a campaign does not re-run a seed that outgrew a device capacity, so the capacities are given: a receive that beat its timeout
        // leaves the timer in the heap until it is due (sixteen 5 s timers per server), a timed-out one its registration until the next delivery
        b.capacities.heap_spill_slots = 128;
        b.capacities.mbox_regs = 8;
        b.capacities.mbox_msgs = 4;
        auto d = b.diff_against(b, body(false), body(true), MADSIM_DIFF_VERDICT, 8);
        std::printf("test lossy_ping_pong, before and after the retry: %llu seeds from %llu, %llu changed verdict\n",
                    (unsigned long long)d.a.seeds_run, (unsigned long long)b.seed, (unsigned long long)d.report.n_differ);
        for (int va = 0; va < 8; va++)
            for (int vb = 0; vb < 8; vb++)
                if (d.report.transitions[va][vb])
                    std::printf("  %s -> %s: %llu\n", names[va], names[vb], (unsigned long long)d.report.transitions[va][vb]);
        for (const madsim_diff_record_t& r : d.records)
            std::printf("  seed %llu: %s after %llu ns -> %s after %llu ns\n", (unsigned long long)r.seed, names[r.a.verdict & 7],
                        (unsigned long long)r.a.clock_ns, names[r.b.verdict & 7], (unsigned long long)r.b.clock_ns);
        if (d.report.n_incomparable) std::printf("  (%llu seeds carry a runner verdict on one side: not compared)\n", (unsigned long long)d.report.n_incomparable);
        // the fix must not break a seed: nothing that passed before may carry another verdict now
        const uint64_t broken = d.regressions();
        if (broken) std::printf("  %llu seeds that passed fail with the fix\n", (unsigned long long)broken);
        return broken ? 101 : 0;                               // cargo test's exit code for a failed test
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
}
