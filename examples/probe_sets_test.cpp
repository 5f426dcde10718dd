// examples/probe_sets_test.cpp — WHICH COMBINATIONS OF PROBES DO THE SEEDS REACH?  Builder::probe_sets (C++ host mirror).
//
// The lossy two-pair ping-pong of probe_census_test.cpp: each pair's client traces 0x10 + pair when it starts its loop and 0x20 + pair when
// the loop completes; a lost packet leaves a pair waiting for ever and the seed deadlocks.  The census counts the seeds behind each probe, one
// probe at a time: "0x20 fired in these many seeds, so many of them deadlock".  Failures are conjunctions, and a table of marginals cannot
// state one.  probe_sets reduces every seed's observations to a set word over the vocabulary on the device and reports each distinct set
// with its per-verdict seed counts and a seed to replay: here the seed passes exactly when 0x20 and 0x21 are both reached.  From the same
// table comes the cover: a few seeds that between them reach every probe that is reached at all — a corpus for over_seeds().
//
// Run:  MADSIM_TEST_SEED=0 MADSIM_TEST_NUM=2000 ./probe_sets_test
#include <cstdio>
#include <string>

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
        b.config.packet_loss_rate = 0.02;
        const std::vector<uint64_t> vocabulary = {0x10, 0x11, 0x20, 0x21, 0x30};
        auto p = b.probe_sets(wl.build(), vocabulary);
        const madsim_probe_sets_t& t = p.totals;
        std::printf("test lossy_ping_pong: %llu seeds from %llu: %llu pass, %llu panic, %llu deadlock, %llu time-limit; %llu probe sets\n",
                    (unsigned long long)b.count, (unsigned long long)b.seed, (unsigned long long)t.n_counted[0], (unsigned long long)t.n_counted[1],
                    (unsigned long long)t.n_counted[2], (unsigned long long)t.n_counted[3], (unsigned long long)p.sets.size());
        static const char* const verdict[4] = {"pass", "panic", "deadlock", "time-limit"};
        uint64_t sum[4] = {0, 0, 0, 0};
        for (const madsim_probe_set_t& e : p.sets) {
            std::string names;
            for (size_t i = 0; i < vocabulary.size(); i++)
                if ((e.set >> i) & 1) { char buf[24]; std::snprintf(buf, sizeof buf, " 0x%llx", (unsigned long long)vocabulary[i]); names += buf; }
            if (e.set & MADSIM_PROBE_SET_OTHER) names += " other";
            if (e.set & MADSIM_PROBE_SET_TRUNCATED) names += " truncated";
            std::printf("  set {%s }: %llu pass, %llu panic, %llu deadlock, %llu time-limit seeds;", names.c_str(), (unsigned long long)e.n_seeds[0],
                        (unsigned long long)e.n_seeds[1], (unsigned long long)e.n_seeds[2], (unsigned long long)e.n_seeds[3]);
            for (int k = 0; k < 4; k++) {
                if (e.n_seeds[k]) std::printf(" a %s at MADSIM_TEST_SEED=%llu", verdict[k], (unsigned long long)e.first_seed[k]);
                sum[k] += e.n_seeds[k];
            }
            std::printf("\n");
        }
        const uint64_t both_pass = p.count({0x20, 0x21}, {}, 0x1), both_fail = p.count({0x20, 0x21}, {}, 0xe);
        if (both_pass == t.n_counted[0] && both_fail == 0)
            std::printf("  passes exactly when 0x20 and 0x21 are both reached (%llu seeds; none of the %llu failing seeds reaches both)\n",
                        (unsigned long long)both_pass, (unsigned long long)(t.n_counted[1] + t.n_counted[2] + t.n_counted[3]));
        else
            std::printf("  0x20 and 0x21 both reached: %llu passing and %llu failing seeds, of %llu passing seeds\n", (unsigned long long)both_pass,
                        (unsigned long long)both_fail, (unsigned long long)t.n_counted[0]);
        for (const auto& x : p.mixed())
            std::printf("  set 0x%llx does not separate: passes at MADSIM_TEST_SEED=%llu, fails at MADSIM_TEST_SEED=%llu\n", (unsigned long long)x.set,
                        (unsigned long long)x.pass_seed, (unsigned long long)x.fail_seed);
        std::printf("  cover:");
        for (uint64_t s : p.cover()) std::printf(" %llu", (unsigned long long)s);
        std::printf("\n");
        if (t.n_runner) std::printf("  ... and %llu seeds left with a runner verdict\n", (unsigned long long)t.n_runner);
        for (int k = 0; k < 4; k++)
            if (sum[k] != t.n_counted[k]) { std::fprintf(stderr, "error: the sets' seeds do not add up to the counted seeds\n"); return 2; }
        return 0;          // (a report, not a verdict)
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
}
