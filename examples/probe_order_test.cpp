// examples/probe_order_test.cpp — WHICH PROBE COMES FIRST?  Builder::probe_order (C++ host mirror).
//
// The lossy two-pair ping-pong of probe_sets_test.cpp: each pair's client traces 0x10 + pair when it starts its loop and 0x20 + pair when
// the loop completes; a lost packet leaves a pair waiting for ever and the seed deadlocks.  The census counts the seeds behind each probe,
// the probe sets the seeds behind each combination — and every set word is symmetric in the two pairs.  The order is not: probe_order
// reduces every seed's observations on the device to the first occurrence of each vocabulary value and reports, per cell (a, b), the
// seeds of each verdict that saw a first before they first saw b, each with a seed to replay.
//
// Run:  MADSIM_TEST_SEED=0 MADSIM_TEST_NUM=2000 ./probe_order_test
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
        b.config.packet_loss_rate = 0.02;
        const std::vector<uint64_t> vocabulary = {0x10, 0x11, 0x20, 0x21, 0x30};
        auto p = b.probe_order(wl.build(), vocabulary);
        const madsim_probe_order_t& t = p.totals;
        std::printf("test lossy_ping_pong: %llu seeds from %llu: %llu pass, %llu panic, %llu deadlock, %llu time-limit; %llu cells\n",
                    (unsigned long long)b.count, (unsigned long long)b.seed, (unsigned long long)t.n_counted[0], (unsigned long long)t.n_counted[1],
                    (unsigned long long)t.n_counted[2], (unsigned long long)t.n_counted[3], (unsigned long long)p.pairs.size());
        static const char* const verdict[4] = {"pass", "panic", "deadlock", "time-limit"};
        for (int k = 0; k < 4; k++) {
            if (!t.n_counted[k]) continue;
            std::printf("  row first seen before column (diagonal: reached), %s:\n    %6s", verdict[k], "");
            for (uint64_t v : vocabulary) std::printf(" %#6llx", (unsigned long long)v);
            std::printf("\n");
            for (uint64_t a : vocabulary) {
                std::printf("    %#6llx", (unsigned long long)a);
                for (uint64_t c : vocabulary) std::printf(" %6llu", (unsigned long long)p.before(a, c, 1u << k));
                std::printf("\n");
            }
        }
        for (uint64_t a : vocabulary)
            for (uint64_t c : vocabulary)
                if (p.always_before(a, c)) std::printf("  %#llx always before %#llx (%llu seeds reached both)\n", (unsigned long long)a, (unsigned long long)c,
                                                       (unsigned long long)p.both(a, c));
        for (auto ab : {std::pair<uint64_t, uint64_t>{0x10, 0x11}, {0x11, 0x10}}) {
            const madsim_probe_order_pair_t* e = p.cell(ab.first, ab.second);
            std::printf("  %#llx before %#llx: %llu pass, %llu panic, %llu deadlock, %llu time-limit seeds;", (unsigned long long)ab.first,
                        (unsigned long long)ab.second, (unsigned long long)(e ? e->n_seeds[0] : 0), (unsigned long long)(e ? e->n_seeds[1] : 0),
                        (unsigned long long)(e ? e->n_seeds[2] : 0), (unsigned long long)(e ? e->n_seeds[3] : 0));
            for (int k = 0; e && k < 4; k++)
                if (e->n_seeds[k]) std::printf(" a %s at MADSIM_TEST_SEED=%llu", verdict[k], (unsigned long long)e->first_seed[k]);
            std::printf("\n");
        }
        if (t.n_runner) std::printf("  ... and %llu seeds left with a runner verdict\n", (unsigned long long)t.n_runner);
        for (uint64_t a : vocabulary)                                   // two values never share an index: one of them came first
            for (uint64_t c : vocabulary)
                if (a != c && p.both(a, c) > std::min(p.reached(a), p.reached(c))) { std::fprintf(stderr, "error: more seeds reached both than either\n"); return 2; }
        return 0;          // (a report, not a verdict)
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
}
