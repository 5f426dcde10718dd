// examples/span_test.cpp — HOW LONG DOES THE LOOP TAKE, AND WHICH SEEDS NEVER FINISH IT?  Builder::probe_spans (C++ host mirror).
//
// The lossy two-pair ping-pong: each pair's client traces 0x10 + pair when it starts its loop, 0x30 + pair in every round and 0x20 + pair
// when the loop completes; a lost packet leaves a pair waiting for ever and the seed deadlocks.  The census says which probes the seeds
// reach and the probe order which comes first; neither says WHEN.  The trace builds keep the virtual time of every traced value, and
// probe_spans reduces, on the device, the time from the first 0x10 + pair to the first 0x20 + pair behind it over every seed: how many
// seeds close the span, the exact extremes and sum, a histogram fine enough to bound any quantile within 25 %, the slowest seed and the
// first seed that never closes it — the one to replay.
//
// Run:  MADSIM_TEST_SEED=0 MADSIM_TEST_NUM=2000 ./span_test
#include <cstdio>

#include "../include/madsim_hip.hpp"

int main() {
    using namespace std::chrono_literals;
    using madsim::runtime::Builder;
    constexpr uint32_t PING = 0x676E6970, PONG = 0x676E6F70, R = 16;
    madsim::WorkloadBuilder wl;
    std::vector<madsim::Task*> tasks;
    for (uint32_t pair = 0; pair < 2; pair++) {
        int n1 = wl.create_node(), n2 = wl.create_node();
        int a1 = wl.addr(n1, 1), a2 = wl.addr(n2, 1);
        madsim::Task& t1 = wl.task(n1);
        t1.bind(a1).sleep(1s).trace(0x10 + pair).set(0, R);
        int top1 = t1.label();
        t1.send_to(a1, a2, 1, PING).recv_from(a1, 1).assert_val(PONG).trace(0x30 + pair).djnz(0, top1).trace(0x20 + pair).done();
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
        auto b = Builder::from_env();
        b.config.packet_loss_rate = 0.004;
        auto p = b.probe_spans(wl.build(), {Builder::Span::between(0x10, 0x20), Builder::Span::between(0x11, 0x21)});
        const madsim_probe_spans_t& t = p.totals;
        std::printf("test lossy_ping_pong: %llu seeds from %llu: %llu pass, %llu panic, %llu deadlock, %llu time-limit\n", (unsigned long long)b.count,
                    (unsigned long long)b.seed, (unsigned long long)t.n_counted[0], (unsigned long long)t.n_counted[1], (unsigned long long)t.n_counted[2],
                    (unsigned long long)t.n_counted[3]);
        for (size_t pair = 0; pair < 2; pair++) {
            std::printf("  pair %zu: %llu seeds finish the loop, %llu never do", pair, (unsigned long long)p.closed(pair),
                        (unsigned long long)p.state(pair, MADSIM_SPAN_OPEN));
            if (!p.closed(pair)) { std::printf("\n"); continue; }
            const auto med = p.quantile_bounds(pair, 0.5), p99 = p.quantile_bounds(pair, 0.99);
            std::printf("; loop time median %llu..%llu ns, p99 %llu..%llu ns, slowest seed %llu (%llu ns)", (unsigned long long)med.first,
                        (unsigned long long)med.second, (unsigned long long)p99.first, (unsigned long long)p99.second,
                        (unsigned long long)*p.slowest(pair), (unsigned long long)p.spans[pair].max);
            if (auto s = p.never_closed(pair)) std::printf("; first seed that never finishes: %llu", (unsigned long long)*s);
            std::printf("\n");
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "span_test: %s\n", e.what());
        return 1;
    }
}
