// examples/diverge_test.cpp — "up to where are the old and the new run the same run?": Builder::diverge_against (C++ host mirror).
//
// fix_check_test.cpp says how many seeds a fix changed, corpus_test.cpp checks the fix over exactly the seeds that failed.  Both stop one
// step short of the question a test author asks next: at which draw and at which observation do the two runs of a changed seed part, and
// what did each side see there?  Here:
//   1. a differential campaign over the range (diff_against with a list) yields the seeds whose verdict the fix changed;
//   2. ONE diverge_against over the listed seeds — madsim_hip_diverge_seeds: both sides replayed on the trace build, their determinism logs
//      and observation logs compared on the device — prints per seed the draw at which the logs part, the last observations both runs
//      share and what each side observed next.  No log travels to the host.
//
// Run:  MADSIM_TEST_SEED=5000000 MADSIM_TEST_NUM=4096 ./diverge_test
#include <cstdio>
#include <string>

#include "../include/madsim_hip.hpp"

namespace {
constexpr uint32_t PING = 0x676E6970, PONG = 0x676E6F70, R = 16;

// the two bodies of fix_check_test.cpp, each client tracing its pair number when its loop completes
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
            t1.send_to(a1, a2, 1, PING).recv_from(a1, 1).assert_val(PONG).djnz(0, top1).trace(pair).done();
            t2.set(0, R);
            int top2 = t2.label();
            t2.recv_from(a2, 1).assert_val(PING).reply(a2, 1, PONG).djnz(0, top2).done();
        } else {
            int top1 = t1.label();                                  // a round: ping until a pong comes back within 100 ms
            t1.send_to(a1, a2, 1, PING).recv_from_timeout(a1, 1, 100ms).jeq(MADSIM_VAL_TIMEOUT, top1).assert_val(PONG).djnz(0, top1).trace(pair).done();
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

const char* status_name(uint32_t s) {
    static const char* const names[] = {"same", "differ", "prefix", "beyond-cap", "incomparable"};
    return s < 5 ? names[s] : "?";
}

std::string list(const std::vector<uint64_t>& v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); i++) s += (i ? ", " : "") + std::to_string(v[i]);
    return s + "]";
}
}  // namespace

int main() {
    try {
        auto b = madsim::runtime::Builder::from_env();
        b.config.packet_loss_rate = 0.002;
        b.capacities.heap_spill_slots = 128;                       // (the fixed body's timers: see fix_check_test.cpp)
        b.capacities.mbox_regs = 8;
        b.capacities.mbox_msgs = 4;
        // 1. which seeds of the range the fix changed
        auto d = b.diff_against(b, body(false), body(true), MADSIM_DIFF_VERDICT, 8);
        std::vector<uint64_t> seeds;
        for (const madsim_diff_record_t& r : d.records) seeds.push_back(r.seed);
        std::printf("test lossy_ping_pong: %llu seeds from %llu, the fix changes %llu, %zu listed\n", (unsigned long long)d.a.seeds_run,
                    (unsigned long long)b.seed, (unsigned long long)d.report.n_differ, seeds.size());
        // 2. up to where the two runs of each listed seed are the same run
        auto parts = b.diverge_against(b, seeds, body(false), body(true), 4096, 8, 4);
        int bad = 0;
        for (const auto& p : parts) {
            const madsim_divergence_t& r = p.rec;
            std::printf("  seed %llu: log %s at draw %llu of %llu / %llu (byte %u / %u); observations %s at %llu: shared %s, then old %s, new %s\n",
                        (unsigned long long)r.seed, status_name(r.log_status), (unsigned long long)r.log_at, (unsigned long long)r.log_len_a,
                        (unsigned long long)r.log_len_b, r.log_a, r.log_b, status_name(r.obs_status), (unsigned long long)r.obs_at, list(p.shared).c_str(),
                        list(p.next_a).c_str(), list(p.next_b).c_str());
            if (r.log_status == MADSIM_DIVERGE_INCOMPARABLE || r.log_status == MADSIM_DIVERGE_SAME) bad++;      // a changed seed's runs do part
        }
        return bad ? 101 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
}
