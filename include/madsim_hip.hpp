// madsim_hip.hpp — C++17 host-side mirror of madsim's seed driver over the C-ABI (include/madsim_hip.h).
//
// The reference's host code is Rust; this image has no Rust toolchain, so the host side above the C-ABI
// is written in C++ with the reference's own names and behaviour:
//   madsim::runtime::Builder            madsim/src/sim/runtime/builder.rs:7-22   (same public fields)
//   Builder::from_env()                 builder.rs:64-118                         (same environment variables)
//   Builder::run(workload)              builder.rs:121-162                        (returns on success; on the
//                                       first failing seed prints the reproduction note of
//                                       runtime/mod.rs:205-210 and throws — the C++ stand-in for the panic)
//   madsim::WorkloadBuilder / Task      the body of a #[madsim::test] as an actor program; method names are
//                                       the reference API calls they stand for (net/endpoint.rs, time/sleep.rs,
//                                       task/mod.rs, runtime/mod.rs:276-303, net/mod.rs:164-222)
// Header-only; link with libmadsim_hip.so.  There is no CPU fallback: without a GPU every run throws.
#ifndef MADSIM_HIP_HPP
#define MADSIM_HIP_HPP

#include <algorithm>
#include <array>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <optional>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "madsim_hip.h"

namespace madsim {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// A failing seed: what `cargo test` would report as the test's panic.
struct SimulationFailure : std::runtime_error {
    uint64_t seed;
    madsim_result_t result;
    SimulationFailure(uint64_t s, const madsim_result_t& r)
        : std::runtime_error("seed " + std::to_string(s) + ": " + verdict_name(r.verdict)), seed(s), result(r) {}
    static const char* verdict_name(uint32_t v) {
        static const char* n[] = {"pass", "panic", "no events, all tasks will block forever", "time limit exceeded",
                                  "device capacity overflow", "step limit", "outside the workload model", "internal invariant"};
        return v < 8 ? n[v] : "?";
    }
};

inline void check(int rc) {
    if (rc < 0) throw Error(rc, std::string(madsim_hip_strerror(rc)) + ": " + madsim_hip_last_error());
}

// madsim::Config.net (net/network.rs:66-89)
struct Config {
    double packet_loss_rate = 0.0;
    uint64_t send_latency_start_ns = 1000000, send_latency_end_ns = 10000000;
    bool buggify = false;
    // ranges Task::set_latency(i) switches to — NetSim::update_config(|c| c.send_latency = ..) (net/mod.rs:138-141); at most four {start, end} in ns
    std::vector<std::pair<uint64_t, uint64_t>> latency_table;

    // `content.parse::<Config>()` of MADSIM_TEST_CONFIG (builder.rs:81-88; config.rs:29-35 = toml::from_str): the [net] table —
    // packet_loss_rate and send_latency = { start = { secs, nanos }, end = { secs, nanos } } — in either TOML spelling (inline
    // tables as in config.rs:52-56, or [net.send_latency.start] sections as Display prints them); [tcp] is an empty struct.
    // A TOML subset on purpose: tables, inline tables, numbers, strings and booleans — what a Config file can hold.
    static Config from_toml(const std::string& text) {
        Config c;
        std::optional<uint64_t> s_secs, s_nanos, e_secs, e_nanos;
        auto set = [&](const std::string& path, const std::string& v) {
            auto num = [&]() -> double {
                char* end = nullptr; double x = std::strtod(v.c_str(), &end);
                if (v.empty() || *end) throw std::invalid_argument("failed to parse config file: `" + path + "` is not a number");
                return x;
            };
            if (path == "net.packet_loss_rate") c.packet_loss_rate = num();
            else if (path == "net.send_latency.start.secs") s_secs = (uint64_t)num();
            else if (path == "net.send_latency.start.nanos") s_nanos = (uint64_t)num();
            else if (path == "net.send_latency.end.secs") e_secs = (uint64_t)num();
            else if (path == "net.send_latency.end.nanos") e_nanos = (uint64_t)num();
            else if (path.rfind("net.", 0) == 0) throw std::invalid_argument("failed to parse config file: unknown field `" + path + "`");
            // (other tables — [tcp] — carry no fields this path reads)
        };
        size_t i = 0; const size_t n = text.size();
        auto ws = [&](bool newlines) {
            while (i < n) {
                if (text[i] == '#') { while (i < n && text[i] != '\n') i++; }
                else if (text[i] == ' ' || text[i] == '\t' || text[i] == '\r' || (newlines && text[i] == '\n')) i++;
                else break;
            }
        };
        auto key = [&]() -> std::string {              // bare or quoted key, dotted: a.b."c"
            std::string k;
            for (;;) {
                ws(false);
                if (i < n && (text[i] == '"' || text[i] == '\'')) { const char q = text[i++]; while (i < n && text[i] != q) k += text[i++]; if (i < n) i++; }
                else { const size_t b = i; while (i < n && (std::isalnum((unsigned char)text[i]) || text[i] == '_' || text[i] == '-')) i++; if (i == b) throw std::invalid_argument("failed to parse config file: key expected"); k.append(text, b, i - b); }
                ws(false);
                if (i < n && text[i] == '.') { k += '.'; i++; } else return k;
            }
        };
        std::function<void(const std::string&)> value = [&](const std::string& path) {
            ws(false);
            if (i < n && text[i] == '{') {               // inline table
                i++; ws(true);
                while (i < n && text[i] != '}') {
                    const std::string k = key();
                    if (i >= n || text[i] != '=') throw std::invalid_argument("failed to parse config file: `=` expected");
                    i++; value(path + "." + k); ws(true);
                    if (i < n && text[i] == ',') { i++; ws(true); }
                }
                if (i >= n) throw std::invalid_argument("failed to parse config file: unterminated inline table");
                i++;
            } else if (i < n && (text[i] == '"' || text[i] == '\'')) {
                const char q = text[i++]; std::string v; while (i < n && text[i] != q) v += text[i++]; if (i < n) i++;
                set(path, v);
            } else {
                const size_t b = i;
                while (i < n && text[i] != ',' && text[i] != '}' && text[i] != '\n' && text[i] != '#' && text[i] != ' ' && text[i] != '\t' && text[i] != '\r') i++;
                std::string v(text, b, i - b);
                v.erase(std::remove(v.begin(), v.end(), '_'), v.end());       // 1_000_000
                set(path, v);
            }
        };
        std::string table;
        for (ws(true); i < n; ws(true)) {
            if (text[i] == '[') {
                i++; table = key();
                if (i >= n || text[i] != ']') throw std::invalid_argument("failed to parse config file: `]` expected");
                i++;
            } else {
                const std::string k = key();
                if (i >= n || text[i] != '=') throw std::invalid_argument("failed to parse config file: `=` expected");
                i++; value(table.empty() ? k : table + "." + k);
            }
        }
        if (s_secs || s_nanos || e_secs || e_nanos) {
            if (!(s_secs && s_nanos && e_secs && e_nanos)) throw std::invalid_argument("failed to parse config file: send_latency needs start and end, secs and nanos");
            c.send_latency_start_ns = *s_secs * 1000000000ull + *s_nanos; c.send_latency_end_ns = *e_secs * 1000000000ull + *e_nanos;
        }
        return c;
    }
    madsim_config_t raw() const {
        madsim_config_t c{};
        c.packet_loss_rate = packet_loss_rate; c.lat_lo_ns = send_latency_start_ns; c.lat_hi_ns = send_latency_end_ns;
        c.buggify = buggify ? 1 : 0;
        if (latency_table.size() > 4) throw std::invalid_argument("at most four latency_table entries");
        c.n_lat_table = (uint32_t)latency_table.size();
        for (size_t i = 0; i < latency_table.size(); i++) { c.lat_table_lo_ns[i] = latency_table[i].first; c.lat_table_hi_ns[i] = latency_table[i].second; }
        return c;
    }
};

class WorkloadBuilder;

// One async block (`node.spawn(async move { ... })`).
class Task {
  public:
    int index() const { return index_; }
    int label() const { return (int)code_.size(); }
    Task& done() { return emit(MS_OP_DONE); }
    Task& spawn(const Task& t) { return emit(MS_OP_SPAWN, (uint8_t)t.index_); }
    Task& join(const Task& t, bool expect_err = false) { return emit(MS_OP_JOIN, (uint8_t)t.index_, expect_err ? 1 : 0); }
    Task& yield_now() { return emit(MS_OP_YIELD); }
    Task& panic(uint8_t code = 0) { return emit(MS_OP_PANIC, 0, 0, code); }            // panic!("<code>"): the message is the decimal text of `code`
    Task& panic(const std::string& message);                                           // panic!("<message>"): interned by WorkloadBuilder::build()
    Task& panic_with_flag(int flag, int32_t offset = 0) { return emit(MS_OP_PANIC, 1, (uint16_t)flag, (uint32_t)offset); }   // panic!("{}", flag + offset)
    Task& set(int reg, uint32_t v) { return emit(MS_OP_SET, (uint8_t)reg, 0, v); }
    Task& djnz(int reg, int target) { return emit(MS_OP_DJNZ, (uint8_t)reg, (uint16_t)target, 0, true); }
    Task& jmp(int target) { return emit(MS_OP_JMP, 0, (uint16_t)target, 0, true); }
    Task& trace(uint32_t v) { return emit(MS_OP_TRACE, 0, 0, v); }
    Task& sleep(std::chrono::nanoseconds d) { return dur(MS_OP_SLEEP, 0, d); }
    Task& mark() { return emit(MS_OP_MARK); }
    // time::interval(p) / interval_at(t0, p) with set_missed_tick_behavior (0 Burst, 1 Delay, 2 Skip), ticker.tick().await, ticker.reset()
    // (MS_OP_INTERVAL / MS_OP_TICK / MS_OP_INTERVAL_RESET).  tick(true) folds the instant the tick was scheduled for.
    Task& interval(std::chrono::nanoseconds p, uint8_t behavior = 0, bool at_mark = false) {
        if (p.count() <= 0 || p.count() / 1000000000 > 0xffff || behavior > 2) throw std::invalid_argument("interval: 0 < period < 65536 s, behavior 0..2");
        return emit(MS_OP_INTERVAL, (uint8_t)(behavior | (at_mark ? 4 : 0)), (uint16_t)(p.count() / 1000000000), (uint32_t)(p.count() % 1000000000));
    }
    Task& tick(bool trace = false) { return emit(MS_OP_TICK, trace ? 1 : 0); }
    Task& interval_reset() { return emit(MS_OP_INTERVAL_RESET); }
    // select! { biased; recv_from(tag), ticker.tick() } (tick_first: the tick arm first) and timeout_at(t0 + d, recv_from(tag)), t0 = this
    // program's mark() (MS_OP_RECV_OR_TICK / MS_OP_RECV_TIMEOUT_AT, ABI v7).  A won tick or an expired deadline: val = MADSIM_VAL_TIMEOUT.
    Task& recv_or_tick(int ep, uint8_t tag, bool tick_first = false, bool trace = false) {
        return emit(MS_OP_RECV_OR_TICK, (uint8_t)ep, (uint16_t)((tag << 8) | (tick_first ? 1 : 0) | (trace ? 2 : 0)));
    }
    Task& recv_from_timeout_at(int ep, uint8_t tag, std::chrono::nanoseconds d) {
        uint64_t ns = (uint64_t)d.count();
        if (ns / 1000000000ull > 0xff) throw std::invalid_argument("recv_from_timeout_at: at most 255 s");
        return emit(MS_OP_RECV_TIMEOUT_AT, (uint8_t)ep, (uint16_t)((tag << 8) | (ns / 1000000000ull)), (uint32_t)(ns % 1000000000ull));
    }
    // signal::ctrl_c().await, Handle::current().send_ctrl_c(node) and select! { biased; ctrl_c(), recv_from(tag) } (recv_first: the recv arm
    // first) — MS_OP_CTRL_C / MS_OP_SEND_CTRL_C / MS_OP_RECV_OR_CTRL_C.  A won ctrl-c arm: val = MADSIM_VAL_TIMEOUT.  Not in a workload with
    // timeout scopes, tickers, recv_or_tick or recv_from_timeout_at.
    Task& ctrl_c() { return emit(MS_OP_CTRL_C); }
    Task& send_ctrl_c(int node) { return emit(MS_OP_SEND_CTRL_C, (uint8_t)node); }
    Task& recv_or_ctrl_c(int ep, uint8_t tag, bool recv_first = false) {
        return emit(MS_OP_RECV_OR_CTRL_C, (uint8_t)ep, (uint16_t)((tag << 8) | (recv_first ? 1 : 0)));
    }
    // time::timeout(d, async { .. }) over the ops up to timeout_end(scope) (MS_OP_TIMEOUT_BEGIN / END): returns the scope handle;
    // jmp_scope_end / jeq_scope_end jump to its END before it exists (an early return, connect1's `?`).  Expired: val = MADSIM_VAL_TIMEOUT.
    int timeout_begin(std::chrono::nanoseconds d) {
        if (d.count() < 0 || d.count() / 1000000000 > 255) throw std::invalid_argument("timeout_begin: 0 .. 255 s");
        emit(MS_OP_TIMEOUT_BEGIN, (uint8_t)(d.count() / 1000000000), SCOPE_END, (uint32_t)(d.count() % 1000000000), true);
        return label() - 1;
    }
    Task& jeq_scope_end(uint32_t v, int scope) { (void)scope; return emit(MS_OP_JEQ, 0, SCOPE_END, v, true); }
    Task& jmp_scope_end(int scope) { (void)scope; return emit(MS_OP_JMP, 0, SCOPE_END, 0, true); }
    Task& timeout_end(int scope) {
        for (size_t i = (size_t)scope; i < code_.size(); i++) if (code_[i].reloc && code_[i].in.b == SCOPE_END) code_[i].in.b = (uint16_t)label();
        return emit(MS_OP_TIMEOUT_END);
    }
    Task& sleep_until(std::chrono::nanoseconds after_mark) { return dur(MS_OP_SLEEP_UNTIL, 0, after_mark); }
    Task& assert_elapsed_eq(std::chrono::nanoseconds d) { return dur(MS_OP_ASSERT_ELAPSED, 0, d); }
    Task& assert_elapsed_ge(std::chrono::nanoseconds d) { return dur(MS_OP_ASSERT_ELAPSED, 1, d); }
    Task& bind(int addr, bool port_to_val = false) { return emit(MS_OP_BIND, (uint8_t)addr, port_to_val ? 2 : 0); }   // val = local_addr().port()
    Task& try_bind(int addr) { return emit(MS_OP_BIND, (uint8_t)addr, 1); }            // val = 0 | MADSIM_VAL_ADDR_NOT_AVAILABLE | MADSIM_VAL_ADDR_IN_USE
    Task& send_to(int ep, int dst, uint8_t tag, uint32_t payload) { return emit(MS_OP_SEND, (uint8_t)ep, (uint16_t)((tag << 8) | dst), payload); }
    Task& reply(int ep, uint8_t tag, uint32_t payload) { return emit(MS_OP_REPLY, (uint8_t)ep, (uint16_t)(tag << 8), payload); }
    Task& recv_from(int ep, uint8_t tag) { return emit(MS_OP_RECV, (uint8_t)ep, (uint16_t)(tag << 8)); }
    Task& assert_val(uint32_t v) { return emit(MS_OP_ASSERT_VAL, 0, 0, v); }
    Task& close(int ep) { return emit(MS_OP_CLOSE, (uint8_t)ep); }
    // timeouts / random sleeps / branching on the received value
    Task& recv_from_timeout(int ep, uint8_t tag, std::chrono::nanoseconds d) {
        uint64_t ns = (uint64_t)d.count();
        return emit(MS_OP_RECV_TIMEOUT, (uint8_t)ep, (uint16_t)((tag << 8) | (ns / 1000000000ull)), (uint32_t)(ns % 1000000000ull));
    }
    Task& sleep_rand(std::chrono::milliseconds lo /* multiple of 50 ms */, std::chrono::nanoseconds hi) {
        uint64_t ns = (uint64_t)hi.count();
        return emit(MS_OP_SLEEP_RAND, (uint8_t)(lo.count() / 50), (uint16_t)(ns / 1000000000ull), (uint32_t)(ns % 1000000000ull));
    }
    Task& random_u32() { return emit(MS_OP_RANDOM, 0); }
    Task& getrandom_byte() { return emit(MS_OP_RANDOM, 1); }
    Task& trace_system_time() { return emit(MS_OP_TRACE_TIME, 0); }
    Task& trace_instant() { return emit(MS_OP_TRACE_TIME, 1); }
    Task& trace_val() { return emit(MS_OP_TRACE_TIME, 2); }
    Task& rand_bool(int table_index) { return emit(MS_OP_RAND_BOOL, (uint8_t)table_index); }
    Task& jeq(uint32_t value, int target) { return emit(MS_OP_JEQ, 0, (uint16_t)target, value, true); }
    // reliable channel (Endpoint::connect1 / accept1)
    Task& connect1(int ep, int dst) { return emit(MS_OP_CONNECT, (uint8_t)ep, (uint16_t)dst); }
    Task& accept1(int ep) { return emit(MS_OP_ACCEPT, (uint8_t)ep); }
    Task& chan_send(uint32_t payload) { return emit(MS_OP_CSEND, 0, 0, payload); }
    Task& chan_recv() { return emit(MS_OP_CRECV); }
    Task& chan_close() { return emit(MS_OP_CCLOSE); }
    Task& spawn_move_conn(const Task& t) { return emit(MS_OP_SPAWN, (uint8_t)t.index_, MADSIM_SPAWN_MOVE_CONN); }
    // typed RPC (Endpoint::call / call_timeout / add_rpc_handler, net/rpc.rs:96-180): req_id = R::ID - 0x80, 8-bit codes
    Task& rpc_call(int ep, int dst, uint8_t req_id, uint8_t code, std::chrono::milliseconds timeout = std::chrono::milliseconds(0)) {
        return emit(MS_OP_RPC_CALL, (uint8_t)ep, (uint16_t)(((MADSIM_TAG_RPC_FIRST + req_id) << 8) | dst), ((uint32_t)timeout.count() << 8) | code);
    }
    Task& rpc_recv(int ep, uint8_t req_id) { return emit(MS_OP_RECV, (uint8_t)ep, (uint16_t)((MADSIM_TAG_RPC_FIRST + req_id) << 8)); }
    Task& rpc_reply(int ep, uint8_t code) { return emit(MS_OP_RPC_REPLY, (uint8_t)ep, 0, code); }
    // NetSim::hook_rpc_req / hook_rpc_rsp (net/mod.rs:240-284): drop requests R leaving `node` / responses on their way to `node`
    Task& hook_rpc_req(int node, uint8_t req_id, std::optional<uint8_t> code = std::nullopt) {
        return emit(MS_OP_HOOK_REQ, (uint8_t)node, (uint16_t)(((MADSIM_TAG_RPC_FIRST + req_id) << 8) | (code ? 0 : 1)), code ? *code : 0);
    }
    Task& hook_rpc_rsp(int node, std::optional<uint8_t> code = std::nullopt) { return emit(MS_OP_HOOK_RSP, (uint8_t)node, code ? 0 : 1, code ? *code : 0); }
    // NetSim::global_ipvs() at run time (net/ipvs.rs:50-85); `service` = the index ipvs_service returned
    Task& ipvs_add_service(int service) { return emit(MS_OP_IPVS, MADSIM_IPVS_ADD_SERVICE, (uint16_t)service); }
    Task& ipvs_del_service(int service) { return emit(MS_OP_IPVS, MADSIM_IPVS_DEL_SERVICE, (uint16_t)service); }
    Task& ipvs_add_server(int service, int server) { return emit(MS_OP_IPVS, MADSIM_IPVS_ADD_SERVER, (uint16_t)service, (uint32_t)server); }
    Task& ipvs_del_server(int service, int server) { return emit(MS_OP_IPVS, MADSIM_IPVS_DEL_SERVER, (uint16_t)service, (uint32_t)server); }
    Task& spawn_move_request(const Task& t) { return emit(MS_OP_SPAWN, (uint8_t)t.index_, MADSIM_SPAWN_MOVE_REQUEST); }
    // supervisor (Handle::kill / restart / pause / resume / is_exit, JoinHandle::abort)
    Task& kill(int node) { return emit(MS_OP_KILL, (uint8_t)node); }
    Task& restart(int node) { return emit(MS_OP_RESTART, (uint8_t)node); }
    Task& pause(int node) { return emit(MS_OP_PAUSE, (uint8_t)node); }
    Task& resume(int node) { return emit(MS_OP_RESUME, (uint8_t)node); }
    Task& abort(const Task& t) { return emit(MS_OP_ABORT, (uint8_t)t.index_); }
    Task& assert_exit(int node, bool expected) { return emit(MS_OP_ASSERT_EXIT, (uint8_t)node, expected ? 1 : 0); }
    Task& build_node(int node) { return emit(MS_OP_BUILD, (uint8_t)node); }
    // shared Arc<AtomicUsize>-style flags
    Task& flag_store(int flag, uint32_t v) { return emit(MS_OP_GSET, (uint8_t)flag, 0, v); }
    Task& flag_add(int flag, uint32_t v) { return emit(MS_OP_GADD, (uint8_t)flag, 0, v); }
    Task& assert_flag(int flag, uint32_t v) { return emit(MS_OP_ASSERT_G, (uint8_t)flag, 0, v); }
    Task& panic_if_flag_lt(int flag, uint32_t v) { return emit(MS_OP_PANIC_IF_G_LT, (uint8_t)flag, 0, v); }
    Task& clog_node(int node) { return emit(MS_OP_CLOG_NODE, (uint8_t)node, 3); }
    Task& unclog_node(int node) { return emit(MS_OP_UNCLOG_NODE, (uint8_t)node, 3); }
    Task& set_latency(int index) { return emit(MS_OP_SET_LATENCY, (uint8_t)index); }   // NetSim::update_config(|c| c.send_latency = latency_table[index])
    Task& clog_link(int src, int dst) { return emit(MS_OP_CLOG_LINK, (uint8_t)src, (uint16_t)dst); }
    Task& unclog_link(int src, int dst) { return emit(MS_OP_UNCLOG_LINK, (uint8_t)src, (uint16_t)dst); }

  private:
    friend class WorkloadBuilder;
    struct Ins { madsim_insn_t in; bool reloc; std::string text; };     // text: the literal message of a panic("..")
    Task(int index, int node, uint8_t flags) : index_(index), node_(node), flags_(flags) {}
    static constexpr uint16_t SCOPE_END = 0xffff;      // (a jump to the END of the scope still open: patched by timeout_end)
    Task& emit(uint8_t op, uint8_t a = 0, uint16_t b = 0, uint32_t imm = 0, bool reloc = false) {
        code_.push_back({madsim_insn_t{op, a, b, imm}, reloc, std::string()});
        return *this;
    }
    Task& dur(uint8_t op, uint8_t a, std::chrono::nanoseconds d) {
        uint64_t ns = (uint64_t)d.count();
        return emit(op, a, (uint16_t)(ns / 1000000000ull), (uint32_t)(ns % 1000000000ull));
    }
    int index_, node_;
    uint8_t flags_;
    std::vector<Ins> code_;
};

// Owns the tables a madsim_workload_t points into.
struct Workload {
    std::vector<madsim_node_t> nodes;
    std::vector<madsim_prog_t> progs;
    std::vector<madsim_sock_t> socks;
    std::vector<madsim_insn_t> insns;
    std::vector<madsim_service_t> services;   // IPVS virtual services (net/ipvs.rs)
    std::vector<uint32_t> panic_match;        // empty, or 8 words per node: which message codes restart it (madsim_workload_t.panic_match)
    uint32_t panic_dyn_max = 0;
    madsim_workload_t raw() const {
        madsim_workload_t w{};
        w.n_nodes = (uint32_t)nodes.size() - 1; w.n_progs = (uint32_t)progs.size(); w.n_socks = (uint32_t)socks.size();
        w.n_insns = (uint32_t)insns.size(); w.nodes = nodes.data(); w.progs = progs.data(); w.socks = socks.data(); w.insns = insns.data();
        w.n_services = (uint32_t)services.size(); w.services = services.empty() ? nullptr : services.data();
        w.panic_dyn_max = panic_dyn_max; w.panic_match = panic_match.empty() ? nullptr : panic_match.data();
        return w;
    }
};

class WorkloadBuilder {
  public:
    WorkloadBuilder() { tasks_.reserve(256); nodes_.push_back(madsim_node_t{}); tasks_.push_back(Task(0, 0, 0)); }   // Task& stay valid
    Task& main() { return tasks_[0]; }                                   // the future handed to block_on
    // Byte strings on the wire never steer the simulation (a Payload is a Box<dyn Any>, endpoint.rs:69-94): the test body can
    // only compare them, so they are interned — equal bytes <=> equal value.  payload(): the 32-bit value of a datagram /
    // channel payload; rpc_message(): the 8-bit code of a typed-RPC message together with its call_with_data bytes
    // (net/rpc.rs:114-131), at most 256 distinct pairs per workload.
    uint32_t payload(const std::string& data) {
        for (size_t i = 0; i < payloads_.size(); i++) if (payloads_[i] == data) return 0x40000000u + (uint32_t)i;
        payloads_.push_back(data); return 0x40000000u + (uint32_t)payloads_.size() - 1;
    }
    uint8_t rpc_message(const std::string& msg, const std::string& data = std::string()) {
        const std::string key = std::to_string(msg.size()) + ":" + msg + data;
        for (size_t i = 0; i < rpc_messages_.size(); i++) if (rpc_messages_[i] == key) return (uint8_t)i;
        if (rpc_messages_.size() >= 256) throw std::length_error("at most 256 distinct typed-RPC (message, data) pairs");
        rpc_messages_.push_back(key); return (uint8_t)(rpc_messages_.size() - 1);
    }
    // Handle::create_node()[.ip(10.0.0.<id>)][.restart_on_panic()][.restart_on_panic_matching(code)..].build()
    int create_node(bool restart_on_panic = false, std::vector<uint8_t> restart_on_panic_matching = {}, bool ip = true) {
        if (restart_on_panic_matching.size() > 2) throw std::length_error("at most two restart_on_panic_matching patterns");
        madsim_node_t n{};
        n.flags = (uint8_t)((restart_on_panic ? MADSIM_NODE_RESTART_ON_PANIC : 0) | (ip ? 0 : MADSIM_NODE_NO_IP) |
                            (restart_on_panic_matching.empty() ? 0 : MADSIM_NODE_RESTART_MATCHING));
        n.n_match = (uint8_t)restart_on_panic_matching.size();
        for (size_t i = 0; i < restart_on_panic_matching.size(); i++) n.match[i] = restart_on_panic_matching[i];
        nodes_.push_back(n); return (int)nodes_.size() - 1;
    }
    // ...restart_on_panic_matching("pattern")...: substrings of the panic message (`error_msg.contains(s)`, task/mod.rs:297-300),
    // any number of them; build() evaluates them against every message code (literal messages, decimal texts of numbers)
    int create_node_matching(std::vector<std::string> patterns, bool ip = true) {
        madsim_node_t n{};
        n.flags = (uint8_t)(MADSIM_NODE_RESTART_MATCHING | (ip ? 0 : MADSIM_NODE_NO_IP));
        nodes_.push_back(n);
        patterns_.resize(nodes_.size());
        patterns_.back() = std::move(patterns);
        return (int)nodes_.size() - 1;
    }
    // a virtual service address that belongs to no node ("1.1.1.<ip_id>:port"): a destination only
    int virtual_addr(uint8_t ip_id, uint16_t port) { socks_.push_back(madsim_sock_t{ip_id, MADSIM_ADDR_VIRTUAL, port}); return (int)socks_.size() - 1; }
    // ipvs.add_service(ServiceAddr::Tcp(vaddr), RoundRobin) + add_server per entry (net/ipvs.rs:50-85), before any task runs
    // (absent = only the address is declared: the service exists once a task calls ipvs_add_service).  Returns the service index.
    int ipvs_service(int vaddr, const std::vector<int>& servers = {}, bool absent = false) {
        if (services_.size() >= MADSIM_MAX_SERVICES || servers.size() > 6 || (absent && !servers.empty())) throw std::length_error("at most 8 services of at most 6 servers");
        madsim_service_t s{};
        s.vaddr = (uint8_t)vaddr; s.n_servers = absent ? (uint8_t)MADSIM_SERVICE_ABSENT : (uint8_t)servers.size();
        for (size_t i = 0; i < servers.size(); i++) s.servers[i] = (uint8_t)servers[i];
        services_.push_back(s);
        return (int)services_.size() - 1;
    }
    // 10.0.0.<node>:port, or 0.0.0.0:port / 127.0.0.1:port as used on `node` (kind = MADSIM_ADDR_*).  port 0 = an ephemeral
    // Endpoint (network.rs:224-236): each bind gets the node's lowest free port for that IP; not a destination operand.
    int addr(int node, uint16_t port, uint8_t kind = MADSIM_ADDR_IP) {
        socks_.push_back(madsim_sock_t{(uint8_t)node, kind, port}); return (int)socks_.size() - 1;
    }
    // spawn_on_drop: the body owns a guard whose Drop calls task::spawn(<the NEXT task declared>) (MADSIM_PROG_DROP_SPAWN)
    Task& task(int node, bool init = false, bool before_block_on = false, bool spawn_on_drop = false) {
        if (tasks_.size() >= 255) throw std::length_error("at most 255 task programs");
        tasks_.push_back(Task((int)tasks_.size(), node, (uint8_t)((init ? MADSIM_PROG_INIT : 0) | (before_block_on ? MADSIM_PROG_PRE : 0) |
                                                                 (spawn_on_drop ? MADSIM_PROG_DROP_SPAWN : 0))));
        return tasks_.back();
    }
    Workload build() {
        Workload w;
        w.nodes = nodes_; w.socks = socks_; w.services = services_;
        // message codes: literal messages are interned from 254 downwards, a number is its decimal text; a node's row has bit c
        // set when one of its patterns is a substring of the text of code c (the rule of madsim_amd/workload.py::_panic_rows)
        std::vector<std::string> literals;
        for (auto& t : tasks_) for (auto& i : t.code_) if (!i.text.empty() && std::find(literals.begin(), literals.end(), i.text) == literals.end()) literals.push_back(i.text);
        std::sort(literals.begin(), literals.end());
        if (literals.size() > 200) throw std::length_error("at most 200 distinct literal panic messages");
        const uint32_t dyn_max = 254 - (uint32_t)literals.size();
        auto text_of = [&](uint32_t c) { return c > dyn_max ? literals[254 - c] : std::to_string(c); };
        bool any_patterns = false;
        for (auto& p : patterns_) any_patterns |= !p.empty();
        if (any_patterns || !literals.empty()) {
            w.panic_dyn_max = dyn_max;
            w.panic_match.assign(8 * nodes_.size(), 0);
            for (size_t n = 0; n < patterns_.size(); n++)
                for (uint32_t c = 0; c <= 254; c++)
                    for (auto& p : patterns_[n]) if (text_of(c).find(p) != std::string::npos) w.panic_match[8 * n + (c >> 5)] |= 1u << (c & 31);
            for (size_t n = 0; n < nodes_.size(); n++)          // numeric patterns given to create_node(): their decimal text
                for (uint32_t k = 0; k < nodes_[n].n_match && k < 2; k++)
                    for (uint32_t c = 0; c <= 254; c++)
                        if (text_of(c).find(std::to_string(nodes_[n].match[k])) != std::string::npos) w.panic_match[8 * n + (c >> 5)] |= 1u << (c & 31);
        }
        for (auto& t : tasks_) {
            uint16_t base = (uint16_t)w.insns.size();
            if (t.code_.empty() || (t.code_.back().in.op != MS_OP_DONE && t.code_.back().in.op != MS_OP_JMP)) t.done();
            w.progs.push_back(madsim_prog_t{(uint8_t)t.node_, t.flags_, base});
            for (auto& i : t.code_) {
                madsim_insn_t in = i.in;
                if (!i.text.empty()) in.imm = 254 - (uint32_t)(std::find(literals.begin(), literals.end(), i.text) - literals.begin());
                else if (in.op == MS_OP_PANIC && in.a == 0 && in.imm > dyn_max) throw std::invalid_argument("numeric panic code collides with a literal message");
                if (i.reloc) in.b = (uint16_t)(in.b + base);
                w.insns.push_back(in);
            }
        }
        return w;
    }

  private:
    std::vector<madsim_node_t> nodes_;
    std::vector<madsim_sock_t> socks_;
    std::vector<Task> tasks_;
    std::vector<std::string> payloads_, rpc_messages_;
    std::vector<std::vector<std::string>> patterns_;      // per node: restart_on_panic_matching strings
    std::vector<madsim_service_t> services_;
};

inline Task& Task::panic(const std::string& message) {
    if (message.empty()) throw std::invalid_argument("empty panic message");
    code_.push_back({madsim_insn_t{MS_OP_PANIC, 0, 0, 0}, false, message});
    return *this;
}

namespace runtime {

// runtime/mod.rs:205-210
inline void panic_with_info(uint64_t seed) {
    std::fprintf(stderr, "note: run with `MADSIM_TEST_SEED=%llu` environment variable to reproduce this error\n",
                 (unsigned long long)seed);
}

struct Builder {
    uint64_t seed = 0;
    uint64_t count = 1;
    uint16_t jobs = 1;
    Config config;
    std::optional<double> time_limit;        // seconds
    bool check = false;
    bool allow_system_thread = false;
    int device = 0;
    madsim_limits_t capacities{};            // device capacities to start from (no reference counterpart; 0 = defaults);
                                             // capacities.no_trace_hash = 1: results without the determinism-log fingerprint (4 % faster on ping-pong)
    uint32_t resolve_flags = 0;              // MADSIM_CAMPAIGN_RESOLVE and its rounds bits, set by resolve_runner() (0 = runner verdicts counted apart)

    // The seeds the four campaign forms below run, when they are not the range seed .. seed + count: search_failures, campaign_stats,
    // failure_groups and diff_against all honour over_seeds() (ONE setter rather than four overloads: the list is a property of the run, like
    // the seed range it replaces).  The list must ascend strictly — sorted, no duplicates: std::sort + std::unique — so that "smallest seed"
    // and "first position" stay one thing; the library refuses any other list (MADSIM_E_ARG), it never sorts silently.  seeds_run then counts
    // positions of the list.  over_range() goes back to seed .. seed + count.  search_first_failure, run and check_determinism ignore it.
    std::vector<uint64_t> seed_list;
    bool listed_seeds = false;
    Builder& over_seeds(std::vector<uint64_t> seeds) { seed_list = std::move(seeds); listed_seeds = true; return *this; }
    Builder& over_range() { seed_list.clear(); listed_seeds = false; return *this; }

    // search_failures, campaign_stats, failure_groups and diff_against report on SETTLED results: seeds that come back with a runner verdict
    // (a device capacity, the step cap) are run again on the device under grown limits, up to `rounds` times (0 = the library's default,
    // at most MADSIM_RESOLVE_MAX_ROUNDS), before their batch is reported (MADSIM_CAMPAIGN_RESOLVE).  resolved() tells what the rounds did.
    Builder& resolve_runner(unsigned rounds = 0) {
        if (rounds > MADSIM_RESOLVE_MAX_ROUNDS) throw std::invalid_argument("resolve_runner: at most MADSIM_RESOLVE_MAX_ROUNDS rounds");
        resolve_flags = MADSIM_CAMPAIGN_RESOLVE | (uint32_t)rounds << MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT;
        return *this;
    }
    // The resolve account of the most recent campaign call on the default context (madsim_hip_campaign_resolved).
    static madsim_resolve_t resolved() {
        madsim_resolve_t r{};
        madsim::check(madsim_hip_campaign_resolved(&r));
        return r;
    }

    // builder.rs:64-118
    static Builder from_env() {
        Builder b;
        auto env = [](const char* k) -> const char* { return std::getenv(k); };
        auto parse_u64 = [](const char* s, const char* what) -> uint64_t {
            char* end = nullptr;
            unsigned long long v = std::strtoull(s, &end, 10);
            if (!s[0] || *end) throw std::invalid_argument(std::string(what) + " should be an integer");
            return v;
        };
        if (auto s = env("MADSIM_TEST_SEED")) b.seed = parse_u64(s, "MADSIM_TEST_SEED");
        else b.seed = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
                          std::chrono::system_clock::now().time_since_epoch()).count();
        if (auto s = env("MADSIM_TEST_JOBS")) b.jobs = (uint16_t)parse_u64(s, "MADSIM_TEST_JOBS");
        if (auto s = env("MADSIM_TEST_CONFIG")) {
            std::ifstream f(s);
            if (!f) throw std::invalid_argument("failed to read config file");
            std::stringstream ss; ss << f.rdbuf();
            b.config = Config::from_toml(ss.str());
        }
        if (auto s = env("MADSIM_TEST_NUM")) b.count = parse_u64(s, "MADSIM_TEST_NUM");
        if (auto s = env("MADSIM_TEST_TIME_LIMIT")) {
            char* end = nullptr;
            double v = std::strtod(s, &end);
            if (!s[0] || *end) throw std::invalid_argument("MADSIM_TEST_TIME_LIMIT should be an number");
            b.time_limit = v;
        }
        b.check = env("MADSIM_TEST_CHECK_DETERMINISM") != nullptr;
        if (b.check && b.count < 2) b.count = 2;
        b.allow_system_thread = env("MADSIM_ALLOW_SYSTEM_THREAD") != nullptr;
        return b;
    }

    // What seeds traced (madsim_hip_trace_seeds): the values their test bodies handed to trace / trace_system_time / trace_instant / trace_val /
    // a traced tick, in execution order — the output of a failing #[madsim::test] — for a whole list of seeds in ONE launch of the trace
    // build.  `observations` holds the first obs_cap values (n_observations says how many there were), `log` the first log_cap bytes of the
    // determinism log.  The builder's resolve_runner() rounds apply: seeds that come back with a re-runnable runner verdict are replayed as
    // one further call under madsim_hip_grow_limits(.., r), r = 1, 2, ..  Under a runner verdict that stays the lists mean nothing.
    struct SeedTrace {
        uint64_t seed = 0;
        madsim_result_t result{};
        std::vector<uint64_t> observations;
        uint64_t n_observations = 0;
        std::vector<uint8_t> log;
        uint64_t log_len = 0;
    };
    static uint64_t fold_observations(const std::vector<uint64_t>& values) {     // the obs_hash of a run that traced `values`: 64-bit FNV-1a
        uint64_t h = 0xCBF29CE484222325ull;
        for (uint64_t v : values) h = (h ^ v) * 0x100000001B3ull;
        return h;
    }
    std::vector<SeedTrace> trace_seeds(const Workload& wl, const std::vector<uint64_t>& seeds, size_t obs_cap = 256, size_t log_cap = 0) const {
        madsim::check(madsim_hip_init(device));
        madsim_workload_t w = wl.raw();
        madsim_config_t cfg = config.raw();
        madsim_limits_t lim0 = capacities;
        if (time_limit) { lim0.time_limit_ns = (uint64_t)(*time_limit * 1e9 + 0.5); if (!lim0.time_limit_ns) lim0.time_limit_ns = 1; }
        return trace_seeds_under(w, cfg, lim0, seeds, obs_cap, log_cap);
    }
    // One seed's observation list (the shape of the oracle's observe_seed); `out`: its result.
    std::vector<uint64_t> observe_seed(const Workload& wl, uint64_t s, madsim_result_t* out = nullptr, size_t obs_cap = 65536) const {
        SeedTrace t = trace_seeds(wl, {s}, obs_cap, 0).front();
        if (out) *out = t.result;
        return t.observations;
    }

  private:
    uint32_t resolve_rounds() const {            // the rounds resolve_runner() asked for (0: none)
        if (!(resolve_flags & MADSIM_CAMPAIGN_RESOLVE)) return 0;
        const uint32_t rounds = (resolve_flags & MADSIM_CAMPAIGN_RESOLVE_ROUNDS_MASK) >> MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT;
        return rounds ? rounds : MADSIM_RESOLVE_DEFAULT_ROUNDS;
    }
    std::vector<SeedTrace> trace_seeds_under(const madsim_workload_t& w, const madsim_config_t& cfg, const madsim_limits_t& lim0,
                                             const std::vector<uint64_t>& seeds, size_t obs_cap, size_t log_cap) const {
        std::vector<SeedTrace> traces(seeds.size());
        std::vector<size_t> idx(seeds.size());
        for (size_t i = 0; i < idx.size(); i++) idx[i] = i;
        uint32_t rounds = 0;
        if (resolve_flags & MADSIM_CAMPAIGN_RESOLVE) {
            rounds = (resolve_flags & MADSIM_CAMPAIGN_RESOLVE_ROUNDS_MASK) >> MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT;
            if (!rounds) rounds = MADSIM_RESOLVE_DEFAULT_ROUNDS;
        }
        for (uint32_t r = 0; r <= rounds && !idx.empty(); r++) {
            madsim_limits_t lim = lim0;
            if (r) madsim::check(madsim_hip_grow_limits(&w, &lim0, r, &lim));
            const size_t m = idx.size();
            std::vector<uint64_t> s(m), obs(m * obs_cap), olen(m), llen(m);
            std::vector<uint8_t> logs(m * log_cap);
            std::vector<madsim_result_t> res(m);
            for (size_t j = 0; j < m; j++) s[j] = seeds[idx[j]];
            madsim::check(madsim_hip_trace_seeds(&w, &cfg, s.data(), m, &lim, log_cap ? logs.data() : nullptr, log_cap, obs_cap ? obs.data() : nullptr,
                                                 obs_cap, llen.data(), olen.data(), res.data()));
            std::vector<size_t> again;
            const uint32_t cap = lim.max_steps ? lim.max_steps : 1u << 24, ceiling = lim.max_steps_ceiling ? lim.max_steps_ceiling : 1u << 28;
            for (size_t j = 0; j < m; j++) {
                SeedTrace& t = traces[idx[j]];
                t.seed = s[j]; t.result = res[j]; t.n_observations = olen[j]; t.log_len = llen[j];
                t.observations.assign(obs.begin() + j * obs_cap, obs.begin() + j * obs_cap + (size_t)std::min<uint64_t>(olen[j], obs_cap));
                t.log.assign(logs.begin() + j * log_cap, logs.begin() + j * log_cap + (size_t)std::min<uint64_t>(llen[j], log_cap));
                if (res[j].verdict == MADSIM_OVERFLOW || (res[j].verdict == MADSIM_STEP_LIMIT && cap < ceiling)) again.push_back(idx[j]);
            }
            idx.swap(again);
        }
        return traces;
    }
    static bool same_result(const madsim_result_t& a, const madsim_result_t& b) {
        return a.verdict == b.verdict && a.steps == b.steps && a.clock_ns == b.clock_ns && a.msg_count == b.msg_count && a.rng_calls == b.rng_calls &&
               a.trace_hash == b.trace_hash && a.obs_hash == b.obs_hash;
    }
    // the `observe` option of search_failures / failure_groups / diff_against: the listed seeds replayed in one trace_seeds call; the trace build
    // must give the bytes the campaign listed (a listed runner verdict says nothing a replay must repeat)
    std::vector<std::vector<uint64_t>> observe_listed(const madsim_workload_t& w, const madsim_config_t& cfg, const madsim_limits_t& lim,
                                                      const std::vector<uint64_t>& seeds, const std::vector<madsim_result_t>& listed, size_t cap) const {
        std::vector<std::vector<uint64_t>> lists;
        if (seeds.empty()) return lists;
        std::vector<SeedTrace> traces = trace_seeds_under(w, cfg, lim, seeds, cap, 0);
        for (size_t i = 0; i < traces.size(); i++) {
            if (!MADSIM_IS_RUNNER_VERDICT(listed[i].verdict) && !same_result(traces[i].result, listed[i]))
                throw Error(MADSIM_E_HIP, "seed " + std::to_string(seeds[i]) + ": the trace build's replay differs from the result the campaign listed");
            lists.push_back(std::move(traces[i].observations));
        }
        return lists;
    }

  public:
    // Seed search: seed .. seed + count as batches the LIBRARY keeps in flight on its own streams (madsim_hip_run_campaign),
    // stopping at the first batch that holds a failing seed; prints the reproduction note for the seed it found.  No per-seed
    // results: re-run the reported seed for details.
    madsim_campaign_t search_first_failure(const Workload& wl) const {
        madsim::check(madsim_hip_init(device));
        madsim_workload_t w = wl.raw();
        madsim_config_t cfg = config.raw();
        madsim_limits_t lim = capacities;
        if (time_limit) { lim.time_limit_ns = (uint64_t)(*time_limit * 1e9 + 0.5); if (!lim.time_limit_ns) lim.time_limit_ns = 1; }
        madsim_campaign_t rep{};
        madsim::check(madsim_hip_run_campaign(&w, &cfg, seed, count, 0, 0, MADSIM_CAMPAIGN_STOP_AT_FAILURE, &lim, &rep));
        if (rep.first_failing_seed != UINT64_MAX) panic_with_info(rep.first_failing_seed);
        return rep;
    }

    // Triage: WHICH seeds of seed .. seed + count fail, and how (madsim_hip_run_campaign_collect).  The whole range runs at the
    // campaign's rate; the `max_failures` smallest failing seeds come back in ascending order, each with the result
    // madsim_hip_run_batch gives for it, beside the number of seeds per verdict value (index = enum madsim_verdict) and the
    // campaign report.  Does not "panic": a caller that wants the reference's behaviour takes failures.front() to run().
    struct Failures {
        std::vector<madsim_failure_t> failures;
        std::array<uint64_t, 8> by_verdict{};
        madsim_campaign_t campaign{};
        std::vector<std::vector<uint64_t>> observations;                  // observe > 0: what failures[i].seed traced, at most `observe` values
    };
    Failures search_failures(const Workload& wl, size_t max_failures, size_t observe = 0) const {
        madsim::check(madsim_hip_init(device));
        madsim_workload_t w = wl.raw();
        madsim_config_t cfg = config.raw();
        madsim_limits_t lim = capacities;
        if (time_limit) { lim.time_limit_ns = (uint64_t)(*time_limit * 1e9 + 0.5); if (!lim.time_limit_ns) lim.time_limit_ns = 1; }
        Failures f;
        f.failures.resize(max_failures);
        madsim_collect_t col{};
        col.failures = max_failures ? f.failures.data() : nullptr;
        col.cap = max_failures;
        madsim::check(listed_seeds ? madsim_hip_run_seeds_campaign(&w, &cfg, seed_list.data(), seed_list.size(), 0, 0, resolve_flags, &lim, &f.campaign, &col, nullptr, nullptr)
                                   : madsim_hip_run_campaign_collect(&w, &cfg, seed, count, 0, 0, resolve_flags, &lim, &f.campaign, &col));
        f.failures.resize((size_t)col.n_listed);
        for (int v = 0; v < 8; v++) f.by_verdict[(size_t)v] = col.n_by_verdict[v];
        if (observe) {
            std::vector<uint64_t> seeds;
            std::vector<madsim_result_t> listed;
            for (const madsim_failure_t& x : f.failures) { seeds.push_back(x.seed); listed.push_back(x.result); }
            f.observations = observe_listed(w, cfg, lim, seeds, listed, observe);
        }
        return f;
    }

    // Statistics: HOW the runs of seed .. seed + count are distributed, and which seeds are the outliers (madsim_hip_run_campaign_stats).
    // The whole range runs at the campaign's rate; over the seeds whose verdict bit is set in `include` (bit v = verdict v, bits 0-3) come
    // back the count, and per metric (index MADSIM_STAT_CLOCK / _STEPS / _MSGS / _RNG) min, max, the 128-bit sum, the bucket counts and the
    // `top_k` (<= MADSIM_STAT_MAX_TOP) seeds that come first by value descending, then seed ascending.
    struct Stats {
        madsim_stats_t stats{};                                           // (stats.top points into `top` while this object is not moved from)
        std::vector<madsim_extreme_t> top;                                // [MADSIM_STAT_METRICS][top_k], stats.n_top valid per row
        madsim_campaign_t campaign{};
        const madsim_extreme_t* top_of(uint32_t metric) const { return top.data() + (size_t)metric * stats.top_k; }
    };
    Stats campaign_stats(const Workload& wl, uint32_t include = 1u << MADSIM_PASS, uint32_t top_k = 0) const {
        madsim::check(madsim_hip_init(device));
        madsim_workload_t w = wl.raw();
        madsim_config_t cfg = config.raw();
        madsim_limits_t lim = capacities;
        if (time_limit) { lim.time_limit_ns = (uint64_t)(*time_limit * 1e9 + 0.5); if (!lim.time_limit_ns) lim.time_limit_ns = 1; }
        Stats s;
        s.top.resize((size_t)MADSIM_STAT_METRICS * top_k);
        s.stats.include = include;
        s.stats.top_k = top_k;
        s.stats.top = top_k ? s.top.data() : nullptr;
        madsim::check(listed_seeds ? madsim_hip_run_seeds_campaign(&w, &cfg, seed_list.data(), seed_list.size(), 0, 0, resolve_flags, &lim, &s.campaign, nullptr, &s.stats, nullptr)
                                   : madsim_hip_run_campaign_stats(&w, &cfg, seed, count, 0, 0, resolve_flags, &lim, &s.campaign, nullptr, &s.stats));
        return s;
    }

    // Failure modes: HOW MANY DIFFERENT failures seed .. seed + count holds (madsim_hip_run_campaign_groups).  The whole range runs at the
    // campaign's rate; the seeds whose verdict bit is set in `include` are grouped by (verdict, key), `key_field` one of MADSIM_GROUP_KEY_*
    // (obs_hash by default: what the test body traced), and the first `max_groups` groups in order of first appearance come back, each with
    // its exact count over the range and its smallest seed — the one to replay.
    struct Groups {
        std::vector<madsim_group_t> groups;                               // ascending by first_seed
        uint64_t n_grouped = 0, n_ungrouped = 0;                          // counted seeds in `groups` / in the groups that did not make the list
        madsim_campaign_t campaign{};
        std::vector<std::vector<uint64_t>> observations;                  // observe > 0: what groups[i].first_seed traced, at most `observe` values
    };
    Groups failure_groups(const Workload& wl, size_t max_groups,
                          uint32_t include = (1u << MADSIM_PANIC) | (1u << MADSIM_DEADLOCK) | (1u << MADSIM_TIME_LIMIT),
                          uint32_t key_field = MADSIM_GROUP_KEY_OBS) const {
        return failure_groups(wl, max_groups, include, key_field, 0);
    }
    // ... with `observe` > 0: each group's smallest seed replayed on the trace build (one trace_seeds call), Groups::observations[i] = the values it
    // traced — the failure mode spelled out.  The replay must carry the verdict and the key the seed was grouped under.
    Groups failure_groups(const Workload& wl, size_t max_groups, uint32_t include, uint32_t key_field, size_t observe) const {
        madsim::check(madsim_hip_init(device));
        madsim_workload_t w = wl.raw();
        madsim_config_t cfg = config.raw();
        madsim_limits_t lim = capacities;
        if (time_limit) { lim.time_limit_ns = (uint64_t)(*time_limit * 1e9 + 0.5); if (!lim.time_limit_ns) lim.time_limit_ns = 1; }
        Groups g;
        g.groups.resize(max_groups);
        madsim_groups_t grp{};
        grp.include = include;
        grp.key_field = key_field;
        grp.groups = max_groups ? g.groups.data() : nullptr;
        grp.cap = max_groups;
        madsim::check(listed_seeds ? madsim_hip_run_seeds_campaign(&w, &cfg, seed_list.data(), seed_list.size(), 0, 0, resolve_flags, &lim, &g.campaign, nullptr, nullptr, &grp)
                                   : madsim_hip_run_campaign_groups(&w, &cfg, seed, count, 0, 0, resolve_flags, &lim, &g.campaign, nullptr, nullptr, &grp));
        g.groups.resize((size_t)grp.n_groups);
        g.n_grouped = grp.n_grouped;
        g.n_ungrouped = grp.n_ungrouped;
        if (observe && !g.groups.empty()) {
            std::vector<uint64_t> seeds;
            for (const madsim_group_t& x : g.groups) seeds.push_back(x.first_seed);
            std::vector<SeedTrace> traces = trace_seeds_under(w, cfg, lim, seeds, observe, 0);
            for (size_t i = 0; i < traces.size(); i++) {
                const madsim_result_t& r = traces[i].result;
                const uint64_t key = key_field == MADSIM_GROUP_KEY_OBS ? r.obs_hash : key_field == MADSIM_GROUP_KEY_TRACE ? r.trace_hash :
                                     key_field == MADSIM_GROUP_KEY_MSGS ? r.msg_count : key_field == MADSIM_GROUP_KEY_CLOCK ? r.clock_ns :
                                     key_field == MADSIM_GROUP_KEY_RNG ? r.rng_calls : r.steps;
                if (r.verdict != g.groups[i].verdict || key != g.groups[i].key)
                    throw Error(MADSIM_E_HIP, "seed " + std::to_string(seeds[i]) + ": the trace build's replay is not of the group the campaign put it in");
                g.observations.push_back(std::move(traces[i].observations));
            }
        }
        return g;
    }

    // Fix check: this builder's run of `wl` (side A) against `other`'s run of `other_wl` (side B) over THIS builder's seed .. seed + count
    // — or THIS builder's over_seeds() list: "did the fix fix all of them?" over exactly the seeds that failed (examples/corpus_test.cpp) —
    // (madsim_hip_run_campaign_diff): both sides run at the campaign's rate and are compared on the device on the result fields named in
    // `fields` (MADSIM_DIFF_*).  Config, capacities and time limit are each side's own; seed range and device are this builder's.  The
    // `max_listed` smallest differing seeds come back with both results, with the counts and the 8 x 8 verdict-transition matrix:
    // transitions[MADSIM_DEADLOCK][MADSIM_PASS] seeds were fixed, transitions[MADSIM_PASS][v != PASS] seeds were broken.
    struct Diff {
        std::vector<madsim_diff_record_t> records;                        // ascending by seed
        madsim_diff_t report{};                                           // (records / cap: of the call; read `records` above)
        madsim_campaign_t a{}, b{};                                       // each side's plain campaign report
        std::vector<std::vector<uint64_t>> observations_a, observations_b; // observe > 0: what records[i].seed traced on each side
        uint64_t regressions() const {                                    // passed on side A, any other verdict on side B
            uint64_t n = 0;
            for (int v = 1; v < 8; v++) n += report.transitions[MADSIM_PASS][v];
            return n;
        }
    };
    Diff diff_against(const Builder& other, const Workload& wl, const Workload& other_wl,
                      uint32_t fields = MADSIM_DIFF_ALL, size_t max_listed = 0) const {
        return diff_against(other, wl, other_wl, fields, max_listed, 0);
    }
    // ... with `observe` > 0: the listed seeds replayed on the trace build, one trace_seeds call per side under that side's configuration and
    // capacities (this builder's resolve rounds), Diff::observations_a[i] / _b[i] = what records[i].seed traced on each side.
    Diff diff_against(const Builder& other, const Workload& wl, const Workload& other_wl, uint32_t fields, size_t max_listed, size_t observe) const {
        madsim::check(madsim_hip_init(device));
        madsim_workload_t wa = wl.raw(), wb = other_wl.raw();
        madsim_config_t ca = config.raw(), cb = other.config.raw();
        madsim_limits_t la = capacities, lb = other.capacities;
        if (time_limit) { la.time_limit_ns = (uint64_t)(*time_limit * 1e9 + 0.5); if (!la.time_limit_ns) la.time_limit_ns = 1; }
        if (other.time_limit) { lb.time_limit_ns = (uint64_t)(*other.time_limit * 1e9 + 0.5); if (!lb.time_limit_ns) lb.time_limit_ns = 1; }
        Diff d;
        d.records.resize(max_listed);
        d.report.fields = fields;
        d.report.records = max_listed ? d.records.data() : nullptr;
        d.report.cap = max_listed;
        madsim::check(listed_seeds ? madsim_hip_run_seeds_campaign_diff(&wa, &ca, &la, &wb, &cb, &lb, seed_list.data(), seed_list.size(), 0, 0, resolve_flags, &d.a, &d.b, &d.report)
                                   : madsim_hip_run_campaign_diff(&wa, &ca, &la, &wb, &cb, &lb, seed, count, 0, 0, resolve_flags, &d.a, &d.b, &d.report));
        d.records.resize((size_t)d.report.n_listed);
        d.report.records = nullptr;                                       // (the vector may move with the struct)
        if (observe) {
            std::vector<uint64_t> seeds;
            std::vector<madsim_result_t> ra, rb;
            for (const madsim_diff_record_t& x : d.records) { seeds.push_back(x.seed); ra.push_back(x.a); rb.push_back(x.b); }
            d.observations_a = observe_listed(wa, ca, la, seeds, ra, observe);
            d.observations_b = observe_listed(wb, cb, lb, seeds, rb, observe);
        }
        return d;
    }
    Diff diff_against(const Builder& other, const Workload& wl, uint32_t fields = MADSIM_DIFF_ALL, size_t max_listed = 0) const {
        return diff_against(other, wl, wl, fields, max_listed);           // one test body under two configurations
    }

    // What a change did to each seed's numbers: this builder's run of `wl` (side A) against `other`'s run of `other_wl` (side B) over THIS
    // builder's seed .. seed + count — or THIS builder's over_seeds() list — (madsim_hip_run_paired_campaign).  A seed is paired when its
    // verdict on side A is named in `include` and on side B in `other_include` (bits 0-3, 1u << MADSIM_PASS ..); for every paired seed and
    // each of clock_ns, steps, msg_count and rng_calls the device takes b - a as a direction and an unsigned magnitude and reduces, per
    // metric and direction, count, min, max, the exact sum, a histogram and the `top_k` (<= MADSIM_STAT_MAX_TOP) extreme seeds.  Config,
    // capacities and time limit are each side's own; seeds, device and resolve_runner() rounds are this builder's.
    struct Paired {
        madsim_paired_t report{};                                         // (top: of the call; read `top` below)
        std::vector<madsim_paired_extreme_t> top[2 * MADSIM_STAT_METRICS]; // [2 * metric + direction]: magnitude descending, then seed ascending
        madsim_campaign_t a{}, b{};                                       // each side's plain campaign report
        static unsigned __int128 wide(uint64_t lo, uint64_t hi) { return (unsigned __int128)hi << 64 | lo; }
        const std::vector<madsim_paired_extreme_t>& regressions(uint32_t metric) const { return top[2 * metric + MADSIM_PAIRED_UP]; }
        const std::vector<madsim_paired_extreme_t>& improvements(uint32_t metric) const { return top[2 * metric + MADSIM_PAIRED_DOWN]; }
        // the mean of b - a over the paired seeds (the sums are exact; the quotient is a double), 0 when nothing is paired
        double mean_delta(uint32_t metric) const {
            if (!report.n_paired) return 0.0;
            const madsim_metric_t &up = report.delta[2 * metric + MADSIM_PAIRED_UP], &down = report.delta[2 * metric + MADSIM_PAIRED_DOWN];
            const unsigned __int128 u = wide(up.sum_lo, up.sum_hi), d = wide(down.sum_lo, down.sum_hi);
            return (u >= d ? (double)(u - d) : -(double)(d - u)) / (double)report.n_paired;
        }
    };
    Paired paired_against(const Builder& other, const Workload& wl, const Workload& other_wl, uint32_t include = 1u << MADSIM_PASS,
                          uint32_t other_include = 0, uint32_t top_k = 0) const {      // other_include 0: the same as `include`
        madsim::check(madsim_hip_init(device));
        madsim_workload_t wa = wl.raw(), wb = other_wl.raw();
        madsim_config_t ca = config.raw(), cb = other.config.raw();
        madsim_limits_t la = capacities, lb = other.capacities;
        if (time_limit) { la.time_limit_ns = (uint64_t)(*time_limit * 1e9 + 0.5); if (!la.time_limit_ns) la.time_limit_ns = 1; }
        if (other.time_limit) { lb.time_limit_ns = (uint64_t)(*other.time_limit * 1e9 + 0.5); if (!lb.time_limit_ns) lb.time_limit_ns = 1; }
        Paired p;
        std::vector<madsim_paired_extreme_t> rows((size_t)2 * MADSIM_STAT_METRICS * top_k);
        p.report.include_a = include;
        p.report.include_b = other_include ? other_include : include;
        p.report.top_k = top_k;
        p.report.top = top_k ? rows.data() : nullptr;
        madsim::check(listed_seeds ? madsim_hip_run_seeds_campaign_paired(&wa, &ca, &la, &wb, &cb, &lb, seed_list.data(), seed_list.size(), 0, 0, resolve_flags, &p.a,
                                                                          &p.b, nullptr, &p.report)
                                   : madsim_hip_run_paired_campaign(&wa, &ca, &la, &wb, &cb, &lb, seed, count, 0, 0, resolve_flags, &p.a, &p.b, nullptr, &p.report));
        p.report.top = nullptr;                                           // (the rows are in `top`)
        for (size_t j = 0; j < 2 * MADSIM_STAT_METRICS; j++) p.top[j].assign(rows.begin() + j * top_k, rows.begin() + j * top_k + (size_t)p.report.n_top[j]);
        return p;
    }
    Paired paired_against(const Builder& other, const Workload& wl, uint32_t include = 1u << MADSIM_PASS, uint32_t other_include = 0, uint32_t top_k = 0) const {
        return paired_against(other, wl, wl, include, other_include, top_k);      // one test body under two configurations
    }

    // Across several variants: up to eight (builder, workload) pairs over THIS builder's seed .. seed + count — or THIS builder's
    // over_seeds() list — in one campaign (madsim_hip_run_sweep_campaign): a parameter sweep, a stack of versions of a test body, one body
    // under every state layout.  Config, capacities and time limit are each variant's own; seed range, device and resolve_runner() rounds
    // are this builder's.  Every seed is classified across all variants on the device: report.n_by_mask[m] counts the settled seeds that
    // fail in exactly the variants whose bits m has, and the `max_listed` smallest seeds `list_rule` (MADSIM_SWEEP_LIST_*) selects come
    // back with their masks and every variant's verdict.  `fields`: the MADSIM_DIFF_* fields compared against variant 0 (0 = none).
    struct Sweep {
        std::vector<madsim_sweep_record_t> records;                       // ascending by seed
        madsim_sweep_t report{};                                          // (records / cap: of the call; read `records` above)
        std::vector<madsim_campaign_t> campaigns;                         // each variant's plain campaign report
        size_t n_variants() const { return campaigns.size(); }
        uint64_t fails(unsigned v) const {                                // settled seeds that fail in variant v
            uint64_t n = 0;
            for (unsigned m = 0; m < 256; m++) if (m >> v & 1) n += report.n_by_mask[m];
            return n;
        }
        uint64_t only(unsigned v) const { return report.n_by_mask[1u << v]; }      // ... in variant v and in no other
        uint64_t fails_not(unsigned i, unsigned j) const {                // ... in variant i and not in variant j
            uint64_t n = 0;
            for (unsigned m = 0; m < 256; m++) if ((m >> i & 1) && !(m >> j & 1)) n += report.n_by_mask[m];
            return n;
        }
        bool nested() const {                                             // every non-empty mask is a suffix set: the failing sets grow with the variant index
            const unsigned full = (1u << n_variants()) - 1u;
            for (unsigned m = 1; m <= full; m++) if (report.n_by_mask[m] && m != (full & ~((m & (0u - m)) - 1u))) return false;
            return true;
        }
        std::vector<uint64_t> first_failing() const {                     // [v] = settled seeds whose lowest failing variant is v: the bisect reading
            std::vector<uint64_t> h(n_variants(), 0);
            for (unsigned m = 1; m < (1u << n_variants()); m++) h[(unsigned)__builtin_ctz(m)] += report.n_by_mask[m];
            return h;
        }
    };
    Sweep sweep(const std::vector<std::pair<const Builder*, const Workload*>>& variants, uint32_t fields = MADSIM_DIFF_VERDICT,
                unsigned list_rule = MADSIM_SWEEP_LIST_MIXED, size_t max_listed = 0) const {
        const size_t V = variants.size();
        if (V < 2 || V > MADSIM_SWEEP_MAX_VARIANTS) throw std::invalid_argument("sweep: 2 .. MADSIM_SWEEP_MAX_VARIANTS variants");
        std::vector<madsim_workload_t> w(V);
        std::vector<madsim_config_t> c(V);
        std::vector<madsim_limits_t> l(V);
        std::vector<madsim_sweep_variant_t> var(V);
        Sweep s;
        s.campaigns.resize(V);
        for (size_t v = 0; v < V; v++) {
            if (!variants[v].first || !variants[v].second) throw std::invalid_argument("sweep: a variant is a builder and a workload");
            const Builder& b = *variants[v].first;
            w[v] = variants[v].second->raw(); c[v] = b.config.raw(); l[v] = b.capacities;
            if (b.time_limit) { l[v].time_limit_ns = (uint64_t)(*b.time_limit * 1e9 + 0.5); if (!l[v].time_limit_ns) l[v].time_limit_ns = 1; }
            var[v] = madsim_sweep_variant_t{&w[v], &c[v], &l[v], &s.campaigns[v]};
        }
        s.records.resize(max_listed);
        s.report.fields = fields; s.report.list_rule = list_rule;
        s.report.records = max_listed ? s.records.data() : nullptr;
        s.report.cap = max_listed;
        if (!listed_seeds || !seed_list.empty()) madsim::check(madsim_hip_init(device));      // (an empty list runs nothing: no device needed)
        static const uint64_t none = 0;                                   // (an empty list is still the list form: a non-null pointer)
        madsim::check(listed_seeds ? madsim_hip_run_sweep_campaign(var.data(), (uint32_t)V, 0, seed_list.size(), seed_list.empty() ? &none : seed_list.data(), 0, 0,
                                                                   resolve_flags, &s.report)
                                   : madsim_hip_run_sweep_campaign(var.data(), (uint32_t)V, seed, count, nullptr, 0, 0, resolve_flags, &s.report));
        s.records.resize((size_t)s.report.n_listed);
        s.report.records = nullptr;                                       // (the vector may move with the struct)
        return s;
    }

    // Which traced values the builder's seeds reach, by verdict (madsim_hip_census_range / madsim_hip_census_seeds): `seed .. seed + count`,
    // or the seed list when one was given, run on the trace build and reduced on the device.  values: ascending by value, one record per
    // distinct value among the first `obs_cap` observations of the counted seeds (verdict in `include`, a bit mask over PASS, PANIC,
    // DEADLOCK, TIME_LIMIT); more than `max_values` of them throws (MADSIM_E_LIMITS: a traced time or random value is no probe vocabulary).
    // This builder's resolve_runner() rounds apply: the seeds a call leaves with a runner verdict are run again in one list call per round
    // under madsim_hip_grow_limits(.., r) and merged in; what stays is counted in totals.n_runner and listed in runner_seeds.
    struct Census {
        std::vector<madsim_census_value_t> values;
        madsim_census_t totals{};                  // the counts (the pointers and caps are the call's own: not meaningful here)
        std::vector<uint64_t> runner_seeds;
        const madsim_census_value_t* row(uint64_t v) const {
            auto it = std::lower_bound(values.begin(), values.end(), v, [](const madsim_census_value_t& e, uint64_t x) { return e.value < x; });
            return it != values.end() && it->value == v ? &*it : nullptr;
        }
        uint64_t reached(uint64_t v) const {       // counted seeds that observed v at least once
            const madsim_census_value_t* e = row(v);
            return e ? e->n_seeds[0] + e->n_seeds[1] + e->n_seeds[2] + e->n_seeds[3] : 0;
        }
        std::vector<uint64_t> never(const std::vector<uint64_t>& expected) const {      // the sometimes-assertion: expected values nobody observed
            std::vector<uint64_t> out;
            for (uint64_t v : expected) if (!row(v)) out.push_back(v);
            return out;
        }
    };
    Census census(const Workload& wl, uint32_t obs_cap = 256, uint64_t max_values = 4096, uint32_t include = 0xf, uint64_t chunk = 0) const {
        madsim::check(madsim_hip_init(device));
        madsim_workload_t w = wl.raw();
        madsim_config_t cfg = config.raw();
        madsim_limits_t lim0 = capacities;
        if (time_limit) { lim0.time_limit_ns = (uint64_t)(*time_limit * 1e9 + 0.5); if (!lim0.time_limit_ns) lim0.time_limit_ns = 1; }
        uint32_t rounds = 0;
        if (resolve_flags & MADSIM_CAMPAIGN_RESOLVE) {
            rounds = (resolve_flags & MADSIM_CAMPAIGN_RESOLVE_ROUNDS_MASK) >> MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT;
            if (!rounds) rounds = MADSIM_RESOLVE_DEFAULT_ROUNDS;
        }
        auto one = [&](const madsim_limits_t& lim, const std::vector<uint64_t>* list) {
            Census c;
            const uint64_t n = list ? list->size() : count;
            c.values.resize(max_values ? max_values : 1);
            c.runner_seeds.resize(n ? n : 1);
            madsim_census_t& t = c.totals;
            t.include = include; t.obs_cap = obs_cap; t.values = c.values.data(); t.cap = max_values;
            t.runner_seeds = c.runner_seeds.data(); t.runner_cap = n;
            madsim::check(list ? madsim_hip_census_seeds(&w, &cfg, list->data(), n, chunk, &lim, &t) : madsim_hip_census_range(&w, &cfg, seed, n, chunk, &lim, &t));
            c.values.resize(t.n_values);
            c.runner_seeds.resize(t.n_runner_listed);
            t.values = nullptr; t.runner_seeds = nullptr;
            return c;
        };
        Census c = one(lim0, listed_seeds ? &seed_list : nullptr);
        for (uint32_t r = 1; r <= rounds && !c.runner_seeds.empty(); r++) {
            madsim_limits_t lim = lim0;
            madsim::check(madsim_hip_grow_limits(&w, &lim0, r, &lim));
            const Census more = one(lim, &c.runner_seeds);
            std::vector<madsim_census_value_t> merged;
            for (size_t i = 0, j = 0; i < c.values.size() || j < more.values.size();) {
                if (j >= more.values.size() || (i < c.values.size() && c.values[i].value < more.values[j].value)) merged.push_back(c.values[i++]);
                else if (i >= c.values.size() || more.values[j].value < c.values[i].value) merged.push_back(more.values[j++]);
                else {
                    madsim_census_value_t e = c.values[i++];
                    const madsim_census_value_t& o = more.values[j++];
                    for (int k = 0; k < 4; k++) e.n_seeds[k] += o.n_seeds[k];
                    e.n_total += o.n_total; e.first_seed = std::min(e.first_seed, o.first_seed); e.max_per_seed = std::max(e.max_per_seed, o.max_per_seed);
                    merged.push_back(e);
                }
            }
            if (merged.size() > max_values) throw Error(MADSIM_E_LIMITS, "census: more than max_values distinct observed values once the runner seeds are settled");
            c.values.swap(merged);
            for (int k = 0; k < 4; k++) { c.totals.n_counted[k] += more.totals.n_counted[k]; c.totals.n_silent[k] += more.totals.n_silent[k]; }
            c.totals.n_truncated += more.totals.n_truncated; c.totals.n_observations += more.totals.n_observations;
            c.totals.n_runner = more.totals.n_runner; c.totals.n_runner_listed = more.totals.n_runner_listed;
            c.totals.n_values = c.values.size();
            c.runner_seeds = more.runner_seeds;
        }
        return c;
    }

    // Where the tasks of the listed seeds stand when their runs end (madsim_hip_task_states): one record per task still alive, in task-slot
    // order — MADSIM_TASK_STATE / _PROG / _PC / _CNT0 / _CNT1 decode one, describe() spells it out against the workload table.  `tasks` holds
    // the first task_cap records, n_tasks says how many there were.  A seed with a runner verdict has none; the builder's resolve_runner()
    // rounds replay such seeds under madsim_hip_grow_limits(.., r), as trace_seeds does.
    struct PostMortem {
        uint64_t seed = 0;
        madsim_result_t result{};
        std::vector<uint64_t> tasks;
        uint64_t n_tasks = 0;
        uint64_t shape() const { return madsim_hip_stall_shape(tasks.data(), tasks.size()); }
    };
    std::vector<PostMortem> post_mortem(const Workload& wl, const std::vector<uint64_t>& seeds, size_t task_cap = 32) const {
        madsim::check(madsim_hip_init(device));
        madsim_workload_t w = wl.raw();
        madsim_config_t cfg = config.raw();
        madsim_limits_t lim0 = capacities;
        if (time_limit) { lim0.time_limit_ns = (uint64_t)(*time_limit * 1e9 + 0.5); if (!lim0.time_limit_ns) lim0.time_limit_ns = 1; }
        std::vector<PostMortem> out(seeds.size());
        std::vector<size_t> idx(seeds.size());
        for (size_t i = 0; i < idx.size(); i++) idx[i] = i;
        const uint32_t rounds = resolve_rounds();
        for (uint32_t r = 0; r <= rounds && !idx.empty(); r++) {
            madsim_limits_t lim = lim0;
            if (r) madsim::check(madsim_hip_grow_limits(&w, &lim0, r, &lim));
            const size_t m = idx.size();
            std::vector<uint64_t> s(m), rows(m * task_cap), lens(m);
            std::vector<madsim_result_t> res(m);
            for (size_t j = 0; j < m; j++) s[j] = seeds[idx[j]];
            madsim::check(madsim_hip_task_states(&w, &cfg, s.data(), m, &lim, task_cap ? rows.data() : nullptr, task_cap, lens.data(), res.data()));
            std::vector<size_t> again;
            const uint32_t cap = lim.max_steps ? lim.max_steps : 1u << 24, ceiling = lim.max_steps_ceiling ? lim.max_steps_ceiling : 1u << 28;
            for (size_t j = 0; j < m; j++) {
                PostMortem& p = out[idx[j]];
                p.seed = s[j]; p.result = res[j]; p.n_tasks = lens[j];
                p.tasks.assign(rows.begin() + j * task_cap, rows.begin() + j * task_cap + (size_t)std::min<uint64_t>(lens[j], task_cap));
                if (res[j].verdict == MADSIM_OVERFLOW || (res[j].verdict == MADSIM_STEP_LIMIT && cap < ceiling)) again.push_back(idx[j]);
            }
            idx.swap(again);
        }
        return out;
    }
    // A site (state << 24 | prog << 16 | pc) or a whole task record as text, decoded from the workload table on the host:
    // "prog 2 (node 2) pc 20 RECV sock 1 tag 1 PARKED" — the op's name and its operands as that op reads them (a socket-table entry, a tag, a
    // program; raw a / b / imm for the rest).
    static const char* op_name(uint32_t op) {       // enum madsim_op, by value
        static const char* const names[] = {"DONE", "SPAWN", "JOIN", "ABORT", "YIELD", "PANIC", "SET", "DJNZ", "JMP", "TRACE", "SLEEP", "MARK", "SLEEP_UNTIL", "ASSERT_ELAPSED", "ADVANCE", "BUILD", "?", "?", "?", "?", "BIND", "SEND", "REPLY", "RECV", "ASSERT_VAL", "RECV_TIMEOUT", "CLOSE", "?", "?", "?", "KILL", "RESTART", "PAUSE", "RESUME", "CLOG_NODE", "UNCLOG_NODE", "CLOG_LINK", "UNCLOG_LINK", "ASSERT_EXIT", "SET_LOSS", "SLEEP_RAND", "GSET", "GADD", "ASSERT_G", "PANIC_IF_G_LT", "JEQ", "CONNECT", "ACCEPT", "CSEND", "CRECV", "CCLOSE", "RPC_CALL", "RPC_REPLY", "RAND_BOOL", "RANDOM", "TRACE_TIME", "HOOK_REQ", "HOOK_RSP", "IPVS", "SET_LATENCY", "TIMEOUT_BEGIN", "TIMEOUT_END", "INTERVAL", "TICK", "INTERVAL_RESET", "RECV_OR_TICK", "RECV_TIMEOUT_AT", "CTRL_C", "SEND_CTRL_C", "RECV_OR_CTRL_C"};
        return op < sizeof names / sizeof *names ? names[op] : "?";
    }
    static std::string describe(const Workload& wl, uint64_t site) {
        if (site >> 32) site >>= 32;
        const uint32_t state = (uint32_t)(site >> 24), prog = (uint32_t)(site >> 16) & 0xff, pc = (uint32_t)site & 0xffff;
        static const char* const states[] = {"?", "PARKED", "QUEUED", "PANICKED", "CANCELLED"};
        const madsim_workload_t w = wl.raw();
        std::string s = "prog " + std::to_string(prog);
        if (prog < w.n_progs && pc < w.n_insns) {
            const madsim_insn_t& in = w.insns[pc];
            const auto n = [](uint32_t v) { return std::to_string(v); };
            s += " (node " + n(w.progs[prog].node) + ") pc " + n(pc) + " " + op_name(in.op);
            switch (in.op) {
            case MS_OP_RECV: case MS_OP_RECV_TIMEOUT: case MS_OP_RECV_TIMEOUT_AT: case MS_OP_RECV_OR_TICK: case MS_OP_RECV_OR_CTRL_C: case MS_OP_REPLY:
                s += " sock " + n(in.a) + " tag " + n(in.b >> 8); break;
            case MS_OP_SEND: s += " sock " + n(in.a) + " to sock " + n(in.b & 0xff) + " tag " + n(in.b >> 8); break;
            case MS_OP_RPC_CALL: s += " sock " + n(in.a) + " to sock " + n(in.b & 0xff) + " request " + n((in.b >> 8) - 0x80); break;
            case MS_OP_CONNECT: s += " sock " + n(in.a) + " to sock " + n(in.b & 0xff); break;
            case MS_OP_BIND: case MS_OP_ACCEPT: case MS_OP_RPC_REPLY: case MS_OP_CLOSE: s += " sock " + n(in.a); break;
            case MS_OP_JOIN: case MS_OP_SPAWN: case MS_OP_ABORT: s += " prog " + n(in.a); break;
            case MS_OP_SLEEP: case MS_OP_SLEEP_UNTIL: s += " " + n(in.b) + " s + " + n(in.imm) + " ns"; break;
            case MS_OP_CRECV: case MS_OP_CTRL_C: case MS_OP_YIELD: case MS_OP_TICK: case MS_OP_DONE: break;
            default: s += " a=" + n(in.a) + " b=" + n(in.b) + " imm=" + n(in.imm);
            }
        } else s += " pc " + std::to_string(pc) + " (outside the workload)";
        return s + " " + (state <= 4 ? states[state] : "?");
    }

    // Where the tasks of the builder's seeds stand when their runs end, by verdict (madsim_hip_stall_census_range / _seeds): `seed .. seed +
    // count`, or the over_seeds() list, run on the trace build with the task log and reduced on the device.  sites: ascending by site
    // (MADSIM_TASK_SITE of a record), per site the counted seeds of each verdict with a task there; shapes: ascending by shape word
    // (madsim_hip_stall_shape), per distinct multiset of sites the counted seeds of each verdict and, in first_seed, the one to replay
    // (max_shapes 0: no shapes pass).  More than max_sites / max_shapes distinct entries throws (MADSIM_E_LIMITS).  The default mask counts
    // the failing verdicts.  This builder's resolve_runner() rounds apply as in census().
    struct StallCensus {
        std::vector<madsim_census_value_t> sites, shapes;
        madsim_stall_census_t totals{};            // the counts (the pointers and caps are the call's own: not meaningful here)
        std::vector<uint64_t> runner_seeds;
        std::vector<madsim_census_value_t> shapes_of(uint32_t verdict) const {       // the shapes seeds of `verdict` ended in, the most frequent first
            std::vector<madsim_census_value_t> out;
            for (const madsim_census_value_t& e : shapes) if (e.n_seeds[verdict]) out.push_back(e);
            std::sort(out.begin(), out.end(), [verdict](const madsim_census_value_t& a, const madsim_census_value_t& b) {
                return a.n_seeds[verdict] != b.n_seeds[verdict] ? a.n_seeds[verdict] > b.n_seeds[verdict] : a.value < b.value; });
            return out;
        }
    };
    StallCensus stall_census(const Workload& wl, uint32_t task_cap = 32, uint64_t max_sites = 4096, uint64_t max_shapes = 4096, uint32_t include = 0xe,
                             uint64_t chunk = 0) const {
        madsim::check(madsim_hip_init(device));
        madsim_workload_t w = wl.raw();
        madsim_config_t cfg = config.raw();
        madsim_limits_t lim0 = capacities;
        if (time_limit) { lim0.time_limit_ns = (uint64_t)(*time_limit * 1e9 + 0.5); if (!lim0.time_limit_ns) lim0.time_limit_ns = 1; }
        auto one = [&](const madsim_limits_t& lim, const std::vector<uint64_t>* list) {
            StallCensus c;
            const uint64_t n = list ? list->size() : count;
            c.sites.resize(max_sites ? max_sites : 1);
            c.shapes.resize(max_shapes ? max_shapes : 1);
            c.runner_seeds.resize(n ? n : 1);
            madsim_stall_census_t& t = c.totals;
            t.include = include; t.task_cap = task_cap; t.sites = c.sites.data(); t.site_cap = max_sites;
            t.shapes = max_shapes ? c.shapes.data() : nullptr; t.shape_cap = max_shapes;
            t.runner_seeds = c.runner_seeds.data(); t.runner_cap = n;
            madsim::check(list ? madsim_hip_stall_census_seeds(&w, &cfg, list->data(), n, chunk, &lim, &t)
                               : madsim_hip_stall_census_range(&w, &cfg, seed, n, chunk, &lim, &t));
            c.sites.resize(t.n_sites);
            c.shapes.resize(t.n_shapes);
            c.runner_seeds.resize(t.n_runner_listed);
            t.sites = t.shapes = nullptr; t.runner_seeds = nullptr;
            return c;
        };
        auto merge = [](std::vector<madsim_census_value_t>& into, const std::vector<madsim_census_value_t>& more) {
            std::vector<madsim_census_value_t> merged;
            for (size_t i = 0, j = 0; i < into.size() || j < more.size();) {
                if (j >= more.size() || (i < into.size() && into[i].value < more[j].value)) merged.push_back(into[i++]);
                else if (i >= into.size() || more[j].value < into[i].value) merged.push_back(more[j++]);
                else {
                    madsim_census_value_t e = into[i++];
                    const madsim_census_value_t& o = more[j++];
                    for (int k = 0; k < 4; k++) e.n_seeds[k] += o.n_seeds[k];
                    e.n_total += o.n_total; e.first_seed = std::min(e.first_seed, o.first_seed); e.max_per_seed = std::max(e.max_per_seed, o.max_per_seed);
                    merged.push_back(e);
                }
            }
            into.swap(merged);
        };
        StallCensus c = one(lim0, listed_seeds ? &seed_list : nullptr);
        const uint32_t rounds = resolve_rounds();
        for (uint32_t r = 1; r <= rounds && !c.runner_seeds.empty(); r++) {
            madsim_limits_t lim = lim0;
            madsim::check(madsim_hip_grow_limits(&w, &lim0, r, &lim));
            const StallCensus more = one(lim, &c.runner_seeds);
            merge(c.sites, more.sites);
            merge(c.shapes, more.shapes);
            if (c.sites.size() > max_sites || c.shapes.size() > max_shapes)
                throw Error(MADSIM_E_LIMITS, "stall_census: more than max_sites distinct sites or max_shapes distinct shapes once the runner seeds are settled");
            for (int k = 0; k < 4; k++) { c.totals.n_counted[k] += more.totals.n_counted[k]; c.totals.n_idle[k] += more.totals.n_idle[k]; }
            c.totals.n_truncated += more.totals.n_truncated; c.totals.n_tasks += more.totals.n_tasks;
            c.totals.n_runner = more.totals.n_runner; c.totals.n_runner_listed = more.totals.n_runner_listed;
            c.totals.n_sites = c.sites.size(); c.totals.n_shapes = c.shapes.size();
            c.runner_seeds = more.runner_seeds;
        }
        return c;
    }

    // Which COMBINATIONS of the values of `vocabulary` (1 .. 62 distinct values; value i owns bit i of a set word) the builder's seeds reach,
    // by verdict (madsim_hip_probe_sets_range / madsim_hip_probe_sets_seeds): `seed .. seed + count`, or the over_seeds() list, run on the
    // trace build and reduced on the device to one record per distinct set.  sets: ascending by set word; MADSIM_PROBE_SET_OTHER = the seed
    // traced a visible value outside the vocabulary, MADSIM_PROBE_SET_TRUNCATED = more than `obs_cap` values.  More than `max_sets` distinct
    // sets throws (MADSIM_E_LIMITS).  This builder's resolve_runner() rounds apply as in census().
    struct ProbeSets {
        std::vector<uint64_t> vocabulary;
        std::vector<madsim_probe_set_t> sets;
        madsim_probe_sets_t totals{};              // the counts (the pointers and caps are the call's own: not meaningful here)
        std::vector<uint64_t> runner_seeds;
        struct Mixed { uint64_t set, pass_seed, fail_seed; };
        uint64_t mask(const std::vector<uint64_t>& values) const {     // the set-word bits of vocabulary values; throws on any other value
            uint64_t m = 0;
            for (uint64_t v : values) {
                auto it = std::find(vocabulary.begin(), vocabulary.end(), v);
                if (it == vocabulary.end()) throw Error(MADSIM_E_ARG, "probe_sets: a value that is not in the vocabulary");
                m |= 1ull << (it - vocabulary.begin());
            }
            return m;
        }
        // counted seeds of the verdicts in `verdicts` (a bit mask) that reached every value of all_of and none of none_of
        uint64_t count(const std::vector<uint64_t>& all_of = {}, const std::vector<uint64_t>& none_of = {}, uint32_t verdicts = 0xf) const {
            const uint64_t want = mask(all_of), avoid = mask(none_of);
            uint64_t n = 0;
            for (const madsim_probe_set_t& e : sets)
                if ((e.set & want) == want && !(e.set & avoid))
                    for (int k = 0; k < 4; k++) if ((verdicts >> k) & 1u) n += e.n_seeds[k];
            return n;
        }
        // the sets that occur under PASS and under a failing verdict, each with its smallest passing and its smallest failing seed
        std::vector<Mixed> mixed() const {
            std::vector<Mixed> out;
            for (const madsim_probe_set_t& e : sets) {
                uint64_t fail = UINT64_MAX; bool any = false;
                for (int k = 1; k < 4; k++) if (e.n_seeds[k]) { fail = std::min(fail, e.first_seed[k]); any = true; }
                if (e.n_seeds[0] && any) out.push_back(Mixed{e.set, e.first_seed[0], fail});
            }
            return out;
        }
        // a greedy set cover of every reached vocabulary value — each round the entry that adds the most new values, ties to the smaller
        // set word —: one seed (its smallest) per chosen entry, ascending and unique, ready for over_seeds()
        std::vector<uint64_t> cover() const {
            const uint64_t vmask = (1ull << vocabulary.size()) - 1;      // (at most 62 values)
            uint64_t missing = 0;
            for (const madsim_probe_set_t& e : sets) missing |= e.set & vmask;
            std::vector<uint64_t> chosen;
            while (missing) {
                const madsim_probe_set_t* best = nullptr;
                for (const madsim_probe_set_t& e : sets)                   // ascending by set word: the first of the best wins
                    if (!best || __builtin_popcountll(e.set & missing) > __builtin_popcountll(best->set & missing)) best = &e;
                uint64_t s = UINT64_MAX;
                for (int k = 0; k < 4; k++) if (best->n_seeds[k]) s = std::min(s, best->first_seed[k]);
                chosen.push_back(s);
                missing &= ~best->set;
            }
            std::sort(chosen.begin(), chosen.end());
            chosen.erase(std::unique(chosen.begin(), chosen.end()), chosen.end());
            return chosen;
        }
    };
    ProbeSets probe_sets(const Workload& wl, const std::vector<uint64_t>& vocabulary, uint32_t obs_cap = 256, uint64_t max_sets = 4096, uint32_t include = 0xf,
                         uint64_t chunk = 0) const {
        madsim::check(madsim_hip_init(device));
        madsim_workload_t w = wl.raw();
        madsim_config_t cfg = config.raw();
        madsim_limits_t lim0 = capacities;
        if (time_limit) { lim0.time_limit_ns = (uint64_t)(*time_limit * 1e9 + 0.5); if (!lim0.time_limit_ns) lim0.time_limit_ns = 1; }
        uint32_t rounds = 0;
        if (resolve_flags & MADSIM_CAMPAIGN_RESOLVE) {
            rounds = (resolve_flags & MADSIM_CAMPAIGN_RESOLVE_ROUNDS_MASK) >> MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT;
            if (!rounds) rounds = MADSIM_RESOLVE_DEFAULT_ROUNDS;
        }
        auto one = [&](const madsim_limits_t& lim, const std::vector<uint64_t>* list) {
            ProbeSets c;
            const uint64_t n = list ? list->size() : count;
            c.vocabulary = vocabulary;
            c.sets.resize(max_sets ? max_sets : 1);
            c.runner_seeds.resize(n ? n : 1);
            madsim_probe_sets_t& t = c.totals;
            t.include = include; t.obs_cap = obs_cap; t.vocab = vocabulary.data(); t.n_vocab = vocabulary.size(); t.sets = c.sets.data(); t.cap = max_sets;
            t.runner_seeds = c.runner_seeds.data(); t.runner_cap = n;
            madsim::check(list ? madsim_hip_probe_sets_seeds(&w, &cfg, list->data(), n, chunk, &lim, &t) : madsim_hip_probe_sets_range(&w, &cfg, seed, n, chunk, &lim, &t));
            c.sets.resize(t.n_sets);
            c.runner_seeds.resize(t.n_runner_listed);
            t.vocab = nullptr; t.sets = nullptr; t.runner_seeds = nullptr;
            return c;
        };
        ProbeSets c = one(lim0, listed_seeds ? &seed_list : nullptr);
        for (uint32_t r = 1; r <= rounds && !c.runner_seeds.empty(); r++) {
            madsim_limits_t lim = lim0;
            madsim::check(madsim_hip_grow_limits(&w, &lim0, r, &lim));
            const ProbeSets more = one(lim, &c.runner_seeds);
            std::vector<madsim_probe_set_t> merged;
            for (size_t i = 0, j = 0; i < c.sets.size() || j < more.sets.size();) {
                if (j >= more.sets.size() || (i < c.sets.size() && c.sets[i].set < more.sets[j].set)) merged.push_back(c.sets[i++]);
                else if (i >= c.sets.size() || more.sets[j].set < c.sets[i].set) merged.push_back(more.sets[j++]);
                else {
                    madsim_probe_set_t e = c.sets[i++];
                    const madsim_probe_set_t& o = more.sets[j++];
                    for (int k = 0; k < 4; k++) {
                        if (o.n_seeds[k]) e.first_seed[k] = e.n_seeds[k] ? std::min(e.first_seed[k], o.first_seed[k]) : o.first_seed[k];
                        e.n_seeds[k] += o.n_seeds[k];
                    }
                    merged.push_back(e);
                }
            }
            if (merged.size() > max_sets) throw Error(MADSIM_E_LIMITS, "probe_sets: more than max_sets distinct probe sets once the runner seeds are settled");
            c.sets.swap(merged);
            for (int k = 0; k < 4; k++) c.totals.n_counted[k] += more.totals.n_counted[k];
            c.totals.n_runner = more.totals.n_runner; c.totals.n_runner_listed = more.totals.n_runner_listed;
            c.totals.n_sets = c.sets.size();
            c.runner_seeds = more.runner_seeds;
        }
        return c;
    }

    // Which of the values of `vocabulary` (1 .. 32 distinct values) the builder's seeds reach FIRST, by verdict (madsim_hip_probe_order_range
    // / madsim_hip_probe_order_seeds): `seed .. seed + count`, or the over_seeds() list, run on the trace build and reduced on the device to
    // one record per non-empty cell (a, b) of vocabulary indices — a == b: the seeds that reached the value; a != b: those that reached both
    // and saw a first.  pairs: ascending by (a, b).  This builder's resolve_runner() rounds apply as in census().
    struct ProbeOrder {
        std::vector<uint64_t> vocabulary;
        std::vector<madsim_probe_order_pair_t> pairs;
        madsim_probe_order_t totals{};             // the counts (the pointers and caps are the call's own: not meaningful here)
        std::vector<uint64_t> runner_seeds;
        size_t index(uint64_t value) const {                            // the vocabulary index of a value; throws on any other value
            auto it = std::find(vocabulary.begin(), vocabulary.end(), value);
            if (it == vocabulary.end()) throw Error(MADSIM_E_ARG, "probe_order: a value that is not in the vocabulary");
            return (size_t)(it - vocabulary.begin());
        }
        const madsim_probe_order_pair_t* cell(uint64_t a, uint64_t b) const {      // the record of cell (a, b) of VALUES, or nullptr: no seed in it
            const size_t ia = index(a), ib = index(b);
            for (const madsim_probe_order_pair_t& e : pairs) if (e.a == ia && e.b == ib) return &e;
            return nullptr;
        }
        // counted seeds of the verdicts in `verdicts` (a bit mask) that reached both and saw `a` first (a == b: that reached a)
        uint64_t before(uint64_t a, uint64_t b, uint32_t verdicts = 0xf) const {
            const madsim_probe_order_pair_t* e = cell(a, b);
            uint64_t n = 0;
            for (int k = 0; e && k < 4; k++) if ((verdicts >> k) & 1u) n += e->n_seeds[k];
            return n;
        }
        uint64_t reached(uint64_t a, uint32_t verdicts = 0xf) const { return before(a, a, verdicts); }
        uint64_t both(uint64_t a, uint64_t b, uint32_t verdicts = 0xf) const { return a == b ? reached(a, verdicts) : before(a, b, verdicts) + before(b, a, verdicts); }
        uint64_t without(uint64_t a, uint64_t b, uint32_t verdicts = 0xf) const { return reached(a, verdicts) - both(a, b, verdicts); }
        bool always_before(uint64_t a, uint64_t b, uint32_t verdicts = 0xf) const { return a != b && both(a, b, verdicts) > 0 && before(b, a, verdicts) == 0; }
    };
    ProbeOrder probe_order(const Workload& wl, const std::vector<uint64_t>& vocabulary, uint32_t obs_cap = 256, uint32_t include = 0xf, uint64_t chunk = 0) const {
        madsim::check(madsim_hip_init(device));
        madsim_workload_t w = wl.raw();
        madsim_config_t cfg = config.raw();
        madsim_limits_t lim0 = capacities;
        if (time_limit) { lim0.time_limit_ns = (uint64_t)(*time_limit * 1e9 + 0.5); if (!lim0.time_limit_ns) lim0.time_limit_ns = 1; }
        uint32_t rounds = 0;
        if (resolve_flags & MADSIM_CAMPAIGN_RESOLVE) {
            rounds = (resolve_flags & MADSIM_CAMPAIGN_RESOLVE_ROUNDS_MASK) >> MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT;
            if (!rounds) rounds = MADSIM_RESOLVE_DEFAULT_ROUNDS;
        }
        const uint64_t cap = vocabulary.size() * vocabulary.size();
        auto one = [&](const madsim_limits_t& lim, const std::vector<uint64_t>* list) {
            ProbeOrder c;
            const uint64_t n = list ? list->size() : count;
            c.vocabulary = vocabulary;
            c.pairs.resize(cap ? cap : 1);
            c.runner_seeds.resize(n ? n : 1);
            madsim_probe_order_t& t = c.totals;
            t.include = include; t.obs_cap = obs_cap; t.vocab = vocabulary.data(); t.n_vocab = vocabulary.size(); t.pairs = c.pairs.data(); t.cap = cap;
            t.runner_seeds = c.runner_seeds.data(); t.runner_cap = n;
            madsim::check(list ? madsim_hip_probe_order_seeds(&w, &cfg, list->data(), n, chunk, &lim, &t) : madsim_hip_probe_order_range(&w, &cfg, seed, n, chunk, &lim, &t));
            c.pairs.resize(t.n_pairs);
            c.runner_seeds.resize(t.n_runner_listed);
            t.vocab = nullptr; t.pairs = nullptr; t.runner_seeds = nullptr;
            return c;
        };
        ProbeOrder c = one(lim0, listed_seeds ? &seed_list : nullptr);
        const auto key = [](const madsim_probe_order_pair_t& e) { return (uint64_t)e.a << 32 | e.b; };
        for (uint32_t r = 1; r <= rounds && !c.runner_seeds.empty(); r++) {
            madsim_limits_t lim = lim0;
            madsim::check(madsim_hip_grow_limits(&w, &lim0, r, &lim));
            const ProbeOrder more = one(lim, &c.runner_seeds);
            std::vector<madsim_probe_order_pair_t> merged;
            for (size_t i = 0, j = 0; i < c.pairs.size() || j < more.pairs.size();) {
                if (j >= more.pairs.size() || (i < c.pairs.size() && key(c.pairs[i]) < key(more.pairs[j]))) merged.push_back(c.pairs[i++]);
                else if (i >= c.pairs.size() || key(more.pairs[j]) < key(c.pairs[i])) merged.push_back(more.pairs[j++]);
                else {
                    madsim_probe_order_pair_t e = c.pairs[i++];
                    const madsim_probe_order_pair_t& o = more.pairs[j++];
                    for (int k = 0; k < 4; k++) {
                        if (o.n_seeds[k]) e.first_seed[k] = e.n_seeds[k] ? std::min(e.first_seed[k], o.first_seed[k]) : o.first_seed[k];
                        e.n_seeds[k] += o.n_seeds[k];
                    }
                    merged.push_back(e);
                }
            }
            c.pairs.swap(merged);
            for (int k = 0; k < 4; k++) { c.totals.n_counted[k] += more.totals.n_counted[k]; c.totals.n_none[k] += more.totals.n_none[k]; }
            c.totals.n_truncated += more.totals.n_truncated;
            c.totals.n_runner = more.totals.n_runner; c.totals.n_runner_listed = more.totals.n_runner_listed;
            c.totals.n_pairs = c.pairs.size();
            c.runner_seeds = more.runner_seeds;
        }
        return c;
    }

    // When the listed seeds traced what they traced (madsim_hip_timeline_seeds): the values trace_seeds returns and, beside each, the runtime's
    // elapsed nanoseconds at that observation — what trace_instant would have folded there.  `observations` and `times` hold the first obs_cap
    // entries, n_observations says how many there were.  The builder's resolve_runner() rounds replay seeds with a runner verdict, as trace_seeds does.
    struct SeedTimeline {
        uint64_t seed = 0;
        madsim_result_t result{};
        std::vector<uint64_t> observations, times;
        uint64_t n_observations = 0;
    };
    std::vector<SeedTimeline> timeline(const Workload& wl, const std::vector<uint64_t>& seeds, size_t obs_cap = 256) const {
        madsim::check(madsim_hip_init(device));
        madsim_workload_t w = wl.raw();
        madsim_config_t cfg = config.raw();
        madsim_limits_t lim0 = capacities;
        if (time_limit) { lim0.time_limit_ns = (uint64_t)(*time_limit * 1e9 + 0.5); if (!lim0.time_limit_ns) lim0.time_limit_ns = 1; }
        std::vector<SeedTimeline> out(seeds.size());
        std::vector<size_t> idx(seeds.size());
        for (size_t i = 0; i < idx.size(); i++) idx[i] = i;
        const uint32_t rounds = resolve_rounds();
        for (uint32_t r = 0; r <= rounds && !idx.empty(); r++) {
            madsim_limits_t lim = lim0;
            if (r) madsim::check(madsim_hip_grow_limits(&w, &lim0, r, &lim));
            const size_t m = idx.size();
            std::vector<uint64_t> s(m), obs(m * obs_cap), tim(m * obs_cap), lens(m);
            std::vector<madsim_result_t> res(m);
            for (size_t j = 0; j < m; j++) s[j] = seeds[idx[j]];
            madsim::check(madsim_hip_timeline_seeds(&w, &cfg, s.data(), m, &lim, obs.data(), tim.data(), obs_cap, lens.data(), res.data()));
            std::vector<size_t> again;
            const uint32_t cap = lim.max_steps ? lim.max_steps : 1u << 24, ceiling = lim.max_steps_ceiling ? lim.max_steps_ceiling : 1u << 28;
            for (size_t j = 0; j < m; j++) {
                SeedTimeline& t = out[idx[j]];
                const size_t k = (size_t)std::min<uint64_t>(lens[j], obs_cap);
                t.seed = s[j]; t.result = res[j]; t.n_observations = lens[j];
                t.observations.assign(obs.begin() + j * obs_cap, obs.begin() + j * obs_cap + k);
                t.times.assign(tim.begin() + j * obs_cap, tim.begin() + j * obs_cap + k);
                if (res[j].verdict == MADSIM_OVERFLOW || (res[j].verdict == MADSIM_STEP_LIMIT && cap < ceiling)) again.push_back(idx[j]);
            }
            idx.swap(again);
        }
        return out;
    }

    // How long, in virtual nanoseconds, from the first traced `from` to the first `to` behind it over the builder's seeds
    // (madsim_hip_probe_spans_range / madsim_hip_probe_spans_seeds): `seed .. seed + count`, or the over_seeds() list, run on the trace build
    // with the time log and reduced on the device to one record per definition.  Span::start(to) begins at the start of the run.  This
    // builder's resolve_runner() rounds apply as in census().
    struct Span {
        static madsim_span_def_t between(uint64_t from, uint64_t to) { return madsim_span_def_t{from, to, 0, 0}; }
        static madsim_span_def_t start(uint64_t to) { return madsim_span_def_t{0, to, MADSIM_SPAN_FROM_START, 0}; }
    };
    struct ProbeSpans {
        std::vector<madsim_span_def_t> definitions;
        std::vector<madsim_span_t> spans;          // one per definition, in that order
        madsim_probe_spans_t totals{};             // the counts (the pointers and caps are the call's own: not meaningful here)
        std::vector<uint64_t> runner_seeds;
        uint64_t closed(size_t i) const { return spans[i].n; }
        uint64_t state(size_t i, uint32_t st, uint32_t verdicts = 0xf) const {      // counted seeds of span i in MADSIM_SPAN_* state st
            uint64_t n = 0;
            for (int k = 0; k < 4; k++) if ((verdicts >> k) & 1u) n += spans[i].n_state[4 * k + st];
            return n;
        }
        long double mean(size_t i) const { return spans[i].n ? ((long double)spans[i].sum_hi * 18446744073709551616.0L + (long double)spans[i].sum_lo) / (long double)spans[i].n : 0.0L; }
        // lo <= the q-quantile (nearest rank) of span i's durations <= hi: its bucket of the histogram, narrowed by the exact min and max
        std::pair<uint64_t, uint64_t> quantile_bounds(size_t i, double q) const {
            const madsim_span_t& s = spans[i];
            if (!s.n) throw Error(MADSIM_E_ARG, "quantile_bounds: no seed closed this span");
            uint64_t rank = (uint64_t)std::ceil(q * (double)s.n), acc = 0;
            if (rank < 1) rank = 1;
            if (rank > s.n) rank = s.n;
            for (uint32_t b = 0; b < MADSIM_STAT_BUCKETS; b++) {
                acc += s.hist[b];
                if (acc >= rank) {
                    const uint64_t lo = madsim_hip_stat_bucket_floor(b), next = madsim_hip_stat_bucket_floor(b + 1);
                    return {std::max(lo, s.min), std::min(next == UINT64_MAX ? next : next - 1, s.max)};
                }
            }
            return {s.min, s.max};
        }
        std::optional<uint64_t> slowest(size_t i) const { return spans[i].n ? std::optional<uint64_t>(spans[i].max_seed) : std::nullopt; }
        std::optional<uint64_t> fastest(size_t i) const { return spans[i].n ? std::optional<uint64_t>(spans[i].min_seed) : std::nullopt; }
        std::optional<uint64_t> never_closed(size_t i) const { return state(i, MADSIM_SPAN_OPEN) ? std::optional<uint64_t>(spans[i].first_open_seed) : std::nullopt; }
    };
    ProbeSpans probe_spans(const Workload& wl, const std::vector<madsim_span_def_t>& definitions, uint32_t obs_cap = 256, uint32_t include = 0xf, uint64_t chunk = 0) const {
        madsim::check(madsim_hip_init(device));
        madsim_workload_t w = wl.raw();
        madsim_config_t cfg = config.raw();
        madsim_limits_t lim0 = capacities;
        if (time_limit) { lim0.time_limit_ns = (uint64_t)(*time_limit * 1e9 + 0.5); if (!lim0.time_limit_ns) lim0.time_limit_ns = 1; }
        const uint32_t rounds = resolve_rounds();
        auto one = [&](const madsim_limits_t& lim, const std::vector<uint64_t>* list) {
            ProbeSpans c;
            const uint64_t n = list ? list->size() : count;
            c.definitions = definitions;
            c.spans.resize(definitions.size() ? definitions.size() : 1);
            c.runner_seeds.resize(n ? n : 1);
            madsim_probe_spans_t& t = c.totals;
            t.include = include; t.obs_cap = obs_cap; t.defs = definitions.data(); t.n_spans = definitions.size(); t.spans = c.spans.data();
            t.runner_seeds = c.runner_seeds.data(); t.runner_cap = n;
            madsim::check(list ? madsim_hip_probe_spans_seeds(&w, &cfg, list->data(), n, chunk, &lim, &t) : madsim_hip_probe_spans_range(&w, &cfg, seed, n, chunk, &lim, &t));
            c.spans.resize(definitions.size());
            c.runner_seeds.resize(t.n_runner_listed);
            t.defs = nullptr; t.spans = nullptr; t.runner_seeds = nullptr;
            return c;
        };
        ProbeSpans c = one(lim0, listed_seeds ? &seed_list : nullptr);
        for (uint32_t r = 1; r <= rounds && !c.runner_seeds.empty(); r++) {
            madsim_limits_t lim = lim0;
            madsim::check(madsim_hip_grow_limits(&w, &lim0, r, &lim));
            const ProbeSpans more = one(lim, &c.runner_seeds);
            for (size_t i = 0; i < c.spans.size(); i++) madsim_hip_span_merge(&c.spans[i], &more.spans[i]);
            for (int k = 0; k < 4; k++) c.totals.n_counted[k] += more.totals.n_counted[k];
            c.totals.n_truncated += more.totals.n_truncated;
            c.totals.n_runner = more.totals.n_runner; c.totals.n_runner_listed = more.totals.n_runner_listed;
            c.runner_seeds = more.runner_seeds;
        }
        return c;
    }

    // Where the two runs part: this builder's run of `wl` (side A) against `other`'s run of `other_wl` (side B) over `seeds` (any order,
    // duplicates allowed), compared on the device on the determinism log and on the observations (madsim_hip_diverge_seeds): per seed the
    // record, the up to `window` observations both runs made just before they part, and the up to `window` each side made from there on.
    // No row travels to the host.  This builder's resolve_runner() rounds apply: seeds that come back incomparable with a re-runnable
    // runner verdict on either side are replayed in one further call per round, each side under its own madsim_hip_grow_limits(.., r).
    struct Divergence {
        madsim_divergence_t rec{};
        std::vector<uint64_t> shared, next_a, next_b;
    };
    std::vector<Divergence> diverge_against(const Builder& other, const std::vector<uint64_t>& seeds, const Workload& wl, const Workload& other_wl,
                                            size_t log_cap = 65536, size_t obs_cap = 256, uint32_t window = 4) const {
        madsim::check(madsim_hip_init(device));
        madsim_workload_t wa = wl.raw(), wb = other_wl.raw();
        madsim_config_t ca = config.raw(), cb = other.config.raw();
        madsim_limits_t la0 = capacities, lb0 = other.capacities;
        if (time_limit) { la0.time_limit_ns = (uint64_t)(*time_limit * 1e9 + 0.5); if (!la0.time_limit_ns) la0.time_limit_ns = 1; }
        if (other.time_limit) { lb0.time_limit_ns = (uint64_t)(*other.time_limit * 1e9 + 0.5); if (!lb0.time_limit_ns) lb0.time_limit_ns = 1; }
        std::vector<Divergence> out(seeds.size());
        std::vector<size_t> idx(seeds.size());
        for (size_t i = 0; i < idx.size(); i++) idx[i] = i;
        uint32_t rounds = 0;
        if (resolve_flags & MADSIM_CAMPAIGN_RESOLVE) {
            rounds = (resolve_flags & MADSIM_CAMPAIGN_RESOLVE_ROUNDS_MASK) >> MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT;
            if (!rounds) rounds = MADSIM_RESOLVE_DEFAULT_ROUNDS;
        }
        for (uint32_t r = 0; r <= rounds && !idx.empty(); r++) {
            madsim_limits_t la = la0, lb = lb0;
            if (r) { madsim::check(madsim_hip_grow_limits(&wa, &la0, r, &la)); madsim::check(madsim_hip_grow_limits(&wb, &lb0, r, &lb)); }
            const size_t m = idx.size();
            std::vector<uint64_t> s(m), ctx(m * 3 * window);
            std::vector<madsim_divergence_t> recs(m);
            for (size_t j = 0; j < m; j++) s[j] = seeds[idx[j]];
            madsim::check(madsim_hip_diverge_seeds(&wa, &ca, &la, &wb, &cb, &lb, s.data(), m, log_cap, obs_cap, window, recs.data(), window ? ctx.data() : nullptr));
            std::vector<size_t> again;
            auto rerunnable = [](const madsim_result_t& x, const madsim_limits_t& lim) {
                const uint32_t cap = lim.max_steps ? lim.max_steps : 1u << 24, ceiling = lim.max_steps_ceiling ? lim.max_steps_ceiling : 1u << 28;
                return x.verdict == MADSIM_OVERFLOW || (x.verdict == MADSIM_STEP_LIMIT && cap < ceiling);
            };
            for (size_t j = 0; j < m; j++) {
                Divergence& d = out[idx[j]];
                d.rec = recs[j];
                d.shared.clear(); d.next_a.clear(); d.next_b.clear();
                if (d.rec.obs_status != MADSIM_DIVERGE_INCOMPARABLE) {
                    const uint64_t at = d.rec.obs_at, w = window;
                    const uint64_t ka = std::min<uint64_t>(d.rec.obs_len_a, obs_cap), kb = std::min<uint64_t>(d.rec.obs_len_b, obs_cap);
                    const uint64_t* row = ctx.data() + j * 3 * w;
                    d.shared.assign(row + (w - std::min(at, w)), row + w);
                    d.next_a.assign(row + w, row + w + (ka > at ? std::min(w, ka - at) : 0));
                    d.next_b.assign(row + 2 * w, row + 2 * w + (kb > at ? std::min(w, kb - at) : 0));
                }
                if (rerunnable(recs[j].a, la) || rerunnable(recs[j].b, lb)) again.push_back(idx[j]);
            }
            idx.swap(again);
        }
        return out;
    }

    // builder.rs:121-162: run seeds seed..seed+count; return on success, "panic" on the first failing seed.
    // Reports the numerically smallest failing seed (the reference reports the first to complete).
    std::vector<madsim_result_t> run(const Workload& wl) const {
        madsim::check(madsim_hip_init(device));
        madsim_workload_t w = wl.raw();
        madsim_config_t cfg = config.raw();
        madsim_limits_t lim = capacities;
        // Some(Duration::ZERO) is a limit too (panics at the first idle advance); 0 means None in the C-ABI
        if (time_limit) { lim.time_limit_ns = (uint64_t)(*time_limit * 1e9 + 0.5); if (!lim.time_limit_ns) lim.time_limit_ns = 1; }
        if (check) {                                   // Runtime::check_determinism (runtime/mod.rs:178-202)
            std::vector<uint8_t> l1(1 << 20), l2(1 << 20);
            madsim_result_t r1{}, r2{};
            madsim_limits_t nolim = capacities;           // check_determinism never sets a time limit (runtime/mod.rs:178-202)
            int64_t n1 = madsim_hip_trace_seed(&w, &cfg, seed, &nolim, l1.data(), l1.size(), &r1);
            int64_t n2 = madsim_hip_trace_seed(&w, &cfg, seed, &nolim, l2.data(), l2.size(), &r2);
            if (n1 < 0) madsim::check((int)n1);
            if (n2 < 0) madsim::check((int)n2);
            size_t n = (size_t)(n1 < (int64_t)l1.size() ? n1 : (int64_t)l1.size());
            if (n1 != n2 || std::memcmp(l1.data(), l2.data(), n) != 0) {
                panic_with_info(seed);
                throw std::runtime_error("non-determinism detected");
            }
            if (r1.verdict != MADSIM_PASS) { panic_with_info(seed); throw SimulationFailure(seed, r1); }
            return {r1};
        }
        std::vector<madsim_result_t> out(count);
        madsim_summary_t s{};
        madsim::check(madsim_hip_run_batch_auto(&w, &cfg, seed, count, &lim, out.data(), &s, 6));   // runner verdicts are re-run
        if (s.n_failed) {
            auto runner = [](uint32_t v) { return MADSIM_IS_RUNNER_VERDICT(v); };
            // a genuine test failure wins over unresolved runner limits: the first failing seed and its note are never hidden
            for (uint64_t i = 0; i < count; i++)
                if (out[i].verdict != MADSIM_PASS && !runner(out[i].verdict)) { panic_with_info(seed + i); throw SimulationFailure(seed + i, out[i]); }
            uint64_t i = 0;
            while (!runner(out[i].verdict)) i++;
            // a capacity / step-cap verdict that survived the re-runs is the runner's limit, not the test's failure
            throw Error(MADSIM_E_LIMITS, "seed " + std::to_string(seed + i) + ": " + SimulationFailure::verdict_name(out[i].verdict) + " (a runner verdict, not a test failure) persists after re-runs with larger limits");
        }
        return out;
    }
};

}  // namespace runtime
}  // namespace madsim

#endif
