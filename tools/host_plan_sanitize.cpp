// Host-only sanitizer run of the planner (madsim_amd/csrc/geometry.h): validate, make_geometry and build_tables over single-field mutations of
// a small workload — every opcode in every slot, operands at and past their ranges — the inputs most likely to index out of range.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/host_plan_sanitize.cpp -o /tmp/host_plan_sanitize && /tmp/host_plan_sanitize
// Any report aborts; otherwise it prints how many mutants each function saw.  No GPU, no Python.
#include <cstdint>
#include <cstdio>
struct uint4 { uint32_t x, y, z, w; };          // the one HIP type sim_kernel.h names (as a pointer's target only)
#include "../madsim_amd/csrc/geometry.h"

int main() {
    using namespace madsim_geo;
    // three programs on two nodes: a scope with a connection, a ticker with a select, a loop with a typed call, an IPVS service
    const madsim_insn_t base[] = {
        {MS_OP_SPAWN, 1, 0, 0}, {MS_OP_SPAWN, 2, 0, 0}, {MS_OP_MARK, 0, 0, 0}, {MS_OP_SET, 0, 0, 2}, {MS_OP_SLEEP, 0, 0, 1000000}, {MS_OP_DJNZ, 0, 4, 0},
        {MS_OP_TIMEOUT_BEGIN, 0, 9, 5000000}, {MS_OP_CONNECT, 0, 1, 0}, {MS_OP_CSEND, 0, 0, 7}, {MS_OP_TIMEOUT_END, 0, 0, 0},
        {MS_OP_RPC_CALL, 0, 0x8001, 0}, {MS_OP_IPVS, MADSIM_IPVS_ADD_SERVER, 0, 1}, {MS_OP_KILL, 2, 0, 0}, {MS_OP_JOIN, 1, 0, 0}, {MS_OP_DONE, 0, 0, 0},
        {MS_OP_BIND, 1, 0, 0}, {MS_OP_INTERVAL, 0, 0, 1000000}, {MS_OP_RECV_OR_TICK, 1, 0x0100, 0}, {MS_OP_TICK, 0, 0, 0}, {MS_OP_ACCEPT, 1, 0, 0}, {MS_OP_DONE, 0, 0, 0},
        {MS_OP_BIND, 2, 0, 0}, {MS_OP_RECV_TIMEOUT, 2, 0x0101, 500}, {MS_OP_SLEEP_RAND, 1, 1, 0}, {MS_OP_SEND, 2, 0x0101, 3}, {MS_OP_DONE, 0, 0, 0}};
    const uint32_t n = sizeof base / sizeof *base;
    madsim_prog_t progs[3] = {{0, 0, 0}, {1, 0, 15}, {2, 0, 21}};
    madsim_sock_t socks[4] = {{1, MADSIM_ADDR_IP, 9}, {1, MADSIM_ADDR_IP, 1}, {2, MADSIM_ADDR_IP, 1}, {1, MADSIM_ADDR_VIRTUAL, 80}};
    madsim_node_t nodes[3] = {};
    madsim_service_t svc[1] = {};
    svc[0].vaddr = 3; svc[0].n_servers = 1; svc[0].servers[0] = 1;
    madsim_insn_t insns[sizeof base / sizeof *base];
    madsim_workload_t w{};
    w.n_nodes = 2; w.n_progs = 3; w.n_socks = 4; w.n_insns = n; w.nodes = nodes; w.progs = progs; w.socks = socks; w.insns = insns;
    w.n_services = 1; w.services = svc;
    const madsim_config_t cfg = probe_config();
    unsigned long seen = 0, valid = 0, planned = 0, tabled = 0;
    std::string err;
    auto plan = [&] {
        seen++;
        if (validate(&w, &cfg, &err)) return;
        valid++;
        for (uint32_t sm = 0; sm < 4; sm++) for (int trace = 0; trace < 2; trace++) {
            madsim_limits_t lim{}; lim.state_mem = sm | MADSIM_STATE_NARROW_HEAP;
            Geo G;
            planned += make_geometry(Device(), &w, &cfg, &lim, 65, &G, &err, trace != 0) == 0;
        }
        DeviceTables T;
        tabled += build_tables(&w, &T, &err) == 0;
    };
    memcpy(insns, base, sizeof base);
    plan();
    if (valid != 1 || planned == 0 || tabled != 1) { fprintf(stderr, "the unmutated workload is refused: %s\n", err.c_str()); return 1; }
    const uint32_t edge8[] = {0, 1, 2, 3, 4, 5, 7, 8, 31, 32, 255}, edge16[] = {0, 1, 2, 3, 4, 5, n - 1, n, 0x00ff, 0x0100, 0x01ff, 0x7f01, 0x8001, 0xfe01, 0xff01, 0xffff};
    const uint32_t edge32[] = {0, 1, 4, 0x100, 999999999u, 1000000000u, 0x7fffffffu, 0xffffffffu};
    for (uint32_t i = 0; i < n; i++) {
        for (uint32_t op = 0; op < 256; op++) { memcpy(insns, base, sizeof base); insns[i].op = (uint8_t)op; plan(); }
        for (uint32_t v : edge8) { memcpy(insns, base, sizeof base); insns[i].a = (uint8_t)v; plan(); }
        for (uint32_t v : edge16) { memcpy(insns, base, sizeof base); insns[i].b = (uint16_t)v; plan(); }
        for (uint32_t v : edge32) { memcpy(insns, base, sizeof base); insns[i].imm = v; plan(); }
    }
    memcpy(insns, base, sizeof base);
    for (uint32_t p = 0; p < 3; p++) for (uint32_t f = 0; f < 256; f++) { const madsim_prog_t keep = progs[p]; progs[p].flags = (uint8_t)f; plan(); progs[p] = keep; }
    for (uint32_t k = 0; k < 3; k++) for (uint32_t f = 0; f < 256; f++) { nodes[k].flags = (uint8_t)f; plan(); nodes[k].flags = 0; }
    for (uint32_t k = 0; k < 4; k++) for (uint32_t v = 0; v < 5; v++) {
        const madsim_sock_t keep = socks[k];
        socks[k].kind = (uint8_t)v; plan(); socks[k] = keep;
        socks[k].node = (uint8_t)v; plan(); socks[k] = keep;
        socks[k].port = (uint16_t)v; plan(); socks[k] = keep;
    }
    for (uint32_t v = 0; v < 256; v++) { const madsim_service_t keep = svc[0]; svc[0].vaddr = (uint8_t)(v & 7); svc[0].n_servers = (uint8_t)v; svc[0].servers[0] = (uint8_t)(v >> 3 & 7); plan(); svc[0] = keep; }
    w.n_insns = n - 1; plan(); w.n_insns = n;
    printf("%lu mutants: validate accepted %lu, make_geometry planned %lu launches of them, build_tables %lu\n", seen, valid, planned, tabled);
    return 0;
}
