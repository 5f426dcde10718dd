// sim_kernel.h — kernel parameter block shared by the host side (madsim_hip.cpp) and sim_kernel.hip.
#ifndef MADSIM_SIM_KERNEL_H
#define MADSIM_SIM_KERNEL_H

#include <stdint.h>

#include "../../include/madsim_hip.h"

#define MADSIM_RUNNING 0xffu /* lane-internal: seed still executing */

/* classes of extended ops a kernel variant may carry (Variant<..., FEAT, ...>, KParams.features) */
#define MADSIM_FEAT_TIME 1  /* timeout(recv_from), t0 family (mark / sleep_until / assert_elapsed), advance, trace_time */
#define MADSIM_FEAT_CHAN 2  /* connect1 / accept1 / channel send + recv                                               */
#define MADSIM_FEAT_RPC  4  /* typed RPC call / reply                                                                   */
#define MADSIM_FEAT_NODE 8  /* kill / restart / pause / resume / abort / is_exit, init programs, restart_on_panic       */
#define MADSIM_FEAT_ADDR 16 /* general address resolution (network.rs:272-313): 0.0.0.0 / 127.0.0.1 entries, IP-less nodes, several
                               table entries naming one address.  Builds without it take every address for a distinct node IP.   */
#define MADSIM_FEAT_ALL  31
/* Variant<..., FEAT, ...> only, never in KParams.features: a base-op build without the determinism-log fold (rng_log), selected
   by KParams.no_log.  The other builds test KParams.no_log at run time (a wave-uniform branch); the base-op builds on full waves
   are issue-bound, so they get a twin compiled without the code instead. */
#define MADSIM_FEAT_NOLOG 32
/* Variant<..., FEAT, ...> only: the COMPACT base-op build (KParams.compact) — a fourth wave per SIMD for small workloads.
   A 4-wave workgroup may hold 40 960 bytes of LDS if four are to share a CU; the 4-node ping-pong's 200 bytes per seed make
   it 51 200.  The compact layout gets it to 152: timer-heap entries of 8 bytes (the low 32 bits of the deadline + meta: exact
   while every live deadline lies within 2^31 ns of the clock, which the host checks against the workload's longest sleep), the
   heap's root in registers, and the main task's state — polled a handful of times per run — in global memory. */
#define MADSIM_FEAT_COMPACT 64
/* Variant<..., FEAT, ...> only: global-state builds with NARROW timer-heap entries (KParams.narrow, madsim_limits_t.state_mem |
   MADSIM_STATE_NARROW_HEAP): every heap entry — in LDS and in the spill region — is 8 bytes {low deadline word, meta} instead of 16
   {deadline, meta, payload}; the 32-bit payload and the tag / sender fields of a datagram delivery (a fifth of the entries) live in a
   per-seed record pool in global memory, written once by the push and read once when the entry is the root (k_timer.h).  Twice
   the heap levels per LDS byte, half the bytes per spilled level.  Exact while every live deadline lies within 2^31 ns of the clock:
   checked per push on the device (a violation is a capacity verdict: the re-run uses the wide entries). */
#define MADSIM_FEAT_NARROW 128
/* The timer-op tiers, kept OUT of MADSIM_FEAT_ALL so that every other workload selects the build it selected before.  Each tier is
   the one before it plus one op family, and its workloads run on four builds of their own (MADSIM_TIER_VARIANTS), every class
   compiled in: timeout scopes (MS_OP_TIMEOUT_BEGIN / END), interval tickers (MS_OP_INTERVAL / TICK / INTERVAL_RESET), selects over a
   receive and a tick and timeout_at (MS_OP_RECV_OR_TICK / RECV_TIMEOUT_AT).  KParams.features carries the bits a workload's ops need;
   feature_tier() rounds them up to the tier. */
#define MADSIM_FEAT_SCOPE 256
#define MADSIM_FEAT_TICK 512
#define MADSIM_FEAT_SELECT 1024
#define MADSIM_FEAT_TIERS (MADSIM_FEAT_SCOPE | MADSIM_FEAT_TICK | MADSIM_FEAT_SELECT)
/* Ctrl-c signals (MS_OP_CTRL_C / SEND_CTRL_C / RECV_OR_CTRL_C).  Outside MADSIM_FEAT_ALL and outside MADSIM_FEAT_TIERS: a class of its own, not a
   timer-op tier.  Its workloads run on four builds of their own — MADSIM_TIER_VARIANTS' shapes with this mask alone, every class compiled
   in — so every other build compiles to what it was; validate() refuses a workload that mixes it with a timer-tier op (no combined build). */
#define MADSIM_FEAT_SIGNAL 2048
/* Global-state builds: identical wake-ups are fired as a batch (k_net.h timer_expire).  Sleep::poll registers ANOTHER timer with the same
   deadline and waker on every not-elapsed poll (time/sleep.rs:51-53), so more than half of the topology's heap entries are copies of an
   earlier one; copies leave the heap back to back, and every one after the first finds its task SCHEDULED already (or gone): a step
   each and nothing else.  The batch pops them without their callback's loads.  (The part of VERDICT r5 #1c that removes work.) */
#ifndef MADSIM_FIRE_COPIES
#define MADSIM_FIRE_COPIES 2        /* 1: a loop of its own behind the wake-up; 2: popped by the fire loop itself, in the other lanes' trips */
#endif
/* Builds with a spill region: BinaryHeap::pop written top-down (k_timer.h timer_pop) — the array sift_down_to_bottom + sift_up leave, without the
   levels below the moved entry's final slot. */
/* Base-op builds that keep the determinism log: the ready-queue draw starts from the number the previous with()'s log entry computed (k_rng.h gen_index). */
#ifndef MADSIM_RNG_PEEK
#define MADSIM_RNG_PEEK 2        /* 1: the ready-queue draw only; 2: every with() whose accepted output is not needed behind its loop */
#endif
#ifndef MADSIM_RNG_PEEK_LIFE
#define MADSIM_RNG_PEEK_LIFE 0   /* ... in the extended builds too */
#endif
/* Base-op builds that keep the determinism log: the xor-fold of the clock that every log entry carries is held in a lane register,
   computed once per pass where the ready-queue draw begins (k_rng.h ClockFold) — the clock does not move between the with()s of one poll there. */
#ifndef MADSIM_CLOCK_FOLD
#define MADSIM_CLOCK_FOLD 1
#endif
/* Register-ready-queue builds: a wave whose lanes all hold ONE queued task pops it without swap_remove's shifts (k_main.h; the vote is the one
   gen_index needs anyway). */
#ifndef MADSIM_POP_ONE
#define MADSIM_POP_ONE 1
#endif
/* Base-op builds: launch parameters that are read once per seed, once per many passes or on rare sides only are loaded from the kernel-argument
   segment where they are used (k_state.h ColdParams / PCOLD) instead of being held in scalar registers for the wave's whole life, where they pushed
   values the pass loop reads through spill lanes (v_readlane_b32 inside the loop). */
#ifndef MADSIM_COLD_PARAMS
#define MADSIM_COLD_PARAMS 1
#endif
/* Base-op builds: a launch whose mailboxes hold ONE registration and queue no message (mbox_regs = 1, mbox_msgs = MADSIM_LIMIT_NONE: the benchmark's
   limits, the compact layout's usual ones) delivers and registers in straight lines — no registration scan, no swap_remove of an entry onto itself, no
   message queue — behind one scalar test of the two launch parameters (k_state.h MboxOne; k_net.h mailbox_deliver_one, k_poll.h MS_OP_RECV). */
#ifndef MADSIM_MBOX_ONE
#define MADSIM_MBOX_ONE 1
#endif
/* MADSIM_STATE_DEDUP_TIMERS builds: the occupancy of the re-registration table mirrored in a register (k_timer.h dedup_note). */
#ifndef MADSIM_DEDUP_OCC
#define MADSIM_DEDUP_OCC 1
#endif
/* Extended builds: whether any clog exists is mirrored in the lane, a send loads the clog masks only then (k_channel.h net_try_send). */
#ifndef MADSIM_CLOG_MIRROR
#define MADSIM_CLOG_MIRROR 1
#endif
#ifndef MADSIM_POP_TOPDOWN
#define MADSIM_POP_TOPDOWN 1
#endif
/* ... with the LDS-resident levels walked before the heap's last entry (a spill-region load) has arrived (k_timer.h timer_pop). */
/* Narrow-heap global-state builds: a poll round requests the parent of the slot its first push will start from when it begins (k_timer.h
   timer_push_prefetch), beside its handler's own reads. */
#ifndef MADSIM_PUSH_PREFETCH
#define MADSIM_PUSH_PREFETCH 0        /* measured: topology 5.75 with, 5.76 without (profiles/r6_ab_chains.txt): the three registers cost what the round trip saves */
#endif
#ifndef MADSIM_POP_LDS_FIRST
#define MADSIM_POP_LDS_FIRST 1
#endif

namespace madsim_k {

struct KParams {
    // workload tables in device memory (copied into LDS by every workgroup)
    const uint4*    insns;     // {op|a<<8|b<<16, imm, fused assert value, fused post-chain word} (geometry.h build_tables)
    const uint32_t* progs;     // node | flags<<8 | entry<<16
    const uint32_t* socks;     // node | kind<<8 | port<<16 (a SocketAddr as one word)
    const uint32_t* nodes;     // n_nodetab words: per node its flags word; then (pm_off != 0) 8 words per node: the 256-bit row "a panic
                               // with message code c restarts this node"; then (n_services != 0) 2 words per IPVS service:
                               // vaddr | n_servers<<8 (| 0x80<<8: declared absent) | servers[0]<<16 | servers[1]<<24, servers[2..5]
    const uint64_t* dur_table; // per MS_OP_SLEEP_RAND (its `a` is rewritten to an index): {mode, low, range, zone}
    uint32_t n_insns, n_progs, n_socks, n_nodes;
    // net config (Bernoulli p_int, UniformDuration parameters precomputed on the host)
    uint64_t loss_pint; uint32_t loss_always; uint32_t buggify; uint64_t bug_pint;
    // (obs_time_words: the trace builds' time log, in the word that was padding here, so every field keeps its kernel-argument offset and the
    // block its size — beside every value kept in the observation log, at the same index of the unit's time row, the runtime's elapsed
    // nanoseconds at that observation (k_rng.h obs_fold).  The time rows lie in the observation log's own allocation: row i at obs_log +
    // obs_time_words + i * obs_cap, obs_time_words 64-bit words behind the observation row.  The observation log's rule: cap-guarded, the rows
    // zero-filled by the host, obs_len the one true length.  0 keeps nothing; never non-zero without obs_log)
    uint32_t lat_mode; uint32_t has_clog_link; uint32_t has_clog; uint32_t obs_time_words; uint64_t lat_low, lat_range, lat_zone;
    uint64_t loss_table_pint[4]; uint32_t loss_table_always[4];
    // MS_OP_SET_LATENCY (extended builds): madsim_config_t.lat_table as UniformDuration parameters; a lane keeps the index of its
    // current entry (Lane::loss_always bits 4-6: 0 = lat_* above) and sample_latency selects
    uint32_t uses_set_lat; uint32_t lat_tab_mode[4]; uint64_t lat_tab_low[4], lat_tab_range[4], lat_tab_zone[4];
    // limits
    uint64_t time_limit; uint32_t max_steps;
    // capacities
    uint32_t heap_lds, heap_spill, max_tasks, mbox_regs, mbox_msgs;
    uint32_t task_units, sock_words, lane_words, uniq_addr;
    uint32_t lw_shift;         // log2(seed-carrying lanes per wave): lane stride of every per-lane LDS array
    // LDS layout, in 32-bit words: workgroup-shared tables, heap units and task units (16-byte
    // aligned, [unit][lane]), then the 32-bit planes ([word][lane])
    uint32_t sh_insns, sh_progs, sh_socks, sh_nodes, sh_heap, sh_tasks, sh_planes;
    // a workgroup is waves_per_block independent waves (one per SIMD): the tables once, then one
    // [heap][tasks][planes] slice of wave_words per wave; sh_heap/sh_tasks/sh_planes are wave 0's
    uint32_t waves_per_block, wave_words;
    // per-lane plane offsets (in words)
    uint32_t off_ready, off_socks, off_handles, off_nodes, off_clog, off_pause, off_greg, off_conn, off_hooks;
    uint32_t n_nodetab, pm_off, svc_off, n_services;   // layout of the node table (word offsets from its start; 0 = absent)
    uint32_t ipvs_dyn;         // MS_OP_IPVS present: the services' server lists are per-seed state (k_state.h IPVSW), initialised from the table
    uint32_t panic_dyn_max;    // largest code a run-time formatted panic message may have (madsim_workload_t.panic_dyn_max)
    uint32_t off_ipvs;         // per-seed plane: one round-robin counter per IPVS service (net/ipvs.rs rr_index)
    uint32_t uses_eph;         // ephemeral Endpoint handles in the socket table (geometry.h device_socks)
    uint32_t uses_hooks;       // MS_OP_HOOK_REQ / MS_OP_HOOK_RSP present: one hook word per node
    uint32_t uses_chan, max_conns, chan_queue, conn_words;   // reliable channel (connect1/accept1) state, if used
    uint32_t chan_unit;            // index of the task unit holding the (tx, rx) pair state
    uint32_t uses_rpc, rpc_unit;   // typed RPC: index of the task unit holding the response tags
    uint32_t rq_in_reg;        // the ready queue needs no LDS region (register variant)
    // global-state builds (Variant::G): a lane's task table + planes are gs_stride logical bytes — [task units: max_tasks x
    // task_units x 16 B][plane words (off_* count from gs_planes, the ready queue stays in LDS)] — stored across the launch
    // as [unit][global lane] then [word][global lane] (k_state.h gs_addr_*): logical byte `at` of lane g lives at
    // at * total_lanes + g * 16 (units) or + g * 4 (words)
    uint32_t gstate_mode, gs_stride, gs_planes, gs_plane_words;
    uint32_t gs_gran_sh;         // log2 of a task slot's granule in the global block: [slot][lane][task_units x 16 bytes, padded to 2^gs_gran_sh]
    uint32_t off_amask, off_omask;     // LDS plane words (after the ready queue) of the alive-task / owned-socket masks
    uint8_t* gstate;
    uint32_t lifecycle;        // any extended op: the extended LDS layout (features != 0)
    uint32_t features;         // MADSIM_FEAT_* classes the workload needs
    uint32_t uses_pause, has_restart_on_panic, restart_nodes;   // restart_nodes: bit n = NodeBuilder::restart_on_panic
    // batch
    uint64_t seed0, count;
    const uint64_t* seed_list; // non-null: unit i runs seed_list[i] instead of seed0 + i (compacted re-run of overflowed seeds)
    madsim_result_t* out;
    unsigned long long* work_ctr; // non-null: a lane that finishes unit i pulls unit total_lanes + atomicAdd(work_ctr, 1) next
    uint4* spill;
    uint32_t total_lanes;
    // trace mode: one row of trace_cap bytes and one length word per unit (obs_log below)
    uint8_t* trace_log; uint64_t trace_cap; uint64_t* trace_len;
    uint32_t compact;          // base-op builds: the compact LDS layout (MADSIM_FEAT_COMPACT); gstate then holds the main tasks' records
    uint32_t no_log;           // madsim_limits_t.no_trace_hash: skip rng_log, report trace_hash = 0 (trace launches ignore it)
    // MADSIM_STATE_DEDUP_TIMERS (global-state timeout-only build): dedup_n (a power of two, 0 = off) 16-byte buckets
    // {deadline lo, hi, wake meta, count} behind the task units, at logical byte dedup_off of the lane's block (k_timer.h dedup_note)
    uint32_t dedup_n, dedup_off;
    // MADSIM_STATE_NARROW_HEAP (Variant::NH): 8-byte heap entries; pool_n (a multiple of 32) delivery records of 8 bytes {meta, payload}
    // behind the planes of the lane's global block, at logical byte pool_off ([record][global lane]); free / used mask = pool_n / 32 LDS
    // plane words from off_pmask
    uint32_t narrow, pool_n, pool_off, off_pmask;
    uint64_t* prof;            // profiling builds (tools/experiment): per-phase cycle accumulators
    uint32_t* iter_est;        // one word per workload: the passes a wave of it runs, as the last finished wave counted them (0 = nothing
                               // finished yet); null = no progress-based priority (k_main.h wave_progress_priority)
    uint32_t scope_unit;       // (last: the other fields keep their kernel-argument offsets) timeout scopes (MADSIM_FEAT_SCOPE): index of the task unit {END pc | active << 16 | made << 17, -, deadline lo, hi}
    uint32_t tick_unit;        // (after scope_unit, same reason) interval tickers (MADSIM_FEAT_TICK): index of the task unit {TICK_ACTIVE | behaviour << 1 | period s << 16, period ns, next deadline lo, hi};
                               // 0 = none (a select build's workload without MS_OP_INTERVAL)
    // trace builds (after tick_unit, same reason): the observation log — the values obs_hash folds, in execution order.  Unit i of a trace
    // launch writes its determinism log to trace_log + i * trace_cap, its observations to obs_log + i * obs_cap (64-bit words) and its
    // true lengths to trace_len[i] / obs_len[i]; a null obs_log or obs_cap == 0 stores no observation, a null obs_len no length
    uint64_t* obs_log; uint64_t obs_cap; uint64_t* obs_len;
    // trace builds (after obs_len, same reason): the task log — one word per task still alive when the unit's result is written
    // (include/madsim_hip.h "Task post-mortems"), in ascending slot order, to task_log + i * task_cap, the true count to task_len[i]; a null
    // task_log keeps nothing and walks nothing, a unit with a runner verdict writes no record and a count of 0
    uint64_t* task_log; uint64_t task_cap; uint64_t* task_len;
};

// The compiled builds, X(TRACE, SPILL, LWS, FEAT, RQ, G) = sim_kernel<Variant<...>>: the trace build; for base-op workloads on
// full 64-lane waves one build per (heap spill, register ready queue) combination plus a runtime-lane-stride build; single-class
// builds for workloads that only use timeouts (FEAT_TIME) or only the reliable channel (FEAT_CHAN) — a third of the code and
// fewer registers than the full build; the full build for every lane stride (64/32/16/8 seed lanes per wave, runtime);
// the global-state builds (G: task table + planes in global memory) of the three extended classes; then the timer-op tiers,
// each with the four shapes of MADSIM_TIER_VARIANTS: the trace build, the LDS-resident build (runtime lane stride) and the
// global-state builds (plain addresses, general resolution), every class compiled in; then the ctrl-c signal builds, the same four shapes.
#ifndef MADSIM_FOR_EACH_VARIANT      // (tools/ may compile a subset: -D'MADSIM_FOR_EACH_VARIANT(X)=X(false,false,6,0,true,false)')
#define MADSIM_TIER_VARIANTS(X, M)                                              \
    X(true, true, -1, MADSIM_FEAT_ALL | (M), false, false)                      \
    X(false, true, -1, MADSIM_FEAT_ALL | (M), false, false)                     \
    X(false, true, 6, (MADSIM_FEAT_ALL & ~MADSIM_FEAT_ADDR) | (M), false, true) \
    X(false, true, 6, MADSIM_FEAT_ALL | (M), false, true)
#define MADSIM_FOR_EACH_VARIANT(X)                     \
    X(true, true, -1, MADSIM_FEAT_ALL, false, false)   \
    X(false, false, 6, 0, false, false)                \
    X(false, false, 6, 0, true, false)                 \
    X(false, false, 6, MADSIM_FEAT_NOLOG, false, false) \
    X(false, false, 6, MADSIM_FEAT_NOLOG, true, false)  \
    X(false, false, 6, MADSIM_FEAT_COMPACT, true, false) \
    X(false, false, 6, MADSIM_FEAT_COMPACT | MADSIM_FEAT_NOLOG, true, false) \
    X(false, true, 6, 0, true, false)                  \
    X(false, true, 6, 0, false, false)                 \
    X(false, true, -1, 0, false, false)                \
    X(false, true, -1, MADSIM_FEAT_TIME, false, false) \
    X(false, true, -1, MADSIM_FEAT_CHAN, false, false) \
    X(false, false, 6, MADSIM_FEAT_ALL, false, false)  \
    X(false, true, 6, MADSIM_FEAT_ALL, false, false)   \
    X(false, true, 5, MADSIM_FEAT_ALL, false, false)   \
    X(false, true, 4, MADSIM_FEAT_ALL, false, false)   \
    X(false, true, 3, MADSIM_FEAT_ALL, false, false)   \
    X(false, true, -1, MADSIM_FEAT_ALL, false, false)  \
    X(false, true, 6, MADSIM_FEAT_TIME, false, true)   \
    X(false, true, 5, MADSIM_FEAT_TIME, false, true)   \
    X(false, true, 6, MADSIM_FEAT_CHAN, false, true)   \
    X(false, false, 6, MADSIM_FEAT_CHAN, false, true)  \
    X(false, true, 6, MADSIM_FEAT_ALL & ~MADSIM_FEAT_ADDR, false, true) \
    X(false, true, 6, MADSIM_FEAT_ALL, false, true)    \
    X(false, true, 6, MADSIM_FEAT_TIME | MADSIM_FEAT_NARROW, false, true) \
    X(false, true, 5, MADSIM_FEAT_TIME | MADSIM_FEAT_NARROW, false, true) \
    X(false, true, 6, (MADSIM_FEAT_ALL & ~MADSIM_FEAT_ADDR) | MADSIM_FEAT_NARROW, false, true) \
    MADSIM_TIER_VARIANTS(X, MADSIM_FEAT_SCOPE)         \
    MADSIM_TIER_VARIANTS(X, MADSIM_FEAT_SCOPE | MADSIM_FEAT_TICK) \
    MADSIM_TIER_VARIANTS(X, MADSIM_FEAT_SCOPE | MADSIM_FEAT_TICK | MADSIM_FEAT_SELECT) \
    MADSIM_TIER_VARIANTS(X, MADSIM_FEAT_SIGNAL)
#endif

// A compiled specialisation of sim_kernel, and the compiled set as a table in MADSIM_FOR_EACH_VARIANT's order (sim_kernel.hip
// builds its kernel table, the host emulation its function table, from the same macro): variant_index() is the one lookup.
struct VariantSel { int trace, spill, lws, feat, rq, g; };
#define MADSIM_VARIANT_ROW(T_, S_, L_, F_, R_, G_) VariantSel{(int)(T_), (int)(S_), (L_), (F_), (int)(R_), (int)(G_)},
inline constexpr VariantSel variant_table[] = {MADSIM_FOR_EACH_VARIANT(MADSIM_VARIANT_ROW)};
#undef MADSIM_VARIANT_ROW
inline constexpr int n_variants = (int)(sizeof variant_table / sizeof *variant_table);
inline int variant_index(const VariantSel& v) {
    for (int i = 0; i < n_variants; i++) {
        const VariantSel& r = variant_table[i];
        if (r.trace == v.trace && r.spill == v.spill && r.lws == v.lws && r.feat == v.feat && r.rq == v.rq && r.g == v.g) return i;
    }
    return -1;
}
inline bool variant_compiled(const VariantSel& v) { return variant_index(v) >= 0; }

// The timer-op tier of a features word: 0, SCOPE, SCOPE|TICK or SCOPE|TICK|SELECT — or SIGNAL, the ctrl-c class, which shares the tiers'
// build shapes and none of their ops (validate() keeps the two apart).
inline int feature_tier(int feat) {
    if (feat & MADSIM_FEAT_SIGNAL) return MADSIM_FEAT_SIGNAL;
    return (feat & MADSIM_FEAT_SELECT) ? MADSIM_FEAT_TIERS : (feat & MADSIM_FEAT_TICK) ? MADSIM_FEAT_SCOPE | MADSIM_FEAT_TICK : feat & MADSIM_FEAT_SCOPE;
}

// Which compiled specialisation of sim_kernel a parameter block runs on (one rule for the launcher and for
// madsim_hip_geometry's report).
inline VariantSel select_variant(const KParams& P, bool trace) {
    const int spill = P.heap_spill > 0, lw = (int)P.lw_shift, feat = (int)P.features;
    if (const int tier = feature_tier(feat)) {                          // timer-op tiers: builds of their own, every class
        if (trace) return {1, 1, -1, MADSIM_FEAT_ALL | tier, 0, 0};
        if (P.gstate_mode) return {0, 1, 6, ((feat & MADSIM_FEAT_ADDR) ? MADSIM_FEAT_ALL : MADSIM_FEAT_ALL & ~MADSIM_FEAT_ADDR) | tier, 0, 1};
        return {0, 1, -1, MADSIM_FEAT_ALL | tier, 0, 0};
    }
    if (trace) return {1, 1, -1, MADSIM_FEAT_ALL, 0, 0};
    if (feat == 0) {                                                    // base ops only
        if (lw == 6 && P.compact) return {0, 0, 6, MADSIM_FEAT_COMPACT | (P.no_log ? MADSIM_FEAT_NOLOG : 0), 1, 0};
        if (lw == 6) return {0, spill, 6, P.no_log && !spill ? MADSIM_FEAT_NOLOG : 0, (int)P.rq_in_reg, 0};
        return {0, 1, -1, 0, 0, 0};                                     // sub-wave lane stride: runtime-stride build
    }
    // single-class workloads: a build without the other classes' code
    // (general address resolution only exists in the full build: rare, and it would cost the lean builds ~5 %)
    const int cls = (feat & ~MADSIM_FEAT_TIME) == 0 ? MADSIM_FEAT_TIME : (feat & ~MADSIM_FEAT_CHAN) == 0 ? MADSIM_FEAT_CHAN : MADSIM_FEAT_ALL;
    if (P.gstate_mode) {                                                // task table + planes in global memory: full waves
        const int nh = P.narrow ? MADSIM_FEAT_NARROW : 0;               // 8-byte heap entries (make_geometry sets it only where such a build exists)
        if (cls == MADSIM_FEAT_ALL && !(feat & MADSIM_FEAT_ADDR)) return {0, 1, 6, (MADSIM_FEAT_ALL & ~MADSIM_FEAT_ADDR) | nh, 0, 1};   // plain addresses
        // (connection workloads keep short heaps — a handful of backoff / timeout timers — that sit in LDS whole: a build
        // without the spill path, like the base-op builds have)
        // 32 seed lanes per wave: the timeout-only build has the variant.  (Round 4 also tried 16 lanes there — the election loop fell
        // from 9.2 to 6.5 G steps/s — and 32 lanes on the every-class build — the topology: 4.10 G steps/s with 20 heap entries in LDS
        // against 4.30 on full waves with 8: neither is compiled, make_geometry refuses both.)
        if (lw == 5 && cls == MADSIM_FEAT_TIME) return {0, 1, 5, cls | nh, 0, 1};
        return {0, cls == MADSIM_FEAT_CHAN ? spill : 1, 6, cls | nh, 0, 1};
    }
    if (cls != MADSIM_FEAT_ALL) return {0, 1, -1, cls, 0, 0};
    if (lw == 6) return {0, spill, 6, MADSIM_FEAT_ALL, 0, 0};
    if (lw >= 3 && lw <= 5) return {0, 1, lw, MADSIM_FEAT_ALL, 0, 0};
    return {0, 1, -1, MADSIM_FEAT_ALL, 0, 0};
}

// The contract between a parameter block and the build that will run it — checked by make_geometry before anything can be launched
// (round 4 ran the 64-lane build of the every-class kernel on a 32-lane geometry once: a selection-order slip that hung a GPU box;
// with this check such a pair is MADSIM_E_LIMITS, never a launch) and walked by tests/test_geometry_consistency.py over every
// workload class x state_mem x lanes_per_wave.  Returns nullptr when consistent, else what is wrong.
inline const char* variant_mismatch(const KParams& P, const VariantSel& v, bool trace) {
    if (!variant_compiled(v)) return "select_variant names a build that is not compiled";
    if (v.lws >= 0 && v.lws != (int)P.lw_shift) return "the build's compile-time lane stride differs from the geometry's";
    if (P.lw_shift < 3 || P.lw_shift > 6) return "lane stride outside 8..64 seed lanes per wave";
    if ((v.g != 0) != (P.gstate_mode != 0)) return "global-state build on an LDS-resident layout (or the reverse)";
    if ((v.rq != 0) != (P.rq_in_reg != 0)) return "register ready queue build on a layout with an LDS ready queue (or the reverse)";
    if (v.rq && (P.max_tasks > 8 || P.lw_shift != 6 || P.lifecycle)) return "register ready queue needs <= 8 tasks, full waves, base ops";
    if (!v.spill && P.heap_spill) return "a build without the spill path on a geometry with spilled heap levels";
    const int classes = v.feat & MADSIM_FEAT_ALL, tier = feature_tier(v.feat);
    if (((int)P.features & ~(classes | MADSIM_FEAT_TIERS | MADSIM_FEAT_SIGNAL)) != 0) return "the build lacks an op class the workload uses";
    if (((int)P.features & MADSIM_FEAT_SIGNAL) && ((int)P.features & MADSIM_FEAT_TIERS)) return "ctrl-c signals and a timer-op tier in one workload: no such build";
    if (tier != feature_tier((int)P.features)) return "the build's timer-op tier differs from the workload's";
    if (tier && (P.narrow || P.dedup_n)) return "a timer-op tier build on a layout with narrow entries or re-registration counts";
    if ((P.scope_unit != 0) != (((int)P.features & MADSIM_FEAT_SCOPE) != 0)) return "the scope unit and the scope class disagree";
    // (a select-tier workload may have no tick unit: its only select-tier op is recv_from_timeout_at)
    if (tier == (MADSIM_FEAT_SCOPE | MADSIM_FEAT_TICK) ? !P.tick_unit : (P.tick_unit && !(tier & MADSIM_FEAT_TICK)))
        return "a tick unit on a build without the ticker tier (or a ticker-tier build without one)";
    if ((classes != 0) != (P.lifecycle != 0)) return "extended-op build on the base-op LDS layout (or the reverse)";
    if (((v.feat & MADSIM_FEAT_COMPACT) != 0) != (P.compact != 0)) return "compact build on a plain layout (or the reverse)";
    if (P.compact && (P.heap_spill || P.lifecycle || P.lw_shift != 6 || !P.rq_in_reg || P.max_tasks > 8)) return "compact layout outside its conditions";
    if ((v.feat & MADSIM_FEAT_NOLOG) && (!P.no_log || trace)) return "a build without the determinism-log fold for a run that wants it";
    if (P.dedup_n && !(v.g && classes == MADSIM_FEAT_TIME)) return "re-registration counts on a build that does not carry them";
    if (P.dedup_n & (P.dedup_n - 1)) return "dedup_n must be a power of two";
    if (((v.feat & MADSIM_FEAT_NARROW) != 0) != (P.narrow != 0)) return "narrow-heap build on a wide-entry layout (or the reverse)";
    if (P.narrow && (!v.g || (P.pool_n & 31) || !P.pool_n)) return "narrow heap entries outside their conditions";
    if (P.waves_per_block != 1 && P.waves_per_block != 2 && P.waves_per_block != 4) return "a workgroup is 1, 2 or 4 waves";
    if (trace != (v.trace != 0)) return "trace build / trace launch mismatch";
    return nullptr;
}

// Grouping campaigns: where the signature (key, verdict) starts probing in a table of `slots` (a power of two) slots — splitmix64's finalizer
// over the key offset by the verdict, so equal keys under different verdicts start apart.  constexpr: one definition for the device
// (group_fold_kernel) and the host (madsim_k_group_slot, with which the tests construct colliding keys).
inline constexpr uint64_t group_slot(uint64_t key, uint32_t verdict, uint64_t slots) {
    uint64_t h = key + ((uint64_t)verdict + 1u) * 0x9E3779B97F4A7C15ull;
    h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
    h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
    return (h ^ (h >> 31)) & (slots - 1);
}

// The observation census: where a value starts probing in a table of `slots` (a power of two) slots — the same finalizer over the value
// alone.  One definition for the device (census_fold_kernel) and the host (madsim_k_census_slot, for the tests' colliding values).
inline constexpr uint64_t census_slot(uint64_t value, uint64_t slots) { return group_slot(value, 0, slots); }

}  // namespace madsim_k

extern "C" {
int  madsim_k_launch_sim(const madsim_k::KParams* P, uint32_t grid, uint32_t lds_bytes, void* stream, int trace);
void madsim_k_launch_summary(const madsim_result_t* out, uint64_t count, uint64_t seed0, unsigned long long* acc, void* stream);
void madsim_k_launch_summary6(const madsim_result_t* out, uint64_t count, uint64_t seed0, unsigned long long* acc6, void* stream);
// the collecting campaign's report kernels: summary6's words, by_verdict[8], n listed (MADSIM_K_COLLECT_WORDS words in `rep`) and the `cap`
// listed seeds of the batch with the smallest seeds, ascending, in `recs`; wave_cnt: MADSIM_K_COLLECT_WAVES words of scratch
#define MADSIM_K_COLLECT_WORDS 15u
#define MADSIM_K_COLLECT_WAVES 1024u
void madsim_k_launch_collect(const madsim_result_t* out, uint64_t count, uint64_t seed0, uint32_t list_runner, unsigned long long* rep,
                             uint32_t* wave_cnt, madsim_failure_t* recs, uint64_t cap, void* stream);
// the statistics campaign's report kernels, behind summary6 / collect on the same stream: `srep` = {n, ~min[4], max[4], low half-sums[4], high
// half-sums[4]} (17 words), hist[4][256] as 32-bit counters (512 words), top[4][16] {value, seed} (128 words); cand: per-workgroup candidate lists
#define MADSIM_K_STATS_WORDS 657u
#define MADSIM_K_STATS_CAND_WORDS 32768u
void madsim_k_launch_stats(const madsim_result_t* out, uint64_t count, uint64_t seed0, uint32_t include, uint32_t top_k, unsigned long long* srep,
                           unsigned long long* cand, void* stream);
// the host fold of one batch's MADSIM_K_STATS_WORDS into the caller's statistics (madsim_hip.cpp; no device involved)
void madsim_k_fold_stats(madsim_stats_t* st, const unsigned long long* s);
// the grouping campaign's report kernels, behind summary6 / collect / stats on the same stream: the distinct (verdict, key) among the batch's
// counted seeds, each with its count and its smallest seed.  `table`: `slots` (a power of two, >= 2 * count and >= MADSIM_K_GROUP_MIN_SLOTS)
// slots of MADSIM_K_GROUP_SLOT_BYTES, ALL ZERO before the launch and all zero again after it (the extraction pass resets the slots it
// reads); `list`: count 32-bit words of scratch (the claimed slots, in arrival order); `grep`: MADSIM_K_GROUP_WORDS words, zero before the
// launch: {groups of the batch, error word: non-zero = a probe ran out or met a slot that no seed of the batch can have claimed};
// `entries`: room for `count` madsim_group_t, the first grep[0] written, in arrival order — the host sorts them.  count <= 2^20.
#define MADSIM_K_GROUP_WORDS 2u         /* 64-bit words of a batch's grouping report      */
#define MADSIM_K_GROUP_SLOT_BYTES 16u   /* {tag, count, ~smallest index, 0}               */
#define MADSIM_K_GROUP_MIN_SLOTS 128u   /* a table is never smaller                       */
#define MADSIM_K_GROUP_MAX_COUNT 1048576u /* = MADSIM_GROUP_MAX_BATCH                      */
// Returns 0, or -1 without launching anything when a size is outside what the kernels are written for.
int  madsim_k_launch_groups(const madsim_result_t* out, uint64_t count, uint64_t seed0, uint32_t include, uint32_t key_field, uint32_t* table,
                            uint64_t slots, uint32_t* list, unsigned long long* grep, madsim_group_t* entries, void* stream);
// the smallest table madsim_k_launch_groups accepts for `count` seeds (madsim_hip.cpp; no device involved)
uint64_t madsim_k_group_slots(uint64_t count);
// the slot at which a (key, verdict) starts probing in a table of `slots` slots (a power of two); probing goes on at slot + 1, wrapping
uint64_t madsim_k_group_slot(uint64_t key, uint32_t verdict, uint64_t slots);
// the host fold of one batch's entries into the caller's groups (madsim_hip.cpp; no device involved): batches in seed order, the entries of a
// batch in any order (sorted here by first_seed - seed0_of_batch, their index in the batch).  `state` remembers which signature sits where.
void* madsim_k_group_state_new(void);
void  madsim_k_group_state_free(void* state);
void  madsim_k_fold_groups(madsim_groups_t* grp, void* state, const madsim_group_t* batch_entries, uint64_t n, uint64_t seed0_of_batch);
// the differential campaign's report kernels, behind the two sides' simulation and summary6 launches on the same stream: `a` and `b` are the
// two sides' results of the same `count` seeds.  `words`: MADSIM_K_DIFF_WORDS words, ALL ZERO before the launch: {n_differ, n_incomparable,
// n_by_field[8], transitions[8][8]} of the batch; `wave_cnt`: MADSIM_K_COLLECT_WAVES words of scratch (every wave's number of differing seeds);
// `recs`: the `cap` differing seeds of the batch with the smallest seeds, ascending (may be null when cap == 0; nothing behind
// min(cap, n_differ) is written).  `fields`: a MADSIM_DIFF_* mask.  Returns 0, or -1 without launching anything for fields == 0, a bit above
// MADSIM_DIFF_ALL, count == 0 or count >= 2^32 (the counters of a workgroup are 32-bit).
#define MADSIM_K_DIFF_WORDS 74u         /* 64-bit words of a batch's diff report: 2 + 8 + 64 */
int  madsim_k_launch_diff(const madsim_result_t* a, const madsim_result_t* b, uint64_t count, uint64_t seed0, uint32_t fields,
                          unsigned long long* words, uint32_t* wave_cnt, madsim_diff_record_t* recs, uint64_t cap, void* stream);
// the host fold of one batch's MADSIM_K_DIFF_WORDS into the caller's report (madsim_hip.cpp; no device involved): batches in seed order.
// Returns how many of the batch's records the list still takes — min(the batch's n_differ, cap - n_listed) — and advances n_listed by it;
// when `batch_recs` (host memory, at least that many) is given they are appended to diff->records, otherwise the caller copies them there.
uint64_t madsim_k_fold_diff(madsim_diff_t* diff, const unsigned long long* words, uint64_t count, const madsim_diff_record_t* batch_recs);
// the sweep campaign's report kernels, behind the variants' simulation and summary6 launches on the same stream: sides[0 .. n_variants) (a HOST
// array of device pointers, 2 .. MADSIM_SWEEP_MAX_VARIANTS of them) are the variants' results of the same `count` seeds.  `words`:
// MADSIM_K_SWEEP_WORDS words, ALL ZERO before the launch: {n_selected, n_incomparable, n_runner_by_variant[8], n_differ_from_first[8],
// n_by_mask[256]} of the batch; `wave_cnt`: MADSIM_K_COLLECT_WAVES words of scratch (every wave's number of selected seeds); `recs`: the `cap`
// selected seeds of the batch with the smallest seeds, ascending (may be null when cap == 0; nothing behind min(cap, n_selected) is written).
// `fields`: a MADSIM_DIFF_* mask (0 = compare nothing), `rule`: MADSIM_SWEEP_LIST_*.  Returns 0, or -1 without launching anything for
// n_variants outside 2 .. 8, a NULL side, count == 0 or count >= 2^32, a bit above MADSIM_DIFF_ALL, rule > 2, LIST_DIFFERING with
// fields == 0, or cap > 0 without records.
#define MADSIM_K_SWEEP_WORDS 274u       /* 64-bit words of a batch's sweep report: 2 + 8 + 8 + 256 */
int  madsim_k_launch_sweep(const madsim_result_t* const* sides, uint32_t n_variants, uint64_t count, uint64_t seed0, uint32_t fields, uint32_t rule,
                           unsigned long long* words, uint32_t* wave_cnt, madsim_sweep_record_t* recs, uint64_t cap, void* stream);
int  madsim_k_launch_sweep_list(const madsim_result_t* const* sides, uint32_t n_variants, uint64_t count, const uint64_t* d_seeds, uint32_t fields,
                                uint32_t rule, unsigned long long* words, uint32_t* wave_cnt, madsim_sweep_record_t* recs, uint64_t cap, void* stream);
// the host fold of one batch's MADSIM_K_SWEEP_WORDS into the caller's report (madsim_hip.cpp; no device involved): batches in seed order.
// Returns how many of the batch's records the list still takes — min(the batch's n_selected, cap - n_listed) — and advances n_listed by it;
// when `batch_recs` (host memory, at least that many) is given they are appended to sweep->records, otherwise the caller copies them there.
uint64_t madsim_k_fold_sweep(madsim_sweep_t* sweep, const unsigned long long* words, uint64_t count, const madsim_sweep_record_t* batch_recs);
// the paired campaign's report kernels, behind the two sides' simulation and summary6 launches (and the diff kernels) on the same stream: `a`
// and `b` are the two sides' results of the same `count` seeds.  `words`: MADSIM_K_PAIRED_WORDS words, ALL ZERO before the launch (the minima
// are kept inverted, so one memset or device copy prepares them): {n_paired, n_incomparable, n[8], ~min[8], max[8], low half-sums of the
// magnitudes[8], high[8], low half-sums of a[4], high[4], low half-sums of b[4], high[4]} (MADSIM_K_PAIRED_HEAD_WORDS), then hist[8][256] as
// 32-bit counters (1 024 words), then top[8][16] {seed, a, b} (384 words); index 8 = 2 * metric + direction.  `cand`:
// MADSIM_K_PAIRED_CAND_WORDS words of scratch, per-workgroup candidate lists; untouched, and may be null, when top_k == 0 — and then nothing
// behind the histograms is written.  Returns 0, or -1 without launching anything for count == 0 or count >= 2^32, an include mask that is 0
// or has a bit at or above 4, top_k > MADSIM_STAT_MAX_TOP, or a missing array.
#define MADSIM_K_PAIRED_HEAD_WORDS 58u    /* 2 + 8 + 4 x 8 + 4 x 4: the words in front of the histograms */
#define MADSIM_K_PAIRED_WORDS 1466u       /* 58 + 8 * 256 / 2 + 8 * 16 * 3 */
#define MADSIM_K_PAIRED_CAND_WORDS 65536u /* 8 sets x 256 workgroups x 16 x {magnitude, index} */
int  madsim_k_launch_paired(const madsim_result_t* a, const madsim_result_t* b, uint64_t count, uint64_t seed0, uint32_t include_a, uint32_t include_b,
                            uint32_t top_k, unsigned long long* words, unsigned long long* cand, void* stream);
int  madsim_k_launch_paired_list(const madsim_result_t* a, const madsim_result_t* b, uint64_t count, const uint64_t* d_seeds, uint32_t include_a,
                                 uint32_t include_b, uint32_t top_k, unsigned long long* words, unsigned long long* cand, void* stream);
// the host fold of one batch's MADSIM_K_PAIRED_WORDS over `count` seeds into the caller's report (madsim_hip.cpp; no device involved): the
// counts, minima, maxima and sums commute, and the extreme seeds are merged under the total order (magnitude descending, seed ascending).
void madsim_k_fold_paired(madsim_paired_t* pr, const unsigned long long* words, uint64_t count);
// resolving campaigns (MADSIM_CAMPAIGN_RESOLVE).  The list pair, over collect's cut of the batch: a result is re-runnable when its verdict is
// MADSIM_OVERFLOW, or MADSIM_STEP_LIMIT with `steps_maxed` == 0.  *total = m, the re-runnable seeds of out[0 .. count); seeds[0 .. m) =
// seed0 + i and idx[0 .. m) = i of those results, ascending, the same on every run; nothing behind m is written.  `wave_cnt`:
// MADSIM_K_RESOLVE_WAVES words of scratch; nothing needs preparing.  Returns 0, or -1 without launching anything for count == 0 or
// count >= 2^32 (the index list is 32-bit).
#define MADSIM_K_RESOLVE_WAVES 1024u    /* = MADSIM_K_COLLECT_WAVES: the same cut            */
#define MADSIM_K_RESOLVE_CHUNKS 3u      /* 16-byte chunks of a madsim_result_t               */
int  madsim_k_launch_resolve_list(const madsim_result_t* out, uint64_t count, uint64_t seed0, uint32_t steps_maxed, uint32_t* wave_cnt,
                                  uint32_t* total, uint64_t* seeds, uint32_t* idx, void* stream);
// out[idx[j]] = rerun[j] for j < m, 48 bytes each as three 16-byte chunks (thread t: chunk t % 3 of record t / 3); idx: distinct indices into
// `out`, nothing else of which is touched.  m == 0 launches nothing.  Returns 0, or -1 without launching anything for 3 * m >= 2^32.
int  madsim_k_launch_resolve_scatter(madsim_result_t* out, const madsim_result_t* rerun, const uint32_t* idx, uint64_t m, void* stream);
// The list forms of the six report launchers above (the list campaigns, madsim_hip_run_seeds_campaign): result i belongs to seed d_seeds[i]
// where the range form says seed0 + i — `d_seeds` a device pointer to the batch's slice of a strictly ascending seed list, `count` entries,
// read only for a result whose seed is reported (a failing, listed, extreme, first-of-its-group, differing or re-runnable one).  Everything
// else — buffers, preparation, cut, return values — is the range form's; for a slice seed0, seed0 + 1, ... every byte written is too.
// The resolve form reads the slice and writes `seeds`: two buffers, never the same one.
void madsim_k_launch_summary6_list(const madsim_result_t* out, uint64_t count, const uint64_t* d_seeds, unsigned long long* acc6, void* stream);
void madsim_k_launch_collect_list(const madsim_result_t* out, uint64_t count, const uint64_t* d_seeds, uint32_t list_runner, unsigned long long* rep,
                                  uint32_t* wave_cnt, madsim_failure_t* recs, uint64_t cap, void* stream);
void madsim_k_launch_stats_list(const madsim_result_t* out, uint64_t count, const uint64_t* d_seeds, uint32_t include, uint32_t top_k,
                                unsigned long long* srep, unsigned long long* cand, void* stream);
int  madsim_k_launch_groups_list(const madsim_result_t* out, uint64_t count, const uint64_t* d_seeds, uint32_t include, uint32_t key_field,
                                 uint32_t* table, uint64_t slots, uint32_t* list, unsigned long long* grep, madsim_group_t* entries, void* stream);
int  madsim_k_launch_diff_list(const madsim_result_t* a, const madsim_result_t* b, uint64_t count, const uint64_t* d_seeds, uint32_t fields,
                               unsigned long long* words, uint32_t* wave_cnt, madsim_diff_record_t* recs, uint64_t cap, void* stream);
int  madsim_k_launch_resolve_list_list(const madsim_result_t* out, uint64_t count, const uint64_t* d_seeds, uint32_t steps_maxed, uint32_t* wave_cnt,
                                       uint32_t* total, uint64_t* seeds, uint32_t* idx, void* stream);
// divergence reports (madsim_hip_diverge_seeds), behind the two sides' trace launches on the same stream: two sets of trace rows of the same
// `n` seeds — log rows of `log_cap` bytes, observation rows of `obs_cap` words, 16-byte aligned arrays (null with a cap of 0), the TRUE
// lengths (which may exceed the caps), the results and the seeds — compared where they lie.  recs[i]: the record of seed d_seeds[i], by the
// status table in include/madsim_hip.h; ctx: n rows of 3 * win words (null iff win == 0).  A pure function of its inputs: nothing needs
// preparing, every word of `recs` and `ctx` is written, nothing else is.  One wave per row pair, MADSIM_K_DIVERGE_WAVES waves at most.
// Returns 0, or -1 without launching anything for n == 0, n >= 2^32, win > MADSIM_DIVERGE_MAX_WIN, a missing or misaligned array.
#define MADSIM_K_DIVERGE_WAVES 1024u    /* = MADSIM_K_COLLECT_WAVES: 256 workgroups of four waves */
int  madsim_k_launch_diverge(const uint8_t* log_a, const uint8_t* log_b, uint64_t log_cap, const uint64_t* obs_a, const uint64_t* obs_b,
                             uint64_t obs_cap, const uint64_t* log_len_a, const uint64_t* log_len_b, const uint64_t* obs_len_a,
                             const uint64_t* obs_len_b, const madsim_result_t* res_a, const madsim_result_t* res_b, const uint64_t* d_seeds,
                             uint64_t n, uint32_t win, madsim_divergence_t* recs, uint64_t* ctx, void* stream);
// the observation census (madsim_hip_census_range / _seeds), behind the chunk's trace launch on the same stream: the observation rows of `n`
// seeds (`obs_cap` words each), their TRUE lengths (which may exceed obs_cap; whatever a row holds behind min(len, obs_cap) is ignored), the
// results and the seeds, reduced where they lie.  `table`: `slots` (a power of two, >= 2 * cap and >= MADSIM_K_CENSUS_MIN_SLOTS) slots of
// MADSIM_K_CENSUS_SLOT_BYTES, ALL ZERO before the launch and all zero again after it, whatever happened; `list`: cap 32-bit words of scratch
// (the claimed slots, in arrival order); `words`: MADSIM_K_CENSUS_WORDS words, zero before the launch: {distinct values of the chunk, error
// word, n_counted[4], n_silent[4], n_truncated, n_observations, n_runner}; `entries`: room for `cap` madsim_census_value_t, the first
// words[0] written, in arrival order — the host sorts them.  d_seeds ASCEND with the row (the range form's seed0 + i, a strictly ascending
// list's slice): an entry's first_seed is the seed of the smallest row that held the value.  A value that would be distinct value
// number cap + 1 sets MADSIM_K_CENSUS_ERR_CAP in the error word and is not inserted; with a non-zero error word no entry is written (words[0] is then not a
// count of anything).  One wave per row, MADSIM_K_CENSUS_WAVES waves at most.  Returns 0, or -1 without launching anything for n == 0,
// n > 2^31, n * obs_cap >= 2^32 - 1 (a slot's tag is 1 + the flat index of an observation), obs_cap outside 1 .. MADSIM_CENSUS_MAX_OBS_CAP, an include
// mask that is 0 or has a bit at or above 4, cap outside 1 .. MADSIM_CENSUS_MAX_VALUES, a table of the wrong size or a missing array.
#define MADSIM_K_CENSUS_WORDS 16u       /* 64-bit words of a chunk's census report: 13 used  */
#define MADSIM_K_CENSUS_SLOT_BYTES 32u  /* {tag, n_seeds[4], n_total, max_per_seed, ~smallest row} */
#define MADSIM_K_CENSUS_MIN_SLOTS 128u  /* a table is never smaller                          */
#define MADSIM_K_CENSUS_WAVES 1024u     /* = MADSIM_K_DIVERGE_WAVES: 256 workgroups of four waves */
#define MADSIM_K_CENSUS_ERR_PROBE 1u    /* a probe ran out                                   */
#define MADSIM_K_CENSUS_ERR_TAG 2u      /* a slot no observation of the chunk can have claimed: the table was not clean */
#define MADSIM_K_CENSUS_ERR_CAP 4u      /* more than `cap` distinct values                   */
int  madsim_k_launch_census(const uint64_t* obs, uint64_t obs_cap, const uint64_t* obs_len, const madsim_result_t* res, const uint64_t* d_seeds,
                            uint64_t n, uint32_t include, uint32_t* table, uint64_t slots, uint32_t* list, uint64_t cap, unsigned long long* words,
                            madsim_census_value_t* entries, void* stream);
// ... with the fold kernel's form named: direct != 0 = one table update per row and distinct value, no wave accumulator in LDS (what
// MADSIM_HIP_CENSUS_DIRECT=1 makes madsim_k_launch_census choose): the correctness baseline and the other side of the A/B
int  madsim_k_launch_census_form(const uint64_t* obs, uint64_t obs_cap, const uint64_t* obs_len, const madsim_result_t* res, const uint64_t* d_seeds,
                                 uint64_t n, uint32_t include, uint32_t* table, uint64_t slots, uint32_t* list, uint64_t cap, unsigned long long* words,
                                 madsim_census_value_t* entries, void* stream, int direct);
// the smallest table madsim_k_launch_census accepts for `cap` values (madsim_hip.cpp; no device involved)
uint64_t madsim_k_census_slots(uint64_t cap);
// the slot at which a value starts probing in a table of `slots` slots (a power of two); probing goes on at slot + 1, wrapping
uint64_t madsim_k_census_slot(uint64_t value, uint64_t slots);
// the host fold of one chunk into the caller's census (madsim_hip.cpp; no device involved): `words` (may be null: no totals) are added to the
// totals, and the chunk's `n` entries (any order, distinct values) merged into cen->values[0 .. n_values), which stay ascending by value —
// counts added, the max of max_per_seed, the min of first_seed.  Returns 0, or -1 with `cen` untouched when the table would pass cen->cap.
int  madsim_k_fold_census(madsim_census_t* cen, const unsigned long long* words, const madsim_census_value_t* entries, uint64_t n);
// the stall-site census (madsim_hip_stall_census_range / _seeds), behind the chunk's trace launch on the same stream: stall_sites_kernel over the
// task rows of `n` seeds (`task_cap` words each, include/madsim_hip.h "Task post-mortems"), their TRUE counts and the results.  sites: n rows of
// task_cap words — MADSIM_TASK_SITE of each of row i's visible records (the first min(len, task_cap); of a runner verdict's row none: the
// row and its count are not read), zeros behind; shape: n words, madsim_hip_stall_shape of the visible records; ones: n words, each 1 — the
// length array under which madsim_k_launch_census folds `shape` as rows of cap 1.  A pure function of its inputs: nothing needs preparing,
// every word of the three outputs is written, nothing else is.  One wave per row, MADSIM_K_CENSUS_WAVES waves at most.  Returns 0, or -1
// without launching anything for n == 0, n > 2^31, task_cap outside 1 .. MADSIM_MAX_LIVE_TASKS, n * task_cap >= 2^32 - 1 or a missing array.
int  madsim_k_launch_stall_sites(const uint64_t* tasks, uint64_t task_cap, const uint64_t* task_len, const madsim_result_t* res, uint64_t n,
                                 uint64_t* sites, uint64_t* shape, uint64_t* ones, void* stream);
// the host fold of one chunk into the caller's report (madsim_hip.cpp; no device involved): the site pass's words and entries and the shape
// pass's entries (null with 0: none), each through madsim_k_fold_census's merge.  Returns 0, or -1 when either table would pass its cap:
// the report is then to be discarded.
int  madsim_k_fold_stall_census(madsim_stall_census_t* sc, const unsigned long long* words, const madsim_census_value_t* sites, uint64_t n_sites,
                                const madsim_census_value_t* shapes, uint64_t n_shapes);
// the probe-set census (madsim_hip_probe_sets_range / _seeds), behind the chunk's trace launch on the same stream: three kernels over the
// observation rows of `n` seeds (`obs_cap` words each), their TRUE lengths, the results and the seeds.  sets_mask_kernel writes the set
// word (include/madsim_hip.h) of every COUNTED row i to sig[i] — `sig`: n 64-bit words of scratch; the words of other rows are neither
// written nor read, and neither are those rows —, against vocab[0 .. n_vocab), HOST memory here: the values travel in the kernel arguments.
// sets_fold_kernel folds equal set words into `table`: `slots` (a power of two, >= 2 * cap and >= MADSIM_K_PROBE_SETS_MIN_SLOTS) slots of
// MADSIM_K_PROBE_SETS_SLOT_BYTES, ALL ZERO before the launch and all zero again after it, whatever happened; a set word starts probing at
// madsim_k_census_slot(set, slots).  `list`: cap 32-bit words of scratch (the claimed slots, in arrival order); `words`:
// MADSIM_K_PROBE_SETS_WORDS words, zero before the launch: {distinct sets of the chunk, error word, n_counted[4], n_runner}; `entries`: room
// for `cap` madsim_probe_set_t, the first words[0] written by sets_extract_kernel, in arrival order — the host sorts them.  d_seeds
// ASCEND with the row.  The set that would be distinct set number cap + 1 sets MADSIM_K_PROBE_SETS_ERR_CAP in the error word and is not
// inserted; with a non-zero error word no entry is written (words[0] is then not a count of anything).  Returns 0, or -1 without launching
// anything for n == 0, n > 2^31, n * obs_cap >= 2^32 - 1, obs_cap outside 1 .. MADSIM_CENSUS_MAX_OBS_CAP, n_vocab outside
// 1 .. MADSIM_PROBE_SETS_MAX_VOCAB, an include mask that is 0 or has a bit at or above 4, cap outside 1 .. MADSIM_PROBE_SETS_MAX, a table
// of the wrong size or a missing array.
#define MADSIM_K_PROBE_SETS_WORDS 8u        /* 64-bit words of a chunk's report: 7 used              */
#define MADSIM_K_PROBE_SETS_SLOT_BYTES 48u  /* {tag, n_seeds[4], ~smallest row[4], 0, 0, 0}          */
#define MADSIM_K_PROBE_SETS_MIN_SLOTS 128u  /* a table is never smaller                              */
#define MADSIM_K_PROBE_SETS_WAVES 1024u     /* = MADSIM_K_CENSUS_WAVES: 256 workgroups of four waves */
#define MADSIM_K_PROBE_SETS_ERR_PROBE 1u    /* a probe ran out                                       */
#define MADSIM_K_PROBE_SETS_ERR_TAG 2u      /* a slot no seed of the chunk can have claimed: the table was not clean */
#define MADSIM_K_PROBE_SETS_ERR_CAP 4u      /* more than `cap` distinct sets                         */
int  madsim_k_launch_probe_sets(const uint64_t* obs, uint64_t obs_cap, const uint64_t* obs_len, const madsim_result_t* res, const uint64_t* d_seeds,
                                uint64_t n, uint32_t include, const uint64_t* vocab, uint64_t n_vocab, uint64_t* sig, uint32_t* table,
                                uint64_t slots, uint32_t* list, uint64_t cap, unsigned long long* words, madsim_probe_set_t* entries, void* stream);
// ... with the fold kernel's form named: per_seed != 0 = one table update per counted seed, no in-wave combine of equal set words: the
// correctness baseline and the other side of the A/B (tools/sets_ab.py); the same bytes either way
int  madsim_k_launch_probe_sets_form(const uint64_t* obs, uint64_t obs_cap, const uint64_t* obs_len, const madsim_result_t* res,
                                     const uint64_t* d_seeds, uint64_t n, uint32_t include, const uint64_t* vocab, uint64_t n_vocab, uint64_t* sig,
                                     uint32_t* table, uint64_t slots, uint32_t* list, uint64_t cap, unsigned long long* words,
                                     madsim_probe_set_t* entries, void* stream, int per_seed);
// the smallest table madsim_k_launch_probe_sets accepts for `cap` sets (madsim_hip.cpp; no device involved)
uint64_t madsim_k_probe_sets_slots(uint64_t cap);
// the host fold of one chunk into the caller's report (madsim_hip.cpp; no device involved): `words` (may be null: no totals) are added to
// the totals, and the chunk's `n` entries (any order) merged into ps->sets[0 .. n_sets), which stay ascending by set — counts added,
// per verdict the smaller first_seed of the sides that have one.  Returns 0, or -1 with `ps` untouched when the table would pass ps->cap.
int  madsim_k_fold_probe_sets(madsim_probe_sets_t* ps, const unsigned long long* words, const madsim_probe_set_t* entries, uint64_t n);
// the probe-order census (madsim_hip_probe_order_range / _seeds), behind the chunk's trace launch on the same stream: two kernels over the
// observation rows of `n` seeds (`obs_cap` words each), their TRUE lengths, the results and the seeds.  order_fold_kernel finds first(j)
// (include/madsim_hip.h) of every COUNTED row against vocab[0 .. n_vocab), HOST memory here: the values travel in the kernel arguments —
// other rows are not read — and adds the row's relation to `matrix`: MADSIM_K_PROBE_ORDER_MATRIX_WORDS 32-bit words, ALL ZERO before the
// launch and all zero again after it, whatever happened — counts [verdict][a][b] (4 x 32 x 32), then as many witnesses, the largest
// inverted row index of the cell.  `words`: MADSIM_K_PROBE_ORDER_WORDS words, zero before the launch: {entries written, error word,
// n_counted[4], n_none[4], n_truncated, n_runner}; `entries`: room for n_vocab * n_vocab madsim_probe_order_pair_t, the first words[0]
// written by order_extract_kernel, ascending by (a, b), with first_seed read from d_seeds.  A witness that is no row of the chunk, or a
// non-zero cell outside the vocabulary, sets MADSIM_K_PROBE_ORDER_ERR_TAG in the error word (a matrix that was not clean); the entry is
// then all zero.  Returns 0, or -1 without launching anything for n == 0, n > 2^31, n * obs_cap >= 2^32 - 1, obs_cap outside
// 1 .. MADSIM_CENSUS_MAX_OBS_CAP, n_vocab outside 1 .. MADSIM_PROBE_ORDER_MAX_VOCAB, an include mask that is 0 or has a bit at or above
// 4, or a missing or misaligned array.
#define MADSIM_K_PROBE_ORDER_WORDS 12u          /* 64-bit words of a chunk's report                                */
#define MADSIM_K_PROBE_ORDER_MATRIX_WORDS 8192u /* 32-bit words: 4 x 32 x 32 counts, 4 x 32 x 32 witnesses: 32 KB   */
#define MADSIM_K_PROBE_ORDER_WAVES 1024u        /* = MADSIM_K_CENSUS_WAVES: 256 workgroups of four waves            */
#define MADSIM_K_PROBE_ORDER_ERR_TAG 2u         /* a cell no seed of the chunk can have written: the matrix was not clean */
int  madsim_k_launch_probe_order(const uint64_t* obs, uint64_t obs_cap, const uint64_t* obs_len, const madsim_result_t* res, const uint64_t* d_seeds,
                                 uint64_t n, uint32_t include, const uint64_t* vocab, uint64_t n_vocab, uint32_t* matrix, unsigned long long* words,
                                 madsim_probe_order_pair_t* entries, void* stream);
// ... with the fold kernel's form named: direct != 0 = every update goes straight to the global matrix, no workgroup accumulator in LDS:
// the correctness baseline and the other side of the A/B (tools/order_ab.py); the same bytes either way
int  madsim_k_launch_probe_order_form(const uint64_t* obs, uint64_t obs_cap, const uint64_t* obs_len, const madsim_result_t* res,
                                      const uint64_t* d_seeds, uint64_t n, uint32_t include, const uint64_t* vocab, uint64_t n_vocab, uint32_t* matrix,
                                      unsigned long long* words, madsim_probe_order_pair_t* entries, void* stream, int direct);
// the host fold of one chunk into the caller's report (madsim_hip.cpp; no device involved): `words` (may be null: no totals) are added to
// the totals, and the chunk's `n` entries (any order) merged into po->pairs[0 .. n_pairs), which stay ascending by (a, b) — counts added,
// per verdict the smaller first_seed of the sides that have one.  Returns 0, or -1 with `po` untouched when the table would pass po->cap.
int  madsim_k_fold_probe_order(madsim_probe_order_t* po, const unsigned long long* words, const madsim_probe_order_pair_t* entries, uint64_t n);
// probe spans (madsim_hip_probe_spans_range / _seeds), behind the chunk's trace launch on the same stream: two kernels over the observation rows
// and the time rows of `n` seeds (`obs_cap` words each), their TRUE lengths, the results and the seeds; defs[0 .. n_spans) in HOST memory (they
// travel in the kernel arguments).  span_fold_kernel places i and j (include/madsim_hip.h) of every COUNTED row — other rows are not read —,
// writes state (32-bit; MADSIM_K_SPAN_UNCOUNTED for a row that is not counted) and duration per (row, span) to `st` / `dur` (n * n_spans each,
// need not be zero) and adds to `recs`: n_spans records of MADSIM_K_SPAN_REC_WORDS 64-bit words, which the launcher zeroes first —
//   [v * 4 + state] counts, [16] n, [17] max of ~duration, [18] max of duration, [19] / [20] the sums of the durations' low / high 32-bit
//   halves, [21] / [22] / [23] max of ~seed over the rows whose duration is the minimum / the maximum / that are OPEN, [24 ..] hist
// — every word is a sum or a maximum from zero, so no arrival order shows, and madsim_k_fold_probe_spans decodes them.  span_witness_kernel,
// behind it, reads the chunk's final [17] / [18] and writes [21 .. 23].  `words`: MADSIM_K_PROBE_SPANS_WORDS words, zero before the launch:
// {n_spans, error word (always 0), n_counted[4], n_truncated, n_runner}.  Returns 0, or -1 without launching anything for n == 0, n > 2^31,
// n * obs_cap >= 2^32 - 1, obs_cap outside 1 .. MADSIM_CENSUS_MAX_OBS_CAP, n_spans outside 1 .. MADSIM_PROBE_SPANS_MAX, an unknown flag, an
// include mask that is 0 or has a bit at or above 4, or a missing or misaligned array.
#define MADSIM_K_PROBE_SPANS_WORDS 8u           /* 64-bit words of a chunk's report                                */
#define MADSIM_K_SPAN_REC_WORDS 280u            /* = sizeof(madsim_span_t) / 8                                     */
#define MADSIM_K_SPAN_UNCOUNTED 4u              /* the state word of a row that is not counted                     */
typedef struct madsim_k_span_rec { unsigned long long w[MADSIM_K_SPAN_REC_WORDS]; } madsim_k_span_rec_t;
int  madsim_k_launch_probe_spans(const uint64_t* obs, const uint64_t* times, uint64_t obs_cap, const uint64_t* obs_len, const madsim_result_t* res,
                                 const uint64_t* d_seeds, uint64_t n, uint32_t include, const madsim_span_def_t* defs, uint64_t n_spans, uint32_t* st,
                                 unsigned long long* dur, madsim_k_span_rec_t* recs, unsigned long long* words, void* stream);
// ... with the fold kernel's form named: direct != 0 = every update goes straight to the global records, no workgroup accumulator in LDS: the
// correctness baseline and the other side of the A/B (tools/spans_ab.py); the same bytes either way
int  madsim_k_launch_probe_spans_form(const uint64_t* obs, const uint64_t* times, uint64_t obs_cap, const uint64_t* obs_len, const madsim_result_t* res,
                                      const uint64_t* d_seeds, uint64_t n, uint32_t include, const madsim_span_def_t* defs, uint64_t n_spans,
                                      uint32_t* st, unsigned long long* dur, madsim_k_span_rec_t* recs, unsigned long long* words, void* stream,
                                      int direct);
// the host fold of one chunk into the caller's report (madsim_hip.cpp; no device involved): `words` (may be null: no totals) are added to the
// totals, and the chunk's `n` == ps->n_spans device records decoded and merged into ps->spans — counts, sums and histograms add, of two equal
// extremes the smaller seed wins, first_open_seed is the minimum.  ps->spans must hold records (madsim_k_span_init gives the empty one).
// Returns 0, or -1 with `ps` untouched when n != ps->n_spans.
int  madsim_k_fold_probe_spans(madsim_probe_spans_t* ps, const unsigned long long* words, const madsim_k_span_rec_t* recs, uint64_t n);
void madsim_k_span_init(madsim_span_t* span);
int  madsim_k_set_max_lds(uint32_t lds_bytes);
int  madsim_k_variant_vgprs(const madsim_k::VariantSel* v);
void madsim_k_launch_keyflip(unsigned long long* acc, void* stream);
}

#endif
