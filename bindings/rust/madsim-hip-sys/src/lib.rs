//! Raw FFI to `libmadsim_hip.so` — the MI355X (gfx950) many-seed runner behind madsim's `Builder::run`
//! (`madsim/src/sim/runtime/builder.rs:121-162`).  One item per item of `include/madsim_hip.h`, same names, same field
//! order; `tests/test_rust_binding.py` keeps the two in step without a Rust toolchain (field order, widths, constant
//! values, function arity and parameter types).  Regenerate with `python tools/gen_rust_sys.py`.
//!
//! Nothing here has a CPU fallback: without the library or a GPU every entry point returns an error code.
#![allow(non_camel_case_types, non_upper_case_globals)]

use std::os::raw::{c_char, c_int, c_void};

/// Opaque per-GPU runner state (`madsim_hip_ctx_t`).
#[repr(C)]
pub struct madsim_hip_ctx_t {
    _private: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_insn_t {
    pub op: u8,
    pub a: u8,
    pub b: u16,
    pub imm: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_prog_t {
    pub node: u8,
    pub flags: u8,
    pub entry: u16,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_sock_t {
    pub node: u8,
    pub kind: u8,
    pub port: u16,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_service_t {
    pub vaddr: u8,
    pub n_servers: u8,
    pub servers: [u8; 6],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_node_t {
    pub flags: u8,
    pub n_match: u8,
    pub r#match: [u8; 2],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_workload_t {
    pub n_nodes: u32,
    pub n_progs: u32,
    pub n_socks: u32,
    pub n_insns: u32,
    pub nodes: *const madsim_node_t,
    pub progs: *const madsim_prog_t,
    pub socks: *const madsim_sock_t,
    pub insns: *const madsim_insn_t,
    pub n_services: u32,
    pub panic_dyn_max: u32,
    pub services: *const madsim_service_t,
    pub panic_match: *const u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_config_t {
    pub packet_loss_rate: f64,
    pub lat_lo_ns: u64,
    pub lat_hi_ns: u64,
    pub buggify: u32,
    pub n_loss_table: u32,
    pub loss_table: [f64; 4],
    pub n_lat_table: u32,
    pub reserved0: u32,
    pub lat_table_lo_ns: [u64; 4],
    pub lat_table_hi_ns: [u64; 4],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_limits_t {
    pub time_limit_ns: u64,
    pub max_steps: u32,
    pub heap_lds_slots: u32,
    pub heap_spill_slots: u32,
    pub max_tasks: u32,
    pub mbox_regs: u32,
    pub mbox_msgs: u32,
    pub lanes_per_wave: u32,
    pub max_conns: u32,
    pub chan_queue: u32,
    pub sched: u32,
    pub state_mem: u32,
    pub max_steps_ceiling: u32,
    pub no_trace_hash: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_result_t {
    pub verdict: u32,
    pub steps: u32,
    pub clock_ns: u64,
    pub msg_count: u64,
    pub rng_calls: u64,
    pub trace_hash: u64,
    pub obs_hash: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_summary_t {
    pub first_failing_seed: u64,
    pub n_failed: u64,
    pub total_steps: u64,
    pub total_clock_ns: u64,
    pub kernel_ms: f64,
    pub wall_s: f64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_divergence_t {
    pub seed: u64,
    pub log_status: u32,
    pub obs_status: u32,
    pub log_at: u64,
    pub obs_at: u64,
    pub log_len_a: u64,
    pub log_len_b: u64,
    pub obs_len_a: u64,
    pub obs_len_b: u64,
    pub obs_a: u64,
    pub obs_b: u64,
    pub log_a: u8,
    pub log_b: u8,
    pub pad: [u8; 6],
    pub a: madsim_result_t,
    pub b: madsim_result_t,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_census_value_t {
    pub value: u64,
    pub n_seeds: [u64; 4],
    pub n_total: u64,
    pub first_seed: u64,
    pub max_per_seed: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_census_t {
    pub include: u32,
    pub obs_cap: u32,
    pub values: *const madsim_census_value_t,
    pub cap: u64,
    pub runner_seeds: *const u64,
    pub runner_cap: u64,
    pub n_values: u64,
    pub n_counted: [u64; 4],
    pub n_silent: [u64; 4],
    pub n_truncated: u64,
    pub n_observations: u64,
    pub n_runner: u64,
    pub n_runner_listed: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_probe_set_t {
    pub set: u64,
    pub n_seeds: [u64; 4],
    pub first_seed: [u64; 4],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_probe_sets_t {
    pub include: u32,
    pub obs_cap: u32,
    pub vocab: *const u64,
    pub n_vocab: u64,
    pub sets: *const madsim_probe_set_t,
    pub cap: u64,
    pub runner_seeds: *const u64,
    pub runner_cap: u64,
    pub n_sets: u64,
    pub n_counted: [u64; 4],
    pub n_runner: u64,
    pub n_runner_listed: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_probe_order_pair_t {
    pub a: u32,
    pub b: u32,
    pub n_seeds: [u64; 4],
    pub first_seed: [u64; 4],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_probe_order_t {
    pub include: u32,
    pub obs_cap: u32,
    pub vocab: *const u64,
    pub n_vocab: u64,
    pub pairs: *const madsim_probe_order_pair_t,
    pub cap: u64,
    pub runner_seeds: *const u64,
    pub runner_cap: u64,
    pub n_pairs: u64,
    pub n_counted: [u64; 4],
    pub n_none: [u64; 4],
    pub n_truncated: u64,
    pub n_runner: u64,
    pub n_runner_listed: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_span_def_t {
    pub from: u64,
    pub to: u64,
    pub flags: u32,
    pub reserved: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_span_t {
    pub n_state: [u64; 16],
    pub n: u64,
    pub min: u64,
    pub max: u64,
    pub sum_lo: u64,
    pub sum_hi: u64,
    pub min_seed: u64,
    pub max_seed: u64,
    pub first_open_seed: u64,
    pub hist: [u64; 256],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_probe_spans_t {
    pub include: u32,
    pub obs_cap: u32,
    pub defs: *const madsim_span_def_t,
    pub n_spans: u64,
    pub spans: *const madsim_span_t,
    pub runner_seeds: *const u64,
    pub runner_cap: u64,
    pub n_counted: [u64; 4],
    pub n_truncated: u64,
    pub n_runner: u64,
    pub n_runner_listed: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_stall_census_t {
    pub include: u32,
    pub task_cap: u32,
    pub sites: *const madsim_census_value_t,
    pub site_cap: u64,
    pub shapes: *const madsim_census_value_t,
    pub shape_cap: u64,
    pub runner_seeds: *const u64,
    pub runner_cap: u64,
    pub n_sites: u64,
    pub n_shapes: u64,
    pub n_counted: [u64; 4],
    pub n_idle: [u64; 4],
    pub n_truncated: u64,
    pub n_tasks: u64,
    pub n_runner: u64,
    pub n_runner_listed: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_campaign_t {
    pub seeds_run: u64,
    pub batches_run: u64,
    pub batches_launched: u64,
    pub first_failing_seed: u64,
    pub n_failed: u64,
    pub n_runner: u64,
    pub total_steps: u64,
    pub total_clock_ns: u64,
    pub kernel_ms: f64,
    pub wall_s: f64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_failure_t {
    pub seed: u64,
    pub result: madsim_result_t,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_collect_t {
    pub failures: *const madsim_failure_t,
    pub cap: u64,
    pub n_listed: u64,
    pub n_by_verdict: [u64; 8],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_extreme_t {
    pub value: u64,
    pub seed: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_metric_t {
    pub min: u64,
    pub max: u64,
    pub sum_lo: u64,
    pub sum_hi: u64,
    pub hist: [u64; 256],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_stats_t {
    pub include: u32,
    pub top_k: u32,
    pub top: *const madsim_extreme_t,
    pub n: u64,
    pub n_top: u64,
    pub metric: [madsim_metric_t; 4],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_group_t {
    pub key: u64,
    pub verdict: u32,
    pub reserved: u32,
    pub count: u64,
    pub first_seed: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_groups_t {
    pub include: u32,
    pub key_field: u32,
    pub groups: *const madsim_group_t,
    pub cap: u64,
    pub n_groups: u64,
    pub n_grouped: u64,
    pub n_ungrouped: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_diff_record_t {
    pub seed: u64,
    pub a: madsim_result_t,
    pub b: madsim_result_t,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_diff_t {
    pub fields: u32,
    pub reserved: u32,
    pub records: *const madsim_diff_record_t,
    pub cap: u64,
    pub n_listed: u64,
    pub n_compared: u64,
    pub n_incomparable: u64,
    pub n_differ: u64,
    pub n_by_field: [u64; 8],
    pub transitions: [[u64; 8]; 8],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_resolve_t {
    pub n_first_pass: u64,
    pub n_resolved: u64,
    pub n_unresolved: u64,
    pub n_by_round: [u64; 8],
    pub batches_resolved: u64,
    pub rounds: u32,
    pub reserved: u32,
    pub rerun_kernel_ms: f64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_sweep_variant_t {
    pub w: *const madsim_workload_t,
    pub cfg: *const madsim_config_t,
    pub lim: *const madsim_limits_t,
    pub out: *const madsim_campaign_t,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_sweep_record_t {
    pub seed: u64,
    pub fail_mask: u32,
    pub differ_mask: u32,
    pub verdict: [u8; 8],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_sweep_t {
    pub fields: u32,
    pub list_rule: u32,
    pub records: *const madsim_sweep_record_t,
    pub cap: u64,
    pub n_listed: u64,
    pub n_selected: u64,
    pub n_settled: u64,
    pub n_incomparable: u64,
    pub n_runner_by_variant: [u64; 8],
    pub n_differ_from_first: [u64; 8],
    pub n_by_mask: [u64; 256],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_paired_extreme_t {
    pub seed: u64,
    pub a: u64,
    pub b: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_paired_t {
    pub include_a: u32,
    pub include_b: u32,
    pub top_k: u32,
    pub reserved: u32,
    pub top: *const madsim_paired_extreme_t,
    pub n_paired: u64,
    pub n_unpaired: u64,
    pub n_incomparable: u64,
    pub n_top: [u64; 8],
    pub n: [u64; 8],
    pub n_equal: [u64; 4],
    pub sum_a_lo: [u64; 4],
    pub sum_a_hi: [u64; 4],
    pub sum_b_lo: [u64; 4],
    pub sum_b_hi: [u64; 4],
    pub delta: [madsim_metric_t; 8],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct madsim_geometry_t {
    pub lds_bytes_per_seed: u32,
    pub lds_bytes_per_block: u32,
    pub block_threads: u32,
    pub blocks_per_cu: u32,
    pub grid_blocks: u32,
    pub heap_lds_slots: u32,
    pub heap_spill_slots: u32,
    pub max_tasks: u32,
    pub lanes_per_wave: u32,
    pub variant: u32,
    pub global_bytes_per_seed: u32,
}

// ---- enum madsim_op / enum madsim_verdict -------------------------------------------------------------------------
pub const MS_OP_DONE: u8 = 0;
pub const MS_OP_SPAWN: u8 = 1;
pub const MS_OP_JOIN: u8 = 2;
pub const MS_OP_ABORT: u8 = 3;
pub const MS_OP_YIELD: u8 = 4;
pub const MS_OP_PANIC: u8 = 5;
pub const MS_OP_SET: u8 = 6;
pub const MS_OP_DJNZ: u8 = 7;
pub const MS_OP_JMP: u8 = 8;
pub const MS_OP_TRACE: u8 = 9;
pub const MS_OP_BUILD: u8 = 15;
pub const MS_OP_SLEEP: u8 = 10;
pub const MS_OP_MARK: u8 = 11;
pub const MS_OP_SLEEP_UNTIL: u8 = 12;
pub const MS_OP_ASSERT_ELAPSED: u8 = 13;
pub const MS_OP_ADVANCE: u8 = 14;
pub const MS_OP_BIND: u8 = 20;
pub const MS_OP_SEND: u8 = 21;
pub const MS_OP_REPLY: u8 = 22;
pub const MS_OP_RECV: u8 = 23;
pub const MS_OP_ASSERT_VAL: u8 = 24;
pub const MS_OP_RECV_TIMEOUT: u8 = 25;
pub const MS_OP_CLOSE: u8 = 26;
pub const MS_OP_KILL: u8 = 30;
pub const MS_OP_RESTART: u8 = 31;
pub const MS_OP_PAUSE: u8 = 32;
pub const MS_OP_RESUME: u8 = 33;
pub const MS_OP_CLOG_NODE: u8 = 34;
pub const MS_OP_UNCLOG_NODE: u8 = 35;
pub const MS_OP_CLOG_LINK: u8 = 36;
pub const MS_OP_UNCLOG_LINK: u8 = 37;
pub const MS_OP_ASSERT_EXIT: u8 = 38;
pub const MS_OP_SET_LOSS: u8 = 39;
pub const MS_OP_SLEEP_RAND: u8 = 40;
pub const MS_OP_GSET: u8 = 41;
pub const MS_OP_GADD: u8 = 42;
pub const MS_OP_ASSERT_G: u8 = 43;
pub const MS_OP_PANIC_IF_G_LT: u8 = 44;
pub const MS_OP_JEQ: u8 = 45;
pub const MS_OP_CONNECT: u8 = 46;
pub const MS_OP_ACCEPT: u8 = 47;
pub const MS_OP_CSEND: u8 = 48;
pub const MS_OP_CRECV: u8 = 49;
pub const MS_OP_CCLOSE: u8 = 50;
pub const MS_OP_RPC_CALL: u8 = 51;
pub const MS_OP_RPC_REPLY: u8 = 52;
pub const MS_OP_RAND_BOOL: u8 = 53;
pub const MS_OP_RANDOM: u8 = 54;
pub const MS_OP_TRACE_TIME: u8 = 55;
pub const MS_OP_HOOK_REQ: u8 = 56;
pub const MS_OP_HOOK_RSP: u8 = 57;
pub const MS_OP_IPVS: u8 = 58;
pub const MS_OP_SET_LATENCY: u8 = 59;
pub const MS_OP_TIMEOUT_BEGIN: u8 = 60;
pub const MS_OP_TIMEOUT_END: u8 = 61;
pub const MS_OP_INTERVAL: u8 = 62;
pub const MS_OP_TICK: u8 = 63;
pub const MS_OP_INTERVAL_RESET: u8 = 64;
pub const MS_OP_RECV_OR_TICK: u8 = 65;
pub const MS_OP_RECV_TIMEOUT_AT: u8 = 66;
pub const MS_OP_CTRL_C: u8 = 67;
pub const MS_OP_SEND_CTRL_C: u8 = 68;
pub const MS_OP_RECV_OR_CTRL_C: u8 = 69;
pub const MADSIM_PASS: u32 = 0;
pub const MADSIM_PANIC: u32 = 1;
pub const MADSIM_DEADLOCK: u32 = 2;
pub const MADSIM_TIME_LIMIT: u32 = 3;
pub const MADSIM_OVERFLOW: u32 = 4;
pub const MADSIM_STEP_LIMIT: u32 = 5;
pub const MADSIM_UNSUPPORTED: u32 = 6;
pub const MADSIM_INTERNAL: u32 = 7;

// ---- #define constants -------------------------------------------------------------------------------------------
pub const MADSIM_HIP_ABI_VERSION: u32 = 7;
pub const MADSIM_IPVS_ADD_SERVICE: u32 = 0;
pub const MADSIM_IPVS_DEL_SERVICE: u32 = 1;
pub const MADSIM_IPVS_ADD_SERVER: u32 = 2;
pub const MADSIM_IPVS_DEL_SERVER: u32 = 3;
pub const MADSIM_TAG_RPC_FIRST: u32 = 0x80;
pub const MADSIM_TAG_RPC_LAST: u32 = 0xFD;
pub const MADSIM_SPAWN_MOVE_CONN: u32 = 2;
pub const MADSIM_SPAWN_MOVE_REQUEST: u32 = 4;
pub const MADSIM_VAL_TIMEOUT: u32 = 0xFFFFFFFF;
pub const MADSIM_VAL_REFUSED: u32 = 0xFFFFFFFE;
pub const MADSIM_VAL_RESET: u32 = 0xFFFFFFFD;
pub const MADSIM_VAL_ADDR_NOT_AVAILABLE: u32 = 0xFFFFFFFC;
pub const MADSIM_VAL_ADDR_IN_USE: u32 = 0xFFFFFFFB;
pub const MADSIM_PROG_INIT: u32 = 1;
pub const MADSIM_PROG_PRE: u32 = 2;
pub const MADSIM_PROG_DROP_SPAWN: u32 = 4;
pub const MADSIM_ADDR_IP: u32 = 0;
pub const MADSIM_ADDR_UNSPECIFIED: u32 = 1;
pub const MADSIM_ADDR_LOOPBACK: u32 = 2;
pub const MADSIM_ADDR_VIRTUAL: u32 = 3;
pub const MADSIM_MAX_SERVICES: u32 = 8;
pub const MADSIM_SERVICE_ABSENT: u32 = 0x80;
pub const MADSIM_NODE_RESTART_ON_PANIC: u32 = 1;
pub const MADSIM_NODE_RESTART_MATCHING: u32 = 4;
pub const MADSIM_PANIC_CODE_OTHER: u32 = 255;
pub const MADSIM_NODE_NO_IP: u32 = 2;
pub const MADSIM_LIMIT_NONE: u32 = 0xffffffff;
pub const MADSIM_STATE_AUTO: u32 = 0;
pub const MADSIM_STATE_LDS: u32 = 1;
pub const MADSIM_STATE_GLOBAL: u32 = 2;
pub const MADSIM_STATE_COMPACT: u32 = 3;
pub const MADSIM_STATE_DEDUP_TIMERS: u32 = 0x100;
pub const MADSIM_STATE_NARROW_HEAP: u32 = 0x200;
pub const MADSIM_SCHED_STATIC: u32 = 0;
pub const MADSIM_SCHED_QUEUE: u32 = 1;
pub const MADSIM_MAX_LIVE_TASKS: u32 = 254;
pub const MADSIM_MAX_MBOX_REGS: u32 = 255;
pub const MADSIM_MAX_CHAN_QUEUE: u32 = 15;
pub const MADSIM_MAX_CONNS: u32 = 127;
pub const MADSIM_MAX_MBOX_MSGS: u32 = 255;
pub const MADSIM_MAX_SOCKET_GUARDS: u32 = 127;
pub const MADSIM_E_ARG: c_int = -1;
pub const MADSIM_E_HIP: c_int = -2;
pub const MADSIM_E_NOINIT: c_int = -3;
pub const MADSIM_E_WORKLOAD: c_int = -4;
pub const MADSIM_E_LIMITS: c_int = -5;
pub const MADSIM_TRACE_MAX_BYTES: u32 = 1073741824;
pub const MADSIM_TASK_PARKED: u32 = 1;
pub const MADSIM_TASK_QUEUED: u32 = 2;
pub const MADSIM_TASK_PANICKED: u32 = 3;
pub const MADSIM_TASK_CANCELLED: u32 = 4;
pub const MADSIM_DIVERGE_SAME: u32 = 0;
pub const MADSIM_DIVERGE_DIFFER: u32 = 1;
pub const MADSIM_DIVERGE_PREFIX: u32 = 2;
pub const MADSIM_DIVERGE_BEYOND_CAP: u32 = 3;
pub const MADSIM_DIVERGE_INCOMPARABLE: u32 = 4;
pub const MADSIM_DIVERGE_MAX_WIN: u32 = 8;
pub const MADSIM_CENSUS_MAX_VALUES: u32 = 1048576;
pub const MADSIM_CENSUS_MAX_OBS_CAP: u32 = 1024;
pub const MADSIM_PROBE_SETS_MAX_VOCAB: u32 = 62;
pub const MADSIM_PROBE_SETS_MAX: u32 = 1048576;
pub const MADSIM_PROBE_SET_OTHER: u64 = 0x4000000000000000;
pub const MADSIM_PROBE_SET_TRUNCATED: u64 = 0x8000000000000000;
pub const MADSIM_PROBE_ORDER_MAX_VOCAB: u32 = 32;
pub const MADSIM_PROBE_SPANS_MAX: u32 = 16;
pub const MADSIM_SPAN_FROM_START: u32 = 1;
pub const MADSIM_SPAN_ABSENT: u32 = 0;
pub const MADSIM_SPAN_CLOSED: u32 = 1;
pub const MADSIM_SPAN_OPEN: u32 = 2;
pub const MADSIM_SPAN_CUT: u32 = 3;
pub const MADSIM_CAMPAIGN_STOP_AT_FAILURE: u32 = 1;
pub const MADSIM_CAMPAIGN_LIST_RUNNER: u32 = 2;
pub const MADSIM_CAMPAIGN_STOP_AT_CAP: u32 = 4;
pub const MADSIM_STAT_CLOCK: u32 = 0;
pub const MADSIM_STAT_STEPS: u32 = 1;
pub const MADSIM_STAT_MSGS: u32 = 2;
pub const MADSIM_STAT_RNG: u32 = 3;
pub const MADSIM_STAT_METRICS: u32 = 4;
pub const MADSIM_STAT_BUCKETS: u32 = 256;
pub const MADSIM_STAT_MAX_TOP: u32 = 16;
pub const MADSIM_GROUP_KEY_OBS: u32 = 0;
pub const MADSIM_GROUP_KEY_TRACE: u32 = 1;
pub const MADSIM_GROUP_KEY_MSGS: u32 = 2;
pub const MADSIM_GROUP_KEY_CLOCK: u32 = 3;
pub const MADSIM_GROUP_KEY_RNG: u32 = 4;
pub const MADSIM_GROUP_KEY_STEPS: u32 = 5;
pub const MADSIM_GROUP_KEYS: u32 = 6;
pub const MADSIM_GROUP_MAX_BATCH: u32 = 1048576;
pub const MADSIM_CAMPAIGN_STOP_AT_GROUPS: u32 = 8;
pub const MADSIM_DIFF_VERDICT: u32 = 1;
pub const MADSIM_DIFF_STEPS: u32 = 2;
pub const MADSIM_DIFF_CLOCK: u32 = 4;
pub const MADSIM_DIFF_MSGS: u32 = 8;
pub const MADSIM_DIFF_RNG: u32 = 16;
pub const MADSIM_DIFF_TRACE: u32 = 32;
pub const MADSIM_DIFF_OBS: u32 = 64;
pub const MADSIM_DIFF_ALL: u32 = 127;
pub const MADSIM_DIFF_FIELDS: u32 = 7;
pub const MADSIM_CAMPAIGN_STOP_AT_DIFFS: u32 = 16;
pub const MADSIM_CAMPAIGN_RESOLVE: u32 = 32;
pub const MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT: u32 = 8;
pub const MADSIM_CAMPAIGN_RESOLVE_ROUNDS_MASK: u32 = 3840;
pub const MADSIM_RESOLVE_DEFAULT_ROUNDS: u32 = 4;
pub const MADSIM_RESOLVE_MAX_ROUNDS: u32 = 8;
pub const MADSIM_SWEEP_MAX_VARIANTS: u32 = 8;
pub const MADSIM_SWEEP_LIST_MIXED: u32 = 0;
pub const MADSIM_SWEEP_LIST_FAILING: u32 = 1;
pub const MADSIM_SWEEP_LIST_DIFFERING: u32 = 2;
pub const MADSIM_CAMPAIGN_STOP_AT_SWEEP: u32 = 64;
pub const MADSIM_PAIRED_UP: u32 = 0;
pub const MADSIM_PAIRED_DOWN: u32 = 1;

#[link(name = "madsim_hip")]
extern "C" {
    pub fn madsim_hip_version() -> u32;
    pub fn madsim_hip_build_info() -> *const c_char;
    pub fn madsim_hip_strerror(code: c_int) -> *const c_char;
    pub fn madsim_hip_last_error() -> *const c_char;
    pub fn madsim_hip_prefer_hw_queues(n: c_int) -> c_int;
    pub fn madsim_hip_ctx_create(device: c_int, out: *mut *mut madsim_hip_ctx_t) -> c_int;
    pub fn madsim_hip_ctx_destroy(ctx: *mut madsim_hip_ctx_t) -> c_int;
    pub fn madsim_hip_ctx_device(ctx: *const madsim_hip_ctx_t) -> c_int;
    pub fn madsim_hip_default_ctx() -> *mut madsim_hip_ctx_t;
    pub fn madsim_hip_init(device: c_int) -> c_int;
    pub fn madsim_hip_shutdown() -> c_int;
    pub fn madsim_hip_run_batch(w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, count: u64, lim: *const madsim_limits_t, out: *mut madsim_result_t, summary: *mut madsim_summary_t) -> c_int;
    pub fn madsim_hip_run_batch_auto(w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, count: u64, lim: *const madsim_limits_t, out: *mut madsim_result_t, summary: *mut madsim_summary_t, max_rounds: c_int) -> c_int;
    pub fn madsim_hip_run_batch_device(w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, count: u64, lim: *const madsim_limits_t, d_out: *mut c_void, stream: *mut c_void, summary: *mut madsim_summary_t) -> c_int;
    pub fn madsim_hip_run_batch_async(w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, count: u64, lim: *const madsim_limits_t, d_out: *mut c_void, d_summary4: *mut c_void, stream: *mut c_void, timing_slot: c_int) -> c_int;
    pub fn madsim_hip_timing_ms(timing_slot: c_int, ms: *mut f64) -> c_int;
    pub fn madsim_hip_trace_seed(w: *const madsim_workload_t, cfg: *const madsim_config_t, seed: u64, lim: *const madsim_limits_t, log: *mut u8, cap: u64, out: *mut madsim_result_t) -> i64;
    pub fn madsim_hip_trace_seeds(w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, lim: *const madsim_limits_t, logs: *mut u8, log_cap: u64, obs: *mut u64, obs_cap: u64, log_len: *mut u64, obs_len: *mut u64, out: *mut madsim_result_t) -> c_int;
    pub fn madsim_hip_observe_seed(w: *const madsim_workload_t, cfg: *const madsim_config_t, seed: u64, lim: *const madsim_limits_t, obs: *mut u64, cap: u64, out: *mut madsim_result_t) -> i64;
    pub fn madsim_hip_task_states(w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, lim: *const madsim_limits_t, tasks: *mut u64, task_cap: u64, task_len: *mut u64, out: *mut madsim_result_t) -> c_int;
    pub fn madsim_hip_stall_shape(tasks: *const u64, n: u64) -> u64;
    pub fn madsim_hip_timeline_seeds(w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, lim: *const madsim_limits_t, obs: *mut u64, times: *mut u64, obs_cap: u64, obs_len: *mut u64, out: *mut madsim_result_t) -> c_int;
    pub fn madsim_hip_diverge_seeds(wA: *const madsim_workload_t, cfgA: *const madsim_config_t, limA: *const madsim_limits_t, wB: *const madsim_workload_t, cfgB: *const madsim_config_t, limB: *const madsim_limits_t, seeds: *const u64, n: u64, log_cap: u64, obs_cap: u64, win: u32, recs: *mut madsim_divergence_t, obs_ctx: *mut u64) -> c_int;
    pub fn madsim_hip_census_range(w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, chunk: u64, lim: *const madsim_limits_t, cen: *mut madsim_census_t) -> c_int;
    pub fn madsim_hip_census_seeds(w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, chunk: u64, lim: *const madsim_limits_t, cen: *mut madsim_census_t) -> c_int;
    pub fn madsim_hip_probe_sets_range(w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, chunk: u64, lim: *const madsim_limits_t, ps: *mut madsim_probe_sets_t) -> c_int;
    pub fn madsim_hip_probe_sets_seeds(w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, chunk: u64, lim: *const madsim_limits_t, ps: *mut madsim_probe_sets_t) -> c_int;
    pub fn madsim_hip_probe_order_range(w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, chunk: u64, lim: *const madsim_limits_t, po: *mut madsim_probe_order_t) -> c_int;
    pub fn madsim_hip_probe_order_seeds(w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, chunk: u64, lim: *const madsim_limits_t, po: *mut madsim_probe_order_t) -> c_int;
    pub fn madsim_hip_probe_spans_range(w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, chunk: u64, lim: *const madsim_limits_t, ps: *mut madsim_probe_spans_t) -> c_int;
    pub fn madsim_hip_probe_spans_seeds(w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, chunk: u64, lim: *const madsim_limits_t, ps: *mut madsim_probe_spans_t) -> c_int;
    pub fn madsim_hip_span_merge(into: *mut madsim_span_t, from: *const madsim_span_t);
    pub fn madsim_hip_stall_census_range(w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, chunk: u64, lim: *const madsim_limits_t, sc: *mut madsim_stall_census_t) -> c_int;
    pub fn madsim_hip_stall_census_seeds(w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, chunk: u64, lim: *const madsim_limits_t, sc: *mut madsim_stall_census_t) -> c_int;
    pub fn madsim_hip_ctx_run_batch(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, count: u64, lim: *const madsim_limits_t, out: *mut madsim_result_t, summary: *mut madsim_summary_t) -> c_int;
    pub fn madsim_hip_ctx_run_batch_auto(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, count: u64, lim: *const madsim_limits_t, out: *mut madsim_result_t, summary: *mut madsim_summary_t, max_rounds: c_int) -> c_int;
    pub fn madsim_hip_ctx_run_batch_device(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, count: u64, lim: *const madsim_limits_t, d_out: *mut c_void, stream: *mut c_void, summary: *mut madsim_summary_t) -> c_int;
    pub fn madsim_hip_ctx_run_batch_async(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, count: u64, lim: *const madsim_limits_t, d_out: *mut c_void, d_summary4: *mut c_void, stream: *mut c_void, timing_slot: c_int) -> c_int;
    pub fn madsim_hip_ctx_timing_ms(ctx: *mut madsim_hip_ctx_t, timing_slot: c_int, ms: *mut f64) -> c_int;
    pub fn madsim_hip_ctx_trace_seed(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed: u64, lim: *const madsim_limits_t, log: *mut u8, cap: u64, out: *mut madsim_result_t) -> i64;
    pub fn madsim_hip_ctx_trace_seeds(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, lim: *const madsim_limits_t, logs: *mut u8, log_cap: u64, obs: *mut u64, obs_cap: u64, log_len: *mut u64, obs_len: *mut u64, out: *mut madsim_result_t) -> c_int;
    pub fn madsim_hip_ctx_observe_seed(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed: u64, lim: *const madsim_limits_t, obs: *mut u64, cap: u64, out: *mut madsim_result_t) -> i64;
    pub fn madsim_hip_ctx_task_states(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, lim: *const madsim_limits_t, tasks: *mut u64, task_cap: u64, task_len: *mut u64, out: *mut madsim_result_t) -> c_int;
    pub fn madsim_hip_ctx_timeline_seeds(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, lim: *const madsim_limits_t, obs: *mut u64, times: *mut u64, obs_cap: u64, obs_len: *mut u64, out: *mut madsim_result_t) -> c_int;
    pub fn madsim_hip_ctx_diverge_seeds(ctx: *mut madsim_hip_ctx_t, wA: *const madsim_workload_t, cfgA: *const madsim_config_t, limA: *const madsim_limits_t, wB: *const madsim_workload_t, cfgB: *const madsim_config_t, limB: *const madsim_limits_t, seeds: *const u64, n: u64, log_cap: u64, obs_cap: u64, win: u32, recs: *mut madsim_divergence_t, obs_ctx: *mut u64) -> c_int;
    pub fn madsim_hip_ctx_census_range(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, chunk: u64, lim: *const madsim_limits_t, cen: *mut madsim_census_t) -> c_int;
    pub fn madsim_hip_ctx_census_seeds(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, chunk: u64, lim: *const madsim_limits_t, cen: *mut madsim_census_t) -> c_int;
    pub fn madsim_hip_ctx_probe_sets_range(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, chunk: u64, lim: *const madsim_limits_t, ps: *mut madsim_probe_sets_t) -> c_int;
    pub fn madsim_hip_ctx_probe_sets_seeds(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, chunk: u64, lim: *const madsim_limits_t, ps: *mut madsim_probe_sets_t) -> c_int;
    pub fn madsim_hip_ctx_probe_order_range(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, chunk: u64, lim: *const madsim_limits_t, po: *mut madsim_probe_order_t) -> c_int;
    pub fn madsim_hip_ctx_probe_order_seeds(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, chunk: u64, lim: *const madsim_limits_t, po: *mut madsim_probe_order_t) -> c_int;
    pub fn madsim_hip_ctx_probe_spans_range(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, chunk: u64, lim: *const madsim_limits_t, ps: *mut madsim_probe_spans_t) -> c_int;
    pub fn madsim_hip_ctx_probe_spans_seeds(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, chunk: u64, lim: *const madsim_limits_t, ps: *mut madsim_probe_spans_t) -> c_int;
    pub fn madsim_hip_ctx_stall_census_range(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, chunk: u64, lim: *const madsim_limits_t, sc: *mut madsim_stall_census_t) -> c_int;
    pub fn madsim_hip_ctx_stall_census_seeds(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, chunk: u64, lim: *const madsim_limits_t, sc: *mut madsim_stall_census_t) -> c_int;
    pub fn madsim_hip_run_batch_multi(ctxs: *const *mut madsim_hip_ctx_t, n_ctx: c_int, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, count: u64, lim: *const madsim_limits_t, out: *mut madsim_result_t, summary: *mut madsim_summary_t, max_rounds: c_int) -> c_int;
    pub fn madsim_hip_ctx_run_campaign(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, batch: u64, in_flight: u32, flags: u32, lim: *const madsim_limits_t, out: *mut madsim_campaign_t) -> c_int;
    pub fn madsim_hip_run_campaign(w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, batch: u64, in_flight: u32, flags: u32, lim: *const madsim_limits_t, out: *mut madsim_campaign_t) -> c_int;
    pub fn madsim_hip_run_campaign_multi(ctxs: *const *mut madsim_hip_ctx_t, n_ctx: c_int, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, batch: u64, in_flight: u32, flags: u32, lim: *const madsim_limits_t, out: *mut madsim_campaign_t) -> c_int;
    pub fn madsim_hip_ctx_run_campaign_collect(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, batch: u64, in_flight: u32, flags: u32, lim: *const madsim_limits_t, out: *mut madsim_campaign_t, col: *mut madsim_collect_t) -> c_int;
    pub fn madsim_hip_run_campaign_collect(w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, batch: u64, in_flight: u32, flags: u32, lim: *const madsim_limits_t, out: *mut madsim_campaign_t, col: *mut madsim_collect_t) -> c_int;
    pub fn madsim_hip_run_campaign_collect_multi(ctxs: *const *mut madsim_hip_ctx_t, n_ctx: c_int, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, batch: u64, in_flight: u32, flags: u32, lim: *const madsim_limits_t, out: *mut madsim_campaign_t, col: *mut madsim_collect_t) -> c_int;
    pub fn madsim_hip_stat_bucket(v: u64) -> u32;
    pub fn madsim_hip_stat_bucket_floor(b: u32) -> u64;
    pub fn madsim_hip_ctx_run_campaign_stats(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, batch: u64, in_flight: u32, flags: u32, lim: *const madsim_limits_t, out: *mut madsim_campaign_t, col: *mut madsim_collect_t, st: *mut madsim_stats_t) -> c_int;
    pub fn madsim_hip_run_campaign_stats(w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, batch: u64, in_flight: u32, flags: u32, lim: *const madsim_limits_t, out: *mut madsim_campaign_t, col: *mut madsim_collect_t, st: *mut madsim_stats_t) -> c_int;
    pub fn madsim_hip_run_campaign_stats_multi(ctxs: *const *mut madsim_hip_ctx_t, n_ctx: c_int, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, batch: u64, in_flight: u32, flags: u32, lim: *const madsim_limits_t, out: *mut madsim_campaign_t, col: *mut madsim_collect_t, st: *mut madsim_stats_t) -> c_int;
    pub fn madsim_hip_ctx_run_campaign_groups(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, batch: u64, in_flight: u32, flags: u32, lim: *const madsim_limits_t, out: *mut madsim_campaign_t, col: *mut madsim_collect_t, st: *mut madsim_stats_t, grp: *mut madsim_groups_t) -> c_int;
    pub fn madsim_hip_run_campaign_groups(w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, batch: u64, in_flight: u32, flags: u32, lim: *const madsim_limits_t, out: *mut madsim_campaign_t, col: *mut madsim_collect_t, st: *mut madsim_stats_t, grp: *mut madsim_groups_t) -> c_int;
    pub fn madsim_hip_run_campaign_groups_multi(ctxs: *const *mut madsim_hip_ctx_t, n_ctx: c_int, w: *const madsim_workload_t, cfg: *const madsim_config_t, seed0: u64, total: u64, batch: u64, in_flight: u32, flags: u32, lim: *const madsim_limits_t, out: *mut madsim_campaign_t, col: *mut madsim_collect_t, st: *mut madsim_stats_t, grp: *mut madsim_groups_t) -> c_int;
    pub fn madsim_hip_ctx_run_campaign_diff(ctx: *mut madsim_hip_ctx_t, wA: *const madsim_workload_t, cfgA: *const madsim_config_t, limA: *const madsim_limits_t, wB: *const madsim_workload_t, cfgB: *const madsim_config_t, limB: *const madsim_limits_t, seed0: u64, total: u64, batch: u64, in_flight: u32, flags: u32, outA: *mut madsim_campaign_t, outB: *mut madsim_campaign_t, diff: *mut madsim_diff_t) -> c_int;
    pub fn madsim_hip_run_campaign_diff(wA: *const madsim_workload_t, cfgA: *const madsim_config_t, limA: *const madsim_limits_t, wB: *const madsim_workload_t, cfgB: *const madsim_config_t, limB: *const madsim_limits_t, seed0: u64, total: u64, batch: u64, in_flight: u32, flags: u32, outA: *mut madsim_campaign_t, outB: *mut madsim_campaign_t, diff: *mut madsim_diff_t) -> c_int;
    pub fn madsim_hip_run_campaign_diff_multi(ctxs: *const *mut madsim_hip_ctx_t, n_ctx: c_int, wA: *const madsim_workload_t, cfgA: *const madsim_config_t, limA: *const madsim_limits_t, wB: *const madsim_workload_t, cfgB: *const madsim_config_t, limB: *const madsim_limits_t, seed0: u64, total: u64, batch: u64, in_flight: u32, flags: u32, outA: *mut madsim_campaign_t, outB: *mut madsim_campaign_t, diff: *mut madsim_diff_t) -> c_int;
    pub fn madsim_hip_campaign_resolved(out: *mut madsim_resolve_t) -> c_int;
    pub fn madsim_hip_ctx_campaign_resolved(ctx: *mut madsim_hip_ctx_t, out: *mut madsim_resolve_t) -> c_int;
    pub fn madsim_hip_grow_limits(w: *const madsim_workload_t, lim: *const madsim_limits_t, rounds: u32, out: *mut madsim_limits_t) -> c_int;
    pub fn madsim_hip_ctx_run_seeds_campaign(ctx: *mut madsim_hip_ctx_t, w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, batch: u64, in_flight: u32, flags: u32, lim: *const madsim_limits_t, out: *mut madsim_campaign_t, col: *mut madsim_collect_t, st: *mut madsim_stats_t, grp: *mut madsim_groups_t) -> c_int;
    pub fn madsim_hip_run_seeds_campaign(w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, batch: u64, in_flight: u32, flags: u32, lim: *const madsim_limits_t, out: *mut madsim_campaign_t, col: *mut madsim_collect_t, st: *mut madsim_stats_t, grp: *mut madsim_groups_t) -> c_int;
    pub fn madsim_hip_run_seeds_campaign_multi(ctxs: *const *mut madsim_hip_ctx_t, n_ctx: c_int, w: *const madsim_workload_t, cfg: *const madsim_config_t, seeds: *const u64, n: u64, batch: u64, in_flight: u32, flags: u32, lim: *const madsim_limits_t, out: *mut madsim_campaign_t, col: *mut madsim_collect_t, st: *mut madsim_stats_t, grp: *mut madsim_groups_t) -> c_int;
    pub fn madsim_hip_ctx_run_seeds_campaign_diff(ctx: *mut madsim_hip_ctx_t, wA: *const madsim_workload_t, cfgA: *const madsim_config_t, limA: *const madsim_limits_t, wB: *const madsim_workload_t, cfgB: *const madsim_config_t, limB: *const madsim_limits_t, seeds: *const u64, n: u64, batch: u64, in_flight: u32, flags: u32, outA: *mut madsim_campaign_t, outB: *mut madsim_campaign_t, diff: *mut madsim_diff_t) -> c_int;
    pub fn madsim_hip_run_seeds_campaign_diff(wA: *const madsim_workload_t, cfgA: *const madsim_config_t, limA: *const madsim_limits_t, wB: *const madsim_workload_t, cfgB: *const madsim_config_t, limB: *const madsim_limits_t, seeds: *const u64, n: u64, batch: u64, in_flight: u32, flags: u32, outA: *mut madsim_campaign_t, outB: *mut madsim_campaign_t, diff: *mut madsim_diff_t) -> c_int;
    pub fn madsim_hip_run_seeds_campaign_diff_multi(ctxs: *const *mut madsim_hip_ctx_t, n_ctx: c_int, wA: *const madsim_workload_t, cfgA: *const madsim_config_t, limA: *const madsim_limits_t, wB: *const madsim_workload_t, cfgB: *const madsim_config_t, limB: *const madsim_limits_t, seeds: *const u64, n: u64, batch: u64, in_flight: u32, flags: u32, outA: *mut madsim_campaign_t, outB: *mut madsim_campaign_t, diff: *mut madsim_diff_t) -> c_int;
    pub fn madsim_hip_ctx_run_sweep_campaign(ctx: *mut madsim_hip_ctx_t, variants: *const madsim_sweep_variant_t, n_variants: u32, seed0: u64, total: u64, seeds: *const u64, batch: u64, in_flight: u32, flags: u32, sweep: *mut madsim_sweep_t) -> c_int;
    pub fn madsim_hip_run_sweep_campaign(variants: *const madsim_sweep_variant_t, n_variants: u32, seed0: u64, total: u64, seeds: *const u64, batch: u64, in_flight: u32, flags: u32, sweep: *mut madsim_sweep_t) -> c_int;
    pub fn madsim_hip_run_sweep_campaign_multi(ctxs: *const *mut madsim_hip_ctx_t, n_ctx: c_int, variants: *const madsim_sweep_variant_t, n_variants: u32, seed0: u64, total: u64, seeds: *const u64, batch: u64, in_flight: u32, flags: u32, sweep: *mut madsim_sweep_t) -> c_int;
    pub fn madsim_hip_ctx_run_paired_campaign(ctx: *mut madsim_hip_ctx_t, wA: *const madsim_workload_t, cfgA: *const madsim_config_t, limA: *const madsim_limits_t, wB: *const madsim_workload_t, cfgB: *const madsim_config_t, limB: *const madsim_limits_t, seed0: u64, total: u64, batch: u64, in_flight: u32, flags: u32, outA: *mut madsim_campaign_t, outB: *mut madsim_campaign_t, diff: *mut madsim_diff_t, pr: *mut madsim_paired_t) -> c_int;
    pub fn madsim_hip_run_paired_campaign(wA: *const madsim_workload_t, cfgA: *const madsim_config_t, limA: *const madsim_limits_t, wB: *const madsim_workload_t, cfgB: *const madsim_config_t, limB: *const madsim_limits_t, seed0: u64, total: u64, batch: u64, in_flight: u32, flags: u32, outA: *mut madsim_campaign_t, outB: *mut madsim_campaign_t, diff: *mut madsim_diff_t, pr: *mut madsim_paired_t) -> c_int;
    pub fn madsim_hip_run_paired_campaign_multi(ctxs: *const *mut madsim_hip_ctx_t, n_ctx: c_int, wA: *const madsim_workload_t, cfgA: *const madsim_config_t, limA: *const madsim_limits_t, wB: *const madsim_workload_t, cfgB: *const madsim_config_t, limB: *const madsim_limits_t, seed0: u64, total: u64, batch: u64, in_flight: u32, flags: u32, outA: *mut madsim_campaign_t, outB: *mut madsim_campaign_t, diff: *mut madsim_diff_t, pr: *mut madsim_paired_t) -> c_int;
    pub fn madsim_hip_ctx_run_seeds_campaign_paired(ctx: *mut madsim_hip_ctx_t, wA: *const madsim_workload_t, cfgA: *const madsim_config_t, limA: *const madsim_limits_t, wB: *const madsim_workload_t, cfgB: *const madsim_config_t, limB: *const madsim_limits_t, seeds: *const u64, n: u64, batch: u64, in_flight: u32, flags: u32, outA: *mut madsim_campaign_t, outB: *mut madsim_campaign_t, diff: *mut madsim_diff_t, pr: *mut madsim_paired_t) -> c_int;
    pub fn madsim_hip_run_seeds_campaign_paired(wA: *const madsim_workload_t, cfgA: *const madsim_config_t, limA: *const madsim_limits_t, wB: *const madsim_workload_t, cfgB: *const madsim_config_t, limB: *const madsim_limits_t, seeds: *const u64, n: u64, batch: u64, in_flight: u32, flags: u32, outA: *mut madsim_campaign_t, outB: *mut madsim_campaign_t, diff: *mut madsim_diff_t, pr: *mut madsim_paired_t) -> c_int;
    pub fn madsim_hip_run_seeds_campaign_paired_multi(ctxs: *const *mut madsim_hip_ctx_t, n_ctx: c_int, wA: *const madsim_workload_t, cfgA: *const madsim_config_t, limA: *const madsim_limits_t, wB: *const madsim_workload_t, cfgB: *const madsim_config_t, limB: *const madsim_limits_t, seeds: *const u64, n: u64, batch: u64, in_flight: u32, flags: u32, outA: *mut madsim_campaign_t, outB: *mut madsim_campaign_t, diff: *mut madsim_diff_t, pr: *mut madsim_paired_t) -> c_int;
    pub fn madsim_hip_geometry(w: *const madsim_workload_t, lim: *const madsim_limits_t, g: *mut madsim_geometry_t) -> c_int;
    pub fn madsim_hip_debug_counters(out16: *mut u64) -> c_int;
    pub fn madsim_workload_pingpong(n_nodes: u32, rounds: u32, nodes: *mut madsim_node_t, progs: *mut madsim_prog_t, socks: *mut madsim_sock_t, insns: *mut madsim_insn_t, cap_insns: u32, w: *mut madsim_workload_t) -> c_int;
}
