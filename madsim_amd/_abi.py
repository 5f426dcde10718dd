"""ctypes mirror of include/madsim_hip.h (the C-ABI drop-in boundary).

Pure data definitions: no device code, no oracle.  Both the product loader
(`madsim_amd.runtime`) and the test-only oracle loader (`oracle/`) feed these
same structs, so a parity test hands identical bytes to both sides.
"""
import ctypes as C

ABI_VERSION = 7
U64_MAX = (1 << 64) - 1
LIMIT_NONE = 0xFFFFFFFF
SCHED_STATIC, SCHED_QUEUE = 0, 1
STATE_AUTO, STATE_LDS, STATE_GLOBAL, STATE_COMPACT = 0, 1, 2, 3
STATE_DEDUP_TIMERS = 0x100     # OR-ed into state_mem: re-registered Sleep timers as counts (include/madsim_hip.h)
STATE_NARROW_HEAP = 0x200      # OR-ed into state_mem: 8-byte timer-heap entries + delivery record pool (global-state builds with a spill region)
VAL_TIMEOUT = 0xFFFFFFFF
VAL_REFUSED = 0xFFFFFFFE
VAL_RESET = 0xFFFFFFFD


class Insn(C.Structure):
    _fields_ = [("op", C.c_uint8), ("a", C.c_uint8), ("b", C.c_uint16), ("imm", C.c_uint32)]


class Prog(C.Structure):
    _fields_ = [("node", C.c_uint8), ("flags", C.c_uint8), ("entry", C.c_uint16)]


ADDR_IP, ADDR_UNSPECIFIED, ADDR_LOOPBACK, ADDR_VIRTUAL = 0, 1, 2, 3
MAX_SERVICES = 8
SERVICE_ABSENT = 0x80       # madsim_service_t.n_servers: the address is declared, the service added by a task (MS_OP_IPVS)
IPVS_ADD_SERVICE, IPVS_DEL_SERVICE, IPVS_ADD_SERVER, IPVS_DEL_SERVER = 0, 1, 2, 3
VAL_ADDR_NOT_AVAILABLE, VAL_ADDR_IN_USE = 0xFFFFFFFC, 0xFFFFFFFB
NODE_NO_IP = 2


class Sock(C.Structure):
    _fields_ = [("node", C.c_uint8), ("kind", C.c_uint8), ("port", C.c_uint16)]


class Node(C.Structure):
    _fields_ = [("flags", C.c_uint8), ("n_match", C.c_uint8), ("match", C.c_uint8 * 2)]


class Service(C.Structure):
    """madsim_service_t: one IPVS virtual service (net/ipvs.rs) — address entry + real servers in add_server order."""
    _fields_ = [("vaddr", C.c_uint8), ("n_servers", C.c_uint8), ("servers", C.c_uint8 * 6)]


class Workload(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_uint32), ("n_progs", C.c_uint32), ("n_socks", C.c_uint32), ("n_insns", C.c_uint32),
        ("nodes", C.POINTER(Node)), ("progs", C.POINTER(Prog)), ("socks", C.POINTER(Sock)),
        ("insns", C.POINTER(Insn)),
        ("n_services", C.c_uint32), ("panic_dyn_max", C.c_uint32), ("services", C.POINTER(Service)),
        ("panic_match", C.POINTER(C.c_uint32)),
    ]


HEADER_STRUCTS = {"madsim_service_t": Service}          # + madsim_campaign_t, registered below its definition


class Config(C.Structure):
    """madsim::Config.net (net/network.rs:66-89) + the buggify switch (rand.rs:113-134)."""
    _fields_ = [
        ("packet_loss_rate", C.c_double), ("lat_lo_ns", C.c_uint64), ("lat_hi_ns", C.c_uint64),
        ("buggify", C.c_uint32), ("n_loss_table", C.c_uint32), ("loss_table", C.c_double * 4),
        ("n_lat_table", C.c_uint32), ("reserved0", C.c_uint32), ("lat_table_lo_ns", C.c_uint64 * 4), ("lat_table_hi_ns", C.c_uint64 * 4),
    ]

    @classmethod
    def default(cls, packet_loss_rate=0.0, lat_lo_ns=1_000_000, lat_hi_ns=10_000_000, buggify=False,
                loss_table=(), lat_table=()):
        """`lat_table`: up to four (lo_ns, hi_ns) ranges that MS_OP_SET_LATENCY (TaskBuilder.set_latency) switches between."""
        c = cls()
        c.n_lat_table = len(lat_table)
        for i, (lo, hi) in enumerate(lat_table):
            c.lat_table_lo_ns[i], c.lat_table_hi_ns[i] = lo, hi
        c.packet_loss_rate = packet_loss_rate
        c.lat_lo_ns, c.lat_hi_ns = lat_lo_ns, lat_hi_ns
        c.buggify = 1 if buggify else 0
        c.n_loss_table = len(loss_table)
        for i, p in enumerate(loss_table):
            c.loss_table[i] = p
        return c


class Limits(C.Structure):
    _fields_ = [
        ("time_limit_ns", C.c_uint64), ("max_steps", C.c_uint32), ("heap_lds_slots", C.c_uint32),
        ("heap_spill_slots", C.c_uint32), ("max_tasks", C.c_uint32), ("mbox_regs", C.c_uint32),
        ("mbox_msgs", C.c_uint32), ("lanes_per_wave", C.c_uint32), ("max_conns", C.c_uint32), ("chan_queue", C.c_uint32),
        ("sched", C.c_uint32), ("state_mem", C.c_uint32), ("max_steps_ceiling", C.c_uint32), ("no_trace_hash", C.c_uint32),
    ]


class Result(C.Structure):
    _fields_ = [
        ("verdict", C.c_uint32), ("steps", C.c_uint32), ("clock_ns", C.c_uint64), ("msg_count", C.c_uint64),
        ("rng_calls", C.c_uint64), ("trace_hash", C.c_uint64), ("obs_hash", C.c_uint64),
    ]

    def astuple(self):
        return (self.verdict, self.steps, self.clock_ns, self.msg_count, self.rng_calls, self.trace_hash,
                self.obs_hash)


class Summary(C.Structure):
    _fields_ = [
        ("first_failing_seed", C.c_uint64), ("n_failed", C.c_uint64), ("total_steps", C.c_uint64),
        ("total_clock_ns", C.c_uint64), ("kernel_ms", C.c_double), ("wall_s", C.c_double),
    ]


class Campaign(C.Structure):
    """madsim_campaign_t: the report of madsim_hip_run_campaign (batches kept in flight by the library)."""
    _fields_ = [
        ("seeds_run", C.c_uint64), ("batches_run", C.c_uint64), ("batches_launched", C.c_uint64),
        ("first_failing_seed", C.c_uint64), ("n_failed", C.c_uint64), ("n_runner", C.c_uint64),
        ("total_steps", C.c_uint64), ("total_clock_ns", C.c_uint64), ("kernel_ms", C.c_double), ("wall_s", C.c_double),
    ]


CAMPAIGN_STOP_AT_FAILURE = 1
CAMPAIGN_LIST_RUNNER = 2      # collecting campaigns: list runner verdicts too
CAMPAIGN_STOP_AT_CAP = 4      # collecting campaigns: stop launching once `cap` listed seeds have been read


class Failure(C.Structure):
    """madsim_failure_t: one record of a collecting campaign's list — the seed and its 48 result bytes."""
    _fields_ = [("seed", C.c_uint64), ("result", Result)]


class Collect(C.Structure):
    """madsim_collect_t: the caller's record array going in, the list length and the verdict histogram coming out."""
    _fields_ = [("failures", C.POINTER(Failure)), ("cap", C.c_uint64), ("n_listed", C.c_uint64), ("n_by_verdict", C.c_uint64 * 8)]


STAT_CLOCK, STAT_STEPS, STAT_MSGS, STAT_RNG = range(4)      # the metrics of a statistics campaign, in madsim_stats_t.metric order
STAT_METRICS, STAT_BUCKETS, STAT_MAX_TOP = 4, 256, 16
STAT_NAMES = ("clock_ns", "steps", "msg_count", "rng_calls")


class Extreme(C.Structure):
    """madsim_extreme_t: one of a metric's extreme seeds."""
    _fields_ = [("value", C.c_uint64), ("seed", C.c_uint64)]


class Metric(C.Structure):
    """madsim_metric_t: one metric over the counted seeds — min, max, the 128-bit sum, the bucket counts."""
    _fields_ = [("min", C.c_uint64), ("max", C.c_uint64), ("sum_lo", C.c_uint64), ("sum_hi", C.c_uint64), ("hist", C.c_uint64 * STAT_BUCKETS)]


class Stats(C.Structure):
    """madsim_stats_t: which verdicts to count and the caller's top array going in, the statistics coming out."""
    _fields_ = [("include", C.c_uint32), ("top_k", C.c_uint32), ("top", C.POINTER(Extreme)), ("n", C.c_uint64), ("n_top", C.c_uint64),
                ("metric", Metric * STAT_METRICS)]


def stat_bucket(v):
    """madsim_hip_stat_bucket: v itself below 4, else four buckets per octave — the top set bit and the two bits after it."""
    if v < 4:
        return v
    e = v.bit_length() - 1
    return 4 * (e - 1) + ((v >> (e - 2)) & 3)


def stat_bucket_floor(b):
    """madsim_hip_stat_bucket_floor: the smallest value of bucket b (2^64 - 1 from 252 on: no such bucket)."""
    if b < 4:
        return b
    return U64_MAX if b >= 252 else (4 + b % 4) << (b // 4 - 1)


CAMPAIGN_STOP_AT_GROUPS = 8   # grouping campaigns: stop launching once `cap` groups have been read
GROUP_KEY_OBS, GROUP_KEY_TRACE, GROUP_KEY_MSGS, GROUP_KEY_CLOCK, GROUP_KEY_RNG, GROUP_KEY_STEPS = range(6)      # madsim_groups_t.key_field
GROUP_KEYS = 6
GROUP_KEY_NAMES = ("obs", "trace", "msgs", "clock", "rng", "steps")      # the `key=` names of runtime.run_campaign_groups, by key_field
GROUP_KEY_FIELDS = ("obs_hash", "trace_hash", "msg_count", "clock_ns", "rng_calls", "steps")      # ... and the result field each one groups by
GROUP_MAX_BATCH = 1 << 20


class Group(C.Structure):
    """madsim_group_t: one failure mode — the signature (verdict, key), how many counted seeds carry it, the smallest of them."""
    _fields_ = [("key", C.c_uint64), ("verdict", C.c_uint32), ("reserved", C.c_uint32), ("count", C.c_uint64), ("first_seed", C.c_uint64)]


class Groups(C.Structure):
    """madsim_groups_t: which verdicts to group by which field and the caller's array going in, the groups and the two totals coming out."""
    _fields_ = [("include", C.c_uint32), ("key_field", C.c_uint32), ("groups", C.POINTER(Group)), ("cap", C.c_uint64), ("n_groups", C.c_uint64),
                ("n_grouped", C.c_uint64), ("n_ungrouped", C.c_uint64)]


# numpy view of a grouping campaign's list: madsim_group_t
GROUP_DTYPE = [("key", "<u8"), ("verdict", "<u4"), ("reserved", "<u4"), ("count", "<u8"), ("first_seed", "<u8")]
assert C.sizeof(Group) == 32 and C.sizeof(Groups) == 48
HEADER_STRUCTS["madsim_group_t"] = Group
HEADER_STRUCTS["madsim_groups_t"] = Groups


CAMPAIGN_STOP_AT_DIFFS = 16   # differential campaigns: stop launching once `cap` differing seeds have been read
DIFF_VERDICT, DIFF_STEPS, DIFF_CLOCK, DIFF_MSGS, DIFF_RNG, DIFF_TRACE, DIFF_OBS = (1 << i for i in range(7))      # madsim_diff_t.fields
DIFF_ALL = 127
DIFF_FIELDS = 7
DIFF_FIELD_NAMES = ("verdict", "steps", "clock_ns", "msg_count", "rng_calls", "trace_hash", "obs_hash")      # the result field behind bit i


class DiffRecord(C.Structure):
    """madsim_diff_record_t: one differing seed of a differential campaign — the seed and its 48 result bytes on each side."""
    _fields_ = [("seed", C.c_uint64), ("a", Result), ("b", Result)]


class Diff(C.Structure):
    """madsim_diff_t: the compared fields and the caller's record array going in; the list length, the counts and the 8 x 8 matrix of
    verdict transitions coming out.  (Like madsim_failure_t and madsim_stats_t it is declared in two statements in the header, so it is
    not in HEADER_STRUCTS: tests/test_campaign_diff.py holds it against the header.)"""
    _fields_ = [("fields", C.c_uint32), ("reserved", C.c_uint32), ("records", C.POINTER(DiffRecord)), ("cap", C.c_uint64), ("n_listed", C.c_uint64),
                ("n_compared", C.c_uint64), ("n_incomparable", C.c_uint64), ("n_differ", C.c_uint64), ("n_by_field", C.c_uint64 * 8),
                ("transitions", C.c_uint64 * 8 * 8)]


assert C.sizeof(DiffRecord) == 104 and C.sizeof(Diff) == 632


CAMPAIGN_STOP_AT_SWEEP = 64   # sweep campaigns: stop launching once `cap` selected seeds have been read
SWEEP_MAX_VARIANTS = 8
SWEEP_LIST_MIXED, SWEEP_LIST_FAILING, SWEEP_LIST_DIFFERING = range(3)      # madsim_sweep_t.list_rule
SWEEP_LIST_NAMES = ("mixed", "failing", "differing")      # the `list_rule=` names of runtime.run_campaign_sweep, by list_rule


class SweepVariant(C.Structure):
    """madsim_sweep_variant_t: one variant of a sweep campaign going in — workload, config, limits (NULL = defaults) — and where its plain
    campaign report goes."""
    _fields_ = [("w", C.POINTER(Workload)), ("cfg", C.POINTER(Config)), ("lim", C.POINTER(Limits)), ("out", C.POINTER(Campaign))]


class SweepRecord(C.Structure):
    """madsim_sweep_record_t: one listed seed of a sweep campaign — the seed, the variants it fails in, the variants whose masked fields differ
    from variant 0's, and every variant's verdict."""
    _fields_ = [("seed", C.c_uint64), ("fail_mask", C.c_uint32), ("differ_mask", C.c_uint32), ("verdict", C.c_uint8 * 8)]


class Sweep(C.Structure):
    """madsim_sweep_t: the compared fields, the list rule and the caller's record array going in; the list length and the counts coming out."""
    _fields_ = [("fields", C.c_uint32), ("list_rule", C.c_uint32), ("records", C.POINTER(SweepRecord)), ("cap", C.c_uint64), ("n_listed", C.c_uint64),
                ("n_selected", C.c_uint64), ("n_settled", C.c_uint64), ("n_incomparable", C.c_uint64), ("n_runner_by_variant", C.c_uint64 * 8),
                ("n_differ_from_first", C.c_uint64 * 8), ("n_by_mask", C.c_uint64 * 256)]


# numpy view of a sweep campaign's list: madsim_sweep_record_t
SWEEP_RECORD_DTYPE = [("seed", "<u8"), ("fail_mask", "<u4"), ("differ_mask", "<u4"), ("verdict", "u1", (8,))]
assert C.sizeof(SweepVariant) == 32 and C.sizeof(SweepRecord) == 24 and C.sizeof(Sweep) == 2232
HEADER_STRUCTS["madsim_sweep_variant_t"] = SweepVariant
HEADER_STRUCTS["madsim_sweep_record_t"] = SweepRecord
HEADER_STRUCTS["madsim_sweep_t"] = Sweep


CAMPAIGN_RESOLVE = 32         # every campaign form: re-run runner verdicts on the device before a batch is reported
CAMPAIGN_RESOLVE_ROUNDS_SHIFT, CAMPAIGN_RESOLVE_ROUNDS_MASK = 8, 0xF00      # flag bits 8-11: the number of rounds, 0 = the default
RESOLVE_DEFAULT_ROUNDS, RESOLVE_MAX_ROUNDS = 4, 8


class Resolve(C.Structure):
    """madsim_resolve_t: what the resolve rounds of the most recent campaign call did (madsim_hip_campaign_resolved)."""
    _fields_ = [("n_first_pass", C.c_uint64), ("n_resolved", C.c_uint64), ("n_unresolved", C.c_uint64), ("n_by_round", C.c_uint64 * 8),
                ("batches_resolved", C.c_uint64), ("rounds", C.c_uint32), ("reserved", C.c_uint32), ("rerun_kernel_ms", C.c_double)]


assert C.sizeof(Resolve) == 112
HEADER_STRUCTS["madsim_resolve_t"] = Resolve

TRACE_MAX_BYTES = 1 << 30     # madsim_hip_trace_seeds: device memory one call may ask for, n * (log_cap + 8 * obs_cap + 72)
FNV_OFFSET, FNV_PRIME = 0xCBF29CE484222325, 0x100000001B3      # obs_hash / trace_hash: 64-bit FNV-1a over whole values

# madsim_hip_diverge_seeds: the status of a channel (determinism log / observations) of one seed's two runs
DIVERGE_SAME, DIVERGE_DIFFER, DIVERGE_PREFIX, DIVERGE_BEYOND_CAP, DIVERGE_INCOMPARABLE = range(5)
DIVERGE_NAMES = ("same", "differ", "prefix", "beyond-cap", "incomparable")
DIVERGE_MAX_WIN = 8


class Divergence(C.Structure):
    """madsim_divergence_t: where the two runs of one seed part, on both channels (declared in two statements in the header, as
    madsim_diff_record_t: tests/test_diverge.py holds it against the header)."""
    _fields_ = [("seed", C.c_uint64), ("log_status", C.c_uint32), ("obs_status", C.c_uint32), ("log_at", C.c_uint64), ("obs_at", C.c_uint64),
                ("log_len_a", C.c_uint64), ("log_len_b", C.c_uint64), ("obs_len_a", C.c_uint64), ("obs_len_b", C.c_uint64),
                ("obs_a", C.c_uint64), ("obs_b", C.c_uint64), ("log_a", C.c_uint8), ("log_b", C.c_uint8), ("pad", C.c_uint8 * 6),
                ("a", Result), ("b", Result)]


assert C.sizeof(Divergence) == 184

CENSUS_MAX_VALUES, CENSUS_MAX_OBS_CAP = 1 << 20, 1024      # madsim_hip_census_range / _seeds: the most distinct values, the most visible observations


class CensusValue(C.Structure):
    """madsim_census_value_t: one observed value — the counted seeds of each verdict that observed it at least once, its occurrences over
    them, the smallest such seed and the most occurrences inside one seed."""
    _fields_ = [("value", C.c_uint64), ("n_seeds", C.c_uint64 * 4), ("n_total", C.c_uint64), ("first_seed", C.c_uint64), ("max_per_seed", C.c_uint64)]


class Census(C.Structure):
    """madsim_census_t: which verdicts count, how many observations of a seed are visible and the caller's two arrays going in; the table's
    length and the totals coming out."""
    _fields_ = [("include", C.c_uint32), ("obs_cap", C.c_uint32), ("values", C.POINTER(CensusValue)), ("cap", C.c_uint64),
                ("runner_seeds", C.POINTER(C.c_uint64)), ("runner_cap", C.c_uint64), ("n_values", C.c_uint64), ("n_counted", C.c_uint64 * 4),
                ("n_silent", C.c_uint64 * 4), ("n_truncated", C.c_uint64), ("n_observations", C.c_uint64), ("n_runner", C.c_uint64),
                ("n_runner_listed", C.c_uint64)]


# numpy view of a census table: madsim_census_value_t
CENSUS_VALUE_DTYPE = [("value", "<u8"), ("n_seeds", "<u8", (4,)), ("n_total", "<u8"), ("first_seed", "<u8"), ("max_per_seed", "<u8")]
assert C.sizeof(CensusValue) == 64 and C.sizeof(Census) == 144
HEADER_STRUCTS["madsim_census_value_t"] = CensusValue
HEADER_STRUCTS["madsim_census_t"] = Census

# madsim_hip_probe_sets_range / _seeds: the most vocabulary values, the most distinct sets, and the two set-word bits beside the vocabulary's
PROBE_SETS_MAX_VOCAB, PROBE_SETS_MAX = 62, 1 << 20
PROBE_SET_OTHER, PROBE_SET_TRUNCATED = 1 << 62, 1 << 63


class ProbeSet(C.Structure):
    """madsim_probe_set_t: one distinct set word — the counted seeds of each verdict with exactly this set and the smallest of them."""
    _fields_ = [("set", C.c_uint64), ("n_seeds", C.c_uint64 * 4), ("first_seed", C.c_uint64 * 4)]


class ProbeSets(C.Structure):
    """madsim_probe_sets_t: which verdicts count, how many observations of a seed are visible, the vocabulary and the caller's two arrays
    going in; the table's length and the totals coming out."""
    _fields_ = [("include", C.c_uint32), ("obs_cap", C.c_uint32), ("vocab", C.POINTER(C.c_uint64)), ("n_vocab", C.c_uint64),
                ("sets", C.POINTER(ProbeSet)), ("cap", C.c_uint64), ("runner_seeds", C.POINTER(C.c_uint64)), ("runner_cap", C.c_uint64),
                ("n_sets", C.c_uint64), ("n_counted", C.c_uint64 * 4), ("n_runner", C.c_uint64), ("n_runner_listed", C.c_uint64)]


# numpy view of a probe-set table: madsim_probe_set_t
PROBE_SET_DTYPE = [("set", "<u8"), ("n_seeds", "<u8", (4,)), ("first_seed", "<u8", (4,))]
assert C.sizeof(ProbeSet) == 72 and C.sizeof(ProbeSets) == 112
HEADER_STRUCTS["madsim_probe_set_t"] = ProbeSet
HEADER_STRUCTS["madsim_probe_sets_t"] = ProbeSets

# madsim_hip_probe_order_range / _seeds: the most vocabulary values (the device's matrix is 32 x 32 cells per verdict)
PROBE_ORDER_MAX_VOCAB = 32


class ProbeOrderPair(C.Structure):
    """madsim_probe_order_pair_t: one cell (a, b) of vocabulary indices — a == b: the counted seeds of each verdict that reached value a;
    a != b: those in which a's first occurrence comes before b's — and the smallest such seed of each verdict."""
    _fields_ = [("a", C.c_uint32), ("b", C.c_uint32), ("n_seeds", C.c_uint64 * 4), ("first_seed", C.c_uint64 * 4)]


class ProbeOrder(C.Structure):
    """madsim_probe_order_t: which verdicts count, how many observations of a seed are visible, the vocabulary and the caller's two arrays
    going in; the number of entries and the totals coming out."""
    _fields_ = [("include", C.c_uint32), ("obs_cap", C.c_uint32), ("vocab", C.POINTER(C.c_uint64)), ("n_vocab", C.c_uint64),
                ("pairs", C.POINTER(ProbeOrderPair)), ("cap", C.c_uint64), ("runner_seeds", C.POINTER(C.c_uint64)), ("runner_cap", C.c_uint64),
                ("n_pairs", C.c_uint64), ("n_counted", C.c_uint64 * 4), ("n_none", C.c_uint64 * 4), ("n_truncated", C.c_uint64),
                ("n_runner", C.c_uint64), ("n_runner_listed", C.c_uint64)]


# numpy view of a probe-order table: madsim_probe_order_pair_t
PROBE_ORDER_PAIR_DTYPE = [("a", "<u4"), ("b", "<u4"), ("n_seeds", "<u8", (4,)), ("first_seed", "<u8", (4,))]
assert C.sizeof(ProbeOrderPair) == 72 and C.sizeof(ProbeOrder) == 152
HEADER_STRUCTS["madsim_probe_order_pair_t"] = ProbeOrderPair
HEADER_STRUCTS["madsim_probe_order_t"] = ProbeOrder

# madsim_hip_probe_spans_range / _seeds: the most span definitions of one call, the one flag, the states of a (seed, span)
PROBE_SPANS_MAX = 16
SPAN_FROM_START = 1
SPAN_ABSENT, SPAN_CLOSED, SPAN_OPEN, SPAN_CUT = 0, 1, 2, 3
SPAN_STATE_NAMES = {SPAN_ABSENT: "ABSENT", SPAN_CLOSED: "CLOSED", SPAN_OPEN: "OPEN", SPAN_CUT: "CUT"}


class SpanDef(C.Structure):
    """madsim_span_def_t: from the first `from` (flags = SPAN_FROM_START: from the start of the run) to the first `to` behind it.  (`from` is
    a Python keyword: getattr(d, "from"), or the numpy view SPAN_DEF_DTYPE.)"""
    _fields_ = [("from", C.c_uint64), ("to", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class Span(C.Structure):
    """madsim_span_t: the counted seeds per verdict and state, and over the CLOSED ones the distribution of the durations with the seeds
    that attain its extremes; the smallest OPEN seed."""
    _fields_ = [("n_state", C.c_uint64 * 16), ("n", C.c_uint64), ("min", C.c_uint64), ("max", C.c_uint64), ("sum_lo", C.c_uint64),
                ("sum_hi", C.c_uint64), ("min_seed", C.c_uint64), ("max_seed", C.c_uint64), ("first_open_seed", C.c_uint64),
                ("hist", C.c_uint64 * STAT_BUCKETS)]


class ProbeSpans(C.Structure):
    """madsim_probe_spans_t: which verdicts count, how many observations of a seed are visible, the definitions and the caller's two arrays
    going in; the totals coming out."""
    _fields_ = [("include", C.c_uint32), ("obs_cap", C.c_uint32), ("defs", C.POINTER(SpanDef)), ("n_spans", C.c_uint64), ("spans", C.POINTER(Span)),
                ("runner_seeds", C.POINTER(C.c_uint64)), ("runner_cap", C.c_uint64), ("n_counted", C.c_uint64 * 4), ("n_truncated", C.c_uint64),
                ("n_runner", C.c_uint64), ("n_runner_listed", C.c_uint64)]


# numpy views: madsim_span_def_t, madsim_span_t (n_state[4 * verdict + state] seen as [verdict][state]); SPAN_REC_WORDS: the 64-bit words of a record, on the device and on the host
SPAN_DEF_DTYPE = [("from", "<u8"), ("to", "<u8"), ("flags", "<u4"), ("reserved", "<u4")]
SPAN_DTYPE = [("n_state", "<u8", (4, 4)), ("n", "<u8"), ("min", "<u8"), ("max", "<u8"), ("sum_lo", "<u8"), ("sum_hi", "<u8"), ("min_seed", "<u8"),
              ("max_seed", "<u8"), ("first_open_seed", "<u8"), ("hist", "<u8", (STAT_BUCKETS,))]
SPAN_REC_WORDS = 280
assert C.sizeof(SpanDef) == 24 and C.sizeof(Span) == 2240 == 8 * SPAN_REC_WORDS and C.sizeof(ProbeSpans) == 104
HEADER_STRUCTS["madsim_span_def_t"] = SpanDef
HEADER_STRUCTS["madsim_span_t"] = Span
HEADER_STRUCTS["madsim_probe_spans_t"] = ProbeSpans

# madsim_hip_task_states: the state byte of a task record (bits 63-56; prog 55-48, pc 47-32, cnt0 31-16, cnt1 15-0)
TASK_PARKED, TASK_QUEUED, TASK_PANICKED, TASK_CANCELLED = 1, 2, 3, 4
TASK_STATE_NAMES = {TASK_PARKED: "PARKED", TASK_QUEUED: "QUEUED", TASK_PANICKED: "PANICKED", TASK_CANCELLED: "CANCELLED"}
MAX_LIVE_TASKS = 254          # the most task records a row can hold (madsim_limits_t.max_tasks' ceiling)


class StallCensus(C.Structure):
    """madsim_stall_census_t: which verdicts count, how many live tasks of a seed are visible and the caller's three arrays going in (the
    site table, the shape table — NULL with 0: no shapes pass —, the runner seeds); the tables' lengths and the totals coming out."""
    _fields_ = [("include", C.c_uint32), ("task_cap", C.c_uint32), ("sites", C.POINTER(CensusValue)), ("site_cap", C.c_uint64),
                ("shapes", C.POINTER(CensusValue)), ("shape_cap", C.c_uint64), ("runner_seeds", C.POINTER(C.c_uint64)), ("runner_cap", C.c_uint64),
                ("n_sites", C.c_uint64), ("n_shapes", C.c_uint64), ("n_counted", C.c_uint64 * 4), ("n_idle", C.c_uint64 * 4),
                ("n_truncated", C.c_uint64), ("n_tasks", C.c_uint64), ("n_runner", C.c_uint64), ("n_runner_listed", C.c_uint64)]


assert C.sizeof(StallCensus) == 168
HEADER_STRUCTS["madsim_stall_census_t"] = StallCensus


class Geometry(C.Structure):
    _fields_ = [
        ("lds_bytes_per_seed", C.c_uint32), ("lds_bytes_per_block", C.c_uint32), ("block_threads", C.c_uint32),
        ("blocks_per_cu", C.c_uint32), ("grid_blocks", C.c_uint32), ("heap_lds_slots", C.c_uint32),
        ("heap_spill_slots", C.c_uint32), ("max_tasks", C.c_uint32), ("lanes_per_wave", C.c_uint32),
        ("variant", C.c_uint32), ("global_bytes_per_seed", C.c_uint32),
    ]


VARIANT_SCOPE = 1 << 20     # madsim_geometry_t.variant: timeout scopes (MS_OP_TIMEOUT_BEGIN / END) compiled in
VARIANT_TICK = 1 << 21      # madsim_geometry_t.variant: interval tickers (MS_OP_INTERVAL / TICK / INTERVAL_RESET) compiled in
VARIANT_SELECT = 1 << 22    # madsim_geometry_t.variant: selects over a receive and a tick, timeout_at (MS_OP_RECV_OR_TICK / RECV_TIMEOUT_AT) compiled in
VARIANT_SIGNAL = 1 << 23    # madsim_geometry_t.variant: ctrl-c signals (MS_OP_CTRL_C / SEND_CTRL_C / RECV_OR_CTRL_C) compiled in
VARIANT_TIER_FEAT = ((VARIANT_SCOPE, 256), (VARIANT_TICK, 512), (VARIANT_SELECT, 1024), (VARIANT_SIGNAL, 2048))   # report bit -> MADSIM_FEAT_SCOPE / TICK / SELECT / SIGNAL


HEADER_STRUCTS["madsim_campaign_t"] = Campaign
HEADER_STRUCTS["madsim_collect_t"] = Collect
HEADER_STRUCTS["madsim_extreme_t"] = Extreme
HEADER_STRUCTS["madsim_metric_t"] = Metric
assert C.sizeof(Insn) == 8 and C.sizeof(Prog) == 4 and C.sizeof(Sock) == 4 and C.sizeof(Node) == 4
assert C.sizeof(Result) == 48 and C.sizeof(Summary) == 48 and C.sizeof(Limits) == 64 and C.sizeof(Config) == 136

# numpy view of a result array: one record per seed, same layout as madsim_result_t
RESULT_DTYPE = [("verdict", "<u4"), ("steps", "<u4"), ("clock_ns", "<u8"), ("msg_count", "<u8"),
                ("rng_calls", "<u8"), ("trace_hash", "<u8"), ("obs_hash", "<u8")]
# numpy view of a collecting campaign's list: madsim_failure_t, the seed in front of the result's fields
FAILURE_DTYPE = [("seed", "<u8")] + RESULT_DTYPE
assert C.sizeof(Failure) == 56 and C.sizeof(Collect) == 88
# numpy view of a differential campaign's list: madsim_diff_record_t, the seed, then side A's result and side B's
DIFF_RECORD_DTYPE = [("seed", "<u8"), ("a", RESULT_DTYPE), ("b", RESULT_DTYPE)]
# numpy view of madsim_hip_diverge_seeds' records: madsim_divergence_t
DIVERGENCE_DTYPE = [("seed", "<u8"), ("log_status", "<u4"), ("obs_status", "<u4"), ("log_at", "<u8"), ("obs_at", "<u8"), ("log_len_a", "<u8"),
                    ("log_len_b", "<u8"), ("obs_len_a", "<u8"), ("obs_len_b", "<u8"), ("obs_a", "<u8"), ("obs_b", "<u8"), ("log_a", "u1"),
                    ("log_b", "u1"), ("pad", "u1", (6,)), ("a", RESULT_DTYPE), ("b", RESULT_DTYPE)]
# numpy view of a statistics campaign's extreme seeds: madsim_extreme_t
EXTREME_DTYPE = [("value", "<u8"), ("seed", "<u8")]
assert C.sizeof(Extreme) == 16 and C.sizeof(Metric) == 2080 and C.sizeof(Stats) == 32 + 4 * 2080

PAIRED_UP, PAIRED_DOWN = 0, 1      # the direction of a paired campaign's delta: side B's value above / below side A's
PAIRED_DIRECTION_NAMES = ("up", "down")


class PairedExtreme(C.Structure):
    """madsim_paired_extreme_t: one of the extreme seeds of a (metric, direction) — the seed and both sides' values of that metric."""
    _fields_ = [("seed", C.c_uint64), ("a", C.c_uint64), ("b", C.c_uint64)]


class Paired(C.Structure):
    """madsim_paired_t: which verdicts pair on each side and the caller's top array going in; the classification counts and, at index
    2 * metric + direction, the seeds that moved that way with the minimum, maximum, 128-bit sum and bucket counts of the magnitudes coming
    out.  (Declared in two statements in the header, as madsim_stats_t: tests/test_campaign_paired.py holds it against the header.)"""
    _fields_ = [("include_a", C.c_uint32), ("include_b", C.c_uint32), ("top_k", C.c_uint32), ("reserved", C.c_uint32), ("top", C.POINTER(PairedExtreme)),
                ("n_paired", C.c_uint64), ("n_unpaired", C.c_uint64), ("n_incomparable", C.c_uint64), ("n_top", C.c_uint64 * 8), ("n", C.c_uint64 * 8),
                ("n_equal", C.c_uint64 * 4), ("sum_a_lo", C.c_uint64 * 4), ("sum_a_hi", C.c_uint64 * 4), ("sum_b_lo", C.c_uint64 * 4),
                ("sum_b_hi", C.c_uint64 * 4), ("delta", Metric * 8)]


# numpy view of a paired campaign's extreme seeds: madsim_paired_extreme_t
PAIRED_EXTREME_DTYPE = [("seed", "<u8"), ("a", "<u8"), ("b", "<u8")]
assert C.sizeof(PairedExtreme) == 24 and C.sizeof(Paired) == 336 + 8 * 2080
HEADER_STRUCTS["madsim_paired_extreme_t"] = PairedExtreme

PASS, PANIC, DEADLOCK, TIME_LIMIT, OVERFLOW, STEP_LIMIT, UNSUPPORTED, INTERNAL = range(8)
VERDICT_NAMES = ["pass", "panic", "deadlock", "time-limit", "resource-overflow", "step-limit", "outside-the-workload-model", "internal-invariant"]


def is_runner_verdict(v):
    """MADSIM_IS_RUNNER_VERDICT: a statement about this runner (capacity, step cap, model frontier, internal), never a test failure."""
    return v >= OVERFLOW

# enum madsim_op
OP = dict(
    DONE=0, SPAWN=1, JOIN=2, ABORT=3, YIELD=4, PANIC=5, SET=6, DJNZ=7, JMP=8, TRACE=9,
    SLEEP=10, MARK=11, SLEEP_UNTIL=12, ASSERT_ELAPSED=13, ADVANCE=14, BUILD=15,
    BIND=20, SEND=21, REPLY=22, RECV=23, ASSERT_VAL=24, RECV_TIMEOUT=25, CLOSE=26,
    KILL=30, RESTART=31, PAUSE=32, RESUME=33, CLOG_NODE=34, UNCLOG_NODE=35, CLOG_LINK=36,
    UNCLOG_LINK=37, ASSERT_EXIT=38, SET_LOSS=39, SLEEP_RAND=40, GSET=41, GADD=42, ASSERT_G=43, PANIC_IF_G_LT=44, JEQ=45, CONNECT=46, ACCEPT=47, CSEND=48, CRECV=49, CCLOSE=50, RPC_CALL=51, RPC_REPLY=52, RAND_BOOL=53, RANDOM=54, TRACE_TIME=55, HOOK_REQ=56, HOOK_RSP=57, IPVS=58, SET_LATENCY=59,
    TIMEOUT_BEGIN=60, TIMEOUT_END=61, INTERVAL=62, TICK=63, INTERVAL_RESET=64, RECV_OR_TICK=65, RECV_TIMEOUT_AT=66,
    CTRL_C=67, SEND_CTRL_C=68, RECV_OR_CTRL_C=69,
)
PROG_INIT, PROG_PRE, PROG_DROP_SPAWN = 1, 2, 4
NODE_RESTART_ON_PANIC = 1
NODE_RESTART_MATCHING = 4
