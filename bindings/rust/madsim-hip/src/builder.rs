//! `Builder`: madsim's seed driver (`madsim::runtime::Builder`, runtime/builder.rs:7-162) over the GPU batch runner.
//!
//! Same public fields, same `MADSIM_TEST_*` environment variables, same outcome: `run_workload` returns when every seed
//! passes and otherwise prints the reference's reproduction note (runtime/mod.rs:205-210) for the failing seed and panics —
//! so `cargo test` verdicts are those of `Builder::run`.  One documented difference: with `jobs > 1` the reference reports
//! the first failing seed to *complete*; a batch has no completion order, so the numerically smallest failing seed is reported.
use crate::workload::Workload;
use madsim_hip_sys as sys;
use std::ffi::CStr;
use std::os::raw::c_int;
use std::sync::OnceLock;
use std::time::{Duration, SystemTime};

/// `madsim::Config.net` (net/network.rs:66-89) + the buggify switch.
#[derive(Clone, Debug)]
pub struct NetConfig {
    pub packet_loss_rate: f64,
    pub send_latency: std::ops::Range<Duration>,
    pub buggify: bool,
    /// Ranges a workload's `set_latency(i)` switches to: `NetSim::update_config(|c| c.send_latency = latency_table[i])`
    /// (`net/mod.rs:138-141`); at most four.
    pub latency_table: Vec<std::ops::Range<Duration>>,
}

impl Default for NetConfig {
    fn default() -> Self {
        NetConfig { packet_loss_rate: 0.0, send_latency: Duration::from_millis(1)..Duration::from_millis(10), buggify: false, latency_table: Vec::new() }
    }
}

impl NetConfig {
    pub fn raw(&self) -> sys::madsim_config_t {
        assert!(self.latency_table.len() <= 4, "at most four latency_table entries");
        let (mut lo, mut hi) = ([0u64; 4], [0u64; 4]);
        for (i, r) in self.latency_table.iter().enumerate() { lo[i] = r.start.as_nanos() as u64; hi[i] = r.end.as_nanos() as u64; }
        sys::madsim_config_t {
            packet_loss_rate: self.packet_loss_rate,
            lat_lo_ns: self.send_latency.start.as_nanos() as u64,
            lat_hi_ns: self.send_latency.end.as_nanos() as u64,
            buggify: self.buggify as u32,
            n_loss_table: 0,
            loss_table: [0.0; 4],
            n_lat_table: self.latency_table.len() as u32,
            reserved0: 0,
            lat_table_lo_ns: lo,
            lat_table_hi_ns: hi,
        }
    }
}

/// A library error (never a test verdict): no GPU, malformed workload, limits that do not fit the device, a runner limit
/// (device capacity / step cap) that persists after the re-runs.
#[derive(Debug)]
pub struct RunError {
    pub code: c_int,
    pub message: String,
}

impl std::fmt::Display for RunError {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "madsim_hip error {}: {}", self.code, self.message)
    }
}
impl std::error::Error for RunError {}

fn last_error(code: c_int) -> RunError {
    let (what, detail) = unsafe {
        (CStr::from_ptr(sys::madsim_hip_strerror(code)).to_string_lossy().into_owned(),
         CStr::from_ptr(sys::madsim_hip_last_error()).to_string_lossy().into_owned())
    };
    RunError { code, message: format!("{what}: {detail}") }
}

struct Contexts(Vec<*mut sys::madsim_hip_ctx_t>);
// the library serialises calls per context; the pointers are only handed back to it
unsafe impl Send for Contexts {}
unsafe impl Sync for Contexts {}

/// One context per visible GPU, created once per process (MADSIM_HIP_DEVICES = how many to use; default: all).
fn contexts() -> Result<&'static Contexts, RunError> {
    static CTX: OnceLock<Result<Contexts, (c_int, String)>> = OnceLock::new();
    let r = CTX.get_or_init(|| {
        let want: usize = std::env::var("MADSIM_HIP_DEVICES").ok().and_then(|s| s.parse().ok()).unwrap_or(usize::MAX);
        let mut v = Vec::new();
        while v.len() < want {
            let mut c: *mut sys::madsim_hip_ctx_t = std::ptr::null_mut();
            let rc = unsafe { sys::madsim_hip_ctx_create(v.len() as c_int, &mut c) };
            if rc != 0 {
                if v.is_empty() {
                    let e = last_error(rc);
                    return Err((e.code, e.message));
                }
                break; // device index past the last GPU
            }
            v.push(c);
        }
        Ok(Contexts(v))
    });
    match r {
        Ok(c) => Ok(c),
        Err((code, message)) => Err(RunError { code: *code, message: message.clone() }),
    }
}

/// What the panic of a failing seed says (the reference's messages: task/mod.rs:250,253-258).
pub fn verdict_message(verdict: u32) -> &'static str {
    match verdict {
        sys::MADSIM_PANIC => "a task panicked",
        sys::MADSIM_DEADLOCK => "no events, all tasks will block forever",
        sys::MADSIM_TIME_LIMIT => "time limit exceeded",
        sys::MADSIM_OVERFLOW => "device capacity exceeded (runner limit, not a test verdict)",
        sys::MADSIM_STEP_LIMIT => "step cap reached (runner limit, not a test verdict)",
        sys::MADSIM_UNSUPPORTED => "the seed left the workload model (runner verdict, not a test verdict)",
        sys::MADSIM_INTERNAL => "internal invariant of the device code broke (runner verdict, not a test verdict)",
        _ => "pass",
    }
}

/// runtime/mod.rs:205-210
fn note_seed(seed: u64) {
    eprintln!("note: run with `MADSIM_TEST_SEED={seed}` environment variable to reproduce this error");
}

/// Builds the many-seed run with custom configuration values (the fields of `madsim::runtime::Builder`).
pub struct Builder {
    /// The random seed for test.
    pub seed: u64,
    /// The number of tests.
    pub count: u64,
    /// The number of jobs to run simultaneously (no meaning for a batch: every seed is in flight).
    pub jobs: u16,
    /// The configuration.
    pub config: NetConfig,
    /// The time limit for the test.
    pub time_limit: Option<Duration>,
    /// Enable determinism check.
    pub check: bool,
    /// Allow spawning system thread (accepted, no effect: a GPU lane has no system threads).
    pub allow_system_thread: bool,
    /// Device capacities to start from (no reference counterpart; all zero = defaults).  `limits.no_trace_hash = 1` drops the
    /// determinism-log fingerprint from the results (the reference logs only under `check`, rand.rs:67): 4 % faster on ping-pong.
    pub limits: sys::madsim_limits_t,
    /// `MADSIM_CAMPAIGN_RESOLVE` and its rounds bits, set by `resolve_runner` (0 = runner verdicts are counted apart).
    pub resolve_flags: u32,
}

fn zero_limits() -> sys::madsim_limits_t {
    // plain-old-data: all zero = "pick defaults"
    unsafe { std::mem::zeroed() }
}

/// What `Builder::search_failures` found: the failing seeds (ascending, at most as many as asked for), the seeds per verdict
/// value over the whole range, and the campaign report.
#[derive(Clone, Debug)]
pub struct Failures {
    pub failures: Vec<sys::madsim_failure_t>,
    pub by_verdict: [u64; 8],
    pub campaign: sys::madsim_campaign_t,
}

/// What `Builder::campaign_stats` found over the counted seeds: `stats.n`, per metric (`MADSIM_STAT_CLOCK` ..) min, max, the
/// 128-bit sum and the bucket counts, and `top[m]`: the extreme seeds of metric `m`, value descending, then seed ascending.
#[derive(Clone, Debug)]
pub struct Stats {
    pub stats: sys::madsim_stats_t,
    pub top: [Vec<sys::madsim_extreme_t>; 4],
    pub campaign: sys::madsim_campaign_t,
}

/// What `Builder::failure_groups` found: the failure modes in order of first appearance (ascending `first_seed`), the counted seeds
/// they hold, the counted seeds of the modes that did not make the list, and the campaign report.
#[derive(Clone, Debug)]
pub struct Groups {
    pub groups: Vec<sys::madsim_group_t>,
    pub n_grouped: u64,
    pub n_ungrouped: u64,
    pub campaign: sys::madsim_campaign_t,
}

/// What `Builder::diff_campaign` found: the smallest differing seeds with both sides' results (ascending), the report — counts and
/// the 8 x 8 matrix `transitions[verdict A][verdict B]` — and each side's plain campaign report.
#[derive(Clone, Debug)]
pub struct Diff {
    pub records: Vec<sys::madsim_diff_record_t>,
    pub report: sys::madsim_diff_t,
    pub a: sys::madsim_campaign_t,
    pub b: sys::madsim_campaign_t,
}

/// What `Builder::paired_campaign` found over the paired seeds (both verdicts named by their side's include mask): the report — at index
/// `2 * metric + direction` (`MADSIM_STAT_*`, `MADSIM_PAIRED_UP` / `_DOWN`) the seeds that moved that way with the minimum, maximum,
/// 128-bit sum and bucket counts of the magnitudes —, `top[2 * metric + direction]`: the extreme seeds with both sides' values, magnitude
/// descending, then seed ascending, and each side's plain campaign report.
#[derive(Clone, Debug)]
pub struct Paired {
    pub report: sys::madsim_paired_t,
    pub top: [Vec<sys::madsim_paired_extreme_t>; 8],
    pub a: sys::madsim_campaign_t,
    pub b: sys::madsim_campaign_t,
}

impl Paired {
    /// Sum over the paired seeds of `b - a` for `metric`: the UP magnitudes minus the DOWN magnitudes.
    pub fn net_sum(&self, metric: usize) -> i128 {
        let sum = |j: usize| ((self.report.delta[j].sum_hi as u128) << 64 | self.report.delta[j].sum_lo as u128) as i128;
        sum(2 * metric + sys::MADSIM_PAIRED_UP as usize) - sum(2 * metric + sys::MADSIM_PAIRED_DOWN as usize)
    }
    /// The seeds whose `metric` grew most from side A to side B.
    pub fn regressions(&self, metric: usize) -> &[sys::madsim_paired_extreme_t] {
        &self.top[2 * metric + sys::MADSIM_PAIRED_UP as usize]
    }
    /// The seeds whose `metric` shrank most.
    pub fn improvements(&self, metric: usize) -> &[sys::madsim_paired_extreme_t] {
        &self.top[2 * metric + sys::MADSIM_PAIRED_DOWN as usize]
    }
}

/// What `Builder::sweep_campaign` found: per variant its plain campaign report; the report — `n_by_mask[m]` = settled seeds that fail in
/// exactly the variants whose bits `m` has, the per-variant counts — and the smallest seeds the list rule selects (ascending), each
/// with its masks and every variant's verdict.
#[derive(Clone, Debug)]
pub struct Sweep {
    pub records: Vec<sys::madsim_sweep_record_t>,
    pub report: sys::madsim_sweep_t,
    pub campaigns: Vec<sys::madsim_campaign_t>,
}

impl Sweep {
    /// Settled seeds that fail in variant `v`.
    pub fn fails(&self, v: usize) -> u64 {
        (0..256usize).filter(|m| m >> v & 1 == 1).map(|m| self.report.n_by_mask[m]).sum()
    }
    /// True when every non-empty mask that occurs is a suffix set: the failing sets grow with the variant index.
    pub fn nested(&self) -> bool {
        let full = (1usize << self.campaigns.len()) - 1;
        (1..=full).all(|m| self.report.n_by_mask[m] == 0 || m == full & !((m & m.wrapping_neg()) - 1))
    }
    /// `[v]` = settled seeds whose lowest failing variant is `v`: the bisect reading.
    pub fn first_failing(&self) -> Vec<u64> {
        let mut h = vec![0u64; self.campaigns.len()];
        for m in 1..(1usize << self.campaigns.len()) {
            h[m.trailing_zeros() as usize] += self.report.n_by_mask[m];
        }
        h
    }
}

/// What `Builder::campaign_over_seeds` found over the listed seeds: the campaign report, and each part that was asked for.
#[derive(Clone, Debug)]
pub struct ListCampaign {
    pub campaign: sys::madsim_campaign_t,
    pub failures: Option<Failures>,
    pub stats: Option<Stats>,
    pub groups: Option<Groups>,
}

/// What one seed traced (`Builder::trace_seeds`): its result; `observations`, the first `obs_cap` values its test body handed to
/// `trace` / `trace_time` / a traced tick, in execution order — what `obs_hash` folds — and `n_observations`, how many there were;
/// `log`, the first `log_cap` bytes of its determinism log, and `log_len`, that log's length.  Under a runner verdict the lists are
/// what was recorded until the verdict: not meaningful.
#[derive(Clone, Debug)]
pub struct SeedTrace {
    pub seed: u64,
    pub result: sys::madsim_result_t,
    pub observations: Vec<u64>,
    pub n_observations: u64,
    pub log: Vec<u8>,
    pub log_len: u64,
}

/// Where the two runs of one seed part (`Builder::diverge_seeds`): `rec`, the record as the library gives it — per channel (determinism log,
/// observations) a `MADSIM_DIVERGE_*` status, the length of the common prefix that was established, the true lengths, each side's entry
/// there, and both results —; `shared`, the observations both runs made just before `rec.obs_at`; `next_a` / `next_b`, what each side
/// observed from there on (each at most `window` values).
#[derive(Clone, Debug)]
pub struct Divergence {
    pub rec: sys::madsim_divergence_t,
    pub shared: Vec<u64>,
    pub next_a: Vec<u64>,
    pub next_b: Vec<u64>,
}

/// Which traced values the seeds of a census reached, by verdict (`Builder::census` / `census_seeds`): `values`, ascending by value — per
/// distinct value the counted seeds of each verdict that observed it at least once, its occurrences, the smallest such seed and the most
/// occurrences inside one seed —; `totals`, the counts of `madsim_census_t` (its pointers are null here); `runner_seeds`, the seeds
/// left with a runner verdict, ascending: they are counted nowhere.
#[derive(Clone, Debug)]
pub struct Census {
    pub values: Vec<sys::madsim_census_value_t>,
    pub totals: sys::madsim_census_t,
    pub runner_seeds: Vec<u64>,
}

impl Census {
    /// The record of value `v`, or `None` when no counted seed observed it.
    pub fn row(&self, v: u64) -> Option<&sys::madsim_census_value_t> {
        self.values.binary_search_by_key(&v, |e| e.value).ok().map(|i| &self.values[i])
    }

    /// How many counted seeds observed `v` at least once.
    pub fn reached(&self, v: u64) -> u64 {
        self.row(v).map_or(0, |e| e.n_seeds.iter().sum())
    }

    /// The sometimes-assertion: those of `expected` that no counted seed observed, in the order given.
    pub fn never(&self, expected: &[u64]) -> Vec<u64> {
        expected.iter().copied().filter(|&v| self.row(v).is_none()).collect()
    }
}

/// When one seed traced what it traced (`Builder::timeline`): `result`, its 48 bytes; `observations`, the first `obs_cap` values its test
/// body handed to trace / trace_time / a traced tick, and `times`, the runtime's elapsed nanoseconds at each of them (what trace_instant
/// would have folded there) — two vectors of one length, the times never decreasing; `n_observations`, how many values there were.
#[derive(Clone, Debug)]
pub struct SeedTimeline {
    pub seed: u64,
    pub result: sys::madsim_result_t,
    pub observations: Vec<u64>,
    pub times: Vec<u64>,
    pub n_observations: u64,
}

/// How long, in virtual nanoseconds, from one traced value to another over a range of seeds (`Builder::probe_spans`): `definitions`, the
/// spans asked for (`ProbeSpans::between` / `ProbeSpans::start`); `spans`, one `madsim_span_t` per definition in that order — counted seeds
/// per verdict and `sys::MADSIM_SPAN_*` state, and over the CLOSED ones n, min, max, the 128-bit sum, the histogram under
/// `madsim_hip_stat_bucket`, the smallest seeds attaining the extremes and the smallest OPEN seed; `totals`, the counts (its pointers are
/// null); `runner_seeds`, the seeds left with a runner verdict.
#[derive(Clone, Debug)]
pub struct ProbeSpans {
    pub definitions: Vec<sys::madsim_span_def_t>,
    pub spans: Vec<sys::madsim_span_t>,
    pub totals: sys::madsim_probe_spans_t,
    pub runner_seeds: Vec<u64>,
}

impl ProbeSpans {
    /// From the first `from` to the first `to` behind it (`from == to`: the time between the first two occurrences).
    pub fn between(from: u64, to: u64) -> sys::madsim_span_def_t {
        sys::madsim_span_def_t { from, to, flags: 0, reserved: 0 }
    }

    /// From the start of the run to the first `to`.
    pub fn start(to: u64) -> sys::madsim_span_def_t {
        sys::madsim_span_def_t { from: 0, to, flags: sys::MADSIM_SPAN_FROM_START, reserved: 0 }
    }

    /// How many counted seeds closed span `i`.
    pub fn closed(&self, i: usize) -> u64 {
        self.spans[i].n
    }

    /// Counted seeds of span `i` in `sys::MADSIM_SPAN_*` state `state`, over the verdicts of the bit mask `verdicts`.
    pub fn state(&self, i: usize, state: u32, verdicts: u32) -> u64 {
        (0..4).filter(|k| (verdicts >> k) & 1 != 0).map(|k| self.spans[i].n_state[4 * k + state as usize]).sum()
    }

    /// The exact sum of span `i`'s durations.
    pub fn total(&self, i: usize) -> u128 {
        (self.spans[i].sum_hi as u128) << 64 | self.spans[i].sum_lo as u128
    }

    /// The smallest seed whose span `i` took the longest / the shortest; the smallest counted seed that never closed it.
    pub fn slowest(&self, i: usize) -> Option<u64> {
        if self.spans[i].n > 0 { Some(self.spans[i].max_seed) } else { None }
    }

    pub fn fastest(&self, i: usize) -> Option<u64> {
        if self.spans[i].n > 0 { Some(self.spans[i].min_seed) } else { None }
    }

    pub fn never_closed(&self, i: usize) -> Option<u64> {
        if self.state(i, sys::MADSIM_SPAN_OPEN, 0xf) > 0 { Some(self.spans[i].first_open_seed) } else { None }
    }
}

/// Where one seed's tasks stand when its run ends (`Builder::post_mortem`): `result`, its 48 bytes; `tasks`, the first `task_cap` records
/// of the tasks still alive, in task-slot order — bits 63-56 the state (`sys::MADSIM_TASK_PARKED` / `_QUEUED` / `_PANICKED` /
/// `_CANCELLED`), 55-48 the program, 47-32 the instruction, 31-16 and 15-0 the loop registers —; `n_tasks`, how many there were.  A seed
/// with a runner verdict has none.
#[derive(Clone, Debug)]
pub struct PostMortem {
    pub seed: u64,
    pub result: sys::madsim_result_t,
    pub tasks: Vec<u64>,
    pub n_tasks: u64,
}

impl PostMortem {
    /// (state, program, instruction, loop register 0, loop register 1) of a task record: the header's `MADSIM_TASK_*` accessors.
    pub fn fields(record: u64) -> (u32, u32, u32, u32, u32) {
        ((record >> 56) as u32, ((record >> 48) & 0xff) as u32, ((record >> 32) & 0xffff) as u32, ((record >> 16) & 0xffff) as u32, (record & 0xffff) as u32)
    }

    /// `MADSIM_TASK_SITE`: state | program | instruction, the loop registers dropped — the key of a stall census.
    pub fn site(record: u64) -> u64 {
        record >> 32
    }

    /// The shape word of this table (`madsim_hip_stall_shape`): what matches it against `StallCensus::shapes`.
    pub fn shape(&self) -> u64 {
        unsafe { sys::madsim_hip_stall_shape(self.tasks.as_ptr(), self.tasks.len() as u64) }
    }
}

/// Where the tasks of a range's seeds stand when their runs end, by verdict (`Builder::stall_census` / `stall_census_seeds`): `sites`,
/// ascending by site (`PostMortem::site` of a record) — per site the counted seeds of each verdict with at least one task there, the
/// tasks there, the most inside one seed and the smallest such seed —; `shapes`, ascending by shape word — per distinct multiset of sites
/// the counted seeds of each verdict and, in `first_seed`, the one to replay —; `totals`, the counts of `madsim_stall_census_t` (its
/// pointers are null here); `runner_seeds`, the seeds left with a runner verdict, ascending: they are counted nowhere.
#[derive(Clone, Debug)]
pub struct StallCensus {
    pub sites: Vec<sys::madsim_census_value_t>,
    pub shapes: Vec<sys::madsim_census_value_t>,
    pub totals: sys::madsim_stall_census_t,
    pub runner_seeds: Vec<u64>,
}

impl StallCensus {
    /// The shapes that counted seeds of `verdict` ended in, the most frequent first.
    pub fn shapes_of(&self, verdict: usize) -> Vec<sys::madsim_census_value_t> {
        let mut out: Vec<_> = self.shapes.iter().copied().filter(|e| e.n_seeds[verdict] != 0).collect();
        out.sort_by(|a, b| b.n_seeds[verdict].cmp(&a.n_seeds[verdict]).then(a.value.cmp(&b.value)));
        out
    }
}

/// Which combinations of the vocabulary's values the seeds reached, by verdict (`Builder::probe_sets` / `probe_sets_seeds`): `vocabulary`,
/// value `i` owning bit `i` of a set word; `sets`, ascending by set word — per distinct set the counted seeds of each verdict with exactly
/// this set and the smallest of them —; `totals`, the counts of `madsim_probe_sets_t` (its pointers are null here); `runner_seeds`, the
/// seeds left with a runner verdict, ascending: they are counted nowhere.
#[derive(Clone, Debug)]
pub struct ProbeSets {
    pub vocabulary: Vec<u64>,
    pub sets: Vec<sys::madsim_probe_set_t>,
    pub totals: sys::madsim_probe_sets_t,
    pub runner_seeds: Vec<u64>,
}

impl ProbeSets {
    /// The set-word bits of the vocabulary values `values` (a value outside the vocabulary owns no bit).
    pub fn mask(&self, values: &[u64]) -> u64 {
        values.iter().filter_map(|v| self.vocabulary.iter().position(|x| x == v)).fold(0, |m, i| m | 1u64 << i)
    }

    /// Counted seeds of the verdicts in `verdicts` (a bit mask, 0xf = all) that reached every value of `all_of` and none of `none_of`.
    pub fn count(&self, all_of: &[u64], none_of: &[u64], verdicts: u32) -> u64 {
        let (want, avoid) = (self.mask(all_of), self.mask(none_of));
        self.sets.iter().filter(|e| e.set & want == want && e.set & avoid == 0)
            .map(|e| (0..4).filter(|k| verdicts >> k & 1 == 1).map(|k| e.n_seeds[k]).sum::<u64>()).sum()
    }

    /// The sets that occur under PASS and under a failing verdict: (set word, the smallest passing seed, the smallest failing seed).
    pub fn mixed(&self) -> Vec<(u64, u64, u64)> {
        self.sets.iter().filter_map(|e| {
            let fail = (1..4).filter(|&k| e.n_seeds[k] > 0).map(|k| e.first_seed[k]).min();
            match fail { Some(f) if e.n_seeds[0] > 0 => Some((e.set, e.first_seed[0], f)), _ => None }
        }).collect()
    }

    /// A greedy set cover of every reached vocabulary value: each round the entry that adds the most new values, ties to the smaller set
    /// word; one seed (its smallest) per chosen entry, ascending and unique — a corpus for `Builder::over_seeds`.
    pub fn cover(&self) -> Vec<u64> {
        let vmask = if self.vocabulary.len() >= 64 { u64::MAX } else { (1u64 << self.vocabulary.len()) - 1 };
        let mut missing = self.sets.iter().fold(0u64, |m, e| m | (e.set & vmask));
        let mut chosen = Vec::new();
        while missing != 0 {
            let mut best: Option<&sys::madsim_probe_set_t> = None;
            for e in &self.sets {                                        // ascending by set word: the first of the best wins
                if best.map_or(true, |b| (e.set & missing).count_ones() > (b.set & missing).count_ones()) {
                    best = Some(e);
                }
            }
            let e = best.unwrap();
            chosen.push((0..4).filter(|&k| e.n_seeds[k] > 0).map(|k| e.first_seed[k]).min().unwrap_or(0));
            missing &= !e.set;
        }
        chosen.sort_unstable();
        chosen.dedup();
        chosen
    }
}

/// Which vocabulary value the seeds reached first, by verdict (`Builder::probe_order` / `probe_order_seeds`): `vocabulary`; `pairs`, ascending
/// by (a, b), a and b indices into the vocabulary — a == b: the counted seeds of each verdict that reached the value; a != b: those that
/// reached both and saw a first — each with the smallest such seed; `totals`, the counts of `madsim_probe_order_t` (its pointers are null
/// here); `runner_seeds`, the seeds left with a runner verdict, ascending: they are counted nowhere.
#[derive(Clone, Debug)]
pub struct ProbeOrder {
    pub vocabulary: Vec<u64>,
    pub pairs: Vec<sys::madsim_probe_order_pair_t>,
    pub totals: sys::madsim_probe_order_t,
    pub runner_seeds: Vec<u64>,
}

impl ProbeOrder {
    /// Counted seeds of the verdicts in `verdicts` (a bit mask, 0xf = all) that reached both values and saw `a` first (a == b: that reached
    /// `a`); 0 for a value outside the vocabulary.
    pub fn before(&self, a: u64, b: u64, verdicts: u32) -> u64 {
        let at = |v: u64| self.vocabulary.iter().position(|x| *x == v);
        match (at(a), at(b)) {
            (Some(ia), Some(ib)) => self.pairs.iter().filter(|e| e.a as usize == ia && e.b as usize == ib)
                .map(|e| (0..4).filter(|k| verdicts >> k & 1 == 1).map(|k| e.n_seeds[k]).sum::<u64>()).sum(),
            _ => 0,
        }
    }

    /// Counted seeds of `verdicts` that reached `a`.
    pub fn reached(&self, a: u64, verdicts: u32) -> u64 {
        self.before(a, a, verdicts)
    }

    /// Counted seeds of `verdicts` that reached both `a` and `b`: two values never share an index, so one of them came first.
    pub fn both(&self, a: u64, b: u64, verdicts: u32) -> u64 {
        if a == b { self.reached(a, verdicts) } else { self.before(a, b, verdicts) + self.before(b, a, verdicts) }
    }

    /// Some counted seed of `verdicts` reached both, and none of them saw `b` first.
    pub fn always_before(&self, a: u64, b: u64, verdicts: u32) -> bool {
        a != b && self.both(a, b, verdicts) > 0 && self.before(b, a, verdicts) == 0
    }
}

/// The `obs_hash` of a run that traced `values`, in that order: 64-bit FNV-1a over whole values (the offset basis for none).
pub fn fold_observations(values: &[u64]) -> u64 {
    values.iter().fold(0xCBF2_9CE4_8422_2325u64, |h, v| (h ^ v).wrapping_mul(0x100_0000_01B3))
}

impl Diff {
    /// Seeds that passed on side A and carry any other verdict on side B.
    pub fn regressions(&self) -> u64 {
        self.report.transitions[sys::MADSIM_PASS as usize][1..].iter().sum()
    }
}

impl Builder {
    /// builder.rs:64-118: `MADSIM_TEST_SEED`, `MADSIM_TEST_NUM`, `MADSIM_TEST_JOBS`, `MADSIM_TEST_TIME_LIMIT`,
    /// `MADSIM_TEST_CHECK_DETERMINISM`, `MADSIM_ALLOW_SYSTEM_THREAD` (`MADSIM_TEST_CONFIG` is read by the caller: the TOML
    /// parser lives in madsim).
    pub fn from_env() -> Self {
        let seed: u64 = if let Ok(s) = std::env::var("MADSIM_TEST_SEED") {
            s.parse().expect("MADSIM_TEST_SEED should be an integer")
        } else {
            SystemTime::now().duration_since(SystemTime::UNIX_EPOCH).unwrap().as_nanos() as _
        };
        let jobs: u16 = if let Ok(s) = std::env::var("MADSIM_TEST_JOBS") {
            s.parse().expect("MADSIM_TEST_JOBS should be an integer")
        } else {
            1
        };
        let mut count: u64 = if let Ok(s) = std::env::var("MADSIM_TEST_NUM") {
            s.parse().expect("MADSIM_TEST_NUM should be an integer")
        } else {
            1
        };
        let time_limit = std::env::var("MADSIM_TEST_TIME_LIMIT")
            .ok()
            .map(|s| Duration::from_secs_f64(s.parse::<f64>().expect("MADSIM_TEST_TIME_LIMIT should be an number")));
        let check = std::env::var("MADSIM_TEST_CHECK_DETERMINISM").is_ok();
        if check {
            count = count.max(2);
        }
        let allow_system_thread = std::env::var("MADSIM_ALLOW_SYSTEM_THREAD").is_ok();
        Builder { seed, count, jobs, config: NetConfig::default(), time_limit, check, allow_system_thread, limits: zero_limits(), resolve_flags: 0 }
    }

    /// `search_failures`, `campaign_stats`, `failure_groups` and `diff_campaign` report on SETTLED results: seeds that come back with a
    /// runner verdict (a device capacity, the step cap) are run again on the device under grown limits, up to `rounds` times (0 = the
    /// library's default, at most `MADSIM_RESOLVE_MAX_ROUNDS`), before their batch is reported (`MADSIM_CAMPAIGN_RESOLVE`).
    pub fn resolve_runner(mut self, rounds: u32) -> Self {
        assert!(rounds <= sys::MADSIM_RESOLVE_MAX_ROUNDS, "resolve_runner: at most MADSIM_RESOLVE_MAX_ROUNDS rounds");
        self.resolve_flags = sys::MADSIM_CAMPAIGN_RESOLVE | rounds << sys::MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT;
        self
    }

    /// The resolve account of the most recent campaign call (`madsim_hip_ctx_campaign_resolved`): how many seeds the first pass left
    /// re-runnable, how many each round re-ran, how many ended settled.
    pub fn resolved(&self) -> Result<sys::madsim_resolve_t, RunError> {
        let ctx = contexts()?.0[0];
        let mut r: sys::madsim_resolve_t = unsafe { std::mem::zeroed() };
        let rc = unsafe { sys::madsim_hip_ctx_campaign_resolved(ctx, &mut r) };
        if rc != 0 {
            return Err(last_error(rc));
        }
        Ok(r)
    }

    fn raw_limits(&self, with_time_limit: bool) -> sys::madsim_limits_t {
        let mut lim = self.limits;
        if with_time_limit {
            if let Some(d) = self.time_limit {
                // 0 means None in the C-ABI; Some(Duration::ZERO) panics at the first idle advance (task/mod.rs:253-258), as 1 ns does
                lim.time_limit_ns = (d.as_nanos() as u64).max(1);
            }
        }
        lim
    }

    /// The raw determinism log of one seed (rand.rs:64-88) and its result.
    fn trace(&self, w: &sys::madsim_workload_t, cfg: &sys::madsim_config_t, lim: &sys::madsim_limits_t) -> Result<(Vec<u8>, sys::madsim_result_t), RunError> {
        let ctx = contexts()?.0[0];
        let mut log = vec![0u8; 1 << 20];
        let mut res: sys::madsim_result_t = unsafe { std::mem::zeroed() };
        let n = unsafe { sys::madsim_hip_ctx_trace_seed(ctx, w, cfg, self.seed, lim, log.as_mut_ptr(), log.len() as u64, &mut res) };
        if n < 0 {
            return Err(last_error(n as c_int));
        }
        log.truncate((n as usize).min(log.len()));
        Ok((log, res))
    }

    /// What `seeds` traced (`madsim_hip_ctx_trace_seeds`): any order, duplicates allowed, the whole list in ONE launch of the trace build,
    /// one `SeedTrace` per seed in the order given — the output a failing `#[madsim::test]` prints, for the seeds `search_failures`,
    /// `failure_groups` and `diff_campaign` list.  With `resolve_runner` set, seeds that come back with a re-runnable runner verdict
    /// are replayed as one further call per round under `madsim_hip_grow_limits(.., r)`, r = 1, 2, .. — a resolving campaign's rounds.
    pub fn trace_seeds(&self, workload: &Workload, seeds: &[u64], obs_cap: usize, log_cap: usize) -> Result<Vec<SeedTrace>, RunError> {
        let w = workload.raw();
        let cfg = self.config.raw();
        let lim0 = self.raw_limits(true);
        let ctx = contexts()?.0[0];
        let zero: sys::madsim_result_t = unsafe { std::mem::zeroed() };
        let mut traces: Vec<SeedTrace> =
            seeds.iter().map(|&seed| SeedTrace { seed, result: zero, observations: Vec::new(), n_observations: 0, log: Vec::new(), log_len: 0 }).collect();
        let mut idx: Vec<usize> = (0..seeds.len()).collect();
        let rounds = if self.resolve_flags & sys::MADSIM_CAMPAIGN_RESOLVE == 0 {
            0
        } else {
            match (self.resolve_flags & sys::MADSIM_CAMPAIGN_RESOLVE_ROUNDS_MASK) >> sys::MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT {
                0 => sys::MADSIM_RESOLVE_DEFAULT_ROUNDS,
                r => r,
            }
        };
        for r in 0..=rounds {
            if idx.is_empty() {
                break;
            }
            let mut lim = lim0;
            if r > 0 {
                let rc = unsafe { sys::madsim_hip_grow_limits(&w, &lim0, r, &mut lim) };
                if rc != 0 {
                    return Err(last_error(rc));
                }
            }
            let m = idx.len();
            let s: Vec<u64> = idx.iter().map(|&i| seeds[i]).collect();
            let (mut obs, mut logs) = (vec![0u64; m * obs_cap], vec![0u8; m * log_cap]);
            let (mut olen, mut llen) = (vec![0u64; m], vec![0u64; m]);
            let mut res = vec![zero; m];
            let rc = unsafe {
                sys::madsim_hip_ctx_trace_seeds(ctx, &w, &cfg, s.as_ptr(), m as u64, &lim,
                                                if log_cap > 0 { logs.as_mut_ptr() } else { std::ptr::null_mut() }, log_cap as u64,
                                                if obs_cap > 0 { obs.as_mut_ptr() } else { std::ptr::null_mut() }, obs_cap as u64,
                                                llen.as_mut_ptr(), olen.as_mut_ptr(), res.as_mut_ptr())
            };
            if rc != 0 {
                return Err(last_error(rc));
            }
            let cap = if lim.max_steps != 0 { lim.max_steps } else { 1 << 24 };
            let ceiling = if lim.max_steps_ceiling != 0 { lim.max_steps_ceiling } else { 1 << 28 };
            let mut again = Vec::new();
            for (j, &i) in idx.iter().enumerate() {
                let t = &mut traces[i];
                t.result = res[j];
                t.n_observations = olen[j];
                t.log_len = llen[j];
                t.observations = obs[j * obs_cap..j * obs_cap + (olen[j] as usize).min(obs_cap)].to_vec();
                t.log = logs[j * log_cap..j * log_cap + (llen[j] as usize).min(log_cap)].to_vec();
                if res[j].verdict == sys::MADSIM_OVERFLOW || (res[j].verdict == sys::MADSIM_STEP_LIMIT && cap < ceiling) {
                    again.push(i);
                }
            }
            idx = again;
        }
        Ok(traces)
    }

    /// Where the two runs of each of `seeds` part (`madsim_hip_ctx_diverge_seeds`): this builder's run of `workload` (side A) against
    /// `other`'s run of `other_workload` (side B), compared on the device on the determinism log and on the observations — per seed the
    /// record, the up to `window` observations both runs made just before they part and the up to `window` each side made from there on.
    /// No row travels to the host.  With `resolve_runner` set, seeds that come back incomparable with a re-runnable runner verdict on
    /// either side are replayed in one further call per round, each side under its own `madsim_hip_grow_limits(.., r)`.
    pub fn diverge_seeds(&self, workload: &Workload, other: &Builder, other_workload: &Workload, seeds: &[u64], log_cap: usize, obs_cap: usize,
                         window: u32) -> Result<Vec<Divergence>, RunError> {
        let (wa, wb) = (workload.raw(), other_workload.raw());
        let (ca, cb) = (self.config.raw(), other.config.raw());
        let (la0, lb0) = (self.raw_limits(true), other.raw_limits(true));
        let ctx = contexts()?.0[0];
        let win = window as usize;
        let mut out: Vec<Divergence> =
            seeds.iter().map(|_| Divergence { rec: unsafe { std::mem::zeroed() }, shared: Vec::new(), next_a: Vec::new(), next_b: Vec::new() }).collect();
        let mut idx: Vec<usize> = (0..seeds.len()).collect();
        let rounds = if self.resolve_flags & sys::MADSIM_CAMPAIGN_RESOLVE == 0 {
            0
        } else {
            match (self.resolve_flags & sys::MADSIM_CAMPAIGN_RESOLVE_ROUNDS_MASK) >> sys::MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT {
                0 => sys::MADSIM_RESOLVE_DEFAULT_ROUNDS,
                r => r,
            }
        };
        let rerunnable = |x: &sys::madsim_result_t, lim: &sys::madsim_limits_t| {
            let cap = if lim.max_steps != 0 { lim.max_steps } else { 1 << 24 };
            let ceiling = if lim.max_steps_ceiling != 0 { lim.max_steps_ceiling } else { 1 << 28 };
            x.verdict == sys::MADSIM_OVERFLOW || (x.verdict == sys::MADSIM_STEP_LIMIT && cap < ceiling)
        };
        for r in 0..=rounds {
            if idx.is_empty() {
                break;
            }
            let (mut la, mut lb) = (la0, lb0);
            if r > 0 {
                for rc in [unsafe { sys::madsim_hip_grow_limits(&wa, &la0, r, &mut la) }, unsafe { sys::madsim_hip_grow_limits(&wb, &lb0, r, &mut lb) }] {
                    if rc != 0 {
                        return Err(last_error(rc));
                    }
                }
            }
            let m = idx.len();
            let s: Vec<u64> = idx.iter().map(|&i| seeds[i]).collect();
            let mut recs: Vec<sys::madsim_divergence_t> = vec![unsafe { std::mem::zeroed() }; m];
            let mut rows = vec![0u64; m * 3 * win];
            let rc = unsafe {
                sys::madsim_hip_ctx_diverge_seeds(ctx, &wa, &ca, &la, &wb, &cb, &lb, s.as_ptr(), m as u64, log_cap as u64, obs_cap as u64, window,
                                                  recs.as_mut_ptr(), if win > 0 { rows.as_mut_ptr() } else { std::ptr::null_mut() })
            };
            if rc != 0 {
                return Err(last_error(rc));
            }
            let mut again = Vec::new();
            for (j, &i) in idx.iter().enumerate() {
                let rec = recs[j];
                let d = &mut out[i];
                d.rec = rec;
                d.shared.clear();
                d.next_a.clear();
                d.next_b.clear();
                if rec.obs_status != sys::MADSIM_DIVERGE_INCOMPARABLE {
                    let row = &rows[j * 3 * win..(j + 1) * 3 * win];
                    let at = rec.obs_at as usize;
                    let (ka, kb) = ((rec.obs_len_a as usize).min(obs_cap), (rec.obs_len_b as usize).min(obs_cap));
                    d.shared = row[win - at.min(win)..win].to_vec();
                    d.next_a = row[win..win + ka.saturating_sub(at).min(win)].to_vec();
                    d.next_b = row[2 * win..2 * win + kb.saturating_sub(at).min(win)].to_vec();
                }
                if rerunnable(&rec.a, &la) || rerunnable(&rec.b, &lb) {
                    again.push(i);
                }
            }
            idx = again;
        }
        Ok(out)
    }

    /// Which traced values the seeds `self.seed .. self.seed + self.count` reach, by verdict (`madsim_hip_ctx_census_range`): the range run
    /// on the trace build and reduced on the device, nothing but the table coming back.  A seed is counted when its verdict bit is set
    /// in `include` (bits 0-3); its first `obs_cap` observations are visible; more than `max_values` distinct values is an error
    /// (`MADSIM_E_LIMITS`: a traced time or random value is not a probe vocabulary).  With `resolve_runner` set, the seeds a call leaves
    /// with a runner verdict are run again in one list call per round under `madsim_hip_grow_limits(.., r)` and merged in.
    pub fn census(&self, workload: &Workload, include: u32, obs_cap: u32, max_values: usize) -> Result<Census, RunError> {
        self.census_over(workload, None, include, obs_cap, max_values)
    }

    /// `census` over an explicit, strictly ascending seed list (`madsim_hip_ctx_census_seeds`).
    pub fn census_seeds(&self, workload: &Workload, seeds: &[u64], include: u32, obs_cap: u32, max_values: usize) -> Result<Census, RunError> {
        self.census_over(workload, Some(seeds), include, obs_cap, max_values)
    }

    fn census_over(&self, workload: &Workload, seeds: Option<&[u64]>, include: u32, obs_cap: u32, max_values: usize) -> Result<Census, RunError> {
        let w = workload.raw();
        let cfg = self.config.raw();
        let lim0 = self.raw_limits(true);
        let ctx = contexts()?.0[0];
        let rounds = if self.resolve_flags & sys::MADSIM_CAMPAIGN_RESOLVE == 0 {
            0
        } else {
            match (self.resolve_flags & sys::MADSIM_CAMPAIGN_RESOLVE_ROUNDS_MASK) >> sys::MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT {
                0 => sys::MADSIM_RESOLVE_DEFAULT_ROUNDS,
                r => r,
            }
        };
        let one = |lim: &sys::madsim_limits_t, list: Option<&[u64]>| -> Result<Census, RunError> {
            let n = list.map_or(self.count, |l| l.len() as u64);
            let mut values: Vec<sys::madsim_census_value_t> = vec![unsafe { std::mem::zeroed() }; max_values.max(1)];
            let mut runner = vec![0u64; (n as usize).max(1)];
            let mut cen: sys::madsim_census_t = unsafe { std::mem::zeroed() };
            cen.include = include;
            cen.obs_cap = obs_cap;
            cen.values = values.as_mut_ptr() as *const _;                // (the library writes through both)
            cen.cap = max_values as u64;
            cen.runner_seeds = runner.as_mut_ptr() as *const _;
            cen.runner_cap = n;
            let rc = unsafe {
                match list {
                    Some(l) => sys::madsim_hip_ctx_census_seeds(ctx, &w, &cfg, l.as_ptr(), n, 0, lim, &mut cen),
                    None => sys::madsim_hip_ctx_census_range(ctx, &w, &cfg, self.seed, n, 0, lim, &mut cen),
                }
            };
            if rc != 0 {
                return Err(last_error(rc));
            }
            values.truncate(cen.n_values as usize);
            runner.truncate(cen.n_runner_listed as usize);
            cen.values = std::ptr::null();
            cen.runner_seeds = std::ptr::null();
            Ok(Census { values, totals: cen, runner_seeds: runner })
        };
        let mut c = one(&lim0, seeds)?;
        for r in 1..=rounds {
            if c.runner_seeds.is_empty() {
                break;
            }
            let mut lim = lim0;
            let rc = unsafe { sys::madsim_hip_grow_limits(&w, &lim0, r, &mut lim) };
            if rc != 0 {
                return Err(last_error(rc));
            }
            let more = one(&lim, Some(&c.runner_seeds))?;
            let mut merged = Vec::with_capacity(c.values.len() + more.values.len());
            let (mut i, mut j) = (0, 0);
            while i < c.values.len() || j < more.values.len() {
                if j >= more.values.len() || (i < c.values.len() && c.values[i].value < more.values[j].value) {
                    merged.push(c.values[i]);
                    i += 1;
                } else if i >= c.values.len() || more.values[j].value < c.values[i].value {
                    merged.push(more.values[j]);
                    j += 1;
                } else {
                    let (mut e, o) = (c.values[i], more.values[j]);
                    for k in 0..4 {
                        e.n_seeds[k] += o.n_seeds[k];
                    }
                    e.n_total += o.n_total;
                    e.first_seed = e.first_seed.min(o.first_seed);
                    e.max_per_seed = e.max_per_seed.max(o.max_per_seed);
                    merged.push(e);
                    i += 1;
                    j += 1;
                }
            }
            if merged.len() > max_values {
                return Err(RunError { code: sys::MADSIM_E_LIMITS, message: "census: more than max_values distinct observed values once the runner seeds are settled".into() });
            }
            for k in 0..4 {
                c.totals.n_counted[k] += more.totals.n_counted[k];
                c.totals.n_silent[k] += more.totals.n_silent[k];
            }
            c.totals.n_truncated += more.totals.n_truncated;
            c.totals.n_observations += more.totals.n_observations;
            c.totals.n_runner = more.totals.n_runner;
            c.totals.n_runner_listed = more.totals.n_runner_listed;
            c.totals.n_values = merged.len() as u64;
            c.values = merged;
            c.runner_seeds = more.runner_seeds;
        }
        Ok(c)
    }

    /// Where the tasks of `seeds` stand when their runs end (`madsim_hip_ctx_task_states`): any order, duplicates allowed, the whole list
    /// in ONE launch of the trace build, one `PostMortem` per seed in the order given.  With `resolve_runner` set, seeds that come back
    /// with a re-runnable runner verdict are replayed as one further call per round under `madsim_hip_grow_limits(.., r)`.
    pub fn post_mortem(&self, workload: &Workload, seeds: &[u64], task_cap: usize) -> Result<Vec<PostMortem>, RunError> {
        let w = workload.raw();
        let cfg = self.config.raw();
        let lim0 = self.raw_limits(true);
        let ctx = contexts()?.0[0];
        let zero: sys::madsim_result_t = unsafe { std::mem::zeroed() };
        let mut out: Vec<PostMortem> = seeds.iter().map(|&seed| PostMortem { seed, result: zero, tasks: Vec::new(), n_tasks: 0 }).collect();
        let mut idx: Vec<usize> = (0..seeds.len()).collect();
        for r in 0..=self.resolve_rounds() {
            if idx.is_empty() {
                break;
            }
            let mut lim = lim0;
            if r > 0 {
                let rc = unsafe { sys::madsim_hip_grow_limits(&w, &lim0, r, &mut lim) };
                if rc != 0 {
                    return Err(last_error(rc));
                }
            }
            let m = idx.len();
            let s: Vec<u64> = idx.iter().map(|&i| seeds[i]).collect();
            let (mut rows, mut lens) = (vec![0u64; m * task_cap], vec![0u64; m]);
            let mut res = vec![zero; m];
            let rc = unsafe {
                sys::madsim_hip_ctx_task_states(ctx, &w, &cfg, s.as_ptr(), m as u64, &lim,
                                                if task_cap > 0 { rows.as_mut_ptr() } else { std::ptr::null_mut() }, task_cap as u64,
                                                lens.as_mut_ptr(), res.as_mut_ptr())
            };
            if rc != 0 {
                return Err(last_error(rc));
            }
            let cap = if lim.max_steps != 0 { lim.max_steps } else { 1 << 24 };
            let ceiling = if lim.max_steps_ceiling != 0 { lim.max_steps_ceiling } else { 1 << 28 };
            let mut again = Vec::new();
            for (j, &i) in idx.iter().enumerate() {
                let p = &mut out[i];
                p.result = res[j];
                p.n_tasks = lens[j];
                p.tasks = rows[j * task_cap..j * task_cap + (lens[j] as usize).min(task_cap)].to_vec();
                if res[j].verdict == sys::MADSIM_OVERFLOW || (res[j].verdict == sys::MADSIM_STEP_LIMIT && cap < ceiling) {
                    again.push(i);
                }
            }
            idx = again;
        }
        Ok(out)
    }

    /// When `seeds` traced what they traced (`madsim_hip_ctx_timeline_seeds`): any order, duplicates allowed, the whole list in ONE launch
    /// of the trace build, one `SeedTimeline` per seed in the order given.  `resolve_runner` rounds apply as in `post_mortem`.
    pub fn timeline(&self, workload: &Workload, seeds: &[u64], obs_cap: usize) -> Result<Vec<SeedTimeline>, RunError> {
        let w = workload.raw();
        let cfg = self.config.raw();
        let lim0 = self.raw_limits(true);
        let ctx = contexts()?.0[0];
        let zero: sys::madsim_result_t = unsafe { std::mem::zeroed() };
        let mut out: Vec<SeedTimeline> =
            seeds.iter().map(|&seed| SeedTimeline { seed, result: zero, observations: Vec::new(), times: Vec::new(), n_observations: 0 }).collect();
        let mut idx: Vec<usize> = (0..seeds.len()).collect();
        for r in 0..=self.resolve_rounds() {
            if idx.is_empty() {
                break;
            }
            let mut lim = lim0;
            if r > 0 {
                let rc = unsafe { sys::madsim_hip_grow_limits(&w, &lim0, r, &mut lim) };
                if rc != 0 {
                    return Err(last_error(rc));
                }
            }
            let m = idx.len();
            let s: Vec<u64> = idx.iter().map(|&i| seeds[i]).collect();
            let (mut obs, mut tim, mut lens) = (vec![0u64; m * obs_cap], vec![0u64; m * obs_cap], vec![0u64; m]);
            let mut res = vec![zero; m];
            let rc = unsafe {
                sys::madsim_hip_ctx_timeline_seeds(ctx, &w, &cfg, s.as_ptr(), m as u64, &lim, obs.as_mut_ptr(), tim.as_mut_ptr(), obs_cap as u64,
                                                   lens.as_mut_ptr(), res.as_mut_ptr())
            };
            if rc != 0 {
                return Err(last_error(rc));
            }
            let cap = if lim.max_steps != 0 { lim.max_steps } else { 1 << 24 };
            let ceiling = if lim.max_steps_ceiling != 0 { lim.max_steps_ceiling } else { 1 << 28 };
            let mut again = Vec::new();
            for (j, &i) in idx.iter().enumerate() {
                let t = &mut out[i];
                let k = (lens[j] as usize).min(obs_cap);
                t.result = res[j];
                t.n_observations = lens[j];
                t.observations = obs[j * obs_cap..j * obs_cap + k].to_vec();
                t.times = tim[j * obs_cap..j * obs_cap + k].to_vec();
                if res[j].verdict == sys::MADSIM_OVERFLOW || (res[j].verdict == sys::MADSIM_STEP_LIMIT && cap < ceiling) {
                    again.push(i);
                }
            }
            idx = again;
        }
        Ok(out)
    }

    /// How long from the first traced `from` to the first `to` behind it, for 1 .. 16 `definitions`, over the seeds
    /// `self.seed .. self.seed + self.count` (`madsim_hip_ctx_probe_spans_range`): the range run on the trace build with the time log and
    /// reduced on the device to one record per definition.  `include`, `obs_cap`: as `census`.  With `resolve_runner` set, the seeds a call
    /// leaves with a runner verdict are run again in one list call per round and merged in (`madsim_hip_span_merge`).
    pub fn probe_spans(&self, workload: &Workload, definitions: &[sys::madsim_span_def_t], include: u32, obs_cap: u32) -> Result<ProbeSpans, RunError> {
        self.probe_spans_over(workload, definitions, None, include, obs_cap)
    }

    /// `probe_spans` over an explicit, strictly ascending seed list (`madsim_hip_ctx_probe_spans_seeds`).
    pub fn probe_spans_seeds(&self, workload: &Workload, definitions: &[sys::madsim_span_def_t], seeds: &[u64], include: u32, obs_cap: u32) -> Result<ProbeSpans, RunError> {
        self.probe_spans_over(workload, definitions, Some(seeds), include, obs_cap)
    }

    fn probe_spans_over(&self, workload: &Workload, definitions: &[sys::madsim_span_def_t], seeds: Option<&[u64]>, include: u32, obs_cap: u32) -> Result<ProbeSpans, RunError> {
        let w = workload.raw();
        let cfg = self.config.raw();
        let lim0 = self.raw_limits(true);
        let ctx = contexts()?.0[0];
        let one = |lim: &sys::madsim_limits_t, list: Option<&[u64]>| -> Result<ProbeSpans, RunError> {
            let n = list.map_or(self.count, |l| l.len() as u64);
            let mut spans: Vec<sys::madsim_span_t> = vec![unsafe { std::mem::zeroed() }; definitions.len().max(1)];
            let mut runner = vec![0u64; (n as usize).max(1)];
            let mut ps: sys::madsim_probe_spans_t = unsafe { std::mem::zeroed() };
            ps.include = include;
            ps.obs_cap = obs_cap;
            ps.defs = definitions.as_ptr();
            ps.n_spans = definitions.len() as u64;
            ps.spans = spans.as_mut_ptr() as *const _;                   // (the library writes through both)
            ps.runner_seeds = runner.as_mut_ptr() as *const _;
            ps.runner_cap = n;
            let rc = unsafe {
                match list {
                    Some(l) => sys::madsim_hip_ctx_probe_spans_seeds(ctx, &w, &cfg, l.as_ptr(), n, 0, lim, &mut ps),
                    None => sys::madsim_hip_ctx_probe_spans_range(ctx, &w, &cfg, self.seed, n, 0, lim, &mut ps),
                }
            };
            if rc != 0 {
                return Err(last_error(rc));
            }
            spans.truncate(definitions.len());
            runner.truncate(ps.n_runner_listed as usize);
            ps.defs = std::ptr::null();
            ps.spans = std::ptr::null();
            ps.runner_seeds = std::ptr::null();
            Ok(ProbeSpans { definitions: definitions.to_vec(), spans, totals: ps, runner_seeds: runner })
        };
        let mut c = one(&lim0, seeds)?;
        for r in 1..=self.resolve_rounds() {
            if c.runner_seeds.is_empty() {
                break;
            }
            let mut lim = lim0;
            let rc = unsafe { sys::madsim_hip_grow_limits(&w, &lim0, r, &mut lim) };
            if rc != 0 {
                return Err(last_error(rc));
            }
            let more = one(&lim, Some(&c.runner_seeds))?;
            for (a, b) in c.spans.iter_mut().zip(more.spans.iter()) {
                unsafe { sys::madsim_hip_span_merge(a, b) };
            }
            for k in 0..4 {
                c.totals.n_counted[k] += more.totals.n_counted[k];
            }
            c.totals.n_truncated += more.totals.n_truncated;
            c.totals.n_runner = more.totals.n_runner;
            c.totals.n_runner_listed = more.totals.n_runner_listed;
            c.runner_seeds = more.runner_seeds;
        }
        Ok(c)
    }

    fn resolve_rounds(&self) -> u32 {
        if self.resolve_flags & sys::MADSIM_CAMPAIGN_RESOLVE == 0 {
            return 0;
        }
        match (self.resolve_flags & sys::MADSIM_CAMPAIGN_RESOLVE_ROUNDS_MASK) >> sys::MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT {
            0 => sys::MADSIM_RESOLVE_DEFAULT_ROUNDS,
            r => r,
        }
    }

    /// Where the tasks of the seeds `self.seed .. self.seed + self.count` stand when their runs end, by verdict
    /// (`madsim_hip_ctx_stall_census_range`): the range run on the trace build with the task log and reduced on the device to one entry
    /// per distinct site and one per distinct shape.  A seed is counted when its verdict bit is set in `include` (bits 0-3); its first
    /// `task_cap` live tasks are visible; more than `max_sites` distinct sites or `max_shapes` distinct shapes is an error
    /// (`MADSIM_E_LIMITS`; `max_shapes` 0: no shapes pass).  With `resolve_runner` set, the seeds a call leaves with a runner verdict are
    /// run again in one list call per round and merged in.
    pub fn stall_census(&self, workload: &Workload, include: u32, task_cap: u32, max_sites: usize, max_shapes: usize) -> Result<StallCensus, RunError> {
        self.stall_census_over(workload, None, include, task_cap, max_sites, max_shapes)
    }

    /// `stall_census` over an explicit, strictly ascending seed list (`madsim_hip_ctx_stall_census_seeds`).
    pub fn stall_census_seeds(&self, workload: &Workload, seeds: &[u64], include: u32, task_cap: u32, max_sites: usize, max_shapes: usize) -> Result<StallCensus, RunError> {
        self.stall_census_over(workload, Some(seeds), include, task_cap, max_sites, max_shapes)
    }

    fn stall_census_over(&self, workload: &Workload, seeds: Option<&[u64]>, include: u32, task_cap: u32, max_sites: usize, max_shapes: usize) -> Result<StallCensus, RunError> {
        let w = workload.raw();
        let cfg = self.config.raw();
        let lim0 = self.raw_limits(true);
        let ctx = contexts()?.0[0];
        let one = |lim: &sys::madsim_limits_t, list: Option<&[u64]>| -> Result<StallCensus, RunError> {
            let n = list.map_or(self.count, |l| l.len() as u64);
            let mut sites: Vec<sys::madsim_census_value_t> = vec![unsafe { std::mem::zeroed() }; max_sites.max(1)];
            let mut shapes: Vec<sys::madsim_census_value_t> = vec![unsafe { std::mem::zeroed() }; max_shapes.max(1)];
            let mut runner = vec![0u64; (n as usize).max(1)];
            let mut sc: sys::madsim_stall_census_t = unsafe { std::mem::zeroed() };
            sc.include = include;
            sc.task_cap = task_cap;
            sc.sites = sites.as_mut_ptr() as *const _;                   // (the library writes through all three)
            sc.site_cap = max_sites as u64;
            sc.shapes = if max_shapes > 0 { shapes.as_mut_ptr() as *const _ } else { std::ptr::null() };
            sc.shape_cap = max_shapes as u64;
            sc.runner_seeds = runner.as_mut_ptr() as *const _;
            sc.runner_cap = n;
            let rc = unsafe {
                match list {
                    Some(l) => sys::madsim_hip_ctx_stall_census_seeds(ctx, &w, &cfg, l.as_ptr(), n, 0, lim, &mut sc),
                    None => sys::madsim_hip_ctx_stall_census_range(ctx, &w, &cfg, self.seed, n, 0, lim, &mut sc),
                }
            };
            if rc != 0 {
                return Err(last_error(rc));
            }
            sites.truncate(sc.n_sites as usize);
            shapes.truncate(sc.n_shapes as usize);
            runner.truncate(sc.n_runner_listed as usize);
            sc.sites = std::ptr::null();
            sc.shapes = std::ptr::null();
            sc.runner_seeds = std::ptr::null();
            Ok(StallCensus { sites, shapes, totals: sc, runner_seeds: runner })
        };
        let merge = |into: &[sys::madsim_census_value_t], more: &[sys::madsim_census_value_t]| {
            let mut merged = Vec::with_capacity(into.len() + more.len());
            let (mut i, mut j) = (0, 0);
            while i < into.len() || j < more.len() {
                if j >= more.len() || (i < into.len() && into[i].value < more[j].value) {
                    merged.push(into[i]);
                    i += 1;
                } else if i >= into.len() || more[j].value < into[i].value {
                    merged.push(more[j]);
                    j += 1;
                } else {
                    let (mut e, o) = (into[i], more[j]);
                    for k in 0..4 {
                        e.n_seeds[k] += o.n_seeds[k];
                    }
                    e.n_total += o.n_total;
                    e.first_seed = e.first_seed.min(o.first_seed);
                    e.max_per_seed = e.max_per_seed.max(o.max_per_seed);
                    merged.push(e);
                    i += 1;
                    j += 1;
                }
            }
            merged
        };
        let mut c = one(&lim0, seeds)?;
        for r in 1..=self.resolve_rounds() {
            if c.runner_seeds.is_empty() {
                break;
            }
            let mut lim = lim0;
            let rc = unsafe { sys::madsim_hip_grow_limits(&w, &lim0, r, &mut lim) };
            if rc != 0 {
                return Err(last_error(rc));
            }
            let more = one(&lim, Some(&c.runner_seeds))?;
            let (sites, shapes) = (merge(&c.sites, &more.sites), merge(&c.shapes, &more.shapes));
            if sites.len() > max_sites || shapes.len() > max_shapes {
                return Err(RunError { code: sys::MADSIM_E_LIMITS, message: "stall_census: more than max_sites distinct sites or max_shapes distinct shapes once the runner seeds are settled".into() });
            }
            for k in 0..4 {
                c.totals.n_counted[k] += more.totals.n_counted[k];
                c.totals.n_idle[k] += more.totals.n_idle[k];
            }
            c.totals.n_truncated += more.totals.n_truncated;
            c.totals.n_tasks += more.totals.n_tasks;
            c.totals.n_runner = more.totals.n_runner;
            c.totals.n_runner_listed = more.totals.n_runner_listed;
            c.totals.n_sites = sites.len() as u64;
            c.totals.n_shapes = shapes.len() as u64;
            c.sites = sites;
            c.shapes = shapes;
            c.runner_seeds = more.runner_seeds;
        }
        Ok(c)
    }

    /// Which combinations of the values of `vocabulary` (1 .. 62 distinct values) the seeds `self.seed .. self.seed + self.count` reach, by
    /// verdict (`madsim_hip_ctx_probe_sets_range`): the range run on the trace build and reduced on the device to one entry per distinct
    /// set.  `include`, `obs_cap`: as `census`; more than `max_sets` distinct sets is an error (`MADSIM_E_LIMITS`).  With `resolve_runner`
    /// set, the seeds a call leaves with a runner verdict are run again in one list call per round and merged in.
    pub fn probe_sets(&self, workload: &Workload, vocabulary: &[u64], include: u32, obs_cap: u32, max_sets: usize) -> Result<ProbeSets, RunError> {
        self.probe_sets_over(workload, vocabulary, None, include, obs_cap, max_sets)
    }

    /// `probe_sets` over an explicit, strictly ascending seed list (`madsim_hip_ctx_probe_sets_seeds`).
    pub fn probe_sets_seeds(&self, workload: &Workload, vocabulary: &[u64], seeds: &[u64], include: u32, obs_cap: u32, max_sets: usize) -> Result<ProbeSets, RunError> {
        self.probe_sets_over(workload, vocabulary, Some(seeds), include, obs_cap, max_sets)
    }

    fn probe_sets_over(&self, workload: &Workload, vocabulary: &[u64], seeds: Option<&[u64]>, include: u32, obs_cap: u32, max_sets: usize) -> Result<ProbeSets, RunError> {
        let w = workload.raw();
        let cfg = self.config.raw();
        let lim0 = self.raw_limits(true);
        let ctx = contexts()?.0[0];
        let rounds = if self.resolve_flags & sys::MADSIM_CAMPAIGN_RESOLVE == 0 {
            0
        } else {
            match (self.resolve_flags & sys::MADSIM_CAMPAIGN_RESOLVE_ROUNDS_MASK) >> sys::MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT {
                0 => sys::MADSIM_RESOLVE_DEFAULT_ROUNDS,
                r => r,
            }
        };
        let one = |lim: &sys::madsim_limits_t, list: Option<&[u64]>| -> Result<ProbeSets, RunError> {
            let n = list.map_or(self.count, |l| l.len() as u64);
            let mut sets: Vec<sys::madsim_probe_set_t> = vec![unsafe { std::mem::zeroed() }; max_sets.max(1)];
            let mut runner = vec![0u64; (n as usize).max(1)];
            let mut ps: sys::madsim_probe_sets_t = unsafe { std::mem::zeroed() };
            ps.include = include;
            ps.obs_cap = obs_cap;
            ps.vocab = vocabulary.as_ptr();
            ps.n_vocab = vocabulary.len() as u64;
            ps.sets = sets.as_mut_ptr() as *const _;                     // (the library writes through both)
            ps.cap = max_sets as u64;
            ps.runner_seeds = runner.as_mut_ptr() as *const _;
            ps.runner_cap = n;
            let rc = unsafe {
                match list {
                    Some(l) => sys::madsim_hip_ctx_probe_sets_seeds(ctx, &w, &cfg, l.as_ptr(), n, 0, lim, &mut ps),
                    None => sys::madsim_hip_ctx_probe_sets_range(ctx, &w, &cfg, self.seed, n, 0, lim, &mut ps),
                }
            };
            if rc != 0 {
                return Err(last_error(rc));
            }
            sets.truncate(ps.n_sets as usize);
            runner.truncate(ps.n_runner_listed as usize);
            ps.vocab = std::ptr::null();
            ps.sets = std::ptr::null();
            ps.runner_seeds = std::ptr::null();
            Ok(ProbeSets { vocabulary: vocabulary.to_vec(), sets, totals: ps, runner_seeds: runner })
        };
        let mut c = one(&lim0, seeds)?;
        for r in 1..=rounds {
            if c.runner_seeds.is_empty() {
                break;
            }
            let mut lim = lim0;
            let rc = unsafe { sys::madsim_hip_grow_limits(&w, &lim0, r, &mut lim) };
            if rc != 0 {
                return Err(last_error(rc));
            }
            let more = one(&lim, Some(&c.runner_seeds))?;
            let mut merged = Vec::with_capacity(c.sets.len() + more.sets.len());
            let (mut i, mut j) = (0, 0);
            while i < c.sets.len() || j < more.sets.len() {
                if j >= more.sets.len() || (i < c.sets.len() && c.sets[i].set < more.sets[j].set) {
                    merged.push(c.sets[i]);
                    i += 1;
                } else if i >= c.sets.len() || more.sets[j].set < c.sets[i].set {
                    merged.push(more.sets[j]);
                    j += 1;
                } else {
                    let (mut e, o) = (c.sets[i], more.sets[j]);
                    for k in 0..4 {
                        if o.n_seeds[k] > 0 {
                            e.first_seed[k] = if e.n_seeds[k] > 0 { e.first_seed[k].min(o.first_seed[k]) } else { o.first_seed[k] };
                        }
                        e.n_seeds[k] += o.n_seeds[k];
                    }
                    merged.push(e);
                    i += 1;
                    j += 1;
                }
            }
            if merged.len() > max_sets {
                return Err(RunError { code: sys::MADSIM_E_LIMITS, message: "probe_sets: more than max_sets distinct probe sets once the runner seeds are settled".into() });
            }
            for k in 0..4 {
                c.totals.n_counted[k] += more.totals.n_counted[k];
            }
            c.totals.n_runner = more.totals.n_runner;
            c.totals.n_runner_listed = more.totals.n_runner_listed;
            c.totals.n_sets = merged.len() as u64;
            c.sets = merged;
            c.runner_seeds = more.runner_seeds;
        }
        Ok(c)
    }

    /// Which of the values of `vocabulary` (1 .. 32 distinct values) the seeds `self.seed .. self.seed + self.count` reach first, by verdict
    /// (`madsim_hip_ctx_probe_order_range`): the range run on the trace build and reduced on the device to one entry per non-empty cell.
    /// `include`, `obs_cap`: as `census`.  With `resolve_runner` set, the seeds a call leaves with a runner verdict are run again in one list
    /// call per round and merged in.
    pub fn probe_order(&self, workload: &Workload, vocabulary: &[u64], include: u32, obs_cap: u32) -> Result<ProbeOrder, RunError> {
        self.probe_order_over(workload, vocabulary, None, include, obs_cap)
    }

    /// `probe_order` over an explicit, strictly ascending seed list (`madsim_hip_ctx_probe_order_seeds`).
    pub fn probe_order_seeds(&self, workload: &Workload, vocabulary: &[u64], seeds: &[u64], include: u32, obs_cap: u32) -> Result<ProbeOrder, RunError> {
        self.probe_order_over(workload, vocabulary, Some(seeds), include, obs_cap)
    }

    fn probe_order_over(&self, workload: &Workload, vocabulary: &[u64], seeds: Option<&[u64]>, include: u32, obs_cap: u32) -> Result<ProbeOrder, RunError> {
        let w = workload.raw();
        let cfg = self.config.raw();
        let lim0 = self.raw_limits(true);
        let ctx = contexts()?.0[0];
        let rounds = if self.resolve_flags & sys::MADSIM_CAMPAIGN_RESOLVE == 0 {
            0
        } else {
            match (self.resolve_flags & sys::MADSIM_CAMPAIGN_RESOLVE_ROUNDS_MASK) >> sys::MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT {
                0 => sys::MADSIM_RESOLVE_DEFAULT_ROUNDS,
                r => r,
            }
        };
        let cap = vocabulary.len() * vocabulary.len();
        let one = |lim: &sys::madsim_limits_t, list: Option<&[u64]>| -> Result<ProbeOrder, RunError> {
            let n = list.map_or(self.count, |l| l.len() as u64);
            let mut pairs: Vec<sys::madsim_probe_order_pair_t> = vec![unsafe { std::mem::zeroed() }; cap.max(1)];
            let mut runner = vec![0u64; (n as usize).max(1)];
            let mut po: sys::madsim_probe_order_t = unsafe { std::mem::zeroed() };
            po.include = include;
            po.obs_cap = obs_cap;
            po.vocab = vocabulary.as_ptr();
            po.n_vocab = vocabulary.len() as u64;
            po.pairs = pairs.as_mut_ptr() as *const _;                   // (the library writes through both)
            po.cap = cap as u64;
            po.runner_seeds = runner.as_mut_ptr() as *const _;
            po.runner_cap = n;
            let rc = unsafe {
                match list {
                    Some(l) => sys::madsim_hip_ctx_probe_order_seeds(ctx, &w, &cfg, l.as_ptr(), n, 0, lim, &mut po),
                    None => sys::madsim_hip_ctx_probe_order_range(ctx, &w, &cfg, self.seed, n, 0, lim, &mut po),
                }
            };
            if rc != 0 {
                return Err(last_error(rc));
            }
            pairs.truncate(po.n_pairs as usize);
            runner.truncate(po.n_runner_listed as usize);
            po.vocab = std::ptr::null();
            po.pairs = std::ptr::null();
            po.runner_seeds = std::ptr::null();
            Ok(ProbeOrder { vocabulary: vocabulary.to_vec(), pairs, totals: po, runner_seeds: runner })
        };
        let key = |e: &sys::madsim_probe_order_pair_t| (e.a as u64) << 32 | e.b as u64;
        let mut c = one(&lim0, seeds)?;
        for r in 1..=rounds {
            if c.runner_seeds.is_empty() {
                break;
            }
            let mut lim = lim0;
            let rc = unsafe { sys::madsim_hip_grow_limits(&w, &lim0, r, &mut lim) };
            if rc != 0 {
                return Err(last_error(rc));
            }
            let more = one(&lim, Some(&c.runner_seeds))?;
            let mut merged = Vec::with_capacity(c.pairs.len() + more.pairs.len());
            let (mut i, mut j) = (0, 0);
            while i < c.pairs.len() || j < more.pairs.len() {
                if j >= more.pairs.len() || (i < c.pairs.len() && key(&c.pairs[i]) < key(&more.pairs[j])) {
                    merged.push(c.pairs[i]);
                    i += 1;
                } else if i >= c.pairs.len() || key(&more.pairs[j]) < key(&c.pairs[i]) {
                    merged.push(more.pairs[j]);
                    j += 1;
                } else {
                    let (mut e, o) = (c.pairs[i], more.pairs[j]);
                    for k in 0..4 {
                        if o.n_seeds[k] > 0 {
                            e.first_seed[k] = if e.n_seeds[k] > 0 { e.first_seed[k].min(o.first_seed[k]) } else { o.first_seed[k] };
                        }
                        e.n_seeds[k] += o.n_seeds[k];
                    }
                    merged.push(e);
                    i += 1;
                    j += 1;
                }
            }
            for k in 0..4 {
                c.totals.n_counted[k] += more.totals.n_counted[k];
                c.totals.n_none[k] += more.totals.n_none[k];
            }
            c.totals.n_truncated += more.totals.n_truncated;
            c.totals.n_runner = more.totals.n_runner;
            c.totals.n_runner_listed = more.totals.n_runner_listed;
            c.totals.n_pairs = merged.len() as u64;
            c.pairs = merged;
            c.runner_seeds = more.runner_seeds;
        }
        Ok(c)
    }

    /// What one seed traced, and its result: the values in execution order (at most 65 536 of them).  A failing `run_workload` names
    /// its seed in the reproduction note; `Builder { seed, ..b }.observe_seed(&w, seed)` prints what that seed's test body traced.
    pub fn observe_seed(&self, workload: &Workload, seed: u64) -> Result<(Vec<u64>, sys::madsim_result_t), RunError> {
        let t = self.trace_seeds(workload, &[seed], 1 << 16, 0)?.remove(0);
        Ok((t.observations, t.result))
    }

    /// Seed search: seeds `self.seed .. self.seed + self.count` as batches the LIBRARY keeps in flight on its own streams
    /// (`madsim_hip_run_campaign`), stopping at the first batch that holds a failing seed.  Returns the campaign report — the
    /// smallest failing seed, how many seeds were searched — without per-seed results: re-run the reported seed for details
    /// (`MADSIM_TEST_SEED=<seed>`).  This is the "first failing seed per hour" use of `MADSIM_TEST_NUM` at its full rate: one
    /// 65 536-seed batch alone leaves two thirds of the GPU's issue slots idle.
    pub fn search_first_failure(&self, workload: &Workload) -> Result<sys::madsim_campaign_t, RunError> {
        let w = workload.raw();
        let cfg = self.config.raw();
        let lim = self.raw_limits(true);
        let ctx = contexts()?.0[0];
        let mut rep: sys::madsim_campaign_t = unsafe { std::mem::zeroed() };
        let rc = unsafe {
            sys::madsim_hip_ctx_run_campaign(ctx, &w, &cfg, self.seed, self.count, 0, 0, sys::MADSIM_CAMPAIGN_STOP_AT_FAILURE, &lim, &mut rep)
        };
        if rc != 0 {
            return Err(last_error(rc));
        }
        if rep.first_failing_seed != u64::MAX {
            note_seed(rep.first_failing_seed);
        }
        Ok(rep)
    }

    /// Triage: WHICH seeds of `self.seed .. self.seed + self.count` fail, and how (`madsim_hip_run_campaign_collect`).  The whole
    /// range runs at the campaign's rate; the `max_failures` smallest failing seeds come back in ascending order, each with the
    /// result `madsim_hip_run_batch` gives for it, beside the number of seeds per verdict value (index = `MADSIM_PASS` ..
    /// `MADSIM_INTERNAL`) and the campaign report.  Never panics: hand `failures[0].seed` to `run_workload` for the reference's
    /// behaviour.
    pub fn search_failures(&self, workload: &Workload, max_failures: usize) -> Result<Failures, RunError> {
        let w = workload.raw();
        let cfg = self.config.raw();
        let lim = self.raw_limits(true);
        let ctx = contexts()?.0[0];
        let mut failures: Vec<sys::madsim_failure_t> = vec![unsafe { std::mem::zeroed() }; max_failures];
        let mut campaign: sys::madsim_campaign_t = unsafe { std::mem::zeroed() };
        let mut col = sys::madsim_collect_t {
            failures: if max_failures > 0 { failures.as_mut_ptr() as *const _ } else { std::ptr::null() },   // (the library writes through it)
            cap: max_failures as u64,
            n_listed: 0,
            n_by_verdict: [0; 8],
        };
        let rc = unsafe { sys::madsim_hip_ctx_run_campaign_collect(ctx, &w, &cfg, self.seed, self.count, 0, 0, self.resolve_flags, &lim, &mut campaign, &mut col) };
        if rc != 0 {
            return Err(last_error(rc));
        }
        failures.truncate(col.n_listed as usize);
        Ok(Failures { failures, by_verdict: col.n_by_verdict, campaign })
    }

    /// Statistics: HOW the runs of `self.seed .. self.seed + self.count` are distributed, and which seeds are the outliers
    /// (`madsim_hip_run_campaign_stats`).  `include`: bit `v` set = count the seeds whose verdict is `v` (bits 0-3: `MADSIM_PASS` ..
    /// `MADSIM_TIME_LIMIT`); `top_k` <= `MADSIM_STAT_MAX_TOP` extreme seeds per metric.
    pub fn campaign_stats(&self, workload: &Workload, include: u32, top_k: u32) -> Result<Stats, RunError> {
        let w = workload.raw();
        let cfg = self.config.raw();
        let lim = self.raw_limits(true);
        let ctx = contexts()?.0[0];
        let k = top_k as usize;
        let mut top: Vec<sys::madsim_extreme_t> = vec![unsafe { std::mem::zeroed() }; 4 * k];
        let mut campaign: sys::madsim_campaign_t = unsafe { std::mem::zeroed() };
        let mut stats: sys::madsim_stats_t = unsafe { std::mem::zeroed() };
        stats.include = include;
        stats.top_k = top_k;
        stats.top = if k > 0 { top.as_mut_ptr() as *const _ } else { std::ptr::null() };   // (the library writes through it)
        let rc = unsafe {
            sys::madsim_hip_ctx_run_campaign_stats(ctx, &w, &cfg, self.seed, self.count, 0, 0, self.resolve_flags, &lim, &mut campaign, std::ptr::null_mut(), &mut stats)
        };
        if rc != 0 {
            return Err(last_error(rc));
        }
        stats.top = std::ptr::null();
        let n_top = stats.n_top as usize;
        let rows: [Vec<sys::madsim_extreme_t>; 4] = std::array::from_fn(|m| top[m * k..m * k + n_top].to_vec());
        Ok(Stats { stats, top: rows, campaign })
    }

    /// Failure modes: HOW MANY DIFFERENT failures `self.seed .. self.seed + self.count` holds (`madsim_hip_run_campaign_groups`).
    /// The seeds whose verdict bit is set in `include` (bits 0-3) are grouped by (verdict, key), `key_field` one of
    /// `MADSIM_GROUP_KEY_*` (`MADSIM_GROUP_KEY_OBS`: `obs_hash`, what the test body traced); the first `max_groups` groups in order
    /// of first appearance come back, each with its exact count over the range and its smallest seed — the one to replay.
    pub fn failure_groups(&self, workload: &Workload, max_groups: usize, include: u32, key_field: u32) -> Result<Groups, RunError> {
        let w = workload.raw();
        let cfg = self.config.raw();
        let lim = self.raw_limits(true);
        let ctx = contexts()?.0[0];
        let mut groups: Vec<sys::madsim_group_t> = vec![unsafe { std::mem::zeroed() }; max_groups];
        let mut campaign: sys::madsim_campaign_t = unsafe { std::mem::zeroed() };
        let mut grp = sys::madsim_groups_t {
            include,
            key_field,
            groups: if max_groups > 0 { groups.as_mut_ptr() as *const _ } else { std::ptr::null() },   // (the library writes through it)
            cap: max_groups as u64,
            n_groups: 0,
            n_grouped: 0,
            n_ungrouped: 0,
        };
        let rc = unsafe {
            sys::madsim_hip_ctx_run_campaign_groups(ctx, &w, &cfg, self.seed, self.count, 0, 0, self.resolve_flags, &lim, &mut campaign, std::ptr::null_mut(),
                                                    std::ptr::null_mut(), &mut grp)
        };
        if rc != 0 {
            return Err(last_error(rc));
        }
        groups.truncate(grp.n_groups as usize);
        Ok(Groups { groups, n_grouped: grp.n_grouped, n_ungrouped: grp.n_ungrouped, campaign })
    }

    /// Fix check: `self` running `workload` (side A) against `other` running `other_workload` (side B) over `self.seed .. self.seed +
    /// self.count` (`madsim_hip_run_campaign_diff`).  Both sides run at the campaign's rate and are compared on the device on the result
    /// fields named in `fields` (`MADSIM_DIFF_*`); config and limits are each side's own.  The `max_listed` smallest differing seeds come
    /// back with both results, with the counts and the verdict-transition matrix.
    pub fn diff_campaign(&self, workload: &Workload, other: &Builder, other_workload: &Workload, fields: u32, max_listed: usize) -> Result<Diff, RunError> {
        let (wa, wb) = (workload.raw(), other_workload.raw());
        let (ca, cb) = (self.config.raw(), other.config.raw());
        let (la, lb) = (self.raw_limits(true), other.raw_limits(true));
        let ctx = contexts()?.0[0];
        let mut records: Vec<sys::madsim_diff_record_t> = vec![unsafe { std::mem::zeroed() }; max_listed];
        let mut a: sys::madsim_campaign_t = unsafe { std::mem::zeroed() };
        let mut b: sys::madsim_campaign_t = unsafe { std::mem::zeroed() };
        let mut report: sys::madsim_diff_t = unsafe { std::mem::zeroed() };
        report.fields = fields;
        report.records = if max_listed > 0 { records.as_mut_ptr() as *const _ } else { std::ptr::null() };   // (the library writes through it)
        report.cap = max_listed as u64;
        let rc = unsafe {
            sys::madsim_hip_ctx_run_campaign_diff(ctx, &wa, &ca, &la, &wb, &cb, &lb, self.seed, self.count, 0, 0, self.resolve_flags, &mut a, &mut b, &mut report)
        };
        if rc != 0 {
            return Err(last_error(rc));
        }
        records.truncate(report.n_listed as usize);
        report.records = std::ptr::null();
        Ok(Diff { records, report, a, b })
    }

    /// The list campaign: `search_failures`, `campaign_stats` and `failure_groups` in one call over the seeds you NAME instead of
    /// `self.seed .. self.seed + self.count` (`madsim_hip_run_seeds_campaign`) — the failing seeds an earlier campaign listed, a
    /// regression corpus, the members of one failure mode.  `seeds` must ascend strictly (sorted, no duplicates: `sort_unstable` +
    /// `dedup`), so that "smallest seed" and "first position" stay one thing; the library refuses any other list, it never sorts
    /// silently.  Position `i` of the list takes the role of `seed + i`: `campaign.seeds_run` counts positions.
    /// `max_failures`: `Some(k)` = list the `k` smallest failing seeds (and count the verdicts); `stats`: `Some((include, top_k))`;
    /// `groups`: `Some((include, key_field, max_groups))`.  A part that is not asked for comes back `None`.
    /// (Like the rest of this crate: written against the header, never compiled — there is no Rust toolchain where it is developed.)
    pub fn campaign_over_seeds(&self, workload: &Workload, seeds: &[u64], max_failures: Option<usize>, stats: Option<(u32, u32)>,
                               groups: Option<(u32, u32, usize)>) -> Result<ListCampaign, RunError> {
        let w = workload.raw();
        let cfg = self.config.raw();
        let lim = self.raw_limits(true);
        let ctx = contexts()?.0[0];
        let mut campaign: sys::madsim_campaign_t = unsafe { std::mem::zeroed() };
        let cap = max_failures.unwrap_or(0);
        let mut failures: Vec<sys::madsim_failure_t> = vec![unsafe { std::mem::zeroed() }; cap];
        let mut col = sys::madsim_collect_t {
            failures: if cap > 0 { failures.as_mut_ptr() as *const _ } else { std::ptr::null() },   // (the library writes through it)
            cap: cap as u64,
            n_listed: 0,
            n_by_verdict: [0; 8],
        };
        let (include, top_k) = stats.unwrap_or((0, 0));
        let k = top_k as usize;
        let mut top: Vec<sys::madsim_extreme_t> = vec![unsafe { std::mem::zeroed() }; 4 * k];
        let mut st: sys::madsim_stats_t = unsafe { std::mem::zeroed() };
        st.include = include;
        st.top_k = top_k;
        st.top = if k > 0 { top.as_mut_ptr() as *const _ } else { std::ptr::null() };
        let (g_include, key_field, max_groups) = groups.unwrap_or((0, 0, 0));
        let mut entries: Vec<sys::madsim_group_t> = vec![unsafe { std::mem::zeroed() }; max_groups];
        let mut grp = sys::madsim_groups_t {
            include: g_include,
            key_field,
            groups: if max_groups > 0 { entries.as_mut_ptr() as *const _ } else { std::ptr::null() },
            cap: max_groups as u64,
            n_groups: 0,
            n_grouped: 0,
            n_ungrouped: 0,
        };
        let rc = unsafe {
            sys::madsim_hip_ctx_run_seeds_campaign(ctx, &w, &cfg, seeds.as_ptr(), seeds.len() as u64, 0, 0, self.resolve_flags, &lim, &mut campaign,
                                                   if max_failures.is_some() { &mut col } else { std::ptr::null_mut() },
                                                   if stats.is_some() { &mut st } else { std::ptr::null_mut() },
                                                   if groups.is_some() { &mut grp } else { std::ptr::null_mut() })
        };
        if rc != 0 {
            return Err(last_error(rc));
        }
        failures.truncate(col.n_listed as usize);
        st.top = std::ptr::null();
        let n_top = st.n_top as usize;
        let rows: [Vec<sys::madsim_extreme_t>; 4] = std::array::from_fn(|m| top[m * k..m * k + n_top].to_vec());
        entries.truncate(grp.n_groups as usize);
        Ok(ListCampaign {
            failures: max_failures.map(|_| Failures { failures, by_verdict: col.n_by_verdict, campaign }),
            stats: stats.map(|_| Stats { stats: st, top: rows, campaign }),
            groups: groups.map(|_| Groups { groups: entries, n_grouped: grp.n_grouped, n_ungrouped: grp.n_ungrouped, campaign }),
            campaign,
        })
    }

    /// `diff_campaign` over the seeds you name (`madsim_hip_run_seeds_campaign_diff`): "did the fix fix all of them?" over exactly the
    /// seeds that failed.  `seeds` as `campaign_over_seeds`': strictly ascending.
    pub fn diff_campaign_seeds(&self, workload: &Workload, other: &Builder, other_workload: &Workload, seeds: &[u64], fields: u32,
                               max_listed: usize) -> Result<Diff, RunError> {
        let (wa, wb) = (workload.raw(), other_workload.raw());
        let (ca, cb) = (self.config.raw(), other.config.raw());
        let (la, lb) = (self.raw_limits(true), other.raw_limits(true));
        let ctx = contexts()?.0[0];
        let mut records: Vec<sys::madsim_diff_record_t> = vec![unsafe { std::mem::zeroed() }; max_listed];
        let mut a: sys::madsim_campaign_t = unsafe { std::mem::zeroed() };
        let mut b: sys::madsim_campaign_t = unsafe { std::mem::zeroed() };
        let mut report: sys::madsim_diff_t = unsafe { std::mem::zeroed() };
        report.fields = fields;
        report.records = if max_listed > 0 { records.as_mut_ptr() as *const _ } else { std::ptr::null() };   // (the library writes through it)
        report.cap = max_listed as u64;
        let rc = unsafe {
            sys::madsim_hip_ctx_run_seeds_campaign_diff(ctx, &wa, &ca, &la, &wb, &cb, &lb, seeds.as_ptr(), seeds.len() as u64, 0, 0, self.resolve_flags,
                                                        &mut a, &mut b, &mut report)
        };
        if rc != 0 {
            return Err(last_error(rc));
        }
        records.truncate(report.n_listed as usize);
        report.records = std::ptr::null();
        Ok(Diff { records, report, a, b })
    }

    /// What a change did to each seed's numbers: `self` running `workload` (side A) against `other` running `other_workload` (side B) over
    /// `self.seed .. self.seed + self.count` (`madsim_hip_run_paired_campaign`).  A seed is paired when its verdict on side A is named in
    /// `include` and on side B in `other_include` (bits 0-3); per metric and direction the device reduces count, min, max, the exact sum,
    /// a histogram and the `top_k` (<= 16) extreme seeds of the unsigned magnitude `|b - a|`.  Config and limits are each side's own; the
    /// seeds and the resolve rounds are `self`'s.
    pub fn paired_campaign(&self, workload: &Workload, other: &Builder, other_workload: &Workload, include: u32, other_include: u32, top_k: u32)
                           -> Result<Paired, RunError> {
        self.paired_impl(workload, other, other_workload, None, include, other_include, top_k)
    }

    /// `paired_campaign` over the seeds you name (`madsim_hip_run_seeds_campaign_paired`).  `seeds` as `campaign_over_seeds`': strictly
    /// ascending.
    pub fn paired_campaign_seeds(&self, workload: &Workload, other: &Builder, other_workload: &Workload, seeds: &[u64], include: u32,
                                 other_include: u32, top_k: u32) -> Result<Paired, RunError> {
        self.paired_impl(workload, other, other_workload, Some(seeds), include, other_include, top_k)
    }

    fn paired_impl(&self, workload: &Workload, other: &Builder, other_workload: &Workload, seeds: Option<&[u64]>, include: u32, other_include: u32,
                   top_k: u32) -> Result<Paired, RunError> {
        let (wa, wb) = (workload.raw(), other_workload.raw());
        let (ca, cb) = (self.config.raw(), other.config.raw());
        let (la, lb) = (self.raw_limits(true), other.raw_limits(true));
        let ctx = contexts()?.0[0];
        let k = top_k as usize;
        let mut top: Vec<sys::madsim_paired_extreme_t> = vec![unsafe { std::mem::zeroed() }; 8 * k];
        let mut a: sys::madsim_campaign_t = unsafe { std::mem::zeroed() };
        let mut b: sys::madsim_campaign_t = unsafe { std::mem::zeroed() };
        let mut report: sys::madsim_paired_t = unsafe { std::mem::zeroed() };
        report.include_a = include;
        report.include_b = other_include;
        report.top_k = top_k;
        report.top = if k > 0 { top.as_mut_ptr() as *const _ } else { std::ptr::null() };   // (the library writes through it)
        let rc = unsafe {
            match seeds {
                None => sys::madsim_hip_ctx_run_paired_campaign(ctx, &wa, &ca, &la, &wb, &cb, &lb, self.seed, self.count, 0, 0, self.resolve_flags, &mut a,
                                                                &mut b, std::ptr::null_mut(), &mut report),
                Some(s) => sys::madsim_hip_ctx_run_seeds_campaign_paired(ctx, &wa, &ca, &la, &wb, &cb, &lb, s.as_ptr(), s.len() as u64, 0, 0,
                                                                         self.resolve_flags, &mut a, &mut b, std::ptr::null_mut(), &mut report),
            }
        };
        if rc != 0 {
            return Err(last_error(rc));
        }
        report.top = std::ptr::null();
        let rows: [Vec<sys::madsim_paired_extreme_t>; 8] = std::array::from_fn(|j| top[j * k..j * k + report.n_top[j] as usize].to_vec());
        Ok(Paired { report, top: rows, a, b })
    }

    /// Across several variants: up to eight `(builder, workload)` pairs over `self.seed .. self.seed + self.count` — or, with
    /// `seeds: Some(list)`, over a strictly ascending list — in one campaign (`madsim_hip_run_sweep_campaign`): a parameter sweep, a stack
    /// of versions of a test body.  Config and limits are each variant's own; the seeds and the resolve rounds are `self`'s.  Every seed is
    /// classified across all variants on the device; `fields`: the `MADSIM_DIFF_*` fields compared against variant 0 (0 = none);
    /// `list_rule`: `MADSIM_SWEEP_LIST_*`; the `max_listed` smallest selected seeds come back.
    pub fn sweep_campaign(&self, variants: &[(&Builder, &Workload)], seeds: Option<&[u64]>, fields: u32, list_rule: u32, max_listed: usize)
                          -> Result<Sweep, RunError> {
        let n = variants.len();
        let ws: Vec<sys::madsim_workload_t> = variants.iter().map(|(_, w)| w.raw()).collect();
        let cs: Vec<sys::madsim_config_t> = variants.iter().map(|(b, _)| b.config.raw()).collect();
        let ls: Vec<sys::madsim_limits_t> = variants.iter().map(|(b, _)| b.raw_limits(true)).collect();
        let mut campaigns: Vec<sys::madsim_campaign_t> = vec![unsafe { std::mem::zeroed() }; n];
        let outs = campaigns.as_mut_ptr();
        let var: Vec<sys::madsim_sweep_variant_t> = (0..n)
            .map(|v| sys::madsim_sweep_variant_t { w: &ws[v], cfg: &cs[v], lim: &ls[v], out: unsafe { outs.add(v) } as *const _ })   // (the library writes through it)
            .collect();
        let ctx = contexts()?.0[0];
        let mut records: Vec<sys::madsim_sweep_record_t> = vec![unsafe { std::mem::zeroed() }; max_listed];
        let mut report: sys::madsim_sweep_t = unsafe { std::mem::zeroed() };
        report.fields = fields;
        report.list_rule = list_rule;
        report.records = if max_listed > 0 { records.as_mut_ptr() as *const _ } else { std::ptr::null() };   // (the library writes through it)
        report.cap = max_listed as u64;
        let none = [0u64];                                                // (an empty list is still the list form: a non-null pointer)
        let (seed0, total, list) = match seeds {
            Some(s) => (0, s.len() as u64, if s.is_empty() { none.as_ptr() } else { s.as_ptr() }),
            None => (self.seed, self.count, std::ptr::null()),
        };
        let rc = unsafe { sys::madsim_hip_ctx_run_sweep_campaign(ctx, var.as_ptr(), n as u32, seed0, total, list, 0, 0, self.resolve_flags, &mut report) };
        if rc != 0 {
            return Err(last_error(rc));
        }
        records.truncate(report.n_listed as usize);
        report.records = std::ptr::null();
        Ok(Sweep { records, report, campaigns })
    }

    /// Same contract as `Builder::run` (builder.rs:121-162) for a test body registered as a workload: returns the per-seed
    /// results when every seed passes, panics (after the reproduction note) on the smallest failing seed.  Library errors
    /// and runner limits that survive the re-runs come back as `Err`, never as a test failure.
    pub fn run_workload(&self, workload: &Workload) -> Result<Vec<sys::madsim_result_t>, RunError> {
        let w = workload.raw();
        let cfg = self.config.raw();
        if self.check {
            // Runtime::check_determinism (runtime/mod.rs:178-202): run the seed twice, compare the RNG log; no time limit there
            let lim = self.raw_limits(false);
            let (l1, r1) = self.trace(&w, &cfg, &lim)?;
            if r1.verdict >= sys::MADSIM_OVERFLOW {
                return Err(RunError { code: sys::MADSIM_E_LIMITS, message: format!("seed {}: {}", self.seed, verdict_message(r1.verdict)) });
            }
            let (l2, r2) = self.trace(&w, &cfg, &lim)?;
            if l1 != l2 || r1.trace_hash != r2.trace_hash || r1.obs_hash != r2.obs_hash {
                note_seed(self.seed);
                panic!("non-determinism detected");
            }
            if r1.verdict != sys::MADSIM_PASS {
                note_seed(self.seed);
                panic!("{}", verdict_message(r1.verdict));
            }
            return Ok(vec![r1]);
        }
        let lim = self.raw_limits(true);
        let ctxs = contexts()?;
        let mut out: Vec<sys::madsim_result_t> = vec![unsafe { std::mem::zeroed() }; self.count as usize];
        let mut summary: sys::madsim_summary_t = unsafe { std::mem::zeroed() };
        // Builder::run drives every seed from this process (builder.rs:129-150): the batch is sharded over all GPUs from this
        // thread; seeds that outgrow a device capacity or the step cap are re-run inside, compacted into one launch per round.
        let rc = unsafe {
            sys::madsim_hip_run_batch_multi(ctxs.0.as_ptr(), ctxs.0.len() as c_int, &w, &cfg, self.seed, self.count, &lim,
                                            out.as_mut_ptr(), &mut summary, 6)
        };
        if rc != 0 {
            return Err(last_error(rc));
        }
        if summary.n_failed > 0 {
            let runner = |v: u32| v >= sys::MADSIM_OVERFLOW;
            // a genuine test failure wins over unresolved runner limits: its seed and repro note are never hidden
            if let Some(i) = out.iter().position(|r| r.verdict != sys::MADSIM_PASS && !runner(r.verdict)) {
                note_seed(self.seed + i as u64);
                panic!("{}", verdict_message(out[i].verdict));
            }
            let i = out.iter().position(|r| runner(r.verdict)).unwrap();
            return Err(RunError {
                code: sys::MADSIM_E_LIMITS,
                message: format!("seed {}: {} persists after re-runs with larger limits", self.seed + i as u64, verdict_message(out[i].verdict)),
            });
        }
        Ok(out)
    }
}
