// madsim_hip.cpp — host side of libmadsim_hip.so: the C-ABI entry points of include/madsim_hip.h.
//
// Replaces the seed fan-out of madsim::runtime::Builder::run (madsim/src/sim/runtime/builder.rs:121-162):
// where the reference spawns one OS thread per seed, this picks an LDS geometry for the workload,
// launches the gfx950 executor kernel (sim_kernel.hip) with one lane per seed, and reduces the
// per-seed verdicts to "first failing seed" on the device.  No CPU execution path exists here: when
// HIP is unavailable every entry point returns MADSIM_E_HIP / MADSIM_E_NOINIT.
//
// State lives in per-device contexts (madsim_hip_ctx_t): a process may hold one context per GPU and drive them all from
// one host thread (madsim_hip_run_batch_multi), which is what a `cargo test` process on an 8-GPU node needs.  The v1
// entry points (madsim_hip_init / madsim_hip_run_batch ...) are wrappers on a process-default context.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <cstdlib>
#include <string>
#include <unordered_map>
#include <vector>

#include "sim_kernel.h"
#include "geometry.h"
#include "device_mem.h"

using madsim_k::KParams;
using madsim_geo::Geo;

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return fail(MADSIM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));    \
    } while (0)

uint64_t fnv(const void* p, size_t n, uint64_t h) {
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

// VGPRs of a kernel build, asked of the loaded code object once per build and process (same on every device of a node).
int variant_vgprs_cached(const madsim_k::VariantSel* v) {
    static std::mutex mu;
    static std::unordered_map<uint32_t, int> cache;
    const uint32_t key = (uint32_t)v->trace | (uint32_t)v->spill << 1 | (uint32_t)v->rq << 2 | (uint32_t)v->g << 3 | (uint32_t)(v->lws & 0xf) << 4 | (uint32_t)v->feat << 8;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int r = madsim_k_variant_vgprs(v);
    cache[key] = r;
    return r;
}

double since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

using madsim_mem::DevBuf;
using madsim_mem::PinnedBuf;
using madsim_mem::Event;
using madsim_mem::Stream;
typedef unsigned long long report_word_t;

// Everything a context owns on its device, each member an owning type of device_mem.h: madsim_hip_ctx::close() releases all of it by
// assigning a fresh one, with the device bound.
struct madsim_hip_resources {
    // Device copies of workload tables.  Looked up by content hash, confirmed by comparing the host bytes kept beside
    // them; entries are immutable once uploaded, so launches still in flight on other streams keep valid pointers when a
    // different workload comes along.
    struct Tables {
        uint64_t hash = 0;
        std::vector<uint32_t> host;      // insns | progs | socks | durs (as 32-bit words) | n_insns
        DevBuf<uint32_t> insns, progs, socks, nodes; DevBuf<uint64_t> durs;      // (insns: four words an instruction, read as uint4)
        DevBuf<uint32_t> iter_est;       // ITER_KEYS words: how many passes a wave of this workload runs, one per launch shape (limits, seeds per lane:
                                         // upload_workload picks the word; written by finishing waves, k_main.h)
    };
    static constexpr uint32_t ITER_KEYS = 16;
    std::vector<Tables> tables;
    // per-stream scratch: launches on one stream run in order, launches on different streams may overlap and must
    // not share the timer-heap spill region or the work-queue counter
    struct Scratch { DevBuf<uint8_t> spill, gstate; DevBuf<unsigned long long> work_ctr; };
    std::unordered_map<hipStream_t, Scratch> scratch;
    // madsim_hip_ctx_run_campaign: batches in flight on the context's own streams
    static constexpr int CAMPAIGN_MAX = 8;
    static constexpr size_t STATS_REP_WORDS = 16 + MADSIM_K_STATS_WORDS;      // a statistics campaign's report: the plain / collecting report's words in front
    static constexpr size_t GROUP_REP_WORDS = STATS_REP_WORDS + MADSIM_K_GROUP_WORDS;
    // The multi-variant forms (differential, paired, sweep) share one word layout: summary6's six words of variant v at 8 v, the form's words at
    // VARIANT_FORM_AT — the diff words, then the paired words with the top records at their end; or the sweep words.
    static constexpr size_t VARIANT_FORM_AT = 8 * MADSIM_SWEEP_MAX_VARIANTS;
    static constexpr size_t DIFF_REP_WORDS = VARIANT_FORM_AT + MADSIM_K_DIFF_WORDS;
    static constexpr size_t PAIRED_REP_WORDS = DIFF_REP_WORDS + MADSIM_K_PAIRED_WORDS;
    static constexpr size_t SWEEP_REP_WORDS = VARIANT_FORM_AT + MADSIM_K_SWEEP_WORDS;
    static constexpr size_t VARIANT_REP_WORDS = PAIRED_REP_WORDS > SWEEP_REP_WORDS ? PAIRED_REP_WORDS : SWEEP_REP_WORDS;
    // One batch in flight: what every form uses, then one group per campaign form, made when a call of that form first comes (ensure)
    // and kept with the flight.  Every resource is ensured on its own — none stands for another —, so a call that ran out of memory
    // half-way leaves nothing that a later call would take for complete.
    struct Flight {
        Stream stream; Event e0, e1, done;
        // the batch's report words (device, page-locked host): 16 report words (summary6's or collect's), then the statistics words, then the
        // grouping words — sized once for all of them; run_pipelined and the plain campaign use the first six
        DevBuf<report_word_t> d_rep; PinnedBuf<report_word_t> h_rep;
        DevBuf<madsim_result_t> d_out; PinnedBuf<madsim_result_t> h_out;      // h_out: page-locked staging of run_pipelined
        int ensure(uint64_t batch, bool staging) {
            HIP_TRY(stream.ensure());
            HIP_TRY(d_rep.room(GROUP_REP_WORDS));
            HIP_TRY(h_rep.room(GROUP_REP_WORDS));
            HIP_TRY(e0.ensure()); HIP_TRY(e1.ensure()); HIP_TRY(done.ensure());
            HIP_TRY(d_out.room(batch, stream));
            if (staging) HIP_TRY(h_out.room(batch, stream));
            return 0;
        }
        // collecting campaigns: per-wave counts, the batch's failure records
        struct Collect {
            DevBuf<uint32_t> wcnt; DevBuf<madsim_failure_t> rec;
            int ensure(uint64_t records, hipStream_t s) {
                HIP_TRY(wcnt.room(MADSIM_K_COLLECT_WAVES));
                HIP_TRY(rec.room(records, s));
                return 0;
            }
        } collect;
        // statistics campaigns: the candidate words
        struct Stats {
            DevBuf<unsigned long long> cand;
            int ensure() { HIP_TRY(cand.room(MADSIM_K_STATS_CAND_WORDS)); return 0; }
        } stats;
        // grouping campaigns: the keyed table (zero between batches: dirty = a batch was queued and never harvested), the list of claimed
        // slots and the batch's entries, sized for batches of `cap` seeds
        struct Groups {
            DevBuf<uint32_t> tab, list; DevBuf<madsim_group_t> ent; size_t cap = 0; bool dirty = false;
            int ensure(uint64_t batch, hipStream_t s) {
                if (batch > cap) {
                    dirty = true; cap = 0;           // (cap counts only once all three have room)
                    HIP_TRY(tab.room(madsim_k_group_slots(batch) * MADSIM_K_GROUP_SLOT_BYTES / sizeof(uint32_t), s));
                    HIP_TRY(list.room(batch, s));
                    HIP_TRY(ent.room(batch, s));
                    cap = batch;
                }
                if (dirty) {                         // a new table, or one that an error left between a batch's two passes: the only time it is cleared whole
                    HIP_TRY(hipMemsetAsync(tab, 0, madsim_k_group_slots(cap) * MADSIM_K_GROUP_SLOT_BYTES, s));
                    HIP_TRY(hipStreamSynchronize(s));
                    dirty = false;
                }
                return 0;
            }
        } groups;
        // the multi-variant forms: the results of variants 1 .. 7 (variant 0 uses d_out), made only up to the number of variants a call
        // needs, an event pair per variant, the report words — VARIANT_REP_WORDS live ones (device, page-locked host) and behind the
        // device's their state before a batch, the same for every form, from which one device copy prepares them
        struct Variants {
            DevBuf<madsim_result_t> out[MADSIM_SWEEP_MAX_VARIANTS - 1]; Event v0[MADSIM_SWEEP_MAX_VARIANTS], v1[MADSIM_SWEEP_MAX_VARIANTS];
            DevBuf<report_word_t> d_rep; PinnedBuf<report_word_t> h_rep;
            int ensure(uint32_t n_variants, uint64_t batch, hipStream_t s) {
                if (!d_rep) {
                    std::vector<report_word_t> init(VARIANT_REP_WORDS, 0);          // the words before a batch: every summary6's two minima all-ones, the rest zero
                    for (uint32_t v = 0; v < MADSIM_SWEEP_MAX_VARIANTS; v++) init[8 * v] = init[8 * v + 4] = ~0ull;
                    HIP_TRY(d_rep.room(2 * VARIANT_REP_WORDS));
                    const hipError_t e = hipMemcpy(d_rep + VARIANT_REP_WORDS, init.data(), VARIANT_REP_WORDS * sizeof(report_word_t), hipMemcpyHostToDevice);
                    if (e != hipSuccess) {                                          // (words without their initial state are no words)
                        d_rep.reset();
                        return fail(MADSIM_E_HIP, std::string("hipMemcpy(initial report words): ") + hipGetErrorString(e));
                    }
                }
                HIP_TRY(h_rep.room(VARIANT_REP_WORDS));
                for (uint32_t v = 0; v < n_variants; v++) {
                    HIP_TRY(v0[v].ensure()); HIP_TRY(v1[v].ensure());
                    if (v) HIP_TRY(out[v - 1].room(batch, s));
                }
                return 0;
            }
        } variants;
        // what each of them adds: per-wave counts and the batch's records (differential, sweep), the candidate words of the top-K (paired)
        struct Diff {
            DevBuf<uint32_t> wcnt; DevBuf<madsim_diff_record_t> rec;
            int ensure(uint64_t records, hipStream_t s) { HIP_TRY(wcnt.room(MADSIM_K_COLLECT_WAVES)); HIP_TRY(rec.room(records, s)); return 0; }
        } diff;
        struct Paired {
            DevBuf<unsigned long long> cand;
            int ensure() { HIP_TRY(cand.room(MADSIM_K_PAIRED_CAND_WORDS)); return 0; }
        } paired;
        struct Sweep {
            DevBuf<uint32_t> wcnt; DevBuf<madsim_sweep_record_t> rec;
            int ensure(uint64_t records, hipStream_t s) { HIP_TRY(wcnt.room(MADSIM_K_COLLECT_WAVES)); HIP_TRY(rec.room(records, s)); return 0; }
        } sweep;
        // resolving campaigns, made when a batch first needs a round (most campaigns never do), enlarged — with the flight's stream drained —
        // when a later call brings larger batches: the seed list, the index list and the re-run results of `want` seeds (60 B per seed), the
        // list kernels' wave counts with the count word behind them (device) and that word's page-locked host copy, the re-run kernel's event pair
        struct Resolve {
            DevBuf<uint64_t> seeds; DevBuf<uint32_t> idx; DevBuf<madsim_result_t> rerun;
            DevBuf<uint32_t> cnt; PinnedBuf<uint32_t> h_cnt; Event r0, r1;
            int ensure(size_t want, hipStream_t s) {
                HIP_TRY(cnt.room(MADSIM_K_RESOLVE_WAVES + 1));
                HIP_TRY(h_cnt.room(1));
                HIP_TRY(r0.ensure()); HIP_TRY(r1.ensure());
                HIP_TRY(seeds.room(want, s));
                HIP_TRY(idx.room(want, s));
                HIP_TRY(rerun.room(want, s));
                return 0;
            }
        } resolve;
        // list campaigns: the batch's slice of the caller's seed list (device) and its page-locked staging copy — 8 bytes per seed of a batch
        // each, proportional to batch x flights, never to the length of the list.  Not resolve.seeds: a resolving list campaign reads this
        // one while it writes that one.
        struct List {
            DevBuf<uint64_t> d; PinnedBuf<uint64_t> h;
            int ensure(uint64_t batch, hipStream_t s) {
                HIP_TRY(d.room(batch, s));
                HIP_TRY(h.room(batch, s));
                return 0;
            }
        } list;
    };
    Flight flights[CAMPAIGN_MAX];
    DevBuf<unsigned long long> d_acc;         // 4 x u64 summary accumulators
    DevBuf<uint64_t> d_seeds;                 // seed list of a compacted re-run
    // One side's buffers of a trace launch: the rows of the determinism log (bytes) and of the observation log (words), the length words
    // and the results.  Set 0 is what every trace call uses, set 1 side B of a divergence report; set 0's `out` is also the result
    // buffer of run_host and run_list.
    struct TraceSet { DevBuf<uint8_t> log; DevBuf<uint64_t> obs, len; DevBuf<madsim_result_t> out; DevBuf<uint64_t> task, task_len; };      // (task, task_len: the task log, only where a call asks for it; obs: with the time log its rows too, n * obs_cap words behind the observation rows)
    TraceSet trace[2];
    DevBuf<madsim_divergence_t> d_drec; DevBuf<uint64_t> d_dctx;      // divergence reports: the records and the context rows
    // One census form's buffers (the observation census, the probe-set census, the probe-order census: each its own, the slots differ in size): the table (all zero
    // between chunks; `dirty` when it is new or an error may have left it otherwise), the claim list, the words and the chunk's entries
    // (device); page-locked: the words, the entries, the range form's seed slice and — only for a chunk with runner verdicts whose seeds the
    // caller still wants — the chunk's results.
    template <class Entry, size_t SlotBytes, size_t Words>
    struct ObsReport {
        DevBuf<uint32_t> tab, list; DevBuf<unsigned long long> words; DevBuf<Entry> ent;
        PinnedBuf<unsigned long long> h_words; PinnedBuf<Entry> h_ent; PinnedBuf<uint64_t> h_seeds; PinnedBuf<madsim_result_t> h_res;
        bool dirty = true;
        int ensure(uint64_t slots, uint64_t cap, uint64_t chunk, bool range, hipStream_t s) {
            const size_t tab_words = (size_t)(slots * SlotBytes / sizeof(uint32_t));
            if (tab_words > tab.cap) dirty = true;
            HIP_TRY(tab.room(tab_words, s));
            HIP_TRY(list.room((size_t)cap, s));
            HIP_TRY(ent.room((size_t)cap, s));
            HIP_TRY(h_ent.room((size_t)cap, s));
            HIP_TRY(words.room(Words));
            HIP_TRY(h_words.room(Words));
            if (range) HIP_TRY(h_seeds.room((size_t)chunk, s));
            if (dirty) {
                HIP_TRY(hipMemsetAsync(tab, 0, tab.cap * sizeof(uint32_t), s));
                HIP_TRY(hipStreamSynchronize(s));
                dirty = false;
            }
            return 0;
        }
    };
    ObsReport<madsim_census_value_t, MADSIM_K_CENSUS_SLOT_BYTES, MADSIM_K_CENSUS_WORDS> census;
    struct ProbeSets : ObsReport<madsim_probe_set_t, MADSIM_K_PROBE_SETS_SLOT_BYTES, MADSIM_K_PROBE_SETS_WORDS> {
        DevBuf<uint64_t> sig;                 // its own: the set word of every seed of a chunk (device only)
        int ensure(uint64_t slots, uint64_t cap, uint64_t chunk, bool range, hipStream_t s) {
            HIP_TRY(sig.room((size_t)chunk, s));
            return ObsReport::ensure(slots, cap, chunk, range, s);
        }
    } probe_sets;
    // the probe-order census: the dense matrix of cells takes the table's place (1024 cells of 32 bytes); the claim list is not used
    ObsReport<madsim_probe_order_pair_t, 32, MADSIM_K_PROBE_ORDER_WORDS> probe_order;
    // the stall-site census: the observation census's buffer group twice — the site pass and the shape pass — and what stall_sites_kernel
    // writes for them (device only): the chunk's site rows, shape words and the length array of ones
    struct Stall {
        ObsReport<madsim_census_value_t, MADSIM_K_CENSUS_SLOT_BYTES, MADSIM_K_CENSUS_WORDS> sites, shapes;
        DevBuf<uint64_t> rows, shape, ones;
    } stall;
    // probe spans: the chunk's records take the entries' place (one per definition; the table and the claim list are not used) and what
    // span_fold_kernel writes for span_witness_kernel (device only): state and duration per (seed, span)
    struct Spans : ObsReport<madsim_k_span_rec_t, 4, MADSIM_K_PROBE_SPANS_WORDS> {
        DevBuf<uint32_t> st; DevBuf<unsigned long long> dur;
    } probe_spans;
    Event ev0, ev1;
    Event pipe_begin;                         // run_pipelined: before the first sub-batch of a call
    Event tev[2 * 64];                        // timing slots of madsim_hip_run_batch_async
    DevBuf<uint64_t> d_prof;                  // debug counters (profiling kernel builds)
};

// One GPU's worth of runner state.  Re-entrant per handle: distinct contexts never share mutable state; one context
// serialises its callers on `mu`.
struct madsim_hip_ctx : madsim_hip_resources {
    std::mutex mu;
    int device = -1;
    int num_cus = 0;
    size_t lds_per_cu = 160 * 1024;
    uint32_t lds_attr = 0;
    madsim_resolve_t resolved{};              // the resolve account of the most recent campaign call (madsim_hip_ctx_campaign_resolved)

    madsim_geo::Device dev() const {
        madsim_geo::Device d; d.num_cus = num_cus > 0 ? num_cus : 256; d.lds_per_cu = lds_per_cu; d.vgprs = variant_vgprs_cached;
        static const int cap = [] { const char* e = getenv("MADSIM_HIP_WAVES_PER_SIMD"); return e ? atoi(e) : 0; }();    // (experiments: geometry.h Device)
        d.max_waves_per_simd = cap;
        return d;
    }
    int bind() { HIP_TRY(hipSetDevice(device)); return 0; }
    int open(int dev_index);
    void close();
    int upload_workload(const madsim_workload_t* w, KParams& P);
    int ensure_scratch(KParams& P, hipStream_t stream, bool work_queue);
    int launch(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t count, const uint64_t* d_seed_list,
               const madsim_limits_t* lim, madsim_result_t* d_out, hipStream_t stream);
    int reduce(const madsim_result_t* d_out, uint64_t count, uint64_t seed0, unsigned long long* d_acc4, hipStream_t stream);
    int run_device(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t count,
                   const madsim_limits_t* lim, madsim_result_t* d_out, hipStream_t stream, madsim_summary_t* summary);
    int run_host(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t count,
                 const madsim_limits_t* lim, madsim_result_t* out, madsim_summary_t* summary);
    int run_list(const madsim_workload_t* w, const madsim_config_t* cfg, const std::vector<uint64_t>& seeds,
                 const madsim_limits_t* lim, std::vector<madsim_result_t>& res, double* kernel_ms);
    int ensure_flights(uint32_t n, uint64_t batch, bool staging);
    uint32_t flights_for(const madsim_workload_t* w, const madsim_config_t* cfg, const madsim_limits_t* lim, uint64_t batch);
};

// The library keeps up to five sub-batches of a call in flight, each on its own HIP stream (run_pipelined, campaigns).  ROCclr maps
// the streams of a process onto GPU_MAX_HW_QUEUES hardware queues (default 4): with more streams than queues two sub-batches share a
// queue and run one after the other — measured on an MI355X (round 5, tools/experiment/exp_r5_runbatch.py): madsim_hip_run_batch(262 144)
// 8.3 ms with the default, ~5 ms with 16 queues.  The variable is read when the HIP runtime initialises, and a library has no business
// changing its host's environment behind its back (setenv races with getenv on other threads, and the value leaks into child
// processes: round 5 did exactly that).  So the HOST sets it — `GPU_MAX_HW_QUEUES=16` in the environment, as madsim_amd/runtime.py and
// bench.py do before they load HIP, or madsim_hip_prefer_hw_queues() as the first thing in main() — and the library only says so,
// once, when it is about to use more streams than the process has queues.
static void hint_hw_queues(uint32_t streams) {
    static bool said = false;
    const char* e = getenv("GPU_MAX_HW_QUEUES");
    const long q = e ? atol(e) : 4;
    if (said || (long)streams <= q || getenv("MADSIM_HIP_QUIET")) return;
    said = true;
    fprintf(stderr, "madsim_hip: note: %u batches in flight but GPU_MAX_HW_QUEUES=%ld hardware queues: streams will share queues (about 1.6x slower "
                    "madsim_hip_run_batch).  Set GPU_MAX_HW_QUEUES=16 before the process first touches HIP, or call madsim_hip_prefer_hw_queues(16) "
                    "at start-up.  (MADSIM_HIP_QUIET=1 silences this.)\n", streams, q);
}

int madsim_hip_ctx::open(int dev_index) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return fail(MADSIM_E_HIP, "no HIP device visible (this library has no CPU fallback)");
    if (dev_index < 0 || dev_index >= n) return fail(MADSIM_E_ARG, "device index out of range");
    device = dev_index;
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    num_cus = prop.multiProcessorCount;
    lds_per_cu = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor : 160 * 1024;
    if (lds_per_cu > 160 * 1024) lds_per_cu = 160 * 1024;
    HIP_TRY(d_acc.room(4));
    HIP_TRY(d_prof.room(16));
    HIP_TRY(hipMemset(d_prof, 0, 16 * sizeof(uint64_t)));
    HIP_TRY(ev0.ensure());
    HIP_TRY(ev1.ensure());
    HIP_TRY(pipe_begin.ensure());
    return 0;
}

// Everything is released here, with the device bound and idle (also what an open() that failed half-way left): the members' destructors
// then find nothing left.
void madsim_hip_ctx::close() {
    if (device < 0) return;
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    static_cast<madsim_hip_resources&>(*this) = madsim_hip_resources();
    device = -1;
}

int madsim_hip_ctx::upload_workload(const madsim_workload_t* w, KParams& P) {
    madsim_geo::DeviceTables T;
    int rc = madsim_geo::build_tables(w, &T, &g_err);
    if (rc) return rc;
    std::vector<uint32_t> host;
    host.reserve(T.insns.size() + w->n_progs + T.socks.size() + T.nodes.size() + 2 * T.durs.size() + 1);
    host.insert(host.end(), T.insns.begin(), T.insns.end());
    host.insert(host.end(), T.progs.begin(), T.progs.begin() + w->n_progs);
    host.insert(host.end(), T.socks.begin(), T.socks.end());
    host.insert(host.end(), T.nodes.begin(), T.nodes.end());
    for (uint64_t d : T.durs) { host.push_back((uint32_t)d); host.push_back((uint32_t)(d >> 32)); }
    host.push_back(w->n_insns);
    const uint64_t h = fnv(host.data(), host.size() * 4, 14695981039346656037ull);
    const Tables* hit = nullptr;
    for (auto& t : tables) if (t.hash == h && t.host == host) hit = &t;     // hash first, then the bytes themselves
    if (!hit) {
        if (tables.size() >= 16) {                       // bounded cache: drop everything once nothing is in flight
            HIP_TRY(hipDeviceSynchronize());
            tables.clear();
        }
        Tables t;
        t.hash = h;
        auto up = [&]() -> int {                         // (16 bytes of slack behind each table)
            HIP_TRY(t.insns.room(T.insns.size() + 4));
            HIP_TRY(t.progs.room(T.progs.size() + 4));
            HIP_TRY(t.socks.room(T.socks.size() + 4));
            HIP_TRY(t.durs.room(T.durs.size() + 2));
            HIP_TRY(t.nodes.room(T.nodes.size() + 4));
            HIP_TRY(t.iter_est.room(ITER_KEYS));
            HIP_TRY(hipMemset(t.iter_est, 0, ITER_KEYS * sizeof(uint32_t)));
            HIP_TRY(hipMemcpy(t.nodes, T.nodes.data(), T.nodes.size() * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(t.insns, T.insns.data(), T.insns.size() * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(t.progs, T.progs.data(), T.progs.size() * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(t.socks, T.socks.data(), T.socks.size() * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(t.durs, T.durs.data(), T.durs.size() * 8, hipMemcpyHostToDevice));
            return 0;
        };
        if ((rc = up())) return rc;                      // (no partial allocation survives an error: `t` frees what it holds)
        t.host = std::move(host);
        tables.push_back(std::move(t));
        hit = &tables.back();
    }
    P.insns = (const uint4*)hit->insns.p; P.progs = hit->progs; P.socks = hit->socks; P.nodes = hit->nodes; P.dur_table = hit->durs;
    // (MADSIM_HIP_NO_PRIO=1 in the environment: launches without the progress-based wave priorities of k_main.h — a diagnostic / A-B switch,
    //  results are the same either way)
    // The pass estimate is a property of the launch SHAPE, not of the workload alone: the capacities change the kernel build and the spilled
    // levels, the seeds per lane (a 65 536-seed campaign batch against a compacted re-run list) the passes a wave runs.  One word per
    // shape, picked by a hash of both (a collision costs fairness between co-resident launches, never a result).
    {
        static const bool off = getenv("MADSIM_HIP_NO_PRIO") != nullptr;
        const uint64_t per_lane = P.total_lanes ? (P.count + P.total_lanes - 1) / P.total_lanes : 1;
        const uint32_t shape[8] = {P.heap_lds, P.heap_spill, P.max_tasks, P.lw_shift, P.gstate_mode | P.narrow << 1 | P.compact << 2 | (P.dedup_n ? 8u : 0u),
                                   P.mbox_regs, P.max_steps, (uint32_t)std::min<uint64_t>(per_lane, 0xffffffffu)};
        P.iter_est = off ? nullptr : hit->iter_est + (fnv(shape, sizeof shape, 14695981039346656037ull) % ITER_KEYS);
    }
    return 0;
}

int madsim_hip_ctx::ensure_scratch(KParams& P, hipStream_t stream, bool work_queue) {
    P.spill = nullptr; P.work_ctr = nullptr; P.gstate = nullptr;
    if (!P.heap_spill && !work_queue && !P.gstate_mode && !P.compact) return 0;
    Scratch& sc = scratch[stream];
    if (P.gstate_mode || P.compact) {    // per-lane state blocks of the global-state builds / main-task records of the compact ones (seed_init writes what it reads)
        size_t need = (size_t)P.gs_stride * P.total_lanes;
        if (need >= (1ull << 32)) return fail(MADSIM_E_LIMITS, "global state region exceeds 4 GiB: lower the capacities");
        HIP_TRY(sc.gstate.room(need, stream));
        P.gstate = sc.gstate;
    }
    if (P.heap_spill) {
        size_t need = (size_t)P.heap_spill * P.total_lanes * (P.narrow ? 8 : sizeof(uint4));
        if (need >= (1ull << 32)) return fail(MADSIM_E_LIMITS, "heap spill region exceeds 4 GiB: lower heap_spill_slots");
        HIP_TRY(sc.spill.room(need, stream));
        P.spill = (uint4*)sc.spill.p;
    }
    if (work_queue) {
        HIP_TRY(sc.work_ctr.room(1));
        HIP_TRY(hipMemsetAsync(sc.work_ctr, 0, sizeof(unsigned long long), stream));
        P.work_ctr = sc.work_ctr;
    }
    return 0;
}

// Queue the simulation kernel for `count` units on `stream`: unit i runs seed d_seed_list[i] (device memory) when a list
// is given, else seed0 + i.  Nothing is synchronised.
int madsim_hip_ctx::launch(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t count, const uint64_t* d_seed_list,
                           const madsim_limits_t* lim, madsim_result_t* d_res, hipStream_t stream) {
    Geo G;
    int rc;
    if ((rc = madsim_geo::make_geometry(dev(), w, cfg, lim, count, &G, &g_err))) return rc;
    G.P.count = count;                              // (upload_workload keys the pass estimate by the launch shape: seeds per lane)
    if ((rc = upload_workload(w, G.P))) return rc;
    // Work distribution: static striding (lane g runs units g, g+G, ...) or a per-launch atomic counter from which a
    // finished lane pulls its next unit.  They only differ when a launch holds more units than resident lanes.
    const bool work_queue = lim && lim->sched == MADSIM_SCHED_QUEUE && count > G.P.total_lanes;
    if ((rc = ensure_scratch(G.P, stream, work_queue))) return rc;
    G.P.seed0 = seed0; G.P.count = count; G.P.seed_list = d_seed_list; G.P.out = d_res; G.P.prof = d_prof;
    if (G.lds_bytes > lds_attr) {
        int e = madsim_k_set_max_lds((uint32_t)lds_per_cu);
        if (e) return fail(MADSIM_E_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
        lds_attr = (uint32_t)lds_per_cu;
    }
    if (madsim_k_launch_sim(&G.P, G.grid, G.lds_bytes, stream, 0)) return fail(MADSIM_E_LIMITS, "no kernel build for this geometry (select_variant)");
    HIP_TRY(hipGetLastError());
    return 0;
}

// Queue the report reduction of d_out[0..count) into d_acc4 = {first failing seed, n_failed, steps, clock} on `stream`.
int madsim_hip_ctx::reduce(const madsim_result_t* d_res, uint64_t count, uint64_t seed0, unsigned long long* d_acc4, hipStream_t stream) {
    HIP_TRY(hipMemsetAsync(d_acc4, 0xff, 8, stream));
    HIP_TRY(hipMemsetAsync((char*)d_acc4 + 8, 0, 24, stream));
    madsim_k_launch_summary(d_res, count, seed0, d_acc4, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int madsim_hip_ctx::run_device(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t count,
                               const madsim_limits_t* lim, madsim_result_t* d_res, hipStream_t stream, madsim_summary_t* summary) {
    auto t0 = std::chrono::steady_clock::now();
    int rc = madsim_geo::validate(w, cfg, &g_err);
    if (rc) return rc;
    if (count == 0) {
        if (summary) { memset(summary, 0, sizeof *summary); summary->first_failing_seed = UINT64_MAX; }
        return 0;
    }
    if (!d_res) return fail(MADSIM_E_ARG, "null result buffer");
    if (summary) HIP_TRY(hipEventRecord(ev0, stream));
    if ((rc = launch(w, cfg, seed0, count, nullptr, lim, d_res, stream))) return rc;
    if (summary) {
        HIP_TRY(hipEventRecord(ev1, stream));
        if ((rc = reduce(d_res, count, seed0, d_acc, stream))) return rc;
        unsigned long long acc[4];
        HIP_TRY(hipMemcpyAsync(acc, d_acc, sizeof acc, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
        summary->first_failing_seed = acc[0]; summary->n_failed = acc[1];
        summary->total_steps = acc[2]; summary->total_clock_ns = acc[3];
        summary->kernel_ms = ms;
        summary->wall_s = since(t0);
    }
    return 0;
}


// One compacted launch over an arbitrary list of seeds (the re-run of seeds that outgrew a capacity).
int madsim_hip_ctx::run_list(const madsim_workload_t* w, const madsim_config_t* cfg, const std::vector<uint64_t>& seeds,
                             const madsim_limits_t* lim, std::vector<madsim_result_t>& res, double* kernel_ms) {
    const size_t n = seeds.size();
    res.resize(n);
    if (!n) return 0;
    int rc;
    DevBuf<madsim_result_t>& d_out = trace[0].out;
    HIP_TRY(d_out.room(n));
    HIP_TRY(d_seeds.room(n));
    HIP_TRY(hipMemcpy(d_seeds, seeds.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipEventRecord(ev0, nullptr));
    if ((rc = launch(w, cfg, 0, n, d_seeds, lim, d_out, nullptr))) return rc;
    HIP_TRY(hipEventRecord(ev1, nullptr));
    HIP_TRY(hipMemcpy(res.data(), d_out, n * sizeof(madsim_result_t), hipMemcpyDeviceToHost));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
    if (kernel_ms) *kernel_ms += ms;
    return 0;
}

// Streams, report words, events and result buffers of the first n flights (campaigns and run_pipelined share them; the
// context's mutex serialises the two).  `staging`: also a page-locked host buffer of `batch` results per flight.  What one campaign
// form needs beyond that its implementation asks of the flight's group for that form (Flight::Collect ... Flight::List).
int madsim_hip_ctx::ensure_flights(uint32_t n, uint64_t batch, bool staging) {
    if (n > (uint32_t)CAMPAIGN_MAX) return fail(MADSIM_E_ARG, "at most 8 batches in flight");
    hint_hw_queues(n);
    for (uint32_t i = 0; i < n; i++)
        if (int rc = flights[i].ensure(batch, staging)) return rc;
    return 0;
}

// Batches in flight by the workload's occupancy: a batch of 65 536 seeds is one wave per SIMD, so as many batches as the
// workload's LDS admits waves per SIMD, and — when that is four (the compact base-op layout) — a fifth, whose launch queues behind
// them and fills the gaps their tails leave.
uint32_t madsim_hip_ctx::flights_for(const madsim_workload_t* w, const madsim_config_t* cfg, const madsim_limits_t* lim, uint64_t batch) {
    madsim_geo::Geo G;
    uint32_t n = 3;
    if (!madsim_geo::make_geometry(dev(), w, cfg, lim, batch, &G, &g_err)) {
        if (G.blocks_per_cu * G.waves_per_block >= 16) n = 5;
        else if (G.P.gstate_mode && G.P.heap_spill) n = 4;      // long launches that end with their slowest wave: one more behind them
    }
    return n;
}

namespace {

madsim_hip_ctx* g_default = nullptr;       // the context behind the v1 entry points
std::mutex g_default_mu;

// Seeds that came back with a RUNNER verdict (a device capacity or the step cap, neither a reference concept) are run
// again, all of them in ONE compacted launch per round, with doubled capacities / a 16x step cap.
// The step cap never grows beyond madsim_limits_t.max_steps_ceiling (default 1 << 28 = the first pass's 1 << 24 and one 16x
// round): a livelocked workload — a yield loop, a 1 ms timer loop without a time limit — must come back as MADSIM_STEP_LIMIT
// after seconds, not hold the GPU (and the context mutex) in one non-preemptible kernel for an hour.
uint64_t step_ceiling(const madsim_limits_t& L) {
    uint64_t c = L.max_steps_ceiling ? L.max_steps_ceiling : (1u << 28);
    const uint64_t first = L.max_steps ? L.max_steps : (1u << 24);
    return c < first ? first : c;
}
// The ceiling of mbox_msgs for this workload: 127 without extended ops (the base-op mailbox header keeps 7 bits, and make_geometry refuses
// more), MADSIM_MAX_MBOX_MSGS with them.  Which ops a workload uses is read off the parameter block of its geometry under the default
// limits — the op classes do not depend on the limits, and they are set before anything a limit could make fail.
uint32_t mbox_msgs_ceiling(const madsim_workload_t* w) {
    Geo G;
    std::string ignored;
    const madsim_config_t cfg = madsim_geo::probe_config();
    madsim_geo::make_geometry(madsim_geo::Device(), w, &cfg, nullptr, 64, &G, &ignored);
    return G.P.lifecycle ? MADSIM_MAX_MBOX_MSGS : 127u;
}
void grow(madsim_limits_t& L, const madsim_workload_t* w, bool any_ovf, bool any_steps) {
    auto dbl = [](uint32_t v, uint32_t dflt, uint32_t cap) { uint32_t x = (v == 0 || v == MADSIM_LIMIT_NONE) ? dflt : v; x *= 2; return x > cap ? cap : x; };
    L.lanes_per_wave = 0;
    if (any_ovf) {
        // the compact base-op layout admits no heap spill and at most eight task slots: a grown re-run must be free to leave
        // it (an explicit MADSIM_STATE_COMPACT would fail make_geometry with MADSIM_E_LIMITS and take the whole call with it)
        if ((L.state_mem & 0xffu) == MADSIM_STATE_COMPACT) L.state_mem = (L.state_mem & ~0xffu) | MADSIM_STATE_AUTO;
        // ... and the 8-byte heap entries: a deadline beyond their 2^31 ns horizon is reported as a capacity verdict (k_timer.h timer_add)
        L.state_mem &= ~MADSIM_STATE_NARROW_HEAP;
        L.heap_lds_slots = L.heap_lds_slots ? L.heap_lds_slots : 8;
        L.heap_spill_slots = dbl(L.heap_spill_slots, 32, 1u << 20);
        L.max_tasks = dbl(L.max_tasks, w->n_progs + 8, 254);
        L.mbox_regs = dbl(L.mbox_regs, 2, 255);
        L.mbox_msgs = dbl(L.mbox_msgs, 2, mbox_msgs_ceiling(w));      // (255 for a base-op workload fits no build: MADSIM_E_LIMITS would take the whole call)
        L.max_conns = dbl(L.max_conns, 4, 127);
        L.chan_queue = dbl(L.chan_queue, 2, 15);
    }
    if (any_steps) {
        uint64_t s = L.max_steps ? L.max_steps : (1u << 24);
        s *= 16;
        const uint64_t ceil = step_ceiling(L);
        L.max_steps = s > ceil ? (uint32_t)ceil : (uint32_t)s;
    }
}

// `ctxs` = the contexts whose locks the caller holds: round r runs on ctxs[r % n] (the shards' overflow is spread, not piled
// on the first device).
int rerun_runner_verdicts(madsim_hip_ctx* const* ctxs, int n_ctx, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t count,
                          const madsim_limits_t* lim, madsim_result_t* out, int max_rounds, double* kernel_ms) {
    madsim_limits_t L{};
    if (lim) L = *lim;
    for (int round = 0; round < max_rounds; round++) {
        std::vector<uint64_t> idx;
        bool any_ovf = false, any_steps = false;
        const bool steps_maxed = (L.max_steps ? L.max_steps : (1u << 24)) >= step_ceiling(L);
        for (uint64_t i = 0; i < count; i++) {
            if (out[i].verdict == MADSIM_OVERFLOW) { idx.push_back(i); any_ovf = true; }
            else if (out[i].verdict == MADSIM_STEP_LIMIT && !steps_maxed) { idx.push_back(i); any_steps = true; }
        }
        if (idx.empty()) break;
        grow(L, w, any_ovf, any_steps);
        std::vector<uint64_t> seeds(idx.size());
        for (size_t k = 0; k < idx.size(); k++) seeds[k] = seed0 + idx[k];
        std::vector<madsim_result_t> res;
        madsim_hip_ctx* c = ctxs[round % n_ctx];
        int rc = c->bind();
        if (rc) return rc;
        if ((rc = c->run_list(w, cfg, seeds, &L, res, kernel_ms))) return rc;
        for (size_t k = 0; k < idx.size(); k++) out[idx[k]] = res[k];
    }
    return 0;
}

void host_summary(const madsim_result_t* out, uint64_t seed0, uint64_t count, madsim_summary_t* f) {
    memset(f, 0, sizeof *f);
    f->first_failing_seed = UINT64_MAX;
    for (uint64_t i = 0; i < count; i++) {
        if (out[i].verdict != MADSIM_PASS) { if (!f->n_failed) f->first_failing_seed = seed0 + i; f->n_failed++; }
        f->total_steps += out[i].steps; f->total_clock_ns += out[i].clock_ns;
    }
}


// Per-seed results at the overlapped rate (one launch of 65 536 seeds is one wave per SIMD and leaves two
// thirds of the issue slots idle).  Builder::run hands over ALL its seeds in one call (runtime/builder.rs:121-162), so the call
// itself cuts [seed0, seed0 + count) into sub-batches: every context runs its contiguous share (context g: the block
// g * ceil(count / n) — the rule of madsim_amd/dist.py shard_range), keeping `flights` sub-batches in flight on its own streams;
// each sub-batch is kernel -> report reduction (accumulating in the flight's six words) -> device-to-host copy into the flight's
// page-locked staging buffer, and the host moves a finished sub-batch into the caller's array while the next ones run.  Every
// launch is queued from the calling thread; once the first kernel is in flight no error returns before every launched stream
// has been drained.  `acc6` (optional): the folded device reports {first failing seed, failed, steps, clock, first genuine, runner}.
constexpr uint64_t PIPE_BATCH = 65536;
int run_pipelined(madsim_hip_ctx* const* ctxs, int n_ctx, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t count,
                  const madsim_limits_t* lim, madsim_result_t* out, unsigned long long* acc6, double* kernel_ms) {
    struct Pipe { madsim_hip_ctx* c; uint64_t lo = 0, n = 0, nb = 0, launched = 0, harvested = 0; uint32_t F = 0; double ms = 0.0; };
    std::vector<Pipe> pp(n_ctx);
    const uint64_t chunk = (count + (uint64_t)n_ctx - 1) / (uint64_t)n_ctx;
    int first_err = 0;
    std::string first_msg;
    auto note = [&](int e) { if (e && !first_err) { first_err = e; first_msg = g_err; } return e; };
    for (int g = 0; g < n_ctx; g++) {
        Pipe& p = pp[g];
        p.c = ctxs[g];
        p.lo = std::min((uint64_t)g * chunk, count);
        p.n = std::min(p.lo + chunk, count) - p.lo;
        p.nb = (p.n + PIPE_BATCH - 1) / PIPE_BATCH;
        if (!p.nb) continue;
        int e;
        if (note(e = p.c->bind())) break;
        p.F = (uint32_t)std::min<uint64_t>(p.nb, p.c->flights_for(w, cfg, lim, std::min(p.n, PIPE_BATCH)));
        if (note(e = p.c->ensure_flights(p.F, std::min(p.n, PIPE_BATCH), out != nullptr))) break;
    }
    if (first_err) return fail(first_err, first_msg);
    auto queue = [&](Pipe& p) -> int {
        const uint64_t k = p.launched;
        madsim_hip_ctx::Flight& f = p.c->flights[k % p.F];
        const uint64_t lo = p.lo + k * PIPE_BATCH, n = std::min(PIPE_BATCH, p.lo + p.n - lo);
        int e;
        if ((e = p.c->bind())) return e;
        if (k < p.F) {                                           // the flight's first sub-batch of this call: a fresh report
            char* const d_words = (char*)f.d_rep.p;
            HIP_TRY(hipMemsetAsync(d_words, 0xff, 8, f.stream));
            HIP_TRY(hipMemsetAsync(d_words + 8, 0, 24, f.stream));
            HIP_TRY(hipMemsetAsync(d_words + 32, 0xff, 8, f.stream));
            HIP_TRY(hipMemsetAsync(d_words + 40, 0, 8, f.stream));
        }
        if (k == 0) HIP_TRY(hipEventRecord(p.c->pipe_begin, f.stream));
        p.launched++;                                            // from here on the flight must be drained before returning
        if ((e = p.c->launch(w, cfg, seed0 + lo, n, nullptr, lim, f.d_out, f.stream))) return e;
        HIP_TRY(hipEventRecord(f.e1, f.stream));
        madsim_k_launch_summary6(f.d_out, n, seed0 + lo, f.d_rep, f.stream);
        HIP_TRY(hipGetLastError());
        if (out) HIP_TRY(hipMemcpyAsync(f.h_out, f.d_out, n * sizeof(madsim_result_t), hipMemcpyDeviceToHost, f.stream));
        HIP_TRY(hipEventRecord(f.done, f.stream));
        return 0;
    };
    auto harvest = [&](Pipe& p) -> int {
        const uint64_t k = p.harvested++;
        madsim_hip_ctx::Flight& f = p.c->flights[k % p.F];
        int e;
        if ((e = p.c->bind())) return e;
        HIP_TRY(hipEventSynchronize(f.done));
        if (first_err) return 0;                                 // (draining after an error: nothing is moved any more)
        const uint64_t lo = p.lo + k * PIPE_BATCH, n = std::min(PIPE_BATCH, p.lo + p.n - lo);
        if (out) memcpy(out + lo, f.h_out, n * sizeof(madsim_result_t));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, p.c->pipe_begin, f.e1));
        p.ms = std::max(p.ms, (double)ms);
        return 0;
    };
    for (;;) {
        bool any = false;
        for (Pipe& p : pp)                                       // 1. fill every device's flights before waiting for any of them
            while (!first_err && p.launched < p.nb && p.launched - p.harvested < p.F) { note(queue(p)); any = true; }
        for (Pipe& p : pp)                                       // 2. then the oldest sub-batch of every device
            if (p.harvested < p.launched) { note(harvest(p)); any = true; }
        if (!any) break;
    }
    if (first_err) {
        // A queue() that failed between its kernel launch and the record of `done` leaves that event stale (or never recorded): the
        // harvest above returned at once.  No kernel may stay in flight behind an error return — it would still be writing the
        // flight's buffers — so every stream this call used is drained for real.
        for (Pipe& p : pp) {
            if (!p.F || p.c->bind()) continue;
            for (uint32_t i = 0; i < p.F; i++) (void)hipStreamSynchronize(p.c->flights[i].stream);
        }
        return fail(first_err, first_msg);
    }
    unsigned long long a[6] = {~0ull, 0, 0, 0, ~0ull, 0};
    double ms = 0.0;
    for (Pipe& p : pp) {
        if (!p.nb) continue;
        int e;
        if ((e = p.c->bind())) return e;
        for (uint32_t i = 0; i < p.F; i++) {
            madsim_hip_ctx::Flight& f = p.c->flights[i];
            HIP_TRY(hipMemcpyAsync(f.h_rep, f.d_rep, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost, f.stream));
            HIP_TRY(hipStreamSynchronize(f.stream));
            a[0] = std::min(a[0], f.h_rep[0]); a[4] = std::min(a[4], f.h_rep[4]);
            a[1] += f.h_rep[1]; a[2] += f.h_rep[2]; a[3] += f.h_rep[3]; a[5] += f.h_rep[5];
        }
        ms = std::max(ms, p.ms);                                 // devices ran concurrently
    }
    if (acc6) memcpy(acc6, a, sizeof a);
    if (kernel_ms) *kernel_ms += ms;
    return 0;
}

}  // namespace

constexpr uint64_t PIPE_BATCH_HOST = 65536 + 32768;     // up to one and a half batches stay one launch
int madsim_hip_ctx::run_host(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t count,
                             const madsim_limits_t* lim, madsim_result_t* out, madsim_summary_t* summary) {
    auto t0 = std::chrono::steady_clock::now();
    int rc;
    if (count > PIPE_BATCH_HOST) {             // more than one batch: sub-launches kept in flight, copies overlapped (run_pipelined)
        if ((rc = madsim_geo::validate(w, cfg, &g_err))) return rc;
        unsigned long long a[6];                     // (`out` may be NULL: summary only — no staging buffers, no copies)
        double ms = 0.0;
        madsim_hip_ctx* one[1] = {this};
        if ((rc = run_pipelined(one, 1, w, cfg, seed0, count, lim, out, a, &ms))) return rc;
        if (summary) {
            summary->first_failing_seed = a[0]; summary->n_failed = a[1]; summary->total_steps = a[2]; summary->total_clock_ns = a[3];
            summary->kernel_ms = ms; summary->wall_s = since(t0);
        }
        return 0;
    }
    DevBuf<madsim_result_t>& d_out = trace[0].out;
    HIP_TRY(d_out.room(count));
    madsim_summary_t tmp;
    if ((rc = run_device(w, cfg, seed0, count, lim, d_out, nullptr, &tmp))) return rc;
    if (out && count) HIP_TRY(hipMemcpy(out, d_out, count * sizeof(madsim_result_t), hipMemcpyDeviceToHost));
    if (summary) { *summary = tmp; summary->wall_s = since(t0); }
    return 0;
}

namespace {

#define CTX_ENTER(c)                                                                              \
    if (!(c) || (c)->device < 0) return fail(MADSIM_E_NOINIT, "no context (madsim_hip_init / madsim_hip_ctx_create has not been called)"); \
    std::lock_guard<std::mutex> lk((c)->mu);                                                      \
    { int brc_ = (c)->bind(); if (brc_) return brc_; }

// The contexts of a _multi call, checked and locked in address order (two threads passing the same contexts in different orders cannot
// deadlock).  `who` names the entry point in "needs at least one context".
int lock_contexts(madsim_hip_ctx* const* ctxs, int n_ctx, const char* who, std::vector<std::unique_lock<std::mutex>>& locks) {
    if (!ctxs || n_ctx < 1) return fail(MADSIM_E_ARG, std::string(who) + " needs at least one context");
    for (int g = 0; g < n_ctx; g++) {
        if (!ctxs[g]) return fail(MADSIM_E_NOINIT, "null context");
        for (int h = 0; h < g; h++) if (ctxs[h] == ctxs[g]) return fail(MADSIM_E_ARG, "the same context appears twice");
    }
    std::vector<madsim_hip_ctx*> order(ctxs, ctxs + n_ctx);
    std::sort(order.begin(), order.end(), [](madsim_hip_ctx* a, madsim_hip_ctx* b) { return std::less<madsim_hip_ctx*>()(a, b); });
    for (madsim_hip_ctx* c : order) locks.emplace_back(c->mu);
    for (int g = 0; g < n_ctx; g++) if (ctxs[g]->device < 0) return fail(MADSIM_E_NOINIT, "closed context");
    return 0;
}

// The contexts a campaign call runs on: one context (what CTX_ENTER does) or the contexts of a _multi call (what lock_contexts does, `who`
// naming the entry point).  enter() checks and locks them; the locks are held for as long as this object lives.
class Contexts {
    madsim_hip_ctx* one_[1];
    madsim_hip_ctx* const* ctxs_;
    int n_;
    const char* who_;                                            // (null: the single-context form)
    std::vector<std::unique_lock<std::mutex>> locks_;
public:
    explicit Contexts(madsim_hip_ctx* c) : one_{c}, ctxs_(one_), n_(1), who_(nullptr) {}
    Contexts(madsim_hip_ctx* const* ctxs, int n_ctx, const char* who) : one_{nullptr}, ctxs_(ctxs), n_(n_ctx), who_(who) {}
    Contexts(const Contexts&) = delete;
    Contexts& operator=(const Contexts&) = delete;
    // `nothing_to_run`: the call's seed list is empty.  An empty list needs no device — the single-context forms' rule, and theirs only:
    // without an open context they run on no context at all (the engines then fill the reports of an empty range and return 0), while a
    // _multi call still asks for at least one context.
    int enter(bool nothing_to_run = false) {
        if (who_) return lock_contexts(ctxs_, n_, who_, locks_);
        madsim_hip_ctx* const c = one_[0];
        if (nothing_to_run && (!c || c->device < 0)) { ctxs_ = nullptr; n_ = 0; return 0; }
        if (!c || c->device < 0) return fail(MADSIM_E_NOINIT, "no context (madsim_hip_init / madsim_hip_ctx_create has not been called)");
        locks_.emplace_back(c->mu);
        return c->bind();
    }
    madsim_hip_ctx* const* ctxs() const { return ctxs_; }
    int n() const { return n_; }
};

}  // namespace

extern "C" {

uint32_t madsim_hip_version(void) { return MADSIM_HIP_ABI_VERSION; }

// Explicit opt-in for hosts that cannot set their own environment: asks ROCclr for `n` hardware queues (GPU_MAX_HW_QUEUES) unless the
// variable is already set.  Only effective before the process's first HIP call, and — like every setenv — only safe while no other
// thread reads the environment: call it first thing in main().  Returns 1 when it set the variable, 0 when the host's own value stands.
int madsim_hip_prefer_hw_queues(int n) {
    if (n < 1 || n > 64) return fail(MADSIM_E_ARG, "hardware queues: 1..64");
    if (getenv("GPU_MAX_HW_QUEUES")) return 0;
    char buf[16];
    snprintf(buf, sizeof buf, "%d", n);
    return setenv("GPU_MAX_HW_QUEUES", buf, 0) == 0 ? 1 : fail(MADSIM_E_ARG, "setenv failed");
}

#define MADSIM_STR2(x) #x
#define MADSIM_STR(x) MADSIM_STR2(x)
const char* madsim_hip_build_info(void) {
    static const std::string info = std::string("madsim_hip abi=") + MADSIM_STR(MADSIM_HIP_ABI_VERSION) + " arch=gfx950 kernels="
        + std::to_string(madsim_k::n_variants) + " backend=hip-rocm"
#ifdef MADSIM_EXPERIMENT_BUILD
        + " experiment-build"
#endif
        ;
    return info.c_str();
}

const char* madsim_hip_strerror(int code) {
    switch (code) {
    case 0: return "ok";
    case MADSIM_E_ARG: return "invalid argument";
    case MADSIM_E_HIP: return "HIP runtime error";
    case MADSIM_E_NOINIT: return "library not initialised (no GPU bound)";
    case MADSIM_E_WORKLOAD: return "malformed workload";
    case MADSIM_E_LIMITS: return "limits do not fit the device";
    default: return "unknown error";
    }
}

const char* madsim_hip_last_error(void) { return g_err.c_str(); }

// ---- per-device contexts ---------------------------------------------------------------------------------------------

int madsim_hip_ctx_create(int device, madsim_hip_ctx_t** out) {
    if (!out) return fail(MADSIM_E_ARG, "null context pointer");
    *out = nullptr;
    madsim_hip_ctx* c = new madsim_hip_ctx();
    int rc = c->open(device);
    if (rc) { c->close(); delete c; return rc; }
    *out = c;
    return 0;
}

int madsim_hip_ctx_destroy(madsim_hip_ctx_t* c) {
    if (!c) return 0;
    { std::lock_guard<std::mutex> lk(c->mu); c->close(); }
    delete c;
    return 0;
}

int madsim_hip_ctx_device(const madsim_hip_ctx_t* c) { return c ? c->device : -1; }

int madsim_hip_ctx_run_batch(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t count,
                             const madsim_limits_t* lim, madsim_result_t* out, madsim_summary_t* summary) {
    CTX_ENTER(c);
    return c->run_host(w, cfg, seed0, count, lim, out, summary);
}

int madsim_hip_ctx_run_batch_device(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t count,
                                    const madsim_limits_t* lim, void* d_out, void* stream, madsim_summary_t* summary) {
    CTX_ENTER(c);
    return c->run_device(w, cfg, seed0, count, lim, (madsim_result_t*)d_out, (hipStream_t)stream, summary);
}

int madsim_hip_ctx_run_batch_async(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t count,
                                   const madsim_limits_t* lim, void* d_out, void* d_summary4, void* stream, int timing_slot) {
    CTX_ENTER(c);
    if (timing_slot >= 64) return fail(MADSIM_E_ARG, "timing_slot must be < 64");
    hipStream_t st = (hipStream_t)stream;
    Event* ev = nullptr;
    if (timing_slot >= 0) {
        ev = &c->tev[2 * timing_slot];
        HIP_TRY(ev[0].ensure()); HIP_TRY(ev[1].ensure());
        HIP_TRY(hipEventRecord(ev[0], st));
    }
    int rc = c->run_device(w, cfg, seed0, count, lim, (madsim_result_t*)d_out, st, nullptr);
    if (rc) return rc;
    if (ev) HIP_TRY(hipEventRecord(ev[1], st));
#ifdef MADSIM_EXP_NO_SUMMARY      // (timing experiment, tools/build_variant.sh only: what the report reduction behind every launch costs the stream)
    d_summary4 = nullptr;
#endif
    if (d_summary4 && count) {
        // {UINT64_MAX, 0, 0, 0}, accumulated by the reduction kernel, then word 0 is flipped into its
        // order-preserving int64 form (seed ^ 1<<63) so a signed all-reduce(MIN) yields the unsigned minimum
        if ((rc = c->reduce((const madsim_result_t*)d_out, count, seed0, (unsigned long long*)d_summary4, st))) return rc;
        madsim_k_launch_keyflip((unsigned long long*)d_summary4, st);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

int madsim_hip_ctx_timing_ms(madsim_hip_ctx_t* c, int timing_slot, double* ms) {
    CTX_ENTER(c);
    if (timing_slot < 0 || timing_slot >= 64 || !c->tev[2 * timing_slot + 1] || !ms) return fail(MADSIM_E_ARG, "bad timing slot");
    float f = 0.f;
    HIP_TRY(hipEventSynchronize(c->tev[2 * timing_slot + 1]));
    HIP_TRY(hipEventElapsedTime(&f, c->tev[2 * timing_slot], c->tev[2 * timing_slot + 1]));
    *ms = f;
    return 0;
}

// The resolve account of the most recent campaign call made through the context (the shape of madsim_hip_ctx_timing_ms).
int madsim_hip_ctx_campaign_resolved(madsim_hip_ctx_t* c, madsim_resolve_t* out) {
    if (!out) return fail(MADSIM_E_ARG, "null madsim_resolve_t");
    memset(out, 0, sizeof *out);
    if (!c || c->device < 0) return fail(MADSIM_E_NOINIT, "no context (madsim_hip_init / madsim_hip_ctx_create has not been called)");
    std::lock_guard<std::mutex> lk(c->mu);
    *out = c->resolved;
    return 0;
}

// G^rounds(lim): `rounds` applications of the growth step a resolve round (and a re-run round of madsim_hip_run_batch_auto that met both
// kinds of runner verdict) takes.  No device involved.
int madsim_hip_grow_limits(const madsim_workload_t* w, const madsim_limits_t* lim, uint32_t rounds, madsim_limits_t* out) {
    if (!w || !out) return fail(MADSIM_E_ARG, "madsim_hip_grow_limits: null workload or result");
    if (rounds > 64) return fail(MADSIM_E_ARG, "madsim_hip_grow_limits: at most 64 rounds");
    madsim_limits_t L{};
    if (lim) L = *lim;
    for (uint32_t r = 0; r < rounds; r++) grow(L, w, true, true);
    *out = L;
    return 0;
}

int madsim_hip_ctx_run_batch_auto(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t count,
                                  const madsim_limits_t* lim, madsim_result_t* out, madsim_summary_t* summary, int max_rounds) {
    if (!out && count) return fail(MADSIM_E_ARG, "run_batch_auto needs the result array");
    CTX_ENTER(c);
    auto t0 = std::chrono::steady_clock::now();
    madsim_summary_t s{};
    int rc = c->run_host(w, cfg, seed0, count, lim, out, &s);
    if (rc) return rc;
    double kernel_ms = s.kernel_ms;
    madsim_hip_ctx* one[1] = {c};
    if ((rc = rerun_runner_verdicts(one, 1, w, cfg, seed0, count, lim, out, max_rounds, &kernel_ms))) return rc;
    if (summary) { host_summary(out, seed0, count, summary); summary->kernel_ms = kernel_ms; summary->wall_s = since(t0); }
    return 0;
}

// One side of a trace call.  trace_prepare: geometry, tables, scratch, the side's buffer set (madsim_hip_ctx::trace) grown to the call's
// sizes and the parameter block filled — nothing is queued.  trace_queue: the set zeroed and the trace launch, behind whatever the stream
// holds; TraceSteps keeps the first error and queues nothing behind it.  Shared by madsim_hip_trace_seeds, madsim_hip_trace_seed (side A's
// set alone) and both sides of madsim_hip_diverge_seeds.
struct TraceSteps {
    hipError_t err = hipSuccess;
    const char* at = nullptr;
    bool no_build = false;
    bool operator()(hipError_t e, const char* what) { if (e != hipSuccess && err == hipSuccess) { err = e; at = what; } return err == hipSuccess && !no_build; }
};

static int trace_prepare(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, const madsim_limits_t* lim, uint64_t n,
                         uint64_t log_cap, uint64_t obs_cap, madsim_hip_ctx::TraceSet& S, Geo& G, hipStream_t st, const uint64_t* task_cap = nullptr, bool times = false) {
    int rc;
    if ((rc = madsim_geo::make_geometry(c->dev(), w, cfg, lim, n, &G, &g_err, true))) return rc;
    G.P.count = n;
    if ((rc = c->upload_workload(w, G.P))) return rc;
    if ((rc = c->ensure_scratch(G.P, st, false))) return rc;
    HIP_TRY(S.log.room((size_t)(n * log_cap)));
    times = times && obs_cap;                                                // (never without the observation log: the kernel addresses the time row from it)
    if (times && n * obs_cap > 0xffffffffull) return fail(MADSIM_E_LIMITS, "the time log: n x obs_cap exceeds 2^32 - 1 words");
    HIP_TRY(S.obs.room((size_t)(n * obs_cap * (times ? 2 : 1))));           // (the time rows: the second half, only where a call asks for them)
    HIP_TRY(S.len.room((size_t)(2 * n)));                                    // [n] log lengths, then [n] observation counts
    HIP_TRY(c->d_seeds.room((size_t)n));
    HIP_TRY(S.out.room((size_t)n));
    if (task_cap) {                                                          // (at least one word: a non-null task_log is what asks the kernel for the counts)
        HIP_TRY(S.task.room((size_t)std::max<uint64_t>(n * *task_cap, 1)));
        HIP_TRY(S.task_len.room((size_t)n));
    }
    if (G.lds_bytes > c->lds_attr) {
        if (madsim_k_set_max_lds((uint32_t)c->lds_per_cu)) return fail(MADSIM_E_HIP, "hipFuncSetAttribute failed");
        c->lds_attr = (uint32_t)c->lds_per_cu;
    }
    G.P.seed0 = 0; G.P.count = n; G.P.seed_list = c->d_seeds; G.P.out = S.out;
    G.P.trace_log = log_cap ? S.log : nullptr; G.P.trace_cap = log_cap; G.P.trace_len = S.len;
    G.P.obs_log = obs_cap ? S.obs : nullptr; G.P.obs_cap = obs_cap; G.P.obs_len = S.len + n;
    if (task_cap) { G.P.task_log = S.task; G.P.task_cap = *task_cap; G.P.task_len = S.task_len; }
    if (times) G.P.obs_time_words = (uint32_t)(n * obs_cap);
    return 0;
}

static bool trace_queue(const Geo& G, const madsim_hip_ctx::TraceSet& S,uint64_t n, uint64_t log_cap, uint64_t obs_cap, bool zero_log, hipStream_t st,
                        TraceSteps& step, bool ok) {
    if (ok && log_cap && zero_log) ok = step(hipMemsetAsync(S.log, 0, n * log_cap, st), "hipMemsetAsync(log rows)");
    if (ok && obs_cap) ok = step(hipMemsetAsync(S.obs, 0, n * obs_cap * sizeof(uint64_t), st), "hipMemsetAsync(observation rows)");
    if (ok && obs_cap && G.P.obs_time_words) ok = step(hipMemsetAsync(S.obs + n * obs_cap, 0, n * obs_cap * sizeof(uint64_t), st), "hipMemsetAsync(time rows)");
    if (ok) ok = step(hipMemsetAsync(S.len, 0, 2 * n * sizeof(uint64_t), st), "hipMemsetAsync(lengths)");
    if (ok && G.P.task_log && G.P.task_cap) ok = step(hipMemsetAsync(S.task, 0, n * G.P.task_cap * sizeof(uint64_t), st), "hipMemsetAsync(task rows)");
    if (ok && G.P.task_log) ok = step(hipMemsetAsync(S.task_len, 0, n * sizeof(uint64_t), st), "hipMemsetAsync(task counts)");
    if (ok) ok = step(hipMemsetAsync(S.out, 0, n * sizeof(madsim_result_t), st), "hipMemsetAsync(results)");
    if (ok) {
        step.no_build = madsim_k_launch_sim(&G.P, G.grid, G.lds_bytes, st, 1) != 0;
        ok = step(step.no_build ? hipSuccess : hipGetLastError(), "trace kernel launch");
    }
    return ok;
}

// Replay a list of seeds on the trace build: one launch, unit i = seeds[i], each unit with its own row of the determinism log and of the
// observation log and its own pair of length words (k_main.h).  The device buffers are zero before the launch, so a row comes back as its
// first min(len, cap) entries and zeros; every output is one copy, and the call ends with one synchronisation of the stream it ran on.
// Once anything is queued that reads or writes the caller's memory no error returns before that synchronisation: the first error is kept
// and nothing more is queued behind it.
// `single` is madsim_hip_trace_seed, as it always was: one seed, the log copied straight into the caller's buffer — its first min(len, cap)
// bytes and nothing behind them, so the device row needs no zeroes —, no bound on `log_cap` but the device's memory, and results that
// carry the fingerprint whatever the limits say.  The list form answers with the bytes madsim_hip_run_batch gives: the trace builds always
// fold the determinism log, so under madsim_limits_t.no_trace_hash its results' trace_hash is zeroed here.
// (`tr`: madsim_hip_task_states — one more optional buffer, the task log's rows and counts; `times`: madsim_hip_timeline_seeds — the time
// log's rows beside the observation rows; madsim_hip_trace_seeds passes neither and queues what it queued)
struct TaskRows { uint64_t* tasks; uint64_t cap; uint64_t* len; };
static int trace_list(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n,
                      const madsim_limits_t* lim, uint8_t* logs, uint64_t log_cap, uint64_t* obs, uint64_t obs_cap,
                      uint64_t* log_len, uint64_t* obs_len, madsim_result_t* out, bool single, const TaskRows* tr = nullptr, uint64_t* times = nullptr) {
    if (n == 0) return 0;
    if (!seeds) return fail(MADSIM_E_ARG, tr ? "task_states: null seed list" : times ? "timeline_seeds: null seed list" : "trace_seeds: null seed list");
    if (times && !obs) return fail(MADSIM_E_ARG, "timeline_seeds: time rows without observation rows");
    if (tr) {
        if ((tr->tasks != nullptr) != (tr->cap != 0)) return fail(MADSIM_E_ARG, "task_states: `tasks` and task_cap are given together or not at all");
        if (tr->cap > MADSIM_MAX_LIVE_TASKS) return fail(MADSIM_E_ARG, "task_states: task_cap exceeds MADSIM_MAX_LIVE_TASKS");
    }
    if ((logs != nullptr) != (log_cap != 0)) return fail(MADSIM_E_ARG, "trace_seeds: `logs` and log_cap are given together or not at all");
    if ((obs != nullptr) != (obs_cap != 0)) return fail(MADSIM_E_ARG, "trace_seeds: `obs` and obs_cap are given together or not at all");
    if (!single) {
        // what the call asks of the device, per seed: the two rows, the two lengths, the seed and the result
        const uint64_t M = MADSIM_TRACE_MAX_BYTES;
        if (log_cap > M || obs_cap > M / 8 || n > M) return fail(MADSIM_E_LIMITS, "trace_seeds: more than MADSIM_TRACE_MAX_BYTES of device memory");
        const uint64_t per_seed = log_cap + (times ? 16 : 8) * obs_cap + 3 * sizeof(uint64_t) + sizeof(madsim_result_t) + (tr ? 8 * tr->cap : 0);
        if (per_seed > M / n) return fail(MADSIM_E_LIMITS, times ? "timeline_seeds: n x (16 obs_cap + 72) exceeds MADSIM_TRACE_MAX_BYTES: fewer seeds per call, or a smaller obs_cap" :
                                                              tr ? "task_states: n x (8 task_cap + 72) exceeds MADSIM_TRACE_MAX_BYTES: fewer seeds per call, or a smaller task_cap"
                                                              : "trace_seeds: n x (log_cap + 8 obs_cap + 72) exceeds MADSIM_TRACE_MAX_BYTES: fewer seeds per call, or smaller caps");
    }
    CTX_ENTER(c);
    int rc = madsim_geo::validate(w, cfg, &g_err);
    if (rc) return rc;
    Geo G;
    hipStream_t st = nullptr;
    madsim_hip_ctx::TraceSet& S = c->trace[0];
    if ((rc = trace_prepare(c, w, cfg, lim, n, log_cap, obs_cap, S, G, st, tr ? &tr->cap : nullptr, times != nullptr))) return rc;
    uint64_t* d_olen = S.len + n;
    // from here on the stream may hold work on the caller's memory: every step is tried only while all before it succeeded, and the
    // synchronisation is reached whatever happened
    TraceSteps step;
    uint64_t one_len = 0;                                                     // (`single`: the length is needed here, before the log is copied)
    bool ok = step(hipMemcpyAsync(c->d_seeds, seeds, n * sizeof(uint64_t), hipMemcpyHostToDevice, st), "hipMemcpyAsync(seeds)");
    ok = trace_queue(G, S, n, log_cap, obs_cap, !single, st, step, ok);
    if (ok && logs && !single) ok = step(hipMemcpyAsync(logs, S.log, n * log_cap, hipMemcpyDeviceToHost, st), "hipMemcpyAsync(log rows)");
    if (ok && obs) ok = step(hipMemcpyAsync(obs, S.obs, n * obs_cap * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync(observation rows)");
    if (ok && times) ok = step(hipMemcpyAsync(times, S.obs + n * obs_cap, n * obs_cap * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync(time rows)");
    if (ok && single) ok = step(hipMemcpyAsync(&one_len, S.len, sizeof one_len, hipMemcpyDeviceToHost, st), "hipMemcpyAsync(length)");
    if (ok && log_len && !single) ok = step(hipMemcpyAsync(log_len, S.len, n * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync(log lengths)");
    if (ok && obs_len) ok = step(hipMemcpyAsync(obs_len, d_olen, n * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync(observation counts)");
    if (ok && tr && tr->tasks) ok = step(hipMemcpyAsync(tr->tasks, S.task, n * tr->cap * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync(task rows)");
    if (ok && tr && tr->len) ok = step(hipMemcpyAsync(tr->len, S.task_len, n * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync(task counts)");
    if (ok && out) ok = step(hipMemcpyAsync(out, S.out, n * sizeof(madsim_result_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync(results)");
    ok = step(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (step.err != hipSuccess) return fail(MADSIM_E_HIP, std::string(step.at) + ": " + hipGetErrorString(step.err));
    if (step.no_build) return fail(MADSIM_E_LIMITS, "no trace kernel build");
    if (single) {
        if (log_len) *log_len = one_len;
        if (logs && one_len) HIP_TRY(hipMemcpy(logs, S.log, (size_t)std::min(one_len, log_cap), hipMemcpyDeviceToHost));      // (synchronous)
    } else if (out && lim && lim->no_trace_hash) {
        for (uint64_t i = 0; i < n; i++) out[i].trace_hash = 0;
    }
    return 0;
}

// Where two variants of a seed's run first part (include/madsim_hip.h): both sides' trace launches into the context's two buffer sets, the
// compare kernel over them, one copy of the records and one of the context rows, one synchronisation — all on one stream; no row is copied.
// Side B is prepared behind side A's queued launch, as a differential campaign's second side is: the tables of both workloads stay
// uploaded (upload_workload's cache), and scratch that side B outgrows is only replaced once the stream has drained.  Until the final
// copies nothing queued touches the caller's memory but the seed list, so an error of side B's preparation drains the stream and returns.
int madsim_hip_ctx_diverge_seeds(madsim_hip_ctx_t* c, const madsim_workload_t* wA, const madsim_config_t* cfgA, const madsim_limits_t* limA,
                                 const madsim_workload_t* wB, const madsim_config_t* cfgB, const madsim_limits_t* limB, const uint64_t* seeds,
                                 uint64_t n, uint64_t log_cap, uint64_t obs_cap, uint32_t win, madsim_divergence_t* recs, uint64_t* obs_ctx) {
    static_assert(sizeof(madsim_divergence_t) == 184, "record layout");
    if (n == 0) return 0;
    if (!seeds || !recs) return fail(MADSIM_E_ARG, "diverge_seeds: null seed list or record array");
    if (win > MADSIM_DIVERGE_MAX_WIN) return fail(MADSIM_E_ARG, "diverge_seeds: win exceeds MADSIM_DIVERGE_MAX_WIN");
    if ((obs_ctx != nullptr) != (win != 0)) return fail(MADSIM_E_ARG, "diverge_seeds: `obs_ctx` and win are given together or not at all");
    if (win && !obs_cap) return fail(MADSIM_E_ARG, "diverge_seeds: a context window needs observation rows (obs_cap > 0)");
    {
        // what the call asks of the device, per seed: both sides' rows, length words, seed and result, the record and the context row
        const uint64_t M = MADSIM_TRACE_MAX_BYTES;
        const char* const msg = "diverge_seeds: n x (2 (log_cap + 8 obs_cap + 72) + 184 + 24 win) exceeds MADSIM_TRACE_MAX_BYTES: fewer seeds per call, or smaller caps";
        if (log_cap > M || obs_cap > M / 8 || n > M) return fail(MADSIM_E_LIMITS, msg);
        const uint64_t per_seed = 2 * (log_cap + 8 * obs_cap + 3 * sizeof(uint64_t) + sizeof(madsim_result_t)) + sizeof(madsim_divergence_t) + 24ull * win;
        if (per_seed > M / n) return fail(MADSIM_E_LIMITS, msg);
    }
    if (madsim_geo::validate(wA, cfgA, &g_err)) return fail(MADSIM_E_ARG, "side A: " + g_err);      // (an argument error of this call, whatever validate calls it)
    if (madsim_geo::validate(wB, cfgB, &g_err)) return fail(MADSIM_E_ARG, "side B: " + g_err);
    CTX_ENTER(c);
    int rc;
    hipStream_t st = nullptr;
    madsim_hip_ctx::TraceSet &SA = c->trace[0], &SB = c->trace[1];
    Geo GA, GB;
    if ((rc = trace_prepare(c, wA, cfgA, limA, n, log_cap, obs_cap, SA, GA, st))) return fail(rc, "side A: " + g_err);
    HIP_TRY(c->d_drec.room((size_t)n));
    HIP_TRY(c->d_dctx.room((size_t)(3ull * win * n)));
    TraceSteps step;
    bool ok = step(hipMemcpyAsync(c->d_seeds, seeds, n * sizeof(uint64_t), hipMemcpyHostToDevice, st), "hipMemcpyAsync(seeds)");
    ok = trace_queue(GA, SA, n, log_cap, obs_cap, true, st, step, ok);
    if (ok && (rc = trace_prepare(c, wB, cfgB, limB, n, log_cap, obs_cap, SB, GB, st))) {
        const std::string why = "side B: " + g_err;
        (void)hipStreamSynchronize(st);
        return fail(rc, why);
    }
    ok = trace_queue(GB, SB, n, log_cap, obs_cap, true, st, step, ok);
    if (ok) {
        const int refused = madsim_k_launch_diverge(log_cap ? SA.log : nullptr, log_cap ? SB.log : nullptr, log_cap, obs_cap ? SA.obs : nullptr,
                                                    obs_cap ? SB.obs : nullptr, obs_cap, SA.len, SB.len, SA.len + n, SB.len + n, SA.out, SB.out, c->d_seeds, n,
                                                    win, c->d_drec, win ? c->d_dctx : nullptr, st);
        if (refused) step.no_build = true;
        ok = step(refused ? hipSuccess : hipGetLastError(), "diverge kernel launch");
    }
    if (ok) ok = step(hipMemcpyAsync(recs, c->d_drec, n * sizeof(madsim_divergence_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync(records)");
    if (ok && win) ok = step(hipMemcpyAsync(obs_ctx, c->d_dctx, 3ull * win * n * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync(context rows)");
    ok = step(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (step.err != hipSuccess) return fail(MADSIM_E_HIP, std::string(step.at) + ": " + hipGetErrorString(step.err));
    if (step.no_build) return fail(MADSIM_E_LIMITS, "no trace kernel build, or sizes the diverge kernel refuses");
    const bool za = limA && limA->no_trace_hash, zb = limB && limB->no_trace_hash;
    if (za || zb)
        for (uint64_t i = 0; i < n; i++) { if (za) recs[i].a.trace_hash = 0; if (zb) recs[i].b.trace_hash = 0; }
    return 0;
}

// ---- the observation census, the probe-set census and the probe-order census: table size, probe start, the host fold of a chunk, and the chunk loop ----
// One of each for all three.  A form says what is its own: the report and its entries (key, combine, the totals a chunk's words add), its
// argument checks and what an empty report is, the sizes, its kernels' launch, the word that counts runner verdicts and its messages.
namespace {
extern "C++" {
// Which traced values the seeds reach: entries keyed by the value.
struct CensusForm {
    typedef madsim_census_t Report;
    typedef madsim_census_value_t Entry;
    static_assert(sizeof(Entry) == 64 && sizeof(Report) == 144, "record layout");
    Report* r;
    static constexpr uint64_t slot_bytes = MADSIM_K_CENSUS_SLOT_BYTES, min_slots = MADSIM_K_CENSUS_MIN_SLOTS, n_words = MADSIM_K_CENSUS_WORDS;
    static constexpr uint64_t per_seed_bytes = 3 * sizeof(uint64_t) + sizeof(madsim_result_t);      // beside the row: two length words, the seed, the result
    static constexpr uint64_t eager = 64;              // entries copied behind a chunk's words, before their number is known (a probe vocabulary is small: 4 KB)
    static constexpr uint32_t runner_word = 12, err_cap = MADSIM_K_CENSUS_ERR_CAP;
    static constexpr uint64_t fixed_slots = 0;         // the table grows with the caller's cap
    uint64_t dev_cap() const { return r->cap; }        // entries a chunk may write on the device
    static constexpr const char *name = "census", *noun = "census";
    static constexpr const char *at_zero = "hipMemsetAsync(census words)", *at_launch = "census kernel launch", *at_words = "hipMemcpyAsync(census words)",
                                *at_entries = "hipMemcpyAsync(census entries)";
    static constexpr const char* too_big = "census: chunk x (8 obs_cap + 72) + 32 slots + 68 cap + 128 exceeds MADSIM_TRACE_MAX_BYTES, or chunk x obs_cap reaches 2^32 - 1: a smaller chunk or smaller caps";
    static constexpr const char* too_many = "census: more than `cap` distinct observed values (a traced time or random value is not a probe vocabulary): raise cap (max_values), or trace less";
    static auto& bufs(madsim_hip_ctx_t* c) { return c->census; }
    Entry* entries() const { return r->values; }
    uint64_t& count() const { return r->n_values; }
    static uint64_t key(const Entry& e) { return e.value; }
    static void combine(Entry& a, const Entry& b) {
        for (int k = 0; k < 4; k++) a.n_seeds[k] += b.n_seeds[k];
        a.n_total += b.n_total;
        a.first_seed = std::min(a.first_seed, b.first_seed);
        a.max_per_seed = std::max(a.max_per_seed, b.max_per_seed);
    }
    void totals(const unsigned long long* words) const {
        for (int k = 0; k < 4; k++) { r->n_counted[k] += words[2 + k]; r->n_silent[k] += words[6 + k]; }
        r->n_truncated += words[10]; r->n_observations += words[11]; r->n_runner += words[12];
    }
    int check() const {
        if (!r) return fail(MADSIM_E_ARG, "census: null census");
        if (r->include == 0 || (r->include & ~0xfu)) return fail(MADSIM_E_ARG, "census: include is 0 or names a verdict at or above 4 (only PASS, PANIC, DEADLOCK, TIME_LIMIT are counted)");
        if (r->cap == 0 || r->cap > MADSIM_CENSUS_MAX_VALUES || !r->values) return fail(MADSIM_E_ARG, "census: cap outside 1 .. MADSIM_CENSUS_MAX_VALUES, or no value array");
        if (r->obs_cap == 0 || r->obs_cap > MADSIM_CENSUS_MAX_OBS_CAP) return fail(MADSIM_E_ARG, "census: obs_cap outside 1 .. MADSIM_CENSUS_MAX_OBS_CAP");
        if (r->runner_cap && !r->runner_seeds) return fail(MADSIM_E_ARG, "census: runner_cap without runner_seeds");
        return 0;
    }
    void nothing() const {
        r->n_values = r->n_truncated = r->n_observations = r->n_runner = r->n_runner_listed = 0;
        for (int k = 0; k < 4; k++) r->n_counted[k] = r->n_silent[k] = 0;
    }
    int launch(madsim_hip_ctx_t* c, uint64_t n, uint64_t slots, hipStream_t st) const {
        const madsim_hip_ctx::TraceSet& S = c->trace[0];
        auto& C = c->census;
        return madsim_k_launch_census(S.obs, r->obs_cap, S.len + n, S.out, c->d_seeds, n, r->include, C.tab, slots, C.list, r->cap, C.words, C.ent, st);
    }
};

// Which combinations of a vocabulary's values the seeds reach: entries keyed by the set word, one more word per seed on the device.
struct ProbeSetsForm {
    typedef madsim_probe_sets_t Report;
    typedef madsim_probe_set_t Entry;
    static_assert(sizeof(Entry) == 72 && sizeof(Report) == 112, "record layout");
    Report* r;
    static constexpr uint64_t slot_bytes = MADSIM_K_PROBE_SETS_SLOT_BYTES, min_slots = MADSIM_K_PROBE_SETS_MIN_SLOTS, n_words = MADSIM_K_PROBE_SETS_WORDS;
    static constexpr uint64_t per_seed_bytes = 4 * sizeof(uint64_t) + sizeof(madsim_result_t);      // beside the row: two length words, the seed, the set word, the result
    static constexpr uint64_t eager = 56;              // entries copied behind a chunk's words, before their number is known (a handful of sets is the usual report): 4 KB
    static constexpr uint32_t runner_word = 6, err_cap = MADSIM_K_PROBE_SETS_ERR_CAP;
    static constexpr uint64_t fixed_slots = 0;
    uint64_t dev_cap() const { return r->cap; }
    static constexpr const char *name = "probe_sets", *noun = "probe-set";
    static constexpr const char *at_zero = "hipMemsetAsync(probe-set words)", *at_launch = "probe-set kernel launch", *at_words = "hipMemcpyAsync(probe-set words)",
                                *at_entries = "hipMemcpyAsync(probe-set entries)";
    static constexpr const char* too_big = "probe_sets: chunk x (8 obs_cap + 80) + 48 slots + 76 cap + 64 exceeds MADSIM_TRACE_MAX_BYTES, or chunk x obs_cap reaches 2^32 - 1: a smaller chunk or smaller caps";
    static constexpr const char* too_many = "probe_sets: more than `cap` distinct probe sets: raise cap (max_sets), or name fewer values in the vocabulary";
    static auto& bufs(madsim_hip_ctx_t* c) { return c->probe_sets; }
    Entry* entries() const { return r->sets; }
    uint64_t& count() const { return r->n_sets; }
    static uint64_t key(const Entry& e) { return e.set; }
    template <class E>
    static void combine_seeds(E& a, const E& b) {      // per verdict: counts added, the smaller first_seed of the sides that have one
        for (int k = 0; k < 4; k++) {
            if (b.n_seeds[k]) a.first_seed[k] = a.n_seeds[k] ? std::min(a.first_seed[k], b.first_seed[k]) : b.first_seed[k];
            a.n_seeds[k] += b.n_seeds[k];
        }
    }
    static void combine(Entry& a, const Entry& b) { combine_seeds(a, b); }
    void totals(const unsigned long long* words) const {
        for (int k = 0; k < 4; k++) r->n_counted[k] += words[2 + k];
        r->n_runner += words[6];
    }
    int check() const {
        if (!r) return fail(MADSIM_E_ARG, "probe_sets: null report");
        if (r->include == 0 || (r->include & ~0xfu)) return fail(MADSIM_E_ARG, "probe_sets: include is 0 or names a verdict at or above 4 (only PASS, PANIC, DEADLOCK, TIME_LIMIT are counted)");
        if (r->cap == 0 || r->cap > MADSIM_PROBE_SETS_MAX || !r->sets) return fail(MADSIM_E_ARG, "probe_sets: cap outside 1 .. MADSIM_PROBE_SETS_MAX, or no set array");
        if (r->obs_cap == 0 || r->obs_cap > MADSIM_CENSUS_MAX_OBS_CAP) return fail(MADSIM_E_ARG, "probe_sets: obs_cap outside 1 .. MADSIM_CENSUS_MAX_OBS_CAP");
        if (r->n_vocab == 0 || r->n_vocab > MADSIM_PROBE_SETS_MAX_VOCAB || !r->vocab) return fail(MADSIM_E_ARG, "probe_sets: n_vocab outside 1 .. MADSIM_PROBE_SETS_MAX_VOCAB, or no vocabulary");
        for (uint64_t i = 1; i < r->n_vocab; i++)
            for (uint64_t j = 0; j < i; j++)
                if (r->vocab[i] == r->vocab[j]) return fail(MADSIM_E_ARG, "probe_sets: a value occurs twice in the vocabulary");
        if (r->runner_cap && !r->runner_seeds) return fail(MADSIM_E_ARG, "probe_sets: runner_cap without runner_seeds");
        return 0;
    }
    void nothing() const {
        r->n_sets = r->n_runner = r->n_runner_listed = 0;
        for (int k = 0; k < 4; k++) r->n_counted[k] = 0;
    }
    int launch(madsim_hip_ctx_t* c, uint64_t n, uint64_t slots, hipStream_t st) const {
        const madsim_hip_ctx::TraceSet& S = c->trace[0];
        auto& P = c->probe_sets;
        return madsim_k_launch_probe_sets(S.obs, r->obs_cap, S.len + n, S.out, c->d_seeds, n, r->include, r->vocab, r->n_vocab, P.sig, P.tab, slots, P.list,
                                          r->cap, P.words, P.ent, st);
    }
};

// Which vocabulary value comes first: entries keyed by the cell (a, b); a dense matrix of 32 x 32 cells in the table's place, so the
// device's entries number n_vocab^2 at most whatever the caller's cap, and there is no "too many".
struct ProbeOrderForm {
    typedef madsim_probe_order_t Report;
    typedef madsim_probe_order_pair_t Entry;
    static_assert(sizeof(Entry) == 72 && sizeof(Report) == 152, "record layout");
    Report* r;
    static constexpr uint64_t slot_bytes = 32, min_slots = 1024, fixed_slots = 1024, n_words = MADSIM_K_PROBE_ORDER_WORDS;      // a cell: four counts, four witnesses
    static_assert(slot_bytes * fixed_slots == 4 * MADSIM_K_PROBE_ORDER_MATRIX_WORDS, "the matrix");
    static constexpr uint64_t per_seed_bytes = 3 * sizeof(uint64_t) + sizeof(madsim_result_t);      // beside the row: two length words, the seed, the result
    static constexpr uint64_t eager = 56;              // entries copied behind a chunk's words, before their number is known (seven values' full matrix): 4 KB
    static constexpr uint32_t runner_word = 11, err_cap = 0;       // (no cap outcome on the device)
    static constexpr const char *name = "probe_order", *noun = "probe-order";
    static constexpr const char *at_zero = "hipMemsetAsync(probe-order words)", *at_launch = "probe-order kernel launch", *at_words = "hipMemcpyAsync(probe-order words)",
                                *at_entries = "hipMemcpyAsync(probe-order entries)";
    static constexpr const char* too_big = "probe_order: chunk x (8 obs_cap + 72) + 32768 + 76 n_vocab^2 + 96 exceeds MADSIM_TRACE_MAX_BYTES, or chunk x obs_cap reaches 2^32 - 1: a smaller chunk or a smaller obs_cap";
    static constexpr const char* too_many = "probe_order: more cells than n_vocab^2 (internal)";
    static auto& bufs(madsim_hip_ctx_t* c) { return c->probe_order; }
    Entry* entries() const { return r->pairs; }
    uint64_t& count() const { return r->n_pairs; }
    uint64_t dev_cap() const { return r->n_vocab * r->n_vocab; }
    static uint64_t key(const Entry& e) { return (uint64_t)e.a << 32 | e.b; }
    static void combine(Entry& a, const Entry& b) { ProbeSetsForm::combine_seeds(a, b); }
    void totals(const unsigned long long* words) const {
        for (int k = 0; k < 4; k++) { r->n_counted[k] += words[2 + k]; r->n_none[k] += words[6 + k]; }
        r->n_truncated += words[10]; r->n_runner += words[11];
    }
    int check() const {
        if (!r) return fail(MADSIM_E_ARG, "probe_order: null report");
        if (r->include == 0 || (r->include & ~0xfu)) return fail(MADSIM_E_ARG, "probe_order: include is 0 or names a verdict at or above 4 (only PASS, PANIC, DEADLOCK, TIME_LIMIT are counted)");
        if (r->obs_cap == 0 || r->obs_cap > MADSIM_CENSUS_MAX_OBS_CAP) return fail(MADSIM_E_ARG, "probe_order: obs_cap outside 1 .. MADSIM_CENSUS_MAX_OBS_CAP");
        if (r->n_vocab == 0 || r->n_vocab > MADSIM_PROBE_ORDER_MAX_VOCAB || !r->vocab) return fail(MADSIM_E_ARG, "probe_order: n_vocab outside 1 .. MADSIM_PROBE_ORDER_MAX_VOCAB, or no vocabulary");
        for (uint64_t i = 1; i < r->n_vocab; i++)
            for (uint64_t j = 0; j < i; j++)
                if (r->vocab[i] == r->vocab[j]) return fail(MADSIM_E_ARG, "probe_order: a value occurs twice in the vocabulary");
        if (r->cap < r->n_vocab * r->n_vocab || !r->pairs) return fail(MADSIM_E_ARG, "probe_order: cap below n_vocab x n_vocab, or no pair array");
        if (r->runner_cap && !r->runner_seeds) return fail(MADSIM_E_ARG, "probe_order: runner_cap without runner_seeds");
        return 0;
    }
    void nothing() const {
        r->n_pairs = r->n_truncated = r->n_runner = r->n_runner_listed = 0;
        for (int k = 0; k < 4; k++) r->n_counted[k] = r->n_none[k] = 0;
    }
    int launch(madsim_hip_ctx_t* c, uint64_t n, uint64_t, hipStream_t st) const {
        const madsim_hip_ctx::TraceSet& S = c->trace[0];
        auto& P = c->probe_order;
        return madsim_k_launch_probe_order(S.obs, r->obs_cap, S.len + n, S.out, c->d_seeds, n, r->include, r->vocab, r->n_vocab, P.tab, P.words, P.ent, st);
    }
};

uint64_t obs_report_slots(uint64_t cap, uint64_t min_slots) {
    uint64_t slots = min_slots;
    while (slots < 2 * cap) slots <<= 1;
    return slots;
}

// The host fold of one chunk into the caller's report: the chunk's entries sorted and equal keys combined, then merged into the ascending
// array — or -1 with the report untouched when that would pass `cap` —, then the totals of `words` (may be null: none) added.  Everything
// it does commutes, so the order of the chunks and of a chunk's entries never shows.
template <class Form>
int fold_chunk(const Form& f, const unsigned long long* words, const typename Form::Entry* entries, uint64_t n) {
    typedef typename Form::Entry Entry;
    std::vector<Entry> add(entries, entries + n);
    std::sort(add.begin(), add.end(), [](const Entry& a, const Entry& b) { return Form::key(a) < Form::key(b); });
    size_t m = 0;
    for (size_t j = 0; j < add.size(); j++) {
        if (m && Form::key(add[m - 1]) == Form::key(add[j])) Form::combine(add[m - 1], add[j]); else add[m++] = add[j];
    }
    Entry* const v = f.entries();
    const uint64_t have = f.count();
    uint64_t fresh = 0;
    for (size_t i = 0, j = 0; j < m; j++) {
        while (i < have && Form::key(v[i]) < Form::key(add[j])) i++;
        if (i >= have || Form::key(v[i]) != Form::key(add[j])) fresh++;
    }
    if (have + fresh > f.r->cap) return -1;
    for (int64_t i = (int64_t)have - 1, j = (int64_t)m - 1, k = (int64_t)(have + fresh) - 1; j >= 0; k--) {      // merged from the back, in place
        if (i >= 0 && Form::key(v[i]) > Form::key(add[j])) v[k] = v[i--];
        else if (i >= 0 && Form::key(v[i]) == Form::key(add[j])) { Entry e = v[i--]; Form::combine(e, add[j--]); v[k] = e; }
        else v[k] = add[j--];
    }
    f.count() = have + fresh;
    if (words) f.totals(words);
    return 0;
}

// The stall-site census (include/madsim_hip.h): the fourth form of obs_report_run, and the one with TWO passes.  The trace launch keeps the task log in
// the observation log's place; stall_sites_kernel turns the task rows into site rows and shape words; the observation census's launch and host fold
// (CensusForm) run over each — the site pass in buffer group 0, the shape pass (none when the caller gave no shape array) in group 1.
int fold_stall(madsim_stall_census_t* sc, const unsigned long long* words, const madsim_census_value_t* sites, uint64_t n_sites,
               const madsim_census_value_t* shapes, uint64_t n_shapes) {
    madsim_census_t a{}, b{};
    a.values = sc->sites; a.cap = sc->site_cap; a.n_values = sc->n_sites;
    b.values = sc->shapes; b.cap = sc->shape_cap; b.n_values = sc->n_shapes;
    if (fold_chunk(CensusForm{&a}, words, sites, n_sites)) return -1;
    if (n_shapes && fold_chunk(CensusForm{&b}, nullptr, shapes, n_shapes)) return -1;
    sc->n_sites = a.n_values; sc->n_shapes = b.n_values;
    for (int k = 0; k < 4; k++) { sc->n_counted[k] += a.n_counted[k]; sc->n_idle[k] += a.n_silent[k]; }
    sc->n_truncated += a.n_truncated; sc->n_tasks += a.n_observations; sc->n_runner += a.n_runner;
    return 0;
}

struct StallForm {
    typedef madsim_stall_census_t Report;
    typedef madsim_census_value_t Entry;
    static_assert(sizeof(Report) == 168, "record layout");
    Report* r;
    static constexpr uint64_t slot_bytes = MADSIM_K_CENSUS_SLOT_BYTES, min_slots = MADSIM_K_CENSUS_MIN_SLOTS, n_words = MADSIM_K_CENSUS_WORDS;
    // beside the task row and the site row: the count, the shape word and its length word, the trace set's two length words, the seed, the result
    static constexpr uint64_t per_seed_bytes = 6 * sizeof(uint64_t) + sizeof(madsim_result_t);
    static constexpr uint64_t eager = CensusForm::eager;
    static constexpr uint32_t runner_word = CensusForm::runner_word, err_cap = MADSIM_K_CENSUS_ERR_CAP;
    static constexpr uint64_t fixed_slots = 0;
    static constexpr const char *name = "stall_census", *noun = "stall census";
    static constexpr const char *at_zero = "hipMemsetAsync(stall census words)", *at_launch = "stall census kernel launch", *at_words = "hipMemcpyAsync(stall census words)",
                                *at_entries = "hipMemcpyAsync(stall census entries)";
    static constexpr const char* too_big = "stall_census: chunk x (16 task_cap + 96) + per pass 32 slots + 68 cap + 128 exceeds MADSIM_TRACE_MAX_BYTES: a smaller chunk or smaller caps";
    static constexpr const char* too_many = "stall_census: more than site_cap distinct sites or more than shape_cap distinct shapes: raise max_sites / max_shapes";
    int check() const {
        if (!r) return fail(MADSIM_E_ARG, "stall_census: null report");
        if (r->include == 0 || (r->include & ~0xfu)) return fail(MADSIM_E_ARG, "stall_census: include is 0 or names a verdict at or above 4 (only PASS, PANIC, DEADLOCK, TIME_LIMIT are counted)");
        if (r->task_cap == 0 || r->task_cap > MADSIM_MAX_LIVE_TASKS) return fail(MADSIM_E_ARG, "stall_census: task_cap outside 1 .. MADSIM_MAX_LIVE_TASKS");
        if (r->site_cap == 0 || r->site_cap > MADSIM_CENSUS_MAX_VALUES || !r->sites) return fail(MADSIM_E_ARG, "stall_census: site_cap outside 1 .. MADSIM_CENSUS_MAX_VALUES, or no site array");
        if ((r->shapes != nullptr) != (r->shape_cap != 0) || r->shape_cap > MADSIM_CENSUS_MAX_VALUES)
            return fail(MADSIM_E_ARG, "stall_census: `shapes` and shape_cap are given together or not at all, shape_cap at most MADSIM_CENSUS_MAX_VALUES");
        if (r->runner_cap && !r->runner_seeds) return fail(MADSIM_E_ARG, "stall_census: runner_cap without runner_seeds");
        return 0;
    }
    void nothing() const {
        r->n_sites = r->n_shapes = r->n_truncated = r->n_tasks = r->n_runner = r->n_runner_listed = 0;
        for (int k = 0; k < 4; k++) r->n_counted[k] = r->n_idle[k] = 0;
    }
};

// Probe spans (include/madsim_hip.h): the fifth form of obs_report_run.  The trace launch keeps the time log beside the observation log; the
// chunk's "entries" are its n_spans device records (sim_kernel.h), always all of them, decoded and merged by fold_spans: there is no table, no
// cap outcome and no "too many".
void span_init(madsim_span_t* sp) {
    memset(sp, 0, sizeof *sp);
    sp->min = sp->min_seed = sp->max_seed = sp->first_open_seed = UINT64_MAX;
}

int fold_spans(madsim_probe_spans_t* ps, const unsigned long long* words, const madsim_k_span_rec_t* recs, uint64_t n) {
    if (n != ps->n_spans) return -1;
    for (uint64_t s = 0; s < n; s++) {
        const unsigned long long* const w = recs[s].w;
        madsim_span_t& sp = ps->spans[s];
        uint64_t open = 0;
        for (int v = 0; v < 4; v++) {
            for (int q = 0; q < 4; q++) sp.n_state[v * 4 + q] += w[v * 4 + q];
            open += w[v * 4 + MADSIM_SPAN_OPEN];
        }
        if (w[16]) {                                                                 // closed seeds: the chunk's extremes against the report's, the smaller seed on a tie
            const uint64_t mn = ~w[17], mx = w[18], mn_seed = ~w[21], mx_seed = ~w[22];
            if (mn < sp.min || (mn == sp.min && mn_seed < sp.min_seed)) { sp.min = mn; sp.min_seed = mn_seed; }
            if (mx > sp.max || (mx == sp.max && mx_seed < sp.max_seed)) { sp.max = mx; sp.max_seed = mx_seed; }
            sp.n += w[16];
            unsigned __int128 sum = ((unsigned __int128)sp.sum_hi << 64) | sp.sum_lo;
            sum += (unsigned __int128)w[19] + ((unsigned __int128)w[20] << 32);
            sp.sum_lo = (uint64_t)sum; sp.sum_hi = (uint64_t)(sum >> 64);
            for (int b = 0; b < 256; b++) sp.hist[b] += w[24 + b];
        }
        if (open) sp.first_open_seed = std::min<uint64_t>(sp.first_open_seed, ~w[23]);
    }
    if (words) {
        for (int k = 0; k < 4; k++) ps->n_counted[k] += words[2 + k];
        ps->n_truncated += words[6]; ps->n_runner += words[7];
    }
    return 0;
}

struct SpansForm {
    typedef madsim_probe_spans_t Report;
    typedef madsim_k_span_rec_t Entry;
    static_assert(sizeof(Entry) == 2240 && sizeof(madsim_span_t) == 2240 && sizeof(Report) == 104 && sizeof(madsim_span_def_t) == 24, "record layout");
    Report* r;
    static constexpr uint64_t slot_bytes = 4, min_slots = 1, fixed_slots = 1, n_words = MADSIM_K_PROBE_SPANS_WORDS;      // (no table: one word of it)
    // beside the two rows: two length words, the seed, the result, and per span a state word and a duration
    static constexpr uint64_t per_seed_bytes = 3 * sizeof(uint64_t) + sizeof(madsim_result_t) + 12 * MADSIM_PROBE_SPANS_MAX;
    static constexpr uint64_t eager = MADSIM_PROBE_SPANS_MAX;         // every record rides behind the words
    static constexpr uint32_t runner_word = 7, err_cap = 0;
    static constexpr const char *name = "probe_spans", *noun = "probe-span";
    static constexpr const char *at_zero = "hipMemsetAsync(probe-span words)", *at_launch = "probe-span kernel launch", *at_words = "hipMemcpyAsync(probe-span words)",
                                *at_entries = "hipMemcpyAsync(probe-span records)";
    static constexpr const char* too_big = "probe_spans: chunk x (16 obs_cap + 72 + 12 n_spans) + 2240 n_spans + 64 exceeds MADSIM_TRACE_MAX_BYTES, or chunk x obs_cap reaches 2^32 - 1: a smaller chunk or a smaller obs_cap";
    static constexpr const char* too_many = "probe_spans: a chunk came back without its records (internal)";
    static auto& bufs(madsim_hip_ctx_t* c) { return c->probe_spans; }
    uint64_t dev_cap() const { return r->n_spans; }
    int check() const {
        if (!r) return fail(MADSIM_E_ARG, "probe_spans: null report");
        if (r->include == 0 || (r->include & ~0xfu)) return fail(MADSIM_E_ARG, "probe_spans: include is 0 or names a verdict at or above 4 (only PASS, PANIC, DEADLOCK, TIME_LIMIT are counted)");
        if (r->obs_cap == 0 || r->obs_cap > MADSIM_CENSUS_MAX_OBS_CAP) return fail(MADSIM_E_ARG, "probe_spans: obs_cap outside 1 .. MADSIM_CENSUS_MAX_OBS_CAP");
        if (r->n_spans == 0 || r->n_spans > MADSIM_PROBE_SPANS_MAX || !r->defs || !r->spans) return fail(MADSIM_E_ARG, "probe_spans: n_spans outside 1 .. MADSIM_PROBE_SPANS_MAX, or no definition or record array");
        for (uint64_t s = 0; s < r->n_spans; s++)
            if (r->defs[s].flags & ~MADSIM_SPAN_FROM_START) return fail(MADSIM_E_ARG, "probe_spans: a definition carries a flag other than MADSIM_SPAN_FROM_START");
        if (r->runner_cap && !r->runner_seeds) return fail(MADSIM_E_ARG, "probe_spans: runner_cap without runner_seeds");
        return 0;
    }
    void nothing() const {
        r->n_truncated = r->n_runner = r->n_runner_listed = 0;
        for (int k = 0; k < 4; k++) r->n_counted[k] = 0;
        for (uint64_t s = 0; s < r->n_spans; s++) span_init(&r->spans[s]);
    }
};

// What obs_report_run asks of a form beyond its own members: how many passes it makes (each with a buffer group, a cap, a table, words and entries of
// its own), what a seed's rows weigh, which log the trace launch keeps, its kernels' launch and its host fold.  One pass over the observation rows for
// the three observation forms; the stall census specialises it.
template <class Form> struct Passes {
    static constexpr int max = 1;
    static constexpr bool task_log = false, time_log = false;
    static int count(const Form&) { return 1; }
    static uint64_t row_cap(const Form& f) { return f.r->obs_cap; }
    static uint64_t row_bytes(uint64_t row_cap) { return 8 * row_cap; }
    static uint64_t cap(const Form& f, int) { return f.dev_cap(); }
    static auto& bufs(madsim_hip_ctx_t* c, int) { return Form::bufs(c); }
    static int ensure_rows(madsim_hip_ctx_t*, uint64_t, uint64_t, hipStream_t) { return 0; }
    static int launch(const Form& f, madsim_hip_ctx_t* c, uint64_t n, const uint64_t* slots, hipStream_t st) { return f.launch(c, n, slots[0], st); }
    static int fold(const Form& f, const unsigned long long* const* W, typename Form::Entry* const* E, const uint64_t* ne) { return fold_chunk(f, W[0], E[0], ne[0]); }
};
template <> struct Passes<StallForm> {
    static constexpr int max = 2;
    static constexpr bool task_log = true, time_log = false;
    static int count(const StallForm& f) { return f.r->shape_cap ? 2 : 1; }
    static uint64_t row_cap(const StallForm& f) { return f.r->task_cap; }
    static uint64_t row_bytes(uint64_t row_cap) { return 16 * row_cap; }      // the task row and the site row
    static uint64_t cap(const StallForm& f, int p) { return p ? f.r->shape_cap : f.r->site_cap; }
    static auto& bufs(madsim_hip_ctx_t* c, int p) { return p ? c->stall.shapes : c->stall.sites; }
    static int ensure_rows(madsim_hip_ctx_t* c, uint64_t chunk, uint64_t task_cap, hipStream_t st) {
        HIP_TRY(c->stall.rows.room((size_t)(chunk * task_cap), st));
        HIP_TRY(c->stall.shape.room((size_t)chunk, st));
        HIP_TRY(c->stall.ones.room((size_t)chunk, st));
        return 0;
    }
    static int launch(const StallForm& f, madsim_hip_ctx_t* c, uint64_t n, const uint64_t* slots, hipStream_t st) {
        const madsim_hip_ctx::TraceSet& S = c->trace[0];
        auto& B = c->stall;
        const madsim_stall_census_t* r = f.r;
        if (int rc = madsim_k_launch_stall_sites(S.task, r->task_cap, S.task_len, S.out, n, B.rows, B.shape, B.ones, st)) return rc;
        if (int rc = madsim_k_launch_census(B.rows, r->task_cap, S.task_len, S.out, c->d_seeds, n, r->include, B.sites.tab, slots[0], B.sites.list, r->site_cap,
                                            B.sites.words, B.sites.ent, st)) return rc;
        if (!r->shape_cap) return 0;
        return madsim_k_launch_census(B.shape, 1, B.ones, S.out, c->d_seeds, n, r->include, B.shapes.tab, slots[1], B.shapes.list, r->shape_cap, B.shapes.words,
                                      B.shapes.ent, st);
    }
    static int fold(const StallForm& f, const unsigned long long* const* W, madsim_census_value_t* const* E, const uint64_t* ne) {
        return fold_stall(f.r, W[0], E[0], ne[0], E[1], ne[1]);
    }
};

template <> struct Passes<SpansForm> {
    static constexpr int max = 1;
    static constexpr bool task_log = false, time_log = true;
    static int count(const SpansForm&) { return 1; }
    static uint64_t row_cap(const SpansForm& f) { return f.r->obs_cap; }
    static uint64_t row_bytes(uint64_t row_cap) { return 16 * row_cap; }      // the observation row and the time row
    static uint64_t cap(const SpansForm& f, int) { return f.dev_cap(); }
    static auto& bufs(madsim_hip_ctx_t* c, int) { return c->probe_spans; }
    static int ensure_rows(madsim_hip_ctx_t* c, uint64_t chunk, uint64_t, hipStream_t st) {
        HIP_TRY(c->probe_spans.st.room((size_t)(chunk * MADSIM_PROBE_SPANS_MAX), st));
        HIP_TRY(c->probe_spans.dur.room((size_t)(chunk * MADSIM_PROBE_SPANS_MAX), st));
        return 0;
    }
    static int launch(const SpansForm& f, madsim_hip_ctx_t* c, uint64_t n, const uint64_t*, hipStream_t st) {
        const madsim_hip_ctx::TraceSet& S = c->trace[0];
        auto& B = c->probe_spans;
        return madsim_k_launch_probe_spans(S.obs, S.obs + n * f.r->obs_cap, f.r->obs_cap, S.len + n, S.out, c->d_seeds, n, f.r->include, f.r->defs, f.r->n_spans, B.st, B.dur, B.ent,
                                           B.words, st);
    }
    static int fold(const SpansForm& f, const unsigned long long* const* W, madsim_k_span_rec_t* const* E, const uint64_t* ne) { return fold_spans(f.r, W[0], E[0], ne[0]); }
};

// The report over [seed0, seed0 + total) (seeds == nullptr) or over seeds[0 .. total): chunk after chunk on one stream, each the trace launch
// into the context's trace set 0, the form's kernels and, per pass, the copies of the words and of the first Form::eager entries, then one
// synchronisation: the chunk of a probe vocabulary is done there.  Entries beyond those — and, where the caller still wants runner seeds and
// the chunk has some, its results — follow by copies of their own.  Once a chunk is queued no error returns before its synchronisation
// (TraceSteps); an error that may have left a table otherwise than zero marks the tables dirty; every failure leaves an empty report.
template <class Form>
int obs_report_run(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, const uint64_t* seeds, uint64_t total,
                   uint64_t chunk, const madsim_limits_t* lim, typename Form::Report* rep, bool list) {
    typedef typename Form::Entry Entry;
    typedef Passes<Form> P;
    const Form f{rep};
    const std::string name = Form::name, noun = Form::noun;
    if (int rc = f.check()) return rc;
    if (list && total && !seeds) return fail(MADSIM_E_ARG, name + "_seeds: null seed list");
    if (list)
        for (uint64_t i = 1; i < total; i++)
            if (seeds[i] <= seeds[i - 1]) return fail(MADSIM_E_ARG, name + "_seeds: the seed list is not strictly ascending (sort and deduplicate it first)");
    f.nothing();
    if (total == 0) return 0;
    // what a chunk asks of the device: per seed the rows and the form's words beside them; once per pass the table, the list, the entries, the words
    // (cap: the entries a chunk may write on the device — the caller's cap, or for the dense matrix its cells)
    const int np = P::count(f);
    const uint64_t M = MADSIM_TRACE_MAX_BYTES, row_cap = P::row_cap(f);
    uint64_t cap[P::max] = {}, slots[P::max] = {}, fixed = 0;
    for (int p = 0; p < np; p++) {
        cap[p] = P::cap(f, p);
        slots[p] = Form::fixed_slots ? Form::fixed_slots : obs_report_slots(cap[p], Form::min_slots);
        fixed += slots[p] * Form::slot_bytes + cap[p] * (sizeof(uint32_t) + sizeof(Entry)) + Form::n_words * 8;
    }
    const uint64_t per_seed = P::row_bytes(row_cap) + Form::per_seed_bytes;
    const uint64_t fits = fixed < M ? std::min<uint64_t>((M - fixed) / per_seed, 0xffffffffull / row_cap - 1) : 0;
    if (chunk == 0) chunk = std::min<uint64_t>(65536, fits);
    if (chunk == 0 || chunk > fits) return fail(MADSIM_E_LIMITS, Form::too_big);
    chunk = std::min(chunk, total);
    int rc = madsim_geo::validate(w, cfg, &g_err);
    if (rc) return rc;
    CTX_ENTER(c);
    hipStream_t st = nullptr;
    madsim_hip_ctx::TraceSet& S = c->trace[0];
    auto& B0 = P::bufs(c, 0);                      // (the range form's seed slice and a chunk's results are staged in the first group)
    const auto failed = [&f](int code, const std::string& msg) { f.nothing(); return fail(code, msg); };
    const auto dirty = [&] { for (int p = 0; p < np; p++) P::bufs(c, p).dirty = true; };
    const uint64_t obs_cap = P::task_log ? 0 : row_cap;
    for (uint64_t done = 0; done < total; done += chunk) {
        const uint64_t n = std::min(chunk, total - done);
        Geo G;
        if ((rc = trace_prepare(c, w, cfg, lim, n, 0, obs_cap, S, G, st, P::task_log ? &row_cap : nullptr, P::time_log))) { f.nothing(); return rc; }
        for (int p = 0; p < np; p++)
            if ((rc = P::bufs(c, p).ensure(slots[p], cap[p], chunk, !list && p == 0, st))) { f.nothing(); return rc; }
        if ((rc = P::ensure_rows(c, chunk, row_cap, st))) { f.nothing(); return rc; }
        const uint64_t* src = list ? seeds + done : B0.h_seeds.p;
        if (!list) for (uint64_t i = 0; i < n; i++) B0.h_seeds.p[i] = seed0 + done + i;
        TraceSteps step;
        bool ok = step(hipMemcpyAsync(c->d_seeds, src, n * sizeof(uint64_t), hipMemcpyHostToDevice, st), "hipMemcpyAsync(seeds)");
        for (int p = 0; p < np; p++)
            if (ok) ok = step(hipMemsetAsync(P::bufs(c, p).words, 0, Form::n_words * sizeof(unsigned long long), st), Form::at_zero);
        ok = trace_queue(G, S, n, 0, obs_cap, true, st, step, ok);
        if (ok) {
            const int refused = P::launch(f, c, n, slots, st);
            if (refused) step.no_build = true;
            ok = step(refused ? hipSuccess : hipGetLastError(), Form::at_launch);
        }
        // the first entries ride behind the words; a chunk with more gets the rest in a copy of its own
        uint64_t eager[P::max] = {};
        for (int p = 0; p < np; p++) {
            auto& B = P::bufs(c, p);
            eager[p] = std::min<uint64_t>(cap[p], Form::eager);
            if (ok) ok = step(hipMemcpyAsync(B.h_words, B.words, Form::n_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, st), Form::at_words);
            if (ok) ok = step(hipMemcpyAsync(B.h_ent, B.ent, eager[p] * sizeof(Entry), hipMemcpyDeviceToHost, st), Form::at_entries);
        }
        ok = step(hipStreamSynchronize(st), "hipStreamSynchronize");
        if (step.err != hipSuccess) { dirty(); return failed(MADSIM_E_HIP, std::string(step.at) + ": " + hipGetErrorString(step.err)); }
        if (step.no_build) return failed(MADSIM_E_LIMITS, "no trace kernel build, or sizes the " + noun + " kernels refuse");
        const unsigned long long* W[P::max] = {};
        Entry* E[P::max] = {};
        uint64_t ne[P::max] = {};
        unsigned long long err = 0;
        for (int p = 0; p < np; p++) { W[p] = P::bufs(c, p).h_words; E[p] = P::bufs(c, p).h_ent.p; err |= W[p][1]; }
        if (err & Form::err_cap) return failed(MADSIM_E_LIMITS, Form::too_many);      // (the extract pass has cleared the table)
        if (err) { dirty(); return failed(MADSIM_E_HIP, name + ": the device table was not clean (internal)"); }
        for (int p = 0; p < np; p++) {
            auto& B = P::bufs(c, p);
            ne[p] = W[p][0];
            if (ne[p] > eager[p]) {
                const hipError_t e = hipMemcpy(B.h_ent + eager[p], B.ent + eager[p], (ne[p] - eager[p]) * sizeof(Entry), hipMemcpyDeviceToHost);
                if (e != hipSuccess) return failed(MADSIM_E_HIP, "hipMemcpy(" + noun + " entries): " + hipGetErrorString(e));
            }
        }
        if (P::fold(f, W, E, ne)) return failed(MADSIM_E_LIMITS, Form::too_many);
        if (W[0][Form::runner_word] && rep->n_runner_listed < rep->runner_cap) {      // chunks and seeds ascend: the first runner_cap met are the smallest
            hipError_t e = B0.h_res.room((size_t)chunk);
            if (e == hipSuccess) e = hipMemcpy(B0.h_res, S.out, n * sizeof(madsim_result_t), hipMemcpyDeviceToHost);
            if (e != hipSuccess) return failed(MADSIM_E_HIP, "hipMemcpy(" + noun + " results): " + hipGetErrorString(e));
            for (uint64_t i = 0; i < n && rep->n_runner_listed < rep->runner_cap; i++)
                if (MADSIM_IS_RUNNER_VERDICT(B0.h_res.p[i].verdict)) rep->runner_seeds[rep->n_runner_listed++] = list ? seeds[done + i] : seed0 + done + i;
        }
    }
    return 0;
}
}  // extern "C++"
}  // namespace

extern "C" uint64_t madsim_k_census_slots(uint64_t cap) { return obs_report_slots(cap, MADSIM_K_CENSUS_MIN_SLOTS); }
extern "C" uint64_t madsim_k_probe_sets_slots(uint64_t cap) { return obs_report_slots(cap, MADSIM_K_PROBE_SETS_MIN_SLOTS); }
extern "C" uint64_t madsim_k_census_slot(uint64_t value, uint64_t slots) { return madsim_k::census_slot(value, slots); }

// Declared in sim_kernel.h beside the launchers (not part of the public ABI): the tests feed them entries without a device.
extern "C" int madsim_k_fold_census(madsim_census_t* cen, const unsigned long long* words, const madsim_census_value_t* entries, uint64_t n) {
    return fold_chunk(CensusForm{cen}, words, entries, n);
}
extern "C" int madsim_k_fold_probe_sets(madsim_probe_sets_t* ps, const unsigned long long* words, const madsim_probe_set_t* entries, uint64_t n) {
    return fold_chunk(ProbeSetsForm{ps}, words, entries, n);
}
extern "C" int madsim_k_fold_probe_order(madsim_probe_order_t* po, const unsigned long long* words, const madsim_probe_order_pair_t* entries, uint64_t n) {
    return fold_chunk(ProbeOrderForm{po}, words, entries, n);
}

extern "C" int madsim_k_fold_probe_spans(madsim_probe_spans_t* ps, const unsigned long long* words, const madsim_k_span_rec_t* recs, uint64_t n) {
    return fold_spans(ps, words, recs, n);
}
extern "C" void madsim_k_span_init(madsim_span_t* span) { span_init(span); }

extern "C" int madsim_k_fold_stall_census(madsim_stall_census_t* sc, const unsigned long long* words, const madsim_census_value_t* sites, uint64_t n_sites,
                                          const madsim_census_value_t* shapes, uint64_t n_shapes) {
    return fold_stall(sc, words, sites, n_sites, shapes, n_shapes);
}

int madsim_hip_ctx_probe_spans_range(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total,
                                     uint64_t chunk, const madsim_limits_t* lim, madsim_probe_spans_t* ps) {
    return obs_report_run<SpansForm>(c, w, cfg, seed0, nullptr, total, chunk, lim, ps, false);
}

int madsim_hip_ctx_probe_spans_seeds(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n,
                                     uint64_t chunk, const madsim_limits_t* lim, madsim_probe_spans_t* ps) {
    return obs_report_run<SpansForm>(c, w, cfg, 0, seeds, n, chunk, lim, ps, true);
}

int madsim_hip_ctx_stall_census_range(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total,
                                      uint64_t chunk, const madsim_limits_t* lim, madsim_stall_census_t* sc) {
    return obs_report_run<StallForm>(c, w, cfg, seed0, nullptr, total, chunk, lim, sc, false);
}

int madsim_hip_ctx_stall_census_seeds(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n,
                                      uint64_t chunk, const madsim_limits_t* lim, madsim_stall_census_t* sc) {
    return obs_report_run<StallForm>(c, w, cfg, 0, seeds, n, chunk, lim, sc, true);
}

int madsim_hip_ctx_census_range(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total,
                                uint64_t chunk, const madsim_limits_t* lim, madsim_census_t* cen) {
    return obs_report_run<CensusForm>(c, w, cfg, seed0, nullptr, total, chunk, lim, cen, false);
}

int madsim_hip_ctx_census_seeds(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n,
                                uint64_t chunk, const madsim_limits_t* lim, madsim_census_t* cen) {
    return obs_report_run<CensusForm>(c, w, cfg, 0, seeds, n, chunk, lim, cen, true);
}

int madsim_hip_ctx_probe_sets_range(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total,
                                    uint64_t chunk, const madsim_limits_t* lim, madsim_probe_sets_t* ps) {
    return obs_report_run<ProbeSetsForm>(c, w, cfg, seed0, nullptr, total, chunk, lim, ps, false);
}

int madsim_hip_ctx_probe_sets_seeds(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n,
                                    uint64_t chunk, const madsim_limits_t* lim, madsim_probe_sets_t* ps) {
    return obs_report_run<ProbeSetsForm>(c, w, cfg, 0, seeds, n, chunk, lim, ps, true);
}

int madsim_hip_ctx_probe_order_range(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total,
                                     uint64_t chunk, const madsim_limits_t* lim, madsim_probe_order_t* po) {
    return obs_report_run<ProbeOrderForm>(c, w, cfg, seed0, nullptr, total, chunk, lim, po, false);
}

int madsim_hip_ctx_probe_order_seeds(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n,
                                     uint64_t chunk, const madsim_limits_t* lim, madsim_probe_order_t* po) {
    return obs_report_run<ProbeOrderForm>(c, w, cfg, 0, seeds, n, chunk, lim, po, true);
}

int madsim_hip_ctx_trace_seeds(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n,
                               const madsim_limits_t* lim, uint8_t* logs, uint64_t log_cap, uint64_t* obs, uint64_t obs_cap,
                               uint64_t* log_len, uint64_t* obs_len, madsim_result_t* out) {
    return trace_list(c, w, cfg, seeds, n, lim, logs, log_cap, obs, obs_cap, log_len, obs_len, out, false);
}

// Where the listed seeds' tasks stand when their runs end (include/madsim_hip.h "Task post-mortems"): the trace launch of trace_list with the task log
// and neither of the other two.
int madsim_hip_ctx_task_states(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n,
                               const madsim_limits_t* lim, uint64_t* tasks, uint64_t task_cap, uint64_t* task_len, madsim_result_t* out) {
    const TaskRows tr{tasks, task_cap, task_len};
    return trace_list(c, w, cfg, seeds, n, lim, nullptr, 0, nullptr, 0, nullptr, nullptr, out, false, &tr);
}

// When the listed seeds traced what they traced (include/madsim_hip.h "Timelines"): trace_list's launch with the time log beside the observation log.
int madsim_hip_ctx_timeline_seeds(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n,
                                  const madsim_limits_t* lim, uint64_t* obs, uint64_t* times, uint64_t obs_cap, uint64_t* obs_len, madsim_result_t* out) {
    if (n && (!obs || !times || !obs_cap)) return fail(MADSIM_E_ARG, "timeline_seeds: needs the observation rows, the time rows and obs_cap > 0");
    return trace_list(c, w, cfg, seeds, n, lim, nullptr, 0, obs, obs_cap, nullptr, obs_len, out, false, nullptr, times);
}

// Two span records over disjoint seed sets as one (include/madsim_hip.h).  No device involved.
void madsim_hip_span_merge(madsim_span_t* into, const madsim_span_t* from) {
    if (!into || !from) return;
    madsim_span_t& a = *into;
    const madsim_span_t& b = *from;
    for (int q = 0; q < 16; q++) a.n_state[q] += b.n_state[q];
    if (b.n) {
        if (b.min < a.min || (b.min == a.min && b.min_seed < a.min_seed)) { a.min = b.min; a.min_seed = b.min_seed; }
        if (b.max > a.max || (b.max == a.max && b.max_seed < a.max_seed)) { a.max = b.max; a.max_seed = b.max_seed; }
        a.n += b.n;
        const unsigned __int128 sum = (((unsigned __int128)a.sum_hi << 64) | a.sum_lo) + (((unsigned __int128)b.sum_hi << 64) | b.sum_lo);
        a.sum_lo = (uint64_t)sum; a.sum_hi = (uint64_t)(sum >> 64);
        for (int k = 0; k < 256; k++) a.hist[k] += b.hist[k];
    }
    a.first_open_seed = std::min(a.first_open_seed, b.first_open_seed);
}

// The shape of a task table: the sum of mix(site) over its records, mix = splitmix64's finaliser (include/madsim_hip.h).  No device involved.
uint64_t madsim_hip_stall_shape(const uint64_t* tasks, uint64_t n) {
    uint64_t s = 0;
    for (uint64_t i = 0; tasks && i < n; i++) {
        uint64_t z = MADSIM_TASK_SITE(tasks[i]);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        s += z ^ (z >> 31);
    }
    return s;
}

// One seed of the list form.  (What it always did: at most min(length, cap) bytes of `log` are written, and a null `log` or a zero cap asks
// for the length alone.)
int64_t madsim_hip_ctx_trace_seed(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed,
                                  const madsim_limits_t* lim, uint8_t* log, uint64_t cap, madsim_result_t* out) {
    if (!log || !cap) { log = nullptr; cap = 0; }
    uint64_t len = 0;
    int rc = trace_list(c, w, cfg, &seed, 1, lim, log, cap, nullptr, 0, &len, nullptr, out, true);
    return rc ? rc : (int64_t)len;
}

int64_t madsim_hip_ctx_observe_seed(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed,
                                    const madsim_limits_t* lim, uint64_t* obs, uint64_t cap, madsim_result_t* out) {
    uint64_t len = 0;
    int rc = madsim_hip_ctx_trace_seeds(c, w, cfg, &seed, 1, lim, nullptr, 0, obs, cap, nullptr, &len, out);
    return rc ? rc : (int64_t)len;
}

// ---- one process, several GPUs -----------------------------------------------------------------------------------------
// Builder::run drives every seed from one process (builder.rs:129-150): shard [seed0, seed0 + count) contiguously over
// the contexts (context g gets [g * ceil(count / n), ...), the rule of madsim_amd/dist.py::shard_range) and run every share
// as sub-batches kept in flight on that device's own streams (run_pipelined: kernels and device-to-host copies of all devices
// queued from this one host thread, page-locked staging so the copies overlap), then fold the reports on the host.
// Why a host fold and not the RCCL gather BASELINE.json's north_star names: the per-seed results travel to the caller's host
// array anyway (Builder::run needs the failing seed's result), so the only thing a collective could carry is n <= 8 reports
// of 32 bytes that the host already holds; a single-process communicator (ncclCommInitAll) plus one collective launch per
// batch would add a dependency and a synchronisation, not remove one.  The RCCL gather lives where ranks really are
// separate processes: bench.py / madsim_amd/dist.py (one process per GPU, one 64-byte all-gather per batch).
// Robustness: context locks are taken in address order (two threads passing the same contexts in different orders cannot
// deadlock); once the first kernel is in flight no error returns before EVERY launched stream has been synchronised; the
// compacted re-runs of runner verdicts go round-robin over the contexts.
int madsim_hip_run_batch_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                               uint64_t seed0, uint64_t count, const madsim_limits_t* lim, madsim_result_t* out,
                               madsim_summary_t* summary, int max_rounds) {
    auto t0 = std::chrono::steady_clock::now();
    if (!out && count) return fail(MADSIM_E_ARG, "run_batch_multi needs the result array");
    int rc = madsim_geo::validate(w, cfg, &g_err);             // (before any lock is taken)
    if (rc) return rc;
    std::vector<std::unique_lock<std::mutex>> locks;
    if ((rc = lock_contexts(ctxs, n_ctx, "run_batch_multi", locks))) return rc;
    // 1 + 2. every device's sub-batches and their device-to-host copies are queued from this thread, each device keeping as many
    //        in flight as the workload's occupancy rewards; finished sub-batches move into the caller's array while the rest run
    double kernel_ms = 0.0;
    if ((rc = run_pipelined(ctxs, n_ctx, w, cfg, seed0, count, lim, out, nullptr, &kernel_ms))) return rc;
    // 3. runner verdicts (capacity / step cap) from every shard: one compacted re-launch per round, round-robin over the devices
    if ((rc = rerun_runner_verdicts(ctxs, n_ctx, w, cfg, seed0, count, lim, out, max_rounds, &kernel_ms))) return rc;
    // 4. fold
    if (summary) { host_summary(out, seed0, count, summary); summary->kernel_ms = kernel_ms; summary->wall_s = since(t0); }
    return 0;
}

// ---- campaign statistics: the bucket rule and the host fold of a batch's report --------------------------------------------
uint32_t madsim_hip_stat_bucket(uint64_t v) {
    if (v < 4) return (uint32_t)v;
    const uint32_t e = 63u - (uint32_t)__builtin_clzll(v);
    return 4u * (e - 1u) + ((uint32_t)(v >> (e - 2u)) & 3u);
}

uint64_t madsim_hip_stat_bucket_floor(uint32_t b) {
    if (b < 4) return b;
    return b >= 252 ? UINT64_MAX : (uint64_t)(4 + b % 4) << (b / 4 - 1);
}

// s = a batch's MADSIM_K_STATS_WORDS (sim_kernel.hip): batches are folded in seed order, but nothing here relies on it — count, min, max and
// the sums commute, and the extreme seeds are merged under the total order (value descending, seed ascending).  Declared in sim_kernel.h
// beside the launchers (not part of the public ABI): the tests feed it synthetic words without a device.
extern "C" void madsim_k_fold_stats(madsim_stats_t* st, const unsigned long long* s) {
    const uint64_t n = s[0];
    if (!n) return;
    const uint32_t* hist = reinterpret_cast<const uint32_t*>(s + 17);
    const madsim_extreme_t* top = reinterpret_cast<const madsim_extreme_t*>(s + 17 + MADSIM_STAT_METRICS * MADSIM_STAT_BUCKETS / 2);
    const uint64_t K = st->top_k, have = st->n_top, got = std::min(K, n), keep = std::min(K, have + got);
    for (uint32_t m = 0; m < MADSIM_STAT_METRICS; m++) {
        madsim_metric_t& M = st->metric[m];
        M.min = std::min<uint64_t>(M.min, ~s[1 + m]);
        M.max = std::max<uint64_t>(M.max, s[5 + m]);
        const unsigned __int128 sum = ((unsigned __int128)M.sum_hi << 64 | M.sum_lo) + s[9 + m] + ((unsigned __int128)s[13 + m] << 32);
        M.sum_lo = (uint64_t)sum; M.sum_hi = (uint64_t)(sum >> 64);
        for (uint32_t b = 0; b < MADSIM_STAT_BUCKETS; b++) M.hist[b] += hist[m * MADSIM_STAT_BUCKETS + b];
        if (!K) continue;
        madsim_extreme_t* row = st->top + m * K;
        const madsim_extreme_t* add = top + m * MADSIM_STAT_MAX_TOP;
        madsim_extreme_t merged[MADSIM_STAT_MAX_TOP];
        for (uint64_t i = 0, a = 0, b = 0; i < keep; i++) {
            const bool from_row = b >= got || (a < have && (row[a].value > add[b].value || (row[a].value == add[b].value && row[a].seed < add[b].seed)));
            merged[i] = from_row ? row[a++] : add[b++];
        }
        memcpy(row, merged, keep * sizeof *row);
    }
    st->n += n;
    st->n_top = keep;
}

// ---- failure-mode grouping: table size, probe start and the host fold of a batch's entries ---------------------------------------
extern "C" uint64_t madsim_k_group_slots(uint64_t count) {
    uint64_t slots = MADSIM_K_GROUP_MIN_SLOTS;
    while (slots < 2 * count) slots <<= 1;
    return slots;
}

extern "C" uint64_t madsim_k_group_slot(uint64_t key, uint32_t verdict, uint64_t slots) { return madsim_k::group_slot(key, verdict, slots); }

// Which signature sits at which index of the caller's list: only WRITTEN signatures are remembered, so the memory is bounded by `cap`.
// Batches are folded in seed order and a batch's entries by first_seed: once the list is full, every signature not in it first appears
// behind all the written ones, so "append while there is room, else count as ungrouped" yields exactly the `cap` groups of smallest
// first_seed, each with the count of the whole prefix.
namespace {
struct GroupSig {
    uint64_t key; uint32_t verdict;
    bool operator==(const GroupSig& o) const { return key == o.key && verdict == o.verdict; }
};
struct GroupSigHash { size_t operator()(const GroupSig& s) const { return (size_t)madsim_k::group_slot(s.key, s.verdict, 0); } };   // (slots = 0: no mask)
struct GroupState { std::unordered_map<GroupSig, uint64_t, GroupSigHash> at; std::vector<madsim_group_t> sorted; };
}  // namespace

extern "C" void* madsim_k_group_state_new(void) { return new GroupState; }
extern "C" void madsim_k_group_state_free(void* state) { delete static_cast<GroupState*>(state); }

extern "C" void madsim_k_fold_groups(madsim_groups_t* grp, void* state, const madsim_group_t* batch_entries, uint64_t n, uint64_t seed0_of_batch) {
    GroupState& S = *static_cast<GroupState*>(state);
    S.sorted.assign(batch_entries, batch_entries + n);
    // (A list campaign passes the batch's FIRST LISTED seed: its entries' seeds ascend with their position in the batch, and none is
    // below the first, so the differences order the entries exactly as their positions would.)
    std::sort(S.sorted.begin(), S.sorted.end(), [seed0_of_batch](const madsim_group_t& a, const madsim_group_t& b) {
        return a.first_seed - seed0_of_batch < b.first_seed - seed0_of_batch;      // the index in the batch: unique per group
    });
    for (const madsim_group_t& e : S.sorted) {
        const GroupSig sig{e.key, e.verdict};
        auto it = S.at.find(sig);
        if (it != S.at.end()) { grp->groups[it->second].count += e.count; grp->n_grouped += e.count; continue; }
        if (grp->n_groups < grp->cap) {
            S.at.emplace(sig, grp->n_groups);
            grp->groups[grp->n_groups++] = madsim_group_t{e.key, e.verdict, 0, e.count, e.first_seed};
            grp->n_grouped += e.count;
        } else grp->n_ungrouped += e.count;
    }
}

// ---- differential campaigns: the host fold of a batch's words --------------------------------------------------------------------
// w = a batch's MADSIM_K_DIFF_WORDS (sim_kernel.hip): {n_differ, n_incomparable, n_by_field[8], transitions[8][8]}.  The counts commute; the list
// is appended in batch order, which is seed order, and never beyond `cap`.
extern "C" uint64_t madsim_k_fold_diff(madsim_diff_t* diff, const unsigned long long* w, uint64_t count, const madsim_diff_record_t* batch_recs) {
    diff->n_differ += w[0];
    diff->n_incomparable += w[1];
    diff->n_compared += count - w[1];
    for (int k = 0; k < 8; k++) diff->n_by_field[k] += w[2 + k];
    for (int k = 0; k < 64; k++) (&diff->transitions[0][0])[k] += w[10 + k];
    const uint64_t take = std::min<uint64_t>(w[0], diff->cap - diff->n_listed);
    if (take && batch_recs) memcpy(diff->records + diff->n_listed, batch_recs, take * sizeof(madsim_diff_record_t));
    diff->n_listed += take;
    return take;
}

// ---- paired campaigns: the host fold of a batch's words ----------------------------------------------------------------------------
// w = a batch's MADSIM_K_PAIRED_WORDS over `count` seeds (sim_kernel.hip).  Batches are folded in seed order, but nothing here relies on it:
// the counts, minima, maxima and sums commute, and the extreme seeds are merged under the total order (magnitude descending, seed
// ascending) — a row of the batch holds min(top_k, the batch's n[j]) entries, in that order.
extern "C" void madsim_k_fold_paired(madsim_paired_t* pr, const unsigned long long* w, uint64_t count) {
    pr->n_paired += w[0];
    pr->n_incomparable += w[1];
    pr->n_unpaired += count - w[0] - w[1];
    const uint32_t* hist = reinterpret_cast<const uint32_t*>(w + MADSIM_K_PAIRED_HEAD_WORDS);
    const madsim_paired_extreme_t* top = reinterpret_cast<const madsim_paired_extreme_t*>(w + MADSIM_K_PAIRED_HEAD_WORDS + 8 * MADSIM_STAT_BUCKETS / 2);
    auto add128 = [](uint64_t& lo, uint64_t& hi, unsigned long long low_halves, unsigned long long high_halves) {
        const unsigned __int128 sum = ((unsigned __int128)hi << 64 | lo) + low_halves + ((unsigned __int128)high_halves << 32);
        lo = (uint64_t)sum; hi = (uint64_t)(sum >> 64);
    };
    for (uint32_t m = 0; m < MADSIM_STAT_METRICS; m++) {
        pr->n_equal[m] += w[0] - w[2 + 2 * m] - w[3 + 2 * m];
        add128(pr->sum_a_lo[m], pr->sum_a_hi[m], w[42 + m], w[46 + m]);
        add128(pr->sum_b_lo[m], pr->sum_b_hi[m], w[50 + m], w[54 + m]);
    }
    const uint64_t K = pr->top_k;
    for (uint32_t j = 0; j < 8; j++) {
        const uint64_t n = w[2 + j];
        if (!n) continue;
        madsim_metric_t& M = pr->delta[j];
        pr->n[j] += n;
        M.min = std::min<uint64_t>(M.min, ~w[10 + j]);
        M.max = std::max<uint64_t>(M.max, w[18 + j]);
        add128(M.sum_lo, M.sum_hi, w[26 + j], w[34 + j]);
        for (uint32_t b = 0; b < MADSIM_STAT_BUCKETS; b++) M.hist[b] += hist[j * MADSIM_STAT_BUCKETS + b];
        if (!K) continue;
        const bool up = (j & 1u) == MADSIM_PAIRED_UP;
        auto mag = [up](const madsim_paired_extreme_t& e) { return up ? e.b - e.a : e.a - e.b; };
        madsim_paired_extreme_t* row = pr->top + j * K;
        const madsim_paired_extreme_t* add = top + j * MADSIM_STAT_MAX_TOP;
        const uint64_t have = pr->n_top[j], got = std::min(K, n), keep = std::min(K, have + got);
        madsim_paired_extreme_t merged[MADSIM_STAT_MAX_TOP];
        for (uint64_t i = 0, a = 0, b = 0; i < keep; i++) {
            const bool from_row = b >= got || (a < have && (mag(row[a]) > mag(add[b]) || (mag(row[a]) == mag(add[b]) && row[a].seed < add[b].seed)));
            merged[i] = from_row ? row[a++] : add[b++];
        }
        memcpy(row, merged, keep * sizeof *row);
        pr->n_top[j] = keep;
    }
}

// ---- sweep campaigns: the host fold of a batch's words -----------------------------------------------------------------------------
// w = a batch's MADSIM_K_SWEEP_WORDS (sim_kernel.hip): {n_selected, n_incomparable, n_runner_by_variant[8], n_differ_from_first[8],
// n_by_mask[256]}.  The counts commute; the list is appended in batch order, which is seed order, and never beyond `cap`.
extern "C" uint64_t madsim_k_fold_sweep(madsim_sweep_t* sweep, const unsigned long long* w, uint64_t count, const madsim_sweep_record_t* batch_recs) {
    sweep->n_selected += w[0];
    sweep->n_incomparable += w[1];
    sweep->n_settled += count - w[1];
    for (int v = 0; v < 8; v++) { sweep->n_runner_by_variant[v] += w[2 + v]; sweep->n_differ_from_first[v] += w[10 + v]; }
    for (int k = 0; k < 256; k++) sweep->n_by_mask[k] += w[18 + k];
    const uint64_t take = std::min<uint64_t>(w[0], sweep->cap - sweep->n_listed);
    if (take && batch_recs) memcpy(sweep->records + sweep->n_listed, batch_recs, take * sizeof(madsim_sweep_record_t));
    sweep->n_listed += take;
    return take;
}

// ---- campaigns -------------------------------------------------------------------------------------------------------------
// One implementation for one context and for several (madsim_hip_run_campaign_multi): batch k of the range runs on context k % n,
// on that context's flight (k / n) % in_flight — the devices advance through the seed space TOGETHER, so with
// MADSIM_CAMPAIGN_STOP_AT_FAILURE the search ends within one round of batches of the first genuine failure (contiguous blocks per
// device — the rule of madsim_hip_run_batch_multi — would leave the devices that hold the smaller seeds running to their end).
// Reports are read in batch order, so `first_failing_seed` is the smallest failing seed of the prefix [seed0, seed0 + seeds_run)
// whatever the number of devices: the report of n contexts equals the report of one.  Builder::run's fan-out with an early exit
// (runtime/builder.rs:129-160: every thread's result is joined in seed order, the first failure is re-raised).
namespace {
// The queue-and-harvest loop every campaign form shares: batch k may be queued once batch k - n * F[k % n] (the previous user of its flight)
// has been harvested; batches are harvested in order.  Returns the number of batches launched; after an error (first_err, first_msg) every
// stream of the flights has been drained.
extern "C++" {                                                   // (a template, inside this file's extern "C" block)
template <class Queue, class Harvest>
uint64_t pump_batches(madsim_hip_ctx* const* ctxs, int n_ctx, uint64_t n_batches, const std::vector<uint32_t>& F, const bool& stop, int& first_err,
                      std::string& first_msg, Queue queue, Harvest harvest) {
    const uint64_t N = (uint64_t)n_ctx;
    auto note = [&](int e) { if (e && !first_err) { first_err = e; first_msg = g_err; } };
    uint64_t launched = 0, harvested = 0;
    while (harvested < launched || (launched < n_batches && !stop && !first_err)) {
        const bool room = launched < n_batches && launched < harvested + N * (uint64_t)F[launched % N];
        if (room && !stop && !first_err) { note(queue(launched)); launched++; continue; }
        note(harvest(harvested)); harvested++;                  // the oldest batch in flight: its stream takes the next launch
    }
    if (first_err) {                                             // (as in run_pipelined: a stale `done` must not let a kernel outlive the call)
        for (int g = 0; g < n_ctx; g++) {
            if (ctxs[g]->bind()) continue;
            for (uint32_t i = 0; i < F[g]; i++) (void)hipStreamSynchronize(ctxs[g]->flights[i].stream);
        }
    }
    return launched;
}

// The flights of a campaign call.  F[g]: how many context g keeps in flight — the caller's number, else what the workload's occupancy
// rewards (`occupancy(context)`), no more than the context has batches.  setup() makes them ready: what every flight has
// (ensure_flights), what the campaign's form adds (`ensure_form(flight)`) and, for a list campaign, the list buffers.
struct CampaignFlights {
    madsim_hip_ctx* const* ctxs; uint64_t N; std::vector<uint32_t> F;
    CampaignFlights(madsim_hip_ctx* const* c, int n) : ctxs(c), N((uint64_t)n), F(n) {}
    madsim_hip_ctx::Flight& of(uint64_t k) const { const uint64_t g = k % N; return ctxs[g]->flights[(k / N) % F[g]]; }
    template <class Occupancy, class EnsureForm>
    int setup(uint64_t n_batches, uint64_t batch, uint64_t width, uint32_t in_flight, bool list, Occupancy occupancy, EnsureForm ensure_form) {
        for (uint64_t g = 0; g < N; g++) {
            madsim_hip_ctx* c = ctxs[g];
            int rc;
            if ((rc = c->bind())) return rc;
            const uint64_t mine = (n_batches + N - 1 - g) / N;      // batches g, g + n, g + 2n, ...
            uint32_t f = in_flight ? in_flight : occupancy(c);
            if ((uint64_t)f > mine) f = (uint32_t)mine;
            F[g] = f;
            if (f && (rc = c->ensure_flights(f, batch, false))) return rc;
            for (uint32_t i = 0; i < f; i++) {
                madsim_hip_ctx::Flight& fl = c->flights[i];
                if ((rc = ensure_form(fl))) return rc;
                if (list && (rc = fl.list.ensure(width, fl.stream))) return rc;
            }
        }
        return 0;
    }
};
}  // extern "C++"

// What every campaign form checks of its range first (batch 0 = the default).
int check_campaign_range(uint64_t& batch, uint32_t in_flight, bool list, uint64_t seed0, uint64_t total) {
    if (batch == 0) batch = 65536;
    if (in_flight > (uint32_t)madsim_hip_ctx::CAMPAIGN_MAX) return fail(MADSIM_E_ARG, "at most 8 batches in flight per context");
    if (!list && seed0 + total < seed0) return fail(MADSIM_E_ARG, "seed0 + total wraps");
    return 0;
}

// A list campaign's batch: its slice list[lo .. lo + n) into the flight, ahead of the launch that reads it (the flight's previous batch
// has been harvested: both buffers are free).
int queue_list_slice(madsim_hip_ctx::Flight& f, const uint64_t* list, uint64_t lo, uint64_t n) {
    memcpy(f.list.h, list + lo, n * sizeof(uint64_t));
    HIP_TRY(hipMemcpyAsync(f.list.d, f.list.h, n * sizeof(uint64_t), hipMemcpyHostToDevice, f.stream));
    return 0;
}

// A harvested batch into its campaign report: a = summary6's six words over the batch's n results, ms = its simulation kernel's time.
void fold_summary(madsim_campaign_t* out, const unsigned long long* a, uint64_t n, double ms) {
    out->kernel_ms += ms;
    out->batches_run++; out->seeds_run += n;
    out->n_runner += a[5];
    out->n_failed += a[1] - a[5];
    out->total_steps += a[2]; out->total_clock_ns += a[3];
    if (a[4] < out->first_failing_seed) out->first_failing_seed = a[4];
}

// ---- resolving campaigns (MADSIM_CAMPAIGN_RESOLVE) ---------------------------------------------------------------------------------
// The rounds a call's flags ask for (0: the call does not resolve), and the one argument error they can hold — told, like the other
// argument errors, before any context is looked at.
uint32_t resolve_rounds(uint32_t flags) {
    if (!(flags & MADSIM_CAMPAIGN_RESOLVE)) return 0;
    const uint32_t r = (flags & MADSIM_CAMPAIGN_RESOLVE_ROUNDS_MASK) >> MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT;
    return r ? r : MADSIM_RESOLVE_DEFAULT_ROUNDS;
}
int check_resolve_flags(uint32_t flags) {
    if (resolve_rounds(flags) > MADSIM_RESOLVE_MAX_ROUNDS) return fail(MADSIM_E_ARG, "MADSIM_CAMPAIGN_RESOLVE: at most MADSIM_RESOLVE_MAX_ROUNDS (8) rounds");
    return 0;
}

// A campaign call's resolve account: zeroed in every context of the call when it starts, stored in every one when it ends (errors included).
struct ResolveAccount {
    madsim_hip_ctx* const* ctxs; int n_ctx; madsim_resolve_t a{};
    ResolveAccount(madsim_hip_ctx* const* c, int n, uint32_t rounds) : ctxs(c), n_ctx(n) { a.rounds = rounds; store(); }
    ~ResolveAccount() { a.n_unresolved = a.n_first_pass - a.n_resolved; store(); }
    void store() { for (int g = 0; g < n_ctx; g++) ctxs[g]->resolved = a; }
};

// The rounds of one harvested batch, all on the flight's own stream (its scratch is keyed by the stream, and the other flights keep running):
// d_res[0 .. n) are the results of seeds seed_lo .. — or, in a list campaign, of d_list[0 .. n), the flight's slice of the list — under `lim`.  Round r compacts the seeds whose result is re-runnable under G^(r-1)(lim)
// (madsim_k_launch_resolve_list), reads the one count word, and — unless it is 0 — runs them in one launch under G^r(lim) and writes their
// new results where the old ones were (madsim_k_launch_resolve_scatter).  Every round grows everything (grow(.., true, true)): what a seed
// ends with does not depend on its batch.  On return the stream holds nothing unfinished but the last scatter; *ran = a round ran, so the
// caller's report is stale.
int resolve_results(madsim_hip_ctx* c, madsim_hip_ctx::Flight& f, const madsim_workload_t* w, const madsim_config_t* cfg, const madsim_limits_t* lim,
                    madsim_result_t* d_res, uint64_t seed_lo, const uint64_t* d_list, uint64_t n, uint32_t rounds, madsim_resolve_t& acct, double* rerun_ms,
                    bool* ran) {
    madsim_limits_t L{};
    if (lim) L = *lim;
    int e;
    madsim_hip_ctx::Flight::Resolve& rr = f.resolve;
    if ((e = rr.ensure(std::max<size_t>(n, f.d_out.cap), f.stream))) return e;      // the flight's batch size: one allocation per campaign
    uint32_t* const d_total = rr.cnt + MADSIM_K_RESOLVE_WAVES;
    bool timed = false;                                          // an event pair recorded and not yet read
    auto take_ms = [&]() -> int {
        if (!timed) return 0;
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, rr.r0, rr.r1));
        *rerun_ms += t; timed = false;
        return 0;
    };
    for (uint32_t r = 1; r <= rounds; r++) {
        const uint32_t steps_maxed = (L.max_steps ? L.max_steps : (1u << 24)) >= step_ceiling(L) ? 1u : 0u;
        if (d_list ? madsim_k_launch_resolve_list_list(d_res, n, d_list, steps_maxed, rr.cnt, d_total, rr.seeds, rr.idx, f.stream)
                   : madsim_k_launch_resolve_list(d_res, n, seed_lo, steps_maxed, rr.cnt, d_total, rr.seeds, rr.idx, f.stream))
            return fail(MADSIM_E_ARG, "madsim_k_launch_resolve_list refused the batch's size");
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(rr.h_cnt, d_total, sizeof(uint32_t), hipMemcpyDeviceToHost, f.stream));
        HIP_TRY(hipStreamSynchronize(f.stream));
        if ((e = take_ms())) return e;
        const uint64_t m = *rr.h_cnt;
        if (m == 0) break;
        if (m > n || m > rr.rerun.cap) return fail(MADSIM_E_HIP, "resolve: a batch lists more re-runnable seeds than it holds");
        if (r == 1) { acct.n_first_pass += m; acct.batches_resolved++; }
        acct.n_by_round[r - 1] += m;
        grow(L, w, true, true);
        HIP_TRY(hipEventRecord(rr.r0, f.stream));
        if ((e = c->launch(w, cfg, 0, m, rr.seeds, &L, rr.rerun, f.stream))) return e;
        HIP_TRY(hipEventRecord(rr.r1, f.stream));
        timed = true;
        if (madsim_k_launch_resolve_scatter(d_res, rr.rerun, rr.idx, m, f.stream))
            return fail(MADSIM_E_ARG, "madsim_k_launch_resolve_scatter refused the list's size");
        HIP_TRY(hipGetLastError());
        *ran = true;
    }
    if (timed) { HIP_TRY(hipStreamSynchronize(f.stream)); if ((e = take_ms())) return e; }      // (the last of the rounds ran: no list pair behind it)
    return 0;
}

int run_campaign_impl(madsim_hip_ctx* const* ctxs, int n_ctx, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total,
                      uint64_t batch, uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim, madsim_campaign_t* out,
                      madsim_collect_t* col = nullptr, madsim_stats_t* st = nullptr, madsim_groups_t* grp = nullptr, const uint64_t* list = nullptr) {
    // `list` (the list campaigns): position i of list[0 .. total) takes the role of seed0 + i, and seed0 is 0.  The loop, the flights, the fold
    // and the stop rules are the range form's; a flight also carries the batch's slice of the list, copied in ahead of its simulation launch.
    auto t0 = std::chrono::steady_clock::now();
    memset(out, 0, sizeof *out);
    out->first_failing_seed = UINT64_MAX;
    const uint32_t R = resolve_rounds(flags);                   // 0: runner verdicts are counted apart, as ever
    ResolveAccount account(ctxs, n_ctx, R);
    madsim_resolve_t& acct = account.a;
    if (st) {
        st->n = st->n_top = 0;
        memset(st->metric, 0, sizeof st->metric);
        for (madsim_metric_t& m : st->metric) m.min = UINT64_MAX;
    }
    if (col) { col->n_listed = 0; memset(col->n_by_verdict, 0, sizeof col->n_by_verdict); }
    else flags &= ~(MADSIM_CAMPAIGN_LIST_RUNNER | MADSIM_CAMPAIGN_STOP_AT_CAP);      // (flags of the collecting form only)
    if (grp) grp->n_groups = grp->n_grouped = grp->n_ungrouped = 0;
    else flags &= ~MADSIM_CAMPAIGN_STOP_AT_GROUPS;                                   // (a flag of the grouping form only)
    struct GroupStateOwner { void* p; ~GroupStateOwner() { if (p) madsim_k_group_state_free(p); } } gstate{grp ? madsim_k_group_state_new() : nullptr};
    std::vector<madsim_group_t> gbatch;                          // a batch's entries, as the device left them
    int rc = madsim_geo::validate(w, cfg, &g_err);
    if (rc) return rc;
    if ((rc = check_campaign_range(batch, in_flight, list != nullptr, seed0, total))) return rc;
    if (total == 0) return 0;
    const uint64_t width = std::min(batch, total);              // seeds in the largest batch
    if (st && width >= 0xffffffffull) return fail(MADSIM_E_ARG, "a statistics campaign's batch holds fewer than 2^32 - 1 seeds");
    if (R && width >= (1ull << 30)) return fail(MADSIM_E_ARG, "a resolving campaign's batch holds fewer than 2^30 seeds");
    const uint64_t n_batches = (total + batch - 1) / batch, N = (uint64_t)n_ctx;
    const uint64_t rec_batch = col ? std::min(col->cap, width) : 0;      // records a flight holds: no batch lists more
    // a grouping campaign's report: the sixteen words, the statistics words when asked for, then the grouping words; its table is sized to the batch
    const size_t goff = 16 + (st ? MADSIM_K_STATS_WORDS : 0);
    const uint64_t gslots = grp ? madsim_k_group_slots(width) : 0;
    uint64_t listed_seen = 0;                                   // listed seeds of the batches folded so far (not cut at cap)
    CampaignFlights flights(ctxs, n_ctx);
    if ((rc = flights.setup(n_batches, batch, width, in_flight, list != nullptr,
                            [&](madsim_hip_ctx* c) { return c->flights_for(w, cfg, lim, batch); },
                            [&](madsim_hip_ctx::Flight& f) -> int {
                                int e = 0;
                                if (col) e = f.collect.ensure(rec_batch, f.stream);
                                if (!e && st) e = f.stats.ensure();
                                if (!e && grp) e = f.groups.ensure(width, f.stream);
                                return e;
                            })))
        return rc;
    int first_err = 0;
    std::string first_msg;
    // A batch's report chain, in two parts that `queue` puts around the simulation launch and a resolving `harvest` queues again back to
    // back: the report words made ready, then the report kernels over f.d_out, the copy of the words and the `done` event.
    const size_t n_words = grp ? goff + MADSIM_K_GROUP_WORDS
                               : st ? madsim_hip_ctx::STATS_REP_WORDS - (st->top_k ? 0 : 2 * MADSIM_STAT_METRICS * MADSIM_STAT_MAX_TOP)
                               : col ? MADSIM_K_COLLECT_WORDS : 6;
    auto prepare_report = [&](madsim_hip_ctx::Flight& f) -> int {
        // the same four memsets, the last one longer when collecting, and longer still with statistics (whose words all start as zero)
        unsigned long long* const d_words = f.d_rep;
        HIP_TRY(hipMemsetAsync(d_words, 0xff, 8, f.stream));
        HIP_TRY(hipMemsetAsync((char*)d_words + 8, 0, 24, f.stream));
        HIP_TRY(hipMemsetAsync((char*)d_words + 32, 0xff, 8, f.stream));
        HIP_TRY(hipMemsetAsync((char*)d_words + 40, 0, (n_words - 5) * 8, f.stream));
        return 0;
    };
    auto queue_report = [&](madsim_hip_ctx::Flight& f, uint64_t lo, uint64_t n) -> int {
        unsigned long long* const d_words = f.d_rep;
        const uint32_t list_runner = (flags & MADSIM_CAMPAIGN_LIST_RUNNER) ? 1u : 0u;
        if (col && list) madsim_k_launch_collect_list(f.d_out, n, f.list.d, list_runner, d_words, f.collect.wcnt, f.collect.rec, std::min(rec_batch, n), f.stream);
        else if (col) madsim_k_launch_collect(f.d_out, n, seed0 + lo, list_runner, d_words, f.collect.wcnt, f.collect.rec, std::min(rec_batch, n), f.stream);
        else if (list) madsim_k_launch_summary6_list(f.d_out, n, f.list.d, d_words, f.stream);
        else madsim_k_launch_summary6(f.d_out, n, seed0 + lo, d_words, f.stream);
        HIP_TRY(hipGetLastError());
        if (st) {                                                // behind the report kernel, into the words after its sixteen
            if (list) madsim_k_launch_stats_list(f.d_out, n, f.list.d, st->include, st->top_k, d_words + 16, f.stats.cand, f.stream);
            else madsim_k_launch_stats(f.d_out, n, seed0 + lo, st->include, st->top_k, d_words + 16, f.stats.cand, f.stream);
            HIP_TRY(hipGetLastError());
        }
        if (grp) {                                               // behind them: the batch's groups; their number rides with the report words
            f.groups.dirty = true;                               // (until the batch is harvested: its extraction pass has then left the table zero)
            if (list ? madsim_k_launch_groups_list(f.d_out, n, f.list.d, grp->include, grp->key_field, f.groups.tab, gslots, f.groups.list, d_words + goff, f.groups.ent, f.stream)
                     : madsim_k_launch_groups(f.d_out, n, seed0 + lo, grp->include, grp->key_field, f.groups.tab, gslots, f.groups.list, d_words + goff, f.groups.ent, f.stream))
                return fail(MADSIM_E_ARG, "madsim_k_launch_groups refused the batch's sizes");
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(f.h_rep, d_words, n_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, f.stream));
        HIP_TRY(hipEventRecord(f.done, f.stream));
        return 0;
    };
    auto queue = [&](uint64_t k) -> int {
        madsim_hip_ctx* c = ctxs[k % N];
        madsim_hip_ctx::Flight& f = flights.of(k);
        const uint64_t lo = k * batch, n = std::min(batch, total - lo);
        int e;
        if ((e = c->bind())) return e;
        if ((e = prepare_report(f))) return e;
        if (list && (e = queue_list_slice(f, list, lo, n))) return e;
        HIP_TRY(hipEventRecord(f.e0, f.stream));
        if ((e = c->launch(w, cfg, seed0 + lo, n, list ? f.list.d : nullptr, lim, f.d_out, f.stream))) return e;
        HIP_TRY(hipEventRecord(f.e1, f.stream));
        return queue_report(f, lo, n);
    };
    bool stop = false;
    auto harvest = [&](uint64_t k) -> int {                     // wait for batch k, fold its report (batches are read in order)
        madsim_hip_ctx* c = ctxs[k % N];
        madsim_hip_ctx::Flight& f = flights.of(k);
        int e;
        if ((e = c->bind())) return e;
        HIP_TRY(hipEventSynchronize(f.done));
        f.groups.dirty = false;                                 // (both grouping passes of the batch, if any, have run)
        if (first_err) return 0;                                // (draining after an error: nothing is folded any more)
        const uint64_t lo = k * batch, n = std::min(batch, total - lo);
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, f.e0, f.e1));
        if (!stop) {                                            // batches launched beyond the failing one are not part of the answer
            const unsigned long long* a = f.h_rep;
            if (R && a[5] > 0) {                                // runner verdicts in a batch that is part of the answer: settle them, report again
                const unsigned long long runner_before = a[5];
                double rerun_ms = 0.0;
                bool ran = false;
                if ((e = resolve_results(c, f, w, cfg, lim, f.d_out, seed0 + lo, list ? f.list.d : nullptr, n, R, acct, &rerun_ms, &ran))) return e;
                acct.rerun_kernel_ms += rerun_ms; out->kernel_ms += rerun_ms;
                if (ran) {                                      // (the grouping table is clean: the first chain's extraction pass left it so)
                    if ((e = prepare_report(f)) || (e = queue_report(f, lo, n))) return e;
                    HIP_TRY(hipEventSynchronize(f.done));
                    f.groups.dirty = false;
                    acct.n_resolved += runner_before - a[5];
                }
            }
            fold_summary(out, a, n, ms);
            if ((flags & MADSIM_CAMPAIGN_STOP_AT_FAILURE) && a[4] != UINT64_MAX) stop = true;
            if (col) {
                for (int v = 0; v < 8; v++) col->n_by_verdict[v] += a[6 + v];
                // the batch's records, as many as the list still takes: batches are read in seed order, so appending keeps the order.
                // The stream is idle (its `done` has passed) and takes no launch before this returns.
                const uint64_t take = std::min<uint64_t>(std::min<uint64_t>(a[14], std::min(rec_batch, n)), col->cap - col->n_listed);
                if (take) {
                    HIP_TRY(hipMemcpyAsync(col->failures + col->n_listed, f.collect.rec, take * sizeof(madsim_failure_t), hipMemcpyDeviceToHost, f.stream));
                    HIP_TRY(hipStreamSynchronize(f.stream));
                    col->n_listed += take;
                }
                listed_seen += a[14];
                if ((flags & MADSIM_CAMPAIGN_STOP_AT_CAP) && listed_seen >= col->cap) stop = true;
            }
            if (st) madsim_k_fold_stats(st, a + 16);
            if (grp) {
                const uint64_t ng = a[goff];
                if (a[goff + 1] || ng > n)
                    return fail(MADSIM_E_HIP, "grouping: a probe of the batch's group table ran out, or the table was not clean (error word " +
                                                  std::to_string(a[goff + 1]) + ", " + std::to_string(ng) + " groups)");
                if (ng) {                                       // the batch's entries, only when there are some and only that many (the stream is idle)
                    gbatch.resize(ng);
                    HIP_TRY(hipMemcpyAsync(gbatch.data(), f.groups.ent, ng * sizeof(madsim_group_t), hipMemcpyDeviceToHost, f.stream));
                    HIP_TRY(hipStreamSynchronize(f.stream));
                    madsim_k_fold_groups(grp, gstate.p, gbatch.data(), ng, list ? list[lo] : seed0 + lo);
                }
                if ((flags & MADSIM_CAMPAIGN_STOP_AT_GROUPS) && grp->n_groups >= grp->cap) stop = true;
            }
        }
        return 0;
    };
    out->batches_launched = pump_batches(ctxs, n_ctx, n_batches, flights.F, stop, first_err, first_msg, queue, harvest);
    out->wall_s = since(t0);
    return first_err ? fail(first_err, first_msg) : 0;
}

// ---- the multi-variant forms: differential, paired, sweep ---------------------------------------------------------------------------
// The same flights, the same loop; per batch every variant's simulation and summary6 launches, then the form's report kernels, all on the
// flight's one stream, and one copy of the words.  Every variant of batch k runs on context k % n.  A form says what is its own: how an error
// names variant v (who), the stop flag it honours, how wide a batch it takes, how many of the words a batch uses (n_copied: both copies stop
// there), what it keeps on a flight (ensure), its report kernels over the variants' results (queue: `words` are the form's, all zero), and
// its host fold with the records the list still takes and its stop rule (fold: the stream is idle — its `done` has passed — and takes no
// launch before fold returns).
extern "C++" {
template <class Rec>
int copy_records(Rec* to, const Rec* d_from, uint64_t take, hipStream_t s) {
    if (!take) return 0;
    HIP_TRY(hipMemcpyAsync(to, d_from, take * sizeof(Rec), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// Differential and paired campaigns: the diff kernels when a diff report is asked for, the paired kernels behind them when a paired one is;
// the diff words first, then the paired words, whose copies end before the top records when there are none.
struct PairForm {
    madsim_diff_t* d; madsim_paired_t* pr;
    static constexpr uint64_t max_width = 1ull << 32;
    static constexpr const char* too_wide = "a differential campaign's batch holds fewer than 2^32 seeds";
    static std::string who(uint32_t v) { return v ? "side B: " : "side A: "; }
    uint32_t stop_flag() const { return d ? MADSIM_CAMPAIGN_STOP_AT_DIFFS : 0u; }
    size_t n_copied() const {
        return !pr ? madsim_hip_ctx::DIFF_REP_WORDS : madsim_hip_ctx::PAIRED_REP_WORDS - (pr->top_k ? 0 : 8 * MADSIM_STAT_MAX_TOP * 3);
    }
    void reset() const {
        if (d) {
            d->n_listed = d->n_compared = d->n_incomparable = d->n_differ = 0;
            memset(d->n_by_field, 0, sizeof d->n_by_field);
            memset(d->transitions, 0, sizeof d->transitions);
        }
        if (pr) {                                                // (everything behind the caller's inputs)
            memset(&pr->n_paired, 0, sizeof *pr - offsetof(madsim_paired_t, n_paired));
            for (madsim_metric_t& M : pr->delta) M.min = UINT64_MAX;
        }
    }
    int ensure(madsim_hip_ctx::Flight& f, uint64_t width) const {
        if (d) if (int e = f.diff.ensure(std::min(d->cap, width), f.stream)) return e;      // (records a flight holds: no batch lists more)
        return pr ? f.paired.ensure() : 0;
    }
    int queue(madsim_hip_ctx::Flight& f, const madsim_result_t* const* res, uint64_t seed_lo, const uint64_t* d_list, uint64_t n, report_word_t* words) const {
        if (d && (d_list ? madsim_k_launch_diff_list(res[0], res[1], n, d_list, d->fields, words, f.diff.wcnt, f.diff.rec, std::min(d->cap, n), f.stream)
                         : madsim_k_launch_diff(res[0], res[1], n, seed_lo, d->fields, words, f.diff.wcnt, f.diff.rec, std::min(d->cap, n), f.stream)))
            return fail(MADSIM_E_ARG, "madsim_k_launch_diff refused the batch's arguments");
        report_word_t* const pw = words + MADSIM_K_DIFF_WORDS;
        if (pr && (d_list ? madsim_k_launch_paired_list(res[0], res[1], n, d_list, pr->include_a, pr->include_b, pr->top_k, pw, f.paired.cand, f.stream)
                          : madsim_k_launch_paired(res[0], res[1], n, seed_lo, pr->include_a, pr->include_b, pr->top_k, pw, f.paired.cand, f.stream)))
            return fail(MADSIM_E_ARG, "madsim_k_launch_paired refused the batch's arguments");
        return 0;
    }
    int fold(madsim_hip_ctx::Flight& f, const report_word_t* words, uint64_t n, uint32_t flags, bool& stop) const {
        if (pr) {
            const report_word_t* const pw = words + MADSIM_K_DIFF_WORDS;
            if (pw[0] + pw[1] > n) return fail(MADSIM_E_HIP, "paired campaign: a batch reports more paired and incomparable seeds than it holds");
            madsim_k_fold_paired(pr, pw, n);
        }
        if (!d) return 0;
        if (words[0] > n) return fail(MADSIM_E_HIP, "differential campaign: a batch reports more differing seeds than it holds");
        const uint64_t at = d->n_listed, take = madsim_k_fold_diff(d, words, n, nullptr);
        if (int e = copy_records(d->records + at, f.diff.rec.p, take, f.stream)) return e;
        if ((flags & MADSIM_CAMPAIGN_STOP_AT_DIFFS) && d->n_differ >= d->cap) stop = true;
        return 0;
    }
};

// Sweep campaigns: the two sweep kernels over all V results.
struct SweepForm {
    madsim_sweep_t* sw; uint32_t V;
    static constexpr uint64_t max_width = 1ull << 32;
    static constexpr const char* too_wide = "a sweep campaign's batch holds fewer than 2^32 seeds";
    static std::string who(uint32_t v) { return "variant " + std::to_string(v) + ": "; }
    static uint32_t stop_flag() { return MADSIM_CAMPAIGN_STOP_AT_SWEEP; }
    static size_t n_copied() { return madsim_hip_ctx::SWEEP_REP_WORDS; }
    void reset() const {
        sw->n_listed = sw->n_selected = sw->n_settled = sw->n_incomparable = 0;
        memset(sw->n_runner_by_variant, 0, sizeof sw->n_runner_by_variant);
        memset(sw->n_differ_from_first, 0, sizeof sw->n_differ_from_first);
        memset(sw->n_by_mask, 0, sizeof sw->n_by_mask);
    }
    int ensure(madsim_hip_ctx::Flight& f, uint64_t width) const { return f.sweep.ensure(std::min(sw->cap, width), f.stream); }      // (no batch lists more)
    int queue(madsim_hip_ctx::Flight& f, const madsim_result_t* const* res, uint64_t seed_lo, const uint64_t* d_list, uint64_t n, report_word_t* words) const {
        if (d_list ? madsim_k_launch_sweep_list(res, V, n, d_list, sw->fields, sw->list_rule, words, f.sweep.wcnt, f.sweep.rec, std::min(sw->cap, n), f.stream)
                   : madsim_k_launch_sweep(res, V, n, seed_lo, sw->fields, sw->list_rule, words, f.sweep.wcnt, f.sweep.rec, std::min(sw->cap, n), f.stream))
            return fail(MADSIM_E_ARG, "madsim_k_launch_sweep refused the batch's arguments");
        return 0;
    }
    int fold(madsim_hip_ctx::Flight& f, const report_word_t* words, uint64_t n, uint32_t flags, bool& stop) const {
        if (words[0] > n) return fail(MADSIM_E_HIP, "sweep campaign: a batch reports more selected seeds than it holds");
        const uint64_t at = sw->n_listed, take = madsim_k_fold_sweep(sw, words, n, nullptr);
        if (int e = copy_records(sw->records + at, f.sweep.rec.p, take, f.stream)) return e;
        if ((flags & MADSIM_CAMPAIGN_STOP_AT_SWEEP) && sw->n_selected >= sw->cap) stop = true;
        return 0;
    }
};

// `var`: the V variants (a differential call's two sides; a sweep's, with a NULL config replaced by the default one).  `list`: as in
// run_campaign_impl — position i of list[0 .. total) for seed0 + i, seed0 = 0; every variant of a batch reads the same slice.
template <class Form>
int run_variants_impl(madsim_hip_ctx* const* ctxs, int n_ctx, const madsim_sweep_variant_t* var, uint32_t V, uint64_t seed0, uint64_t total, uint64_t batch,
                      uint32_t in_flight, uint32_t flags, const uint64_t* list, const Form& form) {
    auto t0 = std::chrono::steady_clock::now();
    for (uint32_t v = 0; v < V; v++) { memset(var[v].out, 0, sizeof *var[v].out); var[v].out->first_failing_seed = UINT64_MAX; }
    form.reset();
    flags &= form.stop_flag() | MADSIM_CAMPAIGN_RESOLVE | MADSIM_CAMPAIGN_RESOLVE_ROUNDS_MASK;      // (the other stop flags belong to the other forms)
    const uint32_t R = resolve_rounds(flags);
    ResolveAccount account(ctxs, n_ctx, R);
    madsim_resolve_t& acct = account.a;
    for (uint32_t v = 0; v < V; v++)                             // (a sweep's variants have passed this before: check_sweep_args)
        if (int rc = madsim_geo::validate(var[v].w, var[v].cfg, &g_err)) return fail(rc, form.who(v) + g_err);
    int rc;
    if ((rc = check_campaign_range(batch, in_flight, list != nullptr, seed0, total))) return rc;
    if (total == 0) return 0;
    const uint64_t width = std::min(batch, total);
    if (width >= form.max_width) return fail(MADSIM_E_ARG, form.too_wide);
    if (R && width >= (1ull << 30)) return fail(MADSIM_E_ARG, "a resolving campaign's batch holds fewer than 2^30 seeds");
    const uint64_t n_batches = (total + batch - 1) / batch, N = (uint64_t)n_ctx;
    CampaignFlights flights(ctxs, n_ctx);
    if ((rc = flights.setup(n_batches, batch, width, in_flight, list != nullptr,
                            [&](madsim_hip_ctx* c) {
                                uint32_t f = c->flights_for(var[0].w, var[0].cfg, var[0].lim, batch);
                                for (uint32_t v = 1; v < V; v++) f = std::min(f, c->flights_for(var[v].w, var[v].cfg, var[v].lim, batch));
                                return f;
                            },
                            [&](madsim_hip_ctx::Flight& f) {
                                if (int e = f.variants.ensure(V, batch, f.stream)) return e;
                                return form.ensure(f, width);
                            })))
        return rc;
    constexpr size_t at_init = madsim_hip_ctx::VARIANT_REP_WORDS, at_form = madsim_hip_ctx::VARIANT_FORM_AT;
    const size_t n_copied = form.n_copied();
    int first_err = 0;
    std::string first_msg;
    bool stop = false;
    auto results_of = [](madsim_hip_ctx::Flight& f, uint32_t v) -> madsim_result_t* { return v ? f.variants.out[v - 1] : f.d_out; };
    // A batch's report chain in the parts that `queue` puts around the simulation launches and a resolving `harvest` queues again back to
    // back: the words reset by one device copy, a variant's summary6 over its results, then the form's kernels, the copy and the `done` event.
    auto prepare_report = [&](madsim_hip_ctx::Flight& f) -> int {
        report_word_t* const d_rep = f.variants.d_rep;
        HIP_TRY(hipMemcpyAsync(d_rep, d_rep + at_init, n_copied * sizeof(report_word_t), hipMemcpyDeviceToDevice, f.stream));
        return 0;
    };
    auto queue_summary = [&](madsim_hip_ctx::Flight& f, uint32_t v, uint64_t lo, uint64_t n) -> int {
        if (list) madsim_k_launch_summary6_list(results_of(f, v), n, f.list.d, f.variants.d_rep + 8 * v, f.stream);
        else madsim_k_launch_summary6(results_of(f, v), n, seed0 + lo, f.variants.d_rep + 8 * v, f.stream);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    auto queue_form = [&](madsim_hip_ctx::Flight& f, uint64_t lo, uint64_t n) -> int {
        const madsim_result_t* res[MADSIM_SWEEP_MAX_VARIANTS] = {};
        for (uint32_t v = 0; v < V; v++) res[v] = results_of(f, v);
        if (int e = form.queue(f, res, seed0 + lo, list ? f.list.d : nullptr, n, f.variants.d_rep + at_form)) return e;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(f.variants.h_rep, f.variants.d_rep, n_copied * sizeof(report_word_t), hipMemcpyDeviceToHost, f.stream));
        HIP_TRY(hipEventRecord(f.done, f.stream));
        return 0;
    };
    auto queue = [&](uint64_t k) -> int {
        madsim_hip_ctx* c = ctxs[k % N];
        madsim_hip_ctx::Flight& f = flights.of(k);
        const uint64_t lo = k * batch, n = std::min(batch, total - lo);
        int e;
        if ((e = c->bind())) return e;
        if ((e = prepare_report(f))) return e;
        if (list && (e = queue_list_slice(f, list, lo, n))) return e;      // (one slice for every variant)
        const uint64_t* const d_list = list ? f.list.d : nullptr;
        for (uint32_t v = 0; v < V; v++) {
            HIP_TRY(hipEventRecord(f.variants.v0[v], f.stream));
            if ((e = c->launch(var[v].w, var[v].cfg, seed0 + lo, n, d_list, var[v].lim, results_of(f, v), f.stream))) return fail(e, form.who(v) + g_err);
            HIP_TRY(hipEventRecord(f.variants.v1[v], f.stream));
            if ((e = queue_summary(f, v, lo, n))) return e;
        }
        return queue_form(f, lo, n);
    };
    auto harvest = [&](uint64_t k) -> int {
        madsim_hip_ctx* c = ctxs[k % N];
        madsim_hip_ctx::Flight& f = flights.of(k);
        int e;
        if ((e = c->bind())) return e;
        HIP_TRY(hipEventSynchronize(f.done));
        if (first_err || stop) return 0;                        // (draining after an error, or a batch launched beyond the stopping one)
        const uint64_t lo = k * batch, n = std::min(batch, total - lo);
        const report_word_t* const h = f.variants.h_rep;
        float ms[MADSIM_SWEEP_MAX_VARIANTS] = {};
        for (uint32_t v = 0; v < V; v++) HIP_TRY(hipEventElapsedTime(&ms[v], f.variants.v0[v], f.variants.v1[v]));
        unsigned long long runner_before[MADSIM_SWEEP_MAX_VARIANTS] = {}, any_runner = 0;
        for (uint32_t v = 0; v < V; v++) any_runner += runner_before[v] = h[8 * v + 5];
        if (R && any_runner) {                                  // runner verdicts in a variant: settle them under that variant's own limits, report again
            bool ran = false;
            for (uint32_t v = 0; v < V; v++) {                  // (one after the other on the flight's stream: they share its re-run scratch)
                if (!runner_before[v]) continue;
                double rerun_ms = 0.0;
                if ((e = resolve_results(c, f, var[v].w, var[v].cfg, var[v].lim, results_of(f, v), seed0 + lo, list ? f.list.d : nullptr, n, R, acct, &rerun_ms,
                                         &ran)))
                    return fail(e, form.who(v) + g_err);
                acct.rerun_kernel_ms += rerun_ms; var[v].out->kernel_ms += rerun_ms;
            }
            if (ran) {
                if ((e = prepare_report(f))) return e;
                for (uint32_t v = 0; v < V; v++) if ((e = queue_summary(f, v, lo, n))) return e;
                if ((e = queue_form(f, lo, n))) return e;
                HIP_TRY(hipEventSynchronize(f.done));
                for (uint32_t v = 0; v < V; v++) acct.n_resolved += runner_before[v] - h[8 * v + 5];
            }
        }
        for (uint32_t v = 0; v < V; v++) fold_summary(var[v].out, h + 8 * v, n, ms[v]);
        return form.fold(f, h + at_form, n, flags, stop);
    };
    const uint64_t launched = pump_batches(ctxs, n_ctx, n_batches, flights.F, stop, first_err, first_msg, queue, harvest);
    for (uint32_t v = 0; v < V; v++) { var[v].out->batches_launched = launched; var[v].out->wall_s = since(t0); }
    return first_err ? fail(first_err, first_msg) : 0;
}
}  // extern "C++"
}  // namespace

// The collecting, statistics and grouping forms and the list campaigns: the argument errors that need no device are told first, so that a
// host without a GPU hears about them too.  `form` is the part the entry point cannot do without; the other parts are checked when given.
// The errors come in the order they always came in: the report, the form's own part, the first part given (grouping before statistics
// before collecting), the resolve flags, a grouping batch's size, the remaining parts, the batches in flight.  (FORM_PLAIN, the form with
// the report alone, hears about its batches in flight from the engine, behind the workload's own errors: where it always did.)
namespace {
enum CampaignForm { FORM_ANY, FORM_PLAIN, FORM_COLLECT, FORM_STATS, FORM_GROUPS };
int check_collect_part(const madsim_collect_t* col, uint32_t flags) {
    if (col->cap && !col->failures) return fail(MADSIM_E_ARG, "madsim_collect_t.cap > 0 without a failures array");
    if ((flags & MADSIM_CAMPAIGN_STOP_AT_CAP) && !col->cap) return fail(MADSIM_E_ARG, "MADSIM_CAMPAIGN_STOP_AT_CAP with cap == 0");
    return 0;
}
int check_stats_part(const madsim_stats_t* st) {
    if (st->include == 0 || (st->include & ~0xfu)) return fail(MADSIM_E_ARG, "madsim_stats_t.include: at least one of bits 0-3 (PASS, PANIC, DEADLOCK, TIME_LIMIT), no other");
    if (st->top_k > MADSIM_STAT_MAX_TOP) return fail(MADSIM_E_ARG, "madsim_stats_t.top_k > MADSIM_STAT_MAX_TOP");
    if (st->top_k && !st->top) return fail(MADSIM_E_ARG, "madsim_stats_t.top_k > 0 without a top array");
    return 0;
}
int check_groups_part(const madsim_groups_t* grp, uint32_t flags) {
    if (grp->include == 0 || (grp->include & ~0xfu)) return fail(MADSIM_E_ARG, "madsim_groups_t.include: at least one of bits 0-3 (PASS, PANIC, DEADLOCK, TIME_LIMIT), no other");
    if (grp->key_field >= MADSIM_GROUP_KEYS) return fail(MADSIM_E_ARG, "madsim_groups_t.key_field: one of MADSIM_GROUP_KEY_*");
    if (grp->cap && !grp->groups) return fail(MADSIM_E_ARG, "madsim_groups_t.cap > 0 without a groups array");
    if ((flags & MADSIM_CAMPAIGN_STOP_AT_GROUPS) && !grp->cap) return fail(MADSIM_E_ARG, "MADSIM_CAMPAIGN_STOP_AT_GROUPS with cap == 0");
    return 0;
}
int check_campaign_args(CampaignForm form, const madsim_campaign_t* out, const madsim_collect_t* col, const madsim_stats_t* st, const madsim_groups_t* grp,
                        uint64_t total, uint64_t batch, uint32_t in_flight, uint32_t flags) {
    if (!out) return fail(MADSIM_E_ARG, "null campaign report");
    if (form == FORM_COLLECT && !col) return fail(MADSIM_E_ARG, "null madsim_collect_t (madsim_hip_run_campaign is the form without a failure list)");
    if (form == FORM_STATS && !st) return fail(MADSIM_E_ARG, "null madsim_stats_t");
    if (form == FORM_GROUPS && !grp) return fail(MADSIM_E_ARG, "null madsim_groups_t");
    int rc = grp ? check_groups_part(grp, flags) : st ? check_stats_part(st) : col ? check_collect_part(col, flags) : 0;
    if (rc || (rc = check_resolve_flags(flags))) return rc;
    if (grp && std::min(batch ? batch : 65536, total) > MADSIM_GROUP_MAX_BATCH)
        return fail(MADSIM_E_ARG, "a grouping campaign's batch holds at most MADSIM_GROUP_MAX_BATCH (2^20) seeds: the device table is sized to the batch");
    if (grp && st && (rc = check_stats_part(st))) return rc;
    if ((grp || st) && col && (rc = check_collect_part(col, flags))) return rc;
    if (form != FORM_PLAIN && in_flight > (uint32_t)madsim_hip_ctx::CAMPAIGN_MAX) return fail(MADSIM_E_ARG, "at most 8 batches in flight per context");
    return 0;
}
}  // namespace

// The differential forms: argument errors first, as the other forms.
namespace {
int check_diff_args(const madsim_campaign_t* outA, const madsim_campaign_t* outB, const madsim_diff_t* d, uint32_t in_flight, uint32_t flags) {
    if (!outA || !outB) return fail(MADSIM_E_ARG, "null campaign report (a differential campaign fills one per side)");
    if (!d) return fail(MADSIM_E_ARG, "null madsim_diff_t");
    if (d->fields == 0 || (d->fields & ~MADSIM_DIFF_ALL)) return fail(MADSIM_E_ARG, "madsim_diff_t.fields: at least one MADSIM_DIFF_* bit, none above MADSIM_DIFF_ALL");
    if (d->reserved) return fail(MADSIM_E_ARG, "madsim_diff_t.reserved must be 0");
    if (d->cap && !d->records) return fail(MADSIM_E_ARG, "madsim_diff_t.cap > 0 without a records array");
    if ((flags & MADSIM_CAMPAIGN_STOP_AT_DIFFS) && !d->cap) return fail(MADSIM_E_ARG, "MADSIM_CAMPAIGN_STOP_AT_DIFFS with cap == 0");
    if (int rc = check_resolve_flags(flags)) return rc;
    if (in_flight > (uint32_t)madsim_hip_ctx::CAMPAIGN_MAX) return fail(MADSIM_E_ARG, "at most 8 batches in flight per context");
    return 0;
}
}  // namespace

// ---- list campaigns: every campaign form over an explicit seed list ----------------------------------------------------------------
// Argument errors first, as the other forms: the list itself (NULL with n > 0; a pair that does not ascend strictly, named by the position
// of its first seed), then each present part's own checks.  All told before any context is looked at.
namespace {
int check_seed_list(const uint64_t* seeds, uint64_t n) {
    if (!seeds && n) return fail(MADSIM_E_ARG, "null seed list with n > 0");
    for (uint64_t i = 0; i + 1 < n; i++)
        if (seeds[i] >= seeds[i + 1])
            return fail(MADSIM_E_ARG, "the seed list must ascend strictly: seeds[" + std::to_string(i) + "] = " + std::to_string(seeds[i]) + " is not below seeds[" +
                                          std::to_string(i + 1) + "] = " + std::to_string(seeds[i + 1]) + " (sort it and drop duplicates)");
    return 0;
}
int check_seeds_args(const uint64_t* seeds, uint64_t n, uint64_t batch, uint32_t in_flight, uint32_t flags, const madsim_campaign_t* out,
                     const madsim_collect_t* col, const madsim_stats_t* st, const madsim_groups_t* grp) {
    if (int rc = check_seed_list(seeds, n)) return rc;
    if (!col) flags &= ~(MADSIM_CAMPAIGN_LIST_RUNNER | MADSIM_CAMPAIGN_STOP_AT_CAP);      // (flags of an absent part are ignored)
    if (!grp) flags &= ~MADSIM_CAMPAIGN_STOP_AT_GROUPS;
    return check_campaign_args(FORM_ANY, out, col, st, grp, n, batch, in_flight, flags);
}
}  // namespace

// ---- paired campaigns: per-seed metric deltas between two variants ------------------------------------------------------------------
// The differential entry points with a trailing madsim_paired_t and an optional diff report.  Argument errors first, as the other forms.
namespace {
int check_paired_args(const madsim_campaign_t* outA, const madsim_campaign_t* outB, const madsim_diff_t* d, const madsim_paired_t* pr, uint32_t in_flight,
                      uint32_t flags) {
    if (!pr) return fail(MADSIM_E_ARG, "null madsim_paired_t");
    if (pr->include_a == 0 || (pr->include_a & ~0xfu) || pr->include_b == 0 || (pr->include_b & ~0xfu))
        return fail(MADSIM_E_ARG, "madsim_paired_t.include_a / include_b: at least one of bits 0-3 (PASS, PANIC, DEADLOCK, TIME_LIMIT), none above");
    if (pr->reserved) return fail(MADSIM_E_ARG, "madsim_paired_t.reserved must be 0");
    if (pr->top_k > MADSIM_STAT_MAX_TOP) return fail(MADSIM_E_ARG, "madsim_paired_t.top_k: at most MADSIM_STAT_MAX_TOP (16)");
    if (pr->top_k && !pr->top) return fail(MADSIM_E_ARG, "madsim_paired_t.top_k > 0 without a top array");
    if (d) return check_diff_args(outA, outB, d, in_flight, flags);
    if (!outA || !outB) return fail(MADSIM_E_ARG, "null campaign report (a paired campaign fills one per side)");
    if (int rc = check_resolve_flags(flags)) return rc;
    if (in_flight > (uint32_t)madsim_hip_ctx::CAMPAIGN_MAX) return fail(MADSIM_E_ARG, "at most 8 batches in flight per context");
    return 0;
}
}  // namespace

// ---- sweep campaigns: up to eight variants over one seed set ------------------------------------------------------------------------
// Argument errors first, as the other forms — here the variants' validate() errors too, all told before any context is looked at.  `var`
// receives the variants with a NULL config replaced by the default one (loss 0, latency 1 .. 10 ms, no tables).
namespace {
const madsim_config_t g_default_config = [] { madsim_config_t c{}; c.lat_lo_ns = 1000000; c.lat_hi_ns = 10000000; return c; }();
int check_sweep_args(const madsim_sweep_variant_t* variants, uint32_t n_variants, uint64_t seed0, uint64_t total, const uint64_t* seeds, uint32_t in_flight,
                     uint32_t flags, const madsim_sweep_t* sw, std::vector<madsim_sweep_variant_t>& var) {
    if (n_variants < 2 || n_variants > MADSIM_SWEEP_MAX_VARIANTS) return fail(MADSIM_E_ARG, "a sweep campaign runs 2 .. MADSIM_SWEEP_MAX_VARIANTS (8) variants");
    if (!variants) return fail(MADSIM_E_ARG, "null variants array");
    if (!sw) return fail(MADSIM_E_ARG, "null madsim_sweep_t");
    for (uint32_t v = 0; v < n_variants; v++) {
        if (!variants[v].w) return fail(MADSIM_E_ARG, "variant " + std::to_string(v) + ": null workload");
        if (!variants[v].out) return fail(MADSIM_E_ARG, "variant " + std::to_string(v) + ": null campaign report (a sweep campaign fills one per variant)");
    }
    if (sw->fields & ~MADSIM_DIFF_ALL) return fail(MADSIM_E_ARG, "madsim_sweep_t.fields: no bit above MADSIM_DIFF_ALL");
    if (sw->list_rule > MADSIM_SWEEP_LIST_DIFFERING) return fail(MADSIM_E_ARG, "madsim_sweep_t.list_rule: one of MADSIM_SWEEP_LIST_*");
    if (sw->list_rule == MADSIM_SWEEP_LIST_DIFFERING && !sw->fields) return fail(MADSIM_E_ARG, "MADSIM_SWEEP_LIST_DIFFERING with fields == 0: nothing is compared");
    if (sw->cap && !sw->records) return fail(MADSIM_E_ARG, "madsim_sweep_t.cap > 0 without a records array");
    if ((flags & MADSIM_CAMPAIGN_STOP_AT_SWEEP) && !sw->cap) return fail(MADSIM_E_ARG, "MADSIM_CAMPAIGN_STOP_AT_SWEEP with cap == 0");
    if (seeds && seed0) return fail(MADSIM_E_ARG, "a sweep campaign over a seed list takes seed0 == 0");
    if (seeds) { if (int rc = check_seed_list(seeds, total)) return rc; }
    else if (seed0 + total < seed0) return fail(MADSIM_E_ARG, "seed0 + total wraps");
    if (int rc = check_resolve_flags(flags)) return rc;
    if (in_flight > (uint32_t)madsim_hip_ctx::CAMPAIGN_MAX) return fail(MADSIM_E_ARG, "at most 8 batches in flight per context");
    var.assign(variants, variants + n_variants);
    for (uint32_t v = 0; v < n_variants; v++) {
        if (!var[v].cfg) var[v].cfg = &g_default_config;
        if (int rc = madsim_geo::validate(var[v].w, var[v].cfg, &g_err)) return fail(rc, "variant " + std::to_string(v) + ": " + g_err);
    }
    return 0;
}
}  // namespace

// ---- the campaign operations, each written once against the contexts it runs on ------------------------------------------------------
// Every body: the argument errors that need no device, then the contexts (Contexts::enter), then the engine.  The entry points below, one per
// context form (madsim_hip_ctx_X) and one per _multi form (madsim_hip_X_multi), only say which contexts and which seeds.  (The bodies are
// static: inside this file's extern "C" block the library would export their plain names, and its list of symbols stays what it is.)
namespace {
// A call's seeds: the range [seed0, seed0 + total), or the strictly ascending list seeds[0 .. total), for which seed0 is 0.
struct Seeds {
    bool listed; uint64_t seed0, total; const uint64_t* seeds;
    static Seeds range(uint64_t seed0, uint64_t total) { return {false, seed0, total, nullptr}; }
    static Seeds list(const uint64_t* seeds, uint64_t n) { return {true, 0, n, seeds}; }
    bool empty_list() const { return listed && total == 0; }
    const uint64_t* engine_list() const { return total ? seeds : nullptr; }      // (the engines take a list by its pointer: none when it is empty)
};

// run_campaign, _collect, _stats, _groups (`form`: the part the range form cannot do without) and run_seeds_campaign.
static int plain_campaign(Contexts&& on, CampaignForm form, const madsim_workload_t* w, const madsim_config_t* cfg, const Seeds& s, uint64_t batch,
                   uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim, madsim_campaign_t* out, madsim_collect_t* col, madsim_stats_t* st,
                   madsim_groups_t* grp) {
    if (int rc = s.listed ? check_seeds_args(s.seeds, s.total, batch, in_flight, flags, out, col, st, grp)
                          : check_campaign_args(form, out, col, st, grp, s.total, batch, in_flight, flags))
        return rc;
    if (int rc = on.enter(s.empty_list())) return rc;
    return run_campaign_impl(on.ctxs(), on.n(), w, cfg, s.seed0, s.total, batch, in_flight, flags, lim, out, col, st, grp, s.engine_list());
}

// The differential and the paired forms, over a range or a list.  `paired`: the entry point takes a madsim_paired_t, and the diff report is optional.
static int pair_campaign(Contexts&& on, bool paired, const madsim_workload_t* wA, const madsim_config_t* cfgA, const madsim_limits_t* limA,
                  const madsim_workload_t* wB, const madsim_config_t* cfgB, const madsim_limits_t* limB, const Seeds& s, uint64_t batch, uint32_t in_flight,
                  uint32_t flags, madsim_campaign_t* outA, madsim_campaign_t* outB, madsim_diff_t* diff, madsim_paired_t* pr) {
    if (s.listed) if (int rc = check_seed_list(s.seeds, s.total)) return rc;
    if (int rc = paired ? check_paired_args(outA, outB, diff, pr, in_flight, flags) : check_diff_args(outA, outB, diff, in_flight, flags)) return rc;
    const madsim_sweep_variant_t side[2] = {{wA, cfgA, limA, outA}, {wB, cfgB, limB, outB}};
    if (int rc = on.enter(s.empty_list())) return rc;
    return run_variants_impl(on.ctxs(), on.n(), side, 2, s.seed0, s.total, batch, in_flight, flags, s.engine_list(), PairForm{diff, pr});
}

// The sweep form: one entry point for the range (seeds == NULL) and the list, so nothing to run is total == 0 either way.
static int sweep_campaign(Contexts&& on, const madsim_sweep_variant_t* variants, uint32_t n_variants, uint64_t seed0, uint64_t total, const uint64_t* seeds,
                   uint64_t batch, uint32_t in_flight, uint32_t flags, madsim_sweep_t* sweep) {
    std::vector<madsim_sweep_variant_t> var;
    if (int rc = check_sweep_args(variants, n_variants, seed0, total, seeds, in_flight, flags, sweep, var)) return rc;
    if (int rc = on.enter(total == 0)) return rc;
    return run_variants_impl(on.ctxs(), on.n(), var.data(), n_variants, seed0, total, batch, in_flight, flags, total ? seeds : nullptr,
                             SweepForm{sweep, n_variants});
}
}  // namespace

int madsim_hip_ctx_run_campaign(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total,
                                uint64_t batch, uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim, madsim_campaign_t* out) {
    return plain_campaign(Contexts(c), FORM_PLAIN, w, cfg, Seeds::range(seed0, total), batch, in_flight, flags, lim, out, nullptr, nullptr, nullptr);
}
int madsim_hip_run_campaign_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                  uint64_t seed0, uint64_t total, uint64_t batch, uint32_t in_flight, uint32_t flags,
                                  const madsim_limits_t* lim, madsim_campaign_t* out) {
    return plain_campaign(Contexts(ctxs, n_ctx, "run_campaign_multi"), FORM_PLAIN, w, cfg, Seeds::range(seed0, total), batch, in_flight, flags, lim, out,
                          nullptr, nullptr, nullptr);
}

int madsim_hip_ctx_run_campaign_collect(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total,
                                        uint64_t batch, uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim, madsim_campaign_t* out,
                                        madsim_collect_t* col) {
    return plain_campaign(Contexts(c), FORM_COLLECT, w, cfg, Seeds::range(seed0, total), batch, in_flight, flags, lim, out, col, nullptr, nullptr);
}
int madsim_hip_run_campaign_collect_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                          uint64_t seed0, uint64_t total, uint64_t batch, uint32_t in_flight, uint32_t flags,
                                          const madsim_limits_t* lim, madsim_campaign_t* out, madsim_collect_t* col) {
    return plain_campaign(Contexts(ctxs, n_ctx, "run_campaign_collect_multi"), FORM_COLLECT, w, cfg, Seeds::range(seed0, total), batch, in_flight, flags,
                          lim, out, col, nullptr, nullptr);
}

int madsim_hip_ctx_run_campaign_stats(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total,
                                      uint64_t batch, uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim, madsim_campaign_t* out,
                                      madsim_collect_t* col, madsim_stats_t* st) {
    return plain_campaign(Contexts(c), FORM_STATS, w, cfg, Seeds::range(seed0, total), batch, in_flight, flags, lim, out, col, st, nullptr);
}
int madsim_hip_run_campaign_stats_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                        uint64_t seed0, uint64_t total, uint64_t batch, uint32_t in_flight, uint32_t flags,
                                        const madsim_limits_t* lim, madsim_campaign_t* out, madsim_collect_t* col, madsim_stats_t* st) {
    return plain_campaign(Contexts(ctxs, n_ctx, "run_campaign_stats_multi"), FORM_STATS, w, cfg, Seeds::range(seed0, total), batch, in_flight, flags, lim,
                          out, col, st, nullptr);
}

int madsim_hip_ctx_run_campaign_groups(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total,
                                       uint64_t batch, uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim, madsim_campaign_t* out,
                                       madsim_collect_t* col, madsim_stats_t* st, madsim_groups_t* grp) {
    return plain_campaign(Contexts(c), FORM_GROUPS, w, cfg, Seeds::range(seed0, total), batch, in_flight, flags, lim, out, col, st, grp);
}
int madsim_hip_run_campaign_groups_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                         uint64_t seed0, uint64_t total, uint64_t batch, uint32_t in_flight, uint32_t flags,
                                         const madsim_limits_t* lim, madsim_campaign_t* out, madsim_collect_t* col, madsim_stats_t* st,
                                         madsim_groups_t* grp) {
    return plain_campaign(Contexts(ctxs, n_ctx, "run_campaign_groups_multi"), FORM_GROUPS, w, cfg, Seeds::range(seed0, total), batch, in_flight, flags,
                          lim, out, col, st, grp);
}

int madsim_hip_ctx_run_seeds_campaign(madsim_hip_ctx_t* c, const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n,
                                      uint64_t batch, uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim, madsim_campaign_t* out,
                                      madsim_collect_t* col, madsim_stats_t* st, madsim_groups_t* grp) {
    return plain_campaign(Contexts(c), FORM_ANY, w, cfg, Seeds::list(seeds, n), batch, in_flight, flags, lim, out, col, st, grp);
}
int madsim_hip_run_seeds_campaign_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                        const uint64_t* seeds, uint64_t n, uint64_t batch, uint32_t in_flight, uint32_t flags,
                                        const madsim_limits_t* lim, madsim_campaign_t* out, madsim_collect_t* col, madsim_stats_t* st,
                                        madsim_groups_t* grp) {
    return plain_campaign(Contexts(ctxs, n_ctx, "run_seeds_campaign_multi"), FORM_ANY, w, cfg, Seeds::list(seeds, n), batch, in_flight, flags, lim, out,
                          col, st, grp);
}

int madsim_hip_ctx_run_campaign_diff(madsim_hip_ctx_t* c, const madsim_workload_t* wA, const madsim_config_t* cfgA, const madsim_limits_t* limA,
                                     const madsim_workload_t* wB, const madsim_config_t* cfgB, const madsim_limits_t* limB, uint64_t seed0,
                                     uint64_t total, uint64_t batch, uint32_t in_flight, uint32_t flags, madsim_campaign_t* outA,
                                     madsim_campaign_t* outB, madsim_diff_t* diff) {
    return pair_campaign(Contexts(c), false, wA, cfgA, limA, wB, cfgB, limB, Seeds::range(seed0, total), batch, in_flight, flags, outA, outB, diff, nullptr);
}
int madsim_hip_run_campaign_diff_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* wA, const madsim_config_t* cfgA,
                                       const madsim_limits_t* limA, const madsim_workload_t* wB, const madsim_config_t* cfgB,
                                       const madsim_limits_t* limB, uint64_t seed0, uint64_t total, uint64_t batch, uint32_t in_flight,
                                       uint32_t flags, madsim_campaign_t* outA, madsim_campaign_t* outB, madsim_diff_t* diff) {
    return pair_campaign(Contexts(ctxs, n_ctx, "run_campaign_diff_multi"), false, wA, cfgA, limA, wB, cfgB, limB, Seeds::range(seed0, total), batch,
                         in_flight, flags, outA, outB, diff, nullptr);
}

int madsim_hip_ctx_run_seeds_campaign_diff(madsim_hip_ctx_t* c, const madsim_workload_t* wA, const madsim_config_t* cfgA, const madsim_limits_t* limA,
                                           const madsim_workload_t* wB, const madsim_config_t* cfgB, const madsim_limits_t* limB,
                                           const uint64_t* seeds, uint64_t n, uint64_t batch, uint32_t in_flight, uint32_t flags,
                                           madsim_campaign_t* outA, madsim_campaign_t* outB, madsim_diff_t* diff) {
    return pair_campaign(Contexts(c), false, wA, cfgA, limA, wB, cfgB, limB, Seeds::list(seeds, n), batch, in_flight, flags, outA, outB, diff, nullptr);
}
int madsim_hip_run_seeds_campaign_diff_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* wA, const madsim_config_t* cfgA,
                                             const madsim_limits_t* limA, const madsim_workload_t* wB, const madsim_config_t* cfgB,
                                             const madsim_limits_t* limB, const uint64_t* seeds, uint64_t n, uint64_t batch, uint32_t in_flight,
                                             uint32_t flags, madsim_campaign_t* outA, madsim_campaign_t* outB, madsim_diff_t* diff) {
    return pair_campaign(Contexts(ctxs, n_ctx, "run_seeds_campaign_diff_multi"), false, wA, cfgA, limA, wB, cfgB, limB, Seeds::list(seeds, n), batch,
                         in_flight, flags, outA, outB, diff, nullptr);
}

int madsim_hip_ctx_run_paired_campaign(madsim_hip_ctx_t* c, const madsim_workload_t* wA, const madsim_config_t* cfgA, const madsim_limits_t* limA,
                                       const madsim_workload_t* wB, const madsim_config_t* cfgB, const madsim_limits_t* limB, uint64_t seed0,
                                       uint64_t total, uint64_t batch, uint32_t in_flight, uint32_t flags, madsim_campaign_t* outA,
                                       madsim_campaign_t* outB, madsim_diff_t* diff, madsim_paired_t* pr) {
    return pair_campaign(Contexts(c), true, wA, cfgA, limA, wB, cfgB, limB, Seeds::range(seed0, total), batch, in_flight, flags, outA, outB, diff, pr);
}
int madsim_hip_run_paired_campaign_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* wA, const madsim_config_t* cfgA,
                                         const madsim_limits_t* limA, const madsim_workload_t* wB, const madsim_config_t* cfgB,
                                         const madsim_limits_t* limB, uint64_t seed0, uint64_t total, uint64_t batch, uint32_t in_flight,
                                         uint32_t flags, madsim_campaign_t* outA, madsim_campaign_t* outB, madsim_diff_t* diff, madsim_paired_t* pr) {
    return pair_campaign(Contexts(ctxs, n_ctx, "run_paired_campaign_multi"), true, wA, cfgA, limA, wB, cfgB, limB, Seeds::range(seed0, total), batch,
                         in_flight, flags, outA, outB, diff, pr);
}

int madsim_hip_ctx_run_seeds_campaign_paired(madsim_hip_ctx_t* c, const madsim_workload_t* wA, const madsim_config_t* cfgA, const madsim_limits_t* limA,
                                             const madsim_workload_t* wB, const madsim_config_t* cfgB, const madsim_limits_t* limB,
                                             const uint64_t* seeds, uint64_t n, uint64_t batch, uint32_t in_flight, uint32_t flags,
                                             madsim_campaign_t* outA, madsim_campaign_t* outB, madsim_diff_t* diff, madsim_paired_t* pr) {
    return pair_campaign(Contexts(c), true, wA, cfgA, limA, wB, cfgB, limB, Seeds::list(seeds, n), batch, in_flight, flags, outA, outB, diff, pr);
}
int madsim_hip_run_seeds_campaign_paired_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* wA, const madsim_config_t* cfgA,
                                               const madsim_limits_t* limA, const madsim_workload_t* wB, const madsim_config_t* cfgB,
                                               const madsim_limits_t* limB, const uint64_t* seeds, uint64_t n, uint64_t batch, uint32_t in_flight,
                                               uint32_t flags, madsim_campaign_t* outA, madsim_campaign_t* outB, madsim_diff_t* diff,
                                               madsim_paired_t* pr) {
    return pair_campaign(Contexts(ctxs, n_ctx, "run_seeds_campaign_paired_multi"), true, wA, cfgA, limA, wB, cfgB, limB, Seeds::list(seeds, n), batch,
                         in_flight, flags, outA, outB, diff, pr);
}

int madsim_hip_ctx_run_sweep_campaign(madsim_hip_ctx_t* c, const madsim_sweep_variant_t* variants, uint32_t n_variants, uint64_t seed0, uint64_t total,
                                      const uint64_t* seeds, uint64_t batch, uint32_t in_flight, uint32_t flags, madsim_sweep_t* sweep) {
    return sweep_campaign(Contexts(c), variants, n_variants, seed0, total, seeds, batch, in_flight, flags, sweep);
}
int madsim_hip_run_sweep_campaign_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_sweep_variant_t* variants, uint32_t n_variants,
                                        uint64_t seed0, uint64_t total, const uint64_t* seeds, uint64_t batch, uint32_t in_flight, uint32_t flags,
                                        madsim_sweep_t* sweep) {
    return sweep_campaign(Contexts(ctxs, n_ctx, "run_sweep_campaign_multi"), variants, n_variants, seed0, total, seeds, batch, in_flight, flags, sweep);
}

// ---- v1 entry points: wrappers on the process-default context ------------------------------------------------------------
// The default context is reference-counted by its users: a wrapper pins it under g_default_mu for the duration of its call,
// and madsim_hip_shutdown waits until no call is inside before destroying it — a concurrent run_batch and shutdown is a
// clean "not initialised" for whichever comes second, never a use-after-free.

namespace {
int g_default_users = 0;
std::condition_variable g_default_cv;
struct DefaultPin {
    madsim_hip_ctx* c;
    DefaultPin() { std::lock_guard<std::mutex> lk(g_default_mu); c = g_default; if (c) g_default_users++; }
    ~DefaultPin() { if (c) { std::lock_guard<std::mutex> lk(g_default_mu); if (--g_default_users == 0) g_default_cv.notify_all(); } }
};
}  // namespace

int madsim_hip_init(int device) {
    std::lock_guard<std::mutex> lk(g_default_mu);
    if (g_default) {
        if (g_default->device == device) { HIP_TRY(hipSetDevice(device)); return 0; }
        return fail(MADSIM_E_ARG, "the default context is bound to another GPU: call madsim_hip_shutdown first, or hold one "
                                  "madsim_hip_ctx_t per GPU (madsim_hip_ctx_create)");
    }
    return madsim_hip_ctx_create(device, &g_default);
}

int madsim_hip_shutdown(void) {
    madsim_hip_ctx* c;
    {
        std::unique_lock<std::mutex> lk(g_default_mu);
        c = g_default;
        g_default = nullptr;                                   // later calls see "not initialised"
        g_default_cv.wait(lk, [] { return g_default_users == 0; });
    }
    return madsim_hip_ctx_destroy(c);
}

madsim_hip_ctx_t* madsim_hip_default_ctx(void) { std::lock_guard<std::mutex> lk(g_default_mu); return g_default; }

int madsim_hip_run_batch(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t count,
                         const madsim_limits_t* lim, madsim_result_t* out, madsim_summary_t* summary) {
    DefaultPin p;
    return madsim_hip_ctx_run_batch(p.c, w, cfg, seed0, count, lim, out, summary);
}

int madsim_hip_run_batch_auto(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t count,
                              const madsim_limits_t* lim, madsim_result_t* out, madsim_summary_t* summary, int max_rounds) {
    DefaultPin p;
    return madsim_hip_ctx_run_batch_auto(p.c, w, cfg, seed0, count, lim, out, summary, max_rounds);
}

int madsim_hip_run_batch_device(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t count,
                                const madsim_limits_t* lim, void* d_out, void* stream, madsim_summary_t* summary) {
    DefaultPin p;
    return madsim_hip_ctx_run_batch_device(p.c, w, cfg, seed0, count, lim, d_out, stream, summary);
}

int madsim_hip_run_batch_async(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t count,
                               const madsim_limits_t* lim, void* d_out, void* d_summary4, void* stream, int timing_slot) {
    DefaultPin p;
    return madsim_hip_ctx_run_batch_async(p.c, w, cfg, seed0, count, lim, d_out, d_summary4, stream, timing_slot);
}

int madsim_hip_timing_ms(int timing_slot, double* ms) { DefaultPin p; return madsim_hip_ctx_timing_ms(p.c, timing_slot, ms); }

int madsim_hip_campaign_resolved(madsim_resolve_t* out) {
    DefaultPin p;
    if (out && !p.c) { memset(out, 0, sizeof *out); return 0; }      // no default context: no campaign has run through it
    return madsim_hip_ctx_campaign_resolved(p.c, out);
}

int64_t madsim_hip_trace_seed(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed,
                              const madsim_limits_t* lim, uint8_t* log, uint64_t cap, madsim_result_t* out) {
    DefaultPin p;
    return madsim_hip_ctx_trace_seed(p.c, w, cfg, seed, lim, log, cap, out);
}

int madsim_hip_task_states(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n, const madsim_limits_t* lim,
                           uint64_t* tasks, uint64_t task_cap, uint64_t* task_len, madsim_result_t* out) {
    DefaultPin p;
    return madsim_hip_ctx_task_states(p.c, w, cfg, seeds, n, lim, tasks, task_cap, task_len, out);
}

int madsim_hip_timeline_seeds(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n, const madsim_limits_t* lim,
                              uint64_t* obs, uint64_t* times, uint64_t obs_cap, uint64_t* obs_len, madsim_result_t* out) {
    DefaultPin p;
    return madsim_hip_ctx_timeline_seeds(p.c, w, cfg, seeds, n, lim, obs, times, obs_cap, obs_len, out);
}

int madsim_hip_trace_seeds(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n, const madsim_limits_t* lim,
                           uint8_t* logs, uint64_t log_cap, uint64_t* obs, uint64_t obs_cap, uint64_t* log_len, uint64_t* obs_len,
                           madsim_result_t* out) {
    DefaultPin p;
    return madsim_hip_ctx_trace_seeds(p.c, w, cfg, seeds, n, lim, logs, log_cap, obs, obs_cap, log_len, obs_len, out);
}

int64_t madsim_hip_observe_seed(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed, const madsim_limits_t* lim,
                                uint64_t* obs, uint64_t cap, madsim_result_t* out) {
    DefaultPin p;
    return madsim_hip_ctx_observe_seed(p.c, w, cfg, seed, lim, obs, cap, out);
}

int madsim_hip_diverge_seeds(const madsim_workload_t* wA, const madsim_config_t* cfgA, const madsim_limits_t* limA, const madsim_workload_t* wB,
                             const madsim_config_t* cfgB, const madsim_limits_t* limB, const uint64_t* seeds, uint64_t n, uint64_t log_cap,
                             uint64_t obs_cap, uint32_t win, madsim_divergence_t* recs, uint64_t* obs_ctx) {
    DefaultPin p;
    return madsim_hip_ctx_diverge_seeds(p.c, wA, cfgA, limA, wB, cfgB, limB, seeds, n, log_cap, obs_cap, win, recs, obs_ctx);
}

int madsim_hip_census_range(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total, uint64_t chunk,
                            const madsim_limits_t* lim, madsim_census_t* cen) {
    DefaultPin p;
    return madsim_hip_ctx_census_range(p.c, w, cfg, seed0, total, chunk, lim, cen);
}

int madsim_hip_census_seeds(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n, uint64_t chunk,
                            const madsim_limits_t* lim, madsim_census_t* cen) {
    DefaultPin p;
    return madsim_hip_ctx_census_seeds(p.c, w, cfg, seeds, n, chunk, lim, cen);
}

int madsim_hip_stall_census_range(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total, uint64_t chunk,
                                  const madsim_limits_t* lim, madsim_stall_census_t* sc) {
    DefaultPin p;
    return madsim_hip_ctx_stall_census_range(p.c, w, cfg, seed0, total, chunk, lim, sc);
}

int madsim_hip_stall_census_seeds(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n, uint64_t chunk,
                                  const madsim_limits_t* lim, madsim_stall_census_t* sc) {
    DefaultPin p;
    return madsim_hip_ctx_stall_census_seeds(p.c, w, cfg, seeds, n, chunk, lim, sc);
}

int madsim_hip_probe_sets_range(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total, uint64_t chunk,
                                const madsim_limits_t* lim, madsim_probe_sets_t* ps) {
    DefaultPin p;
    return madsim_hip_ctx_probe_sets_range(p.c, w, cfg, seed0, total, chunk, lim, ps);
}

int madsim_hip_probe_sets_seeds(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n, uint64_t chunk,
                                const madsim_limits_t* lim, madsim_probe_sets_t* ps) {
    DefaultPin p;
    return madsim_hip_ctx_probe_sets_seeds(p.c, w, cfg, seeds, n, chunk, lim, ps);
}

int madsim_hip_probe_spans_range(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total, uint64_t chunk,
                                 const madsim_limits_t* lim, madsim_probe_spans_t* ps) {
    DefaultPin p;
    return madsim_hip_ctx_probe_spans_range(p.c, w, cfg, seed0, total, chunk, lim, ps);
}

int madsim_hip_probe_spans_seeds(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n, uint64_t chunk,
                                 const madsim_limits_t* lim, madsim_probe_spans_t* ps) {
    DefaultPin p;
    return madsim_hip_ctx_probe_spans_seeds(p.c, w, cfg, seeds, n, chunk, lim, ps);
}

int madsim_hip_probe_order_range(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total, uint64_t chunk,
                                 const madsim_limits_t* lim, madsim_probe_order_t* po) {
    DefaultPin p;
    return madsim_hip_ctx_probe_order_range(p.c, w, cfg, seed0, total, chunk, lim, po);
}

int madsim_hip_probe_order_seeds(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n, uint64_t chunk,
                                 const madsim_limits_t* lim, madsim_probe_order_t* po) {
    DefaultPin p;
    return madsim_hip_ctx_probe_order_seeds(p.c, w, cfg, seeds, n, chunk, lim, po);
}

int madsim_hip_run_campaign(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total, uint64_t batch,
                            uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim, madsim_campaign_t* out) {
    DefaultPin p;
    return madsim_hip_ctx_run_campaign(p.c, w, cfg, seed0, total, batch, in_flight, flags, lim, out);
}

int madsim_hip_run_campaign_collect(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total, uint64_t batch,
                                    uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim, madsim_campaign_t* out, madsim_collect_t* col) {
    DefaultPin p;
    return madsim_hip_ctx_run_campaign_collect(p.c, w, cfg, seed0, total, batch, in_flight, flags, lim, out, col);
}

int madsim_hip_run_campaign_stats(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total, uint64_t batch,
                                  uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim, madsim_campaign_t* out, madsim_collect_t* col,
                                  madsim_stats_t* st) {
    DefaultPin p;
    return madsim_hip_ctx_run_campaign_stats(p.c, w, cfg, seed0, total, batch, in_flight, flags, lim, out, col, st);
}

int madsim_hip_run_campaign_groups(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total, uint64_t batch,
                                   uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim, madsim_campaign_t* out, madsim_collect_t* col,
                                   madsim_stats_t* st, madsim_groups_t* grp) {
    DefaultPin p;
    return madsim_hip_ctx_run_campaign_groups(p.c, w, cfg, seed0, total, batch, in_flight, flags, lim, out, col, st, grp);
}

int madsim_hip_run_campaign_diff(const madsim_workload_t* wA, const madsim_config_t* cfgA, const madsim_limits_t* limA, const madsim_workload_t* wB,
                                 const madsim_config_t* cfgB, const madsim_limits_t* limB, uint64_t seed0, uint64_t total, uint64_t batch,
                                 uint32_t in_flight, uint32_t flags, madsim_campaign_t* outA, madsim_campaign_t* outB, madsim_diff_t* diff) {
    DefaultPin p;
    return madsim_hip_ctx_run_campaign_diff(p.c, wA, cfgA, limA, wB, cfgB, limB, seed0, total, batch, in_flight, flags, outA, outB, diff);
}

int madsim_hip_run_seeds_campaign(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n, uint64_t batch,
                                  uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim, madsim_campaign_t* out, madsim_collect_t* col,
                                  madsim_stats_t* st, madsim_groups_t* grp) {
    DefaultPin p;
    return madsim_hip_ctx_run_seeds_campaign(p.c, w, cfg, seeds, n, batch, in_flight, flags, lim, out, col, st, grp);
}

int madsim_hip_run_seeds_campaign_diff(const madsim_workload_t* wA, const madsim_config_t* cfgA, const madsim_limits_t* limA, const madsim_workload_t* wB,
                                       const madsim_config_t* cfgB, const madsim_limits_t* limB, const uint64_t* seeds, uint64_t n, uint64_t batch,
                                       uint32_t in_flight, uint32_t flags, madsim_campaign_t* outA, madsim_campaign_t* outB, madsim_diff_t* diff) {
    DefaultPin p;
    return madsim_hip_ctx_run_seeds_campaign_diff(p.c, wA, cfgA, limA, wB, cfgB, limB, seeds, n, batch, in_flight, flags, outA, outB, diff);
}

int madsim_hip_run_paired_campaign(const madsim_workload_t* wA, const madsim_config_t* cfgA, const madsim_limits_t* limA, const madsim_workload_t* wB,
                                   const madsim_config_t* cfgB, const madsim_limits_t* limB, uint64_t seed0, uint64_t total, uint64_t batch,
                                   uint32_t in_flight, uint32_t flags, madsim_campaign_t* outA, madsim_campaign_t* outB, madsim_diff_t* diff,
                                   madsim_paired_t* pr) {
    DefaultPin p;
    return madsim_hip_ctx_run_paired_campaign(p.c, wA, cfgA, limA, wB, cfgB, limB, seed0, total, batch, in_flight, flags, outA, outB, diff, pr);
}

int madsim_hip_run_seeds_campaign_paired(const madsim_workload_t* wA, const madsim_config_t* cfgA, const madsim_limits_t* limA, const madsim_workload_t* wB,
                                         const madsim_config_t* cfgB, const madsim_limits_t* limB, const uint64_t* seeds, uint64_t n, uint64_t batch,
                                         uint32_t in_flight, uint32_t flags, madsim_campaign_t* outA, madsim_campaign_t* outB, madsim_diff_t* diff,
                                         madsim_paired_t* pr) {
    DefaultPin p;
    return madsim_hip_ctx_run_seeds_campaign_paired(p.c, wA, cfgA, limA, wB, cfgB, limB, seeds, n, batch, in_flight, flags, outA, outB, diff, pr);
}

int madsim_hip_run_sweep_campaign(const madsim_sweep_variant_t* variants, uint32_t n_variants, uint64_t seed0, uint64_t total, const uint64_t* seeds,
                                  uint64_t batch, uint32_t in_flight, uint32_t flags, madsim_sweep_t* sweep) {
    DefaultPin p;
    return madsim_hip_ctx_run_sweep_campaign(p.c, variants, n_variants, seed0, total, seeds, batch, in_flight, flags, sweep);
}

int madsim_hip_geometry(const madsim_workload_t* w, const madsim_limits_t* lim, madsim_geometry_t* out) {
    if (!out) return fail(MADSIM_E_ARG, "null geometry");
    madsim_config_t cfg = madsim_geo::probe_config();
    int rc = madsim_geo::validate(w, &cfg, &g_err);
    if (rc) return rc;
    Geo G;
    madsim_geo::Device d;
    { std::lock_guard<std::mutex> lk(g_default_mu); if (g_default) d = g_default->dev(); }
    if ((rc = madsim_geo::make_geometry(d, w, &cfg, lim, UINT64_MAX / 2, &G, &g_err))) return rc;
    out->lds_bytes_per_seed = G.lds_per_seed; out->lds_bytes_per_block = G.lds_bytes; out->block_threads = 64 * G.waves_per_block;
    out->blocks_per_cu = G.blocks_per_cu; out->grid_blocks = G.grid; out->heap_lds_slots = G.P.heap_lds;
    out->heap_spill_slots = G.P.heap_spill; out->max_tasks = G.P.max_tasks; out->lanes_per_wave = G.lanes_per_wave;
    const madsim_k::VariantSel v = madsim_k::select_variant(G.P, false);
    out->variant = (v.spill ? 1u : 0u) | ((v.feat & MADSIM_FEAT_ALL) ? 2u : 0u) | (v.rq ? 4u : 0u) | (v.lws < 0 ? 8u : 0u) | (v.g ? 16u : 0u) | ((uint32_t)(v.feat & 0xff) << 8) | ((uint32_t)(v.lws & 0xf) << 16)
                 | (uint32_t)(v.feat & (MADSIM_FEAT_TIERS | MADSIM_FEAT_SIGNAL)) >> 8 << 20;     // bits 20-22: the timer-op tier, MADSIM_FEAT_SCOPE / TICK / SELECT in order; bit 23: MADSIM_FEAT_SIGNAL
    out->global_bytes_per_seed = G.P.gstate_mode ? G.P.gs_stride : 0;
    return 0;
}

// Debug: read and clear the per-phase cycle accumulators a profiling kernel build fills (zeros otherwise).
int madsim_hip_debug_counters(uint64_t* out16) {
    DefaultPin pin;
    madsim_hip_ctx* c = pin.c;
    CTX_ENTER(c);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out16, c->d_prof, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(c->d_prof, 0, 16 * sizeof(uint64_t)));
    return 0;
}

// SURVEY.md §8d workload.  Mirrors madsim_amd/workload.py::pingpong instruction for instruction.
int madsim_workload_pingpong(uint32_t n_nodes, uint32_t rounds, madsim_node_t* nodes, madsim_prog_t* progs,
                             madsim_sock_t* socks, madsim_insn_t* insns, uint32_t cap_insns, madsim_workload_t* w) {
    if (!nodes || !progs || !socks || !insns || !w || n_nodes < 2 || (n_nodes & 1) || n_nodes > 31 || rounds == 0 || rounds > 0xffff)
        return fail(MADSIM_E_ARG, "pingpong: need an even node count in 2..30 and 1..65535 rounds");
    const uint32_t PING = 0x676E6970u, PONG = 0x676E6F70u;
    uint32_t need = 2 * n_nodes + 1 + (n_nodes / 2) * (8 + 7);
    if (cap_insns < need) return fail(MADSIM_E_ARG, "pingpong: instruction buffer too small");
    uint32_t n = 0;
    auto emit = [&](uint8_t op, uint8_t a, uint16_t b, uint32_t imm) { insns[n++] = madsim_insn_t{op, a, b, imm}; };
    memset(nodes, 0, (n_nodes + 1) * sizeof *nodes);
    for (uint32_t i = 0; i < n_nodes; i++) socks[i] = madsim_sock_t{(uint8_t)(i + 1), 0, 1};
    // main: spawn every task in node order, then await every JoinHandle in order
    progs[0] = madsim_prog_t{0, 0, 0};
    for (uint32_t i = 0; i < n_nodes; i++) emit(MS_OP_SPAWN, (uint8_t)(i + 1), 0, 0);
    for (uint32_t i = 0; i < n_nodes; i++) emit(MS_OP_JOIN, (uint8_t)(i + 1), 0, 0);
    emit(MS_OP_DONE, 0, 0, 0);
    for (uint32_t i = 0; i < n_nodes; i++) {
        progs[i + 1] = madsim_prog_t{(uint8_t)(i + 1), 0, (uint16_t)n};
        emit(MS_OP_BIND, (uint8_t)i, 0, 0);
        if ((i & 1) == 0) {            // pinger
            emit(MS_OP_SLEEP, 0, 1, 0);
            emit(MS_OP_SET, 0, 0, rounds);
            uint16_t top = (uint16_t)n;
            emit(MS_OP_SEND, (uint8_t)i, (uint16_t)((1u << 8) | (i + 1)), PING);
            emit(MS_OP_RECV, (uint8_t)i, 1u << 8, 0);
            emit(MS_OP_ASSERT_VAL, 0, 0, PONG);
            emit(MS_OP_DJNZ, 0, top, 0);
        } else {                       // ponger
            emit(MS_OP_SET, 0, 0, rounds);
            uint16_t top = (uint16_t)n;
            emit(MS_OP_RECV, (uint8_t)i, 1u << 8, 0);
            emit(MS_OP_ASSERT_VAL, 0, 0, PING);
            emit(MS_OP_REPLY, (uint8_t)i, 1u << 8, PONG);
            emit(MS_OP_DJNZ, 0, top, 0);
        }
        emit(MS_OP_DONE, 0, 0, 0);
    }
    memset(w, 0, sizeof *w);              // no services, no restart rows: every field of the struct is defined
    w->n_nodes = n_nodes; w->n_progs = n_nodes + 1; w->n_socks = n_nodes; w->n_insns = n;
    w->nodes = nodes; w->progs = progs; w->socks = socks; w->insns = insns;
    return (int)n;
}

}  // extern "C"
