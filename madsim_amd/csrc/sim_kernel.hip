// sim_kernel.hip — the many-seed executor kernel for gfx950 (MI355X, CDNA4).
//
// ONE LANE = ONE SEED.  A workgroup is up to four independent 64-lane wavefronts (one per SIMD of a CU) that share
// nothing but the read-only workload tables.  Each lane runs madsim's whole per-seed executor loop:
//     Executor::block_on / run_all_ready       madsim/src/sim/task/mod.rs:220-323
//     mpsc::Receiver::try_recv_random          madsim/src/sim/utils/mpsc.rs:73-83
//     TimeRuntime::advance_to_next_event       madsim/src/sim/time/mod.rs:45-60
//     TimeHandle::advance / Sleep::poll        time/mod.rs:103-124, time/sleep.rs:47-54
//     GlobalRng (xoshiro256++, gen_range ...)  madsim/src/sim/rand.rs:27-158
//     NetSim::send / Network::try_send / Mailbox   net/mod.rs:287-333, net/network.rs:261-313,
//                                                  net/endpoint.rs:331-362
// on a workload given as an actor program (include/madsim_hip.h).
//
// Data placement (per seed):
//   VGPRs : xoshiro256++ state (4 x u64), clock, counters, hashes, queue lengths.
//   LDS   : timer heap (16-byte entries, [slot][lane] => ds_read/write_b128, conflict-free),
//           lane stride = lw, the number of seed-carrying lanes per wave (8..64, see geometry.h),
//           task table, ready queue, mailboxes, handles, node/clog masks — all as 32-bit
//           "word planes" [word][lane] so that any per-lane dynamic index hits bank = lane % 32.
//           The workload tables (instructions, programs, socket addresses) sit once per
//           workgroup in front of the planes.
//   HBM   : heap entries beyond the LDS quota spill to a [slot][global lane] region
//           (adjacent lanes -> adjacent 16-byte entries: coalesced), results 48 B/seed.
//
// Integer/indexing work only: no MFMA.  No inter-lane communication: lanes only share the
// instruction stream, so there is no barrier anywhere in the kernel.
#include <cstdlib>

#include "kernel/k_mem.h"
#include "sim_kernel.h"

#include "kernel/k_state.h"
#include "kernel/k_rng.h"
#include "kernel/k_timer.h"
#include "kernel/k_net.h"
#include "kernel/k_lifecycle.h"
#include "kernel/k_channel.h"
#include "kernel/k_poll.h"
#include "kernel/k_main.h"

namespace madsim_k {

// ---- summary reduction over the result array (first failing seed = min) -------------------------
__global__ __launch_bounds__(256) void summary_kernel(const madsim_result_t* __restrict__ out, uint64_t count,
                                                      uint64_t seed0, unsigned long long* __restrict__ acc) {
    __shared__ unsigned long long part[4][4];
    unsigned long long first = ~0ull, nfail = 0, steps = 0, clk = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint4* p = reinterpret_cast<const uint4*>(out + i);     // verdict|steps|clock_ns in the first 16 bytes
        uint4 r = p[0];
        if (r.x != MADSIM_PASS) { nfail++; unsigned long long s = seed0 + i; first = s < first ? s : first; }
        steps += r.y; clk += ((unsigned long long)r.w << 32) | r.z;
    }
    for (int o = 32; o > 0; o >>= 1) {
        unsigned long long f2 = __shfl_xor(first, o), n2 = __shfl_xor(nfail, o), s2 = __shfl_xor(steps, o), c2 = __shfl_xor(clk, o);
        first = f2 < first ? f2 : first; nfail += n2; steps += s2; clk += c2;
    }
    const uint32_t wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[wv][0] = first; part[wv][1] = nfail; part[wv][2] = steps; part[wv][3] = clk; }
    __syncthreads();
    if (threadIdx.x == 0) {                                             // one set of atomics per workgroup
        for (int k = 1; k < 4; k++) {
            first = part[k][0] < first ? part[k][0] : first; nfail += part[k][1]; steps += part[k][2]; clk += part[k][3];
        }
        atomicMin(&acc[0], first); atomicAdd(&acc[1], nfail); atomicAdd(&acc[2], steps); atomicAdd(&acc[3], clk);
    }
}

// Where a report kernel takes the seed of result i from: the range forms' seed0 + i, or entry i of the batch's slice of a seed list (the list
// campaigns, madsim_hip_run_seeds_campaign: the list ascends strictly, so every "ascending position" below is still "ascending seed").
// A compile-time switch — the RangeSeeds instantiation is the kernel as it was, the 8 bytes of seed0 in the same kernel-argument slot —
// and a list entry is loaded only inside the branch that uses the seed (a failing, listed, extreme or re-runnable result): the lanes
// outside it are masked off and issue no load, and a wave none of whose lanes takes the branch skips it, so a batch of passing seeds
// reads nothing of its list here.
struct RangeSeeds { uint64_t seed0; __device__ __forceinline__ unsigned long long operator()(uint64_t i) const { return seed0 + i; } };
struct ListSeeds  { const uint64_t* __restrict__ d; __device__ __forceinline__ unsigned long long operator()(uint64_t i) const { return d[i]; } };

// the campaign form: also tells the RUNNER verdicts (device capacity, step cap: not reference verdicts) from genuine failures —
// acc6 = {first failing seed, n_failed, steps, clock, first seed with a GENUINE verdict (panic / deadlock / time limit), n runner verdicts}
template <class Seeds>
__global__ __launch_bounds__(256) void summary6_kernel(const madsim_result_t* __restrict__ out, uint64_t count,
                                                       const Seeds seed_of, unsigned long long* __restrict__ acc) {
    unsigned long long first = ~0ull, nfail = 0, steps = 0, clk = 0, gfirst = ~0ull, nrun = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 r = reinterpret_cast<const uint4*>(out + i)[0];
        if (r.x != MADSIM_PASS) {
            const unsigned long long s = seed_of(i);
            nfail++; first = s < first ? s : first;
            if (MADSIM_IS_RUNNER_VERDICT(r.x)) nrun++; else gfirst = s < gfirst ? s : gfirst;
        }
        steps += r.y; clk += ((unsigned long long)r.w << 32) | r.z;
    }
    for (int o = 32; o > 0; o >>= 1) {
        unsigned long long f2 = __shfl_xor(first, o), g2 = __shfl_xor(gfirst, o);
        first = f2 < first ? f2 : first; gfirst = g2 < gfirst ? g2 : gfirst;
        nfail += __shfl_xor(nfail, o); steps += __shfl_xor(steps, o); clk += __shfl_xor(clk, o); nrun += __shfl_xor(nrun, o);
    }
    if ((threadIdx.x & 63) == 0) {                                      // one set of atomics per wave (<= 1 024 per launch)
        atomicMin(&acc[0], first); atomicAdd(&acc[1], nfail); atomicAdd(&acc[2], steps); atomicAdd(&acc[3], clk);
        atomicMin(&acc[4], gfirst); atomicAdd(&acc[5], nrun);
    }
}

// ---- the collecting campaign form: summary6's six words, a histogram of the verdicts and the ORDERED list of the failing seeds ----
// Two kernels over the same cut of the batch: wave W (= 4 * workgroup + wave of the workgroup, COLLECT_MAX_WAVES at most) owns the
// contiguous piece [W * piece, (W + 1) * piece) of the result array, so "ascending wave, ascending position in the wave" IS ascending
// seed order whatever the grid.  collect_count_kernel reads 16 B per seed (as the summary kernels do), folds the report and leaves
// every wave's number of listed seeds in wave_cnt[W]; collect_write_kernel gives a wave the exclusive prefix of wave_cnt as its offset
// into the record array, and only a wave that has listed seeds AND an offset below `cap` reads its piece again — failures are rare and
// the list is short, so the second kernel touches a few pieces (a 65 536-seed batch: 64 seeds, 1 KB, per piece).  No atomic decides a
// position: the list is the same on every run.
// rep = {acc6[0..5] as summary6_kernel, by_verdict[0..7], n listed} (15 words; 0xff words 0 and 4, the rest 0 before the launch).
// Listed = a genuine verdict (panic / deadlock / time limit), or any verdict but PASS when list_runner is set.
constexpr uint32_t COLLECT_MAX_WAVES = 1024;          // 256 workgroups of 4 waves
constexpr uint32_t COLLECT_REP_WORDS = 15;

__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {       // set bits of `mask` below the calling lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ bool collect_listed(uint32_t verdict, uint32_t list_runner) {
    return verdict != MADSIM_PASS && (list_runner || !MADSIM_IS_RUNNER_VERDICT(verdict));
}

template <class Seeds>
__global__ __launch_bounds__(256) void collect_count_kernel(const madsim_result_t* __restrict__ out, uint64_t count, const Seeds seed_of,
                                                            uint64_t piece, uint32_t list_runner,
                                                            unsigned long long* __restrict__ rep, uint32_t* __restrict__ wave_cnt) {
    const uint32_t W = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint64_t lo = (uint64_t)W * piece, hi = lo + piece < count ? lo + piece : count;
    unsigned long long first = ~0ull, nfail = 0, steps = 0, clk = 0, gfirst = ~0ull, nrun = 0;
    uint32_t hist[8] = {0, 0, 0, 0, 0, 0, 0, 0}, listed = 0;                       // wave-uniform (popcounts of ballots); hist[0] stays 0
    for (uint64_t base = lo; base < hi; base += 64) {
        const uint64_t i = base + lane;
        uint32_t v = MADSIM_PASS;
        if (i < hi) {
            const uint4 r = reinterpret_cast<const uint4*>(out + i)[0];
            v = r.x;
            if (v != MADSIM_PASS) {
                const unsigned long long s = seed_of(i);
                nfail++; first = s < first ? s : first;
                if (MADSIM_IS_RUNNER_VERDICT(v)) nrun++; else gfirst = s < gfirst ? s : gfirst;
            }
            steps += r.y; clk += ((unsigned long long)r.w << 32) | r.z;
        }
        if (__ballot(v != MADSIM_PASS)) {                                          // (wave-uniform: rare-failure batches never get here)
#pragma unroll
            for (uint32_t k = 1; k < 7; k++) hist[k] += (uint32_t)__popcll(__ballot(v == k));
            hist[7] += (uint32_t)__popcll(__ballot(v >= 7));
            listed += (uint32_t)__popcll(__ballot(collect_listed(v, list_runner)));
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        unsigned long long f2 = __shfl_xor(first, o), g2 = __shfl_xor(gfirst, o);
        first = f2 < first ? f2 : first; gfirst = g2 < gfirst ? g2 : gfirst;
        nfail += __shfl_xor(nfail, o); steps += __shfl_xor(steps, o); clk += __shfl_xor(clk, o); nrun += __shfl_xor(nrun, o);
    }
    if (lane == 0) {                                                               // one set of atomics per wave, summary6's six when nothing fails
        wave_cnt[W] = listed;
        atomicMin(&rep[0], first); atomicAdd(&rep[1], nfail); atomicAdd(&rep[2], steps); atomicAdd(&rep[3], clk);
        atomicMin(&rep[4], gfirst); atomicAdd(&rep[5], nrun);
        if (nfail) {
#pragma unroll
            for (uint32_t k = 1; k < 8; k++) if (hist[k]) atomicAdd(&rep[6 + k], (unsigned long long)hist[k]);
            if (listed) atomicAdd(&rep[14], (unsigned long long)listed);
        }
    }
}

template <class Seeds>
__global__ __launch_bounds__(256) void collect_write_kernel(const madsim_result_t* __restrict__ out, uint64_t count, const Seeds seed_of,
                                                            uint64_t piece, uint32_t list_runner, unsigned long long* __restrict__ rep,
                                                            const uint32_t* __restrict__ wave_cnt, madsim_failure_t* __restrict__ recs,
                                                            uint64_t cap) {
    const uint32_t W = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (W == 0 && lane == 0) {                                                     // the PASS count is what the other seven leave
        unsigned long long other = 0;
        for (uint32_t k = 1; k < 8; k++) other += rep[6 + k];
        rep[6] = count - other;
    }
    if (cap == 0 || wave_cnt[W] == 0) return;                                      // (wave-uniform)
    uint64_t at = 0;                                                               // listed seeds of the waves before this one
    for (uint32_t j = lane; j < W; j += 64) at += wave_cnt[j];
    for (int o = 32; o > 0; o >>= 1) at += __shfl_xor(at, o);
    const uint64_t lo = (uint64_t)W * piece, hi = lo + piece < count ? lo + piece : count;
    for (uint64_t base = lo; base < hi && at < cap; base += 64) {
        const uint64_t i = base + lane;
        uint4 r = {MADSIM_PASS, 0, 0, 0};
        if (i < hi) r = reinterpret_cast<const uint4*>(out + i)[0];
        const bool mine = collect_listed(r.x, list_runner);
        const unsigned long long m = __ballot(mine);
        const uint64_t rank = at + lanes_below(m);
        if (mine && rank < cap) {                                                  // the other 32 bytes only of a seed that is listed
            const uint4 r1 = reinterpret_cast<const uint4*>(out + i)[1], r2 = reinterpret_cast<const uint4*>(out + i)[2];
            unsigned long long* p = reinterpret_cast<unsigned long long*>(recs + rank);          // 56 B records: 8-byte stores
            p[0] = seed_of(i);
            p[1] = ((unsigned long long)r.y << 32) | r.x;   p[2] = ((unsigned long long)r.w << 32) | r.z;
            p[3] = ((unsigned long long)r1.y << 32) | r1.x; p[4] = ((unsigned long long)r1.w << 32) | r1.z;
            p[5] = ((unsigned long long)r2.y << 32) | r2.x; p[6] = ((unsigned long long)r2.w << 32) | r2.z;
        }
        at += (uint64_t)__popcll(m);
    }
}

// ---- the statistics campaign form: count, min, max, 128-bit sum, a 252-bucket histogram and the K extreme seeds of four metrics ----
// Two kernels behind the batch's summary6 / collect kernels, over collect's cut of the batch (wave W owns a contiguous piece).
// stats_fold_kernel reads the first 32 of a seed's 48 bytes (verdict, steps, clock_ns, msg_count, rng_calls: two 16-byte loads) once.
// A seed is COUNTED when bit `verdict` of `include` is set (bits 0-3 only, so never a runner verdict).  Min, max and the two half-sums
// (sum of v & 0xffffffff, sum of v >> 32: exact below 2^32 seeds) fold in registers, per wave, then per workgroup through LDS: one set
// of atomics per workgroup.  The four histograms are LDS counters, flushed with one atomic per non-zero bucket.  Integer adds, min and
// max commute: the words do not depend on any order.
// The K extreme seeds of a metric are the K first counted seeds under the TOTAL order "value descending, seed ascending" — the key
// {value, ~index in the batch}, unique per seed — so they are a function of the batch alone, and no atomic decides a position: a wave
// keeps its K first in lanes 0 .. K-1 (topk_merge: K rounds of a wave-wide maximum over the list and the 64 new elements; a round of 64
// elements none of which beats the K-th is skipped, which is also what happens to every later element of a tie), wave m of a workgroup
// merges the four waves' lists of metric m into cand[m][workgroup][0..16), and stats_top_kernel (one workgroup per metric) merges the
// workgroups' lists the same way and writes {value, seed} in order.  Tied values cost what distinct ones cost.
// srep = {n, ~min[4], max[4], sum of low halves[4], sum of high halves[4]} (17 words, all zero before the launch: the minimum is kept
// inverted so that one memset prepares everything), then hist[4][256] as 32-bit counters, then top[4][16] {value, seed}.
constexpr uint32_t STAT_TOP = MADSIM_STAT_MAX_TOP, STAT_WGS = COLLECT_MAX_WAVES / 4;

struct TopKey { unsigned long long v; uint32_t k; };              // k = ~(index in the batch), 0 = no element (then v = 0: below every element)
__device__ __forceinline__ bool key_gt(const TopKey& a, const TopKey& b) { return a.v > b.v || (a.v == b.v && a.k > b.k); }

__device__ __forceinline__ uint32_t stat_bucket(unsigned long long v) {          // madsim_hip_stat_bucket
    if (v < 4) return (uint32_t)v;
    const uint32_t e = 63u - (uint32_t)__clzll((long long)v);
    return 4u * (e - 1u) + ((uint32_t)(v >> (e - 2u)) & 3u);
}

// list[m] (entry r in lane r, r < K <= 16, sorted; {0, 0} elsewhere) := the K first of list[m] and the wave's 64 nw[m].  Wave-uniform flow.
template <int M>
__device__ __forceinline__ void topk_merge(TopKey (&list)[M], TopKey (&nw)[M], uint32_t K, uint32_t lane) {
    TopKey res[M];
#pragma unroll
    for (int m = 0; m < M; m++) res[m] = TopKey{0, 0};
    for (uint32_t r = 0; r < K; r++) {
        TopKey mine[M], best[M];
        bool from_list[M];
#pragma unroll
        for (int m = 0; m < M; m++) { from_list[m] = key_gt(list[m], nw[m]); best[m] = mine[m] = from_list[m] ? list[m] : nw[m]; }
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int m = 0; m < M; m++) {
                const TopKey t = {__shfl_xor(best[m].v, o), __shfl_xor(best[m].k, o)};
                if (key_gt(t, best[m])) best[m] = t;
            }
        }
        uint32_t left = 0;
#pragma unroll
        for (int m = 0; m < M; m++) {                                             // keys are unique: exactly one lane holds the winner
            if (best[m].k != 0 && mine[m].k == best[m].k && mine[m].v == best[m].v) { if (from_list[m]) list[m] = TopKey{0, 0}; else nw[m] = TopKey{0, 0}; }
            if (lane == r) res[m] = best[m];
            left |= best[m].k;
        }
        if (!left) break;                                                          // (wave-uniform) nothing left in any metric
    }
#pragma unroll
    for (int m = 0; m < M; m++) list[m] = res[m];
}

// true (wave-uniform) when one of the wave's nw[m] comes before the K-th entry of list[m]: only then the list changes
template <int M>
__device__ __forceinline__ bool topk_enters(const TopKey (&list)[M], const TopKey (&nw)[M], uint32_t K) {
    bool any = false;
#pragma unroll
    for (int m = 0; m < M; m++) {
        const TopKey kth = {__shfl(list[m].v, (int)K - 1), __shfl(list[m].k, (int)K - 1)};
        any |= key_gt(nw[m], kth);
    }
    return __ballot(any) != 0;
}

__global__ __launch_bounds__(256) void stats_fold_kernel(const madsim_result_t* __restrict__ out, uint64_t count, uint64_t piece, uint32_t include,
                                                         uint32_t K, unsigned long long* __restrict__ srep, uint32_t* __restrict__ ghist,
                                                         unsigned long long* __restrict__ cand) {
    __shared__ uint32_t hist[MADSIM_STAT_METRICS][MADSIM_STAT_BUCKETS];
    __shared__ unsigned long long part[4][17];
    __shared__ unsigned long long lv[MADSIM_STAT_METRICS][4 * STAT_TOP];
    __shared__ uint32_t lk[MADSIM_STAT_METRICS][4 * STAT_TOP];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, W = blockIdx.x * 4 + wave;
    for (uint32_t i = threadIdx.x; i < MADSIM_STAT_METRICS * MADSIM_STAT_BUCKETS; i += 256) (&hist[0][0])[i] = 0;
    __syncthreads();
    const uint64_t lo = (uint64_t)W * piece, hi = lo + piece < count ? lo + piece : count;
    unsigned long long acc[17];                                                    // n, ~min[4], max[4], low halves[4], high halves[4]
#pragma unroll
    for (int j = 0; j < 17; j++) acc[j] = 0;
    TopKey list[MADSIM_STAT_METRICS];
#pragma unroll
    for (int m = 0; m < 4; m++) list[m] = TopKey{0, 0};
    for (uint64_t base = lo; base < hi; base += 64) {
        const uint64_t i = base + lane;
        TopKey nw[MADSIM_STAT_METRICS];
#pragma unroll
        for (int m = 0; m < 4; m++) nw[m] = TopKey{0, 0};
        if (i < hi) {
            const uint4 r0 = reinterpret_cast<const uint4*>(out + i)[0], r1 = reinterpret_cast<const uint4*>(out + i)[1];
            if (r0.x < 4u && ((include >> r0.x) & 1u)) {
                const unsigned long long v[4] = {((unsigned long long)r0.w << 32) | r0.z, r0.y, ((unsigned long long)r1.y << 32) | r1.x,
                                                 ((unsigned long long)r1.w << 32) | r1.z};
                acc[0]++;
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    acc[1 + m] = ~v[m] > acc[1 + m] ? ~v[m] : acc[1 + m];
                    acc[5 + m] = v[m] > acc[5 + m] ? v[m] : acc[5 + m];
                    acc[9 + m] += v[m] & 0xffffffffull; acc[13 + m] += v[m] >> 32;
                    atomicAdd(&hist[m][stat_bucket(v[m])], 1u);
                    nw[m] = TopKey{v[m], ~(uint32_t)i};                            // (a batch holds fewer than 2^32 - 1 seeds: never 0)
                }
            }
        }
        if (K && topk_enters<4>(list, nw, K)) topk_merge<4>(list, nw, K, lane);
    }
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int j = 0; j < 17; j++) {
            const unsigned long long t = __shfl_xor(acc[j], o);
            if (j >= 1 && j < 9) acc[j] = t > acc[j] ? t : acc[j]; else acc[j] += t;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 17; j++) part[wave][j] = acc[j];
    }
    if (K && lane < STAT_TOP) {
#pragma unroll
        for (int m = 0; m < 4; m++) { lv[m][wave * STAT_TOP + lane] = list[m].v; lk[m][wave * STAT_TOP + lane] = list[m].k; }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 4; m++) {                                                  // thread t: bucket t of every metric
        const uint32_t c = hist[m][threadIdx.x];
        if (c) atomicAdd(&ghist[m * MADSIM_STAT_BUCKETS + threadIdx.x], c);
    }
    if (threadIdx.x < 17 && part[0][0] + part[1][0] + part[2][0] + part[3][0] != 0) {        // one set of atomics per workgroup that counted a seed
        const uint32_t j = threadIdx.x;
        unsigned long long a = part[0][j];
        for (int w = 1; w < 4; w++) { const unsigned long long t = part[w][j]; if (j >= 1 && j < 9) a = t > a ? t : a; else a += t; }
        if (j >= 1 && j < 9) atomicMax(&srep[j], a); else atomicAdd(&srep[j], a);
    }
    if (K) {                                                                       // wave m: the workgroup's list of metric m
        TopKey l1[1] = {TopKey{0, 0}}, n1[1] = {TopKey{lv[wave][lane], lk[wave][lane]}};
        topk_merge<1>(l1, n1, K, lane);
        if (lane < STAT_TOP) {
            unsigned long long* p = cand + ((uint64_t)(wave * STAT_WGS + blockIdx.x) * STAT_TOP + lane) * 2;
            p[0] = l1[0].v; p[1] = l1[0].k ? (unsigned long long)(uint32_t)~l1[0].k : ~0ull;
        }
    }
}

// grid = MADSIM_STAT_METRICS workgroups: workgroup m merges cand[m][0 .. n_wg)[0 .. 16) ({value, index in the batch or ~0}), a quarter per
// wave, then wave 0 the four lists; top[m][r] = {value, seed}, r < min(K, counted seeds of the batch).
template <class Seeds>
__global__ __launch_bounds__(256) void stats_top_kernel(const unsigned long long* __restrict__ cand, uint32_t n_wg, uint32_t K, const Seeds seed_of,
                                                        unsigned long long* __restrict__ top) {
    __shared__ unsigned long long lv[4 * STAT_TOP];
    __shared__ uint32_t lk[4 * STAT_TOP];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = blockIdx.x;
    const uint32_t total = n_wg * STAT_TOP, quarter = (total / 4 + 63) / 64 * 64;      // (total is a multiple of 16, at most 4 096)
    const uint32_t lo = wave * quarter, hi = lo + quarter < total ? lo + quarter : total;
    const unsigned long long* src = cand + (uint64_t)m * STAT_WGS * STAT_TOP * 2;
    TopKey list[1] = {TopKey{0, 0}};
    for (uint32_t base = lo; base < hi; base += 64) {
        const uint32_t j = base + lane;
        TopKey nw[1] = {TopKey{0, 0}};
        if (j < hi) {
            const unsigned long long v = src[2 * j], x = src[2 * j + 1];
            if (x != ~0ull) nw[0] = TopKey{v, ~(uint32_t)x};
        }
        if (topk_enters<1>(list, nw, K)) topk_merge<1>(list, nw, K, lane);
    }
    if (lane < STAT_TOP) { lv[wave * STAT_TOP + lane] = list[0].v; lk[wave * STAT_TOP + lane] = list[0].k; }
    __syncthreads();
    if (wave == 0) {
        TopKey l1[1] = {TopKey{0, 0}}, n1[1] = {TopKey{lv[lane], lk[lane]}};
        topk_merge<1>(l1, n1, K, lane);
        if (lane < K && l1[0].k) {
            unsigned long long* p = top + (uint64_t)(m * STAT_TOP + lane) * 2;
            p[0] = l1[0].v; p[1] = seed_of((uint32_t)~l1[0].k);
        }
    }
}

// ---- the grouping campaign form: the distinct signatures (verdict, key) of the batch's counted seeds, each with its count and its smallest seed ----
// Two kernels behind the batch's other report kernels, over collect's cut of the batch.  A seed is COUNTED as in stats_fold_kernel (bit
// `verdict` of `include`, bits 0-3 only); its key is one 8-byte word of its result (key_word 1 .. 5; 0 = steps, which the verdict word holds
// already): 16 + 8 bytes are read per counted seed, 16 per other seed.
// The table in global memory has `mask + 1` slots (a power of two, >= 2 x the batch: load <= 0.5) of {tag, count, ~smallest index, 0}, all
// zero between launches.  A slot's TAG is 1 + the batch index of the seed that claimed it, and the slot's signature is THAT SEED's, read from
// the result array — which nobody writes while these kernels run.  So a slot is complete the moment its tag is set: every 64-bit value is a
// legal key, one 32-bit compare-and-swap claims, and nobody ever waits for a "ready" word.  count and the smallest index (kept inverted, so
// that zero is neutral) follow by atomicAdd / atomicMax.  Linear probing from group_slot(), wrapping, bounded by the slot count; a probe
// that runs out, or a tag no seed of the batch can have written, sets the error word (grep[1]) instead of reading out of bounds.
// Equal signatures are combined inside the wave first: a wave-uniform loop takes the first remaining counted lane, ballots the lanes
// that share its signature and leaves that lane the popcount; then the leaders — one per distinct signature of the round, all at once —
// insert.  Lanes hold ascending seeds, so a leader's index is its signature's smallest of the round.  "600 deadlocks, all one signature" is
// one add and one max per wave that holds any; a round without a counted seed (wave-uniform) touches nothing.
// Every successful claim appends its slot to `list` (position: one atomicAdd on grep[0], the batch's number of groups).
// group_extract_kernel walks the list: entry j = {key, verdict, count, seed0 + smallest index} of slot list[j], and the slot is zeroed
// again — work proportional to the groups, never to the table.  Arrival order places the entries; the host sorts them (madsim_k_fold_groups).
constexpr uint32_t GROUP_ERR_PROBE = 1, GROUP_ERR_TAG = 2, GROUP_ERR_LIST = 4;

__device__ __forceinline__ unsigned long long group_key(const madsim_result_t* __restrict__ r, uint32_t key_word) {
    return key_word ? reinterpret_cast<const unsigned long long*>(r)[key_word] : (unsigned long long)reinterpret_cast<const uint32_t*>(r)[1];
}

// the calling lane's `cnt` seeds of signature (v, key), the smallest of them batch index i
__device__ __forceinline__ void group_insert(const madsim_result_t* __restrict__ out, uint32_t count, uint32_t key_word, uint4* __restrict__ table,
                                             uint32_t mask, uint32_t* __restrict__ list, unsigned long long* __restrict__ grep,
                                             unsigned long long key, uint32_t v, uint32_t cnt, uint32_t i) {
    uint32_t s = (uint32_t)group_slot(key, v, (uint64_t)mask + 1u);
    for (uint32_t probe = 0; probe <= mask; probe++, s = (s + 1u) & mask) {
        uint32_t* const slot = reinterpret_cast<uint32_t*>(table + s);
        uint32_t tag = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (a tag only ever goes from 0 to its value)
        if (tag == 0) {
            tag = atomicCAS(slot, 0u, i + 1u);
            if (tag == 0) {                                                        // claimed: the slot's signature is this seed's
                const unsigned long long pos = atomicAdd(&grep[0], 1ull);
                if (pos < count) list[pos] = s; else atomicOr(&grep[1], (unsigned long long)GROUP_ERR_LIST);
                tag = i + 1u;
            }
        }
        bool match = tag == i + 1u;
        if (!match) {
            const uint32_t rep = tag - 1u;
            if (rep >= count) { atomicOr(&grep[1], (unsigned long long)GROUP_ERR_TAG); return; }       // (a table that was not clean)
            match = reinterpret_cast<const uint32_t*>(out + rep)[0] == v && group_key(out + rep, key_word) == key;
        }
        if (match) { atomicAdd(slot + 1, cnt); atomicMax(slot + 2, ~i); return; }
    }
    atomicOr(&grep[1], (unsigned long long)GROUP_ERR_PROBE);                       // (cannot happen at load <= 0.5)
}

__global__ __launch_bounds__(256) void group_fold_kernel(const madsim_result_t* __restrict__ out, uint32_t count, uint32_t piece, uint32_t include,
                                                         uint32_t key_word, uint4* __restrict__ table, uint32_t mask, uint32_t* __restrict__ list,
                                                         unsigned long long* __restrict__ grep) {
    const uint32_t W = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint64_t lo = (uint64_t)W * piece, hi = lo + piece < count ? lo + piece : count;
    for (uint64_t base = lo; base < hi; base += 64) {
        const uint64_t i = base + lane;
        uint32_t v = ~0u, steps = 0;
        if (i < hi) { const uint4 r = reinterpret_cast<const uint4*>(out + i)[0]; v = r.x; steps = r.y; }
        const bool counted = v < 4u && ((include >> v) & 1u);
        unsigned long long m = __ballot(counted);
        if (!m) continue;                                                          // (wave-uniform: a batch with nothing counted ends here)
        unsigned long long key = 0;
        if (counted) key = key_word ? reinterpret_cast<const unsigned long long*>(out + i)[key_word] : (unsigned long long)steps;
        uint32_t cnt = 0;                                                          // non-zero in the leaders
        while (m) {                                                                // (wave-uniform) one trip per distinct signature of the round
            const int l = __ffsll((long long)m) - 1;
            const unsigned long long lk = __shfl(key, l);
            const uint32_t lv = __shfl(v, l);
            const unsigned long long sm = __ballot(counted && key == lk && v == lv);      // a subset of m: lane l's signature is none of the earlier leaders'
            if ((int)lane == l) cnt = (uint32_t)__popcll(sm);
            m &= ~sm;
        }
        if (cnt) group_insert(out, count, key_word, table, mask, list, grep, key, v, cnt, (uint32_t)i);
    }
}

template <class Seeds>
__global__ __launch_bounds__(256) void group_extract_kernel(const madsim_result_t* __restrict__ out, uint32_t count, const Seeds seed_of, uint32_t key_word,
                                                            uint4* __restrict__ table, uint32_t mask, const uint32_t* __restrict__ list,
                                                            unsigned long long* __restrict__ grep, madsim_group_t* __restrict__ entries) {
    const unsigned long long claimed = grep[0];                                    // (nobody adds to it in this kernel)
    const uint32_t n = claimed < count ? (uint32_t)claimed : count;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < n; j += gridDim.x * 256u) {
        const uint32_t s = list[j] & mask;
        const uint4 e = table[s];
        table[s] = uint4{0, 0, 0, 0};
        const uint32_t rep = e.x - 1u, first = ~e.z;
        unsigned long long* const p = reinterpret_cast<unsigned long long*>(entries + j);
        if (e.x == 0 || rep >= count || first >= count) {                          // (a table that was not clean)
            atomicOr(&grep[1], (unsigned long long)GROUP_ERR_TAG);
            p[0] = p[1] = p[2] = p[3] = 0;
            continue;
        }
        p[0] = group_key(out + rep, key_word);
        p[1] = reinterpret_cast<const uint32_t*>(out + rep)[0];                    // verdict, reserved = 0
        p[2] = e.y;
        p[3] = seed_of(first);
    }
}

// ---- the differential campaign form: two result arrays of the same seeds, compared field by field ----
// Two kernels behind the two sides' simulation and summary6 launches, over collect's cut of the batch (wave W owns a contiguous piece, so
// "ascending wave, ascending lane" is ascending seed order).  A seed is COMPARED when neither verdict is a runner verdict; its difference
// mask has bit k set when field k (verdict, steps, clock_ns, msg_count, rng_calls, trace_hash, obs_hash) is named in `fields` and differs.
// An incomparable seed has mask 0 whatever its bytes.  The first 16 bytes of each side are always read (the verdict is there); the second
// 16 (msg_count, rng_calls) and the third (the two hashes) only when `fields` names one of theirs — a kernel argument, so wave-uniform.
// words = {n_differ, n_incomparable, n_by_field[8], transitions[8][8]}, all zero before the launch.  The PASS -> PASS cell is not counted:
// diff_write_kernel sets it to what the other 63 leave, so a round of 64 seeds that all passed on both sides with no masked difference
// ends at one ballot.  Any other round adds its cells to 64 LDS counters of the workgroup (one global atomic per non-zero cell per
// workgroup) and its ballots' popcounts to the wave's registers (one set of global atomics per wave).
// diff_write_kernel is collect_write_kernel with two sources: the exclusive prefix of wave_cnt is a wave's offset, only a wave with
// differing seeds and an offset below `cap` reads its piece again, rank = offset + lanes_below(ballot): integer adds only, no atomic
// decides a position.  A record is {seed, a, b}: 104 bytes, thirteen 8-byte stores.
struct DiffLoads { bool b1, b2; };                                                 // which of the later 16-byte parts `fields` touches
__device__ __forceinline__ DiffLoads diff_loads(uint32_t fields) {
    return DiffLoads{(fields & (MADSIM_DIFF_MSGS | MADSIM_DIFF_RNG)) != 0, (fields & (MADSIM_DIFF_TRACE | MADSIM_DIFF_OBS)) != 0};
}
__device__ __forceinline__ uint32_t diff_cell(uint32_t va, uint32_t vb) { return (va < 7u ? va : 7u) * 8u + (vb < 7u ? vb : 7u); }

// the difference mask of seed i (0 for an incomparable seed); va / vb: the two verdicts
__device__ __forceinline__ uint32_t diff_mask(const madsim_result_t* __restrict__ a, const madsim_result_t* __restrict__ b, uint64_t i, uint32_t fields,
                                              DiffLoads L, uint32_t& va, uint32_t& vb) {
    const uint4 a0 = reinterpret_cast<const uint4*>(a + i)[0], b0 = reinterpret_cast<const uint4*>(b + i)[0];
    va = a0.x; vb = b0.x;
    uint32_t d = (a0.x != b0.x ? MADSIM_DIFF_VERDICT : 0u) | (a0.y != b0.y ? MADSIM_DIFF_STEPS : 0u) | ((a0.z != b0.z || a0.w != b0.w) ? MADSIM_DIFF_CLOCK : 0u);
    if (L.b1) {
        const uint4 a1 = reinterpret_cast<const uint4*>(a + i)[1], b1 = reinterpret_cast<const uint4*>(b + i)[1];
        d |= ((a1.x != b1.x || a1.y != b1.y) ? MADSIM_DIFF_MSGS : 0u) | ((a1.z != b1.z || a1.w != b1.w) ? MADSIM_DIFF_RNG : 0u);
    }
    if (L.b2) {
        const uint4 a2 = reinterpret_cast<const uint4*>(a + i)[2], b2 = reinterpret_cast<const uint4*>(b + i)[2];
        d |= ((a2.x != b2.x || a2.y != b2.y) ? MADSIM_DIFF_TRACE : 0u) | ((a2.z != b2.z || a2.w != b2.w) ? MADSIM_DIFF_OBS : 0u);
    }
    return (MADSIM_IS_RUNNER_VERDICT(va) || MADSIM_IS_RUNNER_VERDICT(vb)) ? 0u : d & fields;
}

__global__ __launch_bounds__(256) void diff_count_kernel(const madsim_result_t* __restrict__ a, const madsim_result_t* __restrict__ b, uint64_t count,
                                                         uint64_t piece, uint32_t fields, unsigned long long* __restrict__ words,
                                                         uint32_t* __restrict__ wave_cnt) {
    __shared__ uint32_t cells[64];
    const uint32_t W = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (threadIdx.x < 64) cells[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t lo = (uint64_t)W * piece, hi = lo + piece < count ? lo + piece : count;
    const DiffLoads L = diff_loads(fields);
    uint32_t n_differ = 0, n_inc = 0, by_field[MADSIM_DIFF_FIELDS] = {0, 0, 0, 0, 0, 0, 0};      // wave-uniform (popcounts of ballots)
    for (uint64_t base = lo; base < hi; base += 64) {
        const uint64_t i = base + lane;
        uint32_t va = MADSIM_PASS, vb = MADSIM_PASS, d = 0;
        if (i < hi) d = diff_mask(a, b, i, fields, L, va, vb);
        if (!__ballot((va | vb | d) != 0)) continue;                               // (wave-uniform) all PASS -> PASS, nothing differs
        const uint32_t cell = diff_cell(va, vb);
        if (cell) atomicAdd(&cells[cell], 1u);
        n_differ += (uint32_t)__popcll(__ballot(d != 0));
        n_inc += (uint32_t)__popcll(__ballot(MADSIM_IS_RUNNER_VERDICT(va) || MADSIM_IS_RUNNER_VERDICT(vb)));
#pragma unroll
        for (uint32_t k = 0; k < MADSIM_DIFF_FIELDS; k++) by_field[k] += (uint32_t)__popcll(__ballot((d >> k) & 1u));
    }
    if (lane == 0) {                                                               // one set of atomics per wave: none when nothing differs
        wave_cnt[W] = n_differ;
        if (n_differ) atomicAdd(&words[0], (unsigned long long)n_differ);
        if (n_inc) atomicAdd(&words[1], (unsigned long long)n_inc);
#pragma unroll
        for (uint32_t k = 0; k < MADSIM_DIFF_FIELDS; k++) if (by_field[k]) atomicAdd(&words[2 + k], (unsigned long long)by_field[k]);
    }
    __syncthreads();
    if (threadIdx.x > 0 && threadIdx.x < 64 && cells[threadIdx.x]) atomicAdd(&words[10 + threadIdx.x], (unsigned long long)cells[threadIdx.x]);
}

template <class Seeds>
__global__ __launch_bounds__(256) void diff_write_kernel(const madsim_result_t* __restrict__ a, const madsim_result_t* __restrict__ b, uint64_t count,
                                                         const Seeds seed_of, uint64_t piece, uint32_t fields, unsigned long long* __restrict__ words,
                                                         const uint32_t* __restrict__ wave_cnt, madsim_diff_record_t* __restrict__ recs, uint64_t cap) {
    const uint32_t W = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (W == 0 && lane == 0) {                                                     // PASS -> PASS is what the other 63 cells leave
        unsigned long long other = 0;
        for (uint32_t k = 1; k < 64; k++) other += words[10 + k];
        words[10] = count - other;
    }
    if (cap == 0 || wave_cnt[W] == 0) return;                                      // (wave-uniform)
    uint64_t at = 0;                                                               // differing seeds of the waves before this one
    for (uint32_t j = lane; j < W; j += 64) at += wave_cnt[j];
    for (int o = 32; o > 0; o >>= 1) at += __shfl_xor(at, o);
    const uint64_t lo = (uint64_t)W * piece, hi = lo + piece < count ? lo + piece : count;
    const DiffLoads L = diff_loads(fields);
    for (uint64_t base = lo; base < hi && at < cap; base += 64) {
        const uint64_t i = base + lane;
        uint32_t va = MADSIM_PASS, vb = MADSIM_PASS, d = 0;
        if (i < hi) d = diff_mask(a, b, i, fields, L, va, vb);
        const unsigned long long m = __ballot(d != 0);
        const uint64_t rank = at + lanes_below(m);
        if (d != 0 && rank < cap) {                                                // all 96 bytes only of a seed that is listed
            const uint4* qa = reinterpret_cast<const uint4*>(a + i);
            const uint4* qb = reinterpret_cast<const uint4*>(b + i);
            unsigned long long* p = reinterpret_cast<unsigned long long*>(recs) + rank * 13u;      // 104 B records: 8-byte stores
            p[0] = seed_of(i);
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const uint4 x = qa[j], y = qb[j];
                p[1 + 2 * j] = ((unsigned long long)x.y << 32) | x.x; p[2 + 2 * j] = ((unsigned long long)x.w << 32) | x.z;
                p[7 + 2 * j] = ((unsigned long long)y.y << 32) | y.x; p[8 + 2 * j] = ((unsigned long long)y.w << 32) | y.z;
            }
        }
        at += (uint64_t)__popcll(m);
    }
}

// ---- the sweep campaign form: up to eight result arrays of the same seeds, classified across all of them ----
// Two kernels behind the variants' simulation and summary6 launches, over collect's cut of the batch.  Variant v of a seed is PASS
// (verdict 0), FAIL (1 .. 3) or RUNNER; fail / runner: the masks of the variants that are; a seed is SETTLED when runner == 0, and only
// then has a differ mask: bit v (v >= 1) set when a field named in `fields` differs between variant v and variant 0 (diff_mask's
// comparison).  The V array pointers travel by value in SweepSides; every loop over variants is unrolled to 8 with a wave-uniform v < V
// guard, so the table is indexed by constants only and stays in scalar registers.  All V 16-byte heads of a round are loaded before the
// first compare (V independent requests per lane); the second and third 16 bytes only when `fields` names one of theirs.
// words = {n_selected, n_incomparable, n_runner_by_variant[8], n_differ_from_first[8], n_by_mask[256]}, all zero before the launch.
// Cell n_by_mask[0] is not counted: sweep_write_kernel sets it to count - n_incomparable - the other 255, so a round of 64 seeds that
// passed in every variant with no masked difference ends at one ballot.  Any other round adds its settled seeds' cells to 256 LDS
// counters of the workgroup (one global atomic per non-zero cell per workgroup) and its ballots' popcounts to the wave's registers
// (one set of global atomics per wave, none when zero).  wave_cnt[W] = the wave's number of SELECTED seeds (the list rule's).
// sweep_write_kernel is diff_write_kernel with V sources: only a wave with selected seeds and an offset below `cap` reads its piece
// again, rank = offset + lanes_below(ballot).  A record is {seed, fail | differ << 32, the eight verdict bytes}: three 8-byte stores.
struct SweepSides { const madsim_result_t* r[MADSIM_SWEEP_MAX_VARIANTS]; };
struct SweepSeed { uint32_t fail, runner, differ; unsigned long long verdicts; };

// seed i of the batch across the V variants (live: i is inside the wave's piece; a dead lane is PASS everywhere, nothing differing)
__device__ __forceinline__ SweepSeed sweep_classify(const SweepSides& S, uint32_t V, uint64_t i, bool live, uint32_t fields, DiffLoads L) {
    uint4 h[MADSIM_SWEEP_MAX_VARIANTS];
#pragma unroll
    for (uint32_t v = 0; v < MADSIM_SWEEP_MAX_VARIANTS; v++) {
        h[v] = uint4{0, 0, 0, 0};
        if (v < V && live) h[v] = reinterpret_cast<const uint4*>(S.r[v] + i)[0];
    }
    SweepSeed s{0, 0, 0, 0};
#pragma unroll
    for (uint32_t v = 0; v < MADSIM_SWEEP_MAX_VARIANTS; v++) {
        if (v >= V) continue;
        const uint32_t x = h[v].x;
        s.fail |= (x - 1u < 3u ? 1u : 0u) << v;
        s.runner |= (MADSIM_IS_RUNNER_VERDICT(x) ? 1u : 0u) << v;
        s.verdicts |= (unsigned long long)(x & 0xffu) << (8u * v);
        if (v == 0) continue;
        const uint32_t d = (x != h[0].x ? MADSIM_DIFF_VERDICT : 0u) | (h[v].y != h[0].y ? MADSIM_DIFF_STEPS : 0u) |
                           ((h[v].z != h[0].z || h[v].w != h[0].w) ? MADSIM_DIFF_CLOCK : 0u);
        s.differ |= ((d & fields) ? 1u : 0u) << v;
    }
    if (L.b1 && live) {                                                            // (L: wave-uniform)
        uint4 p[MADSIM_SWEEP_MAX_VARIANTS];
#pragma unroll
        for (uint32_t v = 0; v < MADSIM_SWEEP_MAX_VARIANTS; v++) if (v < V) p[v] = reinterpret_cast<const uint4*>(S.r[v] + i)[1];
#pragma unroll
        for (uint32_t v = 1; v < MADSIM_SWEEP_MAX_VARIANTS; v++) {
            if (v >= V) continue;
            const uint32_t d = ((p[v].x != p[0].x || p[v].y != p[0].y) ? MADSIM_DIFF_MSGS : 0u) | ((p[v].z != p[0].z || p[v].w != p[0].w) ? MADSIM_DIFF_RNG : 0u);
            s.differ |= ((d & fields) ? 1u : 0u) << v;
        }
    }
    if (L.b2 && live) {
        uint4 p[MADSIM_SWEEP_MAX_VARIANTS];
#pragma unroll
        for (uint32_t v = 0; v < MADSIM_SWEEP_MAX_VARIANTS; v++) if (v < V) p[v] = reinterpret_cast<const uint4*>(S.r[v] + i)[2];
#pragma unroll
        for (uint32_t v = 1; v < MADSIM_SWEEP_MAX_VARIANTS; v++) {
            if (v >= V) continue;
            const uint32_t d = ((p[v].x != p[0].x || p[v].y != p[0].y) ? MADSIM_DIFF_TRACE : 0u) | ((p[v].z != p[0].z || p[v].w != p[0].w) ? MADSIM_DIFF_OBS : 0u);
            s.differ |= ((d & fields) ? 1u : 0u) << v;
        }
    }
    if (s.runner) s.differ = 0;                                                    // an incomparable seed differs nowhere
    return s;
}
// the list rule; full = the fail mask of a seed that fails in every variant
__device__ __forceinline__ bool sweep_selected(const SweepSeed& s, uint32_t rule, uint32_t full) {
    if (s.runner) return false;
    return rule == MADSIM_SWEEP_LIST_DIFFERING ? s.differ != 0 : rule == MADSIM_SWEEP_LIST_FAILING ? s.fail != 0 : (s.fail != 0 && s.fail != full);
}

__global__ __launch_bounds__(256) void sweep_count_kernel(const SweepSides S, uint32_t V, uint64_t count, uint64_t piece, uint32_t fields, uint32_t rule,
                                                          unsigned long long* __restrict__ words, uint32_t* __restrict__ wave_cnt) {
    __shared__ uint32_t cells[256];
    const uint32_t W = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    cells[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t lo = (uint64_t)W * piece, hi = lo + piece < count ? lo + piece : count;
    const DiffLoads L = diff_loads(fields);
    const uint32_t full = (1u << V) - 1u;
    uint32_t n_sel = 0, n_inc = 0, by_runner[MADSIM_SWEEP_MAX_VARIANTS] = {0, 0, 0, 0, 0, 0, 0, 0}, by_differ[MADSIM_SWEEP_MAX_VARIANTS] = {0, 0, 0, 0, 0, 0, 0, 0};      // wave-uniform
    for (uint64_t base = lo; base < hi; base += 64) {
        const uint64_t i = base + lane;
        const SweepSeed s = sweep_classify(S, V, i, i < hi, fields, L);
        if (!__ballot((s.fail | s.runner | s.differ) != 0)) continue;              // (wave-uniform) every variant passed, nothing masked differs
        if (!s.runner && s.fail) atomicAdd(&cells[s.fail], 1u);
        n_sel += (uint32_t)__popcll(__ballot(sweep_selected(s, rule, full)));
        const unsigned long long inc = __ballot(s.runner != 0);
        if (inc) {                                                                 // (wave-uniform)
            n_inc += (uint32_t)__popcll(inc);
#pragma unroll
            for (uint32_t v = 0; v < MADSIM_SWEEP_MAX_VARIANTS; v++) by_runner[v] += (uint32_t)__popcll(__ballot((s.runner >> v) & 1u));
        }
        if (__ballot(s.differ != 0)) {
#pragma unroll
            for (uint32_t v = 1; v < MADSIM_SWEEP_MAX_VARIANTS; v++) by_differ[v] += (uint32_t)__popcll(__ballot((s.differ >> v) & 1u));
        }
    }
    if (lane == 0) {                                                               // one set of atomics per wave: none when zero
        wave_cnt[W] = n_sel;
        if (n_sel) atomicAdd(&words[0], (unsigned long long)n_sel);
        if (n_inc) atomicAdd(&words[1], (unsigned long long)n_inc);
#pragma unroll
        for (uint32_t v = 0; v < MADSIM_SWEEP_MAX_VARIANTS; v++) {
            if (by_runner[v]) atomicAdd(&words[2 + v], (unsigned long long)by_runner[v]);
            if (by_differ[v]) atomicAdd(&words[10 + v], (unsigned long long)by_differ[v]);
        }
    }
    __syncthreads();
    if (threadIdx.x > 0 && cells[threadIdx.x]) atomicAdd(&words[18 + threadIdx.x], (unsigned long long)cells[threadIdx.x]);
}

template <class Seeds>
__global__ __launch_bounds__(256) void sweep_write_kernel(const SweepSides S, uint32_t V, uint64_t count, const Seeds seed_of, uint64_t piece, uint32_t fields,
                                                          uint32_t rule, unsigned long long* __restrict__ words, const uint32_t* __restrict__ wave_cnt,
                                                          madsim_sweep_record_t* __restrict__ recs, uint64_t cap) {
    const uint32_t W = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (W == 0) {                                                                  // mask 0 is what the incomparable seeds and the other 255 cells leave
        unsigned long long other = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) if (lane + 64u * k) other += words[18 + lane + 64u * k];
        for (int o = 32; o > 0; o >>= 1) other += __shfl_xor(other, o);
        if (lane == 0) words[18] = count - words[1] - other;
    }
    if (cap == 0 || wave_cnt[W] == 0) return;                                      // (wave-uniform)
    uint64_t at = 0;                                                               // selected seeds of the waves before this one
    for (uint32_t j = lane; j < W; j += 64) at += wave_cnt[j];
    for (int o = 32; o > 0; o >>= 1) at += __shfl_xor(at, o);
    const uint64_t lo = (uint64_t)W * piece, hi = lo + piece < count ? lo + piece : count;
    const DiffLoads L = diff_loads(fields);
    const uint32_t full = (1u << V) - 1u;
    for (uint64_t base = lo; base < hi && at < cap; base += 64) {
        const uint64_t i = base + lane;
        const SweepSeed s = sweep_classify(S, V, i, i < hi, fields, L);
        const bool mine = sweep_selected(s, rule, full);
        const unsigned long long m = __ballot(mine);
        const uint64_t rank = at + lanes_below(m);
        if (mine && rank < cap) {                                                  // a list entry only of a seed that is listed
            unsigned long long* p = reinterpret_cast<unsigned long long*>(recs) + rank * 3u;      // 24 B records: 8-byte stores
            p[0] = seed_of(i);
            p[1] = (unsigned long long)s.fail | (unsigned long long)s.differ << 32;
            p[2] = s.verdicts;
        }
        at += (uint64_t)__popcll(m);
    }
}

// ---- the paired campaign form: per-seed metric deltas between two result arrays of the same seeds ----
// Two kernels behind the two sides' simulation and summary6 launches (and the diff kernels, when asked for), over collect's cut of the batch
// (wave W owns a contiguous piece).  A seed is INCOMPARABLE when either verdict is a runner verdict (diff's rule), PAIRED when both verdicts
// are below 4 with bit `verdict A` set in include_a and bit `verdict B` in include_b, and unpaired otherwise (the host: count - the two).
// paired_fold_kernel reads the 16-byte head of both sides of every seed and the second 16 bytes of a paired one (the 32 bytes
// stats_fold_kernel decodes).  Per paired seed and metric m the two values compare as unsigned 64-bit numbers: b > a is UP with magnitude
// b - a, a > b is DOWN with magnitude a - b — never 0 and always 64 bits —, a == b is neither (the host: n_paired - n_up - n_down).  SET
// j = 2 m + direction holds what madsim_metric_t holds of the magnitudes: count (popcounts of ballots: wave-uniform), minimum (kept inverted:
// zero is neutral), maximum and the two half-sums, folded in registers, per wave, then per workgroup through LDS — one set of atomics per
// workgroup that paired a seed —, and a histogram of 256 LDS counters per set (8 KB), flushed with one atomic per non-zero bucket.  The
// half-sums of a and of b over the paired seeds ride along.  A round of 64 seeds none of which is paired ends at two ballots.
// The K extreme seeds of a set are the K first under "magnitude descending, seed ascending": stats_fold_kernel's scheme with the key
// {magnitude, ~index in the batch}, as ONE instantiation of eight lists (topk_merge<8>: the kernel takes 250 of the 512 VGPRs a wave of a
// 256-thread workgroup may have and has no private segment, so a second pass over the batch with two M = 4 instantiations would buy
// nothing; the counts are in profiles/paired_ab.md).  Wave w of a workgroup merges the
// four waves' lists of sets w and w + 4 into cand[set][workgroup][0..16); paired_top_kernel (one workgroup per set) merges the workgroups'
// lists and, for each winner, loads that metric of both sides at the winner's index and writes {seed, a, b}.
// words = {n_paired, n_incomparable, n[8], ~min[8], max[8], low half-sums of the magnitudes[8], high[8], low half-sums of a[4], high[4], of
// b[4], high[4]} (58 words), then hist[8][256] as 32-bit counters, then top[8][16] {seed, a, b}; all zero before the launch.
constexpr uint32_t PAIRED_SETS = 2 * MADSIM_STAT_METRICS, PAIRED_HEAD = 58;

// metric m (MADSIM_STAT_*) of a result: steps is the 32-bit word 1, clock_ns / msg_count / rng_calls the 64-bit words 1 / 2 / 3
__device__ __forceinline__ unsigned long long paired_metric(const madsim_result_t* __restrict__ r, uint32_t m) {
    if (m == MADSIM_STAT_STEPS) return reinterpret_cast<const uint32_t*>(r)[1];
    return reinterpret_cast<const unsigned long long*>(r)[m == MADSIM_STAT_CLOCK ? 1 : m];
}

__global__ __launch_bounds__(256) void paired_fold_kernel(const madsim_result_t* __restrict__ ra, const madsim_result_t* __restrict__ rb, uint64_t count,
                                                          uint64_t piece, uint32_t include_a, uint32_t include_b, uint32_t K,
                                                          unsigned long long* __restrict__ words, uint32_t* __restrict__ ghist,
                                                          unsigned long long* __restrict__ cand) {
    __shared__ uint32_t hist[PAIRED_SETS][MADSIM_STAT_BUCKETS];
    __shared__ unsigned long long part[4][PAIRED_HEAD];
    __shared__ unsigned long long lv[PAIRED_SETS][4 * STAT_TOP];
    __shared__ uint32_t lk[PAIRED_SETS][4 * STAT_TOP];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, W = blockIdx.x * 4 + wave;
    for (uint32_t i = threadIdx.x; i < PAIRED_SETS * MADSIM_STAT_BUCKETS; i += 256) (&hist[0][0])[i] = 0;
    __syncthreads();
    const uint64_t lo = (uint64_t)W * piece, hi = lo + piece < count ? lo + piece : count;
    uint32_t n_pair = 0, n_inc = 0, n_dir[PAIRED_SETS] = {0, 0, 0, 0, 0, 0, 0, 0};       // wave-uniform (popcounts of ballots)
    unsigned long long acc[PAIRED_HEAD - 10];                                      // ~min[8], max[8], low[8], high[8], a low / high[4], b low / high[4]
#pragma unroll
    for (int j = 0; j < (int)PAIRED_HEAD - 10; j++) acc[j] = 0;
    TopKey list[PAIRED_SETS];
#pragma unroll
    for (int j = 0; j < (int)PAIRED_SETS; j++) list[j] = TopKey{0, 0};
    for (uint64_t base = lo; base < hi; base += 64) {
        const uint64_t i = base + lane;
        uint4 a0 = {MADSIM_PASS, 0, 0, 0}, b0 = a0;
        bool paired = false, inc = false;
        if (i < hi) {
            a0 = reinterpret_cast<const uint4*>(ra + i)[0]; b0 = reinterpret_cast<const uint4*>(rb + i)[0];
            inc = MADSIM_IS_RUNNER_VERDICT(a0.x) || MADSIM_IS_RUNNER_VERDICT(b0.x);
            paired = a0.x < 4u && b0.x < 4u && ((include_a >> a0.x) & 1u) && ((include_b >> b0.x) & 1u);
        }
        n_inc += (uint32_t)__popcll(__ballot(inc));
        const unsigned long long pm = __ballot(paired);
        if (!pm) continue;                                                         // (wave-uniform) nothing paired in this round
        n_pair += (uint32_t)__popcll(pm);
        TopKey nw[PAIRED_SETS];
#pragma unroll
        for (int j = 0; j < (int)PAIRED_SETS; j++) nw[j] = TopKey{0, 0};
        if (paired) {
            const uint4 a1 = reinterpret_cast<const uint4*>(ra + i)[1], b1 = reinterpret_cast<const uint4*>(rb + i)[1];
            const unsigned long long va[4] = {((unsigned long long)a0.w << 32) | a0.z, a0.y, ((unsigned long long)a1.y << 32) | a1.x,
                                              ((unsigned long long)a1.w << 32) | a1.z};
            const unsigned long long vb[4] = {((unsigned long long)b0.w << 32) | b0.z, b0.y, ((unsigned long long)b1.y << 32) | b1.x,
                                              ((unsigned long long)b1.w << 32) | b1.z};
#pragma unroll
            for (int m = 0; m < 4; m++) {
                acc[32 + m] += va[m] & 0xffffffffull; acc[36 + m] += va[m] >> 32;
                acc[40 + m] += vb[m] & 0xffffffffull; acc[44 + m] += vb[m] >> 32;
                const bool up = vb[m] > va[m];
                const unsigned long long mag = up ? vb[m] - va[m] : va[m] - vb[m];
                const uint32_t bucket = stat_bucket(mag);
#pragma unroll
                for (int d = 0; d < 2; d++) {                                      // (constant indices only: everything stays in registers)
                    const int j = 2 * m + d;
                    const bool on = mag != 0 && up == (d == (int)MADSIM_PAIRED_UP);
                    const unsigned long long g = on ? mag : 0ull, inv = on ? ~mag : 0ull;
                    acc[j] = inv > acc[j] ? inv : acc[j];
                    acc[8 + j] = g > acc[8 + j] ? g : acc[8 + j];
                    acc[16 + j] += g & 0xffffffffull; acc[24 + j] += g >> 32;
                    if (on) { atomicAdd(&hist[j][bucket], 1u); nw[j] = TopKey{mag, ~(uint32_t)i}; }      // (a batch holds fewer than 2^32 seeds: i < 2^32 - 1, never 0)
                }
            }
        }
#pragma unroll
        for (int j = 0; j < (int)PAIRED_SETS; j++) n_dir[j] += (uint32_t)__popcll(__ballot(nw[j].k != 0));
        if (K && topk_enters<(int)PAIRED_SETS>(list, nw, K)) topk_merge<(int)PAIRED_SETS>(list, nw, K, lane);
    }
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int j = 0; j < (int)PAIRED_HEAD - 10; j++) {
            const unsigned long long t = __shfl_xor(acc[j], o);
            if (j < 16) acc[j] = t > acc[j] ? t : acc[j]; else acc[j] += t;
        }
    }
    if (lane == 0) {
        part[wave][0] = n_pair; part[wave][1] = n_inc;
#pragma unroll
        for (int j = 0; j < (int)PAIRED_SETS; j++) part[wave][2 + j] = n_dir[j];
#pragma unroll
        for (int j = 0; j < (int)PAIRED_HEAD - 10; j++) part[wave][10 + j] = acc[j];
    }
    if (K && lane < STAT_TOP) {
#pragma unroll
        for (int j = 0; j < (int)PAIRED_SETS; j++) { lv[j][wave * STAT_TOP + lane] = list[j].v; lk[j][wave * STAT_TOP + lane] = list[j].k; }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < (int)PAIRED_SETS; j++) {                                   // thread t: bucket t of every set
        const uint32_t c = hist[j][threadIdx.x];
        if (c) atomicAdd(&ghist[j * MADSIM_STAT_BUCKETS + threadIdx.x], c);
    }
    if (threadIdx.x < PAIRED_HEAD) {                                               // one set of atomics per workgroup that paired a seed (word 1: that met a runner verdict)
        const uint32_t j = threadIdx.x;
        const bool is_max = j >= 10 && j < 26;
        unsigned long long a = part[0][j];
        for (int w = 1; w < 4; w++) { const unsigned long long t = part[w][j]; if (is_max) a = t > a ? t : a; else a += t; }
        if (a) { if (is_max) atomicMax(&words[j], a); else atomicAdd(&words[j], a); }
    }
    if (K) {                                                                       // wave w: the workgroup's lists of sets w and w + 4
        for (uint32_t j = wave; j < PAIRED_SETS; j += 4) {
            TopKey l1[1] = {TopKey{0, 0}}, n1[1] = {TopKey{lv[j][lane], lk[j][lane]}};
            topk_merge<1>(l1, n1, K, lane);
            if (lane < STAT_TOP) {
                unsigned long long* p = cand + ((uint64_t)(j * STAT_WGS + blockIdx.x) * STAT_TOP + lane) * 2;
                p[0] = l1[0].v; p[1] = l1[0].k ? (unsigned long long)(uint32_t)~l1[0].k : ~0ull;
            }
        }
    }
}

// grid = PAIRED_SETS workgroups: workgroup j merges cand[j][0 .. n_wg)[0 .. 16) ({magnitude, index in the batch or ~0}) as stats_top_kernel
// does; top[j][r] = {seed, a, b} of metric j / 2, r < min(K, seeds of the batch in set j).  The list is read only for winners.
template <class Seeds>
__global__ __launch_bounds__(256) void paired_top_kernel(const madsim_result_t* __restrict__ ra, const madsim_result_t* __restrict__ rb,
                                                         const unsigned long long* __restrict__ cand, uint32_t n_wg, uint32_t K, const Seeds seed_of,
                                                         unsigned long long* __restrict__ top) {
    __shared__ unsigned long long lv[4 * STAT_TOP];
    __shared__ uint32_t lk[4 * STAT_TOP];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = blockIdx.x;
    const uint32_t total = n_wg * STAT_TOP, quarter = (total / 4 + 63) / 64 * 64;      // (total is a multiple of 16, at most 4 096)
    const uint32_t lo = wave * quarter, hi = lo + quarter < total ? lo + quarter : total;
    const unsigned long long* src = cand + (uint64_t)j * STAT_WGS * STAT_TOP * 2;
    TopKey list[1] = {TopKey{0, 0}};
    for (uint32_t base = lo; base < hi; base += 64) {
        const uint32_t c = base + lane;
        TopKey nw[1] = {TopKey{0, 0}};
        if (c < hi) {
            const unsigned long long v = src[2 * c], x = src[2 * c + 1];
            if (x != ~0ull) nw[0] = TopKey{v, ~(uint32_t)x};
        }
        if (topk_enters<1>(list, nw, K)) topk_merge<1>(list, nw, K, lane);
    }
    if (lane < STAT_TOP) { lv[wave * STAT_TOP + lane] = list[0].v; lk[wave * STAT_TOP + lane] = list[0].k; }
    __syncthreads();
    if (wave == 0) {
        TopKey l1[1] = {TopKey{0, 0}}, n1[1] = {TopKey{lv[lane], lk[lane]}};
        topk_merge<1>(l1, n1, K, lane);
        if (lane < K && l1[0].k) {
            const uint32_t idx = ~l1[0].k;
            unsigned long long* p = top + (uint64_t)(j * STAT_TOP + lane) * 3;         // 24 B records: 8-byte stores
            p[0] = seed_of(idx); p[1] = paired_metric(ra + idx, j >> 1); p[2] = paired_metric(rb + idx, j >> 1);
        }
    }
}

__global__ void keyflip_kernel(unsigned long long* acc) { acc[0] ^= 0x8000000000000000ull; }

// ---- resolving campaigns: which seeds of a batch are run again, and their new results back in place ----------------------------
// A result is RE-RUNNABLE when its verdict is MADSIM_OVERFLOW, or MADSIM_STEP_LIMIT while the step cap can still grow (steps_maxed == 0):
// rerun_runner_verdicts' rule (madsim_hip.cpp).  The list pair runs over collect's cut of the batch — wave W owns a contiguous piece, so
// ascending wave then ascending lane is ascending seed order: resolve_count_kernel reads the 16-byte head of every result and leaves every
// wave's number of re-runnable seeds in wave_cnt[W]; resolve_write_kernel gives a wave the exclusive prefix of wave_cnt as its offset and
// writes, for each re-runnable seed i of its piece, seed0 + i into `seeds` and i into `idx` at rank = offset + its position in the ballot.
// Wave 0 also leaves the total in *total.  No atomic anywhere: the lists are the same on every run, and nothing behind the total is
// written.  A wave without re-runnable seeds leaves after one load.  count < 2^32 (the index list is 32-bit).
__device__ __forceinline__ bool resolve_rerunnable(uint32_t verdict, uint32_t steps_maxed) {
    return verdict == MADSIM_OVERFLOW || (verdict == MADSIM_STEP_LIMIT && !steps_maxed);
}

__global__ __launch_bounds__(256) void resolve_count_kernel(const madsim_result_t* __restrict__ out, uint64_t count, uint64_t piece,
                                                            uint32_t steps_maxed, uint32_t* __restrict__ wave_cnt) {
    const uint32_t W = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint64_t lo = (uint64_t)W * piece, hi = lo + piece < count ? lo + piece : count;
    uint32_t n = 0;                                                                // wave-uniform (popcounts of ballots)
    for (uint64_t base = lo; base < hi; base += 64) {
        const uint64_t i = base + lane;
        uint32_t v = MADSIM_PASS;
        if (i < hi) v = reinterpret_cast<const uint4*>(out + i)[0].x;
        n += (uint32_t)__popcll(__ballot(resolve_rerunnable(v, steps_maxed)));
    }
    if (lane == 0) wave_cnt[W] = n;
}

template <class Seeds>
__global__ __launch_bounds__(256) void resolve_write_kernel(const madsim_result_t* __restrict__ out, uint64_t count, const Seeds seed_of,
                                                            uint64_t piece, uint32_t steps_maxed, const uint32_t* __restrict__ wave_cnt,
                                                            uint32_t n_waves, uint32_t* __restrict__ total, uint64_t* __restrict__ seeds,
                                                            uint32_t* __restrict__ idx) {
    const uint32_t W = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (W == 0) {                                                                  // the total: every wave's count, summed by the first wave
        uint32_t t = 0;
        for (uint32_t j = lane; j < n_waves; j += 64) t += wave_cnt[j];
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
        if (lane == 0) *total = t;
    }
    if (wave_cnt[W] == 0) return;                                                  // (wave-uniform)
    uint32_t at = 0;                                                               // re-runnable seeds of the waves before this one
    for (uint32_t j = lane; j < W; j += 64) at += wave_cnt[j];
    for (int o = 32; o > 0; o >>= 1) at += __shfl_xor(at, o);
    const uint64_t lo = (uint64_t)W * piece, hi = lo + piece < count ? lo + piece : count;
    for (uint64_t base = lo; base < hi; base += 64) {
        const uint64_t i = base + lane;
        uint32_t v = MADSIM_PASS;
        if (i < hi) v = reinterpret_cast<const uint4*>(out + i)[0].x;
        const bool mine = resolve_rerunnable(v, steps_maxed);
        const unsigned long long m = __ballot(mine);
        if (mine) {
            const uint32_t rank = at + lanes_below(m);
            seeds[rank] = seed_of(i);
            idx[rank] = (uint32_t)i;
        }
        at += (uint32_t)__popcll(m);
    }
}

// out[idx[j]] = rerun[j] for j < m: a 48-byte record is three 16-byte chunks and thread t moves chunk t % 3 of record t / 3, so the reads of
// the compact re-run array are one contiguous run of 16-byte loads.  Nothing else of `out` is touched; the indices are distinct.
__global__ __launch_bounds__(256) void resolve_scatter_kernel(madsim_result_t* __restrict__ out, const madsim_result_t* __restrict__ rerun,
                                                              const uint32_t* __restrict__ idx, uint32_t m) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const uint64_t j = t / 3;
    if (j >= m) return;
    const uint32_t chunk = (uint32_t)(t - 3 * j);
    reinterpret_cast<uint4*>(out + idx[j])[chunk] = reinterpret_cast<const uint4*>(rerun)[t];
}

// ---- divergence reports: where two variants of a seed's run first part --------------------------------------------------------------
// Two sets of trace rows of the same n seeds (the determinism log: 1-byte entries; the observation log: 8-byte entries), compared where
// they lie.  One wave per row pair, waves striding over the rows; a pure function of its inputs: no atomics, no LDS.  Both channels walk
// BYTES — an 8-byte entry's index is the byte index >> 3 — and only the first m = min(len_a, len_b, cap) entries: what lies behind
// min(len_x, cap) in a row is never compared (in real rows it is zeros, and a compare that ran into it would turn "one run ended where
// the other went on" into a later difference, or into none).
// diverge_walk: the index of the first byte < n_bytes at which a and b differ, or n_bytes; wave-uniform.  Row i starts at i * cap entries,
// so a and b are 16-byte aligned only when the pitch is; the launcher demands 16-byte aligned row arrays, so the two sides share the
// misalignment: up to 15 head bytes one per lane, then 16 bytes per lane and side per trip (1 KiB per side), the wave leaving at the first
// trip with a hit — a ballot of "my 16 bytes differ", then the lowest set lane's first differing byte —, then up to 15 tail bytes.
__device__ __forceinline__ uint64_t diverge_walk(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint64_t n_bytes, uint32_t lane) {
    const uint64_t mis = (uint64_t)(reinterpret_cast<uintptr_t>(a) & 15u);
    uint64_t head = mis ? 16u - mis : 0u;
    if (head > n_bytes) head = n_bytes;
    if (head) {                                                                    // (wave-uniform)
        const unsigned long long hit = __ballot(lane < head && a[lane] != b[lane]);
        if (hit) return (uint64_t)(__ffsll((long long)hit) - 1);
    }
    const uint4* __restrict__ qa = reinterpret_cast<const uint4*>(a + head);
    const uint4* __restrict__ qb = reinterpret_cast<const uint4*>(b + head);
    const uint64_t chunks = (n_bytes - head) >> 4;
    for (uint64_t base = 0; base < chunks; base += 64) {
        const uint64_t j = base + lane;
        uint32_t off = 16;                                                         // my first differing byte of the 16
        if (j < chunks) {
            const uint4 x = qa[j], y = qb[j];
            const uint32_t d[4] = {x.x ^ y.x, x.y ^ y.y, x.z ^ y.z, x.w ^ y.w};
#pragma unroll
            for (int k = 3; k >= 0; k--) if (d[k]) off = 4u * k + ((uint32_t)__ffs((int)d[k]) - 1u) / 8u;
        }
        const unsigned long long hit = __ballot(off < 16u);
        if (hit) {
            const int l = __ffsll((long long)hit) - 1;
            return head + ((base + (uint64_t)l) << 4) + (uint64_t)__shfl(off, l);
        }
    }
    const uint64_t done = head + (chunks << 4), tail = n_bytes - done;             // < 16
    if (tail) {
        const unsigned long long hit = __ballot(lane < tail && a[done + lane] != b[done + lane]);
        if (hit) return done + (uint64_t)(__ffsll((long long)hit) - 1);
    }
    return n_bytes;
}

// One channel of one row pair: status and `at` (entries of common prefix established), by the table in include/madsim_hip.h.  `shift`: 0 for
// 1-byte entries, 3 for 8-byte ones.  Wave-uniform; reads nothing of the rows when there is nothing to compare.
struct DivergeAt { uint32_t status; uint64_t at; };
__device__ __forceinline__ DivergeAt diverge_channel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint64_t len_a, uint64_t len_b,
                                                     uint64_t cap, uint32_t shift, bool runner, uint32_t lane) {
    if (runner) return DivergeAt{MADSIM_DIVERGE_INCOMPARABLE, 0};
    const uint64_t L = len_a < len_b ? len_a : len_b, m = L < cap ? L : cap;
    const uint64_t d = m ? diverge_walk(a, b, m << shift, lane) : 0;
    if (d < m << shift) return DivergeAt{MADSIM_DIVERGE_DIFFER, d >> shift};
    if (L > cap) return DivergeAt{MADSIM_DIVERGE_BEYOND_CAP, cap};
    return DivergeAt{len_a == len_b ? MADSIM_DIVERGE_SAME : MADSIM_DIVERGE_PREFIX, L};
}

// Record i (23 words, madsim_divergence_t) and context row i (3 * win words: the shared values [at - win, at) right-aligned, then A's and
// B's [at, at + win), each cut at min(len_x, cap); zeros wherever there is no entry, and everywhere under INCOMPARABLE).
__global__ __launch_bounds__(256) void diverge_kernel(const uint8_t* __restrict__ log_a, const uint8_t* __restrict__ log_b, uint64_t log_cap,
                                                      const unsigned long long* __restrict__ obs_a, const unsigned long long* __restrict__ obs_b,
                                                      uint64_t obs_cap, const unsigned long long* __restrict__ log_len_a,
                                                      const unsigned long long* __restrict__ log_len_b, const unsigned long long* __restrict__ obs_len_a,
                                                      const unsigned long long* __restrict__ obs_len_b, const madsim_result_t* __restrict__ res_a,
                                                      const madsim_result_t* __restrict__ res_b, const unsigned long long* __restrict__ seeds, uint64_t n,
                                                      uint32_t win, unsigned long long* __restrict__ recs, unsigned long long* __restrict__ ctx) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t i = blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += (uint64_t)gridDim.x * 4u) {      // (wave-uniform)
        const unsigned long long* ra = reinterpret_cast<const unsigned long long*>(res_a + i);
        const unsigned long long* rb = reinterpret_cast<const unsigned long long*>(res_b + i);
        const bool runner = MADSIM_IS_RUNNER_VERDICT((uint32_t)ra[0]) || MADSIM_IS_RUNNER_VERDICT((uint32_t)rb[0]);
        const uint64_t lla = log_len_a[i], llb = log_len_b[i], ola = obs_len_a[i], olb = obs_len_b[i];
        const uint8_t* la = log_a + i * log_cap;
        const uint8_t* lb = log_b + i * log_cap;
        const unsigned long long* oa = obs_a + i * obs_cap;
        const unsigned long long* ob = obs_b + i * obs_cap;
        const DivergeAt dl = diverge_channel(la, lb, lla, llb, log_cap, 0, runner, lane);
        const DivergeAt dob = diverge_channel(reinterpret_cast<const uint8_t*>(oa), reinterpret_cast<const uint8_t*>(ob), ola, olb, obs_cap, 3, runner, lane);
        const uint64_t ka_l = lla < log_cap ? lla : log_cap, kb_l = llb < log_cap ? llb : log_cap;      // entries kept of each row
        const uint64_t ka_o = ola < obs_cap ? ola : obs_cap, kb_o = olb < obs_cap ? olb : obs_cap;
        unsigned long long* const p = recs + i * 23u;
        if (lane == 0) {
            const bool cmp = !runner;
            p[0] = seeds[i];
            p[1] = (unsigned long long)dl.status | (unsigned long long)dob.status << 32;
            p[2] = dl.at; p[3] = dob.at;
            p[4] = lla; p[5] = llb; p[6] = ola; p[7] = olb;
            p[8] = cmp && dob.at < ka_o ? oa[dob.at] : 0ull;
            p[9] = cmp && dob.at < kb_o ? ob[dob.at] : 0ull;
            p[10] = (cmp && dl.at < ka_l ? (unsigned long long)la[dl.at] : 0ull) | (cmp && dl.at < kb_l ? (unsigned long long)lb[dl.at] << 8 : 0ull);
        }
        if (lane < 6) { p[11 + lane] = ra[lane]; p[17 + lane] = rb[lane]; }
        if (lane < 3 * win) {                                                      // (win <= 8: one word per lane)
            const uint32_t part = lane / win, j = lane - part * win;
            unsigned long long v = 0;
            if (!runner) {
                if (part == 0) { if (dob.at + j >= win) v = oa[dob.at + j - win]; }
                else {
                    const uint64_t k = dob.at + j;
                    if (part == 1) { if (k < ka_o) v = oa[k]; } else if (k < kb_o) v = ob[k];
                }
            }
            ctx[i * 3u * win + lane] = v;
        }
    }
}

// ---- the observation census: the distinct traced values of a chunk's counted seeds, each with its per-verdict seed counts ----
// Two kernels behind the chunk's trace launch.  census_fold_kernel: one wave per row, striding as diverge_kernel does.  A row is COUNTED as in
// stats_fold_kernel (bit `verdict` of `include`, bits 0-3 only); its visible observations are the first min(len, obs_cap), walked in
// rounds of 64.  Equal values of a round are combined by group_fold_kernel's ballot loop: one leader per distinct value, holding the
// popcount.  What a (row, value) adds to the table is {n_seeds[verdict] += 1, n_total += count, max_per_seed = max(count), smallest row =
// min}; the direct form (census_row_direct) adds it at once, the wave accumulator (census_row_acc) gathers a wave's rows in LDS first.
// The table is the grouping campaign's (group_insert), keyed by the value alone: a slot's TAG is 1 + the flat index (row * obs_cap + i) of
// one visible occurrence, the slot's value is read from the rows — which nobody writes while these kernels run —, one 32-bit
// compare-and-swap claims, every 64-bit value is legal.  Two leaders of one round that meet at one empty slot are two lanes of one
// atomicCAS: one claims, the other reads the winner's tag, finds another value behind it and probes on.  Every claim takes a number
// (one atomicAdd on words[0]): below `cap` it appends its slot to `list`, the claim that would be number cap + 1 sets
// MADSIM_K_CENSUS_ERR_CAP and writes nothing more.  The claims of a chunk are its distinct values, so that bit is a property of the data;
// once the error word is set, inserts return at once.  The count words ride in lanes 0 .. 10 of each wave and are added once, at its end.
// census_extract_kernel walks the list: entry j of slot list[j], the slot zeroed again — work proportional to the values.  With the
// error word set it writes no entry and clears the WHOLE table instead, claims beyond the list included.
constexpr uint32_t CENSUS_CLAIMS = 0, CENSUS_ERR = 1, CENSUS_COUNTS = 2, CENSUS_SLOT_WORDS = MADSIM_K_CENSUS_SLOT_BYTES / 4;

// the calling lane adds to `value`'s slot: ns[k] seeds of verdict k, `total` occurrences, `maxp` the most inside one seed, `row` the
// smallest row; one visible occurrence of the value lies at flat index `flat`
__device__ __forceinline__ void census_insert(const unsigned long long* __restrict__ obs, uint32_t total_obs, uint32_t* __restrict__ table, uint32_t mask,
                                              uint32_t* __restrict__ list, uint32_t cap, unsigned long long* __restrict__ words,
                                              unsigned long long value, uint4 ns, uint32_t total, uint32_t maxp, uint32_t row, uint32_t flat) {
    if (__hip_atomic_load(&words[CENSUS_ERR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;      // (the chunk has failed already)
    uint32_t s = (uint32_t)census_slot(value, (uint64_t)mask + 1u);
    for (uint32_t probe = 0; probe <= mask; probe++, s = (s + 1u) & mask) {
        uint32_t* const slot = table + (size_t)s * CENSUS_SLOT_WORDS;
        uint32_t tag = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (a tag only ever goes from 0 to its value)
        if (tag == 0) {
            tag = atomicCAS(slot, 0u, flat + 1u);
            if (tag == 0) {                                                        // claimed: the slot's value is this observation's
                const unsigned long long pos = atomicAdd(&words[CENSUS_CLAIMS], 1ull);
                if (pos >= cap) { atomicOr(&words[CENSUS_ERR], (unsigned long long)MADSIM_K_CENSUS_ERR_CAP); return; }
                list[pos] = s;
                tag = flat + 1u;
            }
        }
        bool match = tag == flat + 1u;
        if (!match) {
            const uint32_t rep = tag - 1u;
            if (rep >= total_obs) { atomicOr(&words[CENSUS_ERR], (unsigned long long)MADSIM_K_CENSUS_ERR_TAG); return; }      // (a table that was not clean)
            match = obs[rep] == value;
        }
        if (match) {
            if (ns.x) atomicAdd(slot + 1, ns.x);
            if (ns.y) atomicAdd(slot + 2, ns.y);
            if (ns.z) atomicAdd(slot + 3, ns.z);
            if (ns.w) atomicAdd(slot + 4, ns.w);
            atomicAdd(slot + 5, total); atomicMax(slot + 6, maxp); atomicMax(slot + 7, ~row);
            return;
        }
    }
    atomicOr(&words[CENSUS_ERR], (unsigned long long)MADSIM_K_CENSUS_ERR_PROBE);   // (a full table: only ever behind claim number cap + 1)
}

// The DIRECT form of a row: one table update per distinct value of the row.  A value that an earlier round of the row held is skipped (the
// seed counts once), and the leader of a value's FIRST round adds the later rounds' occurrences to its popcount, so it holds the row's
// full count.  Everything that steers the loops comes from ballots: the wave stays converged up to the insert.
__device__ __forceinline__ void census_row_direct(const unsigned long long* __restrict__ obs, uint32_t total_obs, uint32_t obs_cap, uint32_t i, uint32_t vis,
                                                  uint32_t v, uint32_t lane, uint32_t* __restrict__ table, uint32_t mask, uint32_t* __restrict__ list,
                                                  uint32_t cap, unsigned long long* __restrict__ words) {
    const unsigned long long* const row = obs + (size_t)i * obs_cap;
    for (uint32_t k = 0; k * 64u < vis; k++) {
        const uint32_t idx = k * 64u + lane;
        const bool have = idx < vis;
        const unsigned long long val = have ? row[idx] : 0ull;
        unsigned long long m = __ballot(have);
        uint32_t cnt = 0;                                                          // non-zero in the leaders
        while (m) {                                                                // (wave-uniform) one trip per distinct value of the round
            const int l = __ffsll((long long)m) - 1;
            const unsigned long long lk = __shfl(val, l);
            const unsigned long long sm = __ballot(have && val == lk);
            m &= ~sm;
            bool earlier = false;                                                  // rounds below k are full: every lane's index is visible
            for (uint32_t j = 0; j < k && !earlier; j++) earlier = __ballot(row[j * 64u + lane] == lk) != 0;
            if (earlier) continue;
            uint32_t c = (uint32_t)__popcll(sm);
            for (uint32_t j = k + 1u; j * 64u < vis; j++) {
                const uint32_t x = j * 64u + lane;
                c += (uint32_t)__popcll(__ballot(x < vis && row[x] == lk));
            }
            if ((int)lane == l) cnt = c;
        }
        if (cnt) census_insert(obs, total_obs, table, mask, list, cap, words, val, make_uint4(v == 0u, v == 1u, v == 2u, v == 3u), cnt, cnt, i, i * obs_cap + idx);
    }
}

// The WAVE ACCUMULATOR: CENSUS_ACC_SLOTS entries per wave in LDS, keyed by value, written by that wave alone — a wave walks its rows one
// after another.  An entry is CENSUS_ACC_WORDS planes wide: {tag = 1 + flat index of one occurrence (0 = free), value low, value high,
// stamp = 1 + the last row that held the value, that row's count so far, n_seeds[4], n_total, max_per_seed, smallest row}.  The stamp gives
// both the once-per-seed rule and the per-row count: a round's leader that finds another row's stamp starts the row (n_seeds[verdict] += 1,
// count = its popcount), one that finds its own row's adds to the count.  Leaders of one round hold different values, so they update
// different entries; two of them that meet at one free entry are two lanes of one LDS compare-and-swap — the loser sees, behind the wave
// fence, the winner's value and probes on.  An entry is only ever claimed while fewer than CENSUS_ACC_FILL are in use, so a probe ends.
// The accumulator is flushed to the table between rows, when CENSUS_ACC_FILL minus the entries in use is less than the next row's
// visible length (it could not be sure to hold the row), and once more at the wave's end; a row longer than CENSUS_ACC_FILL takes the
// direct form.  A flush is one census_insert per entry in use — with a ten-value vocabulary ten per wave, whatever the number of rows.
constexpr uint32_t CENSUS_ACC_SLOTS = 256, CENSUS_ACC_FILL = 192, CENSUS_ACC_WORDS = 12;
enum { ACC_TAG, ACC_LO, ACC_HI, ACC_STAMP, ACC_ROWCNT, ACC_NS, ACC_TOTAL = ACC_NS + 4, ACC_MAXP, ACC_FIRST };
static_assert(ACC_FIRST + 1 == CENSUS_ACC_WORDS && 4 * CENSUS_ACC_WORDS * CENSUS_ACC_SLOTS * sizeof(uint32_t) <= 49152, "the accumulators of a workgroup's four waves");

__device__ __forceinline__ void census_wave_fence() {      // LDS words one lane wrote, read by another lane of the same wave
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// returns the number of entries the row claimed (wave-uniform)
__device__ __forceinline__ uint32_t census_row_acc(uint32_t* __restrict__ A, const unsigned long long* __restrict__ obs, uint32_t obs_cap, uint32_t i,
                                                   uint32_t vis, uint32_t v, uint32_t lane, unsigned long long* __restrict__ words) {
    const unsigned long long* const row = obs + (size_t)i * obs_cap;
    uint32_t claimed = 0;
    for (uint32_t k = 0; k * 64u < vis; k++) {
        const uint32_t idx = k * 64u + lane;
        const bool have = idx < vis;
        const unsigned long long val = have ? row[idx] : 0ull;
        unsigned long long m = __ballot(have);
        uint32_t cnt = 0;                                                          // non-zero in the leaders
        while (m) {                                                                // (wave-uniform) one trip per distinct value of the round
            const int l = __ffsll((long long)m) - 1;
            const unsigned long long lk = __shfl(val, l);
            const unsigned long long sm = __ballot(have && val == lk);
            if ((int)lane == l) cnt = (uint32_t)__popcll(sm);
            m &= ~sm;
        }
        bool pending = cnt != 0;
        uint32_t s = (uint32_t)census_slot(val, CENSUS_ACC_SLOTS);
        for (uint32_t probe = 0; __ballot(pending); probe++) {                     // (wave-uniform) the leaders, all at once
            bool won = false;
            if (pending && A[ACC_TAG * CENSUS_ACC_SLOTS + s] == 0u) {
                won = atomicCAS(&A[ACC_TAG * CENSUS_ACC_SLOTS + s], 0u, i * obs_cap + idx + 1u) == 0u;
                if (won) {                                                         // (every other plane of a free entry is zero)
                    A[ACC_LO * CENSUS_ACC_SLOTS + s] = (uint32_t)val;
                    A[ACC_HI * CENSUS_ACC_SLOTS + s] = (uint32_t)(val >> 32);
                    A[ACC_FIRST * CENSUS_ACC_SLOTS + s] = i;
                }
            }
            claimed += (uint32_t)__popcll(__ballot(won));
            census_wave_fence();
            if (pending) {
                const unsigned long long held = (unsigned long long)A[ACC_LO * CENSUS_ACC_SLOTS + s] | (unsigned long long)A[ACC_HI * CENSUS_ACC_SLOTS + s] << 32;
                if (held == val) {                                                 // (the entry is in use: this lane's claim, or an earlier one)
                    uint32_t rc = cnt;
                    if (A[ACC_STAMP * CENSUS_ACC_SLOTS + s] != i + 1u) {
                        A[ACC_STAMP * CENSUS_ACC_SLOTS + s] = i + 1u;
                        A[(ACC_NS + v) * CENSUS_ACC_SLOTS + s] += 1u;
                    } else {
                        rc += A[ACC_ROWCNT * CENSUS_ACC_SLOTS + s];
                    }
                    A[ACC_ROWCNT * CENSUS_ACC_SLOTS + s] = rc;
                    A[ACC_TOTAL * CENSUS_ACC_SLOTS + s] += cnt;
                    if (rc > A[ACC_MAXP * CENSUS_ACC_SLOTS + s]) A[ACC_MAXP * CENSUS_ACC_SLOTS + s] = rc;
                    pending = false;
                } else if (probe >= CENSUS_ACC_SLOTS) {                            // (cannot happen below CENSUS_ACC_FILL entries in use)
                    atomicOr(&words[CENSUS_ERR], (unsigned long long)MADSIM_K_CENSUS_ERR_PROBE);
                    pending = false;
                } else {
                    s = (s + 1u) & (CENSUS_ACC_SLOTS - 1u);
                }
            }
            census_wave_fence();
        }
    }
    return claimed;
}

__device__ __forceinline__ void census_acc_flush(uint32_t* __restrict__ A, uint32_t lane, const unsigned long long* __restrict__ obs, uint32_t total_obs,
                                                 uint32_t* __restrict__ table, uint32_t mask, uint32_t* __restrict__ list, uint32_t cap,
                                                 unsigned long long* __restrict__ words) {
    census_wave_fence();
    for (uint32_t s = lane; s < CENSUS_ACC_SLOTS; s += 64u) {
        const uint32_t tag = A[ACC_TAG * CENSUS_ACC_SLOTS + s];
        if (tag == 0u) continue;
        const unsigned long long value = (unsigned long long)A[ACC_LO * CENSUS_ACC_SLOTS + s] | (unsigned long long)A[ACC_HI * CENSUS_ACC_SLOTS + s] << 32;
        const uint4 ns = make_uint4(A[(ACC_NS + 0) * CENSUS_ACC_SLOTS + s], A[(ACC_NS + 1) * CENSUS_ACC_SLOTS + s], A[(ACC_NS + 2) * CENSUS_ACC_SLOTS + s],
                                    A[(ACC_NS + 3) * CENSUS_ACC_SLOTS + s]);
        census_insert(obs, total_obs, table, mask, list, cap, words, value, ns, A[ACC_TOTAL * CENSUS_ACC_SLOTS + s], A[ACC_MAXP * CENSUS_ACC_SLOTS + s],
                      A[ACC_FIRST * CENSUS_ACC_SLOTS + s], tag - 1u);
        for (uint32_t q = 0; q < CENSUS_ACC_WORDS; q++) A[q * CENSUS_ACC_SLOTS + s] = 0u;
    }
    census_wave_fence();
}

// ACC = false: every row in the direct form — the correctness baseline and the other side of the A/B (MADSIM_HIP_CENSUS_DIRECT=1)
template <bool ACC>
__global__ __launch_bounds__(256) void census_fold_kernel(const unsigned long long* __restrict__ obs, uint32_t obs_cap,
                                                          const unsigned long long* __restrict__ obs_len, const madsim_result_t* __restrict__ res,
                                                          uint32_t n, uint32_t include, uint32_t* __restrict__ table, uint32_t mask,
                                                          uint32_t* __restrict__ list, uint32_t cap, unsigned long long* __restrict__ words) {
    __shared__ uint32_t lds[ACC ? 4 * CENSUS_ACC_WORDS * CENSUS_ACC_SLOTS : 1];
    const uint32_t lane = threadIdx.x & 63, total_obs = n * obs_cap;
    uint32_t* const A = lds + (ACC ? (threadIdx.x >> 6) * CENSUS_ACC_WORDS * CENSUS_ACC_SLOTS : 0u);
    uint32_t in_use = 0;                                                           // entries of A in use (wave-uniform)
    if (ACC) {
        for (uint32_t q = lane; q < CENSUS_ACC_WORDS * CENSUS_ACC_SLOTS; q += 64u) A[q] = 0u;
        census_wave_fence();
    }
    uint32_t acc = 0;                                                              // lane k < 11: what this wave adds to words[2 + k]
    for (uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += gridDim.x * 4u) {      // (wave-uniform)
        const uint32_t v = reinterpret_cast<const uint32_t*>(res + i)[0];
        if (v >= 4u) { acc += lane == 10u; continue; }                             // a runner verdict: the row is not read
        if (!((include >> v) & 1u)) continue;
        const unsigned long long len = obs_len[i];
        const uint32_t vis = len < obs_cap ? (uint32_t)len : obs_cap;
        acc += (lane == v) + (lane == 4u + v && vis == 0u) + (lane == 8u && len > obs_cap) + (lane == 9u ? vis : 0u);
        if (!ACC || vis > CENSUS_ACC_FILL) {
            census_row_direct(obs, total_obs, obs_cap, i, vis, v, lane, table, mask, list, cap, words);
        } else {
            if (in_use + vis > CENSUS_ACC_FILL) { census_acc_flush(A, lane, obs, total_obs, table, mask, list, cap, words); in_use = 0; }
            in_use += census_row_acc(A, obs, obs_cap, i, vis, v, lane, words);
        }
    }
    if (ACC && in_use) census_acc_flush(A, lane, obs, total_obs, table, mask, list, cap, words);
    if (lane < 11u && acc) atomicAdd(&words[CENSUS_COUNTS + lane], (unsigned long long)acc);
}

__global__ __launch_bounds__(256) void census_extract_kernel(const unsigned long long* __restrict__ obs, uint32_t total_obs,
                                                             const unsigned long long* __restrict__ seeds, uint32_t n, uint32_t* __restrict__ table,
                                                             uint32_t mask, const uint32_t* __restrict__ list, uint32_t cap,
                                                             unsigned long long* __restrict__ words, unsigned long long* __restrict__ entries) {
    uint4* const t = reinterpret_cast<uint4*>(table);                              // a slot is two of them
    if (words[CENSUS_ERR]) {                                                       // (nobody sets it in this branch: uniform over the grid)
        for (uint64_t j = blockIdx.x * 256u + threadIdx.x; j < 2ull * ((uint64_t)mask + 1u); j += gridDim.x * 256u) t[j] = uint4{0, 0, 0, 0};
        return;
    }
    const unsigned long long claimed = words[CENSUS_CLAIMS];                       // (nobody adds to it in this kernel)
    const uint32_t nv = claimed < cap ? (uint32_t)claimed : cap;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < nv; j += gridDim.x * 256u) {
        const uint32_t s = list[j] & mask;
        const uint4 e0 = t[2 * (size_t)s], e1 = t[2 * (size_t)s + 1];
        t[2 * (size_t)s] = uint4{0, 0, 0, 0}; t[2 * (size_t)s + 1] = uint4{0, 0, 0, 0};
        const uint32_t rep = e0.x - 1u, first = ~e1.w;
        unsigned long long* const p = entries + 8 * (size_t)j;
        if (e0.x == 0 || rep >= total_obs || first >= n) {                         // (a table that was not clean)
            atomicOr(&words[CENSUS_ERR], (unsigned long long)MADSIM_K_CENSUS_ERR_TAG);
            for (int q = 0; q < 8; q++) p[q] = 0;
            continue;
        }
        p[0] = obs[rep];
        p[1] = e0.y; p[2] = e0.z; p[3] = e0.w; p[4] = e1.x;
        p[5] = e1.y;
        p[6] = seeds[first];
        p[7] = e1.z;
    }
}

// ---- the stall-site census: a chunk's task rows made into site rows and shape words, which the observation census's kernels then fold ----
// stall_sites_kernel, behind the chunk's trace launch: one wave per row, striding as census_fold_kernel does, a row in rounds of 64 records.
// The visible records of row i are the first min(len, task_cap) — of a row whose verdict is a runner verdict none: neither that row nor
// its count is read.  Site row i: MADSIM_TASK_SITE of each visible record, zeros behind them (every word of the row is written).  Shape
// word i: the sum over the visible records of splitmix64's finaliser of the site — a lane's share added up, then a butterfly over the
// wave: commutative, so the word names the multiset of sites whatever the slot order; 0 for the empty table.  ones[i] = 1: the shape words
// are folded as rows of cap 1 and length 1.  A pure function of its inputs; the inputs are not written.
__device__ __forceinline__ unsigned long long stall_mix(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__global__ __launch_bounds__(256) void stall_sites_kernel(const unsigned long long* __restrict__ tasks, uint32_t task_cap,
                                                          const unsigned long long* __restrict__ task_len, const madsim_result_t* __restrict__ res,
                                                          uint32_t n, unsigned long long* __restrict__ sites, unsigned long long* __restrict__ shape,
                                                          unsigned long long* __restrict__ ones) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += gridDim.x * 4u) {      // (wave-uniform)
        const uint32_t v = reinterpret_cast<const uint32_t*>(res + i)[0];
        uint32_t vis = 0;
        if (v < 4u) { const unsigned long long len = task_len[i]; vis = len < task_cap ? (uint32_t)len : task_cap; }
        const unsigned long long* const row = tasks + (size_t)i * task_cap;
        unsigned long long* const out = sites + (size_t)i * task_cap;
        unsigned long long sum = 0;
        for (uint32_t k = 0; k * 64u < task_cap; k++) {
            const uint32_t idx = k * 64u + lane;
            if (idx < task_cap) {
                unsigned long long site = 0;
                if (idx < vis) { site = row[idx] >> 32; sum += stall_mix(site); }
                out[idx] = site;
            }
        }
        for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == 0) { shape[i] = sum; ones[i] = 1ull; }
    }
}

// ---- the probe-set census: which COMBINATIONS of vocabulary values a chunk's counted seeds reach, each with its per-verdict seed counts ----
// Three kernels behind the chunk's trace launch.  sets_mask_kernel: one wave per row, striding as census_fold_kernel does; rows of uncounted
// and runner seeds are not read.  The row index is made scalar (readfirstlane), so the verdict, the length and the loop bounds live in
// scalar registers and the wave stays converged.  The visible observations are walked in rounds of 64, one coalesced 8-byte load per lane;
// per vocabulary entry one wave-wide 64-bit compare against a scalar operand — the vocabulary travels by value in the kernel arguments
// (496 bytes, as sweep_count_kernel's pointer table does), so entry j is one scalar load from the argument segment —, whose mask says "any
// lane matched" and joins the round's hit mask; valid lanes outside the hit mask give OTHER.  No LDS, no atomics.  The walk ends early
// once every vocabulary bit and OTHER are set.  Lane 0 writes the row's set word to sig[i].
// sets_fold_kernel: one lane per seed over sig[] and the results.  Equal set words of a wave's 64 seeds are combined by group_fold_kernel's
// ballot loop, the verdict NOT part of the key: a leader holds the four per-verdict popcounts and the four per-verdict smallest indices
// (lanes hold ascending seeds: the lowest lane of a verdict's ballot).  One insert per leader into the census's table (census_insert's
// claim rule): the TAG is 1 + the index of the leader's seed, the key is read from sig[] — which nobody writes while this kernel runs —,
// one 32-bit compare-and-swap claims, nobody waits for a "ready" word, every claim takes a number and appends its slot to `list`, the
// claim that would be number cap + 1 sets MADSIM_K_PROBE_SETS_ERR_CAP.  A slot is {tag, n_seeds[4], ~smallest index[4]} (inverted, so that
// zero is neutral).  A range with four sets puts 65 536 seeds onto four slots: the in-wave combine makes that at most four inserts per
// wave (COMBINE = false, one insert per seed, is the baseline of the A/B).  The count words ride in lanes 0 .. 4 and are added once per wave.
// sets_extract_kernel walks the list: entry j of slot list[j], the slot zeroed again; with the error word set it writes no entry and
// clears the WHOLE table instead.
struct SetsVocab { unsigned long long v[MADSIM_PROBE_SETS_MAX_VOCAB]; };
constexpr uint32_t SETS_CLAIMS = 0, SETS_ERR = 1, SETS_COUNTS = 2, SETS_SLOT_WORDS = MADSIM_K_PROBE_SETS_SLOT_BYTES / 4;

__global__ __launch_bounds__(256) void sets_mask_kernel(const unsigned long long* __restrict__ obs, uint32_t obs_cap,
                                                        const unsigned long long* __restrict__ obs_len, const madsim_result_t* __restrict__ res,
                                                        uint32_t n, uint32_t include, const SetsVocab vocab, uint32_t m,
                                                        unsigned long long* __restrict__ sig) {
    const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned long long full = (~0ull >> (64u - m)) | MADSIM_PROBE_SET_OTHER;      // (1 <= m <= 62)
    for (uint32_t i = blockIdx.x * 4u + wave; i < n; i += gridDim.x * 4u) {        // (scalar)
        const uint32_t v = reinterpret_cast<const uint32_t*>(res + i)[0];
        if (v >= 4u || !((include >> v) & 1u)) continue;                           // a runner or left-out verdict: the row is not read
        const unsigned long long len = obs_len[i];
        const uint32_t vis = len < obs_cap ? (uint32_t)len : obs_cap;
        const unsigned long long* const row = obs + (size_t)i * obs_cap;
        unsigned long long set = 0;
        for (uint32_t k = 0; k * 64u < vis && (set & full) != full; k++) {
            const uint32_t idx = k * 64u + lane;
            const bool have = idx < vis;
            const unsigned long long val = have ? row[idx] : 0ull;
            const unsigned long long valid = __ballot(have);
            unsigned long long hit = 0;
            for (uint32_t j = 0; j < m; j++) {
                const unsigned long long b = __ballot(val == vocab.v[j]) & valid;
                hit |= b;
                set |= (unsigned long long)(b != 0ull) << j;
            }
            if (valid & ~hit) set |= MADSIM_PROBE_SET_OTHER;
        }
        if (len > obs_cap) set |= MADSIM_PROBE_SET_TRUNCATED;
        if (lane == 0u) sig[i] = set;
    }
}

// the calling lane adds to set word `key`'s slot: ns[k] seeds of verdict k, the smallest of them index ~nf[k] (nf[k] = 0: none); seed i has the set
__device__ __forceinline__ void sets_insert(const unsigned long long* __restrict__ sig, uint32_t n, uint32_t* __restrict__ table, uint32_t mask,
                                            uint32_t* __restrict__ list, uint32_t cap, unsigned long long* __restrict__ words,
                                            unsigned long long key, uint4 ns, uint4 nf, uint32_t i) {
    if (__hip_atomic_load(&words[SETS_ERR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;        // (the chunk has failed already)
    uint32_t s = (uint32_t)census_slot(key, (uint64_t)mask + 1u);
    for (uint32_t probe = 0; probe <= mask; probe++, s = (s + 1u) & mask) {
        uint32_t* const slot = table + (size_t)s * SETS_SLOT_WORDS;
        uint32_t tag = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (a tag only ever goes from 0 to its value)
        if (tag == 0) {
            tag = atomicCAS(slot, 0u, i + 1u);
            if (tag == 0) {                                                        // claimed: the slot's set is this seed's
                const unsigned long long pos = atomicAdd(&words[SETS_CLAIMS], 1ull);
                if (pos >= cap) { atomicOr(&words[SETS_ERR], (unsigned long long)MADSIM_K_PROBE_SETS_ERR_CAP); return; }
                list[pos] = s;
                tag = i + 1u;
            }
        }
        bool match = tag == i + 1u;
        if (!match) {
            const uint32_t rep = tag - 1u;
            if (rep >= n) { atomicOr(&words[SETS_ERR], (unsigned long long)MADSIM_K_PROBE_SETS_ERR_TAG); return; }      // (a table that was not clean)
            match = sig[rep] == key;
        }
        if (match) {
            if (ns.x) { atomicAdd(slot + 1, ns.x); atomicMax(slot + 5, nf.x); }
            if (ns.y) { atomicAdd(slot + 2, ns.y); atomicMax(slot + 6, nf.y); }
            if (ns.z) { atomicAdd(slot + 3, ns.z); atomicMax(slot + 7, nf.z); }
            if (ns.w) { atomicAdd(slot + 4, ns.w); atomicMax(slot + 8, nf.w); }
            return;
        }
    }
    atomicOr(&words[SETS_ERR], (unsigned long long)MADSIM_K_PROBE_SETS_ERR_PROBE);  // (a full table: only ever behind claim number cap + 1)
}

// COMBINE = false: one insert per counted seed — the correctness baseline and the other side of the A/B
template <bool COMBINE>
__global__ __launch_bounds__(256) void sets_fold_kernel(const unsigned long long* __restrict__ sig, const madsim_result_t* __restrict__ res, uint32_t n,
                                                        uint32_t include, uint32_t* __restrict__ table, uint32_t mask, uint32_t* __restrict__ list,
                                                        uint32_t cap, unsigned long long* __restrict__ words) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t acc = 0;                                                              // lane k < 4: counted seeds of verdict k; lane 4: runner verdicts
    for (uint64_t base = (uint64_t)(blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u; base < n; base += (uint64_t)gridDim.x * 256u) {      // (wave-uniform)
        const uint64_t i = base + lane;
        uint32_t v = 0u;
        const bool in = i < n;
        if (in) v = reinterpret_cast<const uint32_t*>(res + i)[0];
        const bool counted = in && v < 4u && ((include >> v) & 1u);
        const unsigned long long b0 = __ballot(counted && v == 0u), b1 = __ballot(counted && v == 1u), b2 = __ballot(counted && v == 2u),
                                 b3 = __ballot(counted && v == 3u), br = __ballot(in && v >= 4u);
        acc += (uint32_t)__popcll(lane == 0u ? b0 : lane == 1u ? b1 : lane == 2u ? b2 : lane == 3u ? b3 : lane == 4u ? br : 0ull);
        unsigned long long m = b0 | b1 | b2 | b3;
        if (!m) continue;                                                          // (wave-uniform: a round with nothing counted ends here)
        const unsigned long long key = counted ? sig[i] : 0ull;
        if (COMBINE) {
            uint4 ns = {0, 0, 0, 0}, nf = {0, 0, 0, 0};                            // non-zero in the leaders
            while (m) {                                                            // (wave-uniform) one trip per distinct set word of the round
                const int l = __ffsll((long long)m) - 1;
                const unsigned long long lk = __shfl(key, l);
                const unsigned long long sm = __ballot(counted && key == lk);     // a subset of m: lane l's set is none of the earlier leaders'
                if ((int)lane == l) {
                    const unsigned long long s0 = sm & b0, s1 = sm & b1, s2 = sm & b2, s3 = sm & b3;
                    const uint32_t lo = (uint32_t)base;
                    ns = make_uint4((uint32_t)__popcll(s0), (uint32_t)__popcll(s1), (uint32_t)__popcll(s2), (uint32_t)__popcll(s3));
                    nf = make_uint4(s0 ? ~(lo + (uint32_t)__ffsll((long long)s0) - 1u) : 0u, s1 ? ~(lo + (uint32_t)__ffsll((long long)s1) - 1u) : 0u,
                                    s2 ? ~(lo + (uint32_t)__ffsll((long long)s2) - 1u) : 0u, s3 ? ~(lo + (uint32_t)__ffsll((long long)s3) - 1u) : 0u);
                }
                m &= ~sm;
            }
            if (ns.x | ns.y | ns.z | ns.w) sets_insert(sig, n, table, mask, list, cap, words, key, ns, nf, (uint32_t)i);
        } else if (counted) {
            const uint32_t inv = ~(uint32_t)i;
            sets_insert(sig, n, table, mask, list, cap, words, key, make_uint4(v == 0u, v == 1u, v == 2u, v == 3u),
                        make_uint4(v == 0u ? inv : 0u, v == 1u ? inv : 0u, v == 2u ? inv : 0u, v == 3u ? inv : 0u), (uint32_t)i);
        }
    }
    if (lane < 5u && acc) atomicAdd(&words[SETS_COUNTS + lane], (unsigned long long)acc);
}

__global__ __launch_bounds__(256) void sets_extract_kernel(const unsigned long long* __restrict__ sig, const unsigned long long* __restrict__ seeds,
                                                           uint32_t n, uint32_t* __restrict__ table, uint32_t mask, const uint32_t* __restrict__ list,
                                                           uint32_t cap, unsigned long long* __restrict__ words, unsigned long long* __restrict__ entries) {
    uint4* const t = reinterpret_cast<uint4*>(table);                              // a slot is three of them
    if (words[SETS_ERR]) {                                                         // (nobody sets it in this branch: uniform over the grid)
        for (uint64_t j = blockIdx.x * 256u + threadIdx.x; j < 3ull * ((uint64_t)mask + 1u); j += gridDim.x * 256u) t[j] = uint4{0, 0, 0, 0};
        return;
    }
    const unsigned long long claimed = words[SETS_CLAIMS];                         // (nobody adds to it in this kernel)
    const uint32_t ne = claimed < cap ? (uint32_t)claimed : cap;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < ne; j += gridDim.x * 256u) {
        const uint32_t s = list[j] & mask;
        const uint4 e0 = t[3 * (size_t)s], e1 = t[3 * (size_t)s + 1], e2 = t[3 * (size_t)s + 2];
        t[3 * (size_t)s] = uint4{0, 0, 0, 0}; t[3 * (size_t)s + 1] = uint4{0, 0, 0, 0}; t[3 * (size_t)s + 2] = uint4{0, 0, 0, 0};
        const uint32_t rep = e0.x - 1u;
        const uint32_t cnt[4] = {e0.y, e0.z, e0.w, e1.x}, first[4] = {~e1.y, ~e1.z, ~e1.w, ~e2.x};
        unsigned long long* const p = entries + 9 * (size_t)j;
        bool bad = e0.x == 0 || rep >= n;
        for (int k = 0; k < 4; k++) bad |= cnt[k] != 0u && first[k] >= n;
        if (bad) {                                                                 // (a table that was not clean)
            atomicOr(&words[SETS_ERR], (unsigned long long)MADSIM_K_PROBE_SETS_ERR_TAG);
            for (int q = 0; q < 9; q++) p[q] = 0;
            continue;
        }
        p[0] = sig[rep];
        for (int k = 0; k < 4; k++) { p[1 + k] = cnt[k]; p[5 + k] = cnt[k] ? seeds[first[k]] : 0ull; }
    }
}

// ---- the probe-order census: which vocabulary value a chunk's counted seeds reach FIRST, cell (a, b) = "a before b", per verdict -----------
// Two kernels behind the chunk's trace launch.  order_fold_kernel: one wave per row, striding as sets_mask_kernel does, the row index,
// the verdict, the length and the loop bounds in scalar registers; rows of uncounted and runner seeds are not read.  The visible
// observations are walked in rounds of 64, one coalesced 8-byte load per lane; per vocabulary entry j not yet placed one wave-wide compare
// against a scalar operand from the kernel-argument struct (256 bytes) and a ballot; lane j keeps first(j), set ONCE from the lowest bit of
// the first non-empty ballot (64 * round + ctz) and never moved by a later occurrence: a placed entry is not compared again.  The walk
// ends once every entry is placed.  Then the row's relation: for each placed i (a scalar walk over the placed mask, first(i) read from
// lane i into a scalar register) the lanes j with j == i, or first(j) defined and first(i) < first(j), add 1 to cell [verdict][i][j] and
// max the inverted row index into its witness (inverted, so that zero is neutral, as sets_insert does): consecutive lanes, consecutive
// words — one conflict-free add and one max per present i.  LDS_ACC: the cells are a workgroup accumulator in LDS (32 KB: four waves'
// rows meet there, and every row the workgroup strides over), updated with LDS atomics and flushed once, the non-zero cells only, into
// the global matrix with atomicAdd / atomicMax: integer add and max commute, so no arrival order shows.  LDS_ACC = false sends the same
// updates straight to the global matrix: the correctness baseline and the other side of the A/B.  The count words ride in lanes 0 .. 9
// and are added once per wave, as in sets_fold_kernel.
// order_extract_kernel: one workgroup of 1024 threads, thread t owning cell (t >> 5, t & 31).  The non-zero cells are placed by a ballot
// per wave and a prefix sum over the sixteen wave counts — no atomic decides a position —, so the entries leave ascending by (a, b);
// first_seed[k] = seeds[~witness]; every cell is written back to zero.
struct OrderVocab { unsigned long long v[MADSIM_PROBE_ORDER_MAX_VOCAB]; };
constexpr uint32_t ORDER_ENTRIES = 0, ORDER_ERR = 1, ORDER_COUNTS = 2, ORDER_CELLS = 4u * 32u * 32u, ORDER_UNDEF = 0xffffffffu;
static_assert(2 * ORDER_CELLS == MADSIM_K_PROBE_ORDER_MATRIX_WORDS && MADSIM_PROBE_ORDER_MAX_VOCAB == 32, "the matrix");

template <bool LDS_ACC>
__global__ __launch_bounds__(256) void order_fold_kernel(const unsigned long long* __restrict__ obs, uint32_t obs_cap,
                                                         const unsigned long long* __restrict__ obs_len, const madsim_result_t* __restrict__ res,
                                                         uint32_t n, uint32_t include, const OrderVocab vocab, uint32_t m,
                                                         uint32_t* __restrict__ matrix, unsigned long long* __restrict__ words) {
    __shared__ uint32_t acc_lds[LDS_ACC ? 2 * ORDER_CELLS : 1];
    const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (LDS_ACC) {
        for (uint32_t c = threadIdx.x; c < 2 * ORDER_CELLS; c += 256u) acc_lds[c] = 0u;
        __syncthreads();
    }
    uint32_t* const cells = LDS_ACC ? acc_lds : matrix;
    const uint32_t full = 0xffffffffu >> (32u - m);                                // (1 <= m <= 32)
    uint32_t acc = 0;                                                              // lane k < 4: counted seeds of verdict k; 4 + k: of them none visible; 8: truncated; 9: runner
    for (uint32_t i = blockIdx.x * 4u + wave; i < n; i += gridDim.x * 4u) {        // (scalar)
        const uint32_t v = reinterpret_cast<const uint32_t*>(res + i)[0];
        if (v >= 4u) { acc += lane == 9u; continue; }
        if (!((include >> v) & 1u)) continue;                                      // a left-out verdict: the row is not read
        const unsigned long long len = obs_len[i];
        const uint32_t vis = len < obs_cap ? (uint32_t)len : obs_cap;
        const unsigned long long* const row = obs + (size_t)i * obs_cap;
        uint32_t first = ORDER_UNDEF, placed = 0;                                  // lane j: first(j); (scalar) the entries placed so far
        for (uint32_t k = 0; k * 64u < vis && placed != full; k++) {
            const uint32_t idx = k * 64u + lane;
            const bool have = idx < vis;
            const unsigned long long val = have ? row[idx] : 0ull;
            const unsigned long long valid = __ballot(have);
            for (uint32_t j = 0; j < m; j++) {
                if ((placed >> j) & 1u) continue;                                  // (scalar) placed once, never moved
                const unsigned long long b = __ballot(val == vocab.v[j]) & valid;
                if (b) {
                    if (lane == j) first = k * 64u + (uint32_t)__ffsll((long long)b) - 1u;
                    placed |= 1u << j;
                }
            }
        }
        acc += (lane == v) + (lane == 4u + v && !placed) + (lane == 8u && len > obs_cap);
        const uint32_t inv = ~i;
        uint32_t* const cnt = cells + v * 1024u;
        for (uint32_t p = placed; p; p &= p - 1u) {                                // (scalar) one trip per value the row reached
            const uint32_t a = (uint32_t)__ffs((int)p) - 1u;
            const uint32_t fa = (uint32_t)__builtin_amdgcn_readlane((int)first, (int)a);
            if (lane == a || (first != ORDER_UNDEF && fa < first)) {               // (lanes at or above m never hold a first)
                atomicAdd(cnt + a * 32u + lane, 1u);
                atomicMax(cnt + ORDER_CELLS + a * 32u + lane, inv);
            }
        }
    }
    if (lane < 10u && acc) atomicAdd(&words[ORDER_COUNTS + lane], (unsigned long long)acc);
    if (LDS_ACC) {
        __syncthreads();
        for (uint32_t c = threadIdx.x; c < ORDER_CELLS; c += 256u) {
            const uint32_t cn = acc_lds[c];
            if (cn) { atomicAdd(matrix + c, cn); atomicMax(matrix + ORDER_CELLS + c, acc_lds[ORDER_CELLS + c]); }
        }
    }
}

__global__ __launch_bounds__(1024) void order_extract_kernel(const unsigned long long* __restrict__ seeds, uint32_t n, uint32_t m,
                                                             uint32_t* __restrict__ matrix, unsigned long long* __restrict__ words,
                                                             unsigned long long* __restrict__ entries) {
    __shared__ uint32_t wave_n[16];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6, a = t >> 5, b = t & 31;
    uint32_t cnt[4], wit[4];
    bool some = false, stale = false;
    for (uint32_t k = 0; k < 4; k++) {
        cnt[k] = matrix[k * 1024u + t]; wit[k] = matrix[ORDER_CELLS + k * 1024u + t];
        matrix[k * 1024u + t] = 0u; matrix[ORDER_CELLS + k * 1024u + t] = 0u;      // clean for the next chunk
        some |= cnt[k] != 0u;
        stale |= cnt[k] ? ~wit[k] >= n : wit[k] != 0u;
    }
    stale |= some && (a >= m || b >= m);
    const unsigned long long mine = __ballot(some);
    if (lane == 0u) wave_n[wave] = (uint32_t)__popcll(mine);
    __syncthreads();
    uint32_t pos = (uint32_t)__popcll(mine & ((1ull << lane) - 1ull)), total = 0;
    for (uint32_t wv = 0; wv < 16u; wv++) { pos += wv < wave ? wave_n[wv] : 0u; total += wave_n[wv]; }
    if (stale) atomicOr(&words[ORDER_ERR], (unsigned long long)MADSIM_K_PROBE_ORDER_ERR_TAG);
    if (t == 0u) words[ORDER_ENTRIES] = total;
    if (some && pos < m * m) {                                                     // (a clean matrix has no more)
        unsigned long long* const p = entries + 9 * (size_t)pos;
        p[0] = stale ? 0ull : (unsigned long long)a | (unsigned long long)b << 32; // {uint32_t a, b}, little-endian
        for (uint32_t k = 0; k < 4; k++) {
            p[1 + k] = stale ? 0ull : cnt[k];
            p[5 + k] = !stale && cnt[k] ? seeds[~wit[k]] : 0ull;
        }
    }
}

// ---- probe spans: the virtual time from a chunk's counted seeds' first `from` to the first `to` behind it, as a distribution ------------------
// Two kernels behind the chunk's trace launch (sim_kernel.h: the records' words).  span_fold_kernel follows order_fold_kernel: one wave per
// row, striding, the row index, the verdict, the length and the loop bounds in scalar registers; rows of uncounted and runner seeds are not
// read.  The visible observations are walked in rounds of 64, one coalesced 8-byte load per lane; the definitions travel by value in the kernel
// arguments (384 bytes).  Per span not yet closed: while i is not placed one wave-wide compare against `from` and a ballot, and in the round
// that places it the compare against `to` is masked to the lanes behind i; from then on every lane.  `placed` and `closed` are scalar masks;
// lane s keeps i and j of span s.  The walk ends once every span is closed or the row ends.  Lane s then loads the two times of span s and has
// its state and duration, written to st / dur for span_witness_kernel.  LDS_ACC: histogram, state counts, n, ~min, max and the two half-sums
// (the statistics kernels' way to an exact sum) are a workgroup accumulator in LDS (about 18 KB) under LDS atomics — lane s touches span s's
// words only, so a wave never collides with itself — flushed once, the non-zero words only, into the chunk's records with atomicAdd /
// atomicMax: sums and maxima from zero commute, so no arrival order shows.  LDS_ACC = false sends the same updates straight to the records:
// the correctness baseline and the other side of the A/B.
// span_witness_kernel: one thread per row, striding; reads the chunk's final min and max and takes, per workgroup in LDS and then globally,
// the maximum of ~seed over the rows whose duration equals them and over the OPEN rows: the smallest seed, whatever the order of arrival.
struct SpanDefs { madsim_span_def_t d[MADSIM_PROBE_SPANS_MAX]; };
constexpr uint32_t SPAN_N = 16, SPAN_MIN = 17, SPAN_MAX = 18, SPAN_LO = 19, SPAN_HI = 20, SPAN_WIT = 21, SPAN_HIST = 24, SPAN_REC = MADSIM_K_SPAN_REC_WORDS;
constexpr uint32_t SPANS_ENTRIES = 0, SPANS_COUNTS = 2, SPAN_UNDEF = 0xffffffffu;
static_assert(SPAN_HIST + MADSIM_STAT_BUCKETS == SPAN_REC && MADSIM_PROBE_SPANS_MAX == 16, "the record");
struct SpanAcc {
    uint32_t hist[MADSIM_PROBE_SPANS_MAX][MADSIM_STAT_BUCKETS];
    uint32_t n_state[MADSIM_PROBE_SPANS_MAX][16];
    uint32_t n[MADSIM_PROBE_SPANS_MAX];
    unsigned long long mn[MADSIM_PROBE_SPANS_MAX], mx[MADSIM_PROBE_SPANS_MAX], lo[MADSIM_PROBE_SPANS_MAX], hi[MADSIM_PROBE_SPANS_MAX];      // mn: the largest ~duration
};

template <bool LDS_ACC>
__global__ __launch_bounds__(256) void span_fold_kernel(const unsigned long long* __restrict__ obs, const unsigned long long* __restrict__ times,
                                                        uint32_t obs_cap, const unsigned long long* __restrict__ obs_len,
                                                        const madsim_result_t* __restrict__ res, uint32_t n, uint32_t include, const SpanDefs defs,
                                                        uint32_t m, uint32_t* __restrict__ st, unsigned long long* __restrict__ dur,
                                                        unsigned long long* __restrict__ recs, unsigned long long* __restrict__ words) {
    __shared__ unsigned long long acc_lds[LDS_ACC ? sizeof(SpanAcc) / 8 : 1];
    SpanAcc& A = *reinterpret_cast<SpanAcc*>(acc_lds);
    const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (LDS_ACC) {
        for (uint32_t c = threadIdx.x; c < sizeof(SpanAcc) / 8; c += 256u) acc_lds[c] = 0ull;
        __syncthreads();
    }
    const uint32_t full = 0xffffu >> (16u - m);                                    // (1 <= m <= 16)
    uint32_t start = 0;                                                            // (scalar) the spans that begin at the start of the run
    for (uint32_t s = 0; s < m; s++) start |= (defs.d[s].flags & MADSIM_SPAN_FROM_START) << s;
    uint32_t acc = 0;                                                              // lane k < 4: counted seeds of verdict k; 4: truncated; 5: runner
    for (uint32_t i = blockIdx.x * 4u + wave; i < n; i += gridDim.x * 4u) {        // (scalar)
        const uint32_t v = reinterpret_cast<const uint32_t*>(res + i)[0];
        if (v >= 4u || !((include >> v) & 1u)) {                                   // a runner verdict or a left-out one: the row is not read
            acc += lane == 5u && v >= 4u;
            if (lane < m) st[(size_t)i * m + lane] = MADSIM_K_SPAN_UNCOUNTED;
            continue;
        }
        const unsigned long long len = obs_len[i];
        const uint32_t vis = len < obs_cap ? (uint32_t)len : obs_cap;
        const unsigned long long* const row = obs + (size_t)i * obs_cap;
        uint32_t fi = SPAN_UNDEF, fj = SPAN_UNDEF;                                 // lane s: i and j of span s
        uint32_t placed = start, closed = 0;                                       // (scalar) the spans whose i / whose j is known
        for (uint32_t k = 0; k * 64u < vis && closed != full; k++) {
            const uint32_t idx = k * 64u + lane;
            const bool have = idx < vis;
            const unsigned long long val = have ? row[idx] : 0ull;
            const unsigned long long valid = __ballot(have);
            for (uint32_t s = 0; s < m; s++) {
                if ((closed >> s) & 1u) continue;                                  // (scalar)
                unsigned long long behind = ~0ull;
                if (!((placed >> s) & 1u)) {
                    const unsigned long long b = __ballot(val == defs.d[s].from) & valid;
                    if (!b) continue;
                    const uint32_t p = (uint32_t)__ffsll((long long)b) - 1u;
                    if (lane == s) fi = k * 64u + p;
                    placed |= 1u << s;
                    behind = p == 63u ? 0ull : ~0ull << (p + 1u);                  // in this round the higher lanes only
                }
                const unsigned long long b2 = __ballot(val == defs.d[s].to) & valid & behind;
                if (b2) {
                    if (lane == s) fj = k * 64u + (uint32_t)__ffsll((long long)b2) - 1u;
                    closed |= 1u << s;
                }
            }
        }
        acc += (lane == v) + (lane == 4u && len > obs_cap);
        if (lane < m) {
            const bool cl = (closed >> lane) & 1u;
            const uint32_t state = !((placed >> lane) & 1u) ? MADSIM_SPAN_ABSENT : cl ? MADSIM_SPAN_CLOSED : len > obs_cap ? MADSIM_SPAN_CUT : MADSIM_SPAN_OPEN;
            unsigned long long d = 0ull;
            if (cl) {
                const unsigned long long* const trow = times + (size_t)i * obs_cap;
                d = trow[fj] - (fi == SPAN_UNDEF ? 0ull : trow[fi]);               // (the start of the run: time 0)
            }
            st[(size_t)i * m + lane] = state;
            dur[(size_t)i * m + lane] = d;
            if (LDS_ACC) {
                atomicAdd(&A.n_state[lane][v * 4u + state], 1u);
                if (cl) {
                    atomicAdd(&A.hist[lane][stat_bucket(d)], 1u);
                    atomicAdd(&A.n[lane], 1u);
                    atomicMax(&A.mn[lane], ~d); atomicMax(&A.mx[lane], d);
                    atomicAdd(&A.lo[lane], d & 0xffffffffull); atomicAdd(&A.hi[lane], d >> 32);
                }
            } else {
                unsigned long long* const r = recs + (size_t)lane * SPAN_REC;
                atomicAdd(r + v * 4u + state, 1ull);
                if (cl) {
                    atomicAdd(r + SPAN_HIST + stat_bucket(d), 1ull);
                    atomicAdd(r + SPAN_N, 1ull);
                    atomicMax(r + SPAN_MIN, ~d); atomicMax(r + SPAN_MAX, d);
                    atomicAdd(r + SPAN_LO, d & 0xffffffffull); atomicAdd(r + SPAN_HI, d >> 32);
                }
            }
        }
    }
    if (lane < 6u && acc) atomicAdd(&words[SPANS_COUNTS + lane], (unsigned long long)acc);
    if (LDS_ACC) {
        __syncthreads();
        for (uint32_t c = threadIdx.x; c < m * MADSIM_STAT_BUCKETS; c += 256u) {
            const uint32_t cn = A.hist[c >> 8][c & 255u];
            if (cn) atomicAdd(recs + (size_t)(c >> 8) * SPAN_REC + SPAN_HIST + (c & 255u), (unsigned long long)cn);
        }
        if (threadIdx.x < m * 16u) {
            const uint32_t cn = A.n_state[threadIdx.x >> 4][threadIdx.x & 15u];
            if (cn) atomicAdd(recs + (size_t)(threadIdx.x >> 4) * SPAN_REC + (threadIdx.x & 15u), (unsigned long long)cn);
        }
        if (threadIdx.x < m && A.n[threadIdx.x]) {
            unsigned long long* const r = recs + (size_t)threadIdx.x * SPAN_REC;
            atomicAdd(r + SPAN_N, (unsigned long long)A.n[threadIdx.x]);
            atomicMax(r + SPAN_MIN, A.mn[threadIdx.x]); atomicMax(r + SPAN_MAX, A.mx[threadIdx.x]);
            atomicAdd(r + SPAN_LO, A.lo[threadIdx.x]); atomicAdd(r + SPAN_HI, A.hi[threadIdx.x]);
        }
    }
}

__global__ __launch_bounds__(256) void span_witness_kernel(const uint32_t* __restrict__ st, const unsigned long long* __restrict__ dur,
                                                           const unsigned long long* __restrict__ seeds, uint32_t n, uint32_t m,
                                                           unsigned long long* __restrict__ recs, unsigned long long* __restrict__ words) {
    __shared__ unsigned long long wit[MADSIM_PROBE_SPANS_MAX][3], ext[MADSIM_PROBE_SPANS_MAX][2];
    if (threadIdx.x < 3u * MADSIM_PROBE_SPANS_MAX) (&wit[0][0])[threadIdx.x] = 0ull;
    if (threadIdx.x < m) { ext[threadIdx.x][0] = ~recs[(size_t)threadIdx.x * SPAN_REC + SPAN_MIN]; ext[threadIdx.x][1] = recs[(size_t)threadIdx.x * SPAN_REC + SPAN_MAX]; }
    __syncthreads();
    for (uint32_t row = blockIdx.x * 256u + threadIdx.x; row < n; row += gridDim.x * 256u) {
        for (uint32_t s = 0; s < m; s++) {
            const uint32_t state = st[(size_t)row * m + s];
            if (state == MADSIM_SPAN_CLOSED) {
                const unsigned long long d = dur[(size_t)row * m + s];
                if (d == ext[s][0]) atomicMax(&wit[s][0], ~seeds[row]);
                if (d == ext[s][1]) atomicMax(&wit[s][1], ~seeds[row]);
            } else if (state == MADSIM_SPAN_OPEN) atomicMax(&wit[s][2], ~seeds[row]);
        }
    }
    __syncthreads();
    if (threadIdx.x < 3u * m) {
        const unsigned long long w = (&wit[0][0])[threadIdx.x];
        if (w) atomicMax(recs + (size_t)(threadIdx.x / 3u) * SPAN_REC + SPAN_WIT + threadIdx.x % 3u, w);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) words[SPANS_ENTRIES] = m;
}

// one kernel per row of variant_table (sim_kernel.h), same macro, same order
#define MADSIM_VARIANT_KERNEL(T_, S_, L_, F_, R_, G_) (const void*)sim_kernel<Variant<T_, S_, L_, F_, R_, G_>>,
static const void* const variant_kernels[] = {MADSIM_FOR_EACH_VARIANT(MADSIM_VARIANT_KERNEL)};
#undef MADSIM_VARIANT_KERNEL
static_assert(sizeof variant_kernels / sizeof *variant_kernels == n_variants, "one kernel per build");

}  // namespace madsim_k

extern "C" int madsim_k_launch_sim(const madsim_k::KParams* P, uint32_t grid, uint32_t lds_bytes, void* stream, int trace) {
    using namespace madsim_k;
    const int i = variant_index(select_variant(*P, trace != 0));
    if (i < 0) return -1;          // select_variant named a build that is not compiled: a bug, never a silent substitute
    void* args[] = {const_cast<KParams*>(P)};      // the by-value KParams, as the <<<>>> stub passes it
    (void)hipLaunchKernel(variant_kernels[i], dim3(grid), dim3(64 * P->waves_per_block), args, lds_bytes, (hipStream_t)stream);
    return 0;
}

extern "C" void madsim_k_launch_summary(const madsim_result_t* out, uint64_t count, uint64_t seed0, unsigned long long* acc, void* stream) {
    uint32_t grid = (uint32_t)((count + 1023) / 1024);     // >= 4 results per thread, <= 256 workgroups (4 atomics each)
    if (grid > 256) grid = 256;
    if (grid == 0) grid = 1;
    hipLaunchKernelGGL(madsim_k::summary_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, out, count, seed0, acc);
}

// Every launcher of a report family below exists twice: the range form (result i is seed seed0 + i) and the _list form (result i is seed
// d_seeds[i], a device pointer to the batch's slice of the list).  One template each, so that the two cannot drift apart.
namespace madsim_k {
template <class Seeds>
static void launch_summary6(const madsim_result_t* out, uint64_t count, Seeds src, unsigned long long* acc6, void* stream) {
    uint32_t grid = (uint32_t)((count + 1023) / 1024);
    if (grid > 256) grid = 256;
    if (grid == 0) grid = 1;
    hipLaunchKernelGGL((summary6_kernel<Seeds>), dim3(grid), dim3(256), 0, (hipStream_t)stream, out, count, src, acc6);
}
}  // namespace madsim_k
extern "C" void madsim_k_launch_summary6(const madsim_result_t* out, uint64_t count, uint64_t seed0, unsigned long long* acc6, void* stream) {
    madsim_k::launch_summary6(out, count, madsim_k::RangeSeeds{seed0}, acc6, stream);
}
extern "C" void madsim_k_launch_summary6_list(const madsim_result_t* out, uint64_t count, const uint64_t* d_seeds, unsigned long long* acc6, void* stream) {
    madsim_k::launch_summary6(out, count, madsim_k::ListSeeds{d_seeds}, acc6, stream);
}

// rep: COLLECT_REP_WORDS words, wave_cnt: MADSIM_K_COLLECT_WAVES words, recs: `cap` records (may be null when cap == 0); all prepared by the
// caller on `stream` (rep words 0 and 4 all-ones, the rest zero)
namespace madsim_k {
template <class Seeds>
static void launch_collect(const madsim_result_t* out, uint64_t count, Seeds src, uint32_t list_runner,
                           unsigned long long* rep, uint32_t* wave_cnt, madsim_failure_t* recs, uint64_t cap, void* stream) {
    static_assert(madsim_k::COLLECT_MAX_WAVES == MADSIM_K_COLLECT_WAVES && madsim_k::COLLECT_REP_WORDS == MADSIM_K_COLLECT_WORDS, "sim_kernel.h");
    static_assert(sizeof(madsim_failure_t) == 56 && sizeof(madsim_result_t) == 48, "record layout");
    uint32_t grid = (uint32_t)((count + 1023) / 1024);     // summary6's grid; every wave a contiguous piece, a multiple of 64 results
    if (grid > 256) grid = 256;
    if (grid == 0) grid = 1;
    const uint64_t waves = 4ull * grid, piece = ((count + waves - 1) / waves + 63) / 64 * 64;
    hipLaunchKernelGGL((collect_count_kernel<Seeds>), dim3(grid), dim3(256), 0, (hipStream_t)stream, out, count, src, piece, list_runner, rep, wave_cnt);
    hipLaunchKernelGGL((collect_write_kernel<Seeds>), dim3(grid), dim3(256), 0, (hipStream_t)stream, out, count, src, piece, list_runner, rep,
                       (const uint32_t*)wave_cnt, recs, cap);
}
}  // namespace madsim_k
extern "C" void madsim_k_launch_collect(const madsim_result_t* out, uint64_t count, uint64_t seed0, uint32_t list_runner,
                                        unsigned long long* rep, uint32_t* wave_cnt, madsim_failure_t* recs, uint64_t cap, void* stream) {
    madsim_k::launch_collect(out, count, madsim_k::RangeSeeds{seed0}, list_runner, rep, wave_cnt, recs, cap, stream);
}
extern "C" void madsim_k_launch_collect_list(const madsim_result_t* out, uint64_t count, const uint64_t* d_seeds, uint32_t list_runner,
                                             unsigned long long* rep, uint32_t* wave_cnt, madsim_failure_t* recs, uint64_t cap, void* stream) {
    madsim_k::launch_collect(out, count, madsim_k::ListSeeds{d_seeds}, list_runner, rep, wave_cnt, recs, cap, stream);
}

// srep: MADSIM_K_STATS_WORDS words, all zero (prepared by the caller on `stream`); cand: MADSIM_K_STATS_CAND_WORDS words of scratch, untouched
// when top_k == 0; count < 2^32 - 1
namespace madsim_k {
template <class Seeds>
static void launch_stats(const madsim_result_t* out, uint64_t count, Seeds src, uint32_t include, uint32_t top_k,
                         unsigned long long* srep, unsigned long long* cand, void* stream) {
    static_assert(MADSIM_K_STATS_WORDS == 17 + MADSIM_STAT_METRICS * MADSIM_STAT_BUCKETS / 2 + MADSIM_STAT_METRICS * MADSIM_STAT_MAX_TOP * 2, "sim_kernel.h");
    static_assert(MADSIM_K_STATS_CAND_WORDS == MADSIM_STAT_METRICS * madsim_k::STAT_WGS * madsim_k::STAT_TOP * 2, "sim_kernel.h");
    static_assert(MADSIM_STAT_BUCKETS == 256 && MADSIM_STAT_METRICS == 4 && MADSIM_STAT_MAX_TOP == 16, "one bucket per thread, one metric per wave");
    uint32_t grid = (uint32_t)((count + 1023) / 1024);     // collect's cut
    if (grid > madsim_k::STAT_WGS) grid = madsim_k::STAT_WGS;
    if (grid == 0) grid = 1;
    const uint64_t waves = 4ull * grid, piece = ((count + waves - 1) / waves + 63) / 64 * 64;
    uint32_t* const ghist = reinterpret_cast<uint32_t*>(srep + 17);
    hipLaunchKernelGGL(madsim_k::stats_fold_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, out, count, piece, include, top_k, srep, ghist, cand);
    if (top_k)
        hipLaunchKernelGGL((stats_top_kernel<Seeds>), dim3(MADSIM_STAT_METRICS), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)cand, grid,
                           top_k, src, srep + 17 + MADSIM_STAT_METRICS * MADSIM_STAT_BUCKETS / 2);
}
}  // namespace madsim_k
extern "C" void madsim_k_launch_stats(const madsim_result_t* out, uint64_t count, uint64_t seed0, uint32_t include, uint32_t top_k,
                                      unsigned long long* srep, unsigned long long* cand, void* stream) {
    madsim_k::launch_stats(out, count, madsim_k::RangeSeeds{seed0}, include, top_k, srep, cand, stream);
}
extern "C" void madsim_k_launch_stats_list(const madsim_result_t* out, uint64_t count, const uint64_t* d_seeds, uint32_t include, uint32_t top_k,
                                           unsigned long long* srep, unsigned long long* cand, void* stream) {
    madsim_k::launch_stats(out, count, madsim_k::ListSeeds{d_seeds}, include, top_k, srep, cand, stream);
}

// table: `slots` zeroed slots; list: `count` words of scratch; grep: MADSIM_K_GROUP_WORDS zeroed words; entries: room for `count` (sim_kernel.h).
// Returns 0, or -1 (nothing launched) for sizes the kernels are not written for.
namespace madsim_k {
template <class Seeds>
static int launch_groups(const madsim_result_t* out, uint64_t count, Seeds src, uint32_t include, uint32_t key_field, uint32_t* table,
                         uint64_t slots, uint32_t* list, unsigned long long* grep, madsim_group_t* entries, void* stream) {
    static_assert(sizeof(madsim_group_t) == 32 && sizeof(uint4) == MADSIM_K_GROUP_SLOT_BYTES && sizeof(madsim_result_t) == 48, "record layout");
    static_assert(MADSIM_K_GROUP_MAX_COUNT == MADSIM_GROUP_MAX_BATCH && MADSIM_GROUP_KEYS == 6, "sim_kernel.h");
    static const uint32_t key_words[MADSIM_GROUP_KEYS] = {5, 4, 2, 1, 3, 0};      // obs_hash, trace_hash, msg_count, clock_ns, rng_calls; steps
    if (count == 0 || count > MADSIM_K_GROUP_MAX_COUNT || key_field >= MADSIM_GROUP_KEYS || include == 0 || (include & ~0xfu)) return -1;
    if ((slots & (slots - 1)) || slots < 2 * count || slots < MADSIM_K_GROUP_MIN_SLOTS || slots > (1ull << 31)) return -1;
    uint32_t grid = (uint32_t)((count + 1023) / 1024);     // collect's cut
    if (grid > 256) grid = 256;
    const uint64_t waves = 4ull * grid, piece = ((count + waves - 1) / waves + 63) / 64 * 64;
    hipLaunchKernelGGL(madsim_k::group_fold_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, out, (uint32_t)count, (uint32_t)piece, include,
                       key_words[key_field], reinterpret_cast<uint4*>(table), (uint32_t)(slots - 1), list, grep);
    uint32_t xgrid = (uint32_t)((count + 255) / 256);      // the extraction pass: as many threads as there can be groups, 64 workgroups at most
    if (xgrid > 64) xgrid = 64;
    hipLaunchKernelGGL((group_extract_kernel<Seeds>), dim3(xgrid), dim3(256), 0, (hipStream_t)stream, out, (uint32_t)count, src, key_words[key_field],
                       reinterpret_cast<uint4*>(table), (uint32_t)(slots - 1), (const uint32_t*)list, grep, entries);
    return 0;
}
}  // namespace madsim_k
extern "C" int madsim_k_launch_groups(const madsim_result_t* out, uint64_t count, uint64_t seed0, uint32_t include, uint32_t key_field, uint32_t* table,
                                      uint64_t slots, uint32_t* list, unsigned long long* grep, madsim_group_t* entries, void* stream) {
    return madsim_k::launch_groups(out, count, madsim_k::RangeSeeds{seed0}, include, key_field, table, slots, list, grep, entries, stream);
}
extern "C" int madsim_k_launch_groups_list(const madsim_result_t* out, uint64_t count, const uint64_t* d_seeds, uint32_t include, uint32_t key_field,
                                           uint32_t* table, uint64_t slots, uint32_t* list, unsigned long long* grep, madsim_group_t* entries,
                                           void* stream) {
    if (!d_seeds) return -1;
    return madsim_k::launch_groups(out, count, madsim_k::ListSeeds{d_seeds}, include, key_field, table, slots, list, grep, entries, stream);
}

// words: MADSIM_K_DIFF_WORDS zeroed words; wave_cnt: MADSIM_K_COLLECT_WAVES words; recs: `cap` records (may be null when cap == 0); all prepared by
// the caller on `stream` (sim_kernel.h).  Returns 0, or -1 (nothing launched) for arguments the kernels are not written for.
namespace madsim_k {
template <class Seeds>
static int launch_diff(const madsim_result_t* a, const madsim_result_t* b, uint64_t count, Seeds src, uint32_t fields,
                       unsigned long long* words, uint32_t* wave_cnt, madsim_diff_record_t* recs, uint64_t cap, void* stream) {
    static_assert(sizeof(madsim_diff_record_t) == 104 && sizeof(madsim_result_t) == 48, "record layout");
    static_assert(MADSIM_K_DIFF_WORDS == 2 + 8 + 64 && MADSIM_DIFF_FIELDS == 7 && MADSIM_DIFF_ALL == (1u << MADSIM_DIFF_FIELDS) - 1, "sim_kernel.h");
    if (count == 0 || count >= (1ull << 32) || fields == 0 || (fields & ~MADSIM_DIFF_ALL) || (cap && !recs)) return -1;
    uint32_t grid = (uint32_t)((count + 1023) / 1024);     // collect's cut
    if (grid > 256) grid = 256;
    const uint64_t waves = 4ull * grid, piece = ((count + waves - 1) / waves + 63) / 64 * 64;
    hipLaunchKernelGGL(madsim_k::diff_count_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, b, count, piece, fields, words, wave_cnt);
    hipLaunchKernelGGL((diff_write_kernel<Seeds>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a, b, count, src, piece, fields, words,
                       (const uint32_t*)wave_cnt, recs, cap);
    return 0;
}
}  // namespace madsim_k
extern "C" int madsim_k_launch_diff(const madsim_result_t* a, const madsim_result_t* b, uint64_t count, uint64_t seed0, uint32_t fields,
                                    unsigned long long* words, uint32_t* wave_cnt, madsim_diff_record_t* recs, uint64_t cap, void* stream) {
    return madsim_k::launch_diff(a, b, count, madsim_k::RangeSeeds{seed0}, fields, words, wave_cnt, recs, cap, stream);
}
extern "C" int madsim_k_launch_diff_list(const madsim_result_t* a, const madsim_result_t* b, uint64_t count, const uint64_t* d_seeds, uint32_t fields,
                                         unsigned long long* words, uint32_t* wave_cnt, madsim_diff_record_t* recs, uint64_t cap, void* stream) {
    if (!d_seeds) return -1;
    return madsim_k::launch_diff(a, b, count, madsim_k::ListSeeds{d_seeds}, fields, words, wave_cnt, recs, cap, stream);
}

// words: MADSIM_K_PAIRED_WORDS zeroed words; cand: MADSIM_K_PAIRED_CAND_WORDS words of scratch, untouched (and may be null) when top_k == 0;
// all prepared by the caller on `stream` (sim_kernel.h).  Returns 0, or -1 (nothing launched) for arguments the kernels are not written for.
namespace madsim_k {
template <class Seeds>
static int launch_paired(const madsim_result_t* a, const madsim_result_t* b, uint64_t count, Seeds src, uint32_t include_a, uint32_t include_b,
                         uint32_t top_k, unsigned long long* words, unsigned long long* cand, void* stream) {
    static_assert(sizeof(madsim_paired_extreme_t) == 24 && sizeof(madsim_result_t) == 48, "record layout");
    static_assert(MADSIM_K_PAIRED_HEAD_WORDS == madsim_k::PAIRED_HEAD && madsim_k::PAIRED_SETS == 8, "sim_kernel.h");
    static_assert(MADSIM_K_PAIRED_WORDS == madsim_k::PAIRED_HEAD + madsim_k::PAIRED_SETS * MADSIM_STAT_BUCKETS / 2 + madsim_k::PAIRED_SETS * MADSIM_STAT_MAX_TOP * 3,
                  "sim_kernel.h");
    static_assert(MADSIM_K_PAIRED_CAND_WORDS == madsim_k::PAIRED_SETS * madsim_k::STAT_WGS * madsim_k::STAT_TOP * 2, "sim_kernel.h");
    static_assert(MADSIM_PAIRED_UP == 0 && MADSIM_PAIRED_DOWN == 1 && MADSIM_STAT_BUCKETS == 256 && MADSIM_STAT_MAX_TOP == 16, "one bucket per thread, set = 2 * metric + direction");
    if (!a || !b || !words || count == 0 || count >= (1ull << 32)) return -1;
    if (include_a == 0 || (include_a & ~0xfu) || include_b == 0 || (include_b & ~0xfu) || top_k > MADSIM_STAT_MAX_TOP || (top_k && !cand)) return -1;
    uint32_t grid = (uint32_t)((count + 1023) / 1024);     // collect's cut
    if (grid > madsim_k::STAT_WGS) grid = madsim_k::STAT_WGS;
    const uint64_t waves = 4ull * grid, piece = ((count + waves - 1) / waves + 63) / 64 * 64;
    uint32_t* const ghist = reinterpret_cast<uint32_t*>(words + madsim_k::PAIRED_HEAD);
    hipLaunchKernelGGL(madsim_k::paired_fold_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, b, count, piece, include_a, include_b, top_k, words,
                       ghist, cand);
    if (top_k)
        hipLaunchKernelGGL((paired_top_kernel<Seeds>), dim3(madsim_k::PAIRED_SETS), dim3(256), 0, (hipStream_t)stream, a, b, (const unsigned long long*)cand, grid,
                           top_k, src, words + madsim_k::PAIRED_HEAD + madsim_k::PAIRED_SETS * MADSIM_STAT_BUCKETS / 2);
    return 0;
}
}  // namespace madsim_k
extern "C" int madsim_k_launch_paired(const madsim_result_t* a, const madsim_result_t* b, uint64_t count, uint64_t seed0, uint32_t include_a,
                                      uint32_t include_b, uint32_t top_k, unsigned long long* words, unsigned long long* cand, void* stream) {
    return madsim_k::launch_paired(a, b, count, madsim_k::RangeSeeds{seed0}, include_a, include_b, top_k, words, cand, stream);
}
extern "C" int madsim_k_launch_paired_list(const madsim_result_t* a, const madsim_result_t* b, uint64_t count, const uint64_t* d_seeds, uint32_t include_a,
                                           uint32_t include_b, uint32_t top_k, unsigned long long* words, unsigned long long* cand, void* stream) {
    if (!d_seeds) return -1;
    return madsim_k::launch_paired(a, b, count, madsim_k::ListSeeds{d_seeds}, include_a, include_b, top_k, words, cand, stream);
}

// sides: the n_variants result arrays of the same `count` seeds; words: MADSIM_K_SWEEP_WORDS zeroed words; wave_cnt: MADSIM_K_COLLECT_WAVES
// words; recs: `cap` records (may be null when cap == 0); all prepared by the caller on `stream` (sim_kernel.h).  Returns 0, or -1 (nothing
// launched) for arguments the kernels are not written for.
namespace madsim_k {
template <class Seeds>
static int launch_sweep(const madsim_result_t* const* sides, uint32_t n_variants, uint64_t count, Seeds src, uint32_t fields, uint32_t rule,
                        unsigned long long* words, uint32_t* wave_cnt, madsim_sweep_record_t* recs, uint64_t cap, void* stream) {
    static_assert(sizeof(madsim_sweep_record_t) == 24 && sizeof(madsim_result_t) == 48 && MADSIM_SWEEP_MAX_VARIANTS == 8, "record layout");
    static_assert(MADSIM_K_SWEEP_WORDS == 2 + 8 + 8 + 256, "sim_kernel.h");
    if (!sides || n_variants < 2 || n_variants > MADSIM_SWEEP_MAX_VARIANTS || count == 0 || count >= (1ull << 32)) return -1;
    if ((fields & ~MADSIM_DIFF_ALL) || rule > MADSIM_SWEEP_LIST_DIFFERING || (rule == MADSIM_SWEEP_LIST_DIFFERING && !fields) || (cap && !recs)) return -1;
    SweepSides S{};
    for (uint32_t v = 0; v < n_variants; v++) {
        if (!sides[v]) return -1;
        S.r[v] = sides[v];
    }
    uint32_t grid = (uint32_t)((count + 1023) / 1024);     // collect's cut
    if (grid > 256) grid = 256;
    const uint64_t waves = 4ull * grid, piece = ((count + waves - 1) / waves + 63) / 64 * 64;
    hipLaunchKernelGGL(madsim_k::sweep_count_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, S, n_variants, count, piece, fields, rule, words, wave_cnt);
    hipLaunchKernelGGL((sweep_write_kernel<Seeds>), dim3(grid), dim3(256), 0, (hipStream_t)stream, S, n_variants, count, src, piece, fields, rule, words,
                       (const uint32_t*)wave_cnt, recs, cap);
    return 0;
}
}  // namespace madsim_k
extern "C" int madsim_k_launch_sweep(const madsim_result_t* const* sides, uint32_t n_variants, uint64_t count, uint64_t seed0, uint32_t fields,
                                     uint32_t rule, unsigned long long* words, uint32_t* wave_cnt, madsim_sweep_record_t* recs, uint64_t cap, void* stream) {
    return madsim_k::launch_sweep(sides, n_variants, count, madsim_k::RangeSeeds{seed0}, fields, rule, words, wave_cnt, recs, cap, stream);
}
extern "C" int madsim_k_launch_sweep_list(const madsim_result_t* const* sides, uint32_t n_variants, uint64_t count, const uint64_t* d_seeds, uint32_t fields,
                                          uint32_t rule, unsigned long long* words, uint32_t* wave_cnt, madsim_sweep_record_t* recs, uint64_t cap,
                                          void* stream) {
    if (!d_seeds) return -1;
    return madsim_k::launch_sweep(sides, n_variants, count, madsim_k::ListSeeds{d_seeds}, fields, rule, words, wave_cnt, recs, cap, stream);
}

// wave_cnt: MADSIM_K_RESOLVE_WAVES words of scratch; total: one word; seeds / idx: room for `count` entries each, the first *total written
// (sim_kernel.h).  Returns 0, or -1 (nothing launched) for count == 0 or count >= 2^32.
namespace madsim_k {
template <class Seeds>
static int launch_resolve_list(const madsim_result_t* out, uint64_t count, Seeds src, uint32_t steps_maxed, uint32_t* wave_cnt,
                               uint32_t* total, uint64_t* seeds, uint32_t* idx, void* stream) {
    static_assert(madsim_k::COLLECT_MAX_WAVES == MADSIM_K_RESOLVE_WAVES && sizeof(madsim_result_t) == 48, "sim_kernel.h");
    if (count == 0 || count >= (1ull << 32)) return -1;
    uint32_t grid = (uint32_t)((count + 1023) / 1024);     // collect's cut
    if (grid > 256) grid = 256;
    const uint64_t waves = 4ull * grid, piece = ((count + waves - 1) / waves + 63) / 64 * 64;
    hipLaunchKernelGGL(madsim_k::resolve_count_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, out, count, piece, steps_maxed ? 1u : 0u, wave_cnt);
    hipLaunchKernelGGL((resolve_write_kernel<Seeds>), dim3(grid), dim3(256), 0, (hipStream_t)stream, out, count, src, piece, steps_maxed ? 1u : 0u,
                       (const uint32_t*)wave_cnt, (uint32_t)waves, total, seeds, idx);
    return 0;
}
}  // namespace madsim_k
extern "C" int madsim_k_launch_resolve_list(const madsim_result_t* out, uint64_t count, uint64_t seed0, uint32_t steps_maxed, uint32_t* wave_cnt,
                                            uint32_t* total, uint64_t* seeds, uint32_t* idx, void* stream) {
    return madsim_k::launch_resolve_list(out, count, madsim_k::RangeSeeds{seed0}, steps_maxed, wave_cnt, total, seeds, idx, stream);
}
// d_seeds: the batch's slice of a seed list, `count` entries; it must not overlap `seeds`, which receives d_seeds[i] of the re-runnable results
extern "C" int madsim_k_launch_resolve_list_list(const madsim_result_t* out, uint64_t count, const uint64_t* d_seeds, uint32_t steps_maxed,
                                                 uint32_t* wave_cnt, uint32_t* total, uint64_t* seeds, uint32_t* idx, void* stream) {
    if (!d_seeds) return -1;
    return madsim_k::launch_resolve_list(out, count, madsim_k::ListSeeds{d_seeds}, steps_maxed, wave_cnt, total, seeds, idx, stream);
}

// out: the batch's results; rerun: m results; idx: m distinct indices into `out`.  m == 0 launches nothing.  Returns 0, or -1 (nothing
// launched) for m >= 2^32 / 3.
extern "C" int madsim_k_launch_resolve_scatter(madsim_result_t* out, const madsim_result_t* rerun, const uint32_t* idx, uint64_t m, void* stream) {
    static_assert(MADSIM_K_RESOLVE_CHUNKS * sizeof(uint4) == sizeof(madsim_result_t), "three 16-byte chunks per record");
    if (m >= (1ull << 32) / MADSIM_K_RESOLVE_CHUNKS) return -1;
    if (m == 0) return 0;
    const uint32_t grid = (uint32_t)((MADSIM_K_RESOLVE_CHUNKS * m + 255) / 256);
    hipLaunchKernelGGL(madsim_k::resolve_scatter_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, out, rerun, idx, (uint32_t)m);
    return 0;
}

// Rows, lengths, results and seeds of the same n seeds on both sides (sim_kernel.h); recs: n records; ctx: n rows of 3 * win words (null
// when win == 0).  Nothing needs preparing: every record and context word is written.  Returns 0, or -1 (nothing launched) for n == 0,
// n >= 2^32, win > MADSIM_DIVERGE_MAX_WIN, a missing array, a row array that is not 16-byte aligned or rows beyond 2^62 bytes.
extern "C" int madsim_k_launch_diverge(const uint8_t* log_a, const uint8_t* log_b, uint64_t log_cap, const uint64_t* obs_a, const uint64_t* obs_b,
                                       uint64_t obs_cap, const uint64_t* log_len_a, const uint64_t* log_len_b, const uint64_t* obs_len_a,
                                       const uint64_t* obs_len_b, const madsim_result_t* res_a, const madsim_result_t* res_b, const uint64_t* d_seeds,
                                       uint64_t n, uint32_t win, madsim_divergence_t* recs, uint64_t* ctx, void* stream) {
    static_assert(sizeof(madsim_divergence_t) == 184 && sizeof(madsim_result_t) == 48 && MADSIM_K_DIVERGE_WAVES == 1024, "record layout");
    static_assert(MADSIM_DIVERGE_MAX_WIN == 8, "one context word per lane");
    if (n == 0 || n >= (1ull << 32) || win > MADSIM_DIVERGE_MAX_WIN || (win != 0) != (ctx != nullptr)) return -1;
    if (!log_len_a || !log_len_b || !obs_len_a || !obs_len_b || !res_a || !res_b || !d_seeds || !recs) return -1;
    if ((log_cap && (!log_a || !log_b)) || (obs_cap && (!obs_a || !obs_b))) return -1;
    if (((uintptr_t)log_a | (uintptr_t)log_b | (uintptr_t)obs_a | (uintptr_t)obs_b) & 15u) return -1;
    if (log_cap > (1ull << 62) / n || obs_cap > (1ull << 59) / n) return -1;
    const uint64_t waves = n < MADSIM_K_DIVERGE_WAVES ? n : MADSIM_K_DIVERGE_WAVES;      // one wave per row pair, 256 workgroups at most
    hipLaunchKernelGGL(madsim_k::diverge_kernel, dim3((uint32_t)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, log_a, log_b, log_cap,
                       (const unsigned long long*)obs_a, (const unsigned long long*)obs_b, obs_cap, (const unsigned long long*)log_len_a,
                       (const unsigned long long*)log_len_b, (const unsigned long long*)obs_len_a, (const unsigned long long*)obs_len_b, res_a, res_b,
                       (const unsigned long long*)d_seeds, n, win, reinterpret_cast<unsigned long long*>(recs), (unsigned long long*)ctx);
    return 0;
}

// Rows, lengths, results and seeds of the chunk's n seeds; table: `slots` zeroed slots; list: `cap` words of scratch; words:
// MADSIM_K_CENSUS_WORDS zeroed words; entries: room for `cap` (sim_kernel.h).  Returns 0, or -1 (nothing launched) for sizes the kernels
// are not written for.
// `direct` != 0: every row in the direct form, no wave accumulator — the same bytes either way.
extern "C" int madsim_k_launch_census_form(const uint64_t* obs, uint64_t obs_cap, const uint64_t* obs_len, const madsim_result_t* res,
                                           const uint64_t* d_seeds, uint64_t n, uint32_t include, uint32_t* table, uint64_t slots, uint32_t* list,
                                           uint64_t cap, unsigned long long* words, madsim_census_value_t* entries, void* stream, int direct) {
    static_assert(sizeof(madsim_census_value_t) == 64 && 2 * sizeof(uint4) == MADSIM_K_CENSUS_SLOT_BYTES && sizeof(madsim_result_t) == 48, "record layout");
    if (n == 0 || obs_cap == 0 || obs_cap > MADSIM_CENSUS_MAX_OBS_CAP || n >= 0xffffffffull / obs_cap || n > (1ull << 31)) return -1;      // n * obs_cap < 2^32 - 1; the row index plus a grid stride stays 32-bit
    if (include == 0 || (include & ~0xfu) || cap == 0 || cap > MADSIM_CENSUS_MAX_VALUES) return -1;
    if ((slots & (slots - 1)) || slots < 2 * cap || slots < MADSIM_K_CENSUS_MIN_SLOTS || slots > (1ull << 26)) return -1;
    if (!obs || !obs_len || !res || !d_seeds || !table || !list || !words || !entries || ((uintptr_t)table & 15u)) return -1;
    const uint64_t waves = n < MADSIM_K_CENSUS_WAVES ? n : MADSIM_K_CENSUS_WAVES;        // one wave per row, 256 workgroups at most
    const auto fold = direct ? madsim_k::census_fold_kernel<false> : madsim_k::census_fold_kernel<true>;
    hipLaunchKernelGGL(fold, dim3((uint32_t)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned long long*)obs, (uint32_t)obs_cap, (const unsigned long long*)obs_len, res, (uint32_t)n, include, table,
                       (uint32_t)(slots - 1), list, (uint32_t)cap, words);
    uint32_t xgrid = (uint32_t)((cap + 255) / 256);        // the extraction pass: as many threads as there can be values, 64 workgroups at most
    if (xgrid > 64) xgrid = 64;
    hipLaunchKernelGGL(madsim_k::census_extract_kernel, dim3(xgrid), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)obs,
                       (uint32_t)(n * obs_cap), (const unsigned long long*)d_seeds, (uint32_t)n, table, (uint32_t)(slots - 1), (const uint32_t*)list,
                       (uint32_t)cap, words, reinterpret_cast<unsigned long long*>(entries));
    return 0;
}

// The task rows (`task_cap` words each), their true counts and the results of the chunk's n seeds; sites: n rows of task_cap words, shape and
// ones: n words each (sim_kernel.h).  Returns 0, or -1 (nothing launched) for sizes the kernel is not written for.
extern "C" int madsim_k_launch_stall_sites(const uint64_t* tasks, uint64_t task_cap, const uint64_t* task_len, const madsim_result_t* res, uint64_t n,
                                           uint64_t* sites, uint64_t* shape, uint64_t* ones, void* stream) {
    if (n == 0 || task_cap == 0 || task_cap > MADSIM_MAX_LIVE_TASKS || n >= 0xffffffffull / task_cap || n > (1ull << 31)) return -1;
    if (!tasks || !task_len || !res || !sites || !shape || !ones) return -1;
    const uint64_t waves = n < MADSIM_K_CENSUS_WAVES ? n : MADSIM_K_CENSUS_WAVES;        // one wave per row, 256 workgroups at most
    hipLaunchKernelGGL(madsim_k::stall_sites_kernel, dim3((uint32_t)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned long long*)tasks, (uint32_t)task_cap, (const unsigned long long*)task_len, res, (uint32_t)n,
                       (unsigned long long*)sites, (unsigned long long*)shape, (unsigned long long*)ones);
    return 0;
}

// (MADSIM_HIP_CENSUS_DIRECT=1 in the environment: the direct form — a diagnostic / A-B switch, results are the same either way)
extern "C" int madsim_k_launch_census(const uint64_t* obs, uint64_t obs_cap, const uint64_t* obs_len, const madsim_result_t* res, const uint64_t* d_seeds,
                                      uint64_t n, uint32_t include, uint32_t* table, uint64_t slots, uint32_t* list, uint64_t cap,
                                      unsigned long long* words, madsim_census_value_t* entries, void* stream) {
    static const bool direct = [] { const char* e = getenv("MADSIM_HIP_CENSUS_DIRECT"); return e && atoi(e) != 0; }();      // (unset, empty or 0: the accumulator)
    return madsim_k_launch_census_form(obs, obs_cap, obs_len, res, d_seeds, n, include, table, slots, list, cap, words, entries, stream, direct);
}

// Rows, lengths, results and seeds of the chunk's n seeds; vocab: n_vocab values in HOST memory (they travel in the kernel arguments); sig:
// n words of scratch; table: `slots` zeroed slots; list: `cap` words of scratch; words: MADSIM_K_PROBE_SETS_WORDS zeroed words; entries:
// room for `cap` (sim_kernel.h).  Returns 0, or -1 (nothing launched) for sizes the kernels are not written for.
// `per_seed` != 0: one table update per counted seed, no in-wave combine — the same bytes either way.
extern "C" int madsim_k_launch_probe_sets_form(const uint64_t* obs, uint64_t obs_cap, const uint64_t* obs_len, const madsim_result_t* res,
                                               const uint64_t* d_seeds, uint64_t n, uint32_t include, const uint64_t* vocab, uint64_t n_vocab,
                                               uint64_t* sig, uint32_t* table, uint64_t slots, uint32_t* list, uint64_t cap, unsigned long long* words,
                                               madsim_probe_set_t* entries, void* stream, int per_seed) {
    static_assert(sizeof(madsim_probe_set_t) == 72 && 3 * sizeof(uint4) == MADSIM_K_PROBE_SETS_SLOT_BYTES && sizeof(madsim_result_t) == 48, "record layout");
    static_assert(sizeof(madsim_k::SetsVocab) == 496, "the vocabulary in the kernel arguments");
    if (n == 0 || obs_cap == 0 || obs_cap > MADSIM_CENSUS_MAX_OBS_CAP || n >= 0xffffffffull / obs_cap || n > (1ull << 31)) return -1;      // n * obs_cap < 2^32 - 1; the row index plus a grid stride stays 32-bit
    if (include == 0 || (include & ~0xfu) || cap == 0 || cap > MADSIM_PROBE_SETS_MAX || n_vocab == 0 || n_vocab > MADSIM_PROBE_SETS_MAX_VOCAB) return -1;
    if ((slots & (slots - 1)) || slots < 2 * cap || slots < MADSIM_K_PROBE_SETS_MIN_SLOTS || slots > (1ull << 26)) return -1;
    if (!obs || !obs_len || !res || !d_seeds || !vocab || !sig || !table || !list || !words || !entries || ((uintptr_t)table & 15u)) return -1;
    madsim_k::SetsVocab V{};
    for (uint64_t j = 0; j < n_vocab; j++) V.v[j] = vocab[j];
    const uint64_t waves = n < MADSIM_K_PROBE_SETS_WAVES ? n : MADSIM_K_PROBE_SETS_WAVES;      // one wave per row, 256 workgroups at most
    hipLaunchKernelGGL(madsim_k::sets_mask_kernel, dim3((uint32_t)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)obs,
                       (uint32_t)obs_cap, (const unsigned long long*)obs_len, res, (uint32_t)n, include, V, (uint32_t)n_vocab, (unsigned long long*)sig);
    const uint64_t rounds = (n + 63) / 64, fwaves = rounds < MADSIM_K_PROBE_SETS_WAVES ? rounds : MADSIM_K_PROBE_SETS_WAVES;      // one lane per seed
    const auto fold = per_seed ? madsim_k::sets_fold_kernel<false> : madsim_k::sets_fold_kernel<true>;
    hipLaunchKernelGGL(fold, dim3((uint32_t)((fwaves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)sig, res, (uint32_t)n,
                       include, table, (uint32_t)(slots - 1), list, (uint32_t)cap, words);
    uint32_t xgrid = (uint32_t)((cap + 255) / 256);        // the extraction pass: as many threads as there can be sets, 64 workgroups at most
    if (xgrid > 64) xgrid = 64;
    hipLaunchKernelGGL(madsim_k::sets_extract_kernel, dim3(xgrid), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)sig,
                       (const unsigned long long*)d_seeds, (uint32_t)n, table, (uint32_t)(slots - 1), (const uint32_t*)list, (uint32_t)cap, words,
                       reinterpret_cast<unsigned long long*>(entries));
    return 0;
}

extern "C" int madsim_k_launch_probe_sets(const uint64_t* obs, uint64_t obs_cap, const uint64_t* obs_len, const madsim_result_t* res,
                                          const uint64_t* d_seeds, uint64_t n, uint32_t include, const uint64_t* vocab, uint64_t n_vocab, uint64_t* sig,
                                          uint32_t* table, uint64_t slots, uint32_t* list, uint64_t cap, unsigned long long* words,
                                          madsim_probe_set_t* entries, void* stream) {
    return madsim_k_launch_probe_sets_form(obs, obs_cap, obs_len, res, d_seeds, n, include, vocab, n_vocab, sig, table, slots, list, cap, words, entries,
                                           stream, 0);
}

// Rows, lengths, results and seeds of the chunk's n seeds; vocab: n_vocab values in HOST memory (they travel in the kernel arguments);
// matrix: MADSIM_K_PROBE_ORDER_MATRIX_WORDS zeroed words; words: MADSIM_K_PROBE_ORDER_WORDS zeroed words; entries: room for
// n_vocab * n_vocab (sim_kernel.h).  Returns 0, or -1 (nothing launched) for sizes the kernels are not written for.
// `direct` != 0: every update straight to the global matrix, no workgroup accumulator — the same bytes either way.
extern "C" int madsim_k_launch_probe_order_form(const uint64_t* obs, uint64_t obs_cap, const uint64_t* obs_len, const madsim_result_t* res,
                                                const uint64_t* d_seeds, uint64_t n, uint32_t include, const uint64_t* vocab, uint64_t n_vocab,
                                                uint32_t* matrix, unsigned long long* words, madsim_probe_order_pair_t* entries, void* stream,
                                                int direct) {
    static_assert(sizeof(madsim_probe_order_pair_t) == 72 && sizeof(madsim_result_t) == 48, "record layout");
    static_assert(sizeof(madsim_k::OrderVocab) == 256, "the vocabulary in the kernel arguments");
    if (n == 0 || obs_cap == 0 || obs_cap > MADSIM_CENSUS_MAX_OBS_CAP || n >= 0xffffffffull / obs_cap || n > (1ull << 31)) return -1;      // n * obs_cap < 2^32 - 1; the row index plus a grid stride stays 32-bit
    if (include == 0 || (include & ~0xfu) || n_vocab == 0 || n_vocab > MADSIM_PROBE_ORDER_MAX_VOCAB) return -1;
    if (!obs || !obs_len || !res || !d_seeds || !vocab || !matrix || !words || !entries || ((uintptr_t)matrix & 3u) || ((uintptr_t)entries & 7u)) return -1;
    madsim_k::OrderVocab V{};
    for (uint64_t j = 0; j < n_vocab; j++) V.v[j] = vocab[j];
    const uint64_t waves = n < MADSIM_K_PROBE_ORDER_WAVES ? n : MADSIM_K_PROBE_ORDER_WAVES;      // one wave per row, 256 workgroups at most
    const auto fold = direct ? madsim_k::order_fold_kernel<false> : madsim_k::order_fold_kernel<true>;
    hipLaunchKernelGGL(fold, dim3((uint32_t)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)obs, (uint32_t)obs_cap,
                       (const unsigned long long*)obs_len, res, (uint32_t)n, include, V, (uint32_t)n_vocab, matrix, words);
    hipLaunchKernelGGL(madsim_k::order_extract_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const unsigned long long*)d_seeds, (uint32_t)n,
                       (uint32_t)n_vocab, matrix, words, reinterpret_cast<unsigned long long*>(entries));
    return 0;
}

extern "C" int madsim_k_launch_probe_order(const uint64_t* obs, uint64_t obs_cap, const uint64_t* obs_len, const madsim_result_t* res,
                                           const uint64_t* d_seeds, uint64_t n, uint32_t include, const uint64_t* vocab, uint64_t n_vocab,
                                           uint32_t* matrix, unsigned long long* words, madsim_probe_order_pair_t* entries, void* stream) {
    return madsim_k_launch_probe_order_form(obs, obs_cap, obs_len, res, d_seeds, n, include, vocab, n_vocab, matrix, words, entries, stream, 0);
}

// Rows, time rows, lengths, results and seeds of the chunk's n seeds; defs: n_spans definitions in HOST memory (they travel in the kernel
// arguments); st / dur: n * n_spans words each; recs: n_spans records, zeroed here; words: MADSIM_K_PROBE_SPANS_WORDS zeroed words
// (sim_kernel.h).  Returns 0, or -1 (nothing launched) for sizes the kernels are not written for.
extern "C" int madsim_k_launch_probe_spans_form(const uint64_t* obs, const uint64_t* times, uint64_t obs_cap, const uint64_t* obs_len,
                                                const madsim_result_t* res, const uint64_t* d_seeds, uint64_t n, uint32_t include,
                                                const madsim_span_def_t* defs, uint64_t n_spans, uint32_t* st, unsigned long long* dur,
                                                madsim_k_span_rec_t* recs, unsigned long long* words, void* stream, int direct) {
    static_assert(sizeof(madsim_span_t) == 8 * MADSIM_K_SPAN_REC_WORDS && sizeof(madsim_k_span_rec_t) == sizeof(madsim_span_t) && sizeof(madsim_result_t) == 48, "record layout");
    static_assert(sizeof(madsim_k::SpanDefs) == 384 && sizeof(madsim_k::SpanAcc) % 8 == 0 && sizeof(madsim_k::SpanAcc) < 20480, "the definitions in the kernel arguments; the accumulator");
    if (n == 0 || obs_cap == 0 || obs_cap > MADSIM_CENSUS_MAX_OBS_CAP || n >= 0xffffffffull / obs_cap || n > (1ull << 31)) return -1;      // n * obs_cap < 2^32 - 1; the row index plus a grid stride stays 32-bit
    if (include == 0 || (include & ~0xfu) || n_spans == 0 || n_spans > MADSIM_PROBE_SPANS_MAX) return -1;
    if (!obs || !times || !obs_len || !res || !d_seeds || !defs || !st || !dur || !recs || !words || ((uintptr_t)st & 3u) || ((uintptr_t)dur & 7u) || ((uintptr_t)recs & 7u)) return -1;
    madsim_k::SpanDefs D{};
    for (uint64_t s = 0; s < n_spans; s++) {
        if (defs[s].flags & ~MADSIM_SPAN_FROM_START) return -1;
        D.d[s].from = defs[s].from; D.d[s].to = defs[s].to; D.d[s].flags = defs[s].flags;
    }
    if (hipMemsetAsync(recs, 0, n_spans * sizeof(madsim_k_span_rec_t), (hipStream_t)stream) != hipSuccess) return -1;
    const uint64_t waves = n < MADSIM_K_PROBE_ORDER_WAVES ? n : MADSIM_K_PROBE_ORDER_WAVES;      // one wave per row, 256 workgroups at most
    const auto fold = direct ? madsim_k::span_fold_kernel<false> : madsim_k::span_fold_kernel<true>;
    hipLaunchKernelGGL(fold, dim3((uint32_t)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)obs,
                       (const unsigned long long*)times, (uint32_t)obs_cap, (const unsigned long long*)obs_len, res, (uint32_t)n, include, D,
                       (uint32_t)n_spans, st, dur, reinterpret_cast<unsigned long long*>(recs), words);
    const uint64_t wgs = (n + 255) / 256 < 256 ? (n + 255) / 256 : 256;
    hipLaunchKernelGGL(madsim_k::span_witness_kernel, dim3((uint32_t)wgs), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)st,
                       (const unsigned long long*)dur, (const unsigned long long*)d_seeds, (uint32_t)n, (uint32_t)n_spans,
                       reinterpret_cast<unsigned long long*>(recs), words);
    return 0;
}

extern "C" int madsim_k_launch_probe_spans(const uint64_t* obs, const uint64_t* times, uint64_t obs_cap, const uint64_t* obs_len,
                                           const madsim_result_t* res, const uint64_t* d_seeds, uint64_t n, uint32_t include,
                                           const madsim_span_def_t* defs, uint64_t n_spans, uint32_t* st, unsigned long long* dur,
                                           madsim_k_span_rec_t* recs, unsigned long long* words, void* stream) {
    return madsim_k_launch_probe_spans_form(obs, times, obs_cap, obs_len, res, d_seeds, n, include, defs, n_spans, st, dur, recs, words, stream, 0);
}

extern "C" void madsim_k_launch_keyflip(unsigned long long* acc, void* stream) {
    hipLaunchKernelGGL(madsim_k::keyflip_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, acc);
}

// VGPRs per lane of the build select_variant names (0 = not compiled / error): the host sizes waves per CU with it.
extern "C" int madsim_k_variant_vgprs(const madsim_k::VariantSel* v) {
    using namespace madsim_k;
    const int i = variant_index(*v);
    hipFuncAttributes a;
    return i >= 0 && hipFuncGetAttributes(&a, variant_kernels[i]) == hipSuccess ? a.numRegs : 0;
}

extern "C" int madsim_k_set_max_lds(uint32_t lds_bytes) {
    hipError_t e = hipSuccess;
    for (const void* k : madsim_k::variant_kernels)
        if (e == hipSuccess) e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    return (int)e;
}
