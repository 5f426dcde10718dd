// tools/fold_obs_reports_check.cpp — madsim_k_fold_census, madsim_k_fold_probe_sets and madsim_k_fold_probe_order (the host folds of the
// observation census, the probe-set census and the probe-order census: one merge routine in madsim_hip.cpp under three forms) in a stand-alone program, meant to be built with AddressSanitizer
// and UndefinedBehaviorSanitizer on the host side.  No device is touched: the folds are plain host code.  For each fold, random chunks of
// entries (equal keys inside a chunk, keys shared between chunks, the keys 0 and 2^64 - 1) are folded into a table sized EXACTLY to the
// number of distinct keys — every write at the table's last element is inside it — and held against a std::map; then once more into a
// table one entry short, where the fold that would pass the cap must return -1 and leave the table and the totals as they were.
//
//   cd madsim_amd/csrc && make
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -x hip -Xarch_host -fsanitize=address,undefined -c madsim_hip.cpp -o /tmp/madsim_hip_san.o
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -c ../../tools/fold_obs_reports_check.cpp -o /tmp/fold_obs_reports_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/fold_obs_reports_check.o /tmp/madsim_hip_san.o sim_kernel.o
//         (continued) -o /tmp/fold_obs_reports_check && /tmp/fold_obs_reports_check
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "../include/madsim_hip.h"

// (csrc/sim_kernel.h, which needs the HIP headers, declares these)
extern "C" int madsim_k_fold_census(madsim_census_t* cen, const unsigned long long* words, const madsim_census_value_t* entries, uint64_t n);
extern "C" int madsim_k_fold_probe_sets(madsim_probe_sets_t* ps, const unsigned long long* words, const madsim_probe_set_t* entries, uint64_t n);
extern "C" int madsim_k_fold_probe_order(madsim_probe_order_t* po, const unsigned long long* words, const madsim_probe_order_pair_t* entries, uint64_t n);

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }

// What the scheme below asks of a fold: its report and entry types, the words of a chunk (MADSIM_K_*_WORDS), the fold itself, the report's
// array and count, a random entry under a key with the model's rule for combining it (written here from include/madsim_hip.h, not from the
// library), random totals in a chunk's words and the rule that adds them to a report.
struct CensusFold {
    typedef madsim_census_t Report;
    typedef madsim_census_value_t Entry;
    static constexpr const char* name = "madsim_k_fold_census";
    static constexpr size_t words = 16;
    static int fold(Report* r, const unsigned long long* w, const Entry* e, uint64_t n) { return madsim_k_fold_census(r, w, e, n); }
    static void table(Report& r, Entry* t) { r.values = t; }
    static uint64_t& count(Report& r) { return r.n_values; }
    static uint64_t key(const Entry& e) { return e.value; }
    static Entry entry(uint64_t key) {
        Entry x{};
        x.value = key;
        for (int k = 0; k < 4; k++) x.n_seeds[k] = rnd() % 3 ? 1 + rnd() % 1000 : 0;
        x.n_total = rnd() % 100000; x.first_seed = rnd() % 5 ? rnd() : 0; x.max_per_seed = rnd() % 300;      // (seed 0 is a seed like any other)
        return x;
    }
    static void combine(Entry& a, const Entry& b) {                // the smallest seed and the largest count, whatever the counts
        for (int k = 0; k < 4; k++) a.n_seeds[k] += b.n_seeds[k];
        a.n_total += b.n_total; a.first_seed = std::min(a.first_seed, b.first_seed); a.max_per_seed = std::max(a.max_per_seed, b.max_per_seed);
    }
    static void totals(unsigned long long* w) { for (int i = 2; i <= 12; i++) w[i] = rnd() % 1000; }
    static void add(Report& r, const unsigned long long* w) {
        for (int k = 0; k < 4; k++) { r.n_counted[k] += w[2 + k]; r.n_silent[k] += w[6 + k]; }
        r.n_truncated += w[10]; r.n_observations += w[11]; r.n_runner += w[12];
    }
};

struct ProbeSetsFold {
    typedef madsim_probe_sets_t Report;
    typedef madsim_probe_set_t Entry;
    static constexpr const char* name = "madsim_k_fold_probe_sets";
    static constexpr size_t words = 8;
    static int fold(Report* r, const unsigned long long* w, const Entry* e, uint64_t n) { return madsim_k_fold_probe_sets(r, w, e, n); }
    static void table(Report& r, Entry* t) { r.sets = t; }
    static uint64_t& count(Report& r) { return r.n_sets; }
    static uint64_t key(const Entry& e) { return e.set; }
    static Entry entry(uint64_t key) {
        Entry x{};
        x.set = key;
        for (int k = 0; k < 4; k++) {
            if (rnd() % 3 == 0) continue;
            x.n_seeds[k] = 1 + rnd() % 1000;
            x.first_seed[k] = rnd() % 5 ? rnd() : 0;                               // (seed 0 is a seed like any other)
        }
        return x;
    }
    template <class E>
    static void combine_seeds(E& a, const E& b) {                  // per verdict the smallest seed of the sides that have seeds; 0 where neither has
        for (int k = 0; k < 4; k++) {
            if (b.n_seeds[k]) a.first_seed[k] = a.n_seeds[k] ? std::min(a.first_seed[k], b.first_seed[k]) : b.first_seed[k];
            a.n_seeds[k] += b.n_seeds[k];
        }
    }
    static void combine(Entry& a, const Entry& b) { combine_seeds(a, b); }
    static void totals(unsigned long long* w) { for (int i = 2; i <= 6; i++) w[i] = rnd() % 1000; }
    static void add(Report& r, const unsigned long long* w) {
        for (int k = 0; k < 4; k++) r.n_counted[k] += w[2 + k];
        r.n_runner += w[6];
    }
};

struct ProbeOrderFold {
    typedef madsim_probe_order_t Report;
    typedef madsim_probe_order_pair_t Entry;
    static constexpr const char* name = "madsim_k_fold_probe_order";
    static constexpr size_t words = 12;
    static int fold(Report* r, const unsigned long long* w, const Entry* e, uint64_t n) { return madsim_k_fold_probe_order(r, w, e, n); }
    static void table(Report& r, Entry* t) { r.pairs = t; }
    static uint64_t& count(Report& r) { return r.n_pairs; }
    static uint64_t key(const Entry& e) { return (uint64_t)e.a << 32 | e.b; }      // ascending by (a, b)
    static Entry entry(uint64_t key) {
        Entry x{};
        x.a = (uint32_t)(key >> 32); x.b = (uint32_t)key;
        for (int k = 0; k < 4; k++) {
            if (rnd() % 3 == 0) continue;
            x.n_seeds[k] = 1 + rnd() % 1000;
            x.first_seed[k] = rnd() % 5 ? rnd() : 0;                               // (seed 0 is a seed like any other)
        }
        return x;
    }
    static void combine(Entry& a, const Entry& b) { ProbeSetsFold::combine_seeds(a, b); }
    static void totals(unsigned long long* w) { for (int i = 2; i <= 11; i++) w[i] = rnd() % 1000; }
    static void add(Report& r, const unsigned long long* w) {
        for (int k = 0; k < 4; k++) { r.n_counted[k] += w[2 + k]; r.n_none[k] += w[6 + k]; }
        r.n_truncated += w[10]; r.n_runner += w[11];
    }
};

template <class F>
static int check() {
    typedef typename F::Report Report;
    typedef typename F::Entry Entry;
    int failures = 0;
    for (int round = 0; round < 200; round++) {
        const size_t n_chunks = 1 + rnd() % 6;
        std::vector<uint64_t> pool = {0ull, ~0ull, MADSIM_PROBE_SET_OTHER, MADSIM_PROBE_SET_TRUNCATED | 5ull};
        for (size_t i = rnd() % 40; i > 0; i--) pool.push_back(rnd());
        std::vector<std::vector<Entry>> chunks(n_chunks);
        std::vector<std::array<unsigned long long, F::words>> words(n_chunks);
        std::map<uint64_t, Entry> want;
        Report sum{};                                                              // the totals of every chunk
        for (size_t c = 0; c < n_chunks; c++) {
            words[c].fill(0);
            for (size_t e = rnd() % 30; e > 0; e--) {
                const Entry x = F::entry(pool[rnd() % pool.size()]);
                auto at = want.find(F::key(x));
                if (at == want.end()) want.emplace(F::key(x), x); else F::combine(at->second, x);
                chunks[c].push_back(x);
            }
            words[c][0] = chunks[c].size();
            F::totals(words[c].data());
            F::add(sum, words[c].data());
        }
        for (int short_by = 0; short_by < 2; short_by++) {
            if (want.size() < (size_t)short_by + 1) continue;
            const size_t cap = want.size() - short_by;
            std::unique_ptr<Entry[]> table(new Entry[cap]);                        // exactly cap entries: one write too far is a report
            Report rep{};
            F::table(rep, table.get()); rep.cap = cap;
            int rc = 0;
            for (size_t c = 0; c < n_chunks && !rc; c++) {
                std::vector<Entry> before(table.get(), table.get() + F::count(rep));
                const Report was = rep;
                rc = F::fold(&rep, c % 2 ? words[c].data() : nullptr, chunks[c].empty() ? nullptr : chunks[c].data(), chunks[c].size());
                if (!rc && !(c % 2)) F::add(rep, words[c].data());                 // (null words: no totals)
                if (rc && (std::memcmp(&was, &rep, sizeof rep) || (F::count(rep) && std::memcmp(before.data(), table.get(), F::count(rep) * sizeof(Entry))))) {
                    std::printf("%s, round %d: a failing fold changed the report\n", F::name, round); failures++;
                }
            }
            if (short_by) {
                if (rc != -1) { std::printf("%s, round %d: one entry short, and no fold failed\n", F::name, round); failures++; }
                continue;
            }
            F::table(sum, table.get()); sum.cap = cap; F::count(sum) = want.size();      // (then the two reports are equal byte for byte)
            bool ok = rc == 0 && !std::memcmp(&sum, &rep, sizeof rep);
            size_t i = 0;
            for (const auto& kv : want) {
                if (!ok) break;
                ok = !std::memcmp(&table[i++], &kv.second, sizeof(Entry));
            }
            if (!ok) { std::printf("%s, round %d: the folded table differs from the map\n", F::name, round); failures++; }
        }
    }
    std::printf(failures ? "fold_obs_reports_check: %s: %d FAILURES\n" : "fold_obs_reports_check ok: %s: 200 rounds, no difference\n", F::name, failures);
    return failures;
}

int main() {
    const int failures = check<CensusFold>() + check<ProbeSetsFold>() + check<ProbeOrderFold>();
    return failures ? 1 : 0;
}
