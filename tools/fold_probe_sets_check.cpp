// tools/fold_probe_sets_check.cpp — madsim_k_fold_probe_sets (the host fold of the probe-set census, madsim_hip.cpp) in a stand-alone
// program, meant to be built with AddressSanitizer and UndefinedBehaviorSanitizer on the host side.  No device is touched: the fold is
// plain host code.  Random chunks of entries (equal sets inside a chunk, sets shared between chunks, the set words 0 and 2^64 - 1) are
// folded into a table sized EXACTLY to the number of distinct sets — every write at the table's last element is inside it — and held
// against a std::map; then once more into a table one entry short, where the fold that would pass the cap must return -1 and leave the
// table and the totals as they were.
//
//   cd madsim_amd/csrc && make
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -x hip -Xarch_host -fsanitize=address,undefined -c madsim_hip.cpp -o /tmp/madsim_hip_san.o
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -c ../../tools/fold_probe_sets_check.cpp -o /tmp/fold_probe_sets_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/fold_probe_sets_check.o /tmp/madsim_hip_san.o sim_kernel.o
//         (continued) -o /tmp/fold_probe_sets_check && /tmp/fold_probe_sets_check
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
#define MADSIM_K_PROBE_SETS_WORDS 8u
extern "C" int madsim_k_fold_probe_sets(madsim_probe_sets_t* ps, const unsigned long long* words, const madsim_probe_set_t* entries, uint64_t n);

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }

struct Want { std::array<uint64_t, 4> n{}, first{}; };

int main() {
    int failures = 0;
    for (int round = 0; round < 200; round++) {
        const size_t n_chunks = 1 + rnd() % 6;
        std::vector<uint64_t> pool = {0ull, ~0ull, MADSIM_PROBE_SET_OTHER, MADSIM_PROBE_SET_TRUNCATED | 5ull};
        for (size_t i = rnd() % 40; i > 0; i--) pool.push_back(rnd());
        std::vector<std::vector<madsim_probe_set_t>> chunks(n_chunks);
        std::vector<std::array<unsigned long long, MADSIM_K_PROBE_SETS_WORDS>> words(n_chunks);
        std::map<uint64_t, Want> want;
        uint64_t counted[4] = {0, 0, 0, 0}, runner = 0;
        for (size_t c = 0; c < n_chunks; c++) {
            words[c].fill(0);
            for (size_t e = rnd() % 30; e > 0; e--) {
                madsim_probe_set_t x{};
                x.set = pool[rnd() % pool.size()];
                for (int k = 0; k < 4; k++) {
                    if (rnd() % 3 == 0) continue;
                    x.n_seeds[k] = 1 + rnd() % 1000;
                    x.first_seed[k] = rnd() % 5 ? rnd() : 0;                       // (seed 0 is a seed like any other)
                    Want& w = want[x.set];
                    w.first[k] = w.n[k] ? std::min(w.first[k], x.first_seed[k]) : x.first_seed[k];
                    w.n[k] += x.n_seeds[k];
                    words[c][2 + k] += x.n_seeds[k];
                    counted[k] += x.n_seeds[k];
                }
                want[x.set];
                chunks[c].push_back(x);
            }
            words[c][0] = chunks[c].size();
            words[c][6] = rnd() % 7;
            runner += words[c][6];
        }
        for (int short_by = 0; short_by < 2; short_by++) {
            if (want.size() < (size_t)short_by + 1) continue;
            const size_t cap = want.size() - short_by;
            std::unique_ptr<madsim_probe_set_t[]> table(new madsim_probe_set_t[cap]);      // exactly cap entries: one write too far is a report
            madsim_probe_sets_t ps{};
            ps.sets = table.get(); ps.cap = cap;
            int rc = 0;
            for (size_t c = 0; c < n_chunks && !rc; c++) {
                std::vector<madsim_probe_set_t> before(table.get(), table.get() + ps.n_sets);
                const madsim_probe_sets_t was = ps;
                rc = madsim_k_fold_probe_sets(&ps, c % 2 ? words[c].data() : nullptr, chunks[c].empty() ? nullptr : chunks[c].data(), chunks[c].size());
                if (!rc && !(c % 2)) { for (int k = 0; k < 4; k++) ps.n_counted[k] += words[c][2 + k]; ps.n_runner += words[c][6]; }      // (null words: no totals)
                if (rc && (std::memcmp(&was, &ps, sizeof ps) || (ps.n_sets && std::memcmp(before.data(), table.get(), ps.n_sets * sizeof(madsim_probe_set_t))))) {
                    std::printf("round %d: a failing fold changed the report\n", round); failures++;
                }
            }
            if (short_by) {
                if (rc != -1) { std::printf("round %d: one entry short, and no fold failed\n", round); failures++; }
                continue;
            }
            bool ok = rc == 0 && ps.n_sets == want.size() && ps.n_runner == runner;
            for (int k = 0; k < 4; k++) ok = ok && ps.n_counted[k] == counted[k];
            size_t i = 0;
            for (const auto& kv : want) {
                if (!ok) break;
                const madsim_probe_set_t& e = table[i++];
                ok = e.set == kv.first;
                for (int k = 0; k < 4; k++) ok = ok && e.n_seeds[k] == kv.second.n[k] && e.first_seed[k] == (kv.second.n[k] ? kv.second.first[k] : 0);
            }
            if (!ok) { std::printf("round %d: the folded table differs from the map\n", round); failures++; }
        }
    }
    std::printf(failures ? "fold_probe_sets_check: %d FAILURES\n" : "fold_probe_sets_check ok: 200 rounds, no difference\n", failures);
    return failures ? 1 : 0;
}
