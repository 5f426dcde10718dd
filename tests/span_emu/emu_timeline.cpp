// emu_timeline.cpp — the trace builds' time log on the host: tests/emu's driver (the device code, host-compiled, one emulated thread after
// another) with one more entry point, the list form of madsim_hip_timeline_seeds.  Test-only, as tests/emu is: it checks the kernel's
// LOGIC on a box without a GPU; the GPU build is checked by tests/test_spans_gpu.py.
#include "../emu/emu_driver.cpp"

extern "C" int madsim_emu_timeline_seeds(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n,
                                         const madsim_limits_t* lim, uint64_t* obs, uint64_t* times, uint64_t obs_cap, uint64_t* obs_len,
                                         madsim_result_t* out) {
    int rc = madsim_geo::validate(w, cfg, &emu_err);
    if (rc) return rc;
    madsim_geo::Device dev; dev.num_cus = 2;
    madsim_geo::Geo G;
    if ((rc = madsim_geo::make_geometry(dev, w, cfg, lim, n, &G, &emu_err, true))) return rc;
    madsim_k::KParams& P = G.P;
    madsim_geo::DeviceTables T;
    if ((rc = madsim_geo::build_tables(w, &T, &emu_err))) return rc;
    P.insns = (const uint4*)T.insns.data(); P.progs = T.progs.data(); P.socks = T.socks.data(); P.nodes = T.nodes.data(); P.dur_table = T.durs.data();
    std::vector<uint4> spill((size_t)P.heap_spill * P.total_lanes + 1);
    P.spill = P.heap_spill ? spill.data() : nullptr;
    std::vector<uint4> gstate((size_t)P.gs_stride * P.total_lanes / 16 + 4);
    P.gstate = (P.gstate_mode || P.compact) ? (uint8_t*)gstate.data() : nullptr;
    P.seed0 = 0; P.count = n; P.seed_list = seeds; P.out = out;
    std::vector<uint64_t> log_len(n);
    P.trace_log = nullptr; P.trace_cap = 0; P.trace_len = log_len.data();
    memset(obs, 0, (size_t)(n * obs_cap) * sizeof(uint64_t));             // (the host library zero-fills the rows before the launch)
    // (the time rows lie in the observation log's allocation, a 32-bit number of words behind the observation rows: sim_kernel.h obs_time_words)
    if (times && (times <= obs || (uint64_t)(times - obs) > 0xffffffffull)) { emu_err = "the time rows must lie behind the observation rows, within 2^32 - 1 words"; return MADSIM_E_ARG; }
    if (times) memset(times, 0, (size_t)(n * obs_cap) * sizeof(uint64_t));
    P.obs_log = obs; P.obs_cap = obs_cap; P.obs_len = obs_len; P.obs_time_words = times ? (uint32_t)(times - obs) : 0u;
    std::vector<uint32_t> lds(G.lds_bytes / 4 + 4);
    uint32_t* base = lds.data();
    while (((uintptr_t)base) & 15) base++;
    const int vi = madsim_k::variant_index(madsim_k::select_variant(P, true));
    if (vi < 0) { emu_err = "select_variant named a build that is not compiled"; return MADSIM_E_LIMITS; }
    for (uint32_t b = 0; b < G.grid * G.waves_per_block; b++)
        for (uint32_t t = 0; t < G.lanes_per_wave; t++) {
            blockIdx.x = b / G.waves_per_block; threadIdx.x = (b % G.waves_per_block) * 64 + t; emu_smem = base;
            emu_kernels[vi](P);
        }
    return madsim_k::variant_table[vi].feat;          // (>= 0: the feature mask of the trace build that ran, so that a test can see all five were covered)
}
