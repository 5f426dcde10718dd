"""The workloads of tests/test_emu_pass_invariants.py and tests/test_gpu_pass_invariants.py (test infrastructure): what a poll pass of the
base-op kernels holds fixed — the determinism log's fold of the clock, the pop of a queue of one (k_rng.h ClockFold, k_main.h PopOne)."""
import numpy as np

import oracle
from madsim_amd import _abi as A
from madsim_amd import workload as W

SEEDS = 192             # three full waves at 64 seed lanes per wave (six at 32): no partial wave here, lanes leave a wave's vote only by finishing
SEEDS_TIE = 200         # the tie workload: three full waves and a partial one of eight lanes (64 lanes per wave)
SEED0 = 11
ROUNDS = 3
PINGPONG = [(nodes, loss) for nodes in (2, 4, 6) for loss in (0.0, 0.05)]

# One layout per changed build: the word madsim_geometry_t.variant reports for it
# (spill | register queue << 2 | runtime lane stride << 3 | FEAT << 8 | log2 lanes << 16; FEAT 64 = compact, 32 = no determinism log).
LAYOUTS = {
    "compact":       0x64004,   # Variant<false,false,6,COMPACT,true,false>: the benchmark's build (clock fold + short pop)
    "compact_nolog": 0x66004,   # ... without the log: the short pop alone
    "lds":           0x60004,   # Variant<false,false,6,0,true,false>: the plain layout, register queue, no spill region
    "lds_nolog":     0x62004,   # ... without the log: the short pop alone
    "spill":         0x60005,   # Variant<false,true,6,0,true,false>: default limits — register queue and a heap spill region
    "queue":         0x60000,   # Variant<false,false,6,0,false,false>: room for 16 tasks, so the ready queue is an LDS plane (the clock fold alone)
    "queue_spill":   0x60001,   # Variant<false,true,6,0,false,false>
    "stride":        0xf0009,   # Variant<false,true,-1,0,false,false>: 32 seed lanes per wave, the runtime-lane-stride build
}
assert len(set(LAYOUTS.values())) == len(LAYOUTS)


def config(loss):
    return A.Config.default(packet_loss_rate=loss) if loss else None


def limits(layout, tasks):
    """The limits that make the library select the build LAYOUTS names, for a workload of `tasks` tasks beside the main one.  compact / lds:
    the benchmark's own (workload.pingpong_bench_limits: no heap spill, one registration per mailbox) with the layout forced either way."""
    lim = A.Limits()
    if layout in ("compact", "compact_nolog", "lds", "lds_nolog"):
        lim.heap_lds_slots, lim.heap_spill_slots = max(4, tasks), 0
        lim.mbox_regs, lim.mbox_msgs = 1, A.LIMIT_NONE
        lim.state_mem = A.STATE_COMPACT if layout.startswith("compact") else A.STATE_LDS
        lim.no_trace_hash = 1 if layout.endswith("nolog") else 0
    elif layout == "queue":
        lim.max_tasks, lim.lanes_per_wave = 16, 64
        lim.heap_lds_slots, lim.heap_spill_slots = 8, 0
    elif layout == "queue_spill":
        lim.max_tasks, lim.lanes_per_wave = 16, 64
    elif layout == "stride":
        lim.max_tasks, lim.lanes_per_wave = 16, 32
    else:
        assert layout == "spill"
    return lim


def check_variant(w, lim, layout, emu=None):
    """The case runs on exactly the build its layout is named for (the host library's selection, which is the device run's).  The host-compiled
    kernel selects with the same select_variant over the same make_geometry (tests/emu/emu_driver.cpp); its own variant word carries no FEAT
    bits, so it is held to the library's lane stride, LDS footprint (compact is smaller than plain), spill region and register queue."""
    from madsim_amd import runtime
    g = runtime.geometry(w, lim)
    assert g.variant == LAYOUTS[layout], (layout, hex(g.variant), hex(LAYOUTS[layout]))
    if emu is not None:
        e = emu.geometry(w, lim)
        assert (emu.geometry_params(w, lim)["heap_spill"] > 0) == bool(g.variant & 1), layout
        assert (e.lanes_per_wave, e.lds_bytes_per_seed) == (g.lanes_per_wave, g.lds_bytes_per_seed), (layout, e.lanes_per_wave, e.lds_bytes_per_seed)
        assert bool(e.variant & 4) == bool(g.variant & 4) or g.lanes_per_wave != 64, (layout, hex(e.variant))
    if layout.startswith("compact"):
        plain = runtime.geometry(w, limits("lds", lim.heap_lds_slots))
        assert g.lds_bytes_per_seed < plain.lds_bytes_per_seed, (g.lds_bytes_per_seed, plain.lds_bytes_per_seed)


def tie_workload(rounds=ROUNDS):
    """Two tasks whose timers tie in some seeds and not in others.  The main task spawns ONE task (the queue never holds two at start-up), then
    both loop `sleep(gen_range(50 ms .. 50 ms + 128 ns))`: the two deadlines of a round lie a few dozen nanoseconds apart, and the idle jump
    (to the earlier deadline + 50 ns, time/mod.rs:47-53) fires both timers at once when the later one is inside that window — the ready queue
    then holds two tasks in that seed's lane while it holds one in the lanes of the seeds without a tie."""
    wl = W.WorkloadBuilder()
    n = wl.create_node()
    t = wl.task(n)
    t.set(0, rounds)
    top = t.label()
    t.sleep_rand(lo_ms=50, ms=50, ns=128)
    t.djnz(0, top)
    t.done()
    m = wl.main()
    m.spawn(t)
    m.set(0, rounds)
    top = m.label()
    m.sleep_rand(lo_ms=50, ms=50, ns=128)
    m.djnz(0, top)
    m.join(t)
    m.done()
    return wl.build()


def max_ready_by_seed(w, seed0, count, cfg=None, lim=None):
    """The longest ready queue of each seed's run, from the oracle's own high-water mark."""
    return np.array([oracle.run_batch(w, seed0 + i, 1, cfg, lim, want_stats=True)[2].max_ready for i in range(count)])


def assert_ties_in_every_wave(mr, lanes=32):
    """Every group of `lanes` consecutive seeds — a wave's lanes at the narrowest stride the layouts use — holds seeds with a tie and seeds without."""
    for k in range(0, len(mr) - lanes + 1, lanes):
        assert set(mr[k:k + lanes].tolist()) == {1, 2}, (k, np.unique(mr[k:k + lanes], return_counts=True))
