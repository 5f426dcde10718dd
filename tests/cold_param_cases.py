"""The cases of tests/test_emu_cold_params.py and tests/test_gpu_cold_params.py (test infrastructure): the base-op kernels read the launch
parameters that are cold — used once per seed, once per many passes, or on rare sides only — from the kernel-argument segment where they are
used (k_state.h ColdParams / PCOLD) instead of holding them in scalar registers.  A wrong offset there is a wrong seed, a wrong result slot,
a wrong limit or a wrong verdict code, so every cold site has a case of its own besides the ordinary workloads; all of them compare all 48
bytes of every result with the oracle (tests/parity.py).

One layout per base-op build that the switch changes: the eight of tests/pass_invariant_cases.py, with their limits and their build check, and the
ninth build without extended ops, the LDS ready queue without the determinism log (`queue_nolog`)."""
import numpy as np

import oracle
from madsim_amd import workload as W
from tests import pass_invariant_cases as PC

QUEUE_NOLOG = 0x62000                   # Variant<false,false,6,NOLOG,false,false>: room for 16 tasks (an LDS ready queue), no spill region, no log
LAYOUTS = dict(PC.LAYOUTS, queue_nolog=QUEUE_NOLOG)
assert len(set(LAYOUTS.values())) == len(LAYOUTS) == 9
COLD_LAYOUTS = ("compact", "queue")     # the cold sites: the benchmark's build and an LDS-queue build
# buggify: the library refuses it on the compact layout (its delays of whole seconds pass the layout's 2^31 ns deadline window), so the case runs
# on the plain layout with a register queue — the benchmark's build without the compaction — and on the LDS-queue build
BUGGIFY_LAYOUTS = ("lds", "queue")
SEED0 = PC.SEED0
SEED0_HIGH = (1 << 40) + 5              # a seed0 above 2^32: both halves of the 64-bit field are read
ROUNDS = PC.ROUNDS
FIRST = 64                              # the first device contact: one wave of the benchmark's build


def limits(layout, tasks):
    if layout != "queue_nolog":
        return PC.limits(layout, tasks)
    lim = PC.limits("queue", tasks)
    lim.no_trace_hash = 1
    return lim


def check_variant(w, lim, layout, emu=None):
    """The case runs on exactly the build its layout is named for: pass_invariant_cases.check_variant, extended by the ninth layout."""
    if layout in PC.LAYOUTS:
        return PC.check_variant(w, lim, layout, emu)
    from madsim_amd import runtime
    g = runtime.geometry(w, lim)
    assert layout == "queue_nolog" and g.variant == QUEUE_NOLOG, (layout, hex(g.variant))
    if emu is not None:
        e = emu.geometry(w, lim)
        assert emu.geometry_params(w, lim)["heap_spill"] == 0 and not (e.variant & 4)
        assert (e.lanes_per_wave, e.lds_bytes_per_seed) == (g.lanes_per_wave, g.lds_bytes_per_seed)


def pingpong(nodes=2):
    return W.pingpong(nodes, ROUNDS)


def seed_list():
    """130 seeds that are not contiguous: gaps of 1, 2, 3 and 2^33 in turn, so positions and seeds differ above bit 32."""
    gaps = np.array((1, 2, 3, 1 << 33), dtype=np.uint64)[np.arange(129) % 4]
    return np.concatenate([np.array([7], dtype=np.uint64), np.uint64(7) + np.cumsum(gaps, dtype=np.uint64)])


def oracle_of_list(w, seeds, cfg=None, lim=None):
    return np.concatenate([oracle.run_batch(w, int(s), 1, cfg, lim)[0] for s in seeds])


def overflow_limits(layout, nodes):
    """A timer heap of two entries for a workload that holds one timer per node: MADSIM_OVERFLOW in the first pass, same build."""
    lim = PC.limits(layout, nodes)
    lim.heap_lds_slots, lim.heap_spill_slots = 2, 0
    return lim


def step_limits(layout):
    lim = PC.limits(layout, 2)
    lim.max_steps = 20                  # the 2-node ping-pong takes more steps than that in every seed
    return lim


def time_limits(layout):
    lim = PC.limits(layout, 2)
    lim.time_limit_ns = 1_040_000_000   # the lossy 2-node ping-pong ends between 1.00 s and 1.07 s of simulated time
    return lim


def lanes_of_launch(runtime, w, lim):
    """The lanes of a launch that fills the device: KParams.total_lanes of every single launch of at least that many seeds (the grid is capped at
    the blocks resident at once: geometry.h make_geometry), what `next += total_lanes` strides by."""
    g = runtime.geometry(w, lim)
    return g.grid_blocks * g.block_threads // 64 * g.lanes_per_wave
