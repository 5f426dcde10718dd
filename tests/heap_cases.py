"""The cases of tests/test_emu_heap_boundaries.py and tests/test_gpu_heap_boundaries.py (test infrastructure): the timer heap of
k_timer.h at every position of the LDS / spill boundary, under deadlines that tie.

timer_pop is BinaryHeap::pop only in its result.  On the builds with a spill region it walks top-down with a stop test, the LDS-resident
levels first, heap_sift_up takes two levels per trip; the compact layout keeps the root in registers and the narrow builds store 8-byte
entries.  The final array must be the literal algorithm's, the order of EQUAL deadlines included (`l >= r` takes the right child,
`cand <= idl` keeps moving, `idl < m` is strict), and which code decides that depends on where `heap_lds` falls in the tree: both children
in LDS, both spilled, the pair astride the boundary, a single last child, nothing moved below the LDS levels.

So: workloads whose deadlines tie (the oracle's heap_tie_pops counts it), on every build that has a heap path of its own (each case
asserts the build its limits select), at LDS quotas on both sides of every level start.  Every seed of a first pass must be a genuine
verdict: a seed is compared on the build it was aimed at, never on a re-run's."""
import numpy as np

import oracle
from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import parity

SEEDS = 130             # two full waves and two lanes at 64 seed lanes per wave
SEED0 = 11
GOLDEN_SEEDS = 16       # per workload, against tests/golden/make_golden_async.py
QUOTAS = (1, 2, 3, 4, 6, 7, 8, 14, 15, 16, 30, 31, 32)     # both sides of every level start (1, 3, 7, 15, 31), both parities; then n, n + 1
LOCKSTEP = ((40, 8), (40, 32), (12, 64), (5, 128))
STEADY_N, STEADY_ROUNDS = 40, 4


def _storm(n, rounds, flavour, sleep):
    """`n` tasks on one node, each `rounds` x sleep; main spawns them all and joins them all.  flavour "time": a mark() in front of each
    task's loop (the timeouts-only class); "all": that, and main kills an otherwise unused second node behind the joins (every class)."""
    assert flavour in ("base", "time", "all")
    wl = W.WorkloadBuilder()
    node = wl.create_node()
    spare = wl.create_node() if flavour == "all" else None
    tasks = []
    for _ in range(n):
        t = wl.task(node)
        if flavour != "base":
            t.mark()
        t.set(0, rounds)
        top = t.label()
        sleep(t)
        t.djnz(0, top)
        t.done()
        tasks.append(t)
    m = wl.main()
    for t in tasks:
        m.spawn(t)
    for t in tasks:
        m.join(t)
    if spare is not None:
        m.kill(spare)
    m.done()
    return wl.build()


def lockstep(n, rounds, extended=False, every_class=False):
    """Every task loops `sleep(gen_range(50 ms .. 50 ms + 256 ns))`: the heap fills to n and drains to 0 every round — every heap length is
    popped — and the deadlines of a round sit a few hundred nanoseconds apart, so equal ones occur (lo_ms = 0 gives none)."""
    return _storm(n, rounds, "all" if every_class else "time" if extended else "base", lambda t: t.sleep_rand(lo_ms=50, ms=50, ns=256))


def steady(n=STEADY_N, rounds=STEADY_ROUNDS, extended=False, every_class=False):
    """The timer storm with sleeps below 1 s (inside the narrow layout's 2^31 ns horizon): pushes and pops interleaved at a steady depth."""
    return _storm(n, rounds, "all" if every_class else "time" if extended else "base", lambda t: t.sleep_rand(lo_ms=0, secs=1))


_WORKLOADS, _TRUTH, _STATS = {}, {}, {}


def workload(key):
    """key = ("lockstep", n, rounds, flavour) | ("steady", n, rounds, flavour), built once."""
    if key not in _WORKLOADS:
        kind, n, rounds, flavour = key
        _WORKLOADS[key] = (lockstep if kind == "lockstep" else steady)(n, rounds, extended=flavour == "time", every_class=flavour == "all")
    return _WORKLOADS[key]


def quota_limits(n, q, base=None):
    """heap_lds_slots = q, heap_spill_slots = n + 8 - q on top of a layout's limits."""
    lim = A.Limits()
    if base is not None:
        for f, _ in A.Limits._fields_:
            setattr(lim, f, getattr(base, f))
    lim.heap_lds_slots, lim.heap_spill_slots = q, n + 8 - q
    return lim


def truth(key):
    """What every build must answer for the SEEDS seeds of a workload (parity.expected: the oracle with the model's ceilings off), computed
    once and left unchanged.  It does not depend on the heap quotas: held once per workload, at the smallest and the largest."""
    if key not in _TRUTH:
        w, n = workload(key), key[1]
        want = parity.expected(w, SEED0, SEEDS, None, A.Limits())
        for q in (1, n + 1):
            assert (parity.expected(w, SEED0, SEEDS, None, quota_limits(n, q)) == want).all(), (key, q)
        want.setflags(write=False)
        _TRUTH[key] = want
    return _TRUTH[key]


def stats_by_seed(key):
    """Per seed: (heap_tie_pops, heap_pops, max_heap) of the oracle's run."""
    if key not in _STATS:
        w = workload(key)
        rows = []
        for i in range(SEEDS):
            st = oracle.run_batch(w, SEED0 + i, 1, want_stats=True)[2]
            rows.append((st.heap_tie_pops, st.heap_pops, st.max_heap))
        _STATS[key] = np.array(rows)
    return _STATS[key]


def quotas(n):
    return sorted({q for q in QUOTAS + (n, n + 1) if q <= n + 1})


# ---- layouts: name -> the exact build (runtime.variant_name), the limits that select it, its workloads --------------------------------------
def _lim(**kw):
    lim = A.Limits()
    for k, v in kw.items():
        setattr(lim, k, v)
    return lim


def _keys(flavour, sizes=LOCKSTEP, with_steady=True):
    return [("lockstep", n, r, flavour) for n, r in sizes] + ([("steady", STEADY_N, STEADY_ROUNDS, flavour)] if with_steady else [])


SMALL = ((5, 128), (7, 64))                 # the register ready queue holds eight tasks, main among them
LDS_SIZES = ((5, 128), (12, 64))            # extended LDS-resident layouts: 40 task records do not fit beside the heap
G, NH, DD = A.STATE_GLOBAL, A.STATE_NARROW_HEAP, A.STATE_DEDUP_TIMERS
TIME, ALL, PLAIN, NARROW = 1, 31, 15, 128   # FEAT words of the builds' names (sim_kernel.h MADSIM_FEAT_*)


def _v(spill, lws, feat, rq, g):
    b = lambda x: "true" if x else "false"      # noqa: E731
    return f"sim_kernel<Variant<false, {b(spill)}, {lws}, {feat}, {b(rq)}, {b(g)}>>"


class Layout:
    """sweep: the LDS quota is swept (else q = n + 1 with no spill region: the literal pop); dedup / narrow: what the parameter block must
    carry beside the build's name (the de-duplication table is a run-time switch of the timeouts-only global-state build)."""

    def __init__(self, variant, limits, keys, sweep=True, dedup=False, narrow=False):
        self.variant, self.limits, self.keys, self.sweep, self.dedup, self.narrow = variant, limits, keys, sweep, dedup, narrow


LAYOUTS = {
    # base ops, spill region: the top-down pop
    "rq_spill":      Layout(_v(1, 6, 0, 1, 0), _lim(), _keys("base", SMALL, False)),
    "queue_spill":   Layout(_v(1, 6, 0, 0, 0), _lim(max_tasks=48, lanes_per_wave=64), _keys("base")),
    "stride32":      Layout(_v(1, -1, 0, 0, 0), _lim(max_tasks=48, lanes_per_wave=32), _keys("base")),
    "stride16":      Layout(_v(1, -1, 0, 0, 0), _lim(max_tasks=48, lanes_per_wave=16), _keys("base")),
    "stride8":       Layout(_v(1, -1, 0, 0, 0), _lim(max_tasks=48, lanes_per_wave=8), _keys("base")),
    # base ops, no spill region: the literal pop; the compact build keeps the root in registers and 8-byte entries from slot 1
    "queue_lds":     Layout(_v(0, 6, 0, 0, 0), _lim(max_tasks=16, lanes_per_wave=64), _keys("base", SMALL, False), sweep=False),
    "rq_lds":        Layout(_v(0, 6, 0, 1, 0), _lim(state_mem=A.STATE_LDS), _keys("base", SMALL, False), sweep=False),
    "compact":       Layout(_v(0, 6, 64, 1, 0), _lim(state_mem=A.STATE_COMPACT), _keys("base", SMALL, False), sweep=False),
    # extended ops, LDS-resident
    "time_lds":      Layout(_v(1, -1, TIME, 0, 0), _lim(state_mem=A.STATE_LDS), _keys("time", LDS_SIZES, False)),
    "all_lds64":     Layout(_v(1, 6, ALL, 0, 0), _lim(state_mem=A.STATE_LDS, lanes_per_wave=64), _keys("all", LDS_SIZES, False)),
    "all_lds32":     Layout(_v(1, 5, ALL, 0, 0), _lim(state_mem=A.STATE_LDS, lanes_per_wave=32), _keys("all", LDS_SIZES, False)),
    "all_lds16":     Layout(_v(1, 4, ALL, 0, 0), _lim(state_mem=A.STATE_LDS, lanes_per_wave=16), _keys("all", LDS_SIZES, False)),
    "all_lds8":      Layout(_v(1, 3, ALL, 0, 0), _lim(state_mem=A.STATE_LDS, lanes_per_wave=8), _keys("all", LDS_SIZES, False)),
    # global state: wide (16-byte) and narrow (8-byte) entries; the timeouts-only build with and without the de-duplication table
    "g_time64":      Layout(_v(1, 6, TIME, 0, 1), _lim(state_mem=G), _keys("time")),
    "g_time32":      Layout(_v(1, 5, TIME, 0, 1), _lim(state_mem=G, lanes_per_wave=32), _keys("time")),
    "g_time64_dd":   Layout(_v(1, 6, TIME, 0, 1), _lim(state_mem=G | DD), _keys("time"), dedup=True),
    "g_time32_dd":   Layout(_v(1, 5, TIME, 0, 1), _lim(state_mem=G | DD, lanes_per_wave=32), _keys("time"), dedup=True),
    "g_time64_nh":   Layout(_v(1, 6, TIME | NARROW, 0, 1), _lim(state_mem=G | NH), _keys("time"), narrow=True),
    "g_time32_nh":   Layout(_v(1, 5, TIME | NARROW, 0, 1), _lim(state_mem=G | NH, lanes_per_wave=32), _keys("time"), narrow=True),
    "g_time64_nhdd": Layout(_v(1, 6, TIME | NARROW, 0, 1), _lim(state_mem=G | NH | DD), _keys("time"), dedup=True, narrow=True),
    "g_time32_nhdd": Layout(_v(1, 5, TIME | NARROW, 0, 1), _lim(state_mem=G | NH | DD, lanes_per_wave=32), _keys("time"), dedup=True, narrow=True),
    "g_all":         Layout(_v(1, 6, PLAIN, 0, 1), _lim(state_mem=G), _keys("all")),
    "g_all_nh":      Layout(_v(1, 6, PLAIN | NARROW, 0, 1), _lim(state_mem=G | NH), _keys("all"), narrow=True),
}

# the trace build, sim_kernel<Variant<true, true, -1, 31, false, false>> (every trace call of a workload without timer-tier ops runs it)
TRACE_KEY, TRACE_SEEDS, TRACE_QUOTAS = ("lockstep", 12, 64, "all"), 8, (1, 2, 7)


def all_keys():
    keys = []
    for lay in LAYOUTS.values():
        for k in lay.keys:
            if k not in keys:
                keys.append(k)
    return keys


def cases(layout):
    """(key, workload, q, limits) of a layout."""
    lay = LAYOUTS[layout]
    for key in lay.keys:
        n = key[1]
        for q in (quotas(n) if lay.sweep else [n + 1]):
            lim = quota_limits(n, q, lay.limits)
            if not lay.sweep:
                lim.heap_spill_slots = 0
            yield key, workload(key), q, lim


def check_variant(layout, w, lim, emu=None):
    """The case runs on exactly the build its layout names: the host library's selection, which is the device run's.  The host-compiled
    kernel selects with the same select_variant over the same make_geometry; it is held to the library's lane stride, spill region, entry
    width and de-duplication table (its LDS quota on a global-state layout follows ITS register budget: geometry.h `fit`)."""
    from madsim_amd import runtime
    lay = LAYOUTS[layout]
    g = runtime.geometry(w, lim)
    assert runtime.variant_name(g) == lay.variant, (layout, runtime.variant_name(g), lay.variant)
    assert (g.heap_spill_slots > 0) == lay.sweep, (layout, g.heap_spill_slots)
    assert g.heap_lds_slots + g.heap_spill_slots == lim.heap_lds_slots + lim.heap_spill_slots, (layout, "the split keeps the capacity")
    if emu is not None:
        e, p = emu.geometry(w, lim), emu.geometry_params(w, lim)
        assert e.lanes_per_wave == g.lanes_per_wave and (p["heap_spill"] > 0) == (g.heap_spill_slots > 0), (layout, e.lanes_per_wave)
        assert bool(p["narrow"]) == lay.narrow and bool(p["dedup_n"]) == lay.dedup and bool(p["gstate_mode"]) == lay.variant.endswith(", true>>"), (layout, p)
        if not p["gstate_mode"]:
            assert e.heap_lds_slots == g.heap_lds_slots, (layout, e.heap_lds_slots, g.heap_lds_slots)
    return g


def assert_boundaries(layout, seen):
    """The realised boundaries of a swept layout: 1, 2, 3, 4 and, beyond them, an even and an odd one."""
    assert {1, 2, 3, 4} <= seen, (layout, sorted(seen))
    assert any(b > 4 and b % 2 == 0 for b in seen) and any(b > 4 and b % 2 for b in seen), (layout, sorted(seen))


def run_layout(layout, run, boundary, check=None):
    """Every case of a layout: `run(w, seed0, count, cfg, lim)` -> results, compared with the truth on all 48 bytes; no seed of the pass may
    be a runner verdict.  `boundary(w, lim)` = the heap_lds the case really runs with.  -> {realised boundary: cases}."""
    seen = {}
    for key, w, q, lim in cases(layout):
        if check is not None:
            check(layout, w, lim)
        want = truth(key)
        got = run(w, SEED0, SEEDS, None, lim)
        what = (layout, key, q)
        assert not (got["verdict"] >= A.OVERFLOW).any(), (what, "runner verdicts in the first pass", np.unique(got["verdict"], return_counts=True))
        bad = got != want
        assert not bad.any(), (what, f"{int(bad.sum())} of {SEEDS} seeds differ", int(np.nonzero(bad)[0][0]) + SEED0, got[bad][0], want[bad][0])
        b = boundary(w, lim)
        seen[b] = seen.get(b, 0) + 1
    if LAYOUTS[layout].sweep:
        assert_boundaries(layout, set(seen))
    print(f"[heap boundaries] {layout}: {sum(seen.values())} cases, realised LDS quotas {sorted(seen)}, largest {max(seen)}")
    return seen


def count_differing(layout, run):
    """(key, q, seeds that differ from the truth) per case of a layout, nothing asserted: what tools/heap_mutants.py tabulates."""
    for key, w, q, lim in cases(layout):
        yield key, q, int((run(w, SEED0, SEEDS, None, lim) != truth(key)).sum())


def trace_truth(q):
    """(log bytes, result tuple) per seed of the trace case, from the oracle."""
    w = workload(TRACE_KEY)
    out = []
    for s in range(SEED0, SEED0 + TRACE_SEEDS):
        log, res = oracle.trace_seed(w, s, None, quota_limits(TRACE_KEY[1], q))
        out.append((log, res.astuple()))
    return out
