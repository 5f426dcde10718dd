"""The fuzz blocks of the four op families that run on builds of their own — timeout scopes, interval tickers, the biased selects,
ctrl-c signals — shared by the CPU tests that hold the oracle against the families' sims and check the blocks are not vacuous
(tests/test_oracle_tiers.py) and the GPU tests that run the same blocks on the device (tests/test_tier_parity_gpu.py).  Test
infrastructure.

A block is `gen(Random(base + k), general_addr=(k % 3 == 2), hazards=True)` for k < n, SEEDS seeds each from seed k * SEED_MUL, under
`limits_of(family, k)`: the family's limits, global state on odd programs, no determinism-log fingerprint on every fourth — the rule of
tests/test_gpu_parity.py `_fuzz_block`, stated once more here so that the CPU tests see the limits the GPU run will use.
"""
import random

from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import fuzz_interval, fuzz_scope, fuzz_select, fuzz_signal
from tests import interval_sim, scope_sim, select_sim, signal_sim

N_FIXED, N_FRESH, SEEDS, SEED_MUL = 150, 75, 96, 1000          # 96 seeds: one full wave plus a half
FIELDS = ("verdict", "steps", "clock_ns", "msg_count", "rng_calls", "trace_hash", "obs_hash")


class Family:
    def __init__(self, name, gen, base, limits, sim, tier, salt, counters, directed, directed_limits, test_module, lanes=None):
        self.name, self.gen, self.base, self.limits, self.sim = name, gen, base, limits, sim
        self.tier = tier                     # the A.VARIANT_* bits its builds carry, exactly
        self.salt = salt                     # of the fresh block (MADSIM_FUZZ_SEED)
        self.counters = counters             # the oracle's test-only counters that apply to it
        self.directed, self.directed_limits = directed, directed_limits      # the wave-edge workload and its limits
        self.test_module = test_module       # where its DIRECTED workloads live
        # the directed workload at a size whose state fits 64 seed lanes of the LDS-resident build (160 KiB a wave), and its limits
        self.lanes, self.lanes_limits = lanes or (directed, directed_limits)

    def program(self, base, k):
        """-> (workload, config, description) of program k of the block at `base`."""
        return self.gen(random.Random(base + k), **self.gen_kw_of(k))

    def gen_kw_of(self, k):
        return dict(general_addr=general_addr_of(k), hazards=True)


def general_addr_of(k):
    return k % 3 == 2


def limits_of(fam, k):
    lim = fam.limits()
    if k % 2:
        lim.lanes_per_wave, lim.state_mem = 0, A.STATE_GLOBAL
    if k % 4 == 3:
        lim.no_trace_hash = 1
    return lim


def _scope_limits():
    lim = fuzz_scope.scope_limits()
    lim.state_mem = A.STATE_LDS
    lim.max_conns = 16            # (connections a killed server leaves behind: from the default 4 the re-run's doubling needs two rounds,
    return lim                    #  and the second one's 160 task slots no longer fit a seed's share of LDS)


def _tonic_small_limits():
    lim = W.tonic_unary_limits()
    lim.max_conns, lim.max_tasks = 8, 20
    lim.heap_lds_slots, lim.heap_spill_slots = 4, 60
    return lim


def _raft_small_limits():
    lim = W.raft_ticker_limits()
    lim.heap_spill_slots += lim.heap_lds_slots - 8
    lim.heap_lds_slots = 8
    return lim


TIER_BITS = A.VARIANT_SCOPE | A.VARIANT_TICK | A.VARIANT_SELECT | A.VARIANT_SIGNAL

FAMILIES = {f.name: f for f in (
    Family("scope", fuzz_scope.random_scope_workload, 4_100_000, _scope_limits, scope_sim.ScopeSim, A.VARIANT_SCOPE, 101,
           ("scopes_expired", "scopes_completed", "msgs_lost"),
           lambda: W.tonic_unary(), W.tonic_unary_limits, "tests.test_timeout_scope",
           lanes=(lambda: W.tonic_unary(n_clients=3, n_calls=4), _tonic_small_limits)),
    Family("interval", fuzz_interval.random_interval_workload, 4_200_000, lambda: fuzz_interval.interval_limits(A.STATE_LDS), interval_sim.IntervalSim,
           A.VARIANT_SCOPE | A.VARIANT_TICK, 102,
           ("ticks_first_poll", "ticks_parked", "scopes_expired", "scopes_completed"),
           lambda: W.raft_ticker(), W.raft_ticker_limits, "tests.test_interval",
           lanes=(lambda: W.raft_ticker(n_nodes=3, heartbeats=8, pauses=1), _raft_small_limits)),
    Family("select", fuzz_select.random_select_workload, 4_300_000, lambda: fuzz_select.select_limits(A.STATE_LDS), select_sim.SelectSim,
           A.VARIANT_SCOPE | A.VARIANT_TICK | A.VARIANT_SELECT, 103,
           ("sel_won_recv", "sel_won_time", "msgs_lost", "ticks_first_poll", "ticks_parked"),
           lambda: W.lossy_select(), W.lossy_select_limits, "tests.test_select"),
    Family("signal", fuzz_signal.random_signal_workload, 4_400_000, lambda: fuzz_signal.signal_limits(A.STATE_LDS), signal_sim.SignalSim, A.VARIANT_SIGNAL, 104,
           ("sel_won_recv", "sel_won_ctrl_c", "msgs_lost", "sig_lost", "sig_caught", "sig_killed"),
           lambda: W.shutdown_race(), W.shutdown_race_limits, "tests.test_signal"),
)}

TRACED = (0, 2, 5, 11)      # the programs of each fixed block whose raw logs the GPU test reads: plain and general addresses (2, 5, 11)
TRACE_SEEDS = (3, 64)       # ... two seeds each
