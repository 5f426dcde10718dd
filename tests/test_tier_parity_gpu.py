"""Timeout scopes, interval tickers, biased selects and ctrl-c signals on the MI355X against the C oracle: the sixteen builds these
four op families run on (four shapes each, sim_kernel.h MADSIM_TIER_VARIANTS) get what the base-op builds get from
tests/test_gpu_parity.py — fuzz blocks compared on all 48 result bytes with every capacity verdict re-run, batches that cross a wave
edge with a ragged tail, every lane stride of the LDS-resident build, and the raw determinism log of the trace build.  The oracle's
code for these ops is held against the families' sims on the CPU first (tests/test_oracle_tiers.py), which also shows that the
fixed blocks below reach every event, verdict and build.  Seeds are printed on failure."""
import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from tests import parity
from tests import test_gpu_parity as G
from tests import tier_blocks as TB

pytestmark = pytest.mark.gpu

FAMILY_NAMES = sorted(TB.FAMILIES)
LOSS = 0.05                                    # the wave-edge and lane-stride batches run under packet loss
U64 = 1 << 64


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_fuzz_tier_family_equals_the_oracle(hip, name):
    """A fixed block of 150 programs and a fresh one of 75 (MADSIM_FUZZ_SEED), 96 seeds each — one full wave plus a half —, global
    state on odd programs, general addresses on every third, no trace hash on every fourth; expectations from the oracle's pure layer
    (parity.expected), every first-pass MADSIM_OVERFLOW re-run and compared."""
    fam = TB.FAMILIES[name]
    tally = {}
    G._fuzz_two_blocks(hip, fam.gen, fam.base, TB.N_FIXED, TB.N_FRESH, fam.salt, count=TB.SEEDS, seed_mul=TB.SEED_MUL,
                       limits=fam.limits, alt_global=True, gen_kw_of=fam.gen_kw_of, tally=tally)
    seeds, rerun, beyond = G.TALLY.rows[fam.gen.__name__]
    print(f"{name}: seeds {seeds}, re-run {rerun}, beyond ceilings {beyond} [MADSIM_FUZZ_SEED={G.FUZZ_SEED}]")
    assert seeds == (TB.N_FIXED + TB.N_FRESH) * TB.SEEDS and beyond == 0
    assert {A.PASS, A.PANIC, A.DEADLOCK} <= tally["verdicts"]


def _layouts(fam):
    for sm in (A.STATE_LDS, A.STATE_GLOBAL):
        lim = fam.directed_limits()
        lim.state_mem = sm
        yield sm, lim


def _assert_batch_equals_oracle(hip, w, seed0, count, cfg, lim, what):
    got, summ = hip.run_batch(w, seed0, count, cfg, lim)
    want, osumm = oracle.run_batch(w, seed0, count, cfg, lim)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (what, f"{len(bad)} of {count} seeds differ, first seed {(seed0 + int(bad[0])) % U64}", got[bad[0]], want[bad[0]])
    assert (summ.n_failed, summ.first_failing_seed, summ.total_steps) == (osumm.n_failed, osumm.first_failing_seed, osumm.total_steps), what
    return got


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_wave_edge_batches_equal_the_oracle_in_both_layouts(hip, name):
    """The family's directed workload under loss: batches of 1, 63, 65 and 257 seeds from seed 77 — under, across and well past a wave
    edge, each with a ragged tail — and 512 seeds from 2^64 - 600, results and summary."""
    fam = TB.FAMILIES[name]
    w, cfg = fam.directed(), A.Config.default(packet_loss_rate=LOSS)
    for sm, lim in _layouts(fam):
        g = hip.geometry(w, lim)
        assert g.variant & TB.TIER_BITS == fam.tier and bool(g.variant & 16) == (sm == A.STATE_GLOBAL)
        for seed0, count in ((77, 1), (77, 63), (77, 65), (77, 257), (U64 - 600, 512)):
            _assert_batch_equals_oracle(hip, w, seed0, count, cfg, lim, (name, sm, seed0, count))


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_lanes_per_wave_on_the_lds_tier_build(hip, name):
    """The LDS-resident tier build is the runtime-lane-stride one: 8, 16, 32 and 64 seed lanes per wave give the same bytes, the oracle's.
    (tonic_unary and raft_ticker at a size whose per-seed state fits 64 lanes of one wave's LDS.)"""
    fam = TB.FAMILIES[name]
    w, cfg = fam.lanes(), A.Config.default(packet_loss_rate=LOSS)
    first = None
    for lanes in (8, 16, 32, 64):
        lim = fam.lanes_limits()
        lim.state_mem, lim.lanes_per_wave = A.STATE_LDS, lanes
        g = hip.geometry(w, lim)
        assert g.lanes_per_wave == lanes and not g.variant & 16 and (g.variant >> 16) & 0xf == 15 and g.variant & TB.TIER_BITS == fam.tier
        got = _assert_batch_equals_oracle(hip, w, 5000, 1024, cfg, lim, (name, lanes))
        first = got if first is None else first
        assert got.tobytes() == first.tobytes(), (name, lanes)


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_raw_logs_of_the_tier_trace_builds_equal_the_oracle(hip, name):
    """hip.trace_seed against oracle.trace_seed: two seeds each of four programs of the fixed block, three of them with general
    addresses — the tier trace builds, which no sim-based test reaches with such programs."""
    fam = TB.FAMILIES[name]
    for k in TB.TRACED:
        w, cfg, desc = fam.program(fam.base, k)
        for s in TB.TRACE_SEEDS:
            seed = k * TB.SEED_MUL + s
            lim = TB.limits_of(fam, k)
            log, res = hip.trace_seed(w, seed, cfg, lim)
            for _ in range(8):                                  # (a capacity verdict: the trace is run again with grown capacities)
                if int(res.verdict) != A.OVERFLOW:
                    break
                lim = parity.grow(lim, w.struct.n_progs)
                log, res = hip.trace_seed(w, seed, cfg, lim)
            olog, ores = oracle.trace_seed(w, seed, cfg, lim)
            assert res.astuple() == ores.astuple(), (name, k, seed, desc)
            assert log == olog, (name, k, seed, desc, len(log), len(olog))
