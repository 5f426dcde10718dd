"""Every op family on every kernel build that compiles it, on the device: the matrix of tests/build_cases.py through hip.run_batch — per
non-trace row of variant_table its cases, 130 seeds each against the oracle on all 48 result bytes.  Which build a case runs on depends, on
the device, on the CU count, the LDS budget and the builds' register counts as well as on the limits: so every case asserts the build the
DEVICE library's geometry selects for it before it runs, and that no seed of the pass came back a runner verdict — nothing is compared on a
re-run's build.  That the cases of a row poll every opcode the row compiles is the oracle's statement about these same seeds
(tests/test_emu_build_matrix.py); the device equals the oracle seed for seed, so it holds here.

What the emulation cannot check is the device compilation of each handler in each build: its register allocation and spills, the
global-state builds' buffer accesses, the narrow entries, the compile-time lane strides.  `-s` prints the realised builds
(profiles/build_matrix.md)."""
import pytest

from madsim_amd import _abi as A
from tests import build_cases as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", list(B.ROWS))
def test_build_matrix_gpu(hip, row):
    seen = []

    def check(row, w, lim):
        g = B.check_variant(row, w, lim)
        seen.append((g.lanes_per_wave, g.heap_lds_slots, g.heap_spill_slots))

    n = B.run_row(row, lambda *a: hip.run_batch(*a)[0], check=check)
    lanes, lds, spill = (sorted(set(x)) for x in zip(*seen))
    print(f"[build matrix] {row}: {B.ROWS[row].variant}: {n} cases, seed lanes {lanes}, heap entries in LDS {lds}, spilled {spill}")


@pytest.mark.parametrize("row", list(B.TRACE_ROWS))
def test_trace_rows_gpu(hip, row):
    """The trace builds, on the cases of the LDS-resident row of their tier, one launch per case and no resolve round: the raw determinism
    log and the observation log of each seed, byte for byte against the oracle's, and the 48 result bytes.  (A trace launch runs the trace
    shape of the tier the geometry names: asserted from the device library's geometry.)"""
    n = 0
    for name, cs, w, cfg, lim, seeds in B.trace_truth(row):
        g = hip.geometry(w, lim)
        tier = sum(f for bit, f in A.VARIANT_TIER_FEAT if g.variant & bit)
        assert tier == B.TRACE_ROWS[row][0][3] & (B.TIERS | B.SIGNAL), (row, name, tier)
        cap = max(len(log) for _, log, _, _ in seeds) + 64
        got = hip.trace_seeds(w, [s for s, *_ in seeds], cfg, lim, obs_cap=64, log_cap=cap, resolve=None)
        for t, (seed, log, obs, res) in zip(got, seeds):
            assert t.result.astuple() == res, (row, name, cs, seed, t.result.astuple(), res)
            assert t.log_len == len(log) and t.log == log, (row, name, cs, seed, t.log_len, len(log))
            assert t.n_observations == len(obs) <= 64 and t.observations == obs, (row, name, cs, seed, t.observations, obs)
        n += 1
    print(f"[build matrix] {row}: {B._v(*B.TRACE_ROWS[row][0][1:], trace=True)}: {n} cases of {B.TRACE_SEEDS} seeds, logs and observations byte for byte")
