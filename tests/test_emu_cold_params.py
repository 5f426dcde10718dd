"""Cold launch parameters (k_state.h ColdParams / PCOLD) on the host-compiled kernel (tests/emu) against the oracle.

The host-compiled kernel compiles the gate off (ColdParams<K>::ON is false under MADSIM_EMU, PCOLD(f) is P.f), so these twins of
tests/test_gpu_cold_params.py say nothing about the device path: they show that the text around the cold reads — the loops written with a cold
bound, the verdict codes, the flag tests, the references to the main task's record — is, with the gate off, the logic it was, on the same
cases.  What the host-compiled kernel has no entry for (a seed list, two launches on one stream) has a device case only."""
import pytest

import oracle
from madsim_amd import _abi as A
from tests import cold_param_cases as CC
from tests import emu, parity
from tests import pass_invariant_cases as PC


def _run(w, cfg, lim, layout, seed0, count, what):
    CC.check_variant(w, lim, layout, emu)
    final, want = parity.emu_compare(emu, w, seed0, count, cfg, lim, what=what)
    assert not (final["verdict"] == A.INTERNAL).any(), what
    return final, want


@pytest.mark.parametrize("layout", list(CC.LAYOUTS))
@pytest.mark.parametrize("nodes,loss", PC.PINGPONG)
def test_pingpong_cold_params(nodes, loss, layout):
    final, want = _run(CC.pingpong(nodes), PC.config(loss), CC.limits(layout, nodes), layout, CC.SEED0, PC.SEEDS, (nodes, loss, layout))
    assert not (final["verdict"] == A.OVERFLOW).any() and (final["trace_hash"] != 0).all() != layout.endswith("nolog")
    assert ({A.PASS, A.DEADLOCK} <= set(want["verdict"].tolist())) if loss else (want["verdict"] == A.PASS).all()


@pytest.mark.parametrize("layout", list(CC.LAYOUTS))
def test_tied_timers_cold_params(layout):
    final, want = _run(PC.tie_workload(), None, CC.limits(layout, 2), layout, CC.SEED0, PC.SEEDS_TIE, ("ties", layout))
    assert (want["verdict"] == A.PASS).all()


@pytest.mark.parametrize("layout", CC.COLD_LAYOUTS)
def test_seed0_above_2_32(layout):
    final, want = _run(CC.pingpong(), None, CC.limits(layout, 2), layout, CC.SEED0_HIGH, PC.SEEDS, ("seed0", layout))
    low, _ = oracle.run_batch(CC.pingpong(), CC.SEED0_HIGH & 0xffffffff, PC.SEEDS, None, CC.limits(layout, 2))
    assert (want["trace_hash"] != low["trace_hash"]).any()          # the high half matters


@pytest.mark.parametrize("sched", [A.SCHED_STATIC, A.SCHED_QUEUE])
@pytest.mark.parametrize("layout", CC.COLD_LAYOUTS)
def test_more_seeds_than_lanes(layout, sched):
    """One CU of lanes (1 024 in the compact layout, 256 in the LDS-queue one) and 1 300 lossy seeds: every lane takes a second unit, by
    striding or from the work queue."""
    w, lim, cfg = CC.pingpong(), CC.limits(layout, 2), PC.config(0.05)
    lim.sched = sched
    CC.check_variant(w, lim, layout, emu)
    want, _ = oracle.run_batch(w, CC.SEED0, 1300, cfg, lim)
    assert (emu.run_batch(w, CC.SEED0, 1300, cfg, lim, num_cus=1) == want).all()


@pytest.mark.parametrize("layout", CC.COLD_LAYOUTS)
def test_capacity_overflow(layout):
    w, lim = CC.pingpong(6), CC.overflow_limits(layout, 6)
    CC.check_variant(w, lim, layout, emu)
    first = emu.run_batch(w, CC.SEED0, PC.SEEDS, None, lim)
    assert (first["verdict"] == A.OVERFLOW).all()
    parity.emu_compare(emu, w, CC.SEED0, PC.SEEDS, None, lim, what=("overflow", layout))     # ... and the re-run is the oracle's


@pytest.mark.parametrize("layout", CC.COLD_LAYOUTS)
def test_step_limit(layout):
    final, want = _run(CC.pingpong(), None, CC.step_limits(layout), layout, CC.SEED0, PC.SEEDS, ("max_steps", layout))
    assert (want["verdict"] == A.STEP_LIMIT).all()


@pytest.mark.parametrize("layout", CC.COLD_LAYOUTS)
def test_time_limit_ends_lossy_seeds(layout):
    final, want = _run(CC.pingpong(), PC.config(0.05), CC.time_limits(layout), layout, CC.SEED0, PC.SEEDS, ("time_limit", layout))
    assert {A.PASS, A.TIME_LIMIT} <= set(want["verdict"].tolist())


@pytest.mark.parametrize("loss", (0.0, 0.05))
@pytest.mark.parametrize("layout", CC.BUGGIFY_LAYOUTS)
def test_buggify(layout, loss):
    cfg = A.Config.default(packet_loss_rate=loss, buggify=True)
    final, want = _run(CC.pingpong(), cfg, CC.limits(layout, 2), layout, CC.SEED0, PC.SEEDS, ("buggify", layout, loss))
    plain, _ = oracle.run_batch(CC.pingpong(), CC.SEED0, PC.SEEDS, PC.config(loss) or A.Config.default(), CC.limits(layout, 2))
    assert (want["clock_ns"] != plain["clock_ns"]).any()            # the second draw happens in some seeds
