"""What a poll pass of the base-op kernels holds fixed, on the host-compiled kernel (tests/emu) against the oracle.

The builds that keep the determinism log fold the clock ONCE per pass, where the ready-queue draw begins, and every log entry of the pass
reads Lane::clock_fold (k_rng.h ClockFold); the register-ready-queue builds pop a queue of one without swap_remove's shifts when the vote
gen_index needs says every lane holds one task (k_main.h PopOne).  The host-compiled kernel asserts at every use that the cached fold IS the
fold of the clock, and on the short pop that the index is 0 and the general arithmetic would have left the queue empty: a broken invariant is
MADSIM_INTERNAL.  Every case runs in eight layouts, one per build the two forms changed (tests/pass_invariant_cases.py LAYOUTS), the
benchmark's compact build first; each case asserts that its limits select exactly that build.
(One emulated lane at a time: the vote is the lane's own predicate here, so a lane takes the short pop exactly when ITS queue holds one task;
lanes of one wave voting differently is the device's case, tests/test_gpu_pass_invariants.py.)"""
import pytest

from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import emu, parity
from tests import pass_invariant_cases as PC


def _run(w, cfg, lim, layout, count, what):
    PC.check_variant(w, lim, layout, emu)
    final, want = parity.emu_compare(emu, w, PC.SEED0, count, cfg, lim, what=what)
    assert not (final["verdict"] == A.INTERNAL).any(), (what, "an invariant of the pass broke", final[final["verdict"] == A.INTERNAL][0])
    assert not (final["verdict"] == A.OVERFLOW).any(), what
    return want


@pytest.mark.parametrize("layout", list(PC.LAYOUTS))
@pytest.mark.parametrize("nodes,loss", PC.PINGPONG)
def test_pingpong_pass_invariants(nodes, loss, layout):
    """Ping-pong at 2, 4 and 6 nodes, three rounds, 192 seeds, without loss and at 5 %: all 48 result bytes of every seed — trace_hash, which
    the cached fold feeds, among them (0 in the two layouts without the log).  Under loss seeds deadlock early, so the lanes of a wave sit at
    different passes and clocks."""
    want = _run(W.pingpong(nodes, PC.ROUNDS), PC.config(loss), PC.limits(layout, nodes), layout, PC.SEEDS, (nodes, loss, layout))
    assert (want["trace_hash"] != 0).all() != layout.endswith("nolog")
    if loss:
        assert {A.PASS, A.DEADLOCK} <= set(want["verdict"].tolist())
        assert len(set(want["steps"].tolist())) > 4
    else:
        assert (want["verdict"] == A.PASS).all()


def test_start_up_of_six_nodes_queues_six_tasks():
    """The 6-node cases above begin on the general side of the pop: the main task spawns six tasks (the oracle's high-water mark)."""
    assert (PC.max_ready_by_seed(W.pingpong(6, PC.ROUNDS), PC.SEED0, 8) == 6).all()


@pytest.mark.parametrize("layout", list(PC.LAYOUTS))
def test_queue_of_two_beside_queues_of_one(layout):
    """Both sides of the pop among the lanes of every wave: the tie workload's queue holds two tasks only where two timers fire in one idle
    jump — by the oracle's high-water marks in some seeds of every 32 and not in the others.  200 seeds: the last wave is a partial one."""
    w = PC.tie_workload()
    PC.assert_ties_in_every_wave(PC.max_ready_by_seed(w, PC.SEED0, PC.SEEDS_TIE))
    want = _run(w, None, PC.limits(layout, 2), layout, PC.SEEDS_TIE, ("ties", layout))
    assert (want["verdict"] == A.PASS).all()
