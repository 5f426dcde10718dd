"""What a poll pass of the base-op kernels holds fixed, on the device: the workloads, layouts and seed counts of
tests/test_emu_pass_invariants.py through tests/parity.py, every seed of every lane against the oracle on all 48 result bytes — on each of
the eight builds the two forms changed, the benchmark's compact build among them (each case asserts which build its limits select).

Here the vote is a wave's: the short accept test and the short pop (k_rng.h gen_index, k_main.h PopOne) run only when EVERY lane of the wave
holds one queued task, and a lane with a queue of one goes through the general swap_remove beside a neighbour whose queue holds two.  The
cached clock fold (k_rng.h ClockFold) feeds trace_hash, one of the fields compared."""
import pytest

from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import parity
from tests import pass_invariant_cases as PC

pytestmark = pytest.mark.gpu


def _run(hip, w, cfg, lim, layout, count, what):
    PC.check_variant(w, lim, layout)
    final, want = parity.gpu_compare(hip, w, PC.SEED0, count, cfg, lim, what=what)
    assert not (final["verdict"] == A.INTERNAL).any(), what
    assert not (final["verdict"] == A.OVERFLOW).any(), what
    return want


@pytest.mark.parametrize("layout", list(PC.LAYOUTS))
@pytest.mark.parametrize("nodes,loss", PC.PINGPONG)
def test_pingpong_pass_invariants_gpu(hip, nodes, loss, layout):
    want = _run(hip, W.pingpong(nodes, PC.ROUNDS), PC.config(loss), PC.limits(layout, nodes), layout, PC.SEEDS, (nodes, loss, layout))
    assert (want["trace_hash"] != 0).all() != layout.endswith("nolog")
    if loss:
        assert {A.PASS, A.DEADLOCK} <= set(want["verdict"].tolist())
    else:
        assert (want["verdict"] == A.PASS).all()


@pytest.mark.parametrize("layout", list(PC.LAYOUTS))
def test_queue_of_two_beside_queues_of_one_gpu(hip, layout):
    """Start-up of the 6-node ping-pong (six queued tasks in every lane: the whole wave on the general side) rides in the test above; the tie
    workload puts a queue of two beside queues of one in every wave — the oracle's high-water marks say in which seeds — and its 200 seeds
    leave the last wave a partial one (eight lanes at 64 per wave)."""
    w = PC.tie_workload()
    PC.assert_ties_in_every_wave(PC.max_ready_by_seed(w, PC.SEED0, PC.SEEDS_TIE))
    want = _run(hip, w, None, PC.limits(layout, 2), layout, PC.SEEDS_TIE, ("ties", layout))
    assert (want["verdict"] == A.PASS).all()
