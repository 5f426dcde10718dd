"""The short mailbox forms (sim_kernel.h MADSIM_MBOX_ONE) on the host-compiled kernel (tests/emu) against the oracle.

The host-compiled kernel runs the short forms and, at every use, holds them against what the general arithmetic makes of the same inputs — the
header word, the stored registration, the receiver's words, the liveness test one bit away in each of its parts — a mismatch is MADSIM_INTERNAL,
which every case here asserts no seed ends with."""
import pytest

from madsim_amd import _abi as A
from tests import cold_param_cases as CC
from tests import emu, parity
from tests import mbox_one_cases as MC
from tests import pass_invariant_cases as PC


def _run(name, arg, loss, layout, setting, tasks, count=MC.SEEDS):
    w, cfg, want = MC.case(name, arg, loss, layout, count)
    lim = MC.limits(layout, tasks, setting)
    CC.check_variant(w, lim, layout, emu)
    what = (name, arg, loss, layout, setting)
    got, final = MC.compare(emu.run_batch, lambda got: parity.resolve_seed_by_seed(emu.run_batch, w, MC.SEED0, got, cfg, lim), w, cfg, lim, want, count, what)
    return got, want


@pytest.mark.parametrize("setting", list(MC.SETTINGS))
@pytest.mark.parametrize("layout", list(MC.LAYOUTS))
@pytest.mark.parametrize("nodes,loss", PC.PINGPONG)
def test_pingpong_mbox_one(nodes, loss, layout, setting):
    got, want = _run("pingpong", nodes, loss, layout, setting, nodes)
    assert not (got["verdict"] == A.OVERFLOW).any()                  # a ping-pong registers before its datagram arrives: one slot is enough
    assert ({A.PASS, A.DEADLOCK} <= set(want["verdict"].tolist())) if loss else (want["verdict"] == A.PASS).all()


@pytest.mark.parametrize("setting", list(MC.SETTINGS))
@pytest.mark.parametrize("layout", list(MC.LAYOUTS))
def test_tied_timers_mbox_one(layout, setting):
    got, want = _run("ties", 0, 0.0, layout, setting, 2, MC.SEEDS_TIE)
    assert (want["verdict"] == A.PASS).all() and not (got["verdict"] == A.OVERFLOW).any()


@pytest.mark.parametrize("layout", list(MC.LAYOUTS))
@pytest.mark.parametrize("name", list(MC.RUNNER))
def test_runner_verdicts(name, layout):
    """A second registration on a full list, a datagram with no receiver and no queue: MADSIM_OVERFLOW in every seed on the short side AND on the
    general side; the oracle passes every seed, and the re-run with grown capacities is the oracle's.  One slot more: no capacity verdict."""
    _, tasks, full, roomy = MC.RUNNER[name]
    for setting in full:
        got, want = _run(name, 0, 0.0, layout, setting, tasks)
        assert (got["verdict"] == A.OVERFLOW).all() and (want["verdict"] == A.PASS).all(), (name, layout, setting)
    for setting in roomy:
        got, want = _run(name, 0, 0.0, layout, setting, tasks)
        assert (got == want).all(), (name, layout, setting)
