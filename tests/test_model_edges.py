"""The workload model AT its ceilings, on the CPU: what the oracle says about the directed workloads tests/test_model_edges_gpu.py runs on
the device, and the host-compiled kernel on the same workloads.

tests/test_oracle_model_limits.py holds every workload that goes one OVER a ceiling against the oracle; here are the ones that stand AT it
(no event of the workload model on any seed: the device owes the oracle's bytes), the ceilings that had no directed workload (each as a
pair: at, over), the base-op mailbox, the loss-rate mix the campaign tests use and the workload of the largest per-seed state."""
import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from tests import emu, parity
from tests import lifecycle_workloads as LW

PAIRS = LW.model_edge_pairs()
BASE_AT, BASE_OVER, BASE_LIM = LW.base_op_mailbox_pair()
AT = LW.model_at_ceiling_workloads() + [(name + "_at", w_at, lim, 0) for name, w_at, _, lim, _ in PAIRS] + [("base_op_mailbox_127", BASE_AT, BASE_LIM, 0)]
OVER = [(name + "_over", w_over, lim, bit) for name, _, w_over, lim, bit in PAIRS] + LW.model_exactly_one_over_workloads()


def _global(lim):
    g = A.Limits()
    for f, _ in A.Limits._fields_:
        setattr(g, f, getattr(lim, f))
    g.lanes_per_wave, g.state_mem = 0, A.STATE_GLOBAL
    return g


@pytest.mark.parametrize("case", AT, ids=lambda c: c[0])
def test_at_the_ceiling_no_seed_leaves_the_model(case):
    name, w, lim, _ = case
    pure, ev = oracle.run_batch_pure(w, 0, 64, None, lim)
    on, _ = oracle.run_batch(w, 0, 64, None, lim)
    assert not ev.any(), (name, ev)
    assert (on == pure).all()
    assert (pure["verdict"] == A.PASS).all() and pure["steps"].all() and pure["rng_calls"].all()
    assert len(np.unique(pure["rng_calls"])) >= 8, name                 # the seeds are not copies of one run


@pytest.mark.parametrize("case", OVER, ids=lambda c: c[0])
def test_one_over_is_an_event_of_the_pure_run_and_a_verdict_of_the_model_run(case):
    name, w, lim, bit = case
    on, _ = oracle.run_batch(w, 0, 16, None, lim)
    pure, ev = oracle.run_batch_pure(w, 0, 16, None, lim)
    assert (ev == bit).all(), (name, ev)
    assert (on["verdict"] == A.UNSUPPORTED).all() and not on["steps"].any()
    assert (pure["verdict"] <= A.TIME_LIMIT).all() and pure["steps"].all() and pure["rng_calls"].all()
    assert (oracle.expected_of_pure(pure, ev) == on).all()


def test_base_op_mailbox_is_no_ceiling_of_the_oracle():
    """127 and 128 datagrams queued for a socket of a base-op workload: the oracle passes both without an event — the 128th is a capacity of
    the device's base-op mailbox header alone (include/madsim_hip.h: the capacity verdict that stays one)."""
    for w in (BASE_AT, BASE_OVER):
        pure, ev = oracle.run_batch_pure(w, 0, 64, None, BASE_LIM)
        assert not ev.any() and (pure["verdict"] == A.PASS).all() and (oracle.run_batch(w, 0, 64, None, BASE_LIM)[0] == pure).all()


def test_the_mix_leaves_the_model_on_about_every_second_seed():
    w, cfg, lim = LW.model_mix_workload()
    on, _ = oracle.run_batch(w, 0, 1024, cfg, lim)
    pure, ev = oracle.run_batch_pure(w, 0, 1024, cfg, lim)
    assert (oracle.expected_of_pure(pure, ev) == on).all()
    n = np.bincount(on["verdict"], minlength=8)
    assert n[A.PASS] >= 256 and n[A.UNSUPPORTED] >= 256 and n[A.PASS] + n[A.UNSUPPORTED] == 1024, n
    assert (ev[on["verdict"] == A.UNSUPPORTED] == 4096).all()


def test_top_of_state_region_workload():
    """60 addresses, both exchanges arrive (the two payloads are observed), a score of steps, no event."""
    w, lim = LW.top_of_state_region()
    assert w.struct.n_socks == 60
    pure, ev = oracle.run_batch_pure(w, 0, 64, None, lim)
    assert not ev.any() and (pure["verdict"] == A.PASS).all() and (pure["steps"] >= 20).all() and (pure["steps"] < 64).all()
    assert (pure["msg_count"] == 2).all() and len(np.unique(pure["rng_calls"])) >= 8
    assert (oracle.run_batch(w, 0, 64, None, lim)[0] == pure).all()


def test_host_compiled_kernel_at_the_ceilings():
    """The host-compiled kernel on every at-ceiling workload (the oracle's bytes) and on the new over-ceiling ones (MADSIM_UNSUPPORTED), both
    layouts, two seeds each; the base-op mailbox's 128th message is MADSIM_OVERFLOW at its own ceiling of 127 as at the defaults."""
    top_w, top_lim = LW.top_of_state_region()
    for name, w, lim, _ in AT + OVER + [("top_of_state_region", top_w, top_lim, 0)]:
        want = parity.expected(w, 5, 2, None, lim)
        for glob in (0, 1):
            e = emu.run_batch(w, 5, 2, None, _global(lim) if glob else lim)
            assert (e == want).all(), (name, glob, e[0], want[0])
    for lim in (A.Limits(), BASE_LIM, _global(BASE_LIM)):
        e = emu.run_batch(BASE_OVER, 5, 2, None, lim)
        assert (e["verdict"] == A.OVERFLOW).all(), e[0]


def test_the_base_op_ladder_ends_at_127():
    """run_batch_auto and the resolving campaigns double mbox_msgs round by round.  A workload without extended ops has no build for more than
    127 queued messages (the geometry refuses it), so its ladder ends at 127: every rung has a geometry and the last one holds what the
    127-datagram workload needs.  (It went on to 128 and 255: the sixth round failed the whole call with MADSIM_E_LIMITS, and a base-op
    workload that needs 65 .. 127 queued messages could not be resolved from the defaults.)  tests/parity.py grows the same way."""
    from madsim_amd import runtime
    assert parity.msgs_ceiling(BASE_AT) == 127 == parity.msgs_ceiling(BASE_OVER)
    py = A.Limits()
    for r in range(1, 10):
        g = runtime.grown_limits(BASE_OVER, None, r)
        py = parity.grow(py, BASE_OVER.struct.n_progs, 127)
        assert g.mbox_msgs == min(2 << r, 127) == py.mbox_msgs and g.mbox_regs == min(2 << r, 255) == py.mbox_regs, r
        runtime.geometry(BASE_OVER, g)
    assert runtime.grown_limits(BASE_OVER, BASE_LIM, 3).mbox_msgs == 127
    w, _, _ = LW.model_mix_workload()                       # with an extended op the ceiling is 255, as before
    assert parity.msgs_ceiling(w) == 255 and [runtime.grown_limits(w, None, r).mbox_msgs for r in (6, 7, 8)] == [128, 255, 255]
    big = A.Limits(); big.mbox_msgs = 128                   # asked for outright it is still refused
    with pytest.raises(runtime.MadsimHipError, match="without extended ops"):
        runtime.geometry(BASE_OVER, big)
    # the host-compiled kernel up the ladder, seed by seed: 127 datagrams settle with the oracle's bytes, the 128th stays MADSIM_OVERFLOW
    want = parity.expected(BASE_AT, 5, 2, None, BASE_LIM)
    first = emu.run_batch(BASE_AT, 5, 2, None, A.Limits())
    assert (first["verdict"] == A.OVERFLOW).all()
    assert (parity.resolve_seed_by_seed(emu.run_batch, BASE_AT, 5, first, None, A.Limits()) == want).all()
    first = emu.run_batch(BASE_OVER, 5, 2, None, A.Limits())
    assert (parity.resolve_seed_by_seed(emu.run_batch, BASE_OVER, 5, first, None, A.Limits())["verdict"] == A.OVERFLOW).all()
