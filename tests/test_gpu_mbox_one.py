"""The short mailbox forms on the device (sim_kernel.h MADSIM_MBOX_ONE): the cases of tests/mbox_one_cases.py on the nine base-op builds, each at the
mailbox setting the short side is for and at the two nearest that keep the general side — the same build, another side of one scalar branch.  Every
seed against the oracle on all 48 result bytes; each case asserts which build its limits select.

The tied-timer workload fires two timers of one seed in one call beside seeds that fire one — a queue of two beside queues of one in every wave —
and its 200 seeds leave the last wave a partial one."""
import pytest

from madsim_amd import _abi as A
from tests import cold_param_cases as CC
from tests import groups_ref as G
from tests import mbox_one_cases as MC
from tests import parity
from tests import pass_invariant_cases as PC
from tests import seedlist_ref as S

pytestmark = pytest.mark.gpu


def _run(hip, name, arg, loss, layout, setting, tasks, count=MC.SEEDS):
    w, cfg, want = MC.case(name, arg, loss, layout, count)
    lim = MC.limits(layout, tasks, setting)
    CC.check_variant(w, lim, layout)
    what = (name, arg, loss, layout, setting)
    got, final = MC.compare(lambda *a: hip.run_batch(*a)[0], lambda got: parity.resolve_with_auto(hip.run_batch_auto, w, MC.SEED0, count, cfg, lim),
                            w, cfg, lim, want, count, what)
    return got, want


def test_first_contact_one_wave_of_the_headline_build(hip):
    """64 seeds of the 2-node ping-pong on the benchmark's layout and limits: the smallest launch that takes the short delivery and the short
    registration."""
    got, want = _run(hip, "pingpong", 2, 0.0, "compact", "one", 2, MC.FIRST)
    assert (got == want).all() and (want["verdict"] == A.PASS).all() and (got["trace_hash"] != 0).all()


@pytest.mark.parametrize("setting", list(MC.SETTINGS))
@pytest.mark.parametrize("layout", list(MC.LAYOUTS))
@pytest.mark.parametrize("nodes,loss", PC.PINGPONG)
def test_pingpong_mbox_one_gpu(hip, nodes, loss, layout, setting):
    got, want = _run(hip, "pingpong", nodes, loss, layout, setting, nodes)
    assert not (got["verdict"] == A.OVERFLOW).any()
    assert ({A.PASS, A.DEADLOCK} <= set(want["verdict"].tolist())) if loss else (want["verdict"] == A.PASS).all()


@pytest.mark.parametrize("setting", list(MC.SETTINGS))
@pytest.mark.parametrize("layout", list(MC.LAYOUTS))
def test_tied_timers_mbox_one_gpu(hip, layout, setting):
    """A queue of two beside queues of one in every wave (the oracle's high-water marks say in which seeds), a partial last wave."""
    w, _, _ = MC.case("ties", count=MC.SEEDS_TIE)
    PC.assert_ties_in_every_wave(PC.max_ready_by_seed(w, MC.SEED0, MC.SEEDS_TIE))
    got, want = _run(hip, "ties", 0, 0.0, layout, setting, 2, MC.SEEDS_TIE)
    assert (want["verdict"] == A.PASS).all() and not (got["verdict"] == A.OVERFLOW).any()


@pytest.mark.parametrize("layout", list(MC.LAYOUTS))
@pytest.mark.parametrize("name", list(MC.RUNNER))
def test_runner_verdicts_gpu(hip, name, layout):
    """A second registration on a full list, a datagram with no receiver and no queue: MADSIM_OVERFLOW in every seed on the short side AND on the
    general side; the oracle passes every seed, and the library's re-run with grown capacities is the oracle's.  One slot more: no capacity verdict."""
    _, tasks, full, roomy = MC.RUNNER[name]
    for setting in full:
        got, want = _run(hip, name, 0, 0.0, layout, setting, tasks)
        assert (got["verdict"] == A.OVERFLOW).all() and (want["verdict"] == A.PASS).all(), (name, layout, setting)
    for setting in roomy:
        got, want = _run(hip, name, 0, 0.0, layout, setting, tasks)
        assert (got == want).all(), (name, layout, setting)


@pytest.mark.parametrize("setting", list(MC.SETTINGS))
def test_seed_list_gpu(hip, setting):
    """130 non-contiguous seeds of the lossy ping-pong through the corpus entry point (madsim_hip_run_seeds_campaign) on the benchmark's layout."""
    w, cfg, lim, seeds = CC.pingpong(), PC.config(0.05), MC.limits("compact", 2, setting), CC.seed_list()
    CC.check_variant(w, lim, "compact")
    want = CC.oracle_of_list(w, seeds, cfg, lim)
    assert len(seeds) == 130 and {A.PASS, A.DEADLOCK} <= set(want["verdict"].tolist())
    include = (A.PASS, A.PANIC, A.DEADLOCK, A.TIME_LIMIT)
    rep, fails, hist, grp = hip.run_campaign_seeds(w, seeds, config=cfg, limits=lim, collect=130, list_runner=True, groups=(include, "trace", 256))
    assert S.of_campaign(rep) == S.campaign_truth(want, seeds)
    words, rec_bytes = S.collect_truth(want, seeds, 130, 1)
    assert fails.tobytes() == rec_bytes and [int(x) for x in hist] == [int(x) for x in words[6:14]]
    assert G.of_report(grp) == S.groups_truth(want, seeds, 0xf, A.GROUP_KEY_TRACE, 256)
