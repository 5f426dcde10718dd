"""Cold launch parameters on the device: the base-op kernels read the fields of their parameter block that are used once per seed, once per
many passes or on rare sides only from the kernel-argument segment, at the field's offset, where they are used (k_state.h ColdParams / PCOLD).
The host-compiled kernel reads P.f, so these cases carry the proof: the ordinary workloads on every changed build, and one case per cold site
— the seed list, the work queue, static striding past the launch's lanes, a seed0 above 2^32, the capacity, step and time verdicts, buggify, and
two launches on one stream that must each read their own block — on the benchmark's build and on an LDS-queue build.  Every seed against the
oracle on all 48 result bytes; each case asserts which build its limits select."""
import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from tests import cold_param_cases as CC
from tests import parity
from tests import pass_invariant_cases as PC
from tests import seedlist_ref as S
from tests import groups_ref as G

pytestmark = pytest.mark.gpu


def _run(hip, w, cfg, lim, layout, seed0, count, what):
    CC.check_variant(w, lim, layout)
    final, want = parity.gpu_compare(hip, w, seed0, count, cfg, lim, what=what)
    assert not (final["verdict"] == A.INTERNAL).any(), what
    return final, want


def test_first_contact_one_wave_of_the_headline_build(hip):
    """64 seeds, the benchmark's layout: the smallest launch that reads every cold field of an ordinary run."""
    final, want = _run(hip, CC.pingpong(4), None, CC.limits("compact", 4), "compact", CC.SEED0, CC.FIRST, "first contact")
    assert (want["verdict"] == A.PASS).all() and (final["trace_hash"] != 0).all()


@pytest.mark.parametrize("layout", list(CC.LAYOUTS))
@pytest.mark.parametrize("nodes,loss", PC.PINGPONG)
def test_pingpong_cold_params_gpu(hip, nodes, loss, layout):
    final, want = _run(hip, CC.pingpong(nodes), PC.config(loss), CC.limits(layout, nodes), layout, CC.SEED0, PC.SEEDS, (nodes, loss, layout))
    assert not (final["verdict"] == A.OVERFLOW).any() and (final["trace_hash"] != 0).all() != layout.endswith("nolog")
    assert ({A.PASS, A.DEADLOCK} <= set(want["verdict"].tolist())) if loss else (want["verdict"] == A.PASS).all()


@pytest.mark.parametrize("layout", list(CC.LAYOUTS))
def test_tied_timers_cold_params_gpu(hip, layout):
    final, want = _run(hip, PC.tie_workload(), None, CC.limits(layout, 2), layout, CC.SEED0, PC.SEEDS_TIE, ("ties", layout))
    assert (want["verdict"] == A.PASS).all()


@pytest.mark.parametrize("layout", CC.COLD_LAYOUTS)
def test_seed_list_gpu(hip, layout):
    """P.seed_list: 130 non-contiguous seeds through the corpus entry point.  Grouped by trace_hash every seed is a group of its own, so the report
    names each seed with its verdict and its hash; the campaign's totals hold the steps and clocks."""
    w, cfg, lim, seeds = CC.pingpong(), PC.config(0.05), CC.limits(layout, 2), CC.seed_list()
    CC.check_variant(w, lim, layout)
    want = CC.oracle_of_list(w, seeds, cfg, lim)
    assert len(seeds) == 130 and len(set(want["trace_hash"].tolist())) == 130 and {A.PASS, A.DEADLOCK} <= set(want["verdict"].tolist())
    include = (A.PASS, A.PANIC, A.DEADLOCK, A.TIME_LIMIT)
    rep, fails, hist, grp = hip.run_campaign_seeds(w, seeds, config=cfg, limits=lim, collect=130, list_runner=True, groups=(include, "trace", 256))
    assert S.of_campaign(rep) == S.campaign_truth(want, seeds)
    words, rec_bytes = S.collect_truth(want, seeds, 130, 1)
    assert fails.tobytes() == rec_bytes and [int(x) for x in hist] == [int(x) for x in words[6:14]]
    assert G.of_report(grp) == S.groups_truth(want, seeds, 0xf, A.GROUP_KEY_TRACE, 256)


@pytest.mark.parametrize("sched", [A.SCHED_STATIC, A.SCHED_QUEUE])
@pytest.mark.parametrize("layout", CC.COLD_LAYOUTS)
def test_more_seeds_than_lanes_gpu(hip, layout, sched):
    """ONE launch of 2 048 seeds more than the device has lanes for this layout: 2 048 lanes take a second unit, by `next += total_lanes` or from
    the per-launch work queue (P.work_ctr, P.total_lanes).  Lossy, so lanes finish at different times.  Through the device-resident entry
    point, which queues the whole count as a single launch (madsim_hip_run_batch cuts a call of more than 98 304 seeds into launches of
    65 536, none of which has more seeds than lanes); that launch's total_lanes is the device fill, because its count is above it."""
    import torch
    w, lim, cfg = CC.pingpong(), CC.limits(layout, 2), PC.config(0.05)
    lim.sched = sched
    CC.check_variant(w, lim, layout)
    lanes = CC.lanes_of_launch(hip, w, lim)
    count = lanes + 2048
    assert 0 < lanes < count                                # the launch's grid is capped at `lanes`: count - lanes second units
    buf = torch.zeros(count * 48, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    summ = hip.run_batch_device(w, CC.SEED0_HIGH, count, buf.data_ptr(), st.cuda_stream, cfg, lim)
    st.synchronize()
    got = np.frombuffer(buf.cpu().numpy().tobytes(), dtype=A.RESULT_DTYPE)
    want, osumm = oracle.run_batch(w, CC.SEED0_HIGH, count, cfg, lim)
    assert (got == want).all(), (lanes, int((got != want).sum()))
    assert (summ.n_failed, summ.total_steps) == (osumm.n_failed, osumm.total_steps) and summ.n_failed > 0


@pytest.mark.parametrize("layout", CC.COLD_LAYOUTS)
def test_seed0_above_2_32_gpu(hip, layout):
    _run(hip, CC.pingpong(), None, CC.limits(layout, 2), layout, CC.SEED0_HIGH, PC.SEEDS, ("seed0", layout))


@pytest.mark.parametrize("layout", CC.COLD_LAYOUTS)
def test_capacity_overflow_gpu(hip, layout):
    w, lim = CC.pingpong(6), CC.overflow_limits(layout, 6)
    CC.check_variant(w, lim, layout)
    first, _ = hip.run_batch(w, CC.SEED0, PC.SEEDS, None, lim)
    assert (first["verdict"] == A.OVERFLOW).all()
    parity.gpu_compare(hip, w, CC.SEED0, PC.SEEDS, None, lim, what=("overflow", layout))     # ... and the re-run is the oracle's


@pytest.mark.parametrize("layout", CC.COLD_LAYOUTS)
def test_step_limit_gpu(hip, layout):
    final, want = _run(hip, CC.pingpong(), None, CC.step_limits(layout), layout, CC.SEED0, PC.SEEDS, ("max_steps", layout))
    assert (want["verdict"] == A.STEP_LIMIT).all()


@pytest.mark.parametrize("layout", CC.COLD_LAYOUTS)
def test_time_limit_ends_lossy_seeds_gpu(hip, layout):
    final, want = _run(hip, CC.pingpong(), PC.config(0.05), CC.time_limits(layout), layout, CC.SEED0, PC.SEEDS, ("time_limit", layout))
    assert {A.PASS, A.TIME_LIMIT} <= set(want["verdict"].tolist())


@pytest.mark.parametrize("loss", (0.0, 0.05))
@pytest.mark.parametrize("layout", CC.BUGGIFY_LAYOUTS)
def test_buggify_gpu(hip, layout, loss):
    cfg = A.Config.default(packet_loss_rate=loss, buggify=True)
    _run(hip, CC.pingpong(), cfg, CC.limits(layout, 2), layout, CC.SEED0, PC.SEEDS, ("buggify", layout, loss))


@pytest.mark.parametrize("layout", CC.COLD_LAYOUTS)
def test_two_launches_on_one_stream_read_their_own_blocks_gpu(hip, layout):
    """Two launches queued back to back on one stream with different seed0 and count: the second kernel's cold reads come from its own
    kernel-argument block, not the first's."""
    import torch
    w, lim = CC.pingpong(), CC.limits(layout, 2)
    CC.check_variant(w, lim, layout)
    launches = ((CC.SEED0, 192), (CC.SEED0_HIGH, 77))
    bufs = [torch.zeros(n * 48, dtype=torch.uint8, device="cuda") for _, n in launches]
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for (s0, n), buf in zip(launches, bufs):
        hip.run_batch_async(w, s0, n, buf.data_ptr(), 0, st.cuda_stream, None, lim)
    st.synchronize()
    for (s0, n), buf in zip(launches, bufs):
        got = np.frombuffer(buf.cpu().numpy().tobytes(), dtype=A.RESULT_DTYPE)
        want, _ = oracle.run_batch(w, s0, n, None, lim)
        assert (got == want).all(), (s0, n)
