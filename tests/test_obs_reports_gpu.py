"""The observation census and the probe-set census run under one chunk driver on the host and keep one buffer group each on a context
(madsim_hip.cpp: obs_report_run, madsim_hip_resources::ObsReport).  What that sharing could break is one form's state leaking into the
other's, or into its own next call: a table regrown or left unclean, a `dirty` flag, a report half filled by a call that failed.  So the
two forms are interleaved on ONE context — a small table, the other form, the table regrown, a call that fails over its cap, both forms
again — and every report must be, byte for byte, what a fresh context that made only that call reports."""
import pytest

from madsim_amd import _abi as A
from madsim_amd import runtime
from tests import test_census as TC
from tests import test_probe_sets as TP

pytestmark = pytest.mark.gpu

SEEDS, CHUNK = 300, 64                                                             # five chunks, the last of 44


def test_both_forms_interleaved_on_one_context_report_what_a_fresh_context_reports(hip):
    w, cfg, seed0 = TC.probe_pingpong_workload(), A.Config.default(packet_loss_rate=TP.PROBE_LOSS), TP.PROBE_SEED0
    rnd_w, rnd_cfg = TC.random_value_workload(), A.Config.default()
    census = lambda ctx, max_values: ctx.census(w, seed0, SEEDS, max_values=max_values, config=cfg, chunk=CHUNK)           # noqa: E731
    probe_sets = lambda ctx: ctx.probe_sets(w, TP.PROBE_VOCAB, seed0, SEEDS, config=cfg, chunk=CHUNK)                      # noqa: E731
    fresh = {}
    for name, call in (("census8", lambda c: census(c, 8)), ("census4096", lambda c: census(c, 4096)), ("sets", probe_sets)):
        with runtime.Context(0) as ctx:                                            # a context that makes only this call
            fresh[name] = call(ctx)
    assert [int(v) for v in fresh["census8"].values["value"]] == [0x10, 0x11, 0x20, 0x21] and sum(fresh["census8"].n_counted) == SEEDS
    assert len(fresh["sets"]) >= 2 and sum(fresh["sets"].n_counted) == SEEDS      # (neither report is empty)
    assert fresh["census8"].tobytes() == fresh["census4096"].tobytes()
    with runtime.Context(0) as ctx:
        assert census(ctx, 8).tobytes() == fresh["census8"].tobytes()
        assert probe_sets(ctx).tobytes() == fresh["sets"].tobytes()
        assert census(ctx, 4096).tobytes() == fresh["census4096"].tobytes()        # the table is regrown
        for chunk in (TC.RANDOM_SEEDS, 4):                                         # refused on the device; by the host fold, two chunks folded before
            with pytest.raises(runtime.MadsimHipError, match="probe vocabulary"):
                ctx.census(rnd_w, 0, TC.RANDOM_SEEDS, max_values=TC.RANDOM_MAX_VALUES, config=rnd_cfg, chunk=chunk)
        assert census(ctx, 8).tobytes() == fresh["census8"].tobytes()
        assert probe_sets(ctx).tobytes() == fresh["sets"].tobytes()
