"""The timer heap at every LDS / spill boundary under tied deadlines, on the device: the matrix of tests/heap_cases.py through
hip.run_batch, every seed of every case against the oracle on all 48 result bytes, one test per layout over its workloads and quotas (each
case asserts the build its limits select and that no seed of the pass came back a runner verdict: nothing is compared on a re-run's build).

What the emulation (tests/test_emu_heap_boundaries.py) cannot check is the device compilation of these paths: ds_* beside buffer_* accesses,
the pair of children astride the boundary, the compact layout's register root, the 8-byte entries.  The realised boundaries of the
global-state layouts are the device library's here (geometry.h `fit` follows the build's register count): `-s` prints them."""
import pytest

from madsim_amd import _abi as A
from tests import heap_cases as H

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layout", list(H.LAYOUTS))
def test_heap_boundaries_gpu(hip, layout):
    H.run_layout(layout, lambda *a: hip.run_batch(*a)[0], lambda w, lim: hip.geometry(w, lim).heap_lds_slots, check=H.check_variant)


def test_trace_build_gpu(hip):
    """The trace build (every trace call of these workloads runs it): the raw determinism log of each seed, byte for byte against the
    oracle's, and the 48 result bytes — one launch per quota, no resolve round."""
    w = H.workload(H.TRACE_KEY)
    seeds = list(range(H.SEED0, H.SEED0 + H.TRACE_SEEDS))
    for q in H.TRACE_QUOTAS:
        want = H.trace_truth(q)
        cap = max(len(log) for log, _ in want) + 64
        got = hip.trace_seeds(w, seeds, None, H.quota_limits(H.TRACE_KEY[1], q), obs_cap=0, log_cap=cap, resolve=None)
        for t, (log, res) in zip(got, want):
            assert res[0] == A.PASS and t.result.astuple() == res, (q, t.seed, t.result.astuple(), res)
            assert t.log_len == len(log) and t.log == log, (q, t.seed, t.log_len, len(log))
