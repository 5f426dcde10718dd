"""The host-side truth of a grouping campaign (madsim_hip_run_campaign_groups): a filter, np.unique over (verdict, key), counts and first
indices.  Shared by tests/test_campaign_groups.py (which holds it against a plain-Python dict, and the library's host fold against it),
tests/test_group_kernels.py and tests/test_campaign_groups_gpu.py (which hold the GPU's answers against it) — a plain restatement of
include/madsim_hip.h, independent of the library."""
import functools

import numpy as np

import oracle
from madsim_amd import _abi as A
from madsim_amd import workload as W

U64_MAX = (1 << 64) - 1
FNV_BASIS = 0xCBF29CE484222325                                       # the obs_hash of a seed that traced nothing
KEY_FIELDS = ("obs_hash", "trace_hash", "msg_count", "clock_ns", "rng_calls", "steps")      # MADSIM_GROUP_KEY_OBS, _TRACE, _MSGS, _CLOCK, _RNG, _STEPS
FAILURES = 0b1110                                                    # PANIC | DEADLOCK | TIME_LIMIT
ALL = 0b1111


def counted(results, include):
    v = results["verdict"]
    return (v < 4) & (((include >> np.minimum(v, 31)) & 1) != 0)


def all_groups(results, seed0, include, key_field):
    """[(verdict, key, count, first_seed)] of every group of per-seed `results` of [seed0, seed0 + len), ascending by first_seed."""
    idx = np.nonzero(counted(results, include))[0]
    if not len(idx):
        return []
    sig = np.zeros(len(idx), dtype=[("verdict", "<u4"), ("key", "<u8")])
    sig["verdict"], sig["key"] = results["verdict"][idx], results[KEY_FIELDS[key_field]][idx].astype(np.uint64)
    uniq, first, counts = np.unique(sig, return_index=True, return_counts=True)      # first: of the first occurrence, idx is ascending
    order = np.argsort(first)
    return [(int(uniq["verdict"][j]), int(uniq["key"][j]), int(counts[j]), seed0 + int(idx[first[j]])) for j in order]


def groups_truth(results, seed0, include, key_field, cap):
    """{groups: the first `cap` of all_groups, n_grouped, n_ungrouped} — what madsim_groups_t holds after the campaign."""
    every = all_groups(results, seed0, include, key_field)
    kept = every[:cap]
    return {"groups": kept, "n_grouped": sum(g[2] for g in kept), "n_ungrouped": sum(g[2] for g in every[cap:])}


def of_array(groups):
    """An ndarray[A.GROUP_DTYPE] as a list of (verdict, key, count, first_seed), in the order given."""
    return [(int(g["verdict"]), int(g["key"]), int(g["count"]), int(g["first_seed"])) for g in groups]


def of_report(rep):
    """A runtime.CampaignGroups in the shape of groups_truth's answer."""
    return {"groups": of_array(rep.groups), "n_grouped": rep.n_grouped, "n_ungrouped": rep.n_ungrouped}


SEED0, TOTAL, LOSS = 5_000_000, 20_000, 0.002


def traced_pingpong_workload(rounds=16):
    """The lossy two-pair ping-pong of examples/failure_modes_test.cpp: neither side retries, so a lost packet leaves a pair waiting for
    ever; each pair's client traces its pair number when its loop completes.  obs_hash then names the mode: nothing traced = both pairs
    stuck, {1} = pair 0 stuck, {0} = pair 1 stuck, {0, 1} in either order = a pass."""
    wl = W.WorkloadBuilder()
    tasks = []
    for pair in range(2):
        n1, n2 = wl.create_node(), wl.create_node()
        a1, a2 = wl.addr(n1, 1), wl.addr(n2, 1)
        t1 = wl.task(n1)
        t1.bind(a1).sleep(secs=1).set(0, rounds)
        top1 = t1.label()
        t1.send_to(a1, a2, 1, W.PING).recv_from(a1, 1).assert_val(W.PONG).djnz(0, top1).trace(pair).done()
        t2 = wl.task(n2)
        t2.bind(a2).set(0, rounds)
        top2 = t2.label()
        t2.recv_from(a2, 1).assert_val(W.PING).reply(a2, 1, W.PONG).djnz(0, top2).done()
        tasks += [t1, t2]
    m = wl.main()
    for t in tasks:
        m.spawn(t)
    for t in tasks:
        m.join(t)
    m.done()
    return wl.build()


@functools.lru_cache(maxsize=None)
def traced_pingpong():
    """(workload, config, the oracle's results — read-only) of the 20 000 traced lossy ping-pong seeds."""
    w, cfg = traced_pingpong_workload(), A.Config.default(packet_loss_rate=LOSS)
    want, _ = oracle.run_batch(w, SEED0, TOTAL, cfg)
    want.setflags(write=False)
    return w, cfg, want
