"""The host-side truth of a sweep campaign (madsim_hip_run_sweep_campaign): given the per-seed results of the V variants, everything
madsim_sweep_t holds afterwards — a plain numpy restatement of include/madsim_hip.h, independent of the library.  Shared by
tests/test_campaign_sweep.py (which holds it against plain Python ints, and the library's host fold against it), tests/test_sweep_kernels.py and
tests/test_campaign_sweep_gpu.py (which hold the GPU's answers against it)."""
import functools

import numpy as np

import oracle
from madsim_amd import _abi as A
from tests import diff_ref

U64_MAX = (1 << 64) - 1
FIELDS = diff_ref.FIELDS                                                                         # bit i of `fields` = FIELDS[i]
ALL = 127
RUNNER = 4                                                                                       # verdicts at or above it are runner verdicts
WORDS = 274                                                                                      # MADSIM_K_SWEEP_WORDS
MIXED, FAILING, DIFFERING = range(3)                                                             # MADSIM_SWEEP_LIST_*


def classify(results, fields):
    """Per seed: (fail mask, runner mask, differ mask — 0 for an incomparable seed) over the variants' result arrays."""
    n = len(results[0])
    fail, runner, differ = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    for v, r in enumerate(results):
        assert len(r) == n
        fail |= ((r["verdict"] >= 1) & (r["verdict"] < RUNNER)).astype(np.uint32) << np.uint32(v)
        runner |= (r["verdict"] >= RUNNER).astype(np.uint32) << np.uint32(v)
        if v:
            d = np.zeros(n, dtype=bool)
            for i, name in enumerate(FIELDS):
                if fields >> i & 1:
                    d |= r[name] != results[0][name]
            differ |= d.astype(np.uint32) << np.uint32(v)
    differ[runner != 0] = 0
    return fail, runner, differ


def selected(fail, runner, differ, rule, n_variants):
    settled = runner == 0
    if rule == MIXED:
        return settled & (fail != 0) & (fail != (1 << n_variants) - 1)
    return settled & ((fail != 0) if rule == FAILING else (differ != 0))


def seeds_of(seed0_or_seeds, idx):
    """The seeds at positions `idx`: of a range (an int: seed0, wrapping at 2^64 like the device's add) or of a list (an array)."""
    idx = np.asarray(idx, dtype=np.uint64)
    if isinstance(seed0_or_seeds, (int, np.integer)):
        with np.errstate(over="ignore"):
            return idx + np.uint64(int(seed0_or_seeds) & U64_MAX)
    return np.asarray(seed0_or_seeds, dtype=np.uint64)[idx.astype(np.int64)]


def records_of(results, seed0_or_seeds, idx, fail, differ):
    """The records of the seeds at `idx` (ascending positions), as an ndarray[A.SWEEP_RECORD_DTYPE]."""
    r = np.zeros(len(idx), dtype=A.SWEEP_RECORD_DTYPE)
    if len(idx):
        r["seed"] = seeds_of(seed0_or_seeds, idx)
        r["fail_mask"], r["differ_mask"] = fail[idx], differ[idx]
        for v, res in enumerate(results):
            r["verdict"][:, v] = res["verdict"][idx]                                             # (listed seeds are settled: 0 .. 3)
    return r


def sweep_truth(results, seed0_or_seeds, fields, rule, cap):
    """What madsim_sweep_t holds after a campaign whose variants gave `results` (a list of V arrays) for the seeds [seed0, seed0 + len) or
    for the list `seeds`."""
    V, n = len(results), len(results[0])
    assert 2 <= V <= 8 and 0 <= fields <= ALL and rule in (MIXED, FAILING, DIFFERING) and (rule != DIFFERING or fields)
    fail, runner, differ = classify(results, fields)
    settled = runner == 0
    idx = np.nonzero(selected(fail, runner, differ, rule, V))[0]
    by_mask = np.bincount(fail[settled], minlength=256).astype(np.uint64)
    return {"n_listed": min(cap, len(idx)), "n_selected": len(idx), "n_settled": int(settled.sum()), "n_incomparable": int(n - settled.sum()),
            "n_runner_by_variant": [int((runner >> np.uint32(v) & 1).sum()) for v in range(8)],
            "n_differ_from_first": [int((differ >> np.uint32(v) & 1).sum()) for v in range(8)],
            "n_by_mask": [int(x) for x in by_mask], "records": records_of(results, seed0_or_seeds, idx[:cap], fail, differ).tobytes()}


def wave_counts(results, fields, rule):
    """Selected seeds per wave under the cut the report kernels use: grid = min(256, ceil(count / 1024)) workgroups of 4 waves, every wave a
    contiguous piece, a multiple of 64 seeds (zeros for waves of the grid that own nothing)."""
    count = len(results[0])
    grid = max(1, min(256, (count + 1023) // 1024))
    waves = 4 * grid
    piece = ((count + waves - 1) // waves + 63) // 64 * 64
    sel = selected(*classify(results, fields), rule, len(results))
    return piece, [int(sel[w * piece:(w + 1) * piece].sum()) for w in range(waves)]


def words_of(results, fields, rule):
    """The MADSIM_K_SWEEP_WORDS words the device leaves for a batch: {n_selected, n_incomparable, n_runner_by_variant[8],
    n_differ_from_first[8], n_by_mask[256]}."""
    t = sweep_truth(results, 0, fields, rule, 0)
    w = np.array([t["n_selected"], t["n_incomparable"]] + t["n_runner_by_variant"] + t["n_differ_from_first"] + t["n_by_mask"], dtype=np.uint64)
    assert len(w) == WORDS
    return w


def of_struct(s, records):
    """An A.Sweep after a call (and the ndarray its `records` points into) in the shape of sweep_truth's answer."""
    return {"n_listed": int(s.n_listed), "n_selected": int(s.n_selected), "n_settled": int(s.n_settled), "n_incomparable": int(s.n_incomparable),
            "n_runner_by_variant": [int(x) for x in s.n_runner_by_variant], "n_differ_from_first": [int(x) for x in s.n_differ_from_first],
            "n_by_mask": [int(x) for x in s.n_by_mask], "records": records[:s.n_listed].tobytes()}


def of_report(rep):
    """A runtime.CampaignSweep in the shape of sweep_truth's answer."""
    pad = lambda a, n: [int(x) for x in a] + [0] * (n - len(a))
    return {"n_listed": len(rep.records), "n_selected": rep.n_selected, "n_settled": rep.n_settled, "n_incomparable": rep.n_incomparable,
            "n_runner_by_variant": pad(rep.n_runner_by_variant, 8), "n_differ_from_first": pad(rep.n_differ_from_first, 8),
            "n_by_mask": pad(rep.n_by_mask, 256), "records": rep.records.tobytes()}


def synthetic(rng, n, n_variants, p_change=0.05, verdicts=(0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 7, 0xffffffff)):
    """V variants of n results: variant 0 is drawn at random; every other variant is variant 0, except that about p_change of its seeds
    get a few random fields redrawn (the verdict among them)."""
    base, _ = diff_ref.synthetic(rng, n, 0.0, verdicts)
    out = [base]
    for _ in range(1, n_variants):
        b = base.copy()
        for i in np.nonzero(rng.random(n) < p_change)[0]:
            for name in rng.choice(FIELDS, rng.integers(1, 4), replace=False):
                if name == "verdict":
                    b[name][i] = rng.choice(np.array(verdicts, dtype=np.uint32))
                elif name == "steps":
                    b[name][i] ^= np.uint32(1) << np.uint32(rng.integers(0, 32))
                else:
                    b[name][i] ^= np.uint64(1) << np.uint64(rng.integers(0, 64))
        out.append(b)
    return out


SEED0, TOTAL = diff_ref.SEED0, diff_ref.TOTAL
LOSSES = (0.0, 0.0005, diff_ref.LOSS, 0.01)
FAILURES = (0, 299, 1149, 4684)                                                                  # deadlocks per loss rate over the range
MASKS = {0b0000: 5316, 0b1000: 3535, 0b1100: 850, 0b1110: 299}                                   # the non-empty cells of n_by_mask: the sets nest


@functools.lru_cache(maxsize=None)
def four_configs():
    """(workload, the four configs, the oracle's results under each — read-only): diff_ref.two_configs' four-node ping-pong at the loss rates
    LOSSES over TOTAL seeds from SEED0 (tests/test_campaign_sweep.py asserts FAILURES and MASKS of them)."""
    w, cfg0, cfg2, r0, r2 = diff_ref.two_configs()
    cfgs, res = [cfg0, A.Config.default(packet_loss_rate=LOSSES[1]), cfg2, A.Config.default(packet_loss_rate=LOSSES[3])], [r0, None, r2, None]
    for v in (1, 3):
        res[v], _ = oracle.run_batch(w, SEED0, TOTAL, cfgs[v])
        res[v].setflags(write=False)
    return w, cfgs, res
