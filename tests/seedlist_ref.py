"""The host-side truth of the LIST forms of the campaign reports (madsim_hip_run_seeds_campaign, madsim_hip_run_seeds_campaign_diff, and the
madsim_k_launch_*_list launchers): derived from the existing independent truths — tests/report_ref.py, stats_ref.py, groups_ref.py,
diff_ref.py and the resolve rule — by one mapping.  Position i of a strictly ascending list takes the role seed0 + i has in a range, so a
list-form report is the range-form truth at seed0 = 0 with every seed-valued field s replaced by seeds[s]; the sentinel 2^64 - 1 ("no such
seed") stays the sentinel.  tests/test_campaign_seeds.py holds the mapping against plain Python ints.  Also the three list shapes of the
kernel tests and the campaign-level truth (what madsim_campaign_t holds) over the per-seed results of a list."""
import numpy as np

from madsim_amd import _abi as A
from tests import diff_ref as D
from tests import groups_ref as G
from tests import report_ref as T
from tests import stats_ref as R

NONE = (1 << 64) - 1
GAPS = (1, 2, 3, 1 << 33)


def as_list(seeds):
    s = np.ascontiguousarray(seeds, dtype=np.uint64)
    assert s.ndim == 1 and (len(s) < 2 or bool((s[:-1] < s[1:]).all())), "a seed list ascends strictly"
    return s


def seed_at(seeds, s):
    """The mapping: index s of the range truth at seed0 = 0 -> seeds[s]; the sentinel stays."""
    return NONE if int(s) == NONE else int(seeds[int(s)])


# ---- the three lists of the kernel tests ---------------------------------------------------------------------------------------
def dense(count, seed0=(1 << 40) + 7):
    return np.uint64(seed0) + np.arange(count, dtype=np.uint64)


def gapped(count):
    """From 0, the gaps cycling 1, 2, 3, 2^33: positions and seeds differ above bit 32."""
    gaps = np.array(GAPS, dtype=np.uint64)[np.arange(max(count - 1, 0)) % len(GAPS)]
    return np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(gaps, dtype=np.uint64)])[:count]


def top(count):
    """The last `count` integers below 2^64: bit 63 set, the sentinel value itself the last member."""
    return np.uint64(NONE - (count - 1)) + np.arange(count, dtype=np.uint64)


LISTS = (("dense", dense), ("gapped", gapped), ("top", top))


# ---- the report truths ---------------------------------------------------------------------------------------------------------
def summary6_truth(results, seeds):
    six = T.summary_truth(results, 0)[1]
    six[0], six[4] = seed_at(seeds, six[0]), seed_at(seeds, six[4])
    return six


def collect_truth(results, seeds, cap, list_runner):
    """(the 15 words, the bytes of the min(cap, n listed) records)"""
    words, rec_bytes = T.collect_truth(results, 0, cap, list_runner)
    words = words.copy()
    words[0], words[4] = seed_at(seeds, words[0]), seed_at(seeds, words[4])
    recs = np.frombuffer(rec_bytes, dtype=A.FAILURE_DTYPE).copy()
    recs["seed"] = seeds[recs["seed"].astype(np.int64)]
    return words, recs.tobytes()


def stats_truth(results, seeds, include, top_k):
    t = R.stats_truth(results, np.uint64(0), include, top_k)
    for name in R.METRICS:
        t[name]["top"] = [(v, int(seeds[s])) for v, s in t[name]["top"]]
    return t


def all_groups(results, seeds, include, key_field):
    return [(v, k, c, int(seeds[f])) for v, k, c, f in G.all_groups(results, 0, include, key_field)]


def groups_truth(results, seeds, include, key_field, cap):
    every = all_groups(results, seeds, include, key_field)
    return {"groups": every[:cap], "n_grouped": sum(g[2] for g in every[:cap]), "n_ungrouped": sum(g[2] for g in every[cap:])}


def diff_truth(a, b, seeds, fields, cap):
    t = D.diff_truth(a, b, 0, fields, cap)
    recs = np.frombuffer(t["records"], dtype=A.DIFF_RECORD_DTYPE).copy()
    recs["seed"] = seeds[recs["seed"].astype(np.int64)]
    t["records"] = recs.tobytes()
    return t


def resolve_truth(results, seeds, steps_maxed):
    """(seeds, idx) of the re-runnable results: MADSIM_OVERFLOW always, MADSIM_STEP_LIMIT while the step cap can still grow."""
    v = results["verdict"]
    idx = np.nonzero((v == A.OVERFLOW) | ((v == A.STEP_LIMIT) & (not steps_maxed)))[0]
    return seeds[idx], idx.astype(np.uint32)


def campaign_truth(results, seeds):
    """What madsim_campaign_t holds after a list campaign whose per-seed results are `results` (the prefix that was read)."""
    six = summary6_truth(results, seeds) if len(results) else [NONE, 0, 0, 0, NONE, 0]
    return {"seeds_run": len(results), "first_failing_seed": six[4], "n_failed": six[1] - six[5], "n_runner": six[5], "total_steps": six[2],
            "total_clock_ns": six[3]}


def of_campaign(rep):
    return {f: int(getattr(rep, f)) for f in ("seeds_run", "first_failing_seed", "n_failed", "n_runner", "total_steps", "total_clock_ns")}
