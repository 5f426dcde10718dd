"""bench.py's plain run and --dump-outputs: the files hold exactly what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from madsim_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(d, suffix=""):
    return {f[:-len(suffix + ".npy")]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(suffix + ".npy")}


def _results(arrays):
    """The per-seed madsim_result_t rows back from their float64 columns (64-bit fields from their 32-bit halves)."""
    out = np.zeros(len(arrays["seed_offset"]), dtype=A.RESULT_DTYPE)
    for name in out.dtype.names:
        if name in arrays:
            out[name] = arrays[name].astype(np.uint64)
        else:
            out[name] = (arrays[name + "_hi"].astype(np.uint64) << np.uint64(32)) | arrays[name + "_lo"].astype(np.uint64)
    return out


def _report(arrays):
    return (arrays["report_hi"].astype(np.uint64) << np.uint64(32)) | arrays["report_lo"].astype(np.uint64)


def test_dump_outputs_round_trips_every_bit(tmp_path):
    rng = np.random.default_rng(5)
    res = np.zeros(1000, dtype=A.RESULT_DTYPE)
    for name in res.dtype.names:
        res[name] = rng.integers(0, np.iinfo(res.dtype[name]).max, size=len(res), dtype=res.dtype[name], endpoint=True)
    res["trace_hash"][0] = (1 << 64) - 1
    report = np.array([(1 << 64) - 1, 3, 1 << 60, 12345], dtype=np.uint64)
    bench.dump_outputs(str(tmp_path), res, report)
    arrays = _load(str(tmp_path))
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert (arrays["seed_offset"] == np.arange(len(res))).all()
    assert (_results(arrays) == res).all()
    assert (_report(arrays) == report).all()


def test_dump_outputs_samples_large_batches_the_same_way_every_time(tmp_path):
    res = np.zeros(1000, dtype=A.RESULT_DTYPE)
    res["steps"] = np.arange(1000)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), res, np.zeros(4, dtype=np.uint64), max_seeds=64)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    idx = a["seed_offset"].astype(np.int64)
    assert len(idx) == 64 and (np.diff(idx) > 0).all() and (a["seed_offset"] == b["seed_offset"]).all()
    assert (a["steps"] == idx).all()


@pytest.mark.gpu
def test_plain_bench_times_steps_and_dumps_the_last_one(tmp_path, hip):
    """A plain run times exactly --steps steps and leaves the full line's legs out; --dump-outputs holds the per-seed results and
    the report of its last step, equal to the oracle's for the same seeds."""
    from madsim_amd import workload as W
    steps, warmup, seeds = 3, 2, 4096
    hip.shutdown()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--seeds", str(seeds), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    hip.init(0)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == steps and line["extra"]["regions"]["n"] == 1 and line["ms_per_step"] > 0
    assert line["roofline"] is None and line["extra"]["workloads"] is None and "cpu_baseline" not in line
    assert line["verified_seeds"] is None                                                   # no oracle check ran: null, not 0
    w, lim, _ = W.bench_case("pingpong")
    check_dump(_load(str(tmp_path)), w, lim, (warmup + steps - 1) * seeds, seeds)     # the last timed step's seed block


def check_dump(arrays, w, lim, seed0, count):
    """The dumped results and summary of one batch equal the oracle's for seeds [seed0, seed0 + count)."""
    import oracle
    want, osum = oracle.run_batch(w, seed0, count, None, lim)
    assert (arrays["seed_offset"] == np.arange(count)).all()
    assert (_results(arrays) == want).all()
    assert [int(x) for x in _report(arrays)] == [osum.first_failing_seed, osum.n_failed, osum.total_steps, osum.total_clock_ns]
