"""Every op family on every kernel build that compiles it, on the host-compiled kernels (tests/emu): the matrix of tests/build_cases.py — per
non-trace row of variant_table its cases, 130 seeds each on all 48 result bytes, each case on exactly the row it names (the library's
selection, the emulation's, and the function the emulation then called), no seed of the pass a runner verdict.  Beside it the premises the
matrix rests on:

  * the rows are the compiled set: every row of the library's variant_table is a row here, a trace row, or the one row select_variant can
    never name (shown over every parameter block it reads);
  * OP_CLASS, from which "the opcodes a row compiles" follows, against the library: a one-op workload's features are exactly the op's classes;
  * per row, the oracle's op_polls over the cases' seeds cover every opcode the row compiles — the device equals the oracle seed for seed, so
    the same seeds poll the same ops there; the pairs left out are the listed exclusions, the refusals among them asserted with their code;
  * the oracle alone yields no runner verdict at the chosen limits, and agrees with the generator restatement of
    tests/golden/make_golden_async.py on the cases that restatement has the ops for (the tier families' ops are held against their own
    sims by tests/test_oracle_tiers.py).

What these cases see and the rest of the suite does not: tools/build_mutants.py; what they reach line by line: tools/build_coverage.py;
both in profiles/build_matrix.md."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from madsim_amd import runtime
from tests import build_cases as B
from tests import emu

FIELDS = ("verdict", "steps", "clock_ns", "msg_count", "rng_calls", "trace_hash", "obs_hash")


def _table():
    """variant_table as the host-compiled kernel has it: rows of (trace, spill, lws, feat, rq, g)."""
    L = emu.lib()
    tab = (C.c_int32 * (6 * 128))()
    n = L.madsim_emu_variants(tab, 128)
    return [tuple(tab[6 * i:6 * i + 6]) for i in range(n)]


def _ran_on():
    return _table()[emu.lib().madsim_emu_last_variant()]


def test_rows_are_the_compiled_builds():
    table = _table()
    rows = [r.sel for r in B.ROWS.values()]
    traces = [sel for sel, _ in B.TRACE_ROWS.values()]
    assert len(set(rows)) == len(rows) and len(set(table)) == len(table)
    assert sorted(rows + traces + list(B.UNSELECTABLE)) == sorted(table)
    assert {r.variant for r in B.ROWS.values()} == {B._v(s, l, f, q, g) for _, s, l, f, q, g in rows}


def test_the_unselectable_row():
    """select_variant over every parameter block it can read — lane strides 8 .. 64, with and without a spill region, every features word,
    either state placement, narrow, compact, no-log, register queue, trace or not — names every row of the table but the listed one."""
    L = emu.lib()
    reach = (C.c_uint8 * 128)()
    n = L.madsim_emu_selectable(reach, 128)
    table = _table()
    assert {table[i] for i in range(n) if not reach[i]} == set(B.UNSELECTABLE)


@pytest.mark.parametrize("op", sorted(A.OP))
def test_op_class_against_the_library(op):
    """The features geometry.h computes for a workload whose only op is `op` are the op's classes — and the build it selects carries them."""
    w = B.one_op_workload(op)
    assert emu.geometry_params(w)["features"] == B.OP_CLASS[op], op
    g = runtime.geometry(w)
    feat = ((g.variant >> 8) & 0xff) | sum(f for bit, f in A.VARIANT_TIER_FEAT if g.variant & bit)
    assert B.OP_CLASS[op] & ~feat == 0 and (feat & (B.ALL | B.TIERS | B.SIGNAL) == 0) == (B.OP_CLASS[op] == 0), (op, feat)
    assert op in B.compiled_ops(feat)


def test_core_workloads_have_the_features_the_case_rule_assumes():
    for name, feat in B.CORE.items():
        w, _, lim = B.built(name)
        assert emu.geometry_params(w, lim)["features"] == feat, name


def test_a_carrier_moves_no_instruction_and_adds_its_family():
    w, _, _ = B.built("base_ops")
    n = w.struct.n_insns
    for fam in B.FAMILIES:
        c = B.carrier(w, fam)
        assert c.struct.n_progs == w.struct.n_progs + 1 and c.struct.n_nodes == w.struct.n_nodes + 1
        assert bytes(c.insns)[:8 * n] == bytes(w.insns)[:8 * n] and bytes(c.progs)[:4 * w.struct.n_progs] == bytes(w.progs)
        feat = emu.geometry_params(c)["features"]
        want = dict(time=B.TIME, chan=B.CHAN, all=B.TIME | B.NODE, addr=B.ADDR, scope=B.SCOPE, tick=B.TICK, select=B.TIME | B.TICK | B.SELECT,
                    signal=B.NODE | B.SIGNAL)[fam]
        assert feat == want, (fam, feat)


@pytest.mark.parametrize("row", list(B.ROWS))
def test_row_selects_its_build(row):
    """Every case of a row runs on the build the row names, in the library and in the emulation."""
    n = 0
    for _, _, w, _, lim in B.cases(row):
        B.check_variant(row, w, lim, emu)
        n += 1
    assert n >= 2


@pytest.mark.parametrize("row", list(B.ROWS))
def test_build_matrix_emu(row):
    B.run_row(row, emu.run_batch, ran_on=_ran_on)


@pytest.mark.parametrize("row", list(B.ROWS) + list(B.TRACE_ROWS))
def test_the_cases_of_a_row_poll_every_opcode_it_compiles(row):
    """The premise, from the oracle's counters: over the seeds of the row's cases (130 each; 8 each on a trace row) every opcode the row
    compiles is polled; no seed is a runner verdict in the oracle alone (it would be compared with nothing)."""
    got, need = B.polled_by_row(row), set(B.compiled_ops(B.row_feats()[row]))
    assert need <= got, (row, sorted(need - got))
    if row in B.TRACE_ROWS:
        B.trace_truth(row)                              # (asserts the verdicts)
        return
    for name, cs, *_ in B.cases(row):
        want = B.truth(row, name, cs)
        assert not (want["verdict"] >= A.OVERFLOW).any(), (row, name, cs, np.unique(want["verdict"], return_counts=True))
        assert B.polled(row, name, cs) - set(B.compiled_ops(B.ROWS[row].feat)) == set(), (row, name, "polls an op the row does not compile")


def test_no_pair_is_missing():
    """Every (row, opcode) pair is polled by the row's cases or listed in exclusions() with one of the two reasons."""
    ex = B.exclusions()
    assert set(ex.values()) == {B.GUARD, B.REFUSED}
    feats = B.row_feats()
    for row in feats:
        got = B.polled_by_row(row)
        for op in A.OP:
            assert (op in got) != ((row, op) in ex), (row, op)
    # a refused pair is one whose op belongs to the other side of the signals / tiers rule
    for (row, op), why in ex.items():
        other = (B.OP_CLASS[op] & B.SIGNAL and feats[row] & B.TIERS) or (B.OP_CLASS[op] & B.TIERS and feats[row] & B.SIGNAL)
        assert (why == B.REFUSED) == bool(other), (row, op)


@pytest.mark.parametrize("what,w", list(B.refused_workloads()), ids=lambda x: "-".join(x) if isinstance(x, tuple) else "")
def test_signals_beside_a_tier_are_refused(what, w):
    """MADSIM_E_WORKLOAD from the library's geometry and from the emulation's run; the oracle refuses the workload too."""
    with pytest.raises(runtime.MadsimHipError, match=B.E_WORKLOAD):
        runtime.geometry(w)
    with pytest.raises(RuntimeError, match="emu error -4"):
        emu.run_batch(w, B.SEED0, 1)
    with pytest.raises(oracle.OracleError):
        oracle.run_batch(w, B.SEED0, 1)


@pytest.mark.parametrize("row", list(B.TRACE_ROWS))
def test_trace_rows_emu(row):
    """The trace builds, on the cases of the LDS-resident row of their tier: the raw determinism log of each seed byte for byte against the
    oracle's, and the 48 result bytes (obs_hash folds the observations); the emulation ran the trace row."""
    n_obs = 0
    for name, cs, w, cfg, lim, seeds in B.trace_truth(row):
        for seed, log, obs, res in seeds:
            got_log, got = emu.trace_seed(w, seed, cfg, lim)
            assert _ran_on() == B.TRACE_ROWS[row][0], (row, name, _ran_on())
            assert tuple(int(x) for x in got) == res, (row, name, cs, seed, got, res)
            assert got_log == log, (row, name, cs, seed, len(got_log), len(log))
            n_obs += len(obs)
    assert n_obs


def test_op_polls_sum_over_a_batch():
    """op_polls are sums over the seeds of a call, like the heap counters; every poll of the run is counted under exactly one opcode."""
    w, cfg, _ = B.built("base_ops")
    one = [oracle.run_batch(w, B.SEED0 + i, 1, cfg, want_stats=True)[2] for i in range(4)]
    whole = oracle.run_batch(w, B.SEED0, 4, cfg, want_stats=True)[2]
    assert list(whole.op_polls) == [sum(s.op_polls[k] for s in one) for k in range(oracle.OP_COUNT)]
    assert whole.op_polls[A.OP["CLOG_NODE"]] == 4 and whole.op_polls[A.OP["SPAWN"]] == 12 and whole.op_polls[A.OP["MARK"]] == 0


def test_the_earlier_entry_point_writes_the_earlier_struct_only():
    """A caller built before op_polls allocates 80 bytes of statistics: madsim_oracle_run_batch fills those and leaves what lies behind
    them alone; the sized entry point fills what it is given and no more."""
    w, cfg, _ = B.built("base_ops")
    L, v1 = oracle.lib(), C.sizeof(oracle.OracleStats) - 4 * oracle.OP_COUNT
    assert v1 == 80 == oracle.OracleStats.op_polls.offset
    whole = oracle.run_batch(w, B.SEED0, 2, cfg, want_stats=True)[2]
    for size, call in ((v1, lambda buf: L.madsim_oracle_run_batch(w.ref(), C.byref(cfg), B.SEED0, 2, C.byref(A.Limits()), None, None,
                                                                  C.cast(buf, C.POINTER(oracle.OracleStats)))),
                       (v1 + 8, lambda buf: L.madsim_oracle_run_batch_sized(w.ref(), C.byref(cfg), B.SEED0, 2, C.byref(A.Limits()), None, None,
                                                                            C.cast(buf, C.POINTER(oracle.OracleStats)), v1 + 8))):
        buf = (C.c_uint8 * C.sizeof(oracle.OracleStats))()
        C.memset(C.byref(buf, size), 0xA5, C.sizeof(buf) - size)
        C.memset(buf, 0, size)
        assert call(buf) == 0
        assert bytes(buf[:size]) == bytes(whole)[:size] and set(bytes(buf[size:])) == {0xA5}, size


_ASYNC_MOD = None


def _async_mod():
    global _ASYNC_MOD
    if _ASYNC_MOD is None:
        p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_async.py")
        spec = importlib.util.spec_from_file_location("make_golden_async", p)
        _ASYNC_MOD = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_ASYNC_MOD)
    return _ASYNC_MOD


RESTATED = [(name, ()) for name, feat in B.CORE.items() if not feat & (B.TIERS | B.SIGNAL)] + [("base_ops", (f,)) for f in ("time", "chan", "all", "addr")]


@pytest.mark.parametrize("name,cs", RESTATED, ids=lambda x: x if isinstance(x, str) else "+".join(x))
def test_truth_agrees_with_the_generator_restatement(name, cs):
    """The oracle against a second statement of the same semantics (make_golden_async.py's generator-based Sim), every result field."""
    mod = _async_mod()
    w, cfg, lim = B.built(name, cs)
    want = B.parity.expected(w, B.SEED0, B.GOLDEN_SEEDS, cfg, lim or A.Limits())
    for i in range(B.GOLDEN_SEEDS):
        ref = mod.Sim(w, cfg or A.Config.default(), B.SEED0 + i).run(0)
        assert {f: int(want[i][f]) for f in FIELDS} == {f: ref[f] for f in FIELDS}, (name, cs, B.SEED0 + i)
