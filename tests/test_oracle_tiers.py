"""The C oracle's timeout scopes, interval tickers, biased selects and ctrl-c signals, held against the second restatement of each —
the generator sims tests/scope_sim.py, interval_sim.py, select_sim.py and signal_sim.py — before anything on a device is compared
with it; and the conditions under which the GPU comparison of tests/test_tier_parity_gpu.py means something: its fixed blocks reach
every event the families add, every verdict, and every build.  All on the CPU, by the oracle alone.
"""
import importlib

import pytest

import oracle
from madsim_amd import _abi as A
from madsim_amd import runtime
from madsim_amd import workload as W
from tests import parity, select_sim
from tests import tier_blocks as TB

N_PROGRAMS, N_SEEDS = 300, 8
SIM_BASE = {"scope": 5_100_000, "interval": 5_200_000, "select": 5_300_000, "signal": 5_400_000}
FAMILY_NAMES = sorted(TB.FAMILIES)


def assert_oracle_equals_sim(fam, w, cfg, seed, label):
    """oracle.trace_seed == the family's sim on the seven result fields and the raw determinism log.  Two cases need a word.  A seed
    that meets one of the workload MODEL's ceilings (a ninth connection waiting for accept1, say) is MADSIM_UNSUPPORTED for the oracle's
    model-limits layer and an ordinary run for the sim, which has no such layer: there the oracle's PURE run, ceilings off, must have
    recorded the event and must equal the sim on the seven fields.  A send that would wake two ctrl-c waiters is MADSIM_UNSUPPORTED on
    both sides, all fields 0; the sim keeps no log for it."""
    want = fam.sim(w, cfg, seed).run()
    log, res = oracle.trace_seed(w, seed, cfg)
    got = {f: int(getattr(res, f)) for f in TB.FIELDS}
    want_fields = {f: want[f] for f in TB.FIELDS}
    if got["verdict"] == A.UNSUPPORTED and want["verdict"] != A.UNSUPPORTED:
        pure, ev = oracle.run_batch_pure(w, seed, 1, cfg)
        assert ev[0] and not ev[0] & 8192, (label, seed, "MADSIM_UNSUPPORTED without a model event of the oracle's own layer", int(ev[0]))
        assert {f: int(pure[0][f]) for f in TB.FIELDS} == want_fields, (label, seed, "pure run", [oracle.ME_NAMES[b] for b in oracle.ME_NAMES if ev[0] & b])
        return "model"
    assert got == want_fields, (label, seed)
    if want["verdict"] == A.UNSUPPORTED:
        pure, ev = oracle.run_batch_pure(w, seed, 1, cfg)
        assert ev[0] & 8192, (label, seed, "the sim's two-waiter send is not the oracle's model event")
        return "two waiters"
    assert log.hex() == want["log"], (label, seed, "raw log bytes")
    return "equal"


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_oracle_equals_the_family_sim_on_fuzzed_programs(name):
    """300 programs of the family's generator (every third with general addresses, all with the hazards of the GPU blocks) x 8 seeds."""
    fam = TB.FAMILIES[name]
    how = {}
    for k in range(N_PROGRAMS):
        w, cfg, desc = fam.program(SIM_BASE[name], k)
        for seed in range(N_SEEDS):
            r = assert_oracle_equals_sim(fam, w, cfg, 31 * k + seed, f"{fam.gen.__name__}(Random({SIM_BASE[name] + k}), **{fam.gen_kw_of(k)}) {desc}")
            how[r] = how.get(r, 0) + 1
    print(f"{name}: {how}")
    assert how["equal"] >= 0.9 * N_PROGRAMS * N_SEEDS           # (the two special cases stay the exception)


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_oracle_equals_the_family_sim_on_the_directed_workloads(name):
    fam = TB.FAMILIES[name]
    directed = importlib.import_module(fam.test_module).DIRECTED
    assert directed
    for wname, (w, cfg) in sorted(directed.items()):
        for seed in range(N_SEEDS):
            assert_oracle_equals_sim(fam, w, cfg, seed, f"{fam.test_module}.DIRECTED[{wname!r}]")


# ---- an opcode without a case fails the call ------------------------------------------------------------------------------------------
def _with_opcode(w, index, op):
    n = [0]

    def f(ins):
        n[0] += 1
        return A.Insn(op if n[0] - 1 == index else ins.op, ins.a, ins.b, ins.imm)
    return select_sim._rewrite(w, f)


OP_COUNT = max(A.OP.values()) + 1                                # MS_OP__COUNT: the first value beyond the table


@pytest.mark.parametrize("op", [OP_COUNT, 200, 255, 17])
def test_an_opcode_without_a_case_fails_every_entry_point(op):
    """Values beyond the table are refused before anything runs, wherever they stand; a value inside the table that names no op (17: a
    gap of the numbering) fails the call when a task reaches it.  Never a verdict."""
    assert op not in A.OP.values()
    w = W.pingpong(2, 2)
    for index in ((0, w.struct.n_insns - 2) if op >= OP_COUNT else (0,)):
        bad = _with_opcode(w, index, op)
        for call in (lambda: oracle.run_batch(bad, 0, 4), lambda: oracle.run_batch_pure(bad, 0, 4),
                     lambda: oracle.trace_seed(bad, 0), lambda: oracle.observe_seed(bad, 0)):
            with pytest.raises(oracle.OracleError) as e:
                call()
            assert e.value.code == oracle.E_OPCODE
    oracle.run_batch(w, 0, 4)                                    # (the unchanged program runs)


def _append_done(w):
    """The same workload with main as `<slot>; DONE` (the slot is what _with_opcode overwrites)."""
    from madsim_amd import workload as WL
    done = A.OP["DONE"]
    insns = [A.Insn(done, 0, 0, 0), A.Insn(done, 0, 0, 0)]
    nodes = [w.nodes[i] for i in range(w.struct.n_nodes + 1)]
    socks = [w.socks[i] for i in range(w.struct.n_socks)]
    return WL.BuiltWorkload(nodes, [A.Prog(0, 0, 0)], socks, insns, [], None, 0)


def test_validate_refuses_a_nested_scope_and_a_select_inside_one():
    begin, end, sleep, done, rt = A.OP["TIMEOUT_BEGIN"], A.OP["TIMEOUT_END"], A.OP["SLEEP"], A.OP["DONE"], A.OP["RECV_TIMEOUT_AT"]
    base = _append_done(W.pingpong(2, 2))

    def prog(insns):
        nodes = [base.nodes[i] for i in range(base.struct.n_nodes + 1)]
        socks = [base.socks[i] for i in range(base.struct.n_socks)]
        return W.BuiltWorkload(nodes, [A.Prog(0, 0, 0)], socks, [A.Insn(*i) for i in insns], [], None, 0)
    ok = prog([(begin, 0, 2, 5_000_000), (sleep, 0, 0, 1_000_000), (end, 0, 0, 0), (done, 0, 0, 0)])
    out, _ = oracle.run_batch(ok, 0, 2)
    assert (out["verdict"] == A.PASS).all()
    nested = prog([(begin, 0, 4, 5_000_000), (begin, 0, 3, 1_000_000), (sleep, 0, 0, 1_000_000), (end, 0, 0, 0), (end, 0, 0, 0), (done, 0, 0, 0)])
    select_inside = prog([(A.OP["MARK"], 0, 0, 0), (begin, 0, 3, 5_000_000), (rt, 0, 0x100, 1_000_000), (end, 0, 0, 0), (done, 0, 0, 0)])
    for bad in (nested, select_inside):
        with pytest.raises(oracle.OracleError) as e:
            oracle.run_batch(bad, 0, 1)
        assert e.value.code == -1                                # MADSIM_E_ARG: refused, not run


# ---- the GPU blocks are not vacuous -------------------------------------------------------------------------------------------------
MIN_EVENTS = 20


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_the_fixed_block_reaches_every_event_and_verdict(name):
    """Over the fixed block tests/test_tier_parity_gpu.py runs — same programs, seeds and limits: each of the oracle's counters that
    applies to the family >= 20, the verdicts PASS, PANIC and DEADLOCK all present, no seed beyond the device layout's ceilings, and
    in the signal block at least one seed that a two-waiter send makes MADSIM_UNSUPPORTED."""
    fam = TB.FAMILIES[name]
    totals, verdicts, two_waiters = {c: 0 for c in fam.counters}, set(), 0
    for k in range(TB.N_FIXED):
        w, cfg, _ = fam.program(fam.base, k)
        lim = TB.limits_of(fam, k)
        for s in range(TB.SEEDS):                                # (seed by seed: the high-water marks are per seed, parity.beyond_ceiling)
            out, _, st = oracle.run_batch(w, k * TB.SEED_MUL + s, 1, cfg, lim, want_stats=True)
            verdicts.add(int(out[0]["verdict"]))
            for c in fam.counters:
                totals[c] += getattr(st, c)
            for f, cap in parity.CEILINGS.items():
                assert getattr(st, f) <= cap, (name, k, s, f)
        _, ev = oracle.run_batch_pure(w, k * TB.SEED_MUL, TB.SEEDS, cfg, lim)
        two_waiters += int(((ev & 8192) != 0).sum())
    print(f"{name}: {totals}, verdicts {sorted(verdicts)}, two-waiter seeds {two_waiters}")
    for c, n in totals.items():
        assert n >= MIN_EVENTS, (name, c, n)
    assert {A.PASS, A.PANIC, A.DEADLOCK} <= verdicts, (name, sorted(verdicts))
    if name == "signal":
        assert two_waiters >= 1 and A.UNSUPPORTED in verdicts
    else:
        assert two_waiters == 0


def _shape(g):
    return "global, general addresses" if g.variant & 16 and (g.variant >> 8) & 16 else "global, plain addresses" if g.variant & 16 else "LDS"


def test_the_fixed_blocks_select_all_sixteen_builds():
    """Four shapes (MADSIM_TIER_VARIANTS) of four tiers.  The three batch shapes are read from the geometry the host computes for each
    program of a fixed block under its limits: each at least 10 times.  The fourth, the trace build, is what madsim_hip_trace_seed
    selects for a workload of the tier whatever its limits: the raw-log test traces four programs of each fixed block at two seeds,
    programs whose tier is checked here."""
    builds = {}
    for name, fam in TB.FAMILIES.items():
        for k in range(TB.N_FIXED):
            w, _, _ = fam.program(fam.base, k)
            g = runtime.geometry(w, TB.limits_of(fam, k))
            assert g.variant & TB.TIER_BITS == fam.tier, (name, k, hex(g.variant))
            key = (name, runtime.variant_name(g))
            builds[key] = builds.get(key, 0) + 1
            assert bool(g.variant & 16) == bool(k % 2), (name, k)                                    # global state on odd programs
            if g.variant & 16:
                assert bool((g.variant >> 8) & 16) == TB.general_addr_of(k), (name, k)              # MADSIM_FEAT_ADDR
            else:
                assert (g.variant >> 16) & 0xf == 15, (name, k)                                     # the runtime-lane-stride build
            if k in TB.TRACED:
                tkey = (name, "trace")
                builds[tkey] = builds.get(tkey, 0) + len(TB.TRACE_SEEDS)
    print("\n".join(f"{k[0]:9s} {k[1]:60s} {n}" for k, n in sorted(builds.items())))
    assert len(builds) == 16 and len({k[1] for k in builds if k[1] != "trace"}) == 12
    for k, n in builds.items():
        assert n >= (len(TB.TRACED) * len(TB.TRACE_SEEDS) if k[1] == "trace" else 10), (k, n)
    assert {TB.general_addr_of(k) for k in TB.TRACED} == {False, True}
