"""The corpus behind tests/golden/host_plan.json: what the host planner (madsim_amd/csrc/geometry.h: validate, make_geometry, build_tables)
answers, byte for byte, so that a change that is meant to leave it alone can be held to that.

tools/host_plan_record.py writes the record, tests/test_host_plan.py replays it.  CPU only (tests/emu madsim_emu_host_plan).

Accepted side: every workload tests/test_geometry_consistency.py walks (bench cases, lifecycle workloads, a block of every fuzz generator, the
directed tier workloads) and the cases of tests/build_cases.py.  The five bench cases stand in the record field by field.  Every entry — a
workload under the default capacities and its own, or the cases of one build row — has two digests: one over its members as they stand (codes,
messages, Geo, the parameter block, the five tables) and one over the whole cross of STATE x STATE_FLAGS x LANES x TRACE x VGPRS x COUNTS, 1 800
answers a member.  Codes and messages stand in full in one table, and each section counts its answers by their index there.  (One answer per
line would be a million lines; a digest names the entry that moved, and `record(verbose=...)` prints every answer, for a diff of two runs.)

Refused side: single-field mutations of small accepted workloads that between them use every opcode — per base the number of mutants, a digest
over their answers (field by field, codes and messages) and one over what the accepted mutants planned, and the count of every answer."""
import ctypes as C
import hashlib
import os
import random
import re

from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import build_cases as BC
from tests import emu, fuzz, fuzz_interval, fuzz_scope, fuzz_select, fuzz_signal, lifecycle_workloads as LW
from tests import test_geometry_consistency as TG
from tests import test_signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_plan.json")
HEADER = os.path.join(ROOT, "madsim_amd", "csrc", "geometry.h")

STATE = (A.STATE_AUTO, A.STATE_LDS, A.STATE_GLOBAL, A.STATE_COMPACT)
STATE_FLAGS = (0, A.STATE_DEDUP_TIMERS, A.STATE_NARROW_HEAP)
LANES = (0, 8, 16, 32, 64)
TRACE = (0, 1)
VGPRS = (0, 96, 128, 168, 184)
COUNTS = (1, 65, 1 << 20)
FUZZ_BLOCK = 6
N_OPS = 70          # MS_OP__COUNT


def d16(b):
    return hashlib.sha256(b).hexdigest()[:16]


def probe_config():
    """geometry.h probe_config(): what madsim_hip_geometry plans with."""
    return A.Config.default(lat_table=[(1_000_000, 10_000_000)] * 4)


def copy_limits(lim):
    c = A.Limits()
    if lim is not None:
        C.memmove(C.byref(c), C.byref(lim), C.sizeof(A.Limits))
    return c


def copy_config(cfg):
    c = A.Config()
    C.memmove(C.byref(c), C.byref(cfg), C.sizeof(A.Config))
    return c


# ---- the accepted side ------------------------------------------------------------------------------------------------------------------------
def accepted():
    """(entry, workload, config, limits or None) in a fixed order; consecutive members of one entry — a workload under the default capacities
    and its own, the cases of one row of tests/build_cases.py — share its digests."""
    for name in ("pingpong", "raft", "kv", "timers", "topo"):
        w, lim, _ = W.bench_case(name)
        yield f"bench/{name}", w, probe_config(), lim
    for name in sorted(LW.ALL):
        yield f"lifecycle/{name}", LW.ALL[name](), probe_config(), LW.limits(name)
    gens = TG.GENS + [("random_signal_workload", fuzz_signal.signal_limits)]
    for gen, limits in gens:
        make = next(getattr(m, gen) for m in TG.GEN_MODULES + (fuzz_signal,) if hasattr(m, gen))
        for k in range(FUZZ_BLOCK):
            w = make(random.Random(660_000 + k))[0]
            yield f"fuzz/{gen}/{k}", w, probe_config(), None
            yield f"fuzz/{gen}/{k}", w, probe_config(), limits()
    directed = TG.DIRECTED + [(test_signal, n, lambda n=n: test_signal.limits_for(n, 0)) for n in sorted(test_signal.DIRECTED)]
    for mod, name, limits in directed:
        w = mod.DIRECTED[name][0]
        yield f"directed/{mod.__name__.split('.')[-1]}/{name}", w, probe_config(), None
        yield f"directed/{mod.__name__.split('.')[-1]}/{name}", w, probe_config(), limits()
    for row in BC.ROWS:
        for name, cs, w, cfg, lim in BC.cases(row):
            yield f"build/{row}", w, cfg or A.Config.default(), lim


def _answer(r):
    """One plan as bytes: codes, messages, Geo, the parameter block."""
    g = r.get("geometry", (1, ""))
    return repr((r["validate"], g, r.get("tables"), r.get("geo"))).encode() + r.get("kparams", b"")


def _key(r):
    """One plan's codes and messages, in full: a key of the message table."""
    if r["validate"][0]:
        return f"validate {r['validate'][0]}|{r['validate'][1]}"
    return f"geometry {r['geometry'][0]}|{r['geometry'][1]}|tables {r['tables'][0]}|{r['tables'][1]}"


def full_plan(w, cfg, lim):
    """A workload as it stands, field by field: codes and messages, every scalar of Geo, 16 hex digits of sha256 over the parameter block and
    over each device table."""
    r = emu.host_plan(w.ref(), cfg, lim)
    out = {"validate": list(r["validate"])}
    if r["validate"][0] == 0:
        out["geometry"], out["tables"] = list(r["geometry"]), list(r["tables"]) + [d16(t) for t in r.get("table", ())]
        if r["geometry"][0] == 0:
            out["geo"], out["kparams"] = dict(zip(emu.GEO_SCALARS, r["geo"])), d16(r["kparams"])
    return out


def plan_member(name, w, cfg, lim, stands, cross, tally, verbose=None):
    """One (workload, limits) into its entry's two running digests — as it stands (tables included), and through the whole cross — and its
    answers into the section's tally."""
    r = emu.host_plan(w.ref(), cfg, lim)
    stands.update(_answer(r))
    for t in r.get("table", ()):
        stands.update(t)
    tally[_key(r)] = tally.get(_key(r), 0) + 1
    if verbose is not None:
        verbose.write(f"{name} as it stands: {_key(r)} {r.get('geo')} {d16(r.get('kparams', b''))} {[d16(t) for t in r.get('table', ())]}\n")
    if r["validate"][0]:
        return
    for sm, lw in ((sm0 | fl, lw) for sm0 in STATE for fl in STATE_FLAGS for lw in LANES):
        l2 = copy_limits(lim)
        l2.state_mem, l2.lanes_per_wave = sm, lw
        for tr in TRACE:
            for vg in VGPRS:
                for n in COUNTS:
                    r = emu.host_plan(w.ref(), cfg, l2, n, tr, vg, tables=False)
                    cross.update(_answer(r))
                    tally[_key(r)] = tally.get(_key(r), 0) + 1
                    if verbose is not None:
                        verbose.write(f"{name} state_mem={sm:#x} lanes={lw} trace={tr} vgprs={vg} count={n}: {_key(r)} {r.get('geo')} {d16(r.get('kparams', b''))}\n")


# ---- the refused side -------------------------------------------------------------------------------------------------------------------------
class Mutable:
    """A private copy of a workload's tables (with room for one more service), to change one field of and put back."""

    def __init__(self, w):
        s = w.struct
        self.nodes = (A.Node * (s.n_nodes + 1))(*[w.nodes[i] for i in range(s.n_nodes + 1)])
        self.progs = (A.Prog * s.n_progs)(*[w.progs[i] for i in range(s.n_progs)])
        self.socks = (A.Sock * max(1, s.n_socks))(*[w.socks[i] for i in range(s.n_socks)])
        self.insns = (A.Insn * s.n_insns)(*[w.insns[i] for i in range(s.n_insns)])
        self.services = (A.Service * (s.n_services + 1))(*[w.services[i] for i in range(s.n_services)])
        self.struct = A.Workload(s.n_nodes, s.n_progs, s.n_socks, s.n_insns, self.nodes, self.progs, self.socks, self.insns, s.n_services,
                                 s.panic_dyn_max, self.services if s.n_services else None, s.panic_match)
        self.keep = w

    def ref(self):
        return C.byref(self.struct)


def mutation_bases():
    """(name, workload, config): one tiny workload per opcode, and the directed workloads of tests/build_cases.py."""
    for op in A.OP:
        yield f"one_op/{op}", BC.one_op_workload(op), probe_config()
    for name in BC.CORE:
        w, cfg, _ = BC.built(name)
        yield f"core/{name}", w, copy_config(cfg or A.Config.default())
    yield from directed_bases()


def directed_bases():
    """Accepted workloads one field away from the rules that need two things at once."""
    wl = W.WorkloadBuilder()          # a guard that spawns in Drop, beside a node op (-> PAUSE)
    n = wl.create_node()
    g = wl.task(n, spawn_on_drop=True)
    g.sleep(ms=1)
    wl.task(n).yield_now()
    wl.main().spawn(g).resume(n).join(g)
    yield "directed/guard_spawn", wl.build(), probe_config()
    wl = W.WorkloadBuilder()          # two listening Endpoints on one node, beside a node op (-> KILL, RESTART, SEND_CTRL_C)
    n = wl.create_node()
    ts = []
    for port in (1, 2):
        a = wl.addr(n, port)
        ts.append(wl.task(n))
        ts[-1].bind(a).accept1(a)
    wl.main().spawn(ts[0]).spawn(ts[1]).resume(n).sleep(ms=1)
    yield "directed/two_listeners", wl.build(), probe_config()
    wl = W.WorkloadBuilder()          # an IPVS service beside an ephemeral entry (-> the service's address, a server)
    n = wl.create_node()
    s = wl.addr(n, 1)
    wl.addr(n, 0)
    wl.main().ipvs_add_server(wl.ipvs_service(wl.virtual_addr(1, 80), servers=[s]), s)
    yield "directed/ipvs_ephemeral", wl.build(), probe_config()
    wl = W.WorkloadBuilder()          # a loop in front of a timeout scope (-> a jump into it)
    m = wl.main()
    m.set(0, 2)
    top = m.label()
    m.yield_now().djnz(0, top)
    with m.timeout(ms=1):
        m.yield_now().yield_now()
    yield "directed/loop_then_scope", wl.build(), probe_config()


def field_mutations(m):
    """(label, [(object, field, value)]) per field of a Mutable: the values tried in turn."""
    s = m.struct
    n_insns, n_progs, n_socks, n_nodes, n_services = s.n_insns, s.n_progs, s.n_socks, s.n_nodes, s.n_services
    for i in range(n_insns):
        in_ = m.insns[i]
        yield f"insn{i}.op", [(in_, "op", v) for v in range(N_OPS)]
        # the first value out of range of every operand kind: program, socket, node, IPVS call, ticker behaviour, latency entry
        yield f"insn{i}.a", [(in_, "a", v) for v in sorted({n_progs, n_socks, n_nodes + 1, 3, 4, 5, 7, 8, 255} - {in_.a})]
        lo = in_.b & 0xff
        # jump target / scope end (past the table, itself, the pc before), socket, node, service; reserved and untyped tags; select flag bits
        inside = {p + 1 for p in range(n_insns) if m.insns[p].op == A.OP["TIMEOUT_BEGIN"]}          # (a jump into a scope)
        yield f"insn{i}.b", [(in_, "b", v) for v in sorted(inside | {n_insns, i, max(i - 1, 0), i + 1, n_socks, n_nodes + 1, n_services, lo | 0xFE00, lo | 0xFF00, lo | 0x7F00,
                                                            lo | 0x8000, in_.b | 1, in_.b | 2, in_.b | 4, in_.b | 0x80, 0, 0xFFFF} - {in_.b})]
        # nanoseconds of a second, a timed RPC call, a socket (ipvs server), zero (interval period)
        yield f"insn{i}.imm", [(in_, "imm", v) for v in sorted({0, 1_000_000_000, n_socks, in_.imm | 0x100, 0xFFFFFFFF} - {in_.imm})]
    yield "drop_last", [(s, "n_insns", n_insns - 1)]
    yield "counts", [(s, "n_progs", 0), (s, "n_progs", 256), (s, "n_insns", 0), (s, "n_insns", 4097), (s, "n_nodes", 32), (s, "n_socks", 64),
                     (s, "n_services", 9), (s, "panic_dyn_max", 255)]
    for p in range(n_progs):
        pr = m.progs[p]
        yield f"prog{p}.entry", [(pr, "entry", v) for v in sorted({n_insns, pr.entry + 1, 0} - {pr.entry})]
        yield f"prog{p}.node", [(pr, "node", v) for v in sorted({n_nodes + 1, 0, 1, n_nodes} - {pr.node})]
        yield f"prog{p}.flags", [(pr, "flags", pr.flags ^ (1 << k)) for k in range(8)]
    for n in range(n_nodes + 1):
        yield f"node{n}.flags", [(m.nodes[n], "flags", m.nodes[n].flags ^ (1 << k)) for k in range(8)]
    for k in range(n_socks):
        sk = m.socks[k]
        yield f"sock{k}.kind", [(sk, "kind", v) for v in sorted({0, 1, 2, 3, 4} - {sk.kind})]
        yield f"sock{k}.port", [(sk, "port", v) for v in sorted({0, 1, 2, 80} - {sk.port})]
        yield f"sock{k}.node", [(sk, "node", v) for v in sorted({0, 1, n_nodes, n_nodes + 1} - {sk.node})]
    for k in range(n_services):
        sv = m.services[k]
        yield f"service{k}.vaddr", [(sv, "vaddr", v) for v in sorted(set(range(n_socks + 1)) - {sv.vaddr})]
        yield f"service{k}.n_servers", [(sv, "n_servers", v) for v in sorted({0, 1, 6, 7, 0x80, 0x81} - {sv.n_servers})]
        yield f"service{k}.server0", [(sv.servers, 0, v) for v in sorted(set(range(n_socks + 1)) - {sv.servers[0]})]
    if n_services:          # the same address twice (the spare slot holds a copy of service 0)
        m.services[n_services] = m.services[0]
        yield "service.twice", [(s, "n_services", n_services + 1)]


def config_mutations(cfg):
    nan = float("nan")
    yield "cfg.lat", [(cfg, "lat_lo_ns", cfg.lat_hi_ns), (cfg, "lat_hi_ns", 0), (cfg, "lat_hi_ns", 1 << 40)]
    yield "cfg.loss", [(cfg, "packet_loss_rate", v) for v in (-0.5, 1.5, nan, 1.0, 0.25)]
    yield "cfg.buggify", [(cfg, "buggify", 1)]
    yield "cfg.n_lat_table", [(cfg, "n_lat_table", v) for v in (0, 1, 5)]
    yield "cfg.lat_table", [(cfg.lat_table_lo_ns, 0, cfg.lat_table_hi_ns[0] or 1), (cfg.lat_table_hi_ns, 3, 0), (cfg.lat_table_hi_ns, 0, 1 << 40)]
    yield "cfg.n_loss_table", [(cfg, "n_loss_table", 4)]


def limit_mutations(lim):
    """Every madsim_limits_t field make_geometry reads, at its ceiling, just past it and far past it."""
    for f, vals in (("max_tasks", (1, 8, 9, 254, 255, 100000)), ("mbox_regs", (A.LIMIT_NONE, 255, 256)), ("mbox_msgs", (A.LIMIT_NONE, 127, 128, 255, 256)),
                    ("heap_lds_slots", (1, 2, 64, 600, 3000, 100000)), ("heap_spill_slots", (0, 1, 4096)), ("lanes_per_wave", (7, 8, 32, 64, 65)),
                    ("max_conns", (127, 128)), ("chan_queue", (15, 16)), ("max_steps", (1,)), ("no_trace_hash", (1,)), ("time_limit_ns", (1,)),
                    ("state_mem", (1, 2, 3, 4, 0x102, 0x202, 0x203, 0x400, 0x10000))):
        yield f"lim.{f}", [(lim, f, v) for v in vals]
    # two fields at once where one alone cannot reach a rule: explicit lanes with the global and the compact layout, a heap that spills in the compact one
    for sm in (2, 3):
        for lw in (8, 16, 32, 64):
            yield f"lim.state_mem={sm}+lanes={lw}", [(lim, "state_mem", sm), (lim, "lanes_per_wave", lw)], True
    yield "lim.compact+spill", [(lim, "state_mem", 3), (lim, "heap_spill_slots", 8)], True
    yield "lim.wave_lds", [(lim, "lanes_per_wave", 64), (lim, "heap_lds_slots", 600)], True
    yield "lim.wave_lds8", [(lim, "lanes_per_wave", 8), (lim, "heap_lds_slots", 1200), (lim, "max_tasks", 200)], True


def directed_refused():
    """Workloads for the rules no single field of the bases reaches."""
    wl = W.WorkloadBuilder()          # 32 ephemeral endpoints of one node: 32 entries + 32 candidate ports
    n = wl.create_node()
    for _ in range(32):
        wl.addr(n, 0, ip="unspecified")
    wl.main().done()
    yield "directed/refused/ephemeral_candidates", wl.build(), probe_config()


def _get(obj, f):
    return obj[f] if isinstance(f, int) else getattr(obj, f)


def _set(obj, f, v):
    if isinstance(f, int):
        obj[f] = v
    else:
        setattr(obj, f, v)


def record_refused(verbose=None):
    """-> ({base: [mutants, digest over their answers (codes and messages), digest over what the accepted ones planned]}, the tally of answers)."""
    tally = {}

    def run(name, m, cfg, lim, groups, entry, answers, plans):
        for label, steps, *together in groups:
            row = []
            for batch in ([steps] if together or not steps else [[s] for s in steps]):     # together: every step applied, one answer
                old = [_get(o, f) for o, f, _ in batch]
                for o, f, v in batch:
                    _set(o, f, v)
                r = emu.host_plan(m.ref() if m is not None else None, cfg, lim)
                row.append(_key(r))
                if r["validate"][0] == 0:
                    plans.update(_answer(r))
                    for t in r.get("table", ()):
                        plans.update(t)
                for (o, f, _), v in zip(batch, old):
                    _set(o, f, v)
            for key in row:
                tally[key] = tally.get(key, 0) + 1
            answers.update(repr((label, row)).encode())
            entry[0] += len(row)
            if verbose is not None:
                verbose.write(f"{name} {label}: {row} {plans.hexdigest()[:16]}\n")

    refused = {}
    for name, w, cfg in list(mutation_bases()) + list(directed_refused()) + [("null", None, probe_config())]:
        entry, answers, plans = [0], hashlib.sha256(), hashlib.sha256()
        if name.startswith("directed/refused") or w is None:
            run(name, w, cfg, None, [("as built", [])], entry, answers, plans)
        else:
            m = Mutable(w)
            run(name, m, cfg, None, field_mutations(m), entry, answers, plans)
            if name.startswith("core/") or name in ("one_op/SET_LATENCY", "one_op/DONE", "one_op/CONNECT"):
                run(name, m, cfg, None, config_mutations(cfg), entry, answers, plans)
                lim = A.Limits()
                run(name, m, cfg, lim, limit_mutations(lim), entry, answers, plans)
        refused[name] = [entry[0], answers.hexdigest()[:16], plans.hexdigest()[:16]]
    return refused, tally


def record(verbose=None):
    """-> (the record, every message in it).  Messages and codes stand in full in `messages`; the tallies count answers by their index there."""
    table, index = [], {}

    def indexed(tally):
        for key in tally:
            if key not in index:
                index[key] = len(table)
                table.append(key)
        return {str(index[k]): n for k, n in sorted(tally.items(), key=lambda kv: index[kv[0]])}

    bench = {name: full_plan(w, cfg, lim) for name, w, cfg, lim in accepted() if name.startswith("bench/")}
    acc, running, tallies = {}, {}, {}
    for name, w, cfg, lim in accepted():
        if name not in running:
            running[name] = [0, hashlib.sha256(), hashlib.sha256()]
        e = running[name]
        e[0] += 1
        plan_member(name, w, cfg, lim, e[1], e[2], tallies.setdefault(name.split("/")[0], {}), verbose)
        acc[name] = [e[0], e[1].hexdigest()[:16], e[2].hexdigest()[:16]]
    refused, tally = record_refused(verbose)
    rec = {"bench": bench, "accepted": acc, "accepted_answers": {sec: indexed(t) for sec, t in tallies.items()},
           "refused": refused, "refused_answers": indexed(tally), "messages": table}
    return rec, set(table)


# ---- the condition on the record: every rule's message occurs in it ---------------------------------------------------------------------------
# message literals of validate() / make_geometry() that no input reaches, each with the reason
UNREACHABLE = {
    "max_tasks must be <= 254": "the line above it clamps the value",
    "no kernel build for this geometry: ": "variant_mismatch() re-checks what make_geometry itself just chose: a net under its own logic, tripped by no input",
    "no kernel build for this geometry: the workgroups of a CU exceed its LDS": "blocks_per_cu is lds_per_cu / lds_alloc(W) or less: the same net, for the LDS arithmetic",
}


def fail_literals(path=HEADER):
    """{function: [message literal]} of every fail( in validate() and make_geometry(), adjacent literals joined, either arm of a ?: on its own."""
    src = open(path, encoding="utf-8").read()
    out = {}
    for fn, end in (("validate", "inline madsim_config_t probe_config"), ("make_geometry", "struct DeviceTables")):
        start = src.index(f"inline int {fn}(")
        body = re.sub(r"//[^\n]*", lambda c: "" if c.group(0).count('"') % 2 == 0 else c.group(0), src[start:src.index(end, start)])
        lits = []
        for m in re.finditer(r"\bfail\(err,", body):
            i, depth, cur, stmt = m.end(), 1, None, []
            while depth:                                   # to the call's closing parenthesis, strings skipped as strings
                c = body[i]
                if c == '"':
                    j = i + 1
                    while body[j] != '"':
                        j += 2 if body[j] == "\\" else 1
                    text = body[i + 1:j].encode().decode("unicode_escape")
                    cur = text if cur is None else cur + text
                    i = j + 1
                    continue
                if not c.isspace() and cur is not None:
                    stmt.append(cur)
                    cur = None
                depth += (c == "(") - (c == ")")
                i += 1
            lits += stmt
        out[fn] = lits
    return out


def uncovered(msgs, path=HEADER):
    """The reachable message literals of the two functions that no recorded message contains."""
    return [(fn, lit) for fn, lits in fail_literals(path).items() for lit in lits if lit not in UNREACHABLE and not any(lit in m for m in msgs)]
