"""CPU reference for timeout scopes (MS_OP_TIMEOUT_BEGIN / MS_OP_TIMEOUT_END), test infrastructure.

`ScopeSim` extends the generator restatement of tests/golden/make_golden_async.py, where `timeout()` is literally
`select_biased! { fut, sleep }` over a sub-generator (`Sim.timeout`).  What it restates:

* time::timeout / TimeHandle::timeout        madsim/src/sim/time/mod.rs:128-140 — the Sleep is made when timeout() is called
  (sleep / sleep_until, :111-124: deadline max(now + d, now + 1 ms), no draw, no timer); every poll polls the inner future
  first, then the Sleep; Err(Elapsed) drops the inner future wherever it is parked.
* Sleep::poll                                time/sleep.rs:47-54 — ANOTHER timer on every not-elapsed poll (Sim.timeout does it).
* the async block's locals                   the (tx, rx) of a connect1 inside the block (net/endpoint.rs:178-193) drop when the block
  ends, completed or dropped: `finally` below, Sim.conn_drop (tx then rx, each with its guard).
* madsim-tonic's unary call                  madsim-tonic/src/client.rs:52-78,208-219: timeout(d, async { connect1?; send; recv }).

A scope is run as `self.timeout(t, d, self._block(t, begin + 1, end))`.  Every other instruction is delegated, ONE at a time, to
`Sim.body` itself: it runs on a proxy whose `insns` answers the first fetch and ends the body with the next pc at the second, so
this module copies none of the parent's interpreter.
"""
import importlib.util
import os

from madsim_amd import _abi as A

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_async", os.path.join(_HERE, "golden", "make_golden_async.py"))
MGA = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MGA)
Sim = MGA.Sim

BEGIN, END, CONNECT = A.OP["TIMEOUT_BEGIN"], A.OP["TIMEOUT_END"], A.OP["CONNECT"]
RECV_TIMEOUT, RECV, RPC_CALL = A.OP["RECV_TIMEOUT"], A.OP["RECV"], A.OP["RPC_CALL"]
JUMPS = (A.OP["DJNZ"], A.OP["JMP"], A.OP["JEQ"])


class _Next(Exception):
    def __init__(self, pc):
        super().__init__(pc)
        self.pc = pc


class _OneInsn:
    """The Sim seen through one instruction: `insns[pc]` answers once; the second fetch raises _Next(the pc it asked for)."""

    def __init__(self, sim):
        object.__setattr__(self, "_sim", sim)
        object.__setattr__(self, "_n", 0)

    def __getattr__(self, k):
        return self if k == "insns" else getattr(self._sim, k)

    def __setattr__(self, k, v):
        setattr(self._sim, k, v)

    def __getitem__(self, pc):
        if self._n:
            raise _Next(pc)
        object.__setattr__(self, "_n", 1)
        return self._sim.insns[pc]


class ScopeSim(Sim):
    def body(self, t, pc):
        while True:
            op, a, b, imm = self.insns[pc]
            if op == BEGIN:
                made = [False]
                how, _ = yield from self.timeout(t, a * 10**9 + imm, self._block(t, pc + 1, b, made))
                if how != "ok":
                    t.val = A.VAL_TIMEOUT
                pc = b + 1
                continue
            pc = yield from self._one(t, pc)
            if pc is None:                          # the body returned (DONE)
                return

    def _one(self, t, pc):
        try:
            yield from Sim.body(_OneInsn(self), t, pc)
        except _Next as e:
            return e.pc
        return None

    def _block(self, t, pc, end, made):
        """The async block: its instructions up to END (a jump to END returns early).  A connect1 that got past its rand_delay
        has made the block's (tx, rx) — the old pair went with it (the VM's one-pair rule) — and they drop with the block."""
        try:
            while pc != end:
                op = self.insns[pc][0]
                pc = yield from self._one(t, pc)
                if op == CONNECT:
                    made[0] = True
        finally:
            if made[0]:
                self.conn_drop(t)


def run(w, cfg, seed, time_limit=0):
    return ScopeSim(w, cfg, seed).run(time_limit)


# ---- timeout(d, f) == timeout(d, async { f.await }): the single-await timeouts rewritten into scopes ------------------------------
def rewrite_into_scopes(w):
    """A copy of the workload with every MS_OP_RECV_TIMEOUT as BEGIN d; RECV; END and every timed MS_OP_RPC_CALL as BEGIN d;
    RPC_CALL (untimed); END — jump targets and program entries relocated (a jump to the timed op lands on its BEGIN)."""
    from madsim_amd import workload as W
    n = w.struct.n_insns
    old = [w.insns[i] for i in range(n)]
    newpc, k = [], 0
    for ins in old:
        newpc.append(k)
        k += 3 if (ins.op == RECV_TIMEOUT or (ins.op == RPC_CALL and ins.imm >> 8)) else 1
    out = []
    for ins in old:
        op, a, b, imm = ins.op, ins.a, ins.b, ins.imm
        if op in JUMPS:
            b = newpc[b]
        if op == RECV_TIMEOUT:
            here = len(out)
            out += [A.Insn(BEGIN, b & 0xFF, here + 2, imm), A.Insn(RECV, a, b & 0xFF00, 0), A.Insn(END, 0, 0, 0)]
        elif op == RPC_CALL and imm >> 8:
            here, ms = len(out), imm >> 8
            out += [A.Insn(BEGIN, ms // 1000, here + 2, (ms % 1000) * 1_000_000), A.Insn(RPC_CALL, a, b, imm & 0xFF), A.Insn(END, 0, 0, 0)]
        else:
            out.append(A.Insn(op, a, b, imm))
    progs = []
    for i in range(w.struct.n_progs):
        p = w.progs[i]
        progs.append(A.Prog(p.node, p.flags, newpc[p.entry]))
    nodes = [w.nodes[i] for i in range(w.struct.n_nodes + 1)]
    socks = [w.socks[i] for i in range(w.struct.n_socks)]
    services = [w.services[i] for i in range(w.struct.n_services)]
    pm = [w.panic_match[i] for i in range(8 * len(nodes))] if w.panic_match else None
    r = W.BuiltWorkload(nodes, progs, socks, out, services, pm, w.struct.panic_dyn_max)
    for attr in ("panic_patterns", "panic_text_of", "payloads", "rpc_messages"):
        if hasattr(w, attr):
            setattr(r, attr, getattr(w, attr))
    return r


def has_timed_ops(w):
    return any(w.insns[i].op == RECV_TIMEOUT or (w.insns[i].op == RPC_CALL and w.insns[i].imm >> 8) for i in range(w.struct.n_insns))
