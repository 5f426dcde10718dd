"""CPU reference for interval tickers (MS_OP_INTERVAL / MS_OP_TICK / MS_OP_INTERVAL_RESET), test infrastructure.

`IntervalSim` extends tests/scope_sim.py's `ScopeSim` (itself the generator restatement of tests/golden/make_golden_async.py) with
madsim's `Interval`, which is a `Sleep` plus a period and a missed-tick rule (madsim/src/sim/time/interval.rs).  The rules, in the
order a ticker meets them:

1. Creation.  interval(p) is interval_at(now, p), and interval_at(start, p) makes sleep_until(start) (interval.rs:38-58), so the
   first deadline carries the 1 ms floor of TimeHandle::sleep_until (time/mod.rs:118-124): max(start, now + 1 ms).  Executing
   INTERVAL again is a reassignment: the old ticker is dropped, its pending timers stay in the heap and fire for nothing.
2. A tick polls the Sleep (poll_tick, interval.rs:142-169).  Sleep::poll is Ready when now >= deadline (time/sleep.rs:47-54): then
   the tick completes in the same poll, without registering a timer and without yielding to the executor.
3. While the deadline lies ahead, every poll that leaves the tick Pending registers ANOTHER timer at the deadline (sleep.rs:50-53).
   A wake before the deadline (a stale timer of a tick a timeout scope dropped, or the scope's own Sleep) is such a poll.
4. On completion the Sleep is reset (Sleep::reset has no floor, sleep.rs:39-41).  A tick is late when now > deadline + 5 ms,
   strictly (interval.rs:158); a late tick takes its next deadline from the behaviour (interval.rs:76-101): Burst (the default)
   deadline + period, Delay now + period, Skip now + period - (now - deadline) % period.  A tick that is not late always takes
   deadline + period.
5. The tick returns the deadline it was scheduled for, not `now` (the clock runs 50 ns past a timer's deadline when it fires,
   time/mod.rs:45-60).  TICK with a & 1 folds that instant into obs_hash, as MS_OP_TRACE_TIME a=1 folds `now`.
6. reset() sets the deadline to now + period (interval.rs:174-176): no floor, no behaviour.

The ticker is a local of the task body: a spawned program has none of its own until it runs INTERVAL, and it dies with the task.
INTERVAL, TICK and RESET are handled here, by `_one`, which ScopeSim calls for every instruction of a body and of a scope's block;
every other instruction goes on to ScopeSim._one (one instruction at a time through the parent's interpreter).
"""
from madsim_amd import _abi as A
from tests import scope_sim as S

MGA = S.MGA
INTERVAL, TICK, RESET = A.OP["INTERVAL"], A.OP["TICK"], A.OP["INTERVAL_RESET"]
MARK, SLEEP_UNTIL = A.OP["MARK"], A.OP["SLEEP_UNTIL"]
MS = 1_000_000
LATE_NS = 5 * MS
BEHAVIORS = ("burst", "delay", "skip")


class Ticker:
    def __init__(self, behavior, period, deadline):
        self.behavior, self.period, self.deadline = behavior, period, deadline


class IntervalSim(S.ScopeSim):
    def __init__(self, w, cfg, seed):
        super().__init__(w, cfg, seed)
        self.tickers = {}                                   # task -> its Ticker (a local of the task body)
        self.ticks_done = 0                                 # ticks completed
        self.ticks_immediate = 0                            # ... at their first poll: no timer, no yield (rule 2)
        self.ticks_late = {b: 0 for b in BEHAVIORS}         # late ticks per behaviour (rule 4)
        self.tick_spurious = 0                              # polls of a pending tick before its deadline after the first (rule 3)
        self.tick_instants = []                             # what each completed tick returned (rule 5)
        self.tick_log = []                                  # (deadline, now) of each completed tick

    def _one(self, t, pc):
        op, a, b, imm = self.insns[pc]
        if op == INTERVAL:
            start = t.t0 if a & 4 else self.clock
            self.tickers[t] = Ticker(BEHAVIORS[a & 3], b * 10**9 + imm, self.sleep_deadline(start))
            return pc + 1
        if op == RESET:
            k = self.tickers[t]
            k.deadline = self.clock + k.period
            return pc + 1
        if op == TICK:
            yield from self._tick(t, a & 1)
            return pc + 1
        return (yield from super()._one(t, pc))

    def _tick(self, t, fold):
        k = self.tickers[t]
        polls = 0
        while self.clock < k.deadline:                      # Sleep::poll, not elapsed: ANOTHER timer, Pending
            if polls:
                self.tick_spurious += 1
            polls += 1
            self.timer_add(k.deadline, lambda: self.wake(t))
            yield
        if not polls:
            self.ticks_immediate += 1
        due, now = k.deadline, self.clock
        if now > due + LATE_NS:
            self.ticks_late[k.behavior] += 1
            if k.behavior == "burst":
                k.deadline = due + k.period
            elif k.behavior == "delay":
                k.deadline = now + k.period
            else:
                k.deadline = now + k.period - (now - due) % k.period
        else:
            k.deadline = due + k.period
        self.ticks_done += 1
        self.tick_instants.append(due)
        self.tick_log.append((due, now))
        if fold:
            self.obs_list.append(due)
            self.obs = ((self.obs ^ due) * MGA.FNV_PRIME) & MGA.M64

    def finish(self, t, outcome):
        super().finish(t, outcome)
        self.tickers.pop(t, None)


def run(w, cfg, seed, time_limit=0):
    return IntervalSim(w, cfg, seed).run(time_limit)


def stats(sim):
    return dict(done=sim.ticks_done, immediate=sim.ticks_immediate, late=dict(sim.ticks_late), spurious=sim.tick_spurious)


# ---- the oracle yardstick: straight-line ticker programs restated with MARK + SLEEP_UNTIL ---------------------------------------
def rewrite_ticks_as_sleep_until(w):
    """A copy of a straight-line ticker workload (no jumps, one INTERVAL per program, ticks that do not fold, no RESET) with every
    INTERVAL(p) replaced by MARK and the k-th TICK after it by SLEEP_UNTIL(t0 + 1 ms + k p).  Equal to the original exactly when every
    tick is still pending at its first poll with at least 1 ms to go (then sleep_until's floor does not apply and no tick is late):
    the caller's programs guarantee it."""
    from madsim_amd import workload as W
    n = w.struct.n_insns
    entries = {w.progs[p].entry for p in range(w.struct.n_progs)}
    out, period, k = [], None, 0
    for i in range(n):
        ins = w.insns[i]
        op, a, b, imm = ins.op, ins.a, ins.b, ins.imm
        if i in entries:
            period = None                               # (programs without a ticker may loop)
        if (op in S.JUMPS and period is not None) or op == RESET or (op == TICK and a & 1) or (op == INTERVAL and a & 4):
            raise ValueError("not a straight-line ticker program")
        if op == INTERVAL:
            period, k = b * 10**9 + imm, 0
            out.append(A.Insn(MARK, 0, 0, 0))
        elif op == TICK:
            d = MS + k * period
            out.append(A.Insn(SLEEP_UNTIL, 0, d // 10**9, d % 10**9))
            k += 1
        else:
            out.append(A.Insn(op, a, b, imm))
    progs = [A.Prog(w.progs[i].node, w.progs[i].flags, w.progs[i].entry) for i in range(w.struct.n_progs)]
    nodes = [w.nodes[i] for i in range(w.struct.n_nodes + 1)]
    socks = [w.socks[i] for i in range(w.struct.n_socks)]
    services = [w.services[i] for i in range(w.struct.n_services)]
    pm = [w.panic_match[i] for i in range(8 * len(nodes))] if w.panic_match else None
    r = W.BuiltWorkload(nodes, progs, socks, out, services, pm, w.struct.panic_dyn_max)
    for attr in ("panic_patterns", "panic_text_of", "payloads", "rpc_messages"):
        if hasattr(w, attr):
            setattr(r, attr, getattr(w, attr))
    return r
