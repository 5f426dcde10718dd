"""CPU reference for the selects of ABI v7 (MS_OP_RECV_OR_TICK, MS_OP_RECV_TIMEOUT_AT), test infrastructure.

`SelectSim` extends tests/interval_sim.py's `IntervalSim` with `select_biased(t, arms)`, the primitive madsim's own `timeout` is
built on (`select_biased! { fut, sleep }`, time/mod.rs:128-140) and that make_golden_async.py's `Sim.timeout` restates for one
receive and one Sleep.  Here the arms are any generators.  The rules, in the order a select meets them:

1. Each poll of the select polls the arms in the program's order.  The first arm to return wins and the others are dropped
   (`close()`: their `finally` blocks are their Drop impls).  An arm that was never polled has done nothing.
2. The recv arm is Endpoint::recv_from_raw (net/endpoint.rs:140-149): nothing before its first poll.  That poll does Mailbox::recv
   (endpoint.rs:353-362): take a queued message of the tag, or register.  Once the oneshot holds the message, rand_delay follows
   (net/mod.rs:287-292): one with() draw (plus buggify), and a Sleep with the 1 ms floor, so always Pending at first.
3. A recv arm dropped after it took its message loses it: the draw was made and the rand_delay's timer stays in the heap.  This is
   madsim's own cancel-unsafety.  A recv arm dropped while registered leaves a dead registration, as RECV_TIMEOUT's does.
4. The tick arm is Interval::poll_tick (time/interval.rs:142-169) under tests/interval_sim.py's rules: a passed deadline is Ready in
   this poll with no timer; otherwise ANOTHER timer at the deadline on every poll that leaves it Pending.
5. A tick arm dropped while pending keeps the ticker and its deadline.  Its timers stay in the heap and wake the task later for
   nothing: a stale wake.
6. Tick first, deadline passed at the select's first poll: the tick wins without yielding.  The recv arm is never polled, so there
   is no registration and no draw, and the body goes on in the same poll.
7. Recv first, deadline passed, a message queued: the recv arm takes the message and draws its rand_delay (Pending), then the tick
   wins: rule 3, the message is lost.
8. Result.  The recv arm wins: val and from as MS_OP_RECV_TIMEOUT sets them, the typed-RPC tags' request word included.  The tick
   wins: val := VAL_TIMEOUT, the ticker advances as a TICK's does, and flag bit 1 folds the tick's scheduled instant.
9. timeout_at(t0 + d, recv) (time/mod.rs:144-156) is the select of the recv arm and a Sleep made by sleep_until(t0 + d): its
   deadline max(t0 + d, now + 1 ms) is fixed when the op starts, and a message does not move it.  t0 is the program's last MARK.

Counters: selects won by each arm (`won`), messages lost in rand_delay (`lost`), tick wins at the select's first poll
(`tick_immediate`), the wakes by timers of dropped tick arms (`stale_wakes`) and the GlobalRng calls the recv arms made
(`recv_arm_draws`).
"""
from madsim_amd import _abi as A
from tests import interval_sim as I

MGA = I.MGA
RECV_OR_TICK, RECV_TIMEOUT_AT = A.OP["RECV_OR_TICK"], A.OP["RECV_TIMEOUT_AT"]
RECV_TIMEOUT = A.OP["RECV_TIMEOUT"]
MS = I.MS


class _Arm:
    """What the select knows of a tick arm after it is gone: whether it was dropped (its timers are stale from then on)."""
    dropped = False


class SelectSim(I.IntervalSim):
    def __init__(self, w, cfg, seed):
        super().__init__(w, cfg, seed)
        self.won = {"recv": 0, "tick": 0, "deadline": 0}    # selects won by each arm (deadline: timeout_at's Sleep)
        self.lost = 0                                       # messages taken by a recv arm that was dropped in its rand_delay (rule 3)
        self.tick_immediate = 0                             # tick wins at the select's first poll (rule 6 and recv-first rule 7)
        self.stale_wakes = 0                                # timers of dropped tick arms that fired on a live task (rule 5)
        self.recv_arm_draws = 0                             # GlobalRng calls made inside the recv arms of selects (their rand_delay draws)

    def select_biased(self, t, arms):
        """select_biased! over `arms` (generators, in poll order): returns (index of the winner, its value); `select_yields` is
        how often the select was Pending before it (0: won at its first poll)."""
        self.select_yields = 0
        try:
            while True:
                for i, g in enumerate(arms):
                    calls = self.rng.calls
                    try:
                        next(g)
                    except StopIteration as e:
                        return i, e.value
                    finally:
                        if g.gi_code is self.recv_raw.__code__:
                            self.recv_arm_draws += self.rng.calls - calls
                self.select_yields += 1
                yield
        finally:
            for g in arms:
                # (recv_from_raw parked in its rand_delay: `yield from` is active there — the message it took goes with it)
                if g.gi_frame is not None and g.gi_code is self.recv_raw.__code__ and g.gi_yieldfrom is not None:
                    self.lost += 1
                g.close()

    def _tick_arm(self, t, fold, arm):
        """ticker.tick() as an arm: rule 4 with the timers marked as this arm's, then the completion of IntervalSim._tick."""
        k = self.tickers[t]
        while self.clock < k.deadline:
            self.timer_add(k.deadline, lambda: self._tick_timer(t, arm))
            yield
        yield from self._tick(t, fold)                      # (deadline passed: completes without yielding)

    def _tick_timer(self, t, arm):
        if arm.dropped and t.alive:
            self.stale_wakes += 1
        self.wake(t)

    def _one(self, t, pc):
        op, a, b, imm = self.insns[pc]
        if op == RECV_OR_TICK:
            arm = _Arm()
            recv, tick = self.recv_raw(t, a, b >> 8), self._tick_arm(t, b & 2, arm)
            arms = [tick, recv] if b & 1 else [recv, tick]
            try:
                i, v = yield from self.select_biased(t, arms)
            finally:
                arm.dropped = True
            if arms[i] is recv:
                self.won["recv"] += 1
                self._recv_result(t, b, v)
            else:
                self.won["tick"] += 1
                self.tick_immediate += self.select_yields == 0
                t.val = A.VAL_TIMEOUT
            return pc + 1
        if op == RECV_TIMEOUT_AT:
            deadline = self.sleep_deadline(t.t0 + (b & 0xFF) * 10**9 + imm)
            i, v = yield from self.select_biased(t, [self.recv_raw(t, a, b >> 8), self.sleep_until(t, deadline)])
            if i == 0:
                self.won["recv"] += 1
                self._recv_result(t, b, v)
            else:
                self.won["deadline"] += 1
                t.val = A.VAL_TIMEOUT
            return pc + 1
        return (yield from super()._one(t, pc))

    @staticmethod
    def _recv_result(t, b, msg):                            # MS_OP_RECV_TIMEOUT's Ok arm (make_golden_async.py)
        t.val, t.frm = msg[0], msg[1]
        if (b >> 8) >= 0x80:
            t.aux = msg[2]


def run(w, cfg, seed, time_limit=0):
    return SelectSim(w, cfg, seed).run(time_limit)


def stats(sim):
    return dict(won=dict(sim.won), lost=sim.lost, tick_immediate=sim.tick_immediate, stale_wakes=sim.stale_wakes)


# ---- the oracle yardsticks: programs whose select is exactly an op the unchanged oracle knows ---------------------------------------
def _rewrite(w, fn):
    from madsim_amd import workload as W
    out = [fn(w.insns[i]) for i in range(w.struct.n_insns)]
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


def rewrite_timeout_at_as_timeout(w):
    """Every RECV_TIMEOUT_AT as RECV_TIMEOUT with the same operands.  Equal to the original exactly when every timeout_at starts at
    its program's MARK instant (MARK right before it, nothing between that lets time pass): then t0 + d == now + d."""
    def f(ins):
        return A.Insn(RECV_TIMEOUT if ins.op == RECV_TIMEOUT_AT else ins.op, ins.a, ins.b, ins.imm)
    return _rewrite(w, f)


def rewrite_fresh_select_as_timeout(w):
    """INTERVAL p; RECV_OR_TICK (recv first, no fold) as MARK; RECV_TIMEOUT 1 ms.  A fresh ticker's first deadline is
    sleep_until(now)'s, max(now, now + 1 ms) = now + 1 ms, and a recv-first select over it polls the recv arm, then that Sleep, on
    every poll: timeout(1 ms, recv) exactly (the MARK keeps the instruction count, its t0 is never read).  A tick that wins advances
    the ticker, which no later op of these programs looks at."""
    out = []
    n = w.struct.n_insns
    for i in range(n):
        ins = w.insns[i]
        if ins.op == RECV_OR_TICK:
            prev = w.insns[i - 1] if i else None
            if ins.b & 3 or prev is None or prev.op != I.INTERVAL:
                raise ValueError("not INTERVAL; RECV_OR_TICK (recv first, no fold)")
    def f(ins):
        if ins.op == I.INTERVAL:
            return A.Insn(I.MARK, 0, 0, 0)
        if ins.op == RECV_OR_TICK:
            return A.Insn(RECV_TIMEOUT, ins.a, ins.b & 0xFF00, MS)
        if ins.op in (I.TICK, I.RESET):
            raise ValueError("a ticker op other than the select")
        return A.Insn(ins.op, ins.a, ins.b, ins.imm)
    return _rewrite(w, f)
