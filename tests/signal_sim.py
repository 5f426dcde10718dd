"""CPU reference for ctrl-c signals (MS_OP_CTRL_C, MS_OP_SEND_CTRL_C, MS_OP_RECV_OR_CTRL_C), test infrastructure.

`SignalSim` extends tests/select_sim.py's `SelectSim` (and through it the interval, scope and base restatements) with madsim's
`signal::ctrl_c()` (madsim/src/sim/signal.rs:4-8) and `Handle::send_ctrl_c` (task/mod.rs:426-441) over `NodeInfo.ctrl_c:
Mutex<Option<watch::Sender<()>>>` (task/mod.rs:108-110,166-175).  The rules, in the order a program meets them:

1. Install.  `ctrl_c()` is an async fn: nothing happens before its first poll.  That poll calls `node.ctrl_c()` on the TASK's own
   NodeInfo: `get_or_insert_with(watch::channel)` — the handler is installed for the rest of that NodeInfo's life, also after the
   task has ended — and `subscribe()`.  `restart` makes a new NodeInfo with `ctrl_c: None`; `kill` alone keeps the NodeInfo.
2. Subscribe.  A new Receiver starts at the channel's current version, so `changed()` is Pending at that first poll and sees only
   sends after it.  It makes no timer and draws nothing.  It stays registered until the future is dropped.
3. Send, handler installed.  `tx.send(())` fails without receivers (nothing happens: the signal is lost).  With receivers the
   version moves and every registered waiter gets `waker.wake()`: the ordinary wake path (`Sim.wake`: a task that is scheduled already
   is not pushed again; a paused node parks the runnable when it is popped).  The woken task finds the new version on its next poll.
4. Send, no handler.  `kill_id(node)`: what MS_OP_KILL does.
5. `select! { biased; ctrl_c(), recv_from(tag) }` in either order is `select_biased` of tests/select_sim.py over the two futures:
   every poll polls both in the program's order, the first Ready wins, the other is dropped.  A dropped recv arm loses the message it
   took (select_sim rule 3).  A dropped ctrl-c arm drops its Receiver, so a signal between two selects is lost, and so is one that
   reaches a recv-first select in the poll where its message is ready.
6. The order in which `watch::Sender::send` wakes SEVERAL waiters is tokio's (its waiter lists are picked by a thread-local generator
   the seed does not control).  A send that would schedule two or more tasks — waiters that are alive and not scheduled yet — is
   outside the model: `Unsupported`, reported as verdict MADSIM_UNSUPPORTED with every other field 0.

Counters: `killed_by_signal` (rule 4), `caught` (ctrl_c() calls and ctrl-c arms that completed), `lost_signals` (sends without a
receiver, and signals a recv-first select dropped), `lost_messages` (messages a ctrl-c win took with the recv arm), `unsupported`.
"""
from madsim_amd import _abi as A
from tests import select_sim as S

MGA = S.MGA
CTRL_C, SEND_CTRL_C, RECV_OR_CTRL_C = A.OP["CTRL_C"], A.OP["SEND_CTRL_C"], A.OP["RECV_OR_CTRL_C"]
KILL = A.OP["KILL"]
MS = S.MS
ZERO_FIELDS = ("steps", "clock_ns", "msg_count", "rng_calls", "trace_hash", "obs_hash")


class Unsupported(Exception):
    """A send that would schedule two or more waiters (rule 6)."""


class _Watch:
    """NodeInfo.ctrl_c = Some(watch::Sender<()>): the version and the live Receivers (each registered with the Notify)."""

    def __init__(self):
        self.version, self.receivers = 0, []


class _Receiver:
    def __init__(self, task, seen):
        self.task, self.seen = task, seen


class SignalSim(S.SelectSim):
    def __init__(self, w, cfg, seed):
        super().__init__(w, cfg, seed)
        self.killed_by_signal = 0
        self.caught = 0
        self.lost_signals = 0
        self.lost_messages = 0
        self.unsupported = 0

    # ---- signal::ctrl_c / NodeInfo::ctrl_c ------------------------------------------------------------------------------------
    def ctrl_c(self, t, out=None):
        """`ctrl_c().await` as a generator (a future): `out` (a list) is handed the Receiver, for the select to look at after a drop."""
        info = t.info
        if getattr(info, "ctrl_c", None) is None:
            info.ctrl_c = _Watch()                          # get_or_insert_with: "ctrl-c signal handler installed"
        ch = info.ctrl_c
        rx = _Receiver(t, ch.version)                       # subscribe(): sees only later versions
        ch.receivers.append(rx)
        if out is not None:
            out.append(rx)
        try:
            while rx.seen == ch.version:                    # changed(): Pending, registered with the Notify; no timer
                yield
            rx.seen = ch.version
        finally:
            ch.receivers.remove(rx)                         # the Receiver drops with the future

    # ---- TaskHandle::send_ctrl_c ------------------------------------------------------------------------------------------------
    def send_ctrl_c(self, node):
        ch = getattr(self.node_info[node], "ctrl_c", None)
        if ch is None:                                      # "ctrl-c" has never been called: kill node
            self.killed_by_signal += 1
            self.kill(node)
            return
        if not ch.receivers:                                # tx.send(()) -> Err: no receiver, nothing changes
            self.lost_signals += 1
            return
        would = [rx.task for rx in ch.receivers if rx.task.alive and not rx.task.sched]
        if len(would) >= 2:
            raise Unsupported()
        ch.version += 1
        for rx in list(ch.receivers):
            self.wake(rx.task)

    def _one(self, t, pc):
        op, a, b, imm = self.insns[pc]
        if op == CTRL_C:
            yield from self.ctrl_c(t)
            self.caught += 1
            return pc + 1
        if op == SEND_CTRL_C:
            self.send_ctrl_c(a)
            return pc + 1
        if op == RECV_OR_CTRL_C:
            held = []
            sig, recv = self.ctrl_c(t, held), self.recv_raw(t, a, b >> 8)
            arms = [recv, sig] if b & 1 else [sig, recv]
            lost0 = self.lost
            i, v = yield from self.select_biased(t, arms)
            if arms[i] is recv:
                self._recv_result(t, b, v)
                if held and held[0].seen != t.info.ctrl_c.version:      # the arm was dropped with a signal it had not looked at
                    self.lost_signals += 1
            else:
                self.caught += 1
                self.lost_messages += self.lost - lost0
                t.val = A.VAL_TIMEOUT
            return pc + 1
        return (yield from super()._one(t, pc))

    def run(self, time_limit=0):
        try:
            return super().run(time_limit)
        except Unsupported:
            self.unsupported += 1
            r = dict(verdict=A.UNSUPPORTED, log="")
            r.update({f: 0 for f in ZERO_FIELDS})
            return r


def run(w, cfg, seed, time_limit=0):
    return SignalSim(w, cfg, seed).run(time_limit)


def stats(sim):
    return dict(killed_by_signal=sim.killed_by_signal, caught=sim.caught, lost_signals=sim.lost_signals,
                lost_messages=sim.lost_messages, unsupported=sim.unsupported)


# ---- the oracle yardstick: a ctrl-c to a node without a handler is kill_id ------------------------------------------------------------
def uses_handlers(w):
    return any(w.insns[i].op in (CTRL_C, RECV_OR_CTRL_C) for i in range(w.struct.n_insns))


def rewrite_kill_as_send_ctrl_c(w):
    """Every MS_OP_KILL as MS_OP_SEND_CTRL_C: equal to the original exactly when no task installs a handler (rule 4)."""
    if uses_handlers(w):
        raise ValueError("a workload with ctrl_c handlers")
    return S._rewrite(w, lambda ins: A.Insn(SEND_CTRL_C if ins.op == KILL else ins.op, ins.a, ins.b, ins.imm))


def rewrite_send_ctrl_c_as_kill(w):
    """The reverse: what the unchanged oracle can run."""
    if uses_handlers(w):
        raise ValueError("a workload with ctrl_c handlers")
    return S._rewrite(w, lambda ins: A.Insn(KILL if ins.op == SEND_CTRL_C else ins.op, ins.a, ins.b, ins.imm))
