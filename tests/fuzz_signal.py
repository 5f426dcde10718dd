"""Random programs with ctrl-c signals (MS_OP_CTRL_C, MS_OP_SEND_CTRL_C, MS_OP_RECV_OR_CTRL_C): test infrastructure, compared
against tests/signal_sim.py.

Server nodes run a select loop over ctrl_c() and recv_from (either arm order) as the node's init task, so a restart brings a fresh
incarnation without a handler.  Some nodes carry a SECOND potential waiter, a task that sleeps a random while and then awaits a plain
ctrl_c(): once both are parked a send would schedule two tasks, the model's edge (MADSIM_UNSUPPORTED) — rare by construction, since the
second waiter exists on few nodes and parks late.  One node may install no handler at all: a ctrl-c kills it.  Peers send datagrams
at random intervals; the supervisor sends ctrl-cs to random nodes (its own included), and pauses, resumes, kills and restarts nodes in
between.  No timer-tier op appears: validate() refuses the mix.
"""
import random

from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests.fuzz_scope import hazard

T = 9
SECOND_WAITER_P = 0.12


def random_signal_workload(rng: random.Random, general_addr=False, hazards=False):
    """-> (workload, config, description).  `general_addr`: the nodes that are signalled bind 0.0.0.0:port and the peers name them by
    the node's IP (Network::try_send's `.or_else(0.0.0.0:port)` lookup, network.rs:296-313), as tests/fuzz.py random_addr_workload
    does: the workload then needs the build with general address resolution.  `hazards`: fuzz_scope.hazard at the end of every peer.  Both off, the
    programs are the ones this generator always made."""
    wl = W.WorkloadBuilder()
    m = wl.main()
    servers, extra = [], []
    for i in range(rng.randint(1, 3)):
        n = wl.create_node()
        dst = wl.addr(n, 1 + i)                                # what the peers name
        a = wl.addr(n, 1 + i, ip="unspecified") if general_addr else dst      # what the node binds
        s = wl.task(n, init=True, pre=True)
        s.bind(a)
        top = s.label()
        s.recv_or_ctrl_c(a, T, recv_first=rng.random() < 0.5)
        s.trace_val()
        caught = s.label() + 3
        s.jeq(A.VAL_TIMEOUT, caught)
        s.reply(a, T, 0x70 + i)
        s.jmp(top)
        s.flag_add(i, 1)
        if rng.random() < 0.3:
            s.sleep(us=rng.choice([200, 1500, 6000]))         # (unsubscribed meanwhile: signals are lost)
        if rng.random() < 0.25:
            s.ctrl_c(); s.trace_instant()                      # a plain await in the same task
        s.jmp(top)
        servers.append((n, dst))
        if rng.random() < SECOND_WAITER_P:
            x = wl.task(n)
            x.sleep_rand(lo_ms=0, ms=rng.choice([10, 40, 90]))
            x.ctrl_c(); x.trace_instant(); x.flag_add(3, 1); x.done()
            extra.append(x)
    bare = None
    if rng.random() < 0.5:                                     # a node whose tasks never call ctrl_c(): the signal kills it
        nb = wl.create_node()
        db = wl.addr(nb, 7)
        ab = wl.addr(nb, 7, ip="unspecified") if general_addr else db
        b = wl.task(nb, init=True, pre=True)
        b.bind(ab)
        top = b.label()
        b.recv_from(ab, T); b.reply(ab, T, 0x7E); b.jmp(top)
        bare = (nb, db)
    peers = []
    targets = servers + ([bare] if bare else [])
    for i in range(rng.randint(1, 2)):
        npr = wl.create_node()
        ap = wl.addr(npr, 50 + i)
        p = wl.task(npr)
        p.bind(ap)
        p.set(0, rng.randint(3, 10))
        top = p.label()
        p.sleep_rand(lo_ms=0, us=rng.choice([500, 3000, 12000]))
        p.send_to(ap, rng.choice(targets)[1], T, 0x60 + i)
        if rng.random() < 0.5:
            p.recv_from_timeout(ap, T, ms=rng.choice([2, 8])); p.trace_val()
        p.djnz(0, top)
        if hazards:
            hazard(rng, p, ap)
        p.done()
        peers.append(p)
    for x in extra:
        m.spawn(x)
    for p in peers:
        m.spawn(p)
    nodes = [n for n, _ in targets]
    for _ in range(rng.randint(2, 7)):
        m.sleep(us=rng.randint(1, 9000))
        r, n = rng.random(), rng.choice(nodes)
        if r < 0.6:
            m.send_ctrl_c(n)
        elif r < 0.7:
            m.pause(n); m.sleep(us=rng.randint(100, 5000))
            if rng.random() < 0.7:
                m.send_ctrl_c(n)                                # to a paused node: the woken runnable is parked
            m.sleep(us=rng.randint(100, 5000)); m.resume(n)
        elif r < 0.8:
            m.kill(n)
            if rng.random() < 0.5:
                m.sleep(us=rng.randint(1, 3000)); m.send_ctrl_c(n)      # to a killed node
        elif r < 0.92:
            m.restart(n)                                        # a new incarnation: no handler until its select starts
            if rng.random() < 0.5:
                m.send_ctrl_c(n)                                # ... at once: the init task has not run yet, the node dies again
        else:
            m.send_ctrl_c(0)                                    # the main node itself: no handler, kill_id(0)
    for p in peers:
        m.join(p)
    m.done()
    w = wl.build()
    cfg = A.Config.default(packet_loss_rate=rng.choice([0.0, 0.0, 0.1]))
    return w, cfg, f"{len(servers)}s/{len(extra)}x/{len(peers)}p/{w.struct.n_insns}i" + ("/any" if general_addr else "")


def signal_limits(state_mem=0):
    lim = A.Limits()
    lim.max_tasks = 40
    lim.mbox_regs, lim.mbox_msgs = 16, 16
    lim.heap_lds_slots, lim.heap_spill_slots = 16, 240
    lim.state_mem = state_mem
    return lim
