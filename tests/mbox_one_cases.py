"""The cases of tests/test_emu_mbox_one.py and tests/test_gpu_mbox_one.py (test infrastructure): the base-op kernels' short forms for a mailbox
of one registration and no message queue (k_state.h mbox_one; k_net.h mailbox_deliver_one, k_poll.h MS_OP_RECV).

Every workload runs on the nine base-op layouts of tests/cold_param_cases.py at three mailbox settings: the one the short side is for, and the two
nearest that keep the general side — one registration more, one queued message allowed.  The setting is a launch parameter, so all three select
the same build (each case asserts which).  All 48 bytes of every result are compared with the oracle (tests/parity.py); the oracle has no mailbox
capacities, so what it answers is computed once per workload and shared by the layouts and settings."""
import functools

from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import cold_param_cases as CC
from tests import parity
from tests import pass_invariant_cases as PC

LAYOUTS = CC.LAYOUTS
SHORT = (1, A.LIMIT_NONE)                                  # (mbox_regs, mbox_msgs): the short side
SETTINGS = {"one": SHORT, "two_regs": (2, A.LIMIT_NONE), "one_msg": (1, 1)}
SEED0 = PC.SEED0
SEEDS = PC.SEEDS                                           # 192: three full waves
SEEDS_TIE = PC.SEEDS_TIE                                   # 200: a partial last wave
FIRST = 64                                                 # the first device contact: one wave


def limits(layout, tasks, setting):
    lim = CC.limits(layout, tasks)
    lim.mbox_regs, lim.mbox_msgs = SETTINGS[setting] if isinstance(setting, str) else setting
    return lim


def two_receivers():
    """Two tasks of one node receive on ONE socket at the same time (tags 1 and 2): the second registration needs a list of two.  The sender's two
    datagrams leave a second after both registered and arrive in either order."""
    wl = W.WorkloadBuilder()
    na, nb = wl.create_node(), wl.create_node()
    a, b = wl.addr(na, 1), wl.addr(nb, 1)
    t1 = wl.task(na)
    t1.bind(a)
    t1.recv_from(a, 1)
    t1.assert_val(W.PING)
    t1.sleep(secs=1)                                       # (the socket's owner outlives the other receive)
    t1.done()
    t2 = wl.task(na)
    t2.sleep(ms=10)                                        # bound and registered by then
    t2.recv_from(a, 2)
    t2.assert_val(W.PONG)
    t2.done()
    s = wl.task(nb)
    s.bind(b)
    s.sleep(secs=1)
    s.send_to(b, a, 1, W.PING)
    s.send_to(b, a, 2, W.PONG)
    s.done()
    m = wl.main()
    for t in (t1, t2, s):
        m.spawn(t)
    for t in (t1, t2, s):
        m.join(t)
    m.done()
    return wl.build()


def early_sender():
    """A datagram that arrives a second before its receiver asks for it: nobody is registered, so it needs a queue of one."""
    wl = W.WorkloadBuilder()
    na, nb = wl.create_node(), wl.create_node()
    a, b = wl.addr(na, 1), wl.addr(nb, 1)
    r = wl.task(na)
    r.bind(a)
    r.sleep(secs=2)
    r.recv_from(a, 1)
    r.assert_val(W.PING)
    r.done()
    s = wl.task(nb)
    s.bind(b)
    s.sleep(secs=1)
    s.send_to(b, a, 1, W.PING)
    s.done()
    m = wl.main()
    for t in (r, s):
        m.spawn(t)
    for t in (r, s):
        m.join(t)
    m.done()
    return wl.build()


# name -> (workload, tasks beside the main one, the settings under which EVERY seed's first pass is a capacity verdict, those under which none is)
RUNNER = {
    "two_receivers": (two_receivers, 3, (SHORT, (1, 1)), ((2, A.LIMIT_NONE), (2, 1))),
    "early_sender": (early_sender, 2, (SHORT, (2, A.LIMIT_NONE)), ((1, 1), (2, 1))),
}


@functools.lru_cache(maxsize=None)
def _workload(name, arg):
    return {"pingpong": lambda: W.pingpong(arg, PC.ROUNDS), "ties": PC.tie_workload,
            "two_receivers": two_receivers, "early_sender": early_sender}[name]()


@functools.lru_cache(maxsize=None)
def _expected(name, arg, loss, no_log, count):
    """The oracle's answer, derived as tests/parity.py derives it — once per workload, loss rate and log switch: it models no mailbox capacity and
    no layout, so the nine layouts and three settings share it.  Read-only."""
    lim = A.Limits()
    lim.no_trace_hash = no_log
    want = parity.expected(_workload(name, arg), SEED0, count, PC.config(loss), lim)
    want.setflags(write=False)
    return want


def case(name, arg=0, loss=0.0, layout="compact", count=SEEDS):
    """-> (workload, config, expected results) of one case on `layout`."""
    return _workload(name, arg), PC.config(loss), _expected(name, arg, loss, int(layout.endswith("nolog")), count)


def compare(run, resolve, w, cfg, lim, want, count, what):
    """tests/parity.py's comparison with the shared expectation: the first pass, capacity verdicts re-run with grown limits, then all 48 bytes."""
    got = run(w, SEED0, count, cfg, lim)
    final = parity.compare(got, want, lambda: resolve(got), what=what, ceiling=lambda i: parity.beyond_ceiling(w, SEED0 + i, cfg, lim))
    assert not (final["verdict"] == A.INTERNAL).any(), what
    return got, final
