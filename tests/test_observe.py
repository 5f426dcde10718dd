"""Observation logs — what the listed seeds traced (madsim_hip_trace_seeds, runtime.trace_seeds / observe_seed / fold_observations) — on the
CPU: the fold that turns a list back into an obs_hash, held against the oracle's own lists; the workloads and fuzz blocks that
tests/test_observe_gpu.py replays on the device, with the proof that they are not vacuous and that none of their seeds crosses a ceiling
of the workload model (so every one of them is compared there, with no exemption); and the surface of the four new entry points.

The blocks are fixed lists of program indices of the suite's generators, chosen here, by the oracle alone: programs of which no seed meets
a model event in the oracle's pure run, and among those enough that trace something."""
import functools
import importlib
import inspect
import random

import pytest

import oracle
from madsim_amd import _abi as A
from madsim_amd import runtime
from madsim_amd import workload as W
from tests import cheader as H
from tests import fuzz
from tests import groups_ref as G
from tests import lifecycle_workloads as LW
from tests import tier_blocks as TB

N_PROGRAMS, N_SEEDS, SEED_MUL = 40, 16, 1000


def pinned(lim, k=None):
    """`lim` with the step cap held where it is (tests/parity.py pin_step_cap): the oracle models the cap — MADSIM_STEP_LIMIT at the same
    step — so such a seed is compared like any other and no resolve round may move the cap.  Every sixteenth program of a block runs
    under a time limit of 1 ms and every sixteenth under one of 20 ms (Builder.time_limit): lists cut short where the limit struck — the
    timer-tier generators' programs all trace before anything of theirs can fail, so this is where their blocks get the empty list."""
    lim.max_steps_ceiling = 1
    if k is not None and k % 16 == 7:
        lim.time_limit_ns = 1_000_000
    if k is not None and k % 16 == 15:
        lim.time_limit_ns = 20_000_000
    return lim


# ---- the fuzz blocks -------------------------------------------------------------------------------------------------------------------
# name -> (generator base, the 40 program indices).  Program k is gen(Random(base + k)), its seeds k * SEED_MUL .. + N_SEEDS.
BLOCKS = {
    "base": (61_000, tuple(range(40))),
    "lifecycle": (62_000, tuple(range(40))),
    "scope": (TB.FAMILIES["scope"].base, tuple(range(40))),
    "interval": (TB.FAMILIES["interval"].base, tuple(range(40))),
    "select": (TB.FAMILIES["select"].base, tuple(range(40))),
    # (programs 2, 19, 24, 27 and 33 of this generator hold a send that would wake two ctrl-c waiters: outside the workload model)
    "signal": (TB.FAMILIES["signal"].base, tuple(k for k in range(45) if k not in (2, 19, 24, 27, 33))),
}


def block_program(name, k):
    """-> (workload, config, limits, description) of program k of block `name`."""
    base = BLOCKS[name][0]
    if name == "base":
        w, cfg, desc = fuzz.random_workload(random.Random(base + k))
        return w, cfg, pinned(fuzz.generous_limits(), k), f"random_workload(Random({base + k})) {desc}"
    if name == "lifecycle":
        w, cfg, desc = fuzz.random_lifecycle_workload(random.Random(base + k))
        lim = fuzz.generous_limits(); lim.max_tasks = 40
        return w, cfg, pinned(lim, k), f"random_lifecycle_workload(Random({base + k})) {desc}"
    fam = TB.FAMILIES[name]
    w, cfg, desc = fam.program(base, k)
    return w, cfg, pinned(TB.limits_of(fam, k), k), f"{fam.gen.__name__}(Random({base + k}), **{fam.gen_kw_of(k)}) {desc}"


def block_seeds(k):
    return [k * SEED_MUL + s for s in range(N_SEEDS)]


@functools.lru_cache(maxsize=None)
def block_truth(name):
    """[(k, workload, config, limits, description, seeds, [(observations, Result)] per seed)] of block `name`, by the oracle; computed once
    and shared, read-only, by the tests of both files."""
    out = []
    for k in BLOCKS[name][1]:
        w, cfg, lim, desc = block_program(name, k)
        seeds = block_seeds(k)
        out.append((k, w, cfg, lim, desc, seeds, [oracle.observe_seed(w, s, cfg, lim) for s in seeds]))
    return out


# ---- the directed workloads ------------------------------------------------------------------------------------------------------------
def lossy_pingpong():
    """The lossy two-pair ping-pong of examples/failure_modes_test.cpp with trace(pair) (tests/groups_ref.py), lossy enough that eight
    seeds hold passes and deadlocks."""
    return G.traced_pingpong_workload(), A.Config.default(packet_loss_rate=0.02), A.Limits()


def fixed_pingpong():
    """The timeout-and-resend body of examples/fix_check_test.cpp — the client wraps its recv in a timeout and sends the ping again, the
    server answers every ping and leaves after five seconds of silence — with the trace(pair) of the lossy body, and its capacities."""
    wl = W.WorkloadBuilder()
    tasks = []
    for pair in range(2):
        n1, n2 = wl.create_node(), wl.create_node()
        a1, a2 = wl.addr(n1, 1), wl.addr(n2, 1)
        t1, t2 = wl.task(n1), wl.task(n2)
        t1.bind(a1).sleep(secs=1).set(0, 16)
        t2.bind(a2)
        top1 = t1.label()
        t1.send_to(a1, a2, 1, W.PING).recv_from_timeout(a1, 1, ms=100).jeq(A.VAL_TIMEOUT, top1).assert_val(W.PONG).djnz(0, top1).trace(pair).done()
        top2 = t2.label()
        t2.recv_from_timeout(a2, 1, secs=5).jeq(A.VAL_TIMEOUT, top2 + 5).assert_val(W.PING).reply(a2, 1, W.PONG).jmp(top2).done()
        tasks += [t1, t2]
    m = wl.main()
    for t in tasks:
        m.spawn(t)
    for t in tasks:
        m.join(t)
    m.done()
    lim = A.Limits()
    lim.heap_spill_slots, lim.mbox_regs, lim.mbox_msgs = 128, 8, 4
    return wl.build(), lim


def directed():
    """name -> (workload, config, limits): trace(pair); trace_time a = 0 and a = 1; traced ticks; the select; the ctrl-c select."""
    interval, select, signal = (importlib.import_module(m).DIRECTED for m in ("tests.test_interval", "tests.test_select", "tests.test_signal"))
    return {
        "lossy_pingpong": lossy_pingpong(),
        "std_system_time": (LW.ALL["std_system_time"](), LW.config("std_system_time"), LW.limits("std_system_time")),
        "raft_ticker": (interval["raft_ticker"][0], interval["raft_ticker"][1], W.raft_ticker_limits()),
        "lease_keeper": (W.lease_keeper(), A.Config.default(), W.lease_keeper_limits()),
        "lossy_select": (select["lost"][0], select["lost"][1], W.lossy_select_limits()),
        "graceful_shutdown": (signal["graceful_shutdown"][0], signal["graceful_shutdown"][1], W.graceful_shutdown_limits()),
    }


DIRECTED_SEEDS = range(8)


# ---- the fold ------------------------------------------------------------------------------------------------------------------------
def test_fold_of_nothing_is_the_offset_basis_and_the_twin_agrees():
    assert runtime.fold_observations([]) == 0xCBF29CE484222325 == G.FNV_BASIS
    assert runtime.fold_observations([1]) == ((0xCBF29CE484222325 ^ 1) * 0x100000001B3) % (1 << 64)
    assert runtime.fold_observations([(1 << 64) - 1, 0]) == runtime.fold_observations(iter([(1 << 64) - 1, 0]))
    import importlib.util
    spec = importlib.util.spec_from_file_location("twin_workloads", H.ROOT + "/tools/ref_twin/twin_workloads.py")
    twin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(twin)
    for vals in ([], [0], [1, 2, 3], [(1 << 64) - 1, 1 << 63, 12345678901234567]):
        assert twin.fold_obs(vals) == runtime.fold_observations(vals), vals


def test_fold_of_the_oracles_list_is_obs_hash_on_the_directed_workloads():
    seen = set()
    for name, (w, cfg, lim) in sorted(directed().items()):
        for seed in DIRECTED_SEEDS:
            vals, res = oracle.observe_seed(w, seed, cfg, lim)
            assert res.verdict < A.OVERFLOW, (name, seed, res.verdict)
            assert runtime.fold_observations(vals) == res.obs_hash, (name, seed, vals)
            seen.add((name, len(vals) > 0))
        assert (name, True) in seen, (name, "traces nothing")


@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_block_is_inside_the_model_folds_and_is_not_vacuous(name):
    """No seed of the block meets a ceiling of the workload model in the oracle's PURE run (event mask 0: what the device must answer is
    the reference's result, tests/parity.py expected()); every list folds to its obs_hash; and the block is worth replaying: three or
    more different list lengths, an empty list, a list of eight or more values, passes and panics or deadlocks."""
    assert len(BLOCKS[name][1]) == N_PROGRAMS == len(set(BLOCKS[name][1]))
    lengths, verdicts = set(), set()
    for k, w, cfg, lim, desc, seeds, truth in block_truth(name):
        pure, ev = oracle.run_batch_pure(w, seeds[0], N_SEEDS, cfg, lim)
        assert not ev.any(), (desc, [oracle.ME_NAMES[b] for b in oracle.ME_NAMES if int(ev.max()) & b])
        for i, (vals, res) in enumerate(truth):
            assert res.astuple() == tuple(int(x) for x in pure[i]), (desc, seeds[i])
            assert runtime.fold_observations(vals) == res.obs_hash, (desc, seeds[i], vals)
            lengths.add(len(vals)); verdicts.add(res.verdict)
    print(name, "list lengths", sorted(lengths), "verdicts", sorted(verdicts))
    assert len(lengths) >= 3 and 0 in lengths and max(lengths) >= 8, (name, sorted(lengths))
    assert A.PASS in verdicts and verdicts & {A.PANIC, A.DEADLOCK}, (name, sorted(verdicts))
    assert not verdicts & {A.OVERFLOW, A.UNSUPPORTED, A.INTERNAL}, (name, sorted(verdicts))


def test_the_caps_seed_and_the_campaign_range_are_what_the_gpu_file_assumes():
    w, cfg, lim = directed()[CAPS_WORKLOAD]
    lens = [(len(oracle.observe_seed(w, s, cfg, lim)[0]), len(oracle.trace_seed(w, s, cfg, lim)[0])) for s in CAPS_SEEDS]
    assert lens[1][0] >= 4 and lens[1][1] >= 4, lens
    assert lens[0][0] > lens[1][0] + 1 and lens[2][0] < lens[1][0] - 1, lens        # one neighbour's list is cut by every cap walked, the other's by none but the small ones
    w, cfg, want = G.traced_pingpong()
    modes = {(int(v), int(h)) for v, h in zip(want["verdict"][:CAMPAIGN_TOTAL], want["obs_hash"][:CAMPAIGN_TOTAL]) if v != A.PASS}
    assert len(modes) >= 3, modes                                   # pair 0 stuck, pair 1 stuck, both stuck


CAPS_WORKLOAD, CAPS_SEEDS = "raft_ticker", (1, 0, 6)        # the middle one is the seed whose caps are walked
CAMPAIGN_TOTAL = 4096


# ---- the surface -------------------------------------------------------------------------------------------------------------------------
NEW = ("madsim_hip_trace_seeds", "madsim_hip_ctx_trace_seeds", "madsim_hip_observe_seed", "madsim_hip_ctx_observe_seed")


def test_the_header_declares_the_four_functions_and_the_mirror_has_their_prototypes():
    import ctypes as C
    protos = H.functions()
    L = runtime.lib()
    for fn in NEW:
        assert fn in protos, fn
        f = getattr(L, fn)
        ret, params = protos[fn]
        assert len(f.argtypes) == len(params), (fn, len(f.argtypes), params)
        assert {"int": C.c_int, "int64_t": C.c_int64}[ret] is f.restype, (fn, ret, f.restype)
    assert A.TRACE_MAX_BYTES == int(H.defines()["MADSIM_TRACE_MAX_BYTES"].rstrip("u")) == 1 << 30
    assert A.ABI_VERSION == 7                                       # additive: the version stays
    for fn, params in ((runtime.trace_seeds, ("workload", "seeds", "config", "limits", "obs_cap", "log_cap", "resolve")),
                       (runtime.Context.trace_seeds, ("self", "workload", "seeds", "config", "limits", "obs_cap", "log_cap", "resolve"))):
        p = inspect.signature(fn).parameters
        assert tuple(p) == params and (p["obs_cap"].default, p["log_cap"].default, p["resolve"].default) == (256, 0, True)
    for fn in (runtime.run_campaign, runtime.run_campaign_groups, runtime.run_campaign_diff_resolved, runtime.Context.run_campaign,
               runtime.Context.run_campaign_groups, runtime.Context.run_campaign_diff):
        assert inspect.signature(fn).parameters["observe"].default == 0, fn.__name__
    assert runtime.SeedTrace.__slots__ == ("seed", "result", "observations", "n_observations", "log", "log_len")


def test_argument_errors_need_no_device():
    """n == 0 returns 0 and touches nothing (no context either); the argument checks come before the context is looked at."""
    import ctypes as C
    L = runtime.lib()
    w, cfg, lim = W.pingpong(2, 2), A.Config.default(), A.Limits()
    seeds, buf, words = (C.c_uint64 * 2)(1, 2), (C.c_uint8 * 16)(), (C.c_uint64 * 16)()
    call = lambda *a: L.madsim_hip_ctx_trace_seeds(None, w.ref(), C.byref(cfg), *a)            # noqa: E731
    assert call(None, 0, C.byref(lim), None, 0, None, 0, None, None, None) == 0
    assert call(seeds, 0, C.byref(lim), buf, 8, words, 8, None, None, None) == 0
    E_ARG = -1
    E_LIMITS = int(H.defines()["MADSIM_E_LIMITS"])
    assert int(H.defines()["MADSIM_E_ARG"]) == E_ARG != E_LIMITS < 0
    assert call(None, 2, C.byref(lim), None, 0, None, 0, None, None, None) == E_ARG
    assert call(seeds, 2, C.byref(lim), buf, 0, None, 0, None, None, None) == E_ARG          # a buffer without a cap
    assert call(seeds, 2, C.byref(lim), None, 8, None, 0, None, None, None) == E_ARG         # a cap without a buffer
    assert call(seeds, 2, C.byref(lim), None, 0, words, 0, None, None, None) == E_ARG
    assert call(seeds, 2, C.byref(lim), None, 0, None, 8, None, None, None) == E_ARG
    too_much = call(seeds, 2, C.byref(lim), buf, 1 << 29, None, 0, None, None, None)             # 2 x (2^29 + 72) bytes > 1 GiB: refused, never split
    assert too_much == E_LIMITS
    assert b"MADSIM_TRACE_MAX_BYTES" in L.madsim_hip_last_error()
    assert call(seeds, 2, C.byref(lim), None, 0, words, 1 << 27, None, None, None) == too_much
