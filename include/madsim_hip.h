/*
 * madsim_hip.h — C ABI of the MI355X many-seed runner for madsim's deterministic
 * discrete-event executor (Executor + TimeRuntime + GlobalRng + NetSim delivery queue).
 *
 * This is the drop-in boundary.  The reference has no FFI for its executor; the
 * seam this library plugs into is the per-seed fan-out of
 *     madsim::runtime::Builder::run            madsim/src/sim/runtime/builder.rs:121-162
 * (reached from #[madsim::test] / #[madsim::main], madsim-macros/src/lib.rs:134-151) and, per seed,
 *     Runtime::with_seed_and_config + block_on madsim/src/sim/runtime/mod.rs:53-69,127-130
 *     Executor::block_on / run_all_ready       madsim/src/sim/task/mod.rs:220-323
 * One call to madsim_hip_run_batch replaces `count` iterations of that fan-out: seeds
 * seed0 .. seed0+count-1, one GPU lane per seed.  INTEGRATION.md shows the Rust `extern "C"` stub.
 *
 * A GPU lane cannot poll an opaque Rust future (task/mod.rs:279-283), so the test body is handed
 * over as a *workload*: a table-driven actor program whose instructions are one-to-one with the
 * reference API calls a madsim test makes (Endpoint::bind/send_to/recv_from, time::sleep,
 * spawn/JoinHandle, Handle::kill/restart/pause/resume, NetSim::clog_*).  The executor semantics
 * underneath — ready-queue draw, 50..100 ns poll cost, timer heap order, 1 ms sleep floor, link
 * test and latency draw, mailbox tag matching, async-task wake rules — are restated bit-exactly.
 *
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.
 */
#ifndef MADSIM_HIP_H
#define MADSIM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MADSIM_HIP_ABI_VERSION 7u

/* ------------------------------------------------------------------------------------------------
 * Workload: the actor program (read-only, caller-owned POD).
 * ---------------------------------------------------------------------------------------------- */

/* One instruction = 8 bytes.  Durations are encoded as  b seconds + imm nanoseconds. */
typedef struct madsim_insn {
    uint8_t  op;   /* enum madsim_op */
    uint8_t  a;
    uint16_t b;
    uint32_t imm;
} madsim_insn_t;

/* Each op stands for one reference API call; "await" ops may return Pending to the executor. */
enum madsim_op {
    /* -- task / control -- */
    MS_OP_DONE = 0,        /* async block returns: locals drop (endpoints close, net/mod.rs:483-493),
                              JoinHandle awaiter is woken (async-task)                  */
    MS_OP_SPAWN = 1,       /* a=prog: NodeHandle::spawn / task::spawn  (task/mod.rs:607-654);
                              handle[prog] := new task.  b&2: `async move` takes the spawner's (tx, rx) */
    MS_OP_JOIN = 2,        /* a=prog: handle[prog].await (task/join.rs:59-72). b&1: expect Err
                              (unwrap_err) else unwrap -> a mismatch panics the polling task         */
    MS_OP_ABORT = 3,       /* a=prog: handle[prog].abort() (task/join.rs:158-163)                    */
    MS_OP_YIELD = 4,       /* tokio::task::yield_now().await (re-export task/mod.rs:30)              */
    MS_OP_PANIC = 5,       /* a=0: panic!() with message code imm (0..254); a=1: panic!("{}", flag[b & 3] + imm): the message is
                              the decimal text of that value, which is also its code — values above
                              madsim_workload_t.panic_dyn_max yield MADSIM_UNSUPPORTED.  The code is what
                              NodeBuilder::restart_on_panic_matching looks at (task/mod.rs:297-300; madsim_workload_t.panic_match);
                              any other panic (failed assert, unwrap of an Err) carries code 255, which no pattern names */
    MS_OP_SET = 6,         /* a=reg(0..1): cnt[a] = imm (a loop bound; registers are 16 bit)          */
    MS_OP_DJNZ = 7,        /* a=reg, b=target: if (--cnt[a] != 0) goto b                              */
    MS_OP_JMP = 8,         /* b=target                                                               */
    MS_OP_TRACE = 9,       /* obs_hash <- fold(imm + (b&1 ? cnt[a] : 0)): an observable side effect
                              (the std::sync::mpsc send in task/mod.rs:1029)                         */
    MS_OP_BUILD = 15,      /* a=node: create_node().init(..).build() inside a task body: spawns the node's
                              MADSIM_PROG_INIT program(s) now (task/mod.rs:472-474)                  */
    /* -- time -- */
    MS_OP_SLEEP = 10,      /* time::sleep(b s + imm ns).await  (time/sleep.rs:5-8, mod.rs:111-124)   */
    MS_OP_MARK = 11,       /* t0 = Instant::now().  A program's SLEEP_UNTIL / ASSERT_ELAPSED must have a MARK at a lower pc: t0
                              is a local of the task body, and a use before its assignment is refused (MADSIM_E_WORKLOAD) as Rust would */
    MS_OP_SLEEP_UNTIL = 12,/* time::sleep_until(t0 + b s + imm ns).await (time/mod.rs:118-124)       */
    MS_OP_ASSERT_ELAPSED = 13, /* a=cmp (0 ==, 1 >=, 2 <): assert!(t0.elapsed() cmp b s + imm ns)    */
    MS_OP_ADVANCE = 14,    /* time::advance(b s + imm ns) (time/mod.rs:195-198, 103-106)             */
    /* -- net (datagram Endpoint API, net/endpoint.rs) -- */
    MS_OP_BIND = 20,       /* a=sock: Endpoint::bind(addr(sock)).await.unwrap() (endpoint.rs:23-36, network.rs:206-251).
                              b&1: without the unwrap — val := 0, MADSIM_VAL_ADDR_NOT_AVAILABLE or MADSIM_VAL_ADDR_IN_USE;
                              b&2: on success val := ep.local_addr().unwrap().port() (what a port-0 entry was given)        */
    MS_OP_SEND = 21,       /* a=src sock, b=(tag<<8)|dst addr, imm=payload:
                              ep.send_to(addr(dst), tag, payload).await (endpoint.rs:69-72,120-133)  */
    MS_OP_REPLY = 22,      /* a=src sock, b=(tag<<8), imm=payload: ep.send_to(from, tag, ..).await   */
    MS_OP_RECV = 23,       /* a=sock, b=(tag<<8): (val, from) = ep.recv_from(tag).await
                              (endpoint.rs:87-94,140-149)                                            */
    MS_OP_ASSERT_VAL = 24, /* assert_eq!(val, imm)                                                   */
    MS_OP_RECV_TIMEOUT = 25,/* a=sock, b=(tag<<8)|secs, imm=ns: timeout(secs s + ns, ep.recv_from(tag)).await;
                              on Err(Elapsed) val := MADSIM_VAL_TIMEOUT (time/mod.rs:128-140)         */
    MS_OP_CLOSE = 26,      /* a=sock: drop(ep) (BindGuard::drop, net/mod.rs:483-493)                 */
    /* -- supervisor: fault injection (runtime/mod.rs:276-303, net/mod.rs:164-222) -- */
    MS_OP_KILL = 30,       /* a=node: Handle::kill(node)     (task/mod.rs:356-371)                   */
    MS_OP_RESTART = 31,    /* a=node: Handle::restart(node)  (task/mod.rs:374-401)                   */
    MS_OP_PAUSE = 32,      /* a=node: Handle::pause(node)    (task/mod.rs:404-410)                   */
    MS_OP_RESUME = 33,     /* a=node: Handle::resume(node)   (task/mod.rs:413-424)                   */
    MS_OP_CLOG_NODE = 34,  /* a=node, b=dir(1 in,2 out,3 both): NetSim::clog_node{,_in,_out}         */
    MS_OP_UNCLOG_NODE = 35,/* a=node, b=dir                                                          */
    MS_OP_CLOG_LINK = 36,  /* a=src node, b=dst node: NetSim::clog_link (network.rs:184-189)         */
    MS_OP_UNCLOG_LINK = 37,/* a=src node, b=dst node                                                 */
    MS_OP_ASSERT_EXIT = 38,/* a=node, b=expected: assert_eq!(Handle::is_exit(node), b)               */
    MS_OP_SET_LOSS = 39,   /* a=index into madsim_config_t.loss_table: NetSim::update_config(|c|
                              c.packet_loss_rate = ..) (net/mod.rs:138-141)                          */
    MS_OP_SLEEP_RAND = 40, /* sleep(thread_rng().gen_range(a*50 ms .. b s + imm ns)).await: the randomised
                              fault loop of tonic-example/tests/test.rs:198-201 (UniformDuration, A.3) */
    /* -- shared test flags: the Arc<AtomicUsize> the reference's tests observe (task/mod.rs:864-1015) -- */
    MS_OP_GSET = 41,       /* a=flag(0..3): flag.store(imm)                                         */
    MS_OP_GADD = 42,       /* a=flag: flag.fetch_add(imm)                                            */
    MS_OP_ASSERT_G = 43,   /* a=flag: assert_eq!(flag.load(), imm)                                   */
    MS_OP_PANIC_IF_G_LT = 44, /* a=flag: if flag.load() < imm { panic!() }                            */
    MS_OP_JEQ = 45,        /* b=target: if val == imm { goto b } (react to a timeout / a reply value)    */
    /* -- reliable channel: what madsim-tonic / etcd / kafka sims ride on (net/mod.rs:337-430) -- */
    MS_OP_CONNECT = 46,    /* a=ep, b=dst addr: (tx, rx) = ep.connect1(addr).await; val := 0, or
                              MADSIM_VAL_REFUSED on ConnectionRefused (endpoint.rs:178-193)           */
    MS_OP_ACCEPT = 47,     /* a=ep: (tx, rx, _) = ep.accept1().await (endpoint.rs:197-211)           */
    MS_OP_CSEND = 48,      /* imm=payload: tx.send(payload).await; val := MADSIM_VAL_RESET when the
                              peer's receiver is gone (endpoint.rs:240-245, net/mod.rs:417-421)      */
    MS_OP_CRECV = 49,      /* val = rx.recv().await: in-order delivery, 1 ms -> 10 s backoff while the link
                              is down (net/mod.rs:385-402); MADSIM_VAL_RESET when the channel closed */
    MS_OP_CCLOSE = 50,     /* drop(tx); drop(rx)                                                     */
    /* -- typed RPC over the datagram Endpoint (net/rpc.rs:96-180) -- */
    MS_OP_RPC_CALL = 51,   /* a=ep, b=(req_tag<<8)|dst addr, imm=(timeout_ms<<8)|request code:
                              val = ep.call(dst, req).await (rpc.rs:108-131): rsp_tag = random::<u64>() (one
                              RngCore draw), send_to_raw(dst, R::ID, (rsp_tag, req)), recv_from_raw(rsp_tag),
                              assert_eq!(from, dst).  timeout_ms != 0: ep.call_timeout(dst, req, d) (rpc.rs:96-105),
                              val := MADSIM_VAL_TIMEOUT on Err(TimedOut).  req_tag must be a typed tag (>= 0x80).   */
    MS_OP_RPC_REPLY = 52,  /* a=ep, imm=response code: net.send_to_raw(from, rsp_tag, rsp) of the request this
                              task received (or inherited at spawn): the tail of add_rpc_handler (rpc.rs:170-176) */
    MS_OP_RAND_BOOL = 53,  /* a=index into madsim_config_t.loss_table: val = thread_rng().gen_bool(p) as u32 — one
                              RngCore draw unless p == 1 (madsim-etcd-client/src/service.rs:165-166)        */
    MS_OP_RANDOM = 54,     /* a=0: val = thread_rng().gen::<u32>() (rand.rs:142-158, one with());
                              a=1: val = the byte of getrandom(&mut [0u8; 1]) (rand.rs:197-211: with(|r| r.fill_bytes(buf))) */
    MS_OP_TRACE_TIME = 55, /* a=0: obs_hash <- fold(SystemTime::now() in ns since UNIX_EPOCH): the per-seed base time
                              (time/mod.rs:26-33) + elapsed; a=1: fold(Instant elapsed ns) (system_time.rs:122-154);
                              a=2: fold(val): make the last received / drawn value observable                      */
    /* -- NetSim message hooks (net/mod.rs:240-284; consulted by NetSim::send, :307-311 and :323-328) -- */
    MS_OP_HOOK_REQ = 56,   /* a=node, b=(req_tag<<8)|mode, imm=request code: NetSim::hook_rpc_req::<R>(node, f) — replaces the
                              node's request hook.  f returns false (the request is dropped after rand_delay, BEFORE the link
                              test: no loss / latency draws, no delivery timer) for typed-RPC requests of tag req_tag sent FROM
                              `node` whose code == imm (mode 0) or for all of them (mode 1); every other payload passes.    */
    MS_OP_HOOK_RSP = 57,   /* a=node, b=mode, imm=response code: NetSim::hook_rpc_rsp::<R>(node, f) — replaces the node's response
                              hook.  The hook installed when a typed-RPC response is SENT towards `node` judges it when its
                              delivery timer fires: false (code == imm in mode 0, any response in mode 1) = the timer fires and
                              nothing is delivered.  Responses carry no type id here: the hook sees every response.           */
    /* -- IP Virtual Server at run time (net/ipvs.rs:50-85): the calls a test makes on NetSim::global_ipvs() -- */
    MS_OP_IPVS = 58,       /* a=MADSIM_IPVS_*, b=service (index into madsim_workload_t.services), imm=socket-table entry of a
                              server address (ADD_SERVER / DEL_SERVER).  ADD_SERVICE = HashMap::insert of a fresh Service (no
                              servers, rr_index 0: also when the service exists); DEL_SERVICE removes it; ADD_SERVER pushes
                              (`.expect("service not found")`: the calling task panics when the service is absent);
                              DEL_SERVER = servers.retain(|a| a != server_addr), rr_index untouched — get_server resets an
                              index that ran off the end (ipvs.rs:96-98).  No draw, no await.                              */
    /* -- ABI v4 -- */
    MS_OP_SET_LATENCY = 59,/* a=index into madsim_config_t.lat_table: NetSim::update_config(|c| c.send_latency = lo..hi)
                              (net/mod.rs:138-141 -> Network::update_config, net/network.rs:129): every later link test samples
                              the new range (network.rs:267) — datagram sends, connect1, channel sends and their retries alike;
                              messages already in flight keep the latency they drew.  No draw, no await.                    */
    /* -- ABI v5: timeout scopes, time::timeout(d, async { .. several awaits .. }) (time/mod.rs:128-140) -- */
    MS_OP_TIMEOUT_BEGIN = 60,/* a=secs, imm=ns (< 10^9), b=pc of the matching MS_OP_TIMEOUT_END: the timeout's Sleep is created now
                              (deadline max(now + d, now + 1 ms), no draw, no timer); the ops up to END are the inner future.  Each
                              poll that leaves the inner future Pending polls the Sleep (ANOTHER timer while not elapsed,
                              time/sleep.rs:47-54); once elapsed the inner future is dropped at whatever await it is parked on
                              and val := MADSIM_VAL_TIMEOUT, execution goes on at END + 1 in the same poll.  Rules (validate(),
                              MADSIM_E_WORKLOAD otherwise): scopes do not nest, a pair lies in one program, no jump enters a scope
                              and none leaves it except to its END; inside only sleep / sleep_until / sleep_rand / yield, send /
                              reply / recv / untimed rpc_call, connect / csend / crecv, the light ops, trace_time, the flag ops,
                              panic, random, rand_bool, tick / interval_reset (v6); csend / crecv need a connect at a lower pc of the same scope.          */
    MS_OP_TIMEOUT_END = 61,/* closes the scope (completion: val is what the block left).  A connection a MS_OP_CONNECT of the scope
                              made is a local of the async block: dropped here, and on expiry (tx, then rx)                   */
    /* -- ABI v6: interval tickers, `let mut i = time::interval(p); loop { i.tick().await; .. }` (time/interval.rs) -------------- */
    MS_OP_INTERVAL = 62,   /* a bits 0-1 = MissedTickBehavior (0 Burst, 1 Delay, 2 Skip), a bit 2 = interval_at(t0, p) (t0 = the
                              program's MARK, which must stand at a lower pc) instead of interval(p) = interval_at(now, p); b = whole
                              seconds of the period, imm = the nanoseconds below one second (< 10^9); period > 0.  Makes the task's
                              ticker: its Sleep is sleep_until(start), deadline max(start, now + 1 ms) (time/mod.rs:118-124).  Again:
                              the ticker is replaced (Rust reassignment).  Never awaits.  Not inside a timeout scope.          */
    MS_OP_TICK = 63,       /* ticker.tick().await.  Deadline passed (now >= deadline): Ready at once, NO timer and no yield; else a
                              timer at the deadline on every poll that leaves it Pending (time/sleep.rs:47-54).  On completion the
                              next deadline is deadline + period, unless the tick is late (now > deadline + 5 ms): then Burst
                              deadline + period, Delay now + period, Skip now + period - (now - deadline) % period.  a & 1: obs_hash
                              <- fold(the tick's scheduled instant, ns since the runtime's start, as MS_OP_TRACE_TIME a=1); val is
                              unchanged.  Every path from the program's entry must pass an MS_OP_INTERVAL first.  Allowed inside a
                              timeout scope: its expiry drops the tick future only, the ticker keeps its deadline.            */
    MS_OP_INTERVAL_RESET = 64,/* ticker.reset(): next deadline := now + period (no floor, no behaviour).  Never awaits.  Needs a ticker,
                              as MS_OP_TICK does.                                                                             */
    /* -- ABI v7: select_biased! over a receive and a time arm (time/mod.rs:128-156, futures' select_biased!) --------------------- */
    MS_OP_RECV_OR_TICK = 65,/* a=sock, b=(tag<<8)|flags: select! { biased; (msg, from) = ep.recv_from(tag) => .., _ = ticker.tick() => .. },
                              the two arms in the order flags bit 0 gives (0 recv first, 1 tick first); every poll polls both in
                              that order, the first Ready wins and the other is dropped.  The recv arm is MS_OP_RECV_TIMEOUT's:
                              nothing before its first poll, then Mailbox::recv (take a queued message or register), then
                              rand_delay (one draw, 1 ms floor: Pending at first).  Dropped after it took its message, the
                              message is lost (its draw and its timer stay); dropped while registered, the registration is
                              dead.  The tick arm is MS_OP_TICK's: deadline passed -> Ready in that poll, no timer; else a
                              timer at the deadline on every poll that leaves it Pending; dropped, the ticker keeps its
                              deadline and its timers stay.  Tick first with the deadline passed: the tick wins at the first
                              poll, no registration, no draw, no yield.  Recv wins: val / from as MS_OP_RECV_TIMEOUT sets them.
                              Tick wins: val := MADSIM_VAL_TIMEOUT, the ticker advances as MS_OP_TICK's does, flags bit 1 folds
                              the tick's scheduled instant (MS_OP_TICK a=1).  Every path from the program's entry must pass an
                              MS_OP_INTERVAL first.  Not inside a timeout scope.  (tokio's unbiased select! starts at a branch
                              its thread-local FastRand picks: not restated)                                               */
    MS_OP_RECV_TIMEOUT_AT = 66,/* a=sock, b=(tag<<8)|secs, imm=ns (< 10^9): timeout_at(t0 + d, ep.recv_from(tag)).await, t0 = the
                              program's MARK (which must stand at a lower pc); the deadline max(t0 + d, now + 1 ms) is fixed when
                              the op starts (time/mod.rs:144-156, the sleep_until floor).  Otherwise MS_OP_RECV_TIMEOUT: a message
                              does not move the deadline.  Not inside a timeout scope.                                      */
    /* -- ctrl-c signals (signal.rs:4-8, task/mod.rs:166-175,426-441; additive: new opcode values only, the ABI stays v7) -------------- */
    MS_OP_CTRL_C = 67,     /* signal::ctrl_c().await.unwrap().  Its first poll marks the task's NodeInfo "handler installed" (for the rest
                              of that incarnation: a restart makes a NodeInfo without it, a kill alone leaves it) and subscribes: it
                              sees only signals sent after that poll, so it is always Pending there.  No timer, no draw; it is woken
                              by another task's MS_OP_SEND_CTRL_C and completes on that poll.  val is unchanged.                  */
    MS_OP_SEND_CTRL_C = 68,/* a=node: Handle::current().send_ctrl_c(node).  No handler installed on the node's current NodeInfo: exactly
                              MS_OP_KILL (kill_id).  Installed: every task of that NodeInfo parked in a ctrl_c(), or in a select whose
                              ctrl-c arm is pending, is woken (a task that is scheduled already is not queued again; on a paused node the
                              runnable is parked); nothing else happens — a signal nobody waits for is lost.  Never awaits.  A send
                              that would schedule two or more tasks is MADSIM_UNSUPPORTED for that seed: the order in which tokio's
                              watch::Sender wakes several waiters is picked by a thread-local generator the seed does not control.  */
    MS_OP_RECV_OR_CTRL_C = 69,/* a=sock, b=(tag<<8)|flags: select! { biased; _ = ctrl_c() => .., (msg, from) = ep.recv_from(tag) => .. },
                              flags bit 0: the recv arm is polled first.  Every poll polls both arms in that order.  The ctrl-c arm is
                              MS_OP_CTRL_C's (installs and subscribes at the select's first poll, never Ready there); the recv arm is
                              MS_OP_RECV_TIMEOUT's, dropped under MS_OP_RECV_OR_TICK's rules.  Ctrl-c wins: val := MADSIM_VAL_TIMEOUT, a
                              message the recv arm took is lost (its draw and its timer stay), a registration goes dead.  Recv wins: val /
                              from as MS_OP_RECV_TIMEOUT sets them and the subscription is dropped — the next select subscribes afresh, so
                              a signal sent between two selects, or to a recv-first select whose message is ready, is lost.
                              None of the three ops may share a workload with a timer-tier op (MS_OP_TIMEOUT_BEGIN / END, INTERVAL, TICK,
                              INTERVAL_RESET, RECV_OR_TICK, RECV_TIMEOUT_AT): no kernel build carries both (MADSIM_E_WORKLOAD).            */
    MS_OP__COUNT
};
#define MADSIM_IPVS_ADD_SERVICE 0u
#define MADSIM_IPVS_DEL_SERVICE 1u
#define MADSIM_IPVS_ADD_SERVER  2u
#define MADSIM_IPVS_DEL_SERVER  3u

/* Typed RPC (net/rpc.rs): request tags R::ID are the tag values 0x80..0xFD; a message received on one carries the
 * caller's response tag besides its 8-bit request code (val), and MS_OP_SPAWN with MADSIM_SPAWN_MOVE_REQUEST hands
 * (val, from, response tag) to the per-request task like `spawn(async move { .. })` in rpc.rs:170.  Response tags
 * are u64 draws in the reference; here a response is matched to the caller's pending receive itself, which is
 * what an unguessable tag means.  Request and response codes are 8 bits in this build. */
#define MADSIM_TAG_RPC_FIRST 0x80u
#define MADSIM_TAG_RPC_LAST  0xFDu
#define MADSIM_SPAWN_MOVE_CONN    2u   /* MS_OP_SPAWN b: the (tx, rx) pair moves into the child               */
#define MADSIM_SPAWN_MOVE_REQUEST 4u   /* MS_OP_SPAWN b: the received request moves into the child             */

#define MADSIM_VAL_TIMEOUT 0xFFFFFFFFu
#define MADSIM_VAL_REFUSED 0xFFFFFFFEu
#define MADSIM_VAL_RESET   0xFFFFFFFDu
#define MADSIM_VAL_ADDR_NOT_AVAILABLE 0xFFFFFFFCu
#define MADSIM_VAL_ADDR_IN_USE        0xFFFFFFFBu

/* A task program: where it runs and where it starts.  Program 0 is the body handed to block_on
 * (the main task on node 0, task/mod.rs:222-235). */
typedef struct madsim_prog {
    uint8_t  node;   /* 0 = supervisor node "madsim-main"; 1..n_nodes = create_node() order          */
    uint8_t  flags;  /* MADSIM_PROG_* */
    uint16_t entry;  /* first instruction                                                            */
} madsim_prog_t;
#define MADSIM_PROG_INIT 1u /* NodeBuilder::init task: spawned at build() (MS_OP_BUILD, or before
                               block_on when MADSIM_PROG_PRE is also set) and on every restart
                               (runtime/mod.rs:405-418, task/mod.rs:395-400,472-474)                 */
#define MADSIM_PROG_PRE  2u /* spawned before Runtime::block_on pushes the main task, in prog order:
                               `node.spawn(..)` ahead of `runtime.block_on(..)` (task/mod.rs:859-897) */
#define MADSIM_PROG_DROP_SPAWN 4u /* the body owns a guard moved into it whose Drop calls task::spawn(program p + 1)
                               (the reference tests spawn_in_future_drop_by_aborting_task / _by_killing_node,
                               task/mod.rs:1185-1253): whenever an instance finishes — returns, or its future is
                               dropped because it was aborted, its node killed or it panicked — after its other locals
                               have dropped and before its JoinHandle awaiter is notified.  The child is spawned in the
                               dying task's context (run_all_ready enters it for `drop` as for `run`, :284-287): same
                               node, same NodeInfo incarnation, so a guard dropped by a kill spawns a task that is
                               scheduled once and dropped unpolled.  Program p + 1 must run on the same node; not
                               combined with MS_OP_PAUSE (a parked Runnable is dropped in the KILLER's context).    */

/* A socket address an Endpoint may bind or a datagram may be sent to: an IP and a port.  `kind` picks the IP: the node's
 * own 10.0.0.<node>, 0.0.0.0 or 127.0.0.1 as used ON `node` (entries of the last two kinds are per node: only tasks of
 * `node` may bind them).  Resolution happens at try_send time exactly as
 * in network.rs:272-313: loopback or an exact match among the sender's own sockets keeps the message on the sender's
 * node; an IP-less sender or an unknown IP drops it WITHOUT any RNG draw; after the link test (loss + latency draws,
 * msg_count) the destination node's sockets are searched for the exact address, then for 0.0.0.0:port.  The address a
 * receiver sees (`from`, what MS_OP_REPLY answers to) is the sender's real IP — or 127.0.0.1 when the datagram was sent
 * to a loopback address — with the sending socket's port (network.rs:307-311).
 * port == 0 is an EPHEMERAL Endpoint (`Endpoint::bind("0.0.0.0:0")`): every MS_OP_BIND of the entry takes the lowest port
 * from 1 up that no socket of the node holds for that IP (network.rs:224-236) and every other op on the entry works on the
 * Endpoint its last bind made.  Such an entry is not an address anybody can name: it cannot be a destination operand
 * (MS_OP_SEND / MS_OP_CONNECT / MS_OP_RPC_CALL `b`) — peers reach it by replying to `from`, or through a named entry that
 * happens to carry the port it was given.
 * The device table holds one candidate entry per port such an Endpoint can get — as many as the node has entries for that
 * IP — and the total, candidates included, is limited to 63 entries; a workload that keeps more Endpoints of one entry
 * alive than that gets the resource-overflow verdict. */
typedef struct madsim_sock {
    uint8_t  node;
    uint8_t  kind;   /* MADSIM_ADDR_* */
    uint16_t port;
} madsim_sock_t;
#define MADSIM_ADDR_IP          0u  /* 10.0.0.<node>:port */
#define MADSIM_ADDR_UNSPECIFIED 1u  /* 0.0.0.0:port       */
#define MADSIM_ADDR_LOOPBACK    2u  /* 127.0.0.1:port     */
#define MADSIM_ADDR_VIRTUAL     3u  /* a virtual IP that belongs to no node ("1.1.1.1:80"): `node` is an id of the IP (1..255), not a
                                       node.  Only a destination: a workload that binds it is refused (MADSIM_E_WORKLOAD), and a
                                       datagram sent to it is dropped without any draw ("destination not found", :285-289) unless an
                                       IPVS service rewrites the destination first (madsim_service_t)                                */

/* IP Virtual Server (net/ipvs.rs): `NetSim::global_ipvs().add_service(ServiceAddr::Tcp(vaddr), RoundRobin)` plus one
 * `add_server` per entry of `servers`, done before the first task runs (as the reference's own test does,
 * net/tcp/mod.rs:254-315).  NetSim::send and connect1 ask `ipvs.get_server(dst)` after rand_delay and the request hook and
 * before Network::try_send (net/mod.rs:312-317, :345-350): when `dst` equals a service's virtual address and the service has
 * servers, the destination becomes servers[rr_index] and the per-seed rr_index advances (ipvs.rs:88-105) — also when the
 * message is then lost, clogged or finds no socket.  Everything downstream sees the rewritten address: the link test, the
 * socket lookup, the `dst` a connection's channel() halves are built from.  (An RPC caller still asserts `from == dst` with
 * the address it was GIVEN, rpc.rs:126: a typed call through a virtual address panics when the real server answers, as in
 * the reference.)  The table gives every service's address and its state before the first task runs; MS_OP_IPVS changes
 * that state at run time (add_service / del_service / add_server / del_server, ipvs.rs:50-85), per seed, at most 6 servers
 * per service at any time (a seventh add_server yields MADSIM_UNSUPPORTED: no limit grows that word). */
typedef struct madsim_service {
    uint8_t vaddr;       /* socket-table entry holding the service address (any kind; typically MADSIM_ADDR_VIRTUAL) */
    uint8_t n_servers;   /* 0..6 real servers, in add_server order; 0 = get_server() returns None: no rewrite.
                            | MADSIM_SERVICE_ABSENT: only the address is declared — the service does not exist until a task
                            runs MS_OP_IPVS ADD_SERVICE on it (n_servers & 7 must be 0 then)                          */
    uint8_t servers[6];  /* socket-table entries of the real server addresses                                       */
} madsim_service_t;
#define MADSIM_MAX_SERVICES 8u
#define MADSIM_SERVICE_ABSENT 0x80u

typedef struct madsim_node {
    uint8_t flags;       /* MADSIM_NODE_* */
    uint8_t n_match;     /* MADSIM_NODE_RESTART_MATCHING: number of patterns (0..2)                  */
    uint8_t match[2];    /* the panic message codes that restart the node                            */
} madsim_node_t;
#define MADSIM_NODE_RESTART_ON_PANIC 1u /* NodeBuilder::restart_on_panic (task/mod.rs:298-316)      */
#define MADSIM_NODE_RESTART_MATCHING 4u /* NodeBuilder::restart_on_panic_matching(msg) (runtime/mod.rs:384-387,
                                           task/mod.rs:299): restart when the panic's message code is one of
                                           `match[0..n_match)` — or, with madsim_workload_t.panic_match, when the node's
                                           256-bit row has the code's bit set (the host evaluates `contains(pattern)` per code:
                                           substring patterns against literal AND run-time formatted messages)            */
#define MADSIM_PANIC_CODE_OTHER 255u
#define MADSIM_NODE_NO_IP 2u /* create_node() without .ip(..): binds any address, cannot send to another node's IP
                                (network.rs:281-283: "ip not set", no RNG draw)                              */

typedef struct madsim_workload {
    uint32_t n_nodes;   /* nodes 1..n_nodes besides node 0                                           */
    uint32_t n_progs;   /* prog 0 = main                                                             */
    uint32_t n_socks;
    uint32_t n_insns;
    const madsim_node_t* nodes;  /* [n_nodes+1], index = node id                                     */
    const madsim_prog_t* progs;  /* [n_progs]                                                        */
    const madsim_sock_t* socks;  /* [n_socks]                                                        */
    const madsim_insn_t* insns;  /* [n_insns]                                                        */
    /* -- ABI v3 -- */
    uint32_t n_services;         /* IPVS virtual services (<= MADSIM_MAX_SERVICES); their use selects the general-address build */
    uint32_t panic_dyn_max;      /* largest message code a run-time formatted panic (MS_OP_PANIC a=1) may produce; 0 = 254.
                                    A workload that also uses literal messages gives those the codes above it; a formatted value
                                    beyond it yields MADSIM_UNSUPPORTED for the seed (never a silently different answer)       */
    const madsim_service_t* services;   /* [n_services] or NULL                                                       */
    const uint32_t* panic_match; /* NULL, or [n_nodes+1][8]: bit c of row n = "a panic whose message code is c restarts node n"
                                    (NodeBuilder::restart_on_panic_matching, `error_msg.contains(pattern)` task/mod.rs:297-300,
                                    evaluated by the host for every code: literal messages are interned as codes, a formatted
                                    message is the decimal text of its code).  Rows of nodes without MADSIM_NODE_RESTART_MATCHING
                                    are ignored.  NULL: the rows are built from madsim_node_t.match[] (equality on the code).   */
} madsim_workload_t;

/* ------------------------------------------------------------------------------------------------
 * Inputs mirroring Builder's public fields (runtime/builder.rs:7-22) and net Config
 * (net/network.rs:66-89).
 * ---------------------------------------------------------------------------------------------- */
typedef struct madsim_config {
    double   packet_loss_rate;   /* Config.net.packet_loss_rate, default 0.0                         */
    uint64_t lat_lo_ns;          /* Config.net.send_latency.start, default 1 ms                      */
    uint64_t lat_hi_ns;          /* Config.net.send_latency.end (exclusive), default 10 ms           */
    uint32_t buggify;            /* non-zero: buggify enabled for the whole run (rand.rs:113-134)    */
    uint32_t n_loss_table;       /* entries in loss_table used by MS_OP_SET_LOSS                     */
    double   loss_table[4];
    /* -- ABI v4 -- */
    uint32_t n_lat_table;        /* entries in lat_table_* used by MS_OP_SET_LATENCY (<= 4); every entry must be a non-empty range
                                    (`gen_range` of an empty range panics in the reference, network.rs:267), and an op that names
                                    an entry >= n_lat_table is refused (MADSIM_E_WORKLOAD)                                   */
    uint32_t reserved0;          /* 0 */
    uint64_t lat_table_lo_ns[4]; /* send_latency.start of entry i                                    */
    uint64_t lat_table_hi_ns[4]; /* send_latency.end (exclusive) of entry i                          */
} madsim_config_t;

#define MADSIM_LIMIT_NONE 0xffffffffu  /* a capacity of zero (0 itself means "pick a default") */

typedef struct madsim_limits {
    uint64_t time_limit_ns;      /* Builder.time_limit; 0 = None (task/mod.rs:253-258)               */
    uint32_t max_steps;          /* device safety net; 0 = default (1<<24). Not a reference concept. */
    uint32_t heap_lds_slots;     /* timer-heap entries kept in LDS per seed; 0 = auto                */
    uint32_t heap_spill_slots;   /* further entries per seed in the coalesced HBM spill region       */
    uint32_t max_tasks;          /* live task instances per seed; 0 = auto (n_progs + restarts)      */
    uint32_t mbox_regs;          /* pending recv registrations per socket; 0 = auto (2)              */
    uint32_t mbox_msgs;          /* undelivered messages per socket; 0 = auto (2), MADSIM_LIMIT_NONE = none */
    uint32_t lanes_per_wave;     /* seeds carried per 64-lane wave (8/16/32/64); 0 = auto.  With state_mem = MADSIM_STATE_GLOBAL: 64,
                                    or 32 for timeout-only workloads (twice the LDS per seed: more of the timer heap out of the
                                    spill region — the election loop's setting); anything else there is MADSIM_E_LIMITS */
    uint32_t max_conns;          /* live reliable-channel connections per seed; 0 = auto (4)         */
    uint32_t chan_queue;         /* queued payloads per channel direction; 0 = auto (2)              */
    uint32_t sched;              /* MADSIM_SCHED_*: how lanes pick up further seeds when a launch holds more
                                    seeds than resident lanes; 0 = static striding                    */
    uint32_t state_mem;          /* MADSIM_STATE_*: where a seed's task table and planes live; 0 = auto               */
    uint32_t max_steps_ceiling;  /* the largest step cap a re-run of MADSIM_STEP_LIMIT seeds (madsim_hip_run_batch_auto / _multi)
                                    may use; 0 = default (1 << 28: the first pass's 1 << 24, then ONE 16x round).  A seed that
                                    still hits the cap keeps the MADSIM_STEP_LIMIT verdict: a livelocked workload (a yield or
                                    1 ms timer loop without a time limit) costs seconds, not one hour-long kernel              */
    uint32_t no_trace_hash;      /* non-zero: do not fold the determinism log into madsim_result_t.trace_hash (it comes back 0).
                                    The reference computes a log byte per RNG call only while check_determinism logs or checks
                                    (rand.rs:67 `if lock.log.is_some() || lock.check.is_some()`); the per-seed fingerprint of
                                    that log in every result is an extra of this runner — 0 keeps it (default), a plain
                                    Builder::run needs none of it (measured: 4 % faster on the ping-pong kernel; madsim_hip_trace_seed always logs) */
} madsim_limits_t;

#define MADSIM_STATE_AUTO   0u   /* LDS unless an extended-op workload's state leaves a CU fewer than 4 full waves       */
#define MADSIM_STATE_LDS    1u   /* all per-seed state in LDS ([word][lane] planes)                                       */
#define MADSIM_STATE_GLOBAL 2u   /* extended-op workloads: task table + planes in global memory ([unit][lane] across the launch:
                                    L2 / Infinity Cache / HBM), only the timer-heap top and the ready queue in LDS.  A workload
                                    of base ops only has no such build and keeps its state in LDS (the setting is ignored)  */

#define MADSIM_STATE_COMPACT 3u  /* base-op workloads on full waves, <= 8 tasks, no heap spill, sleeps < 2.1 s: 8-byte timer-heap entries (low
                                    deadline word: exact inside that horizon), heap root in registers, the main task in global memory —
                                    a fourth wave per SIMD for the 4-node ping-pong.  AUTO takes it when it gains a workgroup per CU  */

/* OR-ed into madsim_limits_t.state_mem (the low byte keeps MADSIM_STATE_*): global-state builds of timeout-only workloads keep the
   re-registrations of a pending Sleep — time/sleep.rs:51-53 registers ANOTHER timer with the same deadline and waker on every
   not-elapsed poll — as a COUNT beside the first entry instead of as further heap entries (k_timer.h dedup_note).  Identical
   entries fire back to back and every one after the first is a no-op wake-up, so the result is the same bit for bit unless two
   DIFFERENT events tie on a deadline (their order depends on the heap's shape): the kernel notices such a tie when it pops it and
   runs that seed again from the start with the literal heap, so callers never see a difference — only time.  Ignored by the other
   builds.  Worth it where timeouts dominate and ties are rare (the election loop: 34 % of its timer pushes are such duplicates,
   5e-4 of its seeds meet a tie). */
#define MADSIM_STATE_DEDUP_TIMERS 0x100u

/* OR-ed into madsim_limits_t.state_mem like MADSIM_STATE_DEDUP_TIMERS: global-state builds with a heap-spill region keep every timer-heap
   entry as 8 bytes {low 32 bits of the deadline, event word} instead of 16 — twice the heap levels in the same LDS, half the bytes per
   spilled level; the payload of a datagram delivery waits in a per-seed record pool in global memory until its entry reaches the root.
   Exact while every live deadline lies within 2^31 ns (2.1 s) of the clock: the host admits the layout only for workloads whose sleeps,
   timeouts and latencies stay below that (no buggify, no restart_on_panic), and the device checks every push — a seed that does exceed
   it (a channel back-off past 2 s) gets a capacity verdict and is run again on the 16-byte entries by madsim_hip_run_batch_auto.  Results
   never differ.  Ignored by builds without the variant (LDS-resident state, connection-only workloads, general address resolution). */
#define MADSIM_STATE_NARROW_HEAP 0x200u

#define MADSIM_SCHED_STATIC 0u   /* lane g runs seeds g, g+G, g+2G, ...                                */
#define MADSIM_SCHED_QUEUE  1u   /* a finished lane pulls the next seed from a per-launch atomic counter */

/* ------------------------------------------------------------------------------------------------
 * Outputs.
 * ---------------------------------------------------------------------------------------------- */
enum madsim_verdict {
    MADSIM_PASS = 0,        /* block_on returned                                                     */
    MADSIM_PANIC = 1,       /* a task panicked and its node does not restart (task/mod.rs:315)       */
    MADSIM_DEADLOCK = 2,    /* "no events, all tasks will block forever" (task/mod.rs:250)           */
    MADSIM_TIME_LIMIT = 3,  /* "time limit exceeded" (task/mod.rs:253-258)                           */
    MADSIM_OVERFLOW = 4,    /* a device capacity in madsim_limits_t was exceeded: re-run the seed with
                               larger limits (not a reference verdict; never silently wrong).  Capacities a larger limit
                               CAN lift give this verdict (at their ceilings the same events are MADSIM_UNSUPPORTED, below) — with
                               two exceptions that stay capacity verdicts at the ceiling, where a re-run cannot help: the timer
                               heap at 2^20 spilled entries, and the 128th message queued in one mailbox of a workload without
                               extended ops (its header keeps 7 bits).  The FIRST capacity or model event of a seed decides
                               its runner verdict (what follows it in the same round runs on spoiled state)            */
    MADSIM_STEP_LIMIT = 5,  /* max_steps reached (not a reference verdict)                           */
    MADSIM_UNSUPPORTED = 6, /* the seed left the workload MODEL (not a reference verdict, and larger limits do not help:
                               never re-run): a port-0 table entry bound again while the Endpoint of its previous bind is
                               alive — an entry names one Endpoint at a time, `close` it first; a seventh server added to
                               an IPVS service; a ninth connection waiting in one Endpoint's accept1 queue; a 255th live task,
                               a 256th registration of one socket, a 16th queued channel payload, a 128th live connection, a 256th
                               message queued in one mailbox (the ceilings of max_tasks / mbox_regs / chan_queue / max_conns /
                               mbox_msgs: below them the verdict is MADSIM_OVERFLOW and a re-run lifts it); a 128th connection end
                               holding one Endpoint's address; an ephemeral bind when every candidate port the table has for that
                               (node, IP) is taken (addresses kept alive by connections of Endpoints long dropped); a new
                               receive whose registration word — 8 bits of the task's receive count, 8 of its slot's generation —
                               equals a dead registration's still in the list (256 receives of one task while a timed-out one
                               lingers, 256 instances of one slot); a formatted panic value above
                               madsim_workload_t.panic_dyn_max.  The oracle reports the same verdict for the same seed, decided at
                               the same instruction; every other result field is 0                                          */
    MADSIM_INTERNAL = 7     /* an invariant of the device code broke (a bug in this library, never a property of the
                               workload): the parity tests assert that no seed ever carries it; other fields 0        */
};
#define MADSIM_MAX_LIVE_TASKS 254u   /* the ceiling of madsim_limits_t.max_tasks: a 255th live task is MADSIM_UNSUPPORTED (kernel and oracle) */
#define MADSIM_MAX_MBOX_REGS 255u    /* the ceiling of mbox_regs: a 256th pending / dead registration of one socket is MADSIM_UNSUPPORTED          */
#define MADSIM_MAX_CHAN_QUEUE 15u    /* the ceiling of chan_queue: a 16th payload queued in one channel direction is MADSIM_UNSUPPORTED             */
#define MADSIM_MAX_CONNS 127u        /* the ceiling of max_conns: a 128th live connection is MADSIM_UNSUPPORTED                                     */
#define MADSIM_MAX_MBOX_MSGS 255u    /* the ceiling of mbox_msgs (workloads with extended ops; 127 without): a 256th message queued in one mailbox is MADSIM_UNSUPPORTED */
#define MADSIM_MAX_SOCKET_GUARDS 127u /* connection ends (Sender + Receiver pairs) that may hold one Endpoint's BindGuard at a time: the 128th is MADSIM_UNSUPPORTED */
/* verdicts >= MADSIM_OVERFLOW are RUNNER verdicts: statements about this runner, never a test's failure */
#define MADSIM_IS_RUNNER_VERDICT(v) ((v) >= MADSIM_OVERFLOW)

/* 48 bytes per seed.  Everything here is compared bit-for-bit against the oracle. */
typedef struct madsim_result {
    uint32_t verdict;
    uint32_t steps;       /* executor steps: task polls (incl. dropped runnables) + timer fires      */
    uint64_t clock_ns;    /* Clock.elapsed() when block_on left (time/mod.rs:230-233)                */
    uint64_t msg_count;   /* NetSim::stat().msg_count (network.rs:99-105,265)                        */
    uint64_t rng_calls;   /* Xoshiro256PlusPlus::next_u64 invocations on the GlobalRng               */
    uint64_t trace_hash;  /* FNV-1a-64 over the determinism-log bytes of rand.rs:64-88               */
    uint64_t obs_hash;    /* FNV-1a-64 over MS_OP_TRACE values in execution order                    */
} madsim_result_t;

typedef struct madsim_summary {
    uint64_t first_failing_seed; /* minimum seed with verdict != PASS; UINT64_MAX if none — test n_failed, a
                                    batch may legitimately contain seed UINT64_MAX itself            */
    uint64_t n_failed;
    uint64_t total_steps;
    uint64_t total_clock_ns;
    double   kernel_ms;          /* HIP-event time of the simulation kernel(s) on the call's stream   */
    double   wall_s;             /* host wall time of the call                                       */
} madsim_summary_t;

/* ------------------------------------------------------------------------------------------------
 * Entry points.  All return 0 on success, <0 on error (madsim_hip_strerror); they never unwind.
 * Per-seed failures are data (verdict), not errors.
 * ---------------------------------------------------------------------------------------------- */
#define MADSIM_E_ARG      (-1)
#define MADSIM_E_HIP      (-2)
#define MADSIM_E_NOINIT   (-3)
#define MADSIM_E_WORKLOAD (-4)
#define MADSIM_E_LIMITS   (-5)

uint32_t    madsim_hip_version(void);
/* Identity of the loaded library: "madsim_hip abi=<MADSIM_HIP_ABI_VERSION> arch=gfx950 kernels=<builds> ..." — the product is
 * the gfx950 HIP build and nothing else; a host mirror that lets the library path be overridden (A/B builds) checks this
 * string so that no other object exporting the same symbols can stand in for it. */
const char* madsim_hip_build_info(void);
const char* madsim_hip_strerror(int code);
const char* madsim_hip_last_error(void);   /* thread-local text of the calling thread's last failure */
/* The library keeps up to five batches of one call in flight on its own HIP streams; ROCclr maps a process's streams onto
 * GPU_MAX_HW_QUEUES hardware queues (default 4), and streams that share a queue run one after the other (madsim_hip_run_batch(262 144):
 * 8.3 ms against ~5 ms).  The library never touches the environment by itself: set GPU_MAX_HW_QUEUES=16 before the process first uses
 * HIP, or call this FIRST THING in main() (it is a setenv: not safe beside threads that read the environment, no effect once HIP is
 * initialised).  Returns 1 when it set the variable, 0 when the host's own setting stands, <0 on a bad argument. */
int madsim_hip_prefer_hw_queues(int n);

/* ---- Per-device contexts -----------------------------------------------------------------------------
 * "one host thread drives a batch; library is re-entrant per device handle, not thread-safe per
 * handle".  A context owns everything the runner keeps on one GPU (workload tables, spill regions, events);
 * distinct contexts share no mutable state, so a process may hold one per GPU and use them from different threads,
 * or drive all of them from one thread with madsim_hip_run_batch_multi.  Calls on ONE context are serialised.
 * Every madsim_hip_ctx_* function mirrors the v1 function of the same name below, which runs on the
 * process-default context created by madsim_hip_init. */
typedef struct madsim_hip_ctx madsim_hip_ctx_t;
int madsim_hip_ctx_create(int device, madsim_hip_ctx_t** out);
int madsim_hip_ctx_destroy(madsim_hip_ctx_t* ctx);
int madsim_hip_ctx_device(const madsim_hip_ctx_t* ctx);
madsim_hip_ctx_t* madsim_hip_default_ctx(void);   /* NULL before madsim_hip_init */

/* Bind the calling process to one GPU (one process per GPU; replaces nothing in the reference —
 * the reference's per-seed std::thread::spawn, builder.rs:134, has no device). */
int madsim_hip_init(int device);
int madsim_hip_shutdown(void);

/* Replaces the seed loop of Builder::run (builder.rs:129-160) for `count` seeds from `seed0`.
 * `out` is caller-allocated host memory [count] (may be NULL when only the summary is wanted). */
int madsim_hip_run_batch(const madsim_workload_t* w, const madsim_config_t* cfg,
                         uint64_t seed0, uint64_t count, const madsim_limits_t* lim,
                         madsim_result_t* out, madsim_summary_t* summary);

/* madsim_hip_run_batch, then every seed that came back with a RUNNER verdict — MADSIM_OVERFLOW (a device capacity)
 * or MADSIM_STEP_LIMIT (the max_steps safety net) — is run again, all of them gathered into ONE compacted launch per
 * round, with doubled capacities / a 16x step cap (never above madsim_limits_t.max_steps_ceiling), up to `max_rounds` times; the summary is
 * recomputed over the final results.  The reference's containers are unbounded (Vec mailboxes, BinaryHeap timers) and
 * it has no step cap, so neither is ever a test verdict: this is the entry point a Builder::run replacement calls.
 * `out` must not be NULL. */
int madsim_hip_run_batch_auto(const madsim_workload_t* w, const madsim_config_t* cfg,
                              uint64_t seed0, uint64_t count, const madsim_limits_t* lim,
                              madsim_result_t* out, madsim_summary_t* summary, int max_rounds);

/* Same, results stay resident in HBM: `d_out` is device memory [count] owned by the caller,
 * `stream` is a hipStream_t (NULL = the null stream).  Asynchronous unless `summary` != NULL
 * (the summary needs a device reduction + D2H of 32 bytes, which synchronises `stream`). */
int madsim_hip_run_batch_device(const madsim_workload_t* w, const madsim_config_t* cfg,
                                uint64_t seed0, uint64_t count, const madsim_limits_t* lim,
                                void* d_out, void* stream, madsim_summary_t* summary);

/* Fully asynchronous form: nothing is copied to the host.  `d_summary4` (device memory, 4 x uint64_t, may be NULL)
 * receives {first failing seed ^ (1 << 63), n_failed, total_steps, total_clock_ns} from a reduction kernel queued behind
 * the simulation on `stream`.  Word 0 is in order-preserving int64 form (none = INT64_MAX), so a signed RCCL
 * all-reduce(MIN) on it and all-reduce(SUM) on words 1-3 combine ranks without touching the host.  `timing_slot` in [0,64) brackets
 * the simulation kernel with a HIP event pair readable through madsim_hip_timing_ms after the stream has run; -1 = none. */
int madsim_hip_run_batch_async(const madsim_workload_t* w, const madsim_config_t* cfg,
                               uint64_t seed0, uint64_t count, const madsim_limits_t* lim,
                               void* d_out, void* d_summary4, void* stream, int timing_slot);
int madsim_hip_timing_ms(int timing_slot, double* ms);

/* Re-run one seed and return the raw determinism log (rand.rs:64-88 byte per GlobalRng::with),
 * the artefact MADSIM_TEST_CHECK_DETERMINISM compares (runtime/mod.rs:178-202).  Returns the number
 * of bytes the log holds (may exceed cap; only cap bytes are written), <0 on error. */
int64_t madsim_hip_trace_seed(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed,
                              const madsim_limits_t* lim, uint8_t* log, uint64_t cap,
                              madsim_result_t* out);

/* Observation logs: what the listed seeds traced.  madsim_result_t.obs_hash is an FNV-1a fold of the values the test body handed to
 * MS_OP_TRACE, MS_OP_TRACE_TIME and a traced tick (64-bit offset basis 0xcbf29ce484222325, then h = (h ^ value) * 0x100000001b3 per value,
 * the value folded whole); these calls return the values themselves, in execution order — the output a failing #[madsim::test] prints,
 * for the seeds a campaign listed (madsim_failure_t.seed, madsim_group_t.first_seed, madsim_diff_record_t.seed).
 *
 * madsim_hip_trace_seeds replays `n` seeds (any order, duplicates allowed) on the trace build in ONE launch, with one synchronisation of the
 * stream it runs on at the end of the call.  Row i of each output belongs to seeds[i].
 *   logs:  n rows of log_cap bytes (NULL with log_cap 0: none kept): the determinism log, as madsim_hip_trace_seed writes it
 *   obs:   n rows of obs_cap 64-bit words (NULL with obs_cap 0: none kept): the observed values in execution order, what obs_hash folds
 *   log_len / obs_len (either may be NULL): n TRUE lengths, which may exceed the caps; a row holds the first min(len, cap) entries and
 *          zeros behind them
 *   out:   n results (may be NULL), the 48 bytes madsim_hip_run_batch gives for the seed under the same limits (with
 *          madsim_limits_t.no_trace_hash: trace_hash = 0, though the log rows are written all the same)
 * The call runs under the limits it is given and does not re-run: a seed may come back with a runner verdict (MADSIM_IS_RUNNER_VERDICT),
 * and then its lists are what was recorded until that verdict — not meaningful, never to be compared; for a verdict >= MADSIM_UNSUPPORTED
 * every other result field is 0, as everywhere.  Replay such seeds under madsim_hip_grow_limits(w, lim, r), r = 1, 2, ...
 * n == 0 returns 0 and touches nothing.  MADSIM_E_ARG: seeds == NULL with n > 0; a buffer without a cap or a cap without a buffer.
 * MADSIM_E_LIMITS: the call would ask the device for more than MADSIM_TRACE_MAX_BYTES — n * (log_cap + 8 * obs_cap + 72) bytes: the rows,
 * two length words, the seed and the result of every seed.  The library never splits a list behind the caller's back: pass fewer seeds
 * per call, or smaller caps. */
#define MADSIM_TRACE_MAX_BYTES 1073741824u /* 1 GiB of device memory per madsim_hip_trace_seeds call */
int madsim_hip_trace_seeds(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n,
                           const madsim_limits_t* lim, uint8_t* logs, uint64_t log_cap, uint64_t* obs, uint64_t obs_cap,
                           uint64_t* log_len, uint64_t* obs_len, madsim_result_t* out);
/* One seed's observations (the oracle's madsim_oracle_observe_seed, on the device): returns how many values the seed traced (may exceed
 * cap; only the first cap are written, zeros behind a shorter list), <0 on error.  obs may be NULL with cap 0: the count alone. */
int64_t madsim_hip_observe_seed(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed,
                                const madsim_limits_t* lim, uint64_t* obs, uint64_t cap, madsim_result_t* out);

/* Task post-mortems: where the tasks stand when a seed's run ends.  The 48 result bytes say THAT a seed deadlocked, panicked, ran into its
 * time limit or passed; these calls say which tasks were still alive at that moment and what each was doing — the reference's
 * RuntimeMetrics::num_tasks_by_node_by_spawn (runtime/metrics.rs, task/mod.rs:497-541), per instruction instead of per spawn site, with no
 * probe placed in the test body beforehand.  The trace builds keep unit 0 of every live task slot when the result is written: one 64-bit
 * word per task, never 0 (state >= 1):
 *   bits 63-56 state   MADSIM_TASK_PARKED     awaiting, not woken
 *                      MADSIM_TASK_QUEUED     woken and not yet polled: in the ready queue, or held back by a paused node
 *                      MADSIM_TASK_PANICKED   the task whose poll raised the verdict MADSIM_PANIC
 *                      MADSIM_TASK_CANCELLED  aborted, or its node killed, and the executor had not yet dropped the runnable (task/mod.rs:269-273
 *                                             happens at the pop)
 *   bits 55-48 prog    index into madsim_workload_t's program table
 *   bits 47-32 pc      index into the workload's instruction array as the caller wrote it: the instruction whose await has not completed;
 *                      for QUEUED the await that will be polled again, or the program's entry for a task never polled; for PANICKED the
 *                      panicking instruction
 *   bits 31-16 cnt0, bits 15-0 cnt1: the loop registers (MS_OP_SET / MS_OP_DJNZ)
 * Settled from the kernel's code:
 *   pc.     The device runs the caller's instruction array index for index (the fused post-chain words are additions to an instruction, no
 *           instruction moves), and no awaiting op advances pc before its await completes, whatever its stage: a sleep, a rand_delay, a
 *           receive's registration, oneshot and delay, every stage of an rpc call, accept1's delay and queue wait, a channel receive's wait,
 *           backoff and arrival, a join, a yield, a tick, ctrl_c and the selects all leave pc on their own instruction until they are Ready.
 *           A task inside a timeout scope stands at the await inside the block, not at MS_OP_TIMEOUT_BEGIN.  One case is normalised: an
 *           assert_eq!(val, ..) fused into the awaiting op in front of it fails while pc is still that op's; the record names the
 *           MS_OP_ASSERT_VAL, as it does for an assert reached on its own.
 *   panic.  The task whose poll panicked is recorded from the registers of that poll (pc of the panicking instruction, the loop registers
 *           as they stood).  A panic that restart_on_panic absorbs is no verdict and leaves no PANICKED record: the task is gone.
 *   order.  Ascending task slot, the runner's task-table order.  A spawn takes the lowest free slot, so a seed's slots are the same under
 *           every madsim_limits_t whose max_tasks it does not exhaust — and a seed that exhausts it has a runner verdict and no records.
 *           The rows are therefore a function of (workload, configuration, seed) alone and are not sorted.
 *   states. In precedence: PANICKED; CANCELLED (the abort or kill flag is set: every such task has also been woken); QUEUED; PARKED.
 * A seed with a runner verdict (MADSIM_IS_RUNNER_VERDICT) has task_len 0 and an all-zero row: the verdict is the whole answer.
 *
 * madsim_hip_task_states follows madsim_hip_trace_seeds to the letter: ONE launch of the trace build over `n` seeds (any order, duplicates
 * allowed), row i belongs to seeds[i].
 *   tasks:    n rows of task_cap words (NULL with task_cap 0: the counts alone); a row holds the first min(len, task_cap) records and
 *             zeros behind them.  task_cap <= MADSIM_MAX_LIVE_TASKS
 *   task_len: n TRUE counts of live tasks (may be NULL), which may exceed task_cap
 *   out:      n results (may be NULL): the 48 bytes madsim_hip_run_batch gives under the same limits.  No silent re-run
 * n == 0 returns 0 and touches nothing.  MADSIM_E_ARG: seeds == NULL with n > 0; a buffer without a cap or a cap without a buffer;
 * task_cap above MADSIM_MAX_LIVE_TASKS.  MADSIM_E_LIMITS: n * (8 * task_cap + 72) exceeds MADSIM_TRACE_MAX_BYTES; the list is never split. */
#define MADSIM_TASK_PARKED 1
#define MADSIM_TASK_QUEUED 2
#define MADSIM_TASK_PANICKED 3
#define MADSIM_TASK_CANCELLED 4
#define MADSIM_TASK_STATE(w) ((uint32_t)((uint64_t)(w) >> 56))
#define MADSIM_TASK_PROG(w) ((uint32_t)(((uint64_t)(w) >> 48) & 0xffu))
#define MADSIM_TASK_PC(w) ((uint32_t)(((uint64_t)(w) >> 32) & 0xffffu))
#define MADSIM_TASK_CNT0(w) ((uint32_t)(((uint64_t)(w) >> 16) & 0xffffu))
#define MADSIM_TASK_CNT1(w) ((uint32_t)((uint64_t)(w) & 0xffffu))
#define MADSIM_TASK_SITE(w) ((uint64_t)(w) >> 32) /* state | prog | pc: where the task stands, the loop registers dropped */
int madsim_hip_task_states(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n,
                           const madsim_limits_t* lim, uint64_t* tasks, uint64_t task_cap, uint64_t* task_len, madsim_result_t* out);
/* The shape of a task table: the sum over its records of mix(MADSIM_TASK_SITE(record)) mod 2^64, mix the splitmix64 finaliser
 *   z = site; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9; z = (z ^ (z >> 27)) * 0x94d049bb133111eb; mix = z ^ (z >> 31)
 * — commutative, so it names the multiset of sites whatever the order of the records, and two seeds stuck the same way have the same shape
 * whatever their loop registers say.  The empty table's shape is 0.  No device involved. */
uint64_t madsim_hip_stall_shape(const uint64_t* tasks, uint64_t n);

/* Timelines: WHEN the listed seeds traced what they traced.  The observation log holds the values; the trace builds keep beside each value
 * the virtual time of the observation — the runtime's elapsed nanoseconds at that instruction, the number MS_OP_TRACE_TIME a=1
 * (trace_instant) would fold there.  It is the time of the observation, not the value: a traced tick folds the deadline it was scheduled
 * for, which may lie before the clock, and its time entry is the clock.  Within a row the times never decrease.  Stamping every traced
 * value of a test body with a trace_instant behind it leaves the run's result unchanged, so the oracle's observation list of that stamped
 * twin is the reference: its odd entries are this call's time row.
 *
 * madsim_hip_timeline_seeds is madsim_hip_trace_seeds with the time rows beside the observation rows and no determinism log: ONE launch of
 * the trace build over `n` seeds (any order, duplicates allowed), one synchronisation, row i belongs to seeds[i].
 *   obs, times: n rows of obs_cap 64-bit words each (both required, obs_cap > 0): times[i * obs_cap + k] is when obs[i * obs_cap + k] was
 *               traced; both rows hold their first min(len, obs_cap) entries and zeros behind them
 *   obs_len:    n TRUE lengths (may be NULL), the one length of both rows
 *   out:        n results (may be NULL), as madsim_hip_trace_seeds gives them.  No silent re-run: a seed with a runner verdict
 *               (MADSIM_IS_RUNNER_VERDICT) has rows that are not meaningful; replay it under madsim_hip_grow_limits
 * n == 0 returns 0 and touches nothing.  MADSIM_E_ARG: seeds == NULL with n > 0; a missing row array or obs_cap == 0.  MADSIM_E_LIMITS:
 * n * (16 * obs_cap + 72) exceeds MADSIM_TRACE_MAX_BYTES; the list is never split. */
int madsim_hip_timeline_seeds(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n,
                              const madsim_limits_t* lim, uint64_t* obs, uint64_t* times, uint64_t obs_cap, uint64_t* obs_len,
                              madsim_result_t* out);

/* Divergence reports: where two variants of a seed's run first part.  A differential campaign says WHICH seeds a change affected;
 * madsim_hip_diverge_seeds says UP TO WHERE the two runs of each listed seed are the same run, on two rulers: the determinism log (one
 * byte per GlobalRng::with, "channel log") and the observation log (one 64-bit word per traced value, "channel obs").  Side A is
 * (wA, cfgA, limA), side B (wB, cfgB, limB); any of B's pointers may equal A's.  Seeds in any order, duplicates allowed; recs[i] belongs
 * to seeds[i].  One call = side A's trace launch, side B's, one compare kernel over the rows where they lie on the device, one copy of the
 * records and one of the context rows, one synchronisation: no log or observation row travels to the host.
 *
 * Per channel, with L = min(len_a, len_b) and m = min(L, cap), `at` is the length of the common prefix that was established:
 *   MADSIM_DIVERGE_INCOMPARABLE  either side's verdict is a runner verdict (MADSIM_IS_RUNNER_VERDICT): rows not meaningful, not read   at = 0
 *   MADSIM_DIVERGE_DIFFER        there is a smallest i < m with a[i] != b[i]                                                           at = i
 *   MADSIM_DIVERGE_SAME          no such i, L <= cap, len_a == len_b                                                                   at = len
 *   MADSIM_DIVERGE_PREFIX        no such i, L <= cap, len_a != len_b: one run ended where the other went on                            at = L
 *   MADSIM_DIVERGE_BEYOND_CAP    no such i, L > cap: nothing differs in what was kept                                                  at = cap
 * log_a / log_b / obs_a / obs_b: side X's entry at index `at` when at < min(len_x, cap), else 0 (always 0 under SAME and INCOMPARABLE).
 * obs_ctx row i, 3 * win words: the shared observations [obs_at - win, obs_at), right-aligned and zero-filled on the left; then A's
 * [obs_at, obs_at + win) and B's, each cut at min(obs_len_x, obs_cap) and zero-filled; all zeros under INCOMPARABLE.
 * The call does not re-run seeds: replay INCOMPARABLE ones under madsim_hip_grow_limits.  a / b: the 48 bytes madsim_hip_trace_seeds gives
 * (trace_hash = 0 under that side's no_trace_hash).  n == 0 returns 0 and touches nothing.
 * MADSIM_E_ARG: seeds or recs NULL with n > 0; win > MADSIM_DIVERGE_MAX_WIN; obs_ctx given with win == 0, or missing with win > 0; win > 0
 * with obs_cap == 0; a workload or configuration either side's validation refuses ("side A: ..." / "side B: ...").
 * MADSIM_E_LIMITS: n * (2 * (log_cap + 8 * obs_cap + 72) + 184 + 24 * win) exceeds MADSIM_TRACE_MAX_BYTES; never split. */
#define MADSIM_DIVERGE_SAME         0u
#define MADSIM_DIVERGE_DIFFER       1u
#define MADSIM_DIVERGE_PREFIX       2u
#define MADSIM_DIVERGE_BEYOND_CAP   3u
#define MADSIM_DIVERGE_INCOMPARABLE 4u
#define MADSIM_DIVERGE_MAX_WIN      8u
/* (two statements, as madsim_diff_record below: the record holds madsim_result_t by value) */
struct madsim_divergence {
    uint64_t seed;
    uint32_t log_status, obs_status;   /* MADSIM_DIVERGE_*                                                                        */
    uint64_t log_at, obs_at;           /* entries of common prefix established                                                    */
    uint64_t log_len_a, log_len_b, obs_len_a, obs_len_b;      /* the true lengths, which may exceed the caps                     */
    uint64_t obs_a, obs_b;             /* each side's observation at obs_at, or 0                                                 */
    uint8_t  log_a, log_b;             /* each side's log byte at log_at, or 0                                                    */
    uint8_t  pad[6];                   /* 0                                                                                       */
    madsim_result_t a, b;
};                                     /* 184 bytes */
typedef struct madsim_divergence madsim_divergence_t;
int madsim_hip_diverge_seeds(const madsim_workload_t* wA, const madsim_config_t* cfgA, const madsim_limits_t* limA,
                             const madsim_workload_t* wB, const madsim_config_t* cfgB, const madsim_limits_t* limB,
                             const uint64_t* seeds, uint64_t n, uint64_t log_cap, uint64_t obs_cap, uint32_t win,
                             madsim_divergence_t* recs, uint64_t* obs_ctx);

/* Observation census: WHICH traced values the seeds of a range reach, by verdict — "did the interesting thing ever happen?".  The result
 * bytes hold a seed's observations only as a fold (obs_hash); the census runs the seeds on the trace build, as madsim_hip_trace_seeds does
 * (log_cap 0, the caller's obs_cap), and reduces the observation rows where they lie on the device: per chunk the trace launch, a fold
 * kernel, an extract kernel, and the chunk's words and entries (64 bytes per distinct value) coming back — no row travels to the host.
 * madsim_hip_census_range takes [seed0, seed0 + total), madsim_hip_census_seeds a STRICTLY ASCENDING list (the campaign list rule).
 *
 * Everything is exact and all-integer, a function of the per-seed (result, observation list) alone: the same bytes whatever `chunk`, the
 * context and the run.  Of seed s with result r and `len` observations the census sees the first min(len, obs_cap) — what
 * madsim_hip_trace_seeds writes to its row.  A seed is COUNTED when r.verdict < 4 and bit `verdict` of `include` is set, as in
 * madsim_stats_t.include.  A seed with a runner verdict (MADSIM_IS_RUNNER_VERDICT) is never counted — its list is cut where the runner gave
 * up —; such seeds are tallied in n_runner and the runner_cap smallest of them written, ascending, to runner_seeds, to be settled under
 * madsim_hip_grow_limits.  Per distinct value v among the counted seeds' visible observations, values[0 .. n_values) ascending by `value`:
 *   n_seeds[k]    counted seeds of verdict k that observed v at least once (a seed counts once however often it traced v)
 *   n_total       occurrences of v over those seeds
 *   max_per_seed  the most occurrences inside one seed
 *   first_seed    the smallest seed that observed v
 * Every 64-bit value is a legal value: 0, 2^64 - 1 and the FNV offset basis included.
 * n_counted[k] / n_silent[k]: counted seeds of verdict k / those of them without a visible observation; n_truncated: counted seeds with
 * len > obs_cap, whose later values are not in the table; n_observations: the sum of min(len, obs_cap) over the counted seeds, which is
 * the sum of every n_total.
 * More than `cap` distinct values: MADSIM_E_LIMITS, and nothing is reported (every output word 0) — a property of the data alone: no
 * arrival order ever picks which values survive.  The likely cause is a traced time or random value, which is no probe vocabulary: raise
 * `cap` or trace less.
 * The library cuts the seeds into chunks of `chunk` (0 = a default, 65 536 or what fits) itself; a census is a reduction, so the cut is
 * invisible in the result.  One chunk asks the device for chunk * (8 * obs_cap + 72) bytes — the rows, two length words, the seed and the
 * result of every seed — plus 32 * slots + 68 * cap + 128 for the table (slots: the power of two >= 2 * cap, at least 128), the claim list,
 * the entries and the words: MADSIM_E_LIMITS when that exceeds MADSIM_TRACE_MAX_BYTES or chunk * obs_cap >= 2^32 - 1.
 * total == 0 / n == 0 reports the empty census.  MADSIM_E_ARG: cen == NULL; include == 0 or a bit at or above 4; cap == 0 or above
 * MADSIM_CENSUS_MAX_VALUES; values == NULL; obs_cap == 0 or above MADSIM_CENSUS_MAX_OBS_CAP; runner_cap > 0 without runner_seeds; seeds ==
 * NULL with n > 0; a list that is not strictly ascending (sort and deduplicate first). */
#define MADSIM_CENSUS_MAX_VALUES  1048576u /* 2^20 distinct values */
#define MADSIM_CENSUS_MAX_OBS_CAP 1024u    /* observations of a seed the census can see */
typedef struct madsim_census_value {   /* 64 bytes */
    uint64_t value;
    uint64_t n_seeds[4];               /* counted seeds of each verdict that observed it at least once                            */
    uint64_t n_total;                  /* occurrences over those seeds                                                            */
    uint64_t first_seed;               /* the smallest seed that observed it                                                      */
    uint64_t max_per_seed;             /* the most occurrences inside one seed                                                    */
} madsim_census_value_t;
typedef struct madsim_census {
    uint32_t include;                  /* in: bit v set = count the seeds whose verdict is v (bits 0-3 only, as madsim_stats_t.include) */
    uint32_t obs_cap;                  /* in: observations of a seed that are visible, 1 .. MADSIM_CENSUS_MAX_OBS_CAP             */
    madsim_census_value_t* values;     /* in: caller's host array [cap]                                                           */
    uint64_t cap;                      /* in: 1 .. MADSIM_CENSUS_MAX_VALUES                                                       */
    uint64_t* runner_seeds;            /* in: caller's host array [runner_cap]; may be NULL when runner_cap == 0                  */
    uint64_t runner_cap;
    uint64_t n_values;                 /* out: entries written, ascending by value                                                */
    uint64_t n_counted[4];             /* out: counted seeds per verdict                                                          */
    uint64_t n_silent[4];              /* out: ... of them without a visible observation                                          */
    uint64_t n_truncated;              /* out: counted seeds with more than obs_cap observations                                  */
    uint64_t n_observations;           /* out: visible observations of the counted seeds = the sum of n_total                     */
    uint64_t n_runner;                 /* out: seeds with a runner verdict                                                        */
    uint64_t n_runner_listed;          /* out: min(n_runner, runner_cap), the entries of runner_seeds written                     */
} madsim_census_t;
int madsim_hip_census_range(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total, uint64_t chunk,
                            const madsim_limits_t* lim, madsim_census_t* cen);
int madsim_hip_census_seeds(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n, uint64_t chunk,
                            const madsim_limits_t* lim, madsim_census_t* cen);

/* Probe-set census: WHICH COMBINATIONS of traced values the seeds reach, by verdict — the conjunctions ("0x20 and 0x21 both reached") that the
 * census, a table of marginal counts over one value each, cannot answer.  The seeds run on the trace build exactly as for the census
 * (log_cap 0, the caller's obs_cap); per chunk three kernels behind the trace launch reduce the rows where they lie: one 64-bit SET WORD per
 * seed, equal set words folded into a keyed table, one 72-byte entry per distinct set coming back.  No row and no per-seed word travels to
 * the host.  madsim_hip_probe_sets_range takes [seed0, seed0 + total), madsim_hip_probe_sets_seeds a STRICTLY ASCENDING list.
 *
 * Everything is exact and all-integer, a function of each seed's (result, observation list) alone: the same bytes whatever `chunk`, the
 * context and the run, and for a dense list the bytes of the range form.  The caller gives a VOCABULARY vocab[0 .. n_vocab) of distinct
 * 64-bit values, 1 <= n_vocab <= MADSIM_PROBE_SETS_MAX_VOCAB (every value is legal: 0, 2^64 - 1 and the FNV offset basis included), and
 * `include` and `obs_cap` with madsim_census_t's meaning and limits.  A seed is COUNTED exactly as in the census (verdict < 4 and its bit
 * set in `include`).  Of a counted seed with `len` observations the first vis = min(len, obs_cap) are visible; its set word has
 *   bit i (0 <= i < n_vocab)        set when vocab[i] occurs at least once among the visible observations
 *   MADSIM_PROBE_SET_OTHER (62)     set when a visible observation is not in the vocabulary
 *   MADSIM_PROBE_SET_TRUNCATED (63) set when len > obs_cap
 * and bits n_vocab .. 61 zero.  A counted seed without a visible observation has the set word 0, an entry like any other.
 * Per distinct set word, sets[0 .. n_sets) ascending by `set` (unsigned): n_seeds[k], the counted seeds of verdict k with exactly this
 * set, and first_seed[k], the smallest of them (0 when n_seeds[k] == 0).  n_counted[k] is the column sum of n_seeds[k].  Seeds with a
 * runner verdict are never counted; they are tallied in n_runner and listed in runner_seeds exactly as the census does it.
 * More than `cap` distinct sets: MADSIM_E_LIMITS, and nothing is reported (every output word 0) — a property of the data alone, never of
 * an arrival order.
 * The library cuts the seeds into chunks of `chunk` (0 = a default, 65 536 or what fits); the cut is invisible in the result.  One chunk
 * asks the device for chunk * (8 * obs_cap + 80) bytes — the rows, two length words, the seed, the set word and the result of every seed —
 * plus 48 * slots + 76 * cap + 64 for the table (slots: the power of two >= 2 * cap, at least 128), the claim list, the entries and the
 * words: MADSIM_E_LIMITS when that exceeds MADSIM_TRACE_MAX_BYTES or chunk * obs_cap >= 2^32 - 1 — never split silently.
 * total == 0 / n == 0 reports the empty result.  MADSIM_E_ARG: ps == NULL; include == 0 or a bit at or above 4; cap == 0 or above
 * MADSIM_PROBE_SETS_MAX; sets == NULL; obs_cap == 0 or above MADSIM_CENSUS_MAX_OBS_CAP; n_vocab == 0 or above
 * MADSIM_PROBE_SETS_MAX_VOCAB; vocab == NULL; a value that occurs twice in vocab; runner_cap > 0 without runner_seeds; seeds == NULL with
 * n > 0; a list that is not strictly ascending (sort and deduplicate first). */
#define MADSIM_PROBE_SETS_MAX_VOCAB 62u
#define MADSIM_PROBE_SETS_MAX       1048576u /* 2^20 distinct sets */
#define MADSIM_PROBE_SET_OTHER      0x4000000000000000ull /* bit 62: a visible observation outside the vocabulary */
#define MADSIM_PROBE_SET_TRUNCATED  0x8000000000000000ull /* bit 63: more than obs_cap observations               */
typedef struct madsim_probe_set {      /* 72 bytes */
    uint64_t set;
    uint64_t n_seeds[4];               /* counted seeds of each verdict with exactly this set                                     */
    uint64_t first_seed[4];            /* the smallest such seed of each verdict; 0 where n_seeds is 0                            */
} madsim_probe_set_t;
typedef struct madsim_probe_sets {
    uint32_t include;                  /* in: as madsim_census_t.include                                                          */
    uint32_t obs_cap;                  /* in: as madsim_census_t.obs_cap                                                          */
    const uint64_t* vocab;             /* in: caller's host array [n_vocab], distinct values                                      */
    uint64_t n_vocab;                  /* in: 1 .. MADSIM_PROBE_SETS_MAX_VOCAB                                                    */
    madsim_probe_set_t* sets;          /* in: caller's host array [cap]                                                           */
    uint64_t cap;                      /* in: 1 .. MADSIM_PROBE_SETS_MAX                                                          */
    uint64_t* runner_seeds;            /* in: caller's host array [runner_cap]; may be NULL when runner_cap == 0                  */
    uint64_t runner_cap;
    uint64_t n_sets;                   /* out: entries written, ascending by set                                                  */
    uint64_t n_counted[4];             /* out: counted seeds per verdict = the column sums of n_seeds                             */
    uint64_t n_runner;                 /* out: seeds with a runner verdict                                                        */
    uint64_t n_runner_listed;          /* out: min(n_runner, runner_cap), the entries of runner_seeds written                     */
} madsim_probe_sets_t;
int madsim_hip_probe_sets_range(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total, uint64_t chunk,
                                const madsim_limits_t* lim, madsim_probe_sets_t* ps);
int madsim_hip_probe_sets_seeds(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n, uint64_t chunk,
                                const madsim_limits_t* lim, madsim_probe_sets_t* ps);

/* Probe-order census: WHICH TRACED VALUE COMES FIRST, by verdict — the orders ("the timeout fired before the ack", "pair 1 finished before
 * pair 0 had started") that neither the census, a table of marginal counts, nor the probe sets, whose set words are symmetric in what they
 * hold, can answer.  The seeds run on the trace build exactly as for the census (log_cap 0, the caller's obs_cap); per chunk two kernels
 * behind the trace launch reduce the rows where they lie into a dense matrix of cells, one 72-byte entry per non-empty cell coming back.
 * No row and no per-seed word travels to the host.  madsim_hip_probe_order_range takes [seed0, seed0 + total),
 * madsim_hip_probe_order_seeds a STRICTLY ASCENDING list.
 *
 * Everything is exact and all-integer, a function of each seed's (result, observation list) alone: the same bytes whatever `chunk`, the
 * context and the run, and for a dense list the bytes of the range form.  The caller gives a VOCABULARY vocab[0 .. n_vocab) of distinct
 * 64-bit values, 1 <= n_vocab <= MADSIM_PROBE_ORDER_MAX_VOCAB (every value is legal: 0, 2^64 - 1 and the FNV offset basis included), and
 * `include` and `obs_cap` with madsim_census_t's meaning and limits.  A seed is COUNTED exactly as in the census (verdict < 4 and its bit
 * set in `include`).  Of a counted seed with `len` observations the first vis = min(len, obs_cap) are visible; first(i) is the index of
 * the first occurrence of vocab[i] among them, undefined when vocab[i] does not occur there.  A cell is a pair (a, b) of vocabulary
 * INDICES:
 *   the diagonal (a, a):            n_seeds[k] = the counted seeds of verdict k in which first(a) is defined
 *   off the diagonal (a, b), a != b: n_seeds[k] = the counted seeds of verdict k in which first(a) and first(b) are both defined and
 *                                   first(a) < first(b)
 * and first_seed[k] the smallest such seed (0 when n_seeds[k] == 0): the witness to replay.  Only cells with a non-zero count in some
 * verdict become entries, pairs[0 .. n_pairs) ascending by (a, b).  Two values never share an index, so for a != b the cells (a, b) and
 * (b, a) add up to the seeds that reached both, and "a without b" is (a, a) - (a, b) - (b, a).
 * n_counted[k]: the counted seeds of verdict k; n_none[k]: those of them with no vocabulary value visible; n_truncated: counted seeds with
 * len > obs_cap — they are counted on their visible prefix like every other seed: a first occurrence inside a prefix is the true one.
 * Seeds with a runner verdict are never counted; they are tallied in n_runner and listed in runner_seeds exactly as the census does it.
 * `cap`, the room of `pairs`, must be at least n_vocab * n_vocab: there is no "too many" outcome.
 * The library cuts the seeds into chunks of `chunk` (0 = a default, 65 536 or what fits); the cut is invisible in the result.  One chunk
 * asks the device for chunk * (8 * obs_cap + 72) bytes — the rows, two length words, the seed and the result of every seed — plus
 * 32 768 + 76 * n_vocab^2 + 96 for the matrix, the entries and the words: MADSIM_E_LIMITS when that exceeds MADSIM_TRACE_MAX_BYTES or
 * chunk * obs_cap >= 2^32 - 1 — never split silently.
 * total == 0 / n == 0 reports the empty result.  MADSIM_E_ARG: po == NULL; include == 0 or a bit at or above 4; obs_cap == 0 or above
 * MADSIM_CENSUS_MAX_OBS_CAP; n_vocab == 0 or above MADSIM_PROBE_ORDER_MAX_VOCAB; vocab == NULL; a value that occurs twice in vocab;
 * cap < n_vocab * n_vocab; pairs == NULL; runner_cap > 0 without runner_seeds; seeds == NULL with n > 0; a list that is not strictly
 * ascending (sort and deduplicate first). */
#define MADSIM_PROBE_ORDER_MAX_VOCAB 32u
typedef struct madsim_probe_order_pair { /* 72 bytes */
    uint32_t a;                        /* vocabulary index of the value that comes first (or, on the diagonal, of the value reached) */
    uint32_t b;                        /* vocabulary index of the value that comes later; a == b: the diagonal                      */
    uint64_t n_seeds[4];               /* counted seeds of each verdict in this cell                                              */
    uint64_t first_seed[4];            /* the smallest such seed of each verdict; 0 where n_seeds is 0                            */
} madsim_probe_order_pair_t;
typedef struct madsim_probe_order {
    uint32_t include;                  /* in: as madsim_census_t.include                                                          */
    uint32_t obs_cap;                  /* in: as madsim_census_t.obs_cap                                                          */
    const uint64_t* vocab;             /* in: caller's host array [n_vocab], distinct values                                      */
    uint64_t n_vocab;                  /* in: 1 .. MADSIM_PROBE_ORDER_MAX_VOCAB                                                   */
    madsim_probe_order_pair_t* pairs;  /* in: caller's host array [cap]                                                           */
    uint64_t cap;                      /* in: at least n_vocab * n_vocab                                                          */
    uint64_t* runner_seeds;            /* in: caller's host array [runner_cap]; may be NULL when runner_cap == 0                  */
    uint64_t runner_cap;
    uint64_t n_pairs;                  /* out: entries written, ascending by (a, b)                                               */
    uint64_t n_counted[4];             /* out: counted seeds per verdict                                                          */
    uint64_t n_none[4];                /* out: counted seeds per verdict with no vocabulary value visible                         */
    uint64_t n_truncated;              /* out: counted seeds with more than obs_cap observations                                  */
    uint64_t n_runner;                 /* out: seeds with a runner verdict                                                        */
    uint64_t n_runner_listed;          /* out: min(n_runner, runner_cap), the entries of runner_seeds written                     */
} madsim_probe_order_t;
int madsim_hip_probe_order_range(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total, uint64_t chunk,
                                 const madsim_limits_t* lim, madsim_probe_order_t* po);
int madsim_hip_probe_order_seeds(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n, uint64_t chunk,
                                 const madsim_limits_t* lim, madsim_probe_order_t* po);

/* Probe spans: HOW LONG, in virtual time, from one traced value to another — "after the kill, how long until a leader is elected again?",
 * "which seed has the slowest recovery, and which seeds never recover?" — as a distribution over a range of seeds.  The seeds run on the
 * trace build as for the census, with the time log beside the observation log (madsim_hip_timeline_seeds' launch: "Timelines" above); per
 * chunk two kernels behind the trace launch reduce the rows where they lie.  No row and no per-seed word travels to the host.
 * madsim_hip_probe_spans_range takes [seed0, seed0 + total), madsim_hip_probe_spans_seeds a STRICTLY ASCENDING list.
 *
 * The caller gives 1 .. MADSIM_PROBE_SPANS_MAX span definitions {from, to, flags} (every value is legal; from == to is the time between the
 * first two occurrences, a period; equal definitions are allowed and give equal records) and `include` and `obs_cap` with
 * madsim_census_t's meaning and limits.  A seed is COUNTED exactly as in the census.  Per counted seed and span, over the visible
 * observations (the first min(len, obs_cap)):
 *   i = the first index whose value is `from` — or, with MADSIM_SPAN_FROM_START, -1: the start of the run, time 0; `from` is then ignored
 *   j = the first index greater than i whose value is `to`
 *   MADSIM_SPAN_ABSENT  there is no i
 *   MADSIM_SPAN_CLOSED  i and j exist: the duration is time[j] - time[i] (time[-1] = 0), unsigned; the clock never goes back.  A span closed
 *                       inside a cut prefix is the true one
 *   MADSIM_SPAN_OPEN    an i but no j, and len <= obs_cap: the run ended first
 *   MADSIM_SPAN_CUT     an i but no j, and len > obs_cap: unknown, counted apart
 * spans[s], one record per definition, in definition order: n_state[4 * verdict + state] the counted seeds; over the CLOSED seeds of all counted
 * verdicts n, min, max, the exact 128-bit sum of the durations, hist[madsim_hip_stat_bucket(duration)], and min_seed / max_seed, the
 * smallest seed that attains each extreme; first_open_seed, the smallest counted seed that is OPEN: the one to replay.  Where there is no
 * such seed: the seed is UINT64_MAX, min is UINT64_MAX and max 0, as madsim_metric_t has it.  n_counted, n_truncated (counted seeds with
 * len > obs_cap), n_runner, runner_seeds / runner_cap / n_runner_listed: as the probe-order census has them.
 * Everything is exact and all-integer, a function of each seed's (result, observation list, time list) alone: the same bytes whatever
 * `chunk`, the form, the context and the run.  No atomic decides a seed: every witness is a minimum.  There is no "too many".
 * One chunk (0 = a default, 65 536 or what fits) asks the device for chunk * (16 * obs_cap + 72 + 12 * n_spans) + 2240 * n_spans + 64
 * bytes: MADSIM_E_LIMITS when that exceeds MADSIM_TRACE_MAX_BYTES or chunk * obs_cap >= 2^32 - 1 — never split silently.
 * total == 0 / n == 0 reports the empty result.  MADSIM_E_ARG: ps == NULL; include == 0 or a bit at or above 4; obs_cap == 0 or above
 * MADSIM_CENSUS_MAX_OBS_CAP; n_spans == 0 or above MADSIM_PROBE_SPANS_MAX; defs == NULL or spans == NULL; a flag other than
 * MADSIM_SPAN_FROM_START; runner_cap > 0 without runner_seeds; seeds == NULL with n > 0; a list that is not strictly ascending. */
#define MADSIM_PROBE_SPANS_MAX 16u
#define MADSIM_SPAN_FROM_START 1u
#define MADSIM_SPAN_ABSENT 0u
#define MADSIM_SPAN_CLOSED 1u
#define MADSIM_SPAN_OPEN 2u
#define MADSIM_SPAN_CUT 3u
typedef struct madsim_span_def {       /* 24 bytes */
    uint64_t from, to;
    uint32_t flags;                    /* 0 or MADSIM_SPAN_FROM_START */
    uint32_t reserved;                 /* ignored */
} madsim_span_def_t;
typedef struct madsim_span {           /* 2240 bytes */
    uint64_t n_state[16];              /* [4 * verdict + MADSIM_SPAN_*]: counted seeds                                            */
    uint64_t n;                        /* CLOSED seeds over the counted verdicts                                                  */
    uint64_t min, max;                 /* of their durations; UINT64_MAX and 0 when n == 0                                        */
    uint64_t sum_lo, sum_hi;           /* the 128-bit sum of their durations                                                      */
    uint64_t min_seed, max_seed;       /* the smallest seed whose duration is min / max; UINT64_MAX when n == 0                   */
    uint64_t first_open_seed;          /* the smallest counted seed that is OPEN; UINT64_MAX when there is none                   */
    uint64_t hist[256];                /* [MADSIM_STAT_BUCKETS]: CLOSED seeds per bucket of madsim_hip_stat_bucket(duration)      */
} madsim_span_t;
typedef struct madsim_probe_spans {    /* 104 bytes */
    uint32_t include;                  /* in: as madsim_census_t.include                                                          */
    uint32_t obs_cap;                  /* in: as madsim_census_t.obs_cap                                                          */
    const madsim_span_def_t* defs;     /* in: caller's host array [n_spans]                                                       */
    uint64_t n_spans;                  /* in: 1 .. MADSIM_PROBE_SPANS_MAX                                                         */
    madsim_span_t* spans;              /* in: caller's host array [n_spans]; out: one record per definition                       */
    uint64_t* runner_seeds;            /* in: caller's host array [runner_cap]; may be NULL when runner_cap == 0                  */
    uint64_t runner_cap;
    uint64_t n_counted[4];             /* out: counted seeds per verdict                                                          */
    uint64_t n_truncated;              /* out: counted seeds with more than obs_cap observations                                  */
    uint64_t n_runner;                 /* out: seeds with a runner verdict                                                        */
    uint64_t n_runner_listed;          /* out: min(n_runner, runner_cap), the entries of runner_seeds written                     */
} madsim_probe_spans_t;
int madsim_hip_probe_spans_range(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total, uint64_t chunk,
                                 const madsim_limits_t* lim, madsim_probe_spans_t* ps);
int madsim_hip_probe_spans_seeds(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n, uint64_t chunk,
                                 const madsim_limits_t* lim, madsim_probe_spans_t* ps);
/* The record of one definition over the union of two DISJOINT seed sets: `from` merged into `into` — counts, the sum and the histogram add,
 * of two equal extremes the smaller seed wins, first_open_seed is the minimum.  What settles runner seeds under grown limits and merges
 * reports of several ranges; exact, in either order.  No device involved. */
void madsim_hip_span_merge(madsim_span_t* into, const madsim_span_t* from);

/* Stall-site census: WHERE the tasks of a range's seeds stand when their runs end, by verdict — "409 of the 412 deadlocking seeds have a
 * task of program 2 parked in the recv_from at pc 7", with no probe placed in advance.  The seeds run on the trace build with the task log
 * alone (madsim_hip_task_states' launch: log_cap 0, obs_cap 0, the caller's task_cap); per chunk the work runs behind the trace launch on
 * the rows where they lie — no row and no per-seed word travels to the host.  stall_sites_kernel turns every row's visible records, the
 * first min(len, task_cap), into a SITE ROW (each word MADSIM_TASK_SITE(record): state | prog | pc, the loop registers dropped) and one
 * SHAPE word (madsim_hip_stall_shape of the visible records: the multiset of sites, whatever the slot order).  Then the observation
 * census's own kernels, host fold and table run twice, unchanged, on those materialised rows: once over the site rows, once over the shape
 * words as rows of cap 1 and length 1 — so every rule of the census holds as worded there: a seed is COUNTED when r.verdict < 4 and bit
 * `verdict` of `include` is set; runner verdicts are tallied in n_runner and the runner_cap smallest listed in runner_seeds, never counted;
 * the bytes are the same whatever `chunk`, the form (range or list), the context and the run.
 *   sites[0 .. n_sites), ascending by `value` = the site:  n_seeds[k] counted seeds of verdict k with at least one task there; n_total
 *        tasks there over those seeds; max_per_seed the most inside one seed; first_seed the smallest such seed
 *   shapes[0 .. n_shapes), ascending by `value` = the shape word:  n_seeds[k] counted seeds of verdict k with exactly that multiset of
 *        sites; first_seed the one to replay (madsim_hip_task_states, then madsim_hip_stall_shape of its row gives the word back);
 *        n_total = the seeds, max_per_seed = 1.  shapes == NULL with shape_cap 0: no shapes pass, n_shapes = 0
 *   n_counted[k] / n_idle[k]: counted seeds of verdict k / those of them with no live task (the empty table, shape 0); n_truncated: counted
 *        seeds with more than task_cap live tasks, whose later tasks are in neither table; n_tasks: the visible records of the counted
 *        seeds = the sum of every site's n_total
 * More than site_cap distinct sites, or more than shape_cap distinct shapes: MADSIM_E_LIMITS, and nothing is reported (every output word 0).
 * One chunk (0 = a default, 65 536 or what fits) asks the device for chunk * (16 * task_cap + 96) bytes — the task row and the site row, the
 * count, the shape word, its length word, two unused length words, the seed and the result of every seed — plus, per pass, 32 * slots +
 * 68 * cap + 128: MADSIM_E_LIMITS when that exceeds MADSIM_TRACE_MAX_BYTES.
 * total == 0 / n == 0 reports the empty result.  MADSIM_E_ARG: sc == NULL; include == 0 or a bit at or above 4; task_cap == 0 or above
 * MADSIM_MAX_LIVE_TASKS; site_cap == 0 or above MADSIM_CENSUS_MAX_VALUES or sites == NULL; shapes without shape_cap or the reverse, or
 * shape_cap above MADSIM_CENSUS_MAX_VALUES; runner_cap > 0 without runner_seeds; seeds == NULL with n > 0; a list that is not strictly
 * ascending (sort and deduplicate first). */
typedef struct madsim_stall_census {
    uint32_t include;                  /* in: as madsim_census_t.include                                                          */
    uint32_t task_cap;                 /* in: live tasks of a seed that are visible, 1 .. MADSIM_MAX_LIVE_TASKS                   */
    madsim_census_value_t* sites;      /* in: caller's host array [site_cap]                                                      */
    uint64_t site_cap;                 /* in: 1 .. MADSIM_CENSUS_MAX_VALUES                                                       */
    madsim_census_value_t* shapes;     /* in: caller's host array [shape_cap]; NULL with shape_cap 0: no shapes pass             */
    uint64_t shape_cap;
    uint64_t* runner_seeds;            /* in: caller's host array [runner_cap]; may be NULL when runner_cap == 0                  */
    uint64_t runner_cap;
    uint64_t n_sites;                  /* out: entries of `sites` written, ascending by value                                     */
    uint64_t n_shapes;                 /* out: entries of `shapes` written, ascending by value                                    */
    uint64_t n_counted[4];             /* out: counted seeds per verdict                                                          */
    uint64_t n_idle[4];                /* out: ... of them with no live task                                                      */
    uint64_t n_truncated;              /* out: counted seeds with more than task_cap live tasks                                   */
    uint64_t n_tasks;                  /* out: visible records of the counted seeds = the sum of every site's n_total            */
    uint64_t n_runner;                 /* out: seeds with a runner verdict                                                        */
    uint64_t n_runner_listed;          /* out: min(n_runner, runner_cap), the entries of runner_seeds written                     */
} madsim_stall_census_t;
int madsim_hip_stall_census_range(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total, uint64_t chunk,
                                  const madsim_limits_t* lim, madsim_stall_census_t* sc);
int madsim_hip_stall_census_seeds(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n, uint64_t chunk,
                                  const madsim_limits_t* lim, madsim_stall_census_t* sc);

/* The same entry points on an explicit context (see "Per-device contexts" above). */
int madsim_hip_ctx_run_batch(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                             uint64_t seed0, uint64_t count, const madsim_limits_t* lim,
                             madsim_result_t* out, madsim_summary_t* summary);
int madsim_hip_ctx_run_batch_auto(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                  uint64_t seed0, uint64_t count, const madsim_limits_t* lim,
                                  madsim_result_t* out, madsim_summary_t* summary, int max_rounds);
int madsim_hip_ctx_run_batch_device(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                    uint64_t seed0, uint64_t count, const madsim_limits_t* lim,
                                    void* d_out, void* stream, madsim_summary_t* summary);
int madsim_hip_ctx_run_batch_async(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                   uint64_t seed0, uint64_t count, const madsim_limits_t* lim,
                                   void* d_out, void* d_summary4, void* stream, int timing_slot);
int madsim_hip_ctx_timing_ms(madsim_hip_ctx_t* ctx, int timing_slot, double* ms);
int64_t madsim_hip_ctx_trace_seed(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                  uint64_t seed, const madsim_limits_t* lim, uint8_t* log, uint64_t cap,
                                  madsim_result_t* out);
int madsim_hip_ctx_trace_seeds(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                               const uint64_t* seeds, uint64_t n, const madsim_limits_t* lim, uint8_t* logs, uint64_t log_cap,
                               uint64_t* obs, uint64_t obs_cap, uint64_t* log_len, uint64_t* obs_len, madsim_result_t* out);
int64_t madsim_hip_ctx_observe_seed(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                    uint64_t seed, const madsim_limits_t* lim, uint64_t* obs, uint64_t cap,
                                    madsim_result_t* out);
int madsim_hip_ctx_task_states(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                               const uint64_t* seeds, uint64_t n, const madsim_limits_t* lim, uint64_t* tasks, uint64_t task_cap,
                               uint64_t* task_len, madsim_result_t* out);
int madsim_hip_ctx_timeline_seeds(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                  const uint64_t* seeds, uint64_t n, const madsim_limits_t* lim, uint64_t* obs, uint64_t* times,
                                  uint64_t obs_cap, uint64_t* obs_len, madsim_result_t* out);
int madsim_hip_ctx_diverge_seeds(madsim_hip_ctx_t* ctx, const madsim_workload_t* wA, const madsim_config_t* cfgA,
                                 const madsim_limits_t* limA, const madsim_workload_t* wB, const madsim_config_t* cfgB,
                                 const madsim_limits_t* limB, const uint64_t* seeds, uint64_t n, uint64_t log_cap,
                                 uint64_t obs_cap, uint32_t win, madsim_divergence_t* recs, uint64_t* obs_ctx);
int madsim_hip_ctx_census_range(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0,
                                uint64_t total, uint64_t chunk, const madsim_limits_t* lim, madsim_census_t* cen);
int madsim_hip_ctx_census_seeds(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                const uint64_t* seeds, uint64_t n, uint64_t chunk, const madsim_limits_t* lim, madsim_census_t* cen);
int madsim_hip_ctx_probe_sets_range(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0,
                                    uint64_t total, uint64_t chunk, const madsim_limits_t* lim, madsim_probe_sets_t* ps);
int madsim_hip_ctx_probe_sets_seeds(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                    const uint64_t* seeds, uint64_t n, uint64_t chunk, const madsim_limits_t* lim, madsim_probe_sets_t* ps);
int madsim_hip_ctx_probe_order_range(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0,
                                     uint64_t total, uint64_t chunk, const madsim_limits_t* lim, madsim_probe_order_t* po);
int madsim_hip_ctx_probe_order_seeds(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                     const uint64_t* seeds, uint64_t n, uint64_t chunk, const madsim_limits_t* lim, madsim_probe_order_t* po);
int madsim_hip_ctx_probe_spans_range(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0,
                                     uint64_t total, uint64_t chunk, const madsim_limits_t* lim, madsim_probe_spans_t* ps);
int madsim_hip_ctx_probe_spans_seeds(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                     const uint64_t* seeds, uint64_t n, uint64_t chunk, const madsim_limits_t* lim,
                                     madsim_probe_spans_t* ps);
int madsim_hip_ctx_stall_census_range(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0,
                                      uint64_t total, uint64_t chunk, const madsim_limits_t* lim, madsim_stall_census_t* sc);
int madsim_hip_ctx_stall_census_seeds(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                      const uint64_t* seeds, uint64_t n, uint64_t chunk, const madsim_limits_t* lim, madsim_stall_census_t* sc);

/* One process, several GPUs: the whole seed loop of Builder::run (builder.rs:129-150, every seed driven from one
 * process) over `n_ctx` contexts, each on its own GPU (or, for tests on a 1-GPU box, several on the same one).
 * Seeds are sharded contiguously — context g runs [seed0 + g*ceil(count/n_ctx), ...) —, every device's kernel is
 * queued from the calling thread before any is waited for, results land in `out[count]` (host), seeds that outgrew a
 * device capacity or the step cap are re-run in one compacted launch per round (<= max_rounds, as
 * madsim_hip_run_batch_auto), and the n reports are folded on the host into `summary`.  Bit-identical to
 * madsim_hip_run_batch_auto on a single context.  summary.kernel_ms = the MAXIMUM over the devices (they run concurrently) plus the
 * re-run rounds; madsim_campaign_t.kernel_ms, also over several contexts, is the SUM of every batch's kernel time — the two are not
 * comparable. */
int madsim_hip_run_batch_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* w,
                               const madsim_config_t* cfg, uint64_t seed0, uint64_t count,
                               const madsim_limits_t* lim, madsim_result_t* out, madsim_summary_t* summary,
                               int max_rounds);

/* ---- Campaigns: many batches, kept in flight by the library -------------------------------------------------------------
 * One 65 536-seed batch is one wave per SIMD: alone it leaves two thirds of the issue slots idle (a base-op launch takes ~3.2 ms
 * alone, ~1.3 ms per batch with three in flight).  madsim_hip_run_batch cannot overlap anything — it returns the results —, so
 * the overlap lives here: `total` seeds from `seed0` run as batches of `batch` seeds (0 = 65 536) on the context's own HIP
 * streams, `in_flight` at a time (0 = auto: 3; 5 when the workload's LDS admits four waves per SIMD; 4 for a global-state build with a heap-spill region; more streams than hardware queues are pointless: GPU_MAX_HW_QUEUES), each followed by a
 * device reduction whose 48-byte report is the only thing copied to the host.  Per-seed results are NOT returned: a campaign
 * answers "which is the first failing seed, how many fail" — the seed-search use of `MADSIM_TEST_NUM` — and the caller re-runs
 * the seed it is told about (madsim_hip_run_batch / madsim_hip_trace_seed) for details.
 * MADSIM_CAMPAIGN_STOP_AT_FAILURE: stop launching as soon as a completed batch reports a seed with a GENUINE verdict (panic /
 * deadlock / time limit); batches are contiguous and reports are read in order, so `first_failing_seed` is then the smallest
 * failing seed of [seed0, seed0 + seeds_run): at most `in_flight - 1` batches beyond the failing one have been started.
 * Runner verdicts (MADSIM_OVERFLOW / MADSIM_STEP_LIMIT) never stop a campaign and are counted apart (`n_runner`): pass
 * MADSIM_CAMPAIGN_RESOLVE (below) to have them re-run on the device before the batch is reported, or re-run those ranges with
 * madsim_hip_run_batch_auto. */
#define MADSIM_CAMPAIGN_STOP_AT_FAILURE 1u
typedef struct madsim_campaign {
    uint64_t seeds_run;           /* seeds whose batch ran to completion and was read (a prefix of the range)                 */
    uint64_t batches_run;
    uint64_t batches_launched;    /* >= batches_run: with STOP_AT_FAILURE the batches in flight when the failure was read      */
    uint64_t first_failing_seed;  /* smallest seed with a genuine verdict among seeds_run; UINT64_MAX if none                  */
    uint64_t n_failed;            /* genuine failures among seeds_run                                                          */
    uint64_t n_runner;            /* seeds that came back with a runner verdict (not failures; to be re-run) — with
                                   * MADSIM_CAMPAIGN_RESOLVE: those still left with one after the resolve rounds               */
    uint64_t total_steps, total_clock_ns;
    double   kernel_ms;           /* sum of the simulation kernels' HIP-event durations (they overlap: > wall time)            */
    double   wall_s;
} madsim_campaign_t;
int madsim_hip_ctx_run_campaign(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                uint64_t seed0, uint64_t total, uint64_t batch, uint32_t in_flight, uint32_t flags,
                                const madsim_limits_t* lim, madsim_campaign_t* out);
int madsim_hip_run_campaign(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total,
                            uint64_t batch, uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim,
                            madsim_campaign_t* out);
/* The campaign over several devices from ONE host thread (one context per GPU; the multi-GPU form of `first-fail seeds per hour`):
 * batch k of the range runs on context k % n_ctx, `in_flight` batches per context (0 = auto), and the reports are read in batch order.
 * The devices advance through the seed range together, so MADSIM_CAMPAIGN_STOP_AT_FAILURE stops every device within one round of
 * batches of the first genuine failure, and the report — first_failing_seed, n_failed, n_runner, steps, clock of the prefix
 * [seed0, seed0 + seeds_run) — is the one a single context gives for the same prefix (runtime/builder.rs:129-160: the seeds are
 * seed0 .. seed0 + count whatever runs them, the first failure in seed order is the one reported).  No collective: a report is
 * 48 bytes per batch and the calling thread reads them anyway; ranks that are separate processes gather theirs over RCCL
 * (madsim_amd/dist.py).  Locks the contexts in address order, drains every stream before an error return. */
int madsim_hip_run_campaign_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* w,
                                  const madsim_config_t* cfg, uint64_t seed0, uint64_t total, uint64_t batch,
                                  uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim, madsim_campaign_t* out);

/* ---- Collecting campaigns: WHICH seeds fail, and how ------------------------------------------------------------------------
 * The same campaign, with a report kernel that keeps what the plain one folds away: per batch it counts the seeds per verdict
 * value and compacts the LISTED seeds — those with a genuine verdict (panic / deadlock / time limit); with
 * MADSIM_CAMPAIGN_LIST_RUNNER every verdict but MADSIM_PASS, to hand the seeds to madsim_hip_run_batch_auto — into records of
 * {seed, all 48 result bytes} in ascending seed order, on the device, without an atomic deciding a position: the list is the same
 * on every run.  `out` is exactly what the plain campaign reports for the same arguments (early stops included);
 * col->failures[0 .. n_listed) are the `cap` smallest listed seeds of the prefix [seed0, seed0 + seeds_run), ascending, each with the
 * bytes madsim_hip_run_batch returns for that seed — whatever `batch`, `in_flight` and the number of contexts.  n_by_verdict sums to
 * seeds_run: [1] + [2] + [3] = out->n_failed, [4] + .. + [7] = out->n_runner.
 * Per batch 120 bytes of report come back instead of 48; the records of a batch are copied only when it has listed seeds, and only
 * as many as the list can still take (a full list copies nothing more; the histogram goes on).  cap == 0: histogram only.
 * MADSIM_CAMPAIGN_STOP_AT_CAP: stop launching once the batches read so far hold `cap` listed seeds ("the first 32 failing seeds");
 * seeds_run / batches_run / batches_launched follow the rules of MADSIM_CAMPAIGN_STOP_AT_FAILURE, and the two may be combined.
 * MADSIM_E_ARG: col == NULL, cap > 0 without `failures`, STOP_AT_CAP with cap == 0.  The plain entry points ignore both flags. */
/* (declared in two statements: the one struct of this header that holds another by value, which the header parser the ABI tests share,
 * tests/cheader.py, does not lay out by itself — tests/test_collect.py hands it the inner size) */
struct madsim_failure {
    uint64_t seed;
    madsim_result_t result;       /* as madsim_hip_run_batch returns it for `seed` with the same workload, config and limits      */
};                                /* 56 bytes */
typedef struct madsim_failure madsim_failure_t;
typedef struct madsim_collect {
    madsim_failure_t* failures;   /* caller's host array [cap]; may be NULL when cap == 0 (histogram only)                        */
    uint64_t cap;
    uint64_t n_listed;            /* out: records written = min(cap, listed seeds among seeds_run)                                */
    uint64_t n_by_verdict[8];     /* out: seeds of [seed0, seed0 + seeds_run) per verdict value (index = enum madsim_verdict)     */
} madsim_collect_t;
#define MADSIM_CAMPAIGN_LIST_RUNNER 2u   /* list runner verdicts too                                                              */
#define MADSIM_CAMPAIGN_STOP_AT_CAP 4u   /* stop launching once `cap` listed seeds have been read                                 */
int madsim_hip_ctx_run_campaign_collect(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                        uint64_t seed0, uint64_t total, uint64_t batch, uint32_t in_flight, uint32_t flags,
                                        const madsim_limits_t* lim, madsim_campaign_t* out, madsim_collect_t* col);
int madsim_hip_run_campaign_collect(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total,
                                    uint64_t batch, uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim,
                                    madsim_campaign_t* out, madsim_collect_t* col);
int madsim_hip_run_campaign_collect_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* w,
                                          const madsim_config_t* cfg, uint64_t seed0, uint64_t total, uint64_t batch,
                                          uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim, madsim_campaign_t* out,
                                          madsim_collect_t* col);

/* ---- Campaign statistics: HOW the runs are distributed, and which seeds are the outliers -----------------------------------
 * The same campaign, with report kernels that reduce the four per-seed numbers of madsim_result_t — clock_ns, steps, msg_count,
 * rng_calls — over the COUNTED seeds of every batch: count, minimum, maximum, the exact 128-bit sum, a histogram of 252 logarithmic
 * buckets (four per octave: a bucket is at most 25 % wide) and the `top_k` extreme seeds per metric.  All integer, all exact.
 * A seed is counted when bit `verdict` is set in `include`; only bits 0-3 (PASS, PANIC, DEADLOCK, TIME_LIMIT) exist — a seed with a
 * runner verdict carries no usable numbers and is never counted.
 * bucket(v) = v for v < 4; otherwise, with e the index of v's top set bit, 4 * (e - 1) + ((v >> (e - 2)) & 3): values 0 .. 2^64 - 1
 * map to buckets 0 .. 251.  madsim_hip_stat_bucket / madsim_hip_stat_bucket_floor are host helpers (no device needed):
 * floor(b) = b for b < 4, else (4 + b % 4) << (b / 4 - 1), the smallest value of bucket b; b >= 252 gives UINT64_MAX.
 * top[m * top_k + r], r < n_top: the counted seeds that come first when ordered by metric m descending, then seed ascending (among
 * tied values the smaller seeds win).  No atomic and no arrival order decides a position.
 * Everything is a function of the per-seed results of the prefix [seed0, seed0 + seeds_run): the same bytes whatever `batch`,
 * `in_flight` and the number of contexts, on every run; batches launched beyond a stopping one contribute nothing.  The per-batch
 * statistics (about 5 KB) ride back with the batch's report and are folded on the host in batch order.
 * `out` is exactly the plain campaign's report.  `col` may be NULL (no failure list, no verdict histogram); otherwise it is filled
 * exactly as madsim_hip_run_campaign_collect fills it, and the flags of that form apply.  A batch must hold fewer than 2^32 seeds.
 * MADSIM_E_ARG: st == NULL, include == 0 or a bit at or above 4, top_k > MADSIM_STAT_MAX_TOP, top_k > 0 without `top`, and the
 * collecting form's own argument errors when `col` is given. */
#define MADSIM_STAT_CLOCK 0u      /* madsim_result_t.clock_ns  */
#define MADSIM_STAT_STEPS 1u      /* madsim_result_t.steps     */
#define MADSIM_STAT_MSGS  2u      /* madsim_result_t.msg_count */
#define MADSIM_STAT_RNG   3u      /* madsim_result_t.rng_calls */
#define MADSIM_STAT_METRICS 4u
#define MADSIM_STAT_BUCKETS 256u  /* 252 used */
#define MADSIM_STAT_MAX_TOP 16u
typedef struct madsim_extreme {
    uint64_t value, seed;
} madsim_extreme_t;               /* 16 bytes */
typedef struct madsim_metric {
    uint64_t min, max;            /* over the counted seeds; UINT64_MAX and 0 when there is none                                  */
    uint64_t sum_lo, sum_hi;      /* the 128-bit sum                                                                              */
    uint64_t hist[256];           /* [MADSIM_STAT_BUCKETS]: counted seeds per bucket                                              */
} madsim_metric_t;                /* 2080 bytes */
/* (two statements, as madsim_failure above: it holds madsim_metric_t by value) */
struct madsim_stats {
    uint32_t include;             /* in: bit v set = count the seeds whose verdict is v (bits 0-3 only)                           */
    uint32_t top_k;               /* in: 0 .. MADSIM_STAT_MAX_TOP                                                                 */
    madsim_extreme_t* top;        /* in: caller's host array [MADSIM_STAT_METRICS][top_k]; may be NULL when top_k == 0            */
    uint64_t n;                   /* out: counted seeds of [seed0, seed0 + seeds_run)                                             */
    uint64_t n_top;               /* out: min(top_k, n): entries valid per metric row                                             */
    madsim_metric_t metric[4];    /* [MADSIM_STAT_METRICS]                                                                        */
};
typedef struct madsim_stats madsim_stats_t;
uint32_t madsim_hip_stat_bucket(uint64_t v);
uint64_t madsim_hip_stat_bucket_floor(uint32_t b);
int madsim_hip_ctx_run_campaign_stats(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                      uint64_t seed0, uint64_t total, uint64_t batch, uint32_t in_flight, uint32_t flags,
                                      const madsim_limits_t* lim, madsim_campaign_t* out, madsim_collect_t* col,
                                      madsim_stats_t* st);
int madsim_hip_run_campaign_stats(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total,
                                  uint64_t batch, uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim,
                                  madsim_campaign_t* out, madsim_collect_t* col, madsim_stats_t* st);
int madsim_hip_run_campaign_stats_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* w,
                                        const madsim_config_t* cfg, uint64_t seed0, uint64_t total, uint64_t batch,
                                        uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim, madsim_campaign_t* out,
                                        madsim_collect_t* col, madsim_stats_t* st);

/* ---- Failure-mode grouping: HOW MANY DIFFERENT failures there are, each with its size and a seed to replay -----------------
 * The same campaign, with report kernels that group the COUNTED seeds of every batch by their SIGNATURE (verdict, key): `key` is one
 * 64-bit field of madsim_result_t, obs_hash by default — FNV-1a over the MS_OP_TRACE values in execution order, so a test body that
 * traces "which role / which phase" before it asserts or blocks names its failure modes.  A seed is counted when bit `verdict` is set
 * in `include`; only bits 0-3 (PASS, PANIC, DEADLOCK, TIME_LIMIT) exist, as in madsim_stats_t.include: runner verdicts are never
 * grouped.  Every 64-bit value is a key (0, 2^64 - 1 and the FNV offset basis — the obs_hash of a seed that traced nothing —
 * included), and equal keys under different verdicts are different groups.
 * groups[0 .. n_groups) are the first `cap` groups in order of first appearance: of all the groups of the prefix
 * [seed0, seed0 + seeds_run), those with the smallest `first_seed`, ascending by `first_seed` (unique per group).  Each carries its
 * exact `count` over the WHOLE prefix and its smallest seed.  n_grouped is the sum of the written counts, n_ungrouped the counted
 * seeds that belong to none of the written groups: n_grouped + n_ungrouped is the number of counted seeds of the prefix.
 * Everything is a function of the per-seed results of the prefix: the same bytes whatever `batch`, `in_flight` and the number of
 * contexts, on every run; batches launched beyond a stopping one contribute nothing.  Per batch the number of its groups rides back
 * with the report, and its entries (32 bytes per group of the batch) are copied only when there are some, and only that many.
 * `out` is exactly the plain campaign's report.  `col` and `st` may be NULL; when given they are filled exactly as
 * madsim_hip_run_campaign_collect / madsim_hip_run_campaign_stats fill them (their flags apply): one call, the whole triage report.
 * MADSIM_CAMPAIGN_STOP_AT_GROUPS ("find me `cap` different failures"): stop launching once the batches read so far hold `cap` groups;
 * seeds_run / batches_run / batches_launched follow the rules of MADSIM_CAMPAIGN_STOP_AT_FAILURE, and it may be combined with the
 * other stop flags.  The other entry points ignore it.
 * MADSIM_E_ARG: grp == NULL, include == 0 or a bit at or above 4, an unknown key_field, cap > 0 without `groups`, STOP_AT_GROUPS with
 * cap == 0, min(batch, total) above MADSIM_GROUP_MAX_BATCH seeds (the device table is sized to the batch), and the collecting and
 * statistics forms' own argument errors when `col` / `st` are given. */
#define MADSIM_GROUP_KEY_OBS   0u /* madsim_result_t.obs_hash                  */
#define MADSIM_GROUP_KEY_TRACE 1u /* madsim_result_t.trace_hash                */
#define MADSIM_GROUP_KEY_MSGS  2u /* madsim_result_t.msg_count                 */
#define MADSIM_GROUP_KEY_CLOCK 3u /* madsim_result_t.clock_ns                  */
#define MADSIM_GROUP_KEY_RNG   4u /* madsim_result_t.rng_calls                 */
#define MADSIM_GROUP_KEY_STEPS 5u /* madsim_result_t.steps, zero-extended      */
#define MADSIM_GROUP_KEYS 6u
#define MADSIM_GROUP_MAX_BATCH 1048576u /* 2^20 seeds per batch */
typedef struct madsim_group {          /* 32 bytes */
    uint64_t key;                      /* the grouped field's value (obs_hash by default)                                         */
    uint32_t verdict, reserved;        /* reserved = 0                                                                            */
    uint64_t count;                    /* counted seeds of [seed0, seed0 + seeds_run) in this group                               */
    uint64_t first_seed;               /* the smallest of them                                                                    */
} madsim_group_t;
typedef struct madsim_groups {
    uint32_t include;                  /* in: bit v set = group the seeds whose verdict is v (bits 0-3 only, as madsim_stats_t.include) */
    uint32_t key_field;                /* in: MADSIM_GROUP_KEY_*                                                                  */
    madsim_group_t* groups;            /* in: caller's host array [cap]; may be NULL when cap == 0                                */
    uint64_t cap;
    uint64_t n_groups;                 /* out: entries written                                                                    */
    uint64_t n_grouped;                /* out: sum of the written entries' counts                                                 */
    uint64_t n_ungrouped;              /* out: counted seeds that belong to none of the written groups                            */
} madsim_groups_t;
#define MADSIM_CAMPAIGN_STOP_AT_GROUPS 8u /* stop launching once `cap` groups have been read                                      */
int madsim_hip_ctx_run_campaign_groups(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                       uint64_t seed0, uint64_t total, uint64_t batch, uint32_t in_flight, uint32_t flags,
                                       const madsim_limits_t* lim, madsim_campaign_t* out, madsim_collect_t* col,
                                       madsim_stats_t* st, madsim_groups_t* grp);
int madsim_hip_run_campaign_groups(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t total,
                                   uint64_t batch, uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim,
                                   madsim_campaign_t* out, madsim_collect_t* col, madsim_stats_t* st, madsim_groups_t* grp);
int madsim_hip_run_campaign_groups_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* w,
                                         const madsim_config_t* cfg, uint64_t seed0, uint64_t total, uint64_t batch,
                                         uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim, madsim_campaign_t* out,
                                         madsim_collect_t* col, madsim_stats_t* st, madsim_groups_t* grp);

/* ---- Differential campaigns: TWO variants over one seed range, compared on the device --------------------------------------
 * "I changed something: which seeds changed outcome, did the change break a seed that used to pass, and is every other seed still
 * the same run?"  Side A runs (wA, cfgA, limA) and side B runs (wB, cfgB, limB) over the same seeds — any of the three may be the same
 * pointer on both sides: two test bodies, two loss rates, or one workload under two state layouts / limits, which must give the same
 * 48 bytes for every seed.  Per batch both simulations run on the flight's one stream, each followed by the plain campaign's report
 * kernel, then two diff kernels read both result arrays; nothing is copied back but the report words and the disagreements.
 * A seed is COMPARED when neither side's verdict is a runner verdict (MADSIM_IS_RUNNER_VERDICT: such a seed carries no usable
 * numbers); otherwise it is INCOMPARABLE: it still counts in `transitions`, it never differs and is never listed.  With
 * MADSIM_CAMPAIGN_RESOLVE each side's runner verdicts are first re-run under that side's own grown limits, so only the seeds that no
 * round settles stay incomparable.
 * n_compared + n_incomparable = seeds_run.  A compared seed DIFFERS when any field named in `fields` (MADSIM_DIFF_*) differs;
 * n_by_field[i] counts the compared seeds whose field bit i is masked and differs, so one seed may count in several.
 * records[0 .. n_listed) are the `cap` smallest differing seeds of the prefix [seed0, seed0 + seeds_run), ascending, each with the 48
 * bytes madsim_hip_run_batch returns for that seed on each side; no atomic decides a position.  transitions[a][b] counts the seeds
 * with min(verdict A, 7) = a and min(verdict B, 7) = b: the entries sum to seeds_run, the row sums are what
 * madsim_hip_run_campaign_collect reports as n_by_verdict for side A alone, the column sums the same for side B — "deadlock -> pass:
 * N" is transitions[MADSIM_DEADLOCK][MADSIM_PASS].  outA / outB are exactly the plain campaign's report for that side over the same
 * prefix (kernel_ms from an event pair of the side's own; wall_s is the call's).
 * Everything is a function of the per-seed results of the prefix: the same bytes whatever `batch`, `in_flight` and the number of
 * contexts, on every run; batches launched beyond a stopping one contribute nothing.  Both sides of batch k run on context
 * k % n_ctx; automatic `in_flight` is the smaller of the two sides'.  The records of a batch are copied only when it has differing
 * seeds, and only as many as the list still takes.
 * MADSIM_CAMPAIGN_STOP_AT_DIFFS: stop launching once the batches read so far hold `cap` differing seeds; seeds_run / batches_run /
 * batches_launched follow the rules of MADSIM_CAMPAIGN_STOP_AT_FAILURE.  The other stop flags are ignored by this form, and the other
 * entry points ignore this flag.
 * MADSIM_E_ARG: a NULL diff, outA or outB, fields == 0 or a bit above MADSIM_DIFF_ALL, reserved != 0, cap > 0 without `records`,
 * STOP_AT_DIFFS with cap == 0, and the usual in_flight, seed0 + total and validate errors of either side (the message says which). */
#define MADSIM_DIFF_VERDICT 1u    /* madsim_result_t.verdict    */
#define MADSIM_DIFF_STEPS   2u    /* madsim_result_t.steps      */
#define MADSIM_DIFF_CLOCK   4u    /* madsim_result_t.clock_ns   */
#define MADSIM_DIFF_MSGS    8u    /* madsim_result_t.msg_count  */
#define MADSIM_DIFF_RNG     16u   /* madsim_result_t.rng_calls  */
#define MADSIM_DIFF_TRACE   32u   /* madsim_result_t.trace_hash */
#define MADSIM_DIFF_OBS     64u   /* madsim_result_t.obs_hash   */
#define MADSIM_DIFF_ALL     127u
#define MADSIM_DIFF_FIELDS  7u
#define MADSIM_CAMPAIGN_STOP_AT_DIFFS 16u /* stop launching once `cap` differing seeds have been read                             */
/* (two statements each, as madsim_failure above: the record holds madsim_result_t by value, and the report a two-dimensional array,
 * neither of which tests/cheader.py lays out by itself) */
struct madsim_diff_record {
    uint64_t seed;
    madsim_result_t a, b;              /* as madsim_hip_run_batch returns them for `seed` on side A and on side B                 */
};                                     /* 104 bytes */
typedef struct madsim_diff_record madsim_diff_record_t;
struct madsim_diff {
    uint32_t fields, reserved;         /* in: MADSIM_DIFF_* mask of the fields compared; reserved = 0                             */
    madsim_diff_record_t* records;     /* in: caller's host array [cap]; may be NULL when cap == 0                                */
    uint64_t cap;
    uint64_t n_listed;                 /* out: min(cap, n_differ)                                                                 */
    uint64_t n_compared, n_incomparable, n_differ;
    uint64_t n_by_field[8];            /* out: [i] = compared seeds whose field bit i is masked and differs; [7] = 0              */
    uint64_t transitions[8][8];        /* out: seeds with min(verdict A, 7) = row and min(verdict B, 7) = column                  */
};                                     /* 632 bytes */
typedef struct madsim_diff madsim_diff_t;
int madsim_hip_ctx_run_campaign_diff(madsim_hip_ctx_t* ctx, const madsim_workload_t* wA, const madsim_config_t* cfgA,
                                     const madsim_limits_t* limA, const madsim_workload_t* wB, const madsim_config_t* cfgB,
                                     const madsim_limits_t* limB, uint64_t seed0, uint64_t total, uint64_t batch,
                                     uint32_t in_flight, uint32_t flags, madsim_campaign_t* outA, madsim_campaign_t* outB,
                                     madsim_diff_t* diff);
int madsim_hip_run_campaign_diff(const madsim_workload_t* wA, const madsim_config_t* cfgA, const madsim_limits_t* limA,
                                 const madsim_workload_t* wB, const madsim_config_t* cfgB, const madsim_limits_t* limB,
                                 uint64_t seed0, uint64_t total, uint64_t batch, uint32_t in_flight, uint32_t flags,
                                 madsim_campaign_t* outA, madsim_campaign_t* outB, madsim_diff_t* diff);
int madsim_hip_run_campaign_diff_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* wA,
                                       const madsim_config_t* cfgA, const madsim_limits_t* limA, const madsim_workload_t* wB,
                                       const madsim_config_t* cfgB, const madsim_limits_t* limB, uint64_t seed0, uint64_t total,
                                       uint64_t batch, uint32_t in_flight, uint32_t flags, madsim_campaign_t* outA,
                                       madsim_campaign_t* outB, madsim_diff_t* diff);

/* ---- Self-resolving campaigns: runner verdicts re-run on the device, every report over SETTLED results ----------------------
 * A runner verdict (MADSIM_OVERFLOW, MADSIM_STEP_LIMIT) is a statement about this runner, never an answer: real madsim gives pass /
 * panic / deadlock / time limit for such a seed, so a report that sets those seeds aside is biased — a genuine failure can hide
 * behind an overflow.  MADSIM_CAMPAIGN_RESOLVE, honoured by every campaign entry point (the list forms too), closes the gap: when a harvested
 * batch reports runner verdicts, the re-runnable seeds are compacted into a seed list on the device, run again under grown limits
 * in one launch per round, their 48 bytes written back where they were, and the batch's report kernels run once more — so every
 * field of madsim_campaign_t, madsim_collect_t, madsim_stats_t, madsim_groups_t and madsim_diff_t, and every stop rule, is taken
 * over the RESOLVED results.  A batch without runner verdicts costs nothing new, and without the flag nothing changes at all.
 * The contract is per seed.  Let G(L) be the limits madsim_hip_grow_limits gives for one round over L — the growth step of
 * madsim_hip_run_batch_auto with BOTH the capacities and the step cap grown — and r_j(s) the 48 bytes madsim_hip_run_batch gives
 * for seed s under G^j(lim).  A result is RE-RUNNABLE under L when its verdict is MADSIM_OVERFLOW, or MADSIM_STEP_LIMIT while L's
 * step cap is below its ceiling (max_steps_ceiling); MADSIM_UNSUPPORTED and MADSIM_INTERNAL are never re-run.  With R rounds the
 * resolved result of s is r_k(s) for the smallest k <= R such that k == R or r_k(s) is not re-runnable under G^k(lim).  A round
 * always grows everything and never looks at which verdicts a batch happened to hold, so the resolved result is a function of the
 * seed alone: the same bytes whatever `batch`, `in_flight` and the number of contexts.  It can differ from
 * madsim_hip_run_batch_auto, which grows only what the verdicts at hand ask for, in one corner: a seed that needs more steps only
 * after its capacities grew.
 * R rides in flag bits 8-11 (flags |= R << MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT): 0 means MADSIM_RESOLVE_DEFAULT_ROUNDS, more than
 * MADSIM_RESOLVE_MAX_ROUNDS with the flag set is MADSIM_E_ARG, and without the flag the bits are ignored.  A resolving campaign's
 * batch holds fewer than 2^30 seeds.  The differential form resolves each side with that side's own limits before the diff kernels
 * read the two arrays.  Stop flags are evaluated on the resolved report of each batch (MADSIM_CAMPAIGN_STOP_AT_FAILURE finds a
 * genuine failure that a first-pass overflow was hiding); n_runner and n_by_verdict[4..7] are what is left after the rounds;
 * madsim_campaign_t.kernel_ms includes the re-run kernels.  Grown limits that fit no kernel build fail the call as they fail
 * madsim_hip_run_batch_auto (MADSIM_E_LIMITS), with every stream drained.  Re-run scratch (60 bytes per seed of a batch) is
 * allocated per flight on first need.
 * madsim_hip_campaign_resolved / madsim_hip_ctx_campaign_resolved read the account of the most recent campaign call made through
 * that context (all zero when that call did not resolve, and before any call; the default form also gives zeros when no default
 * context exists): the shape of madsim_hip_timing_ms.  A _multi call stores the same totals in every context it was given; a
 * differential call sums its two sides.  Every integer field is a function of the per-seed ladder r_0 .. r_R over the prefix
 * [seed0, seed0 + seeds_run): batches launched beyond a stopping one contribute nothing. */
#define MADSIM_CAMPAIGN_RESOLVE 32u              /* re-run runner verdicts on the device before a batch is reported          */
#define MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT 8u  /* flag bits 8-11: the number of rounds, 0 = the default                    */
#define MADSIM_CAMPAIGN_RESOLVE_ROUNDS_MASK 3840u    /* 0xf00 (written in decimal: the header's flag parsers read decimal words)  */
#define MADSIM_RESOLVE_DEFAULT_ROUNDS 4u
#define MADSIM_RESOLVE_MAX_ROUNDS 8u
typedef struct madsim_resolve {
    uint64_t n_first_pass;        /* seeds of the prefix whose first pass was re-runnable                                      */
    uint64_t n_resolved;          /* of those, seeds whose resolved verdict is not a runner verdict                            */
    uint64_t n_unresolved;        /* n_first_pass - n_resolved                                                                 */
    uint64_t n_by_round[8];       /* [r]: seeds re-run in round r + 1 ([MADSIM_RESOLVE_MAX_ROUNDS])                            */
    uint64_t batches_resolved;    /* batches of the prefix that needed a round (a differential call: both sides summed)        */
    uint32_t rounds;              /* the R in force; 0 when the call did not resolve                                           */
    uint32_t reserved;
    double   rerun_kernel_ms;     /* sum of the re-run simulation kernels' HIP-event durations (part of kernel_ms)             */
} madsim_resolve_t;
int madsim_hip_campaign_resolved(madsim_resolve_t* out);
int madsim_hip_ctx_campaign_resolved(madsim_hip_ctx_t* ctx, madsim_resolve_t* out);
/* Host helper, no device needed: *out = G^rounds(*lim) (lim == NULL: the defaults), the limits round `rounds` of a resolving
 * campaign runs under — which limits a resolved seed needed, and what to hand madsim_hip_run_batch to reproduce r_j(s).  One round:
 * lanes_per_wave = 0; MADSIM_STATE_COMPACT becomes MADSIM_STATE_AUTO and MADSIM_STATE_NARROW_HEAP is cleared; heap_lds_slots keeps
 * its value (0 becomes 8); heap_spill_slots, max_tasks, mbox_regs, mbox_msgs, max_conns and chan_queue double from their value or,
 * from 0, from 32, n_progs + 8, 2, 2, 4 and 2, up to 2^20, 254, 255, 255 (mbox_msgs of a workload without extended ops: 127, the most its
 * builds take), 127 and 15; max_steps (0 = 2^24) grows 16-fold up to
 * max_steps_ceiling (0 = 2^28, and never below the first pass's cap).  MADSIM_E_ARG: w or out NULL, rounds above 64. */
int madsim_hip_grow_limits(const madsim_workload_t* w, const madsim_limits_t* lim, uint32_t rounds, madsim_limits_t* out);

/* ---- List campaigns: every campaign form over the seeds you NAME -----------------------------------------------------------------
 * The forms above run one contiguous range.  The step behind each of them is not a range: the failing seeds a collecting campaign
 * returned, diffed against a fixed test body; a regression corpus of every seed that ever failed; the members of one failure mode.
 * These entry points take an explicit list instead of (seed0, total): seeds[0 .. n), host memory, read only during the call.
 * THE LIST MUST ASCEND STRICTLY (seeds[i] < seeds[i + 1]) — so that nothing about ordering changes: with an ascending list "smallest
 * seed" and "first position" are the same thing, and every ordering rule of the range forms keeps its wording.  A list that is
 * unsorted or holds a duplicate is MADSIM_E_ARG, never sorted silently.
 * Position i of the list takes the role seed0 + i has in a range campaign:
 *  - batch k is positions [k * batch, min((k + 1) * batch, n)) and runs on context k % n_ctx; reports are read in batch order;
 *  - seeds_run counts POSITIONS of the prefix that was read: where the sections above say "of the prefix [seed0, seed0 + seeds_run)",
 *    read "of seeds[0 .. seeds_run)";
 *  - unchanged in wording: the collect records and the diff records ascend by seed; the statistics' top-K tie-break is "seed
 *    ascending"; a group's first_seed is its smallest seed and the groups come in order of first appearance; first_failing_seed is
 *    the smallest genuinely failing seed of the prefix;
 *  - every flag keeps its meaning (MADSIM_CAMPAIGN_STOP_AT_FAILURE, LIST_RUNNER, STOP_AT_CAP, STOP_AT_GROUPS, STOP_AT_DIFFS, RESOLVE
 *    and its rounds), and madsim_hip_campaign_resolved accounts for a list call as for a range call.
 * Identity: when seeds is seed0, seed0 + 1, .., seed0 + n - 1, every byte of every report (madsim_campaign_t, madsim_collect_t and its
 * records, madsim_stats_t, madsim_groups_t and its entries, madsim_diff_t and its records, madsim_resolve_t) equals the range entry
 * point's, the timing fields kernel_ms, wall_s and rerun_kernel_ms apart.  Restriction: every report is a function of the per-seed
 * results madsim_hip_run_batch returns for each listed seed (after the resolve rounds, if asked for) — the same bytes whatever
 * `batch`, `in_flight` and the number of contexts.
 * madsim_hip_run_seeds_campaign is all four non-differential forms in one: `col`, `st` and `grp` work as in
 * madsim_hip_run_campaign_groups, and each of the three may be NULL (all three NULL: the plain campaign).  Flags that belong to an
 * absent part are ignored; each present part's own argument checks apply.  The differential form is madsim_hip_run_campaign_diff
 * with the list in place of the range; both sides of a batch run the same seeds.
 * Errors are told before any context is looked at, like the other argument errors: MADSIM_E_ARG for seeds == NULL with n > 0, and for
 * a pair that does not ascend (the message names the first offending position i: seeds[i] >= seeds[i + 1]).  The batch-size limits
 * of the statistics, resolving, grouping and differential forms apply to min(batch, n).  n == 0 returns 0 with the reports
 * initialised as for total == 0 (the ctx and default forms: with or without a device).  A list may contain UINT64_MAX: as the
 * remark at first_failing_seed says, test n_failed, not the sentinel.
 * Device memory for the list is 8 bytes per seed of a batch and flight, never proportional to n: a batch's slice is staged through
 * page-locked memory onto the flight's stream ahead of its simulation launch.  The report kernels read a list entry only for a
 * result whose seed they report. */
int madsim_hip_ctx_run_seeds_campaign(madsim_hip_ctx_t* ctx, const madsim_workload_t* w, const madsim_config_t* cfg,
                                      const uint64_t* seeds, uint64_t n, uint64_t batch, uint32_t in_flight, uint32_t flags,
                                      const madsim_limits_t* lim, madsim_campaign_t* out, madsim_collect_t* col,
                                      madsim_stats_t* st, madsim_groups_t* grp);
int madsim_hip_run_seeds_campaign(const madsim_workload_t* w, const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n,
                                  uint64_t batch, uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim,
                                  madsim_campaign_t* out, madsim_collect_t* col, madsim_stats_t* st, madsim_groups_t* grp);
int madsim_hip_run_seeds_campaign_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* w,
                                        const madsim_config_t* cfg, const uint64_t* seeds, uint64_t n, uint64_t batch,
                                        uint32_t in_flight, uint32_t flags, const madsim_limits_t* lim, madsim_campaign_t* out,
                                        madsim_collect_t* col, madsim_stats_t* st, madsim_groups_t* grp);
int madsim_hip_ctx_run_seeds_campaign_diff(madsim_hip_ctx_t* ctx, const madsim_workload_t* wA, const madsim_config_t* cfgA,
                                           const madsim_limits_t* limA, const madsim_workload_t* wB, const madsim_config_t* cfgB,
                                           const madsim_limits_t* limB, const uint64_t* seeds, uint64_t n, uint64_t batch,
                                           uint32_t in_flight, uint32_t flags, madsim_campaign_t* outA, madsim_campaign_t* outB,
                                           madsim_diff_t* diff);
int madsim_hip_run_seeds_campaign_diff(const madsim_workload_t* wA, const madsim_config_t* cfgA, const madsim_limits_t* limA,
                                       const madsim_workload_t* wB, const madsim_config_t* cfgB, const madsim_limits_t* limB,
                                       const uint64_t* seeds, uint64_t n, uint64_t batch, uint32_t in_flight, uint32_t flags,
                                       madsim_campaign_t* outA, madsim_campaign_t* outB, madsim_diff_t* diff);
int madsim_hip_run_seeds_campaign_diff_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* wA,
                                             const madsim_config_t* cfgA, const madsim_limits_t* limA,
                                             const madsim_workload_t* wB, const madsim_config_t* cfgB,
                                             const madsim_limits_t* limB, const uint64_t* seeds, uint64_t n, uint64_t batch,
                                             uint32_t in_flight, uint32_t flags, madsim_campaign_t* outA,
                                             madsim_campaign_t* outB, madsim_diff_t* diff);

/* ---- Sweep campaigns: UP TO EIGHT variants over one seed set, classified across all of them on the device -------------------
 * A differential campaign compares two sides.  The questions behind it are often N-way: one test body under four loss rates
 * ("which settings does this seed fail in: are the failing sets nested?"), a stack of K versions of a test body ("which
 * version first breaks this seed?"), one workload under every state layout ("the same 48 bytes everywhere?").  A sweep campaign
 * runs all n_variants variants (workload, config, limits — any pointer may repeat) of a batch on the flight's one stream, a
 * summary6 kernel after each, then two sweep kernels read all the result arrays; nothing is copied back but the report words
 * and the listed records.  variants[v].out receives the plain campaign's report of variant v over the same prefix.
 * Per seed: variant v's result is PASS (verdict 0), FAIL (1 .. 3) or RUNNER (MADSIM_IS_RUNNER_VERDICT).  fail_mask has bit v set
 * when variant v is FAIL, runner_mask when it is RUNNER.  A seed is SETTLED when runner_mask == 0, otherwise INCOMPARABLE: an
 * incomparable seed counts in n_incomparable and in n_runner_by_variant[v] for every v with runner_mask bit v set, appears
 * nowhere else and is never listed.  n_settled + n_incomparable = seeds_run.  For a settled seed, differ_mask has bit v (v >= 1)
 * set when any field named in `fields` (MADSIM_DIFF_*; 0 = compare nothing) differs between variant v and variant 0 — the field
 * comparison of a differential campaign; n_differ_from_first[v] counts those seeds, n_by_mask[m] the settled seeds with
 * fail_mask == m (entries at or above 2^n_variants stay 0; their sum is n_settled).
 * list_rule names the SELECTED seeds: MADSIM_SWEEP_LIST_MIXED (settled, fail_mask neither 0 nor all n_variants bits: the variants
 * disagree on pass / fail), _FAILING (settled, fail_mask != 0), _DIFFERING (settled, differ_mask != 0).  records[0 .. n_listed) are
 * the `cap` smallest selected seeds of the prefix, ascending by seed, each with its two masks and every variant's verdict; no
 * atomic decides a position.  Every integer is a function of the per-seed results of the prefix: the same bytes whatever `batch`,
 * `in_flight` and the number of contexts; batches launched beyond a stopping one contribute nothing.
 * One signature carries the range and the list form: seeds == NULL runs [seed0, seed0 + total); otherwise seeds[0 .. total) is a
 * strictly ascending list, seed0 must be 0, and every rule of the list section above applies (positions, total == 0 without a
 * device — here for the range too —, the message naming the first offending position).  The entry points are spelled
 * run_sweep_campaign as the list forms are run_seeds_campaign.  Every variant of batch k runs on context k % n_ctx;
 * automatic `in_flight` is the smallest of the variants'.  A batch holds fewer than 2^32 seeds.
 * MADSIM_CAMPAIGN_STOP_AT_SWEEP: stop launching once the batches read so far hold `cap` selected seeds; seeds_run / batches_run /
 * batches_launched (set on every variant's report, as wall_s is) follow the rules of MADSIM_CAMPAIGN_STOP_AT_FAILURE.  The other
 * stop flags are ignored by this form, and the other entry points ignore this one.  With MADSIM_CAMPAIGN_RESOLVE each variant's
 * runner verdicts are first re-run under that variant's own grown limits; madsim_hip_campaign_resolved sums the variants.
 * MADSIM_E_ARG, all told before any context is looked at: n_variants outside 2 .. MADSIM_SWEEP_MAX_VARIANTS; variants, sweep or
 * any w / out NULL; a `fields` bit above MADSIM_DIFF_ALL; list_rule > 2; MADSIM_SWEEP_LIST_DIFFERING with fields == 0; cap > 0
 * without `records`; STOP_AT_SWEEP with cap == 0; seeds != NULL with seed0 != 0 or a list that does not ascend; the usual
 * seed0 + total, in_flight and resolve-flag errors; a validate error of any variant (the message starts "variant 3: "). */
#define MADSIM_SWEEP_MAX_VARIANTS 8u
#define MADSIM_SWEEP_LIST_MIXED     0u  /* settled seeds whose variants disagree on pass/fail: fail_mask not 0 and not all V bits */
#define MADSIM_SWEEP_LIST_FAILING   1u  /* settled seeds that fail in at least one variant: fail_mask != 0                        */
#define MADSIM_SWEEP_LIST_DIFFERING 2u  /* settled seeds with differ_mask != 0                                                    */
#define MADSIM_CAMPAIGN_STOP_AT_SWEEP 64u /* stop launching once `cap` selected seeds have been read                              */
typedef struct madsim_sweep_variant {   /* in: one variant; any pointer may repeat across variants                                */
    const madsim_workload_t* w; const madsim_config_t* cfg; const madsim_limits_t* lim;  /* cfg / lim NULL = defaults, as elsewhere */
    madsim_campaign_t* out;             /* out: the plain campaign's report for this variant over the same prefix                 */
} madsim_sweep_variant_t;
typedef struct madsim_sweep_record {    /* 24 bytes                                                                               */
    uint64_t seed;
    uint32_t fail_mask, differ_mask;
    uint8_t  verdict[8];                /* [v] = variant v's verdict (0..3: listed seeds are settled); 0 for v >= n_variants      */
} madsim_sweep_record_t;
typedef struct madsim_sweep {
    uint32_t fields, list_rule;         /* in: MADSIM_DIFF_* mask compared against variant 0 (0 = compare nothing); MADSIM_SWEEP_LIST_* */
    madsim_sweep_record_t* records;     /* in: caller's host array [cap]; may be NULL when cap == 0                               */
    uint64_t cap;
    uint64_t n_listed;                  /* out: min(cap, n_selected)                                                              */
    uint64_t n_selected;                /* out: seeds of the prefix the list rule selects                                         */
    uint64_t n_settled, n_incomparable; /* out: sum = seeds_run                                                                   */
    uint64_t n_runner_by_variant[8];    /* out: [v] = seeds whose variant v came back with a runner verdict                       */
    uint64_t n_differ_from_first[8];    /* out: [v] = settled seeds whose masked fields differ between variant v and variant 0; [0] = 0 */
    uint64_t n_by_mask[256];            /* out: settled seeds per fail_mask; entries at or above 2^n_variants are 0; sum = n_settled */
} madsim_sweep_t;                       /* 2232 bytes                                                                             */
int madsim_hip_ctx_run_sweep_campaign(madsim_hip_ctx_t* ctx, const madsim_sweep_variant_t* variants, uint32_t n_variants,
                                      uint64_t seed0, uint64_t total, const uint64_t* seeds, uint64_t batch, uint32_t in_flight,
                                      uint32_t flags, madsim_sweep_t* sweep);
int madsim_hip_run_sweep_campaign(const madsim_sweep_variant_t* variants, uint32_t n_variants, uint64_t seed0, uint64_t total,
                                  const uint64_t* seeds, uint64_t batch, uint32_t in_flight, uint32_t flags, madsim_sweep_t* sweep);
int madsim_hip_run_sweep_campaign_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_sweep_variant_t* variants,
                                        uint32_t n_variants, uint64_t seed0, uint64_t total, const uint64_t* seeds, uint64_t batch,
                                        uint32_t in_flight, uint32_t flags, madsim_sweep_t* sweep);

/* ---- Paired campaigns: WHAT A CHANGE DID TO EACH SEED'S NUMBERS ---------------------------------------------------------------
 * A differential campaign says which seeds a change affected; two statistics campaigns give two marginal distributions.  Neither
 * says what a same-seed simulator gives for free: the per-seed DELTA — did the new election timeout make convergence slower in
 * virtual time, by how much, for how many seeds, and which seeds regressed most.  A paired campaign runs side A (wA, cfgA, limA) and
 * side B (wB, cfgB, limB) over the same seeds exactly as a differential campaign does (one stream per flight, a summary6 kernel
 * behind each side), then two paired kernels read both result arrays; nothing is copied back but the report words.
 * Classification, per seed: INCOMPARABLE when either side's verdict is a runner verdict (MADSIM_IS_RUNNER_VERDICT: the differential
 * campaign's rule); PAIRED when both verdicts are below 4, bit `verdict A` is set in include_a and bit `verdict B` in include_b (only
 * bits 0-3 exist, as in madsim_stats_t.include); UNPAIRED otherwise.  n_paired + n_unpaired + n_incomparable = seeds_run.
 * Magnitude rule, per paired seed and metric m (MADSIM_STAT_*: clock_ns, steps, msg_count, rng_calls), a and b the two sides' values
 * compared as unsigned 64-bit numbers: b > a is direction MADSIM_PAIRED_UP with magnitude b - a; a > b is MADSIM_PAIRED_DOWN with
 * magnitude a - b; a == b counts in n_equal[m].  A magnitude is at least 1 and always fits 64 bits: no signed 65-bit quantity
 * appears anywhere.  n[2 m] + n[2 m + 1] + n_equal[m] = n_paired.
 * Index j = 2 * metric + direction: n[j] seeds; delta[j] holds the minimum and maximum magnitude (UINT64_MAX and 0 when there is
 * none, as madsim_metric_t says), the exact 128-bit sum of the magnitudes and hist[madsim_hip_stat_bucket(magnitude)] (bucket 0
 * stays empty).  sum_a / sum_b[m] are the 128-bit sums of the two sides' values over the PAIRED seeds, so both means over the same
 * population come from one call.
 * Order: top[j * top_k + r], r < n_top[j] = min(top_k, n[j]), are the seeds of (metric, direction) j that come first when ordered by
 * magnitude descending, then seed ascending; each entry carries both sides' values of that metric.  No atomic and no arrival order
 * decides a position.
 * Invariants: all integer, all exact; every output is a function of the per-seed results of the prefix that was run — the same bytes
 * whatever `batch`, `in_flight` and the number of contexts, on every run; batches launched beyond a stopping one contribute nothing.
 * A batch holds fewer than 2^32 seeds.  The per-batch words (about 8.5 KB, 11.5 KB with top_k > 0) ride back in one copy and are
 * folded on the host in batch order.
 * `diff` may be NULL.  When given it is filled exactly as madsim_hip_run_campaign_diff fills it (the diff kernels run between side
 * B's summary and the paired kernels), and MADSIM_CAMPAIGN_STOP_AT_DIFFS applies; without it the flag is ignored.  outA / outB are
 * the plain campaign's reports of the two sides.  With MADSIM_CAMPAIGN_RESOLVE each side's runner verdicts are first re-run under
 * that side's own grown limits, the paired kernels run again over the resolved results, and n_incomparable is what no round settled.
 * The run_seeds_campaign_paired forms take a strictly ascending list in place of (seed0, total), under every rule of the list section
 * above.  (The range entry points are spelled run_paired_campaign, as the sweep forms are run_sweep_campaign.)
 * MADSIM_E_ARG: pr == NULL; include_a or include_b 0 or with a bit at or above 4; reserved != 0; top_k > MADSIM_STAT_MAX_TOP;
 * top_k > 0 without `top`; NULL outA or outB; and, when `diff` is given, the differential form's own argument errors. */
#define MADSIM_PAIRED_UP   0u     /* b > a: the metric grew from side A to side B   */
#define MADSIM_PAIRED_DOWN 1u     /* a > b: it shrank                               */
typedef struct madsim_paired_extreme {
    uint64_t seed, a, b;          /* both sides' values of the row's metric         */
} madsim_paired_extreme_t;        /* 24 bytes */
/* (two statements, as madsim_stats above: it holds madsim_metric_t by value) */
struct madsim_paired {
    uint32_t include_a, include_b;     /* in: bit v set = side A's / side B's verdict v qualifies (bits 0-3 only)                 */
    uint32_t top_k, reserved;          /* in: 0 .. MADSIM_STAT_MAX_TOP; reserved = 0                                              */
    madsim_paired_extreme_t* top;      /* in: caller's host array [MADSIM_STAT_METRICS][2][top_k]; may be NULL when top_k == 0    */
    uint64_t n_paired, n_unpaired, n_incomparable;      /* out: sum = seeds_run                                                  */
    uint64_t n_top[8];                 /* out: [2 * metric + direction] = min(top_k, n[..]): entries valid in that row of `top`   */
    uint64_t n[8];                     /* out: [2 * metric + direction] = paired seeds that moved in that direction               */
    uint64_t n_equal[4];               /* out: [metric] = paired seeds with a == b                                                */
    uint64_t sum_a_lo[4];              /* out: [metric] = the 128-bit sum of side A's values over the paired seeds, low word ...  */
    uint64_t sum_a_hi[4];              /*      ... and high word                                                                  */
    uint64_t sum_b_lo[4];              /* out: the same of side B's                                                               */
    uint64_t sum_b_hi[4];
    madsim_metric_t delta[8];          /* out: [2 * metric + direction] = min, max, 128-bit sum and histogram of the magnitudes   */
};                                     /* 16976 bytes */
typedef struct madsim_paired madsim_paired_t;
int madsim_hip_ctx_run_paired_campaign(madsim_hip_ctx_t* ctx, const madsim_workload_t* wA, const madsim_config_t* cfgA,
                                       const madsim_limits_t* limA, const madsim_workload_t* wB, const madsim_config_t* cfgB,
                                       const madsim_limits_t* limB, uint64_t seed0, uint64_t total, uint64_t batch,
                                       uint32_t in_flight, uint32_t flags, madsim_campaign_t* outA, madsim_campaign_t* outB,
                                       madsim_diff_t* diff, madsim_paired_t* pr);
int madsim_hip_run_paired_campaign(const madsim_workload_t* wA, const madsim_config_t* cfgA, const madsim_limits_t* limA,
                                   const madsim_workload_t* wB, const madsim_config_t* cfgB, const madsim_limits_t* limB,
                                   uint64_t seed0, uint64_t total, uint64_t batch, uint32_t in_flight, uint32_t flags,
                                   madsim_campaign_t* outA, madsim_campaign_t* outB, madsim_diff_t* diff, madsim_paired_t* pr);
int madsim_hip_run_paired_campaign_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* wA,
                                         const madsim_config_t* cfgA, const madsim_limits_t* limA, const madsim_workload_t* wB,
                                         const madsim_config_t* cfgB, const madsim_limits_t* limB, uint64_t seed0, uint64_t total,
                                         uint64_t batch, uint32_t in_flight, uint32_t flags, madsim_campaign_t* outA,
                                         madsim_campaign_t* outB, madsim_diff_t* diff, madsim_paired_t* pr);
int madsim_hip_ctx_run_seeds_campaign_paired(madsim_hip_ctx_t* ctx, const madsim_workload_t* wA, const madsim_config_t* cfgA,
                                             const madsim_limits_t* limA, const madsim_workload_t* wB, const madsim_config_t* cfgB,
                                             const madsim_limits_t* limB, const uint64_t* seeds, uint64_t n, uint64_t batch,
                                             uint32_t in_flight, uint32_t flags, madsim_campaign_t* outA, madsim_campaign_t* outB,
                                             madsim_diff_t* diff, madsim_paired_t* pr);
int madsim_hip_run_seeds_campaign_paired(const madsim_workload_t* wA, const madsim_config_t* cfgA, const madsim_limits_t* limA,
                                         const madsim_workload_t* wB, const madsim_config_t* cfgB, const madsim_limits_t* limB,
                                         const uint64_t* seeds, uint64_t n, uint64_t batch, uint32_t in_flight, uint32_t flags,
                                         madsim_campaign_t* outA, madsim_campaign_t* outB, madsim_diff_t* diff, madsim_paired_t* pr);
int madsim_hip_run_seeds_campaign_paired_multi(madsim_hip_ctx_t* const* ctxs, int n_ctx, const madsim_workload_t* wA,
                                               const madsim_config_t* cfgA, const madsim_limits_t* limA,
                                               const madsim_workload_t* wB, const madsim_config_t* cfgB,
                                               const madsim_limits_t* limB, const uint64_t* seeds, uint64_t n, uint64_t batch,
                                               uint32_t in_flight, uint32_t flags, madsim_campaign_t* outA,
                                               madsim_campaign_t* outB, madsim_diff_t* diff, madsim_paired_t* pr);

/* Geometry the library picked for a workload (for DESIGN/bench reporting). */
typedef struct madsim_geometry {
    uint32_t lds_bytes_per_seed;
    uint32_t lds_bytes_per_block;
    uint32_t block_threads;
    uint32_t blocks_per_cu;
    uint32_t grid_blocks;
    uint32_t heap_lds_slots;
    uint32_t heap_spill_slots;
    uint32_t max_tasks;
    uint32_t lanes_per_wave;
    uint32_t variant;              /* kernel specialisation: bit0 heap spill, bit1 extended ops, bit2 ready queue in a
                                    * register, bit3 runtime lane stride, bit4 global-state build; bits 8-12 = classes of extended ops compiled in
                                    * (1 timeouts, 2 channel, 4 RPC, 8 node lifecycle, 16 general address resolution), bit 13 = built without the determinism-log
                                    * fold (madsim_limits_t.no_trace_hash on a base-op workload), bit 14 = the compact base-op layout (MADSIM_STATE_COMPACT), bit 15 = 8-byte
                                    * timer-heap entries (MADSIM_STATE_NARROW_HEAP); bits 16-19 = compile-time log2 lane
                                    * stride (15 = runtime); bit 20 = timeout scopes compiled in (MS_OP_TIMEOUT_BEGIN / END); bit 21 = interval
                                    * tickers compiled in (MS_OP_INTERVAL / TICK / INTERVAL_RESET); bit 22 = selects compiled in (MS_OP_RECV_OR_TICK /
                                    * RECV_TIMEOUT_AT, v7); bit 23 = ctrl-c signals compiled in (MS_OP_CTRL_C / SEND_CTRL_C / RECV_OR_CTRL_C) */
    uint32_t global_bytes_per_seed; /* size of a lane's state block in global memory (global-state builds), else 0 */
} madsim_geometry_t;
int madsim_hip_geometry(const madsim_workload_t* w, const madsim_limits_t* lim, madsim_geometry_t* g);

/* Debug aid: per-phase cycle accumulators of a profiling build of the kernel (all zero otherwise). */
int madsim_hip_debug_counters(uint64_t* out16);

/* Built-in workload of SURVEY.md §8d: N-node ping-pong, R rounds per pair.  Fills caller storage;
 * returns the number of instructions written or <0 if `cap_insns` is too small. */
int madsim_workload_pingpong(uint32_t n_nodes, uint32_t rounds, madsim_node_t* nodes /*[n_nodes+1]*/,
                             madsim_prog_t* progs /*[n_nodes+1]*/, madsim_sock_t* socks /*[n_nodes]*/,
                             madsim_insn_t* insns, uint32_t cap_insns, madsim_workload_t* w);

#ifdef __cplusplus
}
#endif
#endif /* MADSIM_HIP_H */
