/*
 * madsim_oracle.h — CPU ORACLE (test infrastructure, NOT the product; see madsim_oracle.c).
 * Same workload/config/result types as the product ABI so parity tests feed both the same bytes.
 */
#ifndef MADSIM_ORACLE_H
#define MADSIM_ORACLE_H

#include "../include/madsim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* High-water marks of the reference's unbounded containers, used to size device capacities. */
typedef struct madsim_oracle_stats {
    uint32_t max_heap;   /* naive_timer BinaryHeap length */
    uint32_t max_ready;  /* ready Vec length */
    uint32_t max_tasks;  /* live futures */
    uint32_t max_msgs;   /* Mailbox.msgs per socket */
    uint32_t max_regs;   /* Mailbox.registered per socket */
    uint32_t max_conns;  /* live connections */
    uint32_t max_cq;     /* queued payloads per channel direction */
    /* TEST-ONLY event counters of the timer-tier and signal ops, SUMMED over the seeds of the run (the fields above are maxima): what
     * tests/test_oracle_tiers.py checks a fuzz block against, so that a block which never expires a scope cannot pass for one that does */
    uint32_t scopes_expired;    /* timeout scopes whose Sleep elapsed: the block was dropped                           */
    uint32_t scopes_completed;  /* timeout scopes whose block reached its MS_OP_TIMEOUT_END                            */
    uint32_t ticks_first_poll;  /* MS_OP_TICKs Ready at their first poll (no timer, no yield)                          */
    uint32_t ticks_parked;      /* MS_OP_TICKs that were Pending at their first poll                                   */
    uint32_t sel_won_recv;      /* selects (RECV_OR_TICK, RECV_TIMEOUT_AT, RECV_OR_CTRL_C) the recv arm won            */
    uint32_t sel_won_time;      /* ... the tick arm or timeout_at's Sleep won                                          */
    uint32_t sel_won_ctrl_c;    /* ... the ctrl-c arm won                                                              */
    uint32_t msgs_lost;         /* messages a dropped recv arm had taken into its rand_delay                           */
    uint32_t sig_lost;          /* ctrl-c signals nobody waited for, or dropped with a select's subscription           */
    uint32_t sig_caught;        /* ctrl_c() calls and ctrl-c arms that completed                                       */
    uint32_t sig_killed;        /* ctrl-c signals to a node without a handler: kill_id                                 */
    /* TEST-ONLY counters of the timer heap, summed likewise: what tests/heap_cases.py holds its tie-dense workloads to */
    uint32_t heap_pops;         /* BinaryHeap::pop calls                                                               */
    uint32_t heap_tie_pops;     /* ... after which the new root's deadline equals the popped entry's                   */
    /* TEST-ONLY poll counters, summed likewise: op_polls[op] = how often a task body was polled while it stood at an instruction with
     * that opcode (first polls and re-polls alike; a light op that runs through counts once).  The device equals this oracle seed for
     * seed, so "the seeds of a case poll op X" holds for every build the case runs on: what tests/build_cases.py rests on */
    uint32_t op_polls[MS_OP__COUNT];
} madsim_oracle_stats_t;

/* Events in which a seed leaves the device runner's workload MODEL (not reference concepts; madsim_oracle.c model_event). */
#define MADSIM_ORACLE_ME_TASKS      1u   /* a 255th live task                                                              */
#define MADSIM_ORACLE_ME_REGS       2u   /* a 256th registration in one socket's mailbox                                   */
#define MADSIM_ORACLE_ME_REG_ALIAS  4u   /* a new registration whose 8-bit rxseq / generation bytes equal a dead one's      */
#define MADSIM_ORACLE_ME_CHAN_QUEUE 8u   /* a 16th payload queued in one channel direction                                 */
#define MADSIM_ORACLE_ME_ACCEPTQ    16u  /* a ninth connection waiting in one Endpoint's accept1 queue                     */
#define MADSIM_ORACLE_ME_IPVS       32u  /* a seventh server of one IPVS service                                           */
#define MADSIM_ORACLE_ME_PANIC_DYN  64u  /* a formatted panic value above madsim_workload_t.panic_dyn_max                  */
#define MADSIM_ORACLE_ME_EPH_REBIND 128u /* a port-0 entry bound again beside the live Endpoint of its previous bind       */
#define MADSIM_ORACLE_ME_EPH_STALE  256u /* an op through a port-0 entry that no longer names the socket its last bind made */
#define MADSIM_ORACLE_ME_GUARDS     512u /* a 128th connection end holding one Endpoint's BindGuard                          */
#define MADSIM_ORACLE_ME_EPH_PORTS  1024u /* an ephemeral bind whose port lies beyond the table's candidate ports of that (node, IP) */
#define MADSIM_ORACLE_ME_CONNS      2048u /* a 128th live connection                                                        */
#define MADSIM_ORACLE_ME_MSGS       4096u /* a 256th message queued in one mailbox                                          */
#define MADSIM_ORACLE_ME_SIG_WAITERS 8192u /* a ctrl-c signal that would schedule two or more waiters of one node           */

/* An opcode this oracle has no case for (one beyond the table, or of an op family it does not restate): the call fails, it never
 * becomes a verdict.  Returned by every entry point below (the trace / observe ones return it as their negative length). */
#define MADSIM_ORACLE_E_OPCODE (-100)

/* `stats` here is the struct as it was before op_polls: the caller allocates it, and callers built against the earlier header pass those
 * MADSIM_ORACLE_STATS_V1_BYTES — this entry point writes nothing behind them.  The whole struct: madsim_oracle_run_batch_sized. */
#define MADSIM_ORACLE_STATS_V1_BYTES 80u   /* offsetof(madsim_oracle_stats_t, op_polls) */
int madsim_oracle_run_batch(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0,
                            uint64_t count, const madsim_limits_t* lim, madsim_result_t* out,
                            madsim_summary_t* summary, madsim_oracle_stats_t* stats);
/* ... with `stats_bytes` = the size of the caller's struct (sizeof(madsim_oracle_stats_t) for the current one): nothing behind it is
 * read or written, so the struct can go on growing at its end. */
int madsim_oracle_run_batch_sized(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0,
                                  uint64_t count, const madsim_limits_t* lim, madsim_result_t* out,
                                  madsim_summary_t* summary, void* stats, uint64_t stats_bytes);

/* The same restatement with the model's ceilings switched OFF: unbounded containers throughout, `events[i]` = MADSIM_ORACLE_ME_*
 * mask of seed i (0 = the seed never met a ceiling, and its result equals madsim_oracle_run_batch's byte for byte). */
int madsim_oracle_run_batch_pure(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t count,
                                 const madsim_limits_t* lim, madsim_result_t* out, uint32_t* events);

/* CPU twin of madsim_hip_run_batch with the identical signature. */
int madsim_cpu_run_batch(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed0, uint64_t count,
                         const madsim_limits_t* lim, madsim_result_t* out, madsim_summary_t* summary);

int64_t madsim_oracle_trace_seed(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed,
                                 const madsim_limits_t* lim, uint8_t* log, uint64_t cap,
                                 madsim_result_t* out);

/* One seed plus the list of values it made observable (MS_OP_TRACE / MS_OP_TRACE_TIME, what obs_hash folds). */
int64_t madsim_oracle_observe_seed(const madsim_workload_t* w, const madsim_config_t* cfg, uint64_t seed,
                                   const madsim_limits_t* lim, uint64_t* obs, uint64_t cap, madsim_result_t* out);

/* Building blocks exposed for the known-answer tests. */
void     oracle_seed_from_u64(uint64_t seed, uint64_t s[4]);
uint64_t oracle_xoshiro_next(uint64_t s[4]);
uint64_t madsim_oracle_gen_range(uint64_t s[4], uint64_t lo, uint64_t hi, uint64_t* ncalls);
void     oracle_uniform_duration_params(uint64_t lo, uint64_t hi, int* mode, uint64_t* low,
                                        uint64_t* range, uint64_t* zone);

#ifdef __cplusplus
}
#endif
#endif
