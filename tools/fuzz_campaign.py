#!/usr/bin/env python3
"""Extended parity fuzzing on a GPU box: fresh random workloads (tests/fuzz.py generators, new generator seeds) through the
C-ABI vs the CPU oracle, bit-exact on all 48 result bytes.  Usage: fuzz_campaign.py [seconds] [base_seed] [generators]"""
import os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import oracle
from madsim_amd import runtime, _abi as A
from tests import fuzz, parity
from tests import tier_blocks as TB

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
base = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
runtime.init(0)
gens = [("plain", fuzz.random_workload, None), ("lifecycle", fuzz.random_lifecycle_workload, 24), ("rpc", fuzz.random_rpc_workload, 24),
        ("rpc+hooks", lambda r: fuzz.random_rpc_workload(r, hooks=True), 24), ("addresses", fuzz.random_addr_workload, None),
        ("ephemeral", fuzz.random_ephemeral_workload, None), ("channel", fuzz.random_channel_workload, 24),
        ("guards", fuzz.random_guard_workload, 24), ("supervisor", fuzz.random_supervisor_workload, 48),
        ("mixed", fuzz.random_mixed_workload, 60), ("ipvs", fuzz.random_ipvs_workload, 24), ("ipvs_rt", fuzz.random_ipvs_runtime_workload, 24),
        ("timeouts", fuzz.random_timeout_workload, None), ("stale_from", fuzz.random_reply_without_receive_workload, None),
        ("op_soup", fuzz.random_unstructured_workload, 16), ("latency", fuzz.random_latency_workload, None)]
# the op families with builds of their own (timeout scopes, interval tickers, selects, ctrl-c signals): "tier_<family>", with the
# hazards of the test blocks, general addresses on a third of the programs, under the family's limits (LDS; global on alternate rounds)
tiers = {"tier_" + f.name: f for f in TB.FAMILIES.values()}
gens += [(name, (lambda r, f=f: f.gen(r, general_addr=r.random() < 1 / 3, hazards=True)), None) for name, f in tiers.items()]
if len(sys.argv) > 3:                              # optional: only the generators whose name contains one of these (comma-separated)
    gens = [g for g in gens if any(x in g[0] for x in sys.argv[3].split(","))]
t0 = time.time(); k = 0; tally = parity.Tally(); n_narrow = 0
while time.time() - t0 < budget:
    name, gen, max_tasks = gens[k % len(gens)]
    w, cfg, desc = gen(random.Random(base + k))
    lim = tiers[name].limits() if name in tiers else fuzz.mailbox_limits() if name in ("timeouts", "stale_from", "latency") else fuzz.generous_limits()
    if max_tasks: lim.max_tasks = max_tasks
    if (k // len(gens)) % 2:          # every other round: per-seed state in the global-memory block instead of LDS (Variant::G)
        lim.lanes_per_wave, lim.state_mem = 0, A.STATE_GLOBAL
        if name == "timeouts":
            lim.state_mem |= A.STATE_DEDUP_TIMERS      # re-registered Sleep timers as counts (k_timer.h dedup_note)
            if (k // len(gens)) % 4 == 3: lim.lanes_per_wave = 32     # ... on 32 seed lanes per wave (the election loop's layout since round 4)
        if (k // len(gens)) % 8 >= 5:     # every other global round: 8-byte heap entries + delivery record pool (round 6), a small LDS quota so that the
            lim.state_mem |= A.STATE_NARROW_HEAP          # spill region is in use; honoured where a narrow build exists for the program's op classes
            q = 1 + (k // len(gens)) % 5
            lim.heap_spill_slots, lim.heap_lds_slots = lim.heap_spill_slots + max(0, lim.heap_lds_slots - q), q
    if k % 5 == 4:                    # every fifth program in the reference's plain mode: no determinism-log fingerprint (rand.rs:67)
        lim.no_trace_hash = 1
    n = 96
    try:
        if (runtime.geometry(w, lim).variant >> 8) & 0x80: n_narrow += 1                # every seed is compared: first-pass capacity verdicts go through madsim_hip_run_batch_auto and are then held against the oracle
        parity.gpu_compare(runtime, w, 1000 + 7 * k, n, cfg, lim, name, tally, (f"generator={name} gen_seed={base + k}", desc))
    except runtime.MadsimHipError:            # refused by validate() (the op-soup generator writes programs that are): nothing to compare
        k += 1
        continue
    except AssertionError as ex:
        print("MISMATCH", ex)
        sys.exit(1)
    k += 1
verdicts = np.bincount(np.array(sorted(tally.verdicts), dtype=np.int64), minlength=8)
print(f"fuzz campaign ok: {k} workloads, {tally.n} seeds in {time.time() - t0:.0f} s, all 48 result bytes of EVERY seed equal to the oracle's; "
      f"{tally.rerun} of them after a re-run with grown capacities (first pass MADSIM_OVERFLOW); unresolved: {tally.unresolved} "
      f"(proven beyond the layout's ceilings by the oracle's high-water marks; anything else fails); oracle verdicts seen: {sorted(tally.verdicts)}")
print(f"programs run on the narrow-heap builds: {n_narrow}")
print("per generator:", tally)
if tally.reasons: print("beyond the ceilings, by capacity (the oracle's high-water mark of the seed exceeds what the layout can hold at all):", tally.reasons)
