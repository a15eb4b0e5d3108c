#!/usr/bin/env python3
"""Time hindsight_posterior_budget_curve(B) next to the hindsight_posterior_optimum() calls it replaces, in one process
on bench.py's configs[2] tables (100 draws), B = 19 (the batch's largest default remaining budget): HIP events around
whole calls (host side included), every side with share=False, one warm-up round, the calls interleaved
(A B C A B C ...), median and spread of --reps. The sweep the curve replaces is B + 1 hindsight_posterior_optimum()
calls, one per twin budget, timed as that loop (--sweep-reps times, after a warm-up call). Also the share=True call and
the number of distinct problems it ran. One JSON line.

    python tools/bench_hindsight_posterior_curve.py [--envs 65536] [--reps 3] [--sweep-reps 1]   # needs one ROCm GPU
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, synth

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=1 << 16)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--sweep-reps", type=int, default=1)
ap.add_argument("--max-budget", type=int, default=19)
args = ap.parse_args()

tables = compile_from_synth(synth.make_synth("linear", years=list(range(2006, 2017)), n_samples=100, seed=0,
                                             extra_confounder_fips=60))  # bench.py's configs[2]
n = args.envs
env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
env.reset(seed=0)
st0 = {k: v.clone() for k, v in env.state().items()}
B = args.max_budget


def once(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def twin(b):
    return {**st0, "budget": st0["used"] + b}


calls = {"optimum": lambda: env.hindsight_posterior_optimum(st0, share=False),
         "optimum_twin_B": lambda: env.hindsight_posterior_optimum(twin(B), share=False),
         "curve": lambda: env.hindsight_posterior_budget_curve(B, start_state=st0, share=False),
         "curve_schedules": lambda: env.hindsight_posterior_budget_curve(B, start_state=st0, schedules=True, packed=True,
                                                                         share=False),
         "curve_shared": lambda: env.hindsight_posterior_budget_curve(B, start_state=st0)}
times = {k: [] for k in calls}
keys = None
for i in range(args.reps + 1):  # the first round warms every call up
    for k, fn in calls.items():
        ms, out = once(fn)
        del out
        if k == "curve_shared":
            keys = env.last_hindsight_posterior_keys
        if i:
            times[k].append(ms)
med = {k: statistics.median(v) for k, v in times.items()}
row = {"envs": n, "days": tables.T, "n_samples": tables.n_samples, "max_budget": B, "reps": args.reps,
       "default_max_remaining": int((st0["budget"] - st0["used"]).max())}
for k, v in times.items():
    row[k + "_ms"] = round(med[k], 3)
    row[k + "_spread_ms"] = round(max(v) - min(v), 3)
row["shared_keys"] = keys
row["curve_over_one_call"] = round(med["curve"] / med["optimum"], 3)
row["curve_schedules_over_one_call"] = round(med["curve_schedules"] / med["optimum"], 3)
twins = [twin(b) for b in range(B + 1)]
sweeps = [once(lambda: [env.hindsight_posterior_optimum(t, share=False)["return"] for t in twins])[0]
          for _ in range(args.sweep_reps)]
if sweeps:  # the B + 1 calls themselves, budgets 0 .. B
    ms = statistics.median(sweeps)
    row["sweep_ms"] = round(ms, 3)
    row["sweep_over_curve"] = round(ms / med["curve"], 3)
    row["sweep_over_curve_schedules"] = round(ms / med["curve_schedules"], 3)
    row["curve_faster_than_sweep"] = bool(med["curve"] < ms and med["curve_schedules"] < ms)
print(json.dumps(row))
env.close()
