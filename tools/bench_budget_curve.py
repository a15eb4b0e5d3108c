#!/usr/bin/env python3
"""Time hindsight_budget_curve(B) next to the hindsight_optimum() calls it replaces, in one process on bench.py's
configs[2] tables, B the batch's largest default remaining budget: HIP events around whole calls (host side included),
one warm-up round, the calls interleaved (A B C A B C ...), median and spread of --reps. The sweep the curve replaces is
B + 1 hindsight_optimum() calls, one per twin budget; --sweep also times that loop itself (B + 1 calls, once). One JSON
line.

    python tools/bench_budget_curve.py [--envs 1048576] [--reps 5] [--sweep]      # needs one ROCm GPU
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
ap.add_argument("--envs", type=int, default=1 << 20)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sweep", action="store_true")
args = ap.parse_args()

tables = compile_from_synth(synth.make_synth("linear", years=list(range(2006, 2017)), n_samples=100, seed=0,
                                             extra_confounder_fips=60))  # bench.py's configs[2]
n = args.envs
env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
env.reset(seed=0)
st0 = {k: v.clone() for k, v in env.state().items()}
B = int((st0["budget"] - st0["used"]).max())


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


calls = {"hindsight_optimum": lambda: env.hindsight_optimum(st0),
         "hindsight_optimum_twin_B": lambda: env.hindsight_optimum(twin(B)),
         "curve": lambda: env.hindsight_budget_curve(B, start_state=st0),
         "curve_schedules": lambda: env.hindsight_budget_curve(B, start_state=st0, schedules=True, packed=True)}
times = {k: [] for k in calls}
for i in range(args.reps + 1):  # the first round warms every call up
    for k, fn in calls.items():
        ms, out = once(fn)
        del out
        if i:
            times[k].append(ms)
med = {k: statistics.median(v) for k, v in times.items()}
row = {"envs": n, "days": tables.T, "max_budget": B, "reps": args.reps}
for k, v in times.items():
    row[k + "_ms"] = round(med[k], 3)
    row[k + "_spread_ms"] = round(max(v) - min(v), 3)
row["curve_over_one_call"] = round(med["curve"] / med["hindsight_optimum"], 3)
row["curve_schedules_over_one_call"] = round(med["curve_schedules"] / med["hindsight_optimum"], 3)
if args.sweep:  # the B + 1 calls themselves, budgets 0 .. B
    twins = [twin(b) for b in range(B + 1)]
    ms, _ = once(lambda: [env.hindsight_optimum(t)["return"] for t in twins])
    row["sweep_ms"] = round(ms, 3)
    row["sweep_over_curve"] = round(ms / med["curve"], 3)
    row["sweep_over_curve_schedules"] = round(ms / med["curve_schedules"], 3)
print(json.dumps(row))
env.close()
