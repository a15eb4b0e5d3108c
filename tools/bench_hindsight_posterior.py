#!/usr/bin/env python3
"""Time hindsight_posterior_optimum() next to hindsight_optimum() in one process on bench.py's configs[2] tables
(n_samples = 100): HIP events around whole calls (host side included: torch.unique and the gather of share=True are
part of that call), one warm-up, the three calls interleaved (A B C A B C ...), median and spread of --reps. One JSON
line per batch size with the number of distinct problems share=True found and the ratio of the share=False time to
n_samples x the hindsight_optimum() time of the same run. A size is skipped (and says so) once the share=False call of
the size before it, scaled by the env count, would pass --max-seconds.

    python tools/bench_hindsight_posterior.py [--envs 65536 1048576] [--reps 3] [--max-seconds 60]   # needs one ROCm GPU
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
ap.add_argument("--envs", type=int, nargs="+", default=[1 << 16, 1 << 20])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--max-seconds", type=float, default=60.0)
args = ap.parse_args()

tables = compile_from_synth(synth.make_synth("linear", years=list(range(2006, 2017)), n_samples=100, seed=0,
                                             extra_confounder_fips=60))  # bench.py's configs[2]


def once(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


per_env_ms = None  # share=False milliseconds per env at the size before
for n in args.envs:
    if per_env_ms is not None and per_env_ms * n > args.max_seconds * 1e3:
        print(json.dumps({"envs": n, "skipped": f"share=False would take about {per_env_ms * n / 1e3:.0f} s"}))
        continue
    env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
    env.reset(seed=0)
    st0 = {k: v.clone() for k, v in env.state().items()}
    calls = {"hindsight_optimum": lambda: env.hindsight_optimum(st0),
             "posterior_unshared": lambda: env.hindsight_posterior_optimum(st0, share=False),
             "posterior_shared": lambda: env.hindsight_posterior_optimum(st0, share=True)}
    times = {k: [] for k in calls}
    keys = None
    for i in range(args.reps + 1):  # the first round warms all three up
        for k, fn in calls.items():
            ms = once(fn)[0]
            if k == "posterior_shared":
                keys = env.last_hindsight_posterior_keys
            if i:
                times[k].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    per_env_ms = med["posterior_unshared"] / n
    line = {"envs": n, "days": tables.T, "n_samples": tables.n_samples, "distinct_keys": keys, "reps": args.reps}
    for k, v in times.items():
        line[k + "_ms"] = round(med[k], 3)
        line[k + "_spread_ms"] = round(max(v) - min(v), 3)
    line["unshared_over_n_samples_x_optimum"] = round(med["posterior_unshared"] / (tables.n_samples * med["hindsight_optimum"]), 3)
    line["shared_over_unshared"] = round(med["posterior_shared"] / med["posterior_unshared"], 4)
    print(json.dumps(line), flush=True)
    env.close()
