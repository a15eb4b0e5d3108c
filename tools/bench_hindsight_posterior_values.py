#!/usr/bin/env python3
"""Time hindsight_posterior_values() next to hindsight_posterior_optimum() in one process on bench.py's configs[2]
tables (n_samples = 100), both with share=False (every env runs its own DP: the kernels are compared, not the host-side
sharing): HIP events around whole calls (host side included: the packed schedule is passed as int32 words, so nothing
is packed per call), one warm-up, the three calls interleaved (A B C A B C ...), median and spread of --reps. One JSON
line per batch size with the ratios of the medians to hindsight_posterior_optimum()'s.

    python tools/bench_hindsight_posterior_values.py [--envs 1048576 65536] [--reps 3]      # needs one ROCm GPU
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, policy, synth

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, nargs="+", default=[1 << 20, 1 << 16])
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

tables = compile_from_synth(synth.make_synth("linear", years=list(range(2006, 2017)), n_samples=100, seed=0,
                                             extra_confounder_fips=60))  # bench.py's configs[2]
words = (tables.T + 31) // 32


def once(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


for n in args.envs:
    env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
    env.reset(seed=0)
    st0 = {k: v.clone() for k, v in env.state().items()}
    gen = torch.Generator(device=env.device).manual_seed(0)
    sched = policy.pack_alert_days(torch.rand((n, tables.T), generator=gen, device=env.device) < 0.1, words)
    calls = {"posterior_optimum": lambda: env.hindsight_posterior_optimum(st0, share=False),
             "posterior_values": lambda: env.hindsight_posterior_values(sched, start_state=st0, share=False),
             "posterior_values_value_loss": lambda: env.hindsight_posterior_values(sched, start_state=st0, value=True,
                                                                                   loss=True, share=False)}
    times = {k: [] for k in calls}
    for i in range(args.reps + 1):  # the first round warms all three up
        for k, fn in calls.items():
            ms = once(fn)[0]
            if i:
                times[k].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    line = {"envs": n, "days": tables.T, "n_samples": tables.n_samples, "reps": args.reps}
    for k, v in times.items():
        line[k + "_ms"] = round(med[k], 3)
        line[k + "_spread_ms"] = round(max(v) - min(v), 3)
    line["values_over_optimum"] = round(med["posterior_values"] / med["posterior_optimum"], 3)
    line["values_value_loss_over_optimum"] = round(med["posterior_values_value_loss"] / med["posterior_optimum"], 3)
    print(json.dumps(line), flush=True)
    env.close()
