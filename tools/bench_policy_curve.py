#!/usr/bin/env python3
"""Time policy_budget_curve(B = 19) next to what it replaces, in one process on bench.py's configs[2] tables: one
rollout(linear), the curve with and without packed schedules, and the B + 1 reset(budget=b) + rollout() calls of the
sweep. HIP events around whole calls (host side included), one warm-up round, the calls interleaved (A B C D A B C D
...), median and spread of --reps. The sweep is existing code on the same commit: the yardstick. One JSON line per batch
size.

    python tools/bench_policy_curve.py [--envs 1048576 65536] [--reps 5] [--budget 19]      # needs one ROCm GPU
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, synth

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, nargs="+", default=[1 << 20, 1 << 16])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--budget", type=int, default=19)
ap.add_argument("--groups", type=int, default=16)
args = ap.parse_args()

tables = compile_from_synth(synth.make_synth("linear", years=list(range(2006, 2017)), n_samples=100, seed=0,
                                             extra_confounder_fips=60))  # bench.py's configs[2]
B, G = args.budget, args.groups


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
    # (fixes={"budget"}: a later reset(budget=b) takes b instead of the first reset's sticky budget; the same kernels)
    twin = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled", fixes={"budget"})
    env.reset(seed=0)
    rng = np.random.default_rng(1)
    W = (rng.standard_normal((G, tables.n_obs)) * 0.4).astype(np.float32)
    W[:, tables.feature_names.index("remaining_budget")] = np.float32(0.15)
    pol = dict(kind="linear", weight=torch.as_tensor(W, device=env.device),
               bias=torch.as_tensor((rng.standard_normal(G) * 0.5).astype(np.float32), device=env.device),
               group=torch.as_tensor(rng.integers(0, G, n), device=env.device), sample=True, seed=3)

    def one_rollout():
        twin.reset(seed=0)  # outside the timed region
        return once(lambda: twin.rollout(pol)["return"])

    def sweep():
        def run():
            out = []
            for b in range(B + 1):
                twin.reset(seed=0, options={"budget": b})
                out.append(twin.rollout(pol)["return"])
            return out
        return once(run)

    calls = {"rollout": one_rollout,
             "curve": lambda: once(lambda: env.policy_budget_curve(pol, B)),
             "curve_schedules": lambda: once(lambda: env.policy_budget_curve(pol, B, schedules=True, packed=True)),
             "sweep": sweep}
    times = {k: [] for k in calls}
    check = None
    for i in range(args.reps + 1):  # the first round warms every call up
        for k, fn in calls.items():
            ms, out = fn()
            if i == 0 and k == "curve":
                check = out["return"].clone()
            if i == 0 and k == "sweep":  # the two routes agree bit for bit
                same = all(torch.equal(check[:, b].contiguous().view(torch.int32), out[b].view(torch.int32))
                           for b in range(B + 1))
            del out
            if i:
                times[k].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    row = {"envs": n, "days": tables.T, "max_budget": B, "reps": args.reps, "curve_equals_sweep_bits": same}
    for k, v in times.items():
        row[k + "_ms"] = round(med[k], 3)
        row[k + "_spread_ms"] = round(max(v) - min(v), 3)
    row["curve_over_one_rollout"] = round(med["curve"] / med["rollout"], 3)
    row["curve_schedules_over_one_rollout"] = round(med["curve_schedules"] / med["rollout"], 3)
    row["sweep_over_curve"] = round(med["sweep"] / med["curve"], 3)
    row["sweep_over_curve_schedules"] = round(med["sweep"] / med["curve_schedules"], 3)
    print(json.dumps(row), flush=True)
    env.close()
    twin.close()
    del env, twin, pol, check
    torch.cuda.empty_cache()
