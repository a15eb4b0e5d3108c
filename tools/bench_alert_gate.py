#!/usr/bin/env python3
"""Time the gated linear-kind calls next to their ungated forms (HIP events, median of --reps after a warm-up), and
alert_gate() itself. One JSON line per call.

    python tools/bench_alert_gate.py [--envs 1048576] [--reps 7]      # needs one ROCm GPU
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
ap.add_argument("--envs", type=int, default=1 << 20)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()

tables = compile_from_synth(synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=20, seed=0,
                                             extra_confounder_fips=6))
n = args.envs
env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
rng = np.random.default_rng(0)
W = (rng.standard_normal((1, tables.n_obs)) * 0.3).astype(np.float32)
pol = dict(kind="linear", weight=W, bias=np.zeros(1, np.float32), sample=True, seed=1)


def timed(fn, reset=True):
    ms = []
    for i in range(args.reps + 1):
        if reset:
            env.reset(seed=0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), max(ms) - min(ms)


env.reset(seed=0)
allowed = env.alert_gate("heat_qi", 0.8)
sched = torch.as_tensor(rng.random((n, tables.T)) < 0.2, device=env.device)
gated = dict(pol, allowed_days=allowed)
gated_p = dict(pol, allowed_days=env.alert_gate("heat_qi", 0.8, packed=True))  # int32 words: nothing is packed per call
rows = [("alert_gate", lambda: env.alert_gate("heat_qi", 0.8), False),
        ("rollout", lambda: env.rollout(pol), True), ("rollout gated", lambda: env.rollout(gated), True),
        ("rollout gated, packed mask", lambda: env.rollout(gated_p), True),
        ("imitation_gradient", lambda: env.imitation_gradient(pol, sched), False),
        ("imitation_gradient gated", lambda: env.imitation_gradient(gated, sched), False),
        ("imitation_gradient gated, packed mask", lambda: env.imitation_gradient(gated_p, sched), False)]
for name, fn, reset in rows:
    med, spread = timed(fn, reset)
    print(json.dumps({"call": name, "envs": n, "days": tables.T, "median_ms": round(med, 3), "spread_ms": round(spread, 3),
                      "note": "host side included (packing the mask, allocating outputs)"}))
env.close()
