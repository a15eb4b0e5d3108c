#!/usr/bin/env python3
"""Time hindsight_values() next to hindsight_optimum(), and imitation_gradient(labels=...) next to the call without
labels, in one process on bench.py's configs[2] tables: HIP events around whole calls (host side included: the packed
schedule is passed as int32 words, so nothing is packed per call), one warm-up, the pair's calls interleaved
(A B A B ...), median and spread of --reps. One JSON line per pair, with the ratio of the medians.

    python tools/bench_hindsight_values.py [--envs 1048576] [--reps 7]      # needs one ROCm GPU
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, policy, synth

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=1 << 20)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()

tables = compile_from_synth(synth.make_synth("linear", years=list(range(2006, 2017)), n_samples=100, seed=0,
                                             extra_confounder_fips=60))  # bench.py's configs[2]
n = args.envs
env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
env.reset(seed=0)
st0 = {k: v.clone() for k, v in env.state().items()}
words = (tables.T + 31) // 32
gen = torch.Generator(device=env.device).manual_seed(0)
sched = policy.pack_alert_days(torch.rand((n, tables.T), generator=gen, device=env.device) < 0.1, words)


def once(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def pair(name, a_name, fa, b_name, fb):
    ta, tb = [], []
    for i in range(args.reps + 1):  # the first round warms both up
        ma, mb = once(fa)[0], once(fb)[0]
        if i:
            ta.append(ma)
            tb.append(mb)
    a, b = statistics.median(ta), statistics.median(tb)
    print(json.dumps({"pair": name, "envs": n, "days": tables.T, a_name + "_ms": round(a, 3),
                      a_name + "_spread_ms": round(max(ta) - min(ta), 3), b_name + "_ms": round(b, 3),
                      b_name + "_spread_ms": round(max(tb) - min(tb), 3), "ratio": round(b / a, 3), "reps": args.reps}))


pair("hindsight", "hindsight_optimum", lambda: env.hindsight_optimum(st0),
     "hindsight_values", lambda: env.hindsight_values(sched, start_state=st0))
pair("hindsight, value and loss", "hindsight_optimum", lambda: env.hindsight_optimum(st0),
     "hindsight_values", lambda: env.hindsight_values(sched, start_state=st0, value=True, loss=True))
labels = policy.pack_alert_days(env.hindsight_values(sched, start_state=st0)["expert_alert_days"], words)
sched_b = policy.unpack_alert_days(sched, tables.T)  # imitation_gradient() takes the schedule as bool [N, T]
rng = np.random.default_rng(0)
W = (rng.standard_normal((1, tables.n_obs)) * 0.3).astype(np.float32)
lin = dict(kind="linear", weight=W, bias=np.zeros(1, np.float32))
dims = [tables.n_obs, 64, 64, 1]
mlp = dict(kind="mlp", activation="tanh",
           layers=[((rng.standard_normal((1, dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32),
                    np.zeros((1, dims[i + 1]), np.float32)) for i in range(3)])
for kind, pol in (("linear", lin), ("mlp 64x64", mlp)):
    pair(f"imitation_gradient, {kind}", "plain", lambda: env.imitation_gradient(pol, sched_b),
         "labels", lambda: env.imitation_gradient(pol, sched_b, labels=labels))
env.close()
