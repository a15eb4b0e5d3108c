#!/usr/bin/env python3
"""Cross-entropy-method search over linear alert policies, scored inside the rollout kernel: G = 256 candidate parameter
vectors, each evaluated on its own 4096 envs per iteration (one rollout(kind="linear") launch for all of them), the
elite fraction refits the sampling distribution. Prints the elite mean return per iteration next to the built-in
`never` and `threshold` policies on the same batch.

    python examples/linear_policy_search.py            # needs one ROCm GPU
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, synth

data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=20, seed=0, extra_confounder_fips=6)
tables = compile_from_synth(data)
G, per, iters, elite = 256, 4096, 12, 26
n = G * per
env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True)  # lock step: every rollout is a fresh episode
env.reset(seed=0)
group = torch.arange(n, device=env.device, dtype=torch.int32) // per
k = tables.n_obs
# the observation columns differ in scale by orders of magnitude: search in units of each column's spread
obs = env._obs
scale = obs.std(dim=0).clamp_min(0.1).cpu().numpy().astype(np.float64)
rng = np.random.default_rng(0)
mu, sd = np.zeros(k + 1), np.ones(k + 1)
mu[k] = -1.0  # start near "rarely alert"

never = float(env.rollout({"kind": "never"})["return"].mean())
thr = float(env.rollout({"kind": "threshold", "feature": "heat_qi", "threshold": 0.9, "require_budget": True})["return"].mean())
print(f"never     {never:9.3f}")
print(f"threshold {thr:9.3f}   (heat_qi > 0.9 while budget is left)")
for it in range(iters):
    theta = mu + sd * rng.standard_normal((G, k + 1))
    W = (theta[:, :k] / scale).astype(np.float32)
    b = theta[:, k].astype(np.float32)
    out = env.rollout({"kind": "linear", "weight": W, "bias": b, "group": group, "require_budget": True})
    score = out["group_mean_return"].cpu().numpy()
    top = np.argsort(score)[-elite:]
    mu, sd = theta[top].mean(axis=0), theta[top].std(axis=0) + 0.05
    print(f"iter {it:2d}   elite mean return {score[top].mean():9.3f}   best {score[top[-1]]:9.3f}   "
          f"alerts/env {float(out['alerts'].float().mean()):5.2f}")
env.close()
