#!/usr/bin/env python3
"""Cross-entropy-method search over [16]-tanh MLP alert policies, scored inside the rollout kernel: G = 256 candidate
networks, each evaluated on its own 4096 envs per iteration (one rollout(kind="mlp") launch for all of them), the elite
fraction refits the sampling distribution over the flattened parameters. Prints the elite mean return per iteration
next to the built-in `never` and `threshold` policies on the same batch.

    python examples/mlp_policy_search.py            # needs one ROCm GPU
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, synth

data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=20, seed=0, extra_confounder_fips=6)
tables = compile_from_synth(data)
G, per, iters, elite, H = 256, 4096, 12, 26, 16
n = G * per
env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True)  # lock step: every rollout is a fresh episode
env.reset(seed=0)
group = torch.arange(n, device=env.device, dtype=torch.int32) // per
k = tables.n_obs
# the observation columns differ in scale by orders of magnitude: the first layer works in units of each column's spread
scale = env._obs.std(dim=0).clamp_min(0.1).cpu().numpy().astype(np.float64)
sizes = [H * k, H, H, 1]  # W1, b1, w_out, b_out
rng = np.random.default_rng(0)
mu, sd = np.zeros(sum(sizes)), np.full(sum(sizes), 0.5)
mu[-1] = -1.0  # start near "rarely alert"


def unpack(theta):
    W1, b1, wo, bo = np.split(theta, np.cumsum(sizes)[:-1], axis=1)
    W1 = W1.reshape(G, H, k) / np.sqrt(k) / scale[None, None, :]
    return [(W1.astype(np.float32), b1.astype(np.float32)), (wo.reshape(G, 1, H).astype(np.float32), bo.astype(np.float32))]


never = float(env.rollout({"kind": "never"})["return"].mean())
thr = float(env.rollout({"kind": "threshold", "feature": "heat_qi", "threshold": 0.9, "require_budget": True})["return"].mean())
print(f"never     {never:9.3f}")
print(f"threshold {thr:9.3f}   (heat_qi > 0.9 while budget is left)")
for it in range(iters):
    theta = mu + sd * rng.standard_normal((G, mu.size))
    out = env.rollout({"kind": "mlp", "layers": unpack(theta), "activation": "tanh", "group": group,
                       "require_budget": True})
    score = out["group_mean_return"].cpu().numpy()
    top = np.argsort(score)[-elite:]
    mu, sd = theta[top].mean(axis=0), theta[top].std(axis=0) + 0.02
    print(f"iter {it:2d}   elite mean return {score[top].mean():9.3f}   best {score[top[-1]]:9.3f}   "
          f"alerts/env {float(out['alerts'].float().mean()):5.2f}")
env.close()
