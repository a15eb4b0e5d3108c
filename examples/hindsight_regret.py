#!/usr/bin/env python3
"""How far from the best possible schedule is a policy? One batch of episodes (the same reset for every policy), the
hindsight optimum of every env -- the best alert schedule for its summer's weather, its own posterior draw and its
budget -- and the regret (optimum minus return) of `never`, `threshold` and a small CEM-tuned linear policy: overall,
and per group of envs with similar budgets.

    python examples/hindsight_regret.py            # needs one ROCm GPU
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, synth

data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=100, seed=0, extra_confounder_fips=6)
tables = compile_from_synth(data)
n = 1 << 16
env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
k = tables.n_obs

# a short CEM search (G candidates on their own envs)
G, iters, elite = 64, 6, 8
env.reset(seed=0)
scale = env._obs.std(dim=0).clamp_min(0.1).cpu().numpy().astype(np.float64)
cand = torch.arange(n, device=env.device, dtype=torch.int32) // (n // G)
rng = np.random.default_rng(0)
mu, sd = np.zeros(k + 1), np.ones(k + 1)
mu[k] = -1.0
for it in range(iters):
    env.reset(seed=1 + it)
    theta = mu + sd * rng.standard_normal((G, k + 1))
    out = env.rollout({"kind": "linear", "weight": (theta[:, :k] / scale).astype(np.float32),
                       "bias": theta[:, k].astype(np.float32), "group": cand, "require_budget": True})
    top = np.argsort(out["group_mean_return"].cpu().numpy())[-elite:]
    mu, sd = theta[top].mean(axis=0), theta[top].std(axis=0) + 0.05

# every policy on the same episodes; the optimum comes from the same start state in the same call. The linear policy's
# envs are grouped by budget band (the same parameters in every group), so "group_hindsight_return" is per band.
env.reset(seed=123)
budget = env.state()["budget"].cpu().numpy()
edges = [0, 5, 9, 13, 1 << 30]
band = np.searchsorted(edges, budget, side="right") - 1
names = [f"budget {edges[i]}-{edges[i + 1] - 1}" if edges[i + 1] < 1 << 30 else f"budget {edges[i]}+"
         for i in range(len(edges) - 1)]
B = len(names)
learned = {"kind": "linear", "weight": np.repeat((mu[None, :k] / scale).astype(np.float32), B, 0),
           "bias": np.full(B, mu[k], np.float32), "group": band, "require_budget": True}
policies = {"never": {"kind": "never"},
            "threshold": {"kind": "threshold", "feature": "heat_qi", "threshold": 0.9, "require_budget": True},
            "cem linear": learned}
print(f"{n} episodes; regret = hindsight optimum - return, mean per episode; envs per band "
      f"{[int((band == b).sum()) for b in range(B)]}")
print(f"{'policy':12s} {'return':>9s} {'optimum':>9s} {'regret':>8s}  " + "".join(f"{s:>14s}" for s in names))
for name, pol in policies.items():
    env.reset(seed=123)
    out = env.rollout(pol, hindsight=True)
    ret = out["return"].double().cpu().numpy()
    opt = out["hindsight_return"].double().cpu().numpy()
    reg = opt - ret
    assert (reg >= -2e-6 * np.abs(ret)).all()
    per = "".join(f"{reg[band == b].mean() if (band == b).any() else float('nan'):14.3f}" for b in range(B))
    print(f"{name:12s} {ret.mean():9.3f} {opt.mean():9.3f} {reg.mean():8.3f}  {per}")
    if "group_hindsight_return" in out:
        gh = out["group_hindsight_return"].double().cpu().numpy()
        ref = [opt[band == b].mean() if (band == b).any() else np.nan for b in range(B)]
        assert np.allclose(gh, ref, rtol=1e-6, equal_nan=True)
env.close()
