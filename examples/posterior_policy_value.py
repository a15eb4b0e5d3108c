#!/usr/bin/env python3
"""How sure are we that a policy beats the threshold policy, under the reward model's posterior? One batch of episodes
(the same reset for every policy, so all of them face the same counties, years and budgets), three policies -- `never`,
`threshold` and a linear policy from a short cross-entropy search -- each scored with rollout(posterior_returns=True):
the batch mean of every posterior draw's return is one posterior sample of the policy's value. Prints the posterior
mean, the 90 % credible interval, the CVaR over the worst 10 % of draws and P(better than threshold), paired by draw.

    python examples/posterior_policy_value.py            # needs one ROCm GPU
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, stats, synth

data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=100, seed=0, extra_confounder_fips=6)
tables = compile_from_synth(data)
n = 1 << 16
env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
k = tables.n_obs


def evaluate(policy):
    """posterior draws [K] of the batch-mean return: every policy on the same episodes"""
    env.reset(seed=123)
    out = env.rollout(policy, posterior_returns=True)
    return out["posterior_returns"].double().mean(0)


# a short CEM search (G candidates on their own envs, scored by the return under each env's own draw)
G, iters, elite = 64, 6, 8
env.reset(seed=0)
scale = env._obs.std(dim=0).clamp_min(0.1).cpu().numpy().astype(np.float64)
group = torch.arange(n, device=env.device, dtype=torch.int32) // (n // G)
rng = np.random.default_rng(0)
mu, sd = np.zeros(k + 1), np.ones(k + 1)
mu[k] = -1.0
for it in range(iters):
    env.reset(seed=1 + it)
    theta = mu + sd * rng.standard_normal((G, k + 1))
    out = env.rollout({"kind": "linear", "weight": (theta[:, :k] / scale).astype(np.float32),
                       "bias": theta[:, k].astype(np.float32), "group": group, "require_budget": True})
    top = np.argsort(out["group_mean_return"].cpu().numpy())[-elite:]
    mu, sd = theta[top].mean(axis=0), theta[top].std(axis=0) + 0.05
learned = {"kind": "linear", "weight": (mu[None, :k] / scale).astype(np.float32),
           "bias": np.asarray([mu[k]], np.float32), "require_budget": True}

R = {"never": evaluate({"kind": "never"}),
     "threshold": evaluate({"kind": "threshold", "feature": "heat_qi", "threshold": 0.9, "require_budget": True}),
     "cem linear": evaluate(learned)}
print(f"{n} episodes, {tables.n_samples} posterior draws")
print(f"{'policy':12s} {'mean':>9s} {'90% interval':>22s} {'CVaR10%':>9s} {'P(> threshold)':>15s}")
for name, r in R.items():
    s = stats.posterior_summary(r)
    q = s["quantiles"]
    print(f"{name:12s} {float(s['mean']):9.3f}   [{float(q[0]):9.3f}, {float(q[2]):9.3f}] {float(s['cvar']):9.3f} "
          f"{float(stats.prob_better(r, R['threshold'])):15.3f}")
env.close()
