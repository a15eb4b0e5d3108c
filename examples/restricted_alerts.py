#!/usr/bin/env python3
"""Alerts restricted to hot days, the older reference env's `restrict_alerts` / `HI_restriction`: a threshold sweep as
one launch. G groups of envs share one linear policy; group g may alert only on days whose observed heat_qi is >=
tau_g. alert_gate(threshold=tau[group]) builds the mask, rollout() applies it inside the kernel, and
hindsight_optimum(allowed_days=) gives the best schedule under each restriction next to it.

    python examples/restricted_alerts.py [--envs 65536]      # needs one ROCm GPU
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, policy, synth

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=1 << 16)
args = ap.parse_args()

tables = compile_from_synth(synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=20, seed=0,
                                             extra_confounder_fips=6))
n = args.envs
env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
env.reset(seed=0)
taus = torch.tensor([0.0, 0.5, 0.7, 0.8, 0.9, 0.95], device=env.device)
G = len(taus)
group = torch.arange(n, device=env.device) % G
allowed = env.alert_gate("heat_qi", taus[group])  # bool [N, T]

# one policy for every group: alert when it is hot (the restriction decides how hot it has to be)
W = np.zeros((G, tables.n_obs), np.float32)
W[:, tables.feature_names.index("heat_qi")] = 4.0
pol = dict(kind="linear", weight=W, bias=np.full(G, -1.0, np.float32), group=group, require_budget=True,
           allowed_days=allowed)
best = env.hindsight_optimum(allowed_days=allowed)
out = env.rollout(pol)
best_mean = policy.group_mean(best["return"], group.to(torch.int32), G)
share = policy.group_mean(allowed.float().mean(1), group.to(torch.int32), G)
print(f"envs {n}  days {tables.T}  device {torch.cuda.get_device_name(0)}")
print("  tau   allowed days   mean return   best under the restriction")
for g in range(G):
    print(f"{float(taus[g]):5.2f}   {float(share[g]):12.3f}   {float(out['group_mean_return'][g]):11.3f}   {float(best_mean[g]):11.3f}")
env.close()
