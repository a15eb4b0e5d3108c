#!/usr/bin/env python3
"""DAgger / hindsight relabelling without leaving the device, next to plain behaviour cloning.

Behaviour cloning fits the policy to the hindsight optimum's own schedule: it only ever sees the states the expert
visits. DAgger runs the learner, asks the expert what it would have done in the states the LEARNER reached
(hindsight_values()["expert_alert_days"]) and fits to those labels along the learner's own schedule
(imitation_gradient(labels=...)). Both take one Adam step per iteration on the same episodes; the table shows the
learner's mean regret per episode (hindsight_values()["regret"] of its own sampled rollout) for each.

    python examples/dagger_on_device.py [--envs 65536] [--iters 30]      # needs one ROCm GPU
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, synth

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=1 << 16)
ap.add_argument("--iters", type=int, default=30)
args = ap.parse_args()

tables = compile_from_synth(synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=100, seed=0,
                                             extra_confounder_fips=6))
n, k = args.envs, tables.n_obs
env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
env.reset(seed=0)
scale = env._obs.std(dim=0).clamp_min(0.1)  # the policy sees standardised columns: W = theta / scale


def learner(name):
    theta = torch.zeros(k, device=env.device, requires_grad=True)
    bias = torch.full((1,), -2.0, device=env.device, requires_grad=True)
    return dict(name=name, theta=theta, bias=bias, opt=torch.optim.Adam([theta, bias], lr=0.05))


def as_policy(L, **kw):
    return dict(kind="linear", weight=(L["theta"].detach() / scale)[None, :].contiguous(), bias=L["bias"].detach(),
                require_budget=True, **kw)


def ascend(L, grad):
    """one Adam step UP the log-likelihood whose gradient the kernel returned (with respect to W = theta / scale)"""
    L["opt"].zero_grad()
    L["theta"].grad = -(grad["weight"][0] / scale)
    L["bias"].grad = -grad["bias"].clone()
    L["opt"].step()


bc, dagger = learner("behaviour cloning"), learner("DAgger")
print(f"{n} episodes per iteration; mean regret per episode of the learner's own sampled rollout")
print(f"{'iter':>4s} {'behaviour cloning':>18s} {'DAgger':>10s} {'label != action (DAgger)':>26s}")
for it in range(args.iters):
    env.reset(seed=1 + it)
    best = env.hindsight_optimum()
    row = []
    for L in (bc, dagger):
        env.reset(seed=1 + it)  # the same episodes for both
        out = env.rollout(as_policy(L, sample=True, seed=100 + it), alert_mask=True)
        env.reset(seed=1 + it)
        hv = env.hindsight_values(out["alert_days"])  # the expert in the learner's states, and the learner's regret
        row.append(float(hv["regret"].double().mean()))
        if L is bc:
            g = env.imitation_gradient(as_policy(L), best["alert_days"])
        else:
            g = env.imitation_gradient(as_policy(L), out["alert_days"], labels=hv["expert_alert_days"])
            differ = float((hv["expert_alert_days"] != out["alert_days"]).double().mean())
        ascend(L, g["policy_gradient"])
    print(f"{it:4d} {row[0]:18.3f} {row[1]:10.3f} {differ:26.4f}")
env.close()
