#!/usr/bin/env python3
"""Gradient ascent on one linear-logistic alert policy, entirely on the device: rollout(policy_gradient="no_alert")
returns the reward-to-go score-function gradient of the batch's mean return next to the returns themselves, Adam takes
the step, and every few iterations the current parameters are evaluated greedily (sample=False) on a FIXED set of
episodes, next to the threshold policy and the hindsight optimum of the same episodes.

Parameters live in standardised coordinates (each observation column divided by its spread on a reset batch), start at
zero, and the policy never attempts an alert without budget (require_budget). What this shows on the synthetic tables
is printed as it is: the synthetic coefficients were not built to reward learning, so the gap the policy closes between
`never alert` and the hindsight optimum is whatever it is -- the point is the loop evaluate -> improve -> evaluate
without an observation row leaving the kernel.

    python examples/linear_policy_gradient.py [--iters 60] [--envs 65536]      # needs one ROCm GPU
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, synth

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=60)
ap.add_argument("--envs", type=int, default=1 << 16)
ap.add_argument("--lr", type=float, default=0.05)
ap.add_argument("--eval-every", type=int, default=10)
args = ap.parse_args()

data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=100, seed=0, extra_confounder_fips=6)
tables = compile_from_synth(data)
n, k = args.envs, tables.n_obs
env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
EVAL_SEED = 123

env.reset(seed=0)
scale = env._obs.std(dim=0).clamp_min(0.1)  # [n_obs]: the policy's weights are theta / scale

theta = torch.zeros(k + 1, device=env.device, requires_grad=True)  # standardised weights, bias last
opt = torch.optim.Adam([theta], lr=args.lr)


def as_policy(sample, seed=0):
    th = theta.detach()
    return {"kind": "linear", "weight": (th[:k] / scale)[None, :], "bias": th[k:], "sample": sample, "seed": seed,
            "require_budget": True}


def evaluate():
    env.reset(seed=EVAL_SEED)
    return float(env.rollout(as_policy(False))["return"].double().mean())


env.reset(seed=EVAL_SEED)
base = env.rollout({"kind": "never"}, hindsight=True)
never, best = float(base["return"].double().mean()), float(base["hindsight_return"].double().mean())
env.reset(seed=EVAL_SEED)
thr = float(env.rollout({"kind": "threshold", "feature": "heat_qi", "threshold": 0.9, "require_budget": True})
            ["return"].double().mean())
print(f"{n} fixed evaluation episodes: never {never:.3f}   threshold(heat_qi > 0.9) {thr:.3f}   hindsight optimum {best:.3f}")
print(f"{'iter':>5s} {'train return (sampled)':>24s} {'|grad|':>10s} {'eval return (greedy)':>22s} {'gap closed':>11s}")
for it in range(args.iters + 1):
    ev = ""
    if it % args.eval_every == 0:
        r = evaluate()
        ev = f"{r:22.3f} {100.0 * (r - never) / (best - never):10.1f}%"
    if it == args.iters:
        print(f"{it:5d} {'':>24s} {'':>10s} {ev}")
        break
    env.reset(seed=1000 + it)  # fresh training episodes every iteration
    out = env.rollout(as_policy(True, seed=it), policy_gradient="no_alert")
    g = out["policy_gradient"]
    # d return / d theta = (d return / d weight) / scale; Adam minimises, so the ascent direction goes in negated
    grad = torch.cat([g["weight"][0] / scale, g["bias"]])
    opt.zero_grad()
    theta.grad = -grad
    opt.step()
    print(f"{it:5d} {float(out['return'].double().mean()):24.3f} {float(grad.norm()):10.3e} {ev}")
env.close()
