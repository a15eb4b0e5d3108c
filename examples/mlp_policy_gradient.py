#!/usr/bin/env python3
"""The twin of examples/linear_policy_gradient.py with a [16] tanh actor: a torch.nn.Sequential is handed to the kernel
with policy.mlp_from_module, rollout(policy_gradient="no_alert") returns the reward-to-go score-function gradient of the
batch's mean return with respect to every weight and bias (backpropagated inside the kernel, no observation row leaves
it), policy.mlp_grad_to_module writes it into the module's .grad, and torch Adam takes the step. Same envs, iterations
and evaluation as the linear example: every few iterations the current network is evaluated greedily (sample=False) on
a FIXED set of episodes, next to never alerting, the threshold policy and the hindsight optimum of the same episodes.

The observation columns are standardised by a fixed first Linear-free step: each column's spread on a reset batch is
folded into the first layer's weights when the policy dict is built, so the module itself sees standardised inputs. What
the learned network reaches on the synthetic tables is printed as it is.

    python examples/mlp_policy_gradient.py [--iters 60] [--envs 65536]      # needs one ROCm GPU
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, policy, synth

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=60)
ap.add_argument("--envs", type=int, default=1 << 16)
ap.add_argument("--lr", type=float, default=0.02)
ap.add_argument("--eval-every", type=int, default=10)
args = ap.parse_args()

data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=100, seed=0, extra_confounder_fips=6)
tables = compile_from_synth(data)
n, k = args.envs, tables.n_obs
env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
EVAL_SEED = 123

obs0, _ = env.reset(seed=0)
scale = obs0.std(dim=0).clamp_min(0.1).cpu()  # [n_obs]: the module acts on obs / scale

torch.manual_seed(0)
actor = torch.nn.Sequential(torch.nn.Linear(k, 16), torch.nn.Tanh(), torch.nn.Linear(16, 1))
with torch.no_grad():  # start near "never alert", like the linear example's zero logit but with the budget in mind
    actor[2].weight.mul_(0.1)
    actor[2].bias.zero_()
opt = torch.optim.Adam(actor.parameters(), lr=args.lr)


def as_policy(sample, seed=0):
    pol = policy.mlp_from_module(actor)
    W1, b1 = pol["layers"][0]
    pol["layers"][0] = (W1 / scale[None, :], b1)  # the kernel's first layer acts on the raw columns
    pol.update(sample=sample, seed=seed, require_budget=True)
    return pol


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
r = never
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
    g = {"layers": [(dW.cpu(), db.cpu()) for dW, db in out["policy_gradient"]["layers"]]}
    # d return / d (module's first weight) = (d return / d (kernel's first weight)) / scale
    g["layers"][0] = (g["layers"][0][0] / scale[None, None, :], g["layers"][0][1])
    opt.zero_grad()
    policy.mlp_grad_to_module(actor, g, group=0, ascent=True)  # negated: Adam's step ascends the return
    gn = float(torch.sqrt(sum((p.grad ** 2).sum() for p in actor.parameters())))
    opt.step()
    print(f"{it:5d} {float(out['return'].double().mean()):24.3f} {gn:10.3e} {ev}")
print(f"never {never:.3f}   threshold {thr:.3f}   hindsight optimum {best:.3f}   learned [16] tanh {r:.3f}")
env.close()
