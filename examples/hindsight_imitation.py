#!/usr/bin/env python3
"""Behaviour cloning of the hindsight optimum, all inside the kernels: hindsight_optimum() gives every env's best alert
schedule, imitation_gradient() the gradient of that schedule's log-likelihood under a [16] tanh actor (the env is forced
along the schedule and the actor evaluated on the rows it would have held -- no observation row leaves the kernel),
policy.mlp_grad_to_module writes it into the module's .grad, and torch Adam takes the step. The call changes neither
the env nor the RNG, so every epoch runs on the same episodes without a reset in between. Before, during and after,
the actor's regret against the hindsight optimum on a FIXED set of evaluation episodes, rollout(pol, hindsight=True):
sampled as it was fitted (alert with probability sigmoid(logit)) and greedy (alert iff logit > 0; the expert alerts on
about one day in twenty, so a greedy clone alerts only where it has become confident). What the clone reaches on the
synthetic tables is printed as it is: there the likelihood rises steadily while the regret does not fall --
a one-row-at-a-time clone of a schedule chosen with knowledge of the whole season learns its base rate first.

    python examples/hindsight_imitation.py [--epochs 40] [--envs 65536]      # needs one ROCm GPU
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, policy, synth

ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=40)
ap.add_argument("--envs", type=int, default=1 << 16)
ap.add_argument("--lr", type=float, default=0.02)
ap.add_argument("--eval-every", type=int, default=10)
args = ap.parse_args()

data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=100, seed=0, extra_confounder_fips=6)
tables = compile_from_synth(data)
n, k = args.envs, tables.n_obs
train = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
evals = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled", env_gid0=n)

obs0, _ = train.reset(seed=0)
scale = obs0.std(dim=0).clamp_min(0.1).cpu()  # [n_obs]: the module acts on obs / scale

torch.manual_seed(0)
actor = torch.nn.Sequential(torch.nn.Linear(k, 16), torch.nn.Tanh(), torch.nn.Linear(16, 1))
opt = torch.optim.Adam(actor.parameters(), lr=args.lr)


def as_policy(sample=False):
    pol = policy.mlp_from_module(actor)
    W1, b1 = pol["layers"][0]
    pol["layers"][0] = (W1 / scale[None, :], b1)  # the kernel's first layer acts on the raw columns
    pol.update(require_budget=True, sample=sample, seed=7)
    return pol


def regret():
    """(sampled, greedy): the clone as it was fitted (alert with probability sigmoid(logit)), and alert iff logit > 0"""
    res = []
    for sample in (True, False):
        evals.reset(seed=123)
        out = evals.rollout(as_policy(sample), hindsight=True)
        res.append(float((out["hindsight_return"].double() - out["return"].double()).mean()))
    return tuple(res)


expert = train.hindsight_optimum()
print(f"{n} training episodes, {float(expert['alerts'].double().mean()):.2f} expert alerts per episode; "
      f"regret on {n} other episodes:")
print(f"{'epoch':>5s} {'mean log-likelihood / day':>26s} {'|grad|':>10s} {'regret (sampled)':>17s} {'regret (greedy)':>16s}")
first = last = regret()
for ep in range(args.epochs + 1):
    ev = ""
    if ep % args.eval_every == 0:
        last = regret()
        ev = f"{last[0]:17.4f} {last[1]:16.4f}"
    if ep == args.epochs:
        print(f"{ep:5d} {'':>26s} {'':>10s} {ev}")
        break
    out = train.imitation_gradient(as_policy(), expert["alert_days"])  # the same episodes every epoch: no reset
    g = {"layers": [(dW.cpu(), db.cpu()) for dW, db in out["policy_gradient"]["layers"]]}
    # d ll / d (module's first weight) = (d ll / d (kernel's first weight)) / scale
    g["layers"][0] = (g["layers"][0][0] / scale[None, None, :], g["layers"][0][1])
    opt.zero_grad()
    policy.mlp_grad_to_module(actor, g, group=0, ascent=True)  # negated: Adam's step ascends the likelihood
    gn = float(torch.sqrt(sum((p.grad ** 2).sum() for p in actor.parameters())))
    opt.step()
    per_day = float(out["log_likelihood"].double().sum() / out["days"].double().sum().clamp_min(1))
    print(f"{ep:5d} {per_day:26.4f} {gn:10.3e} {ev}")
print(f"regret of the [16] tanh actor, sampled: {first[0]:.4f} before, {last[0]:.4f} after {args.epochs} epochs "
      f"(greedy: {first[1]:.4f} before, {last[1]:.4f} after)")
train.close()
evals.close()
