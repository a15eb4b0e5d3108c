#!/usr/bin/env python3
"""PPO on ONE network with a shared trunk -- Linear, Tanh, Linear, Tanh, Linear with two outputs: row 0 the policy
logit, row 1 the state value (older SB3 net_arch=[64, 64], most small PPO codes) -- with every pass over the experience
inside the kernels and no observation row recorded. Per iteration:
  1. collection: reset(seed) and rollout(actor | {"sample": True}, alert_mask=True), the actor being the trunk and row 0;
     the episodes are then regenerated from the seed.
  2. collect call: actor_critic_gradient(net, alert_days, gamma=, gae_lambda=, gradient=False) forms the rewards, the
     GAE(lambda) advantages and targets from the net's own value row and the log-probabilities -- the cheap first pass.
  3. K epochs: actor_critic_gradient(net, alert_days, advantage=normalised, value_target=, old_log_prob=) returns the
     ascent direction of clip + entropy - value loss in one row rebuild, one forward and one backward per env-day;
     policy.mlp_heads_grad_to_module writes it into the torch module's .grad and Adam steps.
The value loss carries the factor 1/2, so SB3's vf_coef = 0.5 is --vf-coef 1.0 here.

    python examples/ppo_shared_trunk.py [--iters 30] [--num-envs 16384]      # needs one ROCm GPU
    python examples/ppo_shared_trunk.py --num-envs 1024 --iters 6          # seconds
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
from torch import nn

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, policy, synth

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--num-envs", type=int, default=1 << 14)
ap.add_argument("--epochs", type=int, default=4)
ap.add_argument("--gamma", type=float, default=0.99)
ap.add_argument("--gae-lambda", type=float, default=0.95)
ap.add_argument("--clip", type=float, default=0.2)
ap.add_argument("--vf-coef", type=float, default=1.0)
ap.add_argument("--entropy-coef", type=float, default=0.0)
ap.add_argument("--lr", type=float, default=3e-4)
args = ap.parse_args()

data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=20, seed=0, extra_confounder_fips=6)
tables = compile_from_synth(data)
n, k = args.num_envs, tables.n_obs
env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
obs0, _ = env.reset(seed=0)
scale = obs0.std(dim=0).clamp_min(0.1).cpu()
torch.manual_seed(0)

net = nn.Sequential(nn.Linear(k, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 2))
with torch.no_grad():
    net[0].weight /= scale[None, :]  # the raw columns, divided by their spread
    net[4].weight *= 0.01
    net[4].bias[0] = -2.0  # few alerts to start with
opt = torch.optim.Adam(net.parameters(), lr=args.lr)


def both_rows():
    return policy.mlp_from_module(net) | {"require_budget": True}


def actor(**kw):
    """the trunk and row 0 alone: what rollout() samples from"""
    pol = both_rows()
    Wo, bo = pol["layers"][-1]
    pol["layers"][-1] = (Wo[:1], bo[:1])
    return pol | kw


for it in range(args.iters):
    seed = 1000 + it
    env.reset(seed=seed)
    out = env.rollout(actor(sample=True, seed=seed), alert_mask=True)
    sched, ret = out["alert_days"], float(out["return"].mean())
    env.reset(seed=seed)  # the same episodes again: the calls below force them along the schedule
    col = env.actor_critic_gradient(both_rows(), sched, gamma=args.gamma, gae_lambda=args.gae_lambda, gradient=False)
    adv, days = col["advantage"], float(col["days"].sum())
    scored = col["log_prob"] != 0
    adv_n = torch.where(scored, (adv - adv[scored].mean()) / (adv[scored].std() + 1e-8), torch.zeros_like(adv))
    for _ in range(args.epochs):
        ep = env.actor_critic_gradient(both_rows(), sched, advantage=adv_n, value_target=col["value_target"],
                                       old_log_prob=col["log_prob"], clip=args.clip, vf_coef=args.vf_coef,
                                       entropy_coef=args.entropy_coef)
        policy.mlp_heads_grad_to_module(net, ep["gradient"])  # the negated ascent direction: Adam descends -J
        for p in net.parameters():  # the kernels sum over an env's days: per transition, as SB3's mean over a batch
            p.grad *= n / days
        torch.nn.utils.clip_grad_norm_(net.parameters(), 0.5)
        opt.step()
        opt.zero_grad()
    print(f"iter {it:3d}  return of the sampled rollout {ret:9.4f}  value loss per day {float(ep['value_loss'].sum()) / days:.5f}  "
          f"approx_kl per day {float(ep['approx_kl'].sum()) / days:.2e}  clipped {float(ep['clipped_days'].sum()) / days:.3f}  "
          f"entropy per day {float(ep['entropy'].sum()) / days:.3f}")
env.close()
