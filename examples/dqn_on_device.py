#!/usr/bin/env python3
"""Double-DQN with every pass over the experience inside the kernels and a replay buffer that stores no observation:
an episode is regenerated from its seed, and the env can be forced along a schedule, so a transition batch is a
(reset seed, alert_days bitmap) pair -- 1 bit per env-day. Per iteration:
  1. collection: reset(seed) and rollout(q | {"sample": True}, alert_mask=True). rollout() folds the two action values
     into sigmoid(Q1 - Q0), so sampling it is Boltzmann exploration over the two actions; the output layer is divided
     by the temperature for the call. The pair (seed, the alerts the rollout issued) goes into the buffer.
  2. replay: for a few pairs drawn from the buffer, a twin env is reset to the pair's seed -- the same episodes -- and
     q_gradient(q, alert_days, target_net, double=True) returns the TD semi-gradient of the [64, 64] Q-net in the net's
     own shapes; policy.mlp_heads_grad_to_module writes it into the torch module's .grad and Adam steps.
  3. every --target-every updates the target net is a copy of the online net.
The Q-net is SB3-shaped (model.q_net.q_net: Linear, ReLU, Linear, ReLU, Linear with two outputs), so the same loop
trains an SB3 DQN's network in place. "require_budget" masks the next state's max once the budget is spent.

    python examples/dqn_on_device.py [--iters 30] [--num-envs 16384]      # needs one ROCm GPU
    python examples/dqn_on_device.py --num-envs 1024 --iters 6          # seconds
"""
import argparse
import copy
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
from torch import nn

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, policy, synth

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--num-envs", type=int, default=1 << 14)
ap.add_argument("--replays", type=int, default=2, help="buffer entries replayed per iteration")
ap.add_argument("--buffer", type=int, default=16, help="(seed, schedule) pairs kept")
ap.add_argument("--target-every", type=int, default=8, help="updates between copies into the target net")
ap.add_argument("--gamma", type=float, default=0.99)
ap.add_argument("--lr", type=float, default=1e-3)
ap.add_argument("--temperature", type=float, default=0.05, help="of the Boltzmann exploration, in units of return")
args = ap.parse_args()

data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=20, seed=0, extra_confounder_fips=6)
tables = compile_from_synth(data)
n, k = args.num_envs, tables.n_obs
env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
twin = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
obs0, _ = env.reset(seed=0)
scale = obs0.std(dim=0).clamp_min(0.1).cpu()
torch.manual_seed(0)
random.seed(0)

q_net = nn.Sequential(nn.Linear(k, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 2))
with torch.no_grad():
    q_net[0].weight /= scale[None, :]  # the raw columns, divided by their spread
    q_net[4].weight *= 0.01
target_net = copy.deepcopy(q_net)
opt = torch.optim.Adam(q_net.parameters(), lr=args.lr)


def as_dict(module, **kw):
    return policy.mlp_from_module(module) | {"require_budget": True} | kw


def behaviour(module, seed):
    """the collecting policy: P(alert) = sigmoid((Q1 - Q0) / temperature), by scaling the output layer"""
    pol = as_dict(module, sample=True, seed=seed)
    Wo, bo = pol["layers"][-1]
    pol["layers"][-1] = (Wo / args.temperature, bo / args.temperature)
    return pol


buffer, updates = [], 0
for it in range(args.iters):
    # 1. collect one batch of episodes with the current net; keep (seed, attempted alerts)
    seed = 1000 + it
    env.reset(seed=seed)
    out = env.rollout(behaviour(q_net, seed), alert_mask=True)
    buffer.append((seed, out["alert_days"]))  # with require_budget every attempt is issued: attempts = alerts
    buffer = buffer[-args.buffer:]
    ret = float(out["return"].mean())
    # greedy evaluation on the same episodes: alert iff Q1 > Q0
    env.reset(seed=seed)
    greedy = float(env.rollout(as_dict(q_net))["return"].mean())
    # 2. replay: regenerate the episodes of a stored pair on the twin and take the TD semi-gradient along its schedule
    loss = 0.0
    for s_seed, sched in random.sample(buffer, min(args.replays, len(buffer))):
        twin.reset(seed=s_seed)
        td = twin.q_gradient(as_dict(q_net), sched, target_net=as_dict(target_net), gamma=args.gamma, double=True)
        policy.mlp_heads_grad_to_module(q_net, td["q_gradient"])  # the negated gradient: Adam descends the TD loss
        days = float(td["days"].sum())
        for p in q_net.parameters():  # the kernels sum over an env's days: per transition, as SB3's mean over a batch
            p.grad *= n / days
        torch.nn.utils.clip_grad_norm_(q_net.parameters(), 10.0)
        opt.step()
        opt.zero_grad()
        loss = float(td["loss"].sum()) / days
        updates += 1
        # 3. periodic copy into the target net
        if updates % args.target_every == 0:
            target_net.load_state_dict(q_net.state_dict())
    print(f"iter {it:3d}  return of the exploring rollout {ret:9.4f}  greedy {greedy:9.4f}  "
          f"Huber TD loss per transition {loss:.5f}  buffer {len(buffer)} x {n} episodes "
          f"({len(buffer) * n * tables.T // 8} B of schedules)")
env.close()
twin.close()
