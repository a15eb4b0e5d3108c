#!/usr/bin/env python3
"""Two hindsight experts, one clone each. hindsight_optimum() knows the season's weather AND the env's own posterior
draw; no policy observes the draw, so its labels are partly noise to a learner and its return is a bound no policy
reaches. hindsight_posterior_optimum() knows the weather only: the schedule that is best on average over the draws,
the tight bound, and labels that are functions of what a policy can see.
The loop of examples/hindsight_imitation.py runs twice on the same episodes, once per expert's labels (the same [16]
tanh actor from the same initial weights, imitation_gradient() inside the kernels, torch Adam). Printed: both experts'
posterior-mean returns (the draw-mean of posterior_returns() on their schedules), the share of env-days on which the
labels differ, and each clone's regret on held-out episodes against each yardstick -- posterior-mean returns
throughout, the clone's from rollout(posterior_returns=True). What the clones reach is printed as it is.

    python examples/draw_blind_expert.py [--epochs 40] [--envs 16384]      # needs one ROCm GPU
"""
import argparse
import copy
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, policy, synth

ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=40)
ap.add_argument("--envs", type=int, default=1 << 14)
ap.add_argument("--lr", type=float, default=0.02)
args = ap.parse_args()

data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=100, seed=0, extra_confounder_fips=6)
tables = compile_from_synth(data)
n, k = args.envs, tables.n_obs
train = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
evals = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled", env_gid0=n)

obs0, _ = train.reset(seed=0)
scale = obs0.std(dim=0).clamp_min(0.1).cpu()  # [n_obs]: the modules act on obs / scale
st0 = {key: v.clone() for key, v in train.state().items()}


def mean_return(env, state, alert_days):
    """f64 [N]: the schedule's return averaged over the draws"""
    return env.posterior_returns(state, alert_days).double().mean(1)


own = train.hindsight_optimum(st0)
blind = train.hindsight_posterior_optimum(st0)
experts = {"own draw": own["alert_days"], "draw-blind": blind["alert_days"]}
print(f"{n} training episodes, {train.last_hindsight_posterior_keys} distinct (county, year, column, budget) problems")
for name, days in experts.items():
    print(f"  expert {name:10s}: posterior-mean return {float(mean_return(train, st0, days).mean()):10.4f}, "
          f"{float(days.sum(1).double().mean()):.2f} alerts per episode")
live = torch.arange(tables.T, device=train.device)[None, :] < st0["n_days"][:, None]
print(f"  the labels differ on {float((experts['own draw'] != experts['draw-blind'])[live].double().mean()):.4f} of the "
      f"env-days, on {float((experts['own draw'] != experts['draw-blind']).any(1).double().mean()):.3f} of the episodes")

# the held-out episodes and their two yardsticks, in posterior-mean returns
evals.reset(seed=123)
ev0 = {key: v.clone() for key, v in evals.state().items()}
yard = {"own draw": mean_return(evals, ev0, evals.hindsight_optimum(ev0)["alert_days"]),
        "draw-blind": evals.hindsight_posterior_optimum(ev0)["return"].double()}

torch.manual_seed(0)
init = torch.nn.Sequential(torch.nn.Linear(k, 16), torch.nn.Tanh(), torch.nn.Linear(16, 1))


def as_policy(actor, sample):
    pol = policy.mlp_from_module(actor)
    W1, b1 = pol["layers"][0]
    pol["layers"][0] = (W1 / scale[None, :], b1)  # the kernel's first layer acts on the raw columns
    pol.update(require_budget=True, sample=sample, seed=7)
    return pol


def clone_return(actor):
    """f64 [N]: the sampled clone's posterior-mean return on the held-out episodes"""
    evals.reset(seed=123)
    return evals.rollout(as_policy(actor, True), posterior_returns=True)["posterior_returns"].double().mean(1)


for name, labels in experts.items():
    actor = copy.deepcopy(init)
    opt = torch.optim.Adam(actor.parameters(), lr=args.lr)
    before = clone_return(actor)
    for ep in range(args.epochs):
        out = train.imitation_gradient(as_policy(actor, False), labels)  # the same episodes every epoch: no reset
        g = {"layers": [(dW.cpu(), db.cpu()) for dW, db in out["policy_gradient"]["layers"]]}
        g["layers"][0] = (g["layers"][0][0] / scale[None, None, :], g["layers"][0][1])
        opt.zero_grad()
        policy.mlp_grad_to_module(actor, g, group=0, ascent=True)  # negated: Adam's step ascends the likelihood
        opt.step()
    ll = float(out["log_likelihood"].double().sum() / out["days"].double().sum().clamp_min(1))
    after = clone_return(actor)
    print(f"clone of the {name} expert: log-likelihood / day {ll:.4f} after {args.epochs} epochs; posterior-mean regret "
          f"before -> after")
    for y, ref in yard.items():
        print(f"    against the {y:10s} optimum: {float((ref - before).mean()):9.4f} -> {float((ref - after).mean()):9.4f}")
print(f"the value of knowing the draw, in posterior-mean return (draw-blind minus own-draw optimum): "
      f"{float((yard['draw-blind'] - yard['own draw']).mean()):.4f}")
train.close()
evals.close()
