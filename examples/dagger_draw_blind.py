#!/usr/bin/env python3
"""DAgger with the draw-blind expert: the loop of examples/dagger_on_device.py with labels that are functions of what
a policy sees.

Every iteration the learner (a linear policy on standardised columns) plays its own sampled rollout on fresh episodes,
hindsight_posterior_values() says what the expert that knows the weather but NOT the posterior draw would have done in
the states the LEARNER reached ("expert_alert_days") and what the rollout lost against it ("regret"), and
imitation_gradient(labels=...) fits the learner to those labels along its own schedule; one Adam step per iteration.
Evaluated as examples/draw_blind_expert.py evaluates its clones: the sampled learner's posterior-mean return on held-out
episodes (rollout(posterior_returns=True)) against both yardsticks -- the own-draw optimum's posterior-mean return and
hindsight_posterior_optimum()'s. What the learner reaches is printed as it is.

    python examples/dagger_draw_blind.py [--envs 16384] [--iters 30]      # needs one ROCm GPU
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, synth

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=1 << 14)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--lr", type=float, default=0.05)
args = ap.parse_args()

tables = compile_from_synth(synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=100, seed=0,
                                             extra_confounder_fips=6))
n, k = args.envs, tables.n_obs
env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
evals = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled", env_gid0=n)
env.reset(seed=0)
scale = env._obs.std(dim=0).clamp_min(0.1)  # the policy sees standardised columns: W = theta / scale

theta = torch.zeros(k, device=env.device, requires_grad=True)
bias = torch.full((1,), -2.0, device=env.device, requires_grad=True)
opt = torch.optim.Adam([theta, bias], lr=args.lr)


def as_policy(**kw):
    return dict(kind="linear", weight=(theta.detach() / scale)[None, :].contiguous(), bias=bias.detach(),
                require_budget=True, **kw)


# the held-out episodes and their two yardsticks, in posterior-mean returns
evals.reset(seed=123)
ev0 = {key: v.clone() for key, v in evals.state().items()}
yard = {"own draw": evals.posterior_returns(ev0, evals.hindsight_optimum(ev0)["alert_days"]).double().mean(1),
        "draw-blind": evals.hindsight_posterior_optimum(ev0)["return"].double()}


def held_out_regret():
    """the sampled learner's posterior-mean regret on the held-out episodes against each yardstick"""
    evals.reset(seed=123)
    ret = evals.rollout(as_policy(sample=True, seed=7), posterior_returns=True)["posterior_returns"].double().mean(1)
    return {y: float((ref - ret).mean()) for y, ref in yard.items()}


before = held_out_regret()
print(f"{n} fresh episodes per iteration; the learner's own sampled rollout against the draw-blind expert")
print(f"{'iter':>4s} {'regret (draw-blind)':>20s} {'label != action':>16s} {'DPs run':>8s}")
for it in range(args.iters):
    env.reset(seed=1 + it)
    out = env.rollout(as_policy(sample=True, seed=100 + it), alert_mask=True)
    env.reset(seed=1 + it)
    hv = env.hindsight_posterior_values(out["alert_days"])  # the draw-blind expert in the learner's states
    g = env.imitation_gradient(as_policy(), out["alert_days"], labels=hv["expert_alert_days"])["policy_gradient"]
    opt.zero_grad()  # one Adam step UP the log-likelihood (its gradient is with respect to W = theta / scale)
    theta.grad = -(g["weight"][0] / scale)
    bias.grad = -g["bias"].clone()
    opt.step()
    differ = float((hv["expert_alert_days"] != out["alert_days"]).double().mean())
    print(f"{it:4d} {float(hv['regret'].double().mean()):20.3f} {differ:16.4f} {env.last_hindsight_posterior_keys:8d}")
after = held_out_regret()
print(f"held-out episodes, posterior-mean regret of the sampled learner before -> after {args.iters} iterations")
for y in yard:
    print(f"    against the {y:10s} optimum: {before[y]:9.4f} -> {after[y]:9.4f}")
env.close()
evals.close()
