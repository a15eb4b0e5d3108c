#!/usr/bin/env python3
"""PPO with every step past the rollout inside the kernels -- examples/ppo_rollout.py (the torch route: a recorded
rollout, a forward over [S, N, n_obs] and torch.min(ratio * A, ratio.clamp(...) * A) in minibatches) without
record=True: no observation row leaves the device code. Per iteration, on a fresh batch of episodes:
  1. rollout(actor | sample, require_budget, alert_mask=True) samples the actor and returns the schedule it issued;
  2. on a twin env reset to the same episodes (the gradient calls read its state and change nothing, so every call and
     every epoch runs on the same episodes): value_gradient(critic, alert_days, advantage=True) fits a [64, 64] tanh
     critic to the reward-to-go along that schedule and returns the advantages Q_s - V_s (--gamma / --gae-lambda:
     GAE(lambda) advantages and lambda-returns instead; --fixed-targets: the later critic epochs regress on the first
     epoch's lambda-returns through target=, as PPO's critic epochs do);
  3. surrogate_gradient(actor, alert_days, advantage, log_prob=True) once: epoch 0's gradient (rho = 1) and the
     log-probabilities of the collecting policy;
  4. K more epochs of surrogate_gradient(actor, alert_days, advantage, old_log_prob=lp0): the clipped importance ratio
     is formed inside the kernel; policy.mlp_grad_to_module writes each gradient into the module's .grad and torch Adam
     takes the step.
Prints, per iteration, the surrogate per scored day, approx_kl per scored day and the clipped share of the last epoch,
and the mean return next to the built-in `never` and `threshold` policies.

--min-heat-qi TAU restricts the actor to hot days, the older reference env's HI_restriction: alert_gate() builds the mask
once per batch of episodes (packed, so nothing is packed again per call) and the sampling rollout and every surrogate
epoch take it as "allowed_days"; gated days are forced choices and carry no ratio.

    python examples/ppo_on_device.py [--iters 12] [--envs 65536] [--epochs 4] [--clip 0.2] [--gamma 0.99 --gae-lambda 0.95 --fixed-targets] [--min-heat-qi 0.8]      # needs one ROCm GPU
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
from torch import nn

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, policy, synth

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=12)
ap.add_argument("--envs", type=int, default=1 << 16)
ap.add_argument("--epochs", type=int, default=4, help="PPO epochs after epoch 0, and critic epochs")
ap.add_argument("--clip", type=float, default=0.2)
ap.add_argument("--entropy-coef", type=float, default=0.0)
ap.add_argument("--lr", type=float, default=3e-3)
ap.add_argument("--gamma", type=float, default=1.0, help="discount of the advantages (1: the Monte-Carlo residual)")
ap.add_argument("--gae-lambda", type=float, default=1.0, help="GAE(lambda) of the advantages")
ap.add_argument("--fixed-targets", action="store_true",
                help="critic epochs after the first regress on the first epoch's lambda-returns (target=), as PPO does")
ap.add_argument("--min-heat-qi", type=float, default=None,
                help="alerts only on days whose observed heat_qi is >= this (alert_gate -> \"allowed_days\")")
args = ap.parse_args()

data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=20, seed=0, extra_confounder_fips=6)
tables = compile_from_synth(data)
n, k = args.envs, tables.n_obs
env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")
twin = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")

obs0, _ = env.reset(seed=0)
scale = obs0.std(dim=0).clamp_min(0.1).cpu()  # [n_obs]: the modules act on obs / scale
torch.manual_seed(0)


def mlp(n_out):
    return nn.Sequential(nn.Linear(k, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, n_out))


actor, critic = mlp(1), mlp(1)
with torch.no_grad():  # start near "rarely alert", as examples/ppo_rollout.py
    actor[-1].weight.mul_(0.01)
    actor[-1].bias.fill_(-2.0)
opt_a = torch.optim.Adam(actor.parameters(), lr=args.lr)
opt_c = torch.optim.Adam(critic.parameters(), lr=args.lr)


def exported(module, **kw):
    """The module on raw rows: the kernel's first layer acts on the raw columns."""
    pol = policy.mlp_from_module(module)
    W1, b1 = pol["layers"][0]
    pol["layers"][0] = (W1 / scale[None, :], b1)
    pol.update(kw)
    return pol


def apply(module, opt, grad):
    """`grad` (the kernels': theta += lr * grad improves) into the module's .grad, negated for Adam's descent step"""
    g = {"layers": [(dW.cpu(), db.cpu()) for dW, db in grad["layers"]]}
    g["layers"][0] = (g["layers"][0][0] / scale[None, None, :], g["layers"][0][1])  # d / d (module's first weight)
    opt.zero_grad()
    policy.mlp_grad_to_module(module, g, group=0, ascent=True)
    nn.utils.clip_grad_norm_(module.parameters(), 10.0)
    opt.step()


never = float(env.rollout({"kind": "never"})["return"].mean())
env.reset(seed=0)
thr = float(env.rollout({"kind": "threshold", "feature": "heat_qi", "threshold": 0.9, "require_budget": True})["return"].mean())
print(f"envs {n}  days {tables.T}  device {torch.cuda.get_device_name(0)}")
print(f"never     {never:9.3f}")
print(f"threshold {thr:9.3f}   (heat_qi > 0.9 while budget is left)")
for it in range(args.iters):
    env.reset(seed=it)
    twin.reset(seed=it)  # the same episodes, left at their first day
    gate = {} if args.min_heat_qi is None else {"allowed_days": env.alert_gate("heat_qi", args.min_heat_qi, packed=True)}
    ro = env.rollout(exported(actor, sample=True, seed=it, require_budget=True, **gate), alert_mask=True)
    sched = ro["alert_days"]
    for ep in range(args.epochs):  # the same episodes every epoch: no reset in between
        if ep > 0 and args.fixed_targets:  # targets fixed at collection time: returns = advantage + old values
            vg = twin.value_gradient(exported(critic), sched, target=returns)
        else:
            vg = twin.value_gradient(exported(critic), sched, advantage=(ep == 0), gamma=args.gamma,
                                     gae_lambda=args.gae_lambda, value_target=(ep == 0 and args.fixed_targets))
        if ep == 0:  # the advantages the actor is updated with come from the critic BEFORE this iteration's fit
            adv, days, returns = vg["advantage"], vg["days"], vg.get("value_target")
        apply(critic, opt_c, vg["value_gradient"])
    valid = torch.arange(adv.shape[0], device=adv.device)[:, None] < days[None, :]
    a = adv[valid]
    A = torch.where(valid, (adv - a.mean()) / (a.std() + 1e-8), torch.zeros_like(adv))
    kw = dict(clip=args.clip, entropy_coef=args.entropy_coef)
    sg = twin.surrogate_gradient(exported(actor, require_budget=True, **gate), sched, A, log_prob=True, **kw)  # epoch 0: rho = 1
    lp0 = sg["log_prob"]
    apply(actor, opt_a, sg["policy_gradient"])
    for ep in range(args.epochs):
        sg = twin.surrogate_gradient(exported(actor, require_budget=True, **gate), sched, A, old_log_prob=lp0, **kw)
        apply(actor, opt_a, sg["policy_gradient"])
    scored = float(sg["days"].double().sum().clamp_min(1))
    print(f"iter {it:2d}   mean return {float(ro['return'].mean()):9.3f}   alerts/env "
          f"{float(ro['alerts'].float().mean()):5.2f}   surrogate/day {float(sg['surrogate'].double().sum()) / scored:9.5f}   "
          f"approx_kl/day {float(sg['approx_kl'].double().sum()) / scored:9.6f}   "
          f"clipped {float(sg['clipped_days'].double().sum()) / scored:6.3f}")
env.close()
twin.close()
