#!/usr/bin/env python3
"""PPO on an SB3-shaped [64, 64] tanh actor (two action values, logit = row1 - row0) with a separate torch critic, with
the data collected inside the rollout kernel: each iteration is one rollout(mlp_from_module(actor) | {"sample": True},
record=True) over 65 536 envs x one whole 153-day episode (lock step: every call is a fresh episode), then GAE from
the recorded reward / valid / terminated with obs[S] as the bootstrap row, and clipped-ratio updates whose old
log-probabilities come from the recorded logits (policy.action_log_prob). The learner works on normalised
observations; the normaliser is folded into the exported actor's first layer, so the kernel sees raw rows. Prints the
mean episode return per iteration next to the built-in `never` and `threshold` policies on the same batch.

    python examples/ppo_rollout.py            # needs one ROCm GPU
"""
import copy
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
from torch import nn

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, policy, synth

data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=20, seed=0, extra_confounder_fips=6)
tables = compile_from_synth(data)
N, iters, epochs, mb = 65536, 15, 4, 1 << 16
gamma, lam, clip, lr = 0.99, 0.95, 0.2, 3e-4
env = HeatAlertVecEnv(N, tables=tables, similar_climate_counties=True)  # lock step: every rollout is a fresh episode
env.reset(seed=0)
dev, k = env.device, tables.n_obs
torch.manual_seed(0)


def mlp(n_out):
    return nn.Sequential(nn.Linear(k, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, n_out)).to(dev)


actor, critic = mlp(2), mlp(1)
with torch.no_grad():  # small initial output layer, as SB3 does (orthogonal gain 0.01): start near p = 0.5 ...
    actor[-1].weight.mul_(0.01)
    actor[-1].bias.copy_(torch.tensor([0.0, -2.0], device=dev))  # ... shifted to "rarely alert"
opt = torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()), lr=lr)
# observation normaliser from the first observations of the batch (fixed for the run)
mean, std = env._obs.mean(dim=0), env._obs.std(dim=0).clamp_min(0.1)


def exported():
    """The actor on raw rows: ((x - mean) / std) folded into the first Linear."""
    a = copy.deepcopy(actor)
    with torch.no_grad():
        a[0].weight.div_(std)
        a[0].bias.sub_(a[0].weight @ mean)
    return policy.mlp_from_module(a)


def logit_of(x):
    y = actor((x - mean) / std)
    return y[:, 1] - y[:, 0]


never = float(env.rollout({"kind": "never"})["return"].mean())
thr = float(env.rollout({"kind": "threshold", "feature": "heat_qi", "threshold": 0.9, "require_budget": True})["return"].mean())
print(f"envs {N}  days {tables.T}  device {torch.cuda.get_device_name(0)}")
print(f"never     {never:9.3f}")
print(f"threshold {thr:9.3f}   (heat_qi > 0.9 while budget is left)")
for it in range(iters):
    t0 = time.perf_counter()
    out = env.rollout(exported() | {"sample": True, "seed": it}, record=True)
    tr = out["trajectory"]
    torch.cuda.synchronize()
    t_col = time.perf_counter() - t0
    S = tr["reward"].shape[0]
    valid, term = tr["valid"], tr["terminated"]
    with torch.no_grad():
        V = torch.cat([critic((tr["obs"][s] - mean) / std)[:, 0].unsqueeze(0) for s in range(S + 1)])
        adv = torch.zeros_like(tr["reward"])
        nxt = torch.zeros(N, device=dev)
        for s in reversed(range(S)):  # GAE; obs[S] bootstraps envs whose episode did not end inside the call
            nonterm = (~term[s]).float()
            delta = tr["reward"][s] + gamma * V[s + 1] * nonterm - V[s]
            nxt = torch.where(valid[s], delta + gamma * lam * nonterm * nxt, torch.zeros_like(nxt))
            adv[s] = nxt
        ret = adv + V[:S]
    x, a = tr["obs"][:S][valid], tr["action"][valid]
    old_lp = policy.action_log_prob(tr["logit"][valid], a)
    A, R = adv[valid], ret[valid]
    A = (A - A.mean()) / (A.std() + 1e-8)
    drift = float((logit_of(x[:mb]).detach() - tr["logit"][valid][:mb]).abs().max())  # kernel vs torch, same params
    M = x.shape[0]
    for _ in range(epochs):
        perm = torch.randperm(M, device=dev)
        for i in range(0, M, mb):
            j = perm[i:i + mb]
            lp = policy.action_log_prob(logit_of(x[j]), a[j])
            ratio = torch.exp(lp - old_lp[j])
            pg = -torch.min(ratio * A[j], ratio.clamp(1 - clip, 1 + clip) * A[j]).mean()
            vf = ((critic((x[j] - mean) / std)[:, 0] - R[j]) ** 2).mean()
            opt.zero_grad()
            (pg + 0.5 * vf).backward()
            nn.utils.clip_grad_norm_(list(actor.parameters()) + list(critic.parameters()), 0.5)
            opt.step()
    print(f"iter {it:2d}   mean return {float(out['return'].mean()):9.3f}   alerts/env "
          f"{float(out['alerts'].float().mean()):5.2f}   env-days {M}   collect {1e3 * t_col:6.1f} ms   "
          f"update {time.perf_counter() - t0 - t_col:5.2f} s   max |logit kernel - torch| {drift:.1e}")
    del out, tr, x, a, old_lp, A, R, V, adv, ret
env.close()
