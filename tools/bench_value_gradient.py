#!/usr/bin/env python3
"""ms per call of value_gradient()'s library entry points at 1 048 576 envs over one whole 153-day episode, next to
imitation_gradient()'s at the same shape, in one process:
  linear        w2a_value_gradient_linear (advantage off / on)   against  w2a_imitation_gradient_linear
  [64,64] tanh  w2a_value_gradient_mlp    (advantage off / on)   against  w2a_imitation_gradient_mlp
The difference is the two reward chains (and, for the linear kind, the second pass over 9 B of scratch per env-day)
plus the advantage stores. The schedule is the hindsight optimum of the episodes. Every figure is the library call
alone (preallocated outputs and workspace, HIP events on the launch stream), so the host-side group mean of the linear
kinds is in none of them. The calls alternate inside every repetition; medians, minima and maxima of --reps after
--warmup rounds. There is no pass bar: nobody has measured these before.
--torch-critic also times what examples/ppo_rollout.py pays for its critic at --torch-envs envs (the recorded rows do
not fit beside the rest at 1 M envs x 153 days): rollout(record=True) of a [64, 64] actor, the torch critic over
[S + 1, N, n_obs], the GAE loop over days and one epoch of critic minibatch updates, per env-day.
usage: python tools/bench_value_gradient.py [--envs N] [--reps 10] [--warmup 3] [--torch-critic] [--json PATH]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from weather2alert_amd import HeatAlertVecEnv, _ffi, compile_from_synth, policy, synth  # noqa: E402


def torch_critic(ct, n, dev):
    """seconds of the critic's share of one iteration of examples/ppo_rollout.py: values of every recorded row, GAE,
    one epoch of minibatch regression (the recorded rollout itself is timed apart)"""
    from torch import nn

    env = HeatAlertVecEnv(n, tables=ct, similar_climate_counties=True)
    env.reset(seed=0)
    k = ct.n_obs
    mk = lambda o: nn.Sequential(nn.Linear(k, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, o)).to(dev)  # noqa: E731
    torch.manual_seed(0)
    actor, critic = mk(2), mk(1)
    opt = torch.optim.Adam(critic.parameters(), lr=3e-4)
    res = {}
    for rep in range(2):  # the first round warms up allocator and kernels
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = env.rollout(policy.mlp_from_module(actor) | {"sample": True, "seed": rep}, record=True)
        tr = out["trajectory"]
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        S = tr["reward"].shape[0]
        valid, term = tr["valid"], tr["terminated"]
        with torch.no_grad():
            V = torch.cat([critic(tr["obs"][s])[:, 0].unsqueeze(0) for s in range(S + 1)])
            adv, nxt = torch.zeros_like(tr["reward"]), torch.zeros(n, device=dev)
            for s in reversed(range(S)):
                nonterm = (~term[s]).float()
                delta = tr["reward"][s] + 0.99 * V[s + 1] * nonterm - V[s]
                nxt = torch.where(valid[s], delta + 0.99 * 0.95 * nonterm * nxt, torch.zeros_like(nxt))
                adv[s] = nxt
            ret = adv + V[:S]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        x, R = tr["obs"][:S][valid], ret[valid]
        M, mb = x.shape[0], 1 << 16
        perm = torch.randperm(M, device=dev)
        for i in range(0, M, mb):
            j = perm[i:i + mb]
            opt.zero_grad()
            ((critic(x[j])[:, 0] - R[j]) ** 2).mean().backward()
            opt.step()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        res = {"envs": n, "env_days": int(M), "rollout_record_ms": 1e3 * (t1 - t0), "values_and_gae_ms": 1e3 * (t2 - t1),
               "one_epoch_updates_ms": 1e3 * (t3 - t2)}
        del out, tr, x, R, V, adv, ret
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-critic", action="store_true")
    ap.add_argument("--torch-envs", type=int, default=1 << 16)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=20, seed=0, extra_confounder_fips=6)
    ct = compile_from_synth(data)
    n, dev = args.envs, torch.device("cuda:0")
    print(f"envs {n}  days {ct.T}  obs columns {ct.n_obs}  device {torch.cuda.get_device_name(0)}")
    env = HeatAlertVecEnv(n, tables=ct, similar_climate_counties=True, autoreset="disabled")
    env.reset(seed=0)
    lib, h, stream = env._lib, env._h, env._stream()
    words = (ct.T + 31) // 32
    sched = env.hindsight_optimum()["alert_days"]
    mask = policy.pack_alert_days(sched, words)
    del sched
    rng = np.random.default_rng(0)
    W = (rng.standard_normal((1, ct.n_obs)) * 0.2).astype(np.float32)
    lin = policy.check_linear_policy(dict(kind="linear", weight=W, bias=np.zeros(1, np.float32)), ct.n_obs, n, ct.obs_slot, dev)
    dims = [ct.n_obs, 64, 64, 1]
    layers = [((rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32),
               (rng.standard_normal(dims[i + 1]) * 0.3).astype(np.float32)) for i in range(3)]
    mlp = policy.check_mlp_policy(dict(kind="mlp", layers=layers, activation="tanh"), ct.n_obs, n, ct.obs_slot, dev)
    lp = _ffi.LinearPolicy()
    lp.weight, lp.bias, lp.group = lin.weight_slots.data_ptr(), lin.bias.data_ptr(), None
    lp.n_groups, lp.sample, lp.require_budget, lp.seed = 1, 0, 0, 0
    mp = _ffi.MlpPolicy()
    mp.params, mp.group, mp.order = mlp.params.data_ptr(), None, None
    mp.n_groups, mp.n_layers, mp.width, mp.activation = 1, mlp.n_layers, mlp.width, _ffi.MLP_ACTIVATIONS["tanh"]
    mp.sample, mp.require_budget, mp.seed = 0, 0, 0
    rows = torch.empty((ct.n_obs + 1, n), dtype=torch.float32, device=dev)
    blocks = torch.empty((1, policy.mlp_stride(mlp.width, mlp.n_layers)), dtype=torch.float32, device=dev)
    f32 = lambda: torch.empty(n, dtype=torch.float32, device=dev)  # noqa: E731
    ll, sq, ret = f32(), f32(), f32()
    days = torch.empty(n, dtype=torch.int32, device=dev)
    adv = torch.empty((ct.T, n), dtype=torch.float32, device=dev)
    ws_lin = torch.empty(lib.w2a_value_gradient_linear_workspace_bytes(n, ct.T), dtype=torch.uint8, device=dev)
    ws_mlp = torch.empty(lib.w2a_value_gradient_mlp_workspace_bytes(n, ct.T, 1, mlp.width, mlp.n_layers),
                         dtype=torch.uint8, device=dev)
    obs, T = env._obs.data_ptr(), ct.T

    def vg_lin(a):
        return lambda: lib.w2a_value_gradient_linear(
            h, C.byref(lp), mask.data_ptr(), words, None, T, obs, rows.data_ptr(), sq.data_ptr(), days.data_ptr(),
            ret.data_ptr(), a, ws_lin.data_ptr(), ws_lin.numel(), stream)

    def vg_mlp(a):
        return lambda: lib.w2a_value_gradient_mlp(
            h, C.byref(mp), mask.data_ptr(), words, None, T, obs, blocks.data_ptr(), sq.data_ptr(), days.data_ptr(),
            ret.data_ptr(), a, ws_mlp.data_ptr(), ws_mlp.numel(), stream)

    calls = {
        "imitation linear": lambda: lib.w2a_imitation_gradient_linear(
            h, C.byref(lp), mask.data_ptr(), words, None, T, obs, rows.data_ptr(), ll.data_ptr(), days.data_ptr(), stream),
        "value linear": vg_lin(None),
        "value linear + advantage": vg_lin(adv.data_ptr()),
        "imitation [64,64] tanh": lambda: lib.w2a_imitation_gradient_mlp(
            h, C.byref(mp), mask.data_ptr(), words, None, T, obs, blocks.data_ptr(), ll.data_ptr(), days.data_ptr(),
            ws_mlp.data_ptr(), ws_mlp.numel(), stream),
        "value [64,64] tanh": vg_mlp(None),
        "value [64,64] tanh + advantage": vg_mlp(adv.data_ptr()),
    }
    ms = {k: [] for k in calls}
    with torch.cuda.device(dev):
        for rep in range(args.warmup + args.reps):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _ffi.check(fn(), k)
                e1.record()
                e1.synchronize()
                if rep >= args.warmup:
                    ms[k].append(e0.elapsed_time(e1))
    res = {"envs": n, "days": ct.T, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "ms": {}}
    for k, v in ms.items():
        res["ms"][k] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print(f"{k:32s} {statistics.median(v):9.3f} ms/call  (min {min(v):.3f}, max {max(v):.3f}, spread {max(v) - min(v):.3f})")
    for kind in ("linear", "[64,64] tanh"):
        base = res["ms"][f"imitation {kind}"]["median"]
        print(f"{kind:13s} value / imitation = {res['ms'][f'value {kind}']['median'] / base:.3f}   "
              f"with advantage = {res['ms'][f'value {kind} + advantage']['median'] / base:.3f}")
    env.close()
    del rows, adv, ws_lin, ws_mlp
    if args.torch_critic:
        res["torch_critic"] = torch_critic(ct, args.torch_envs, dev)
        print("torch critic (examples/ppo_rollout.py), " + "  ".join(f"{k} {v:.1f}" if isinstance(v, float) else f"{k} {v}"
                                                                     for k, v in res["torch_critic"].items()))
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
