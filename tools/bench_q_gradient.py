#!/usr/bin/env python3
"""ms per call of q_gradient()'s library entry point over one whole 153-day episode at the [64, 64] net of
examples/dqn_on_device.py, next to the two routes it is measured against, in one process:
  q_gradient        w2a_q_gradient_mlp, double-DQN with a distinct target net (and with the online net as its own target:
                    the second evaluation of every row is skipped)
  value_gradient    w2a_value_gradient_mlp on a one-output [64, 64] net at the same shape: the same passes minus one
                    forward per row -- the yardstick (its kernels are the parent's, byte for byte)
  torch route       what a user pays without the entry point, at --torch-envs envs (the recorded rows do not fit beside
                    the rest at 1 M envs x 153 days): rollout(record=True) of the Q-net, then a torch double-DQN Huber
                    loss over the recorded rows [S + 1, N, n_obs] and backward(); reported per env-day next to the
                    kernel route's figure per env-day
The library calls are timed alone (preallocated outputs and workspace, HIP events on the launch stream) and alternate
inside every repetition; medians, minima and maxima of --reps after --warmup rounds. No figure is fixed in advance.
usage: python tools/bench_q_gradient.py [--envs N] [--torch-envs M] [--reps 10] [--warmup 3] [--json PATH]"""
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


def torch_route(ct, n, dev, gamma, reps=3):
    """seconds of one double-DQN gradient the torch way: the recorded rollout, then forward and backward over its rows"""
    from torch import nn

    env = HeatAlertVecEnv(n, tables=ct, similar_climate_counties=True, autoreset="disabled")
    k = ct.n_obs
    mk = lambda: nn.Sequential(nn.Linear(k, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 2)).to(dev)  # noqa: E731
    torch.manual_seed(0)
    q_net, target = mk(), mk()
    res = {}
    for rep in range(reps):  # the first rounds warm up allocator and kernels; the last is reported
        env.reset(seed=rep)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr = env.rollout(policy.mlp_from_module(q_net) | {"sample": True, "seed": rep}, record=True)["trajectory"]
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        S = tr["reward"].shape[0]
        valid, term, obs = tr["valid"], tr["terminated"], tr["obs"]
        q_net.zero_grad()
        with torch.no_grad():
            nxt_online = q_net(obs[1:]).argmax(dim=-1, keepdim=True)
            nxt = target(obs[1:]).gather(-1, nxt_online)[..., 0]
            last = torch.zeros_like(term)
            last[S - 1] = True
            y = tr["reward"] + gamma * torch.where(term | last, torch.zeros_like(nxt), nxt)
        qsa = q_net(obs[:S]).gather(-1, tr["alert"].long()[..., None])[..., 0]
        loss = torch.nn.functional.smooth_l1_loss(qsa, y, reduction="none")
        (torch.where(valid, loss, torch.zeros_like(loss)).sum() / n).backward()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        days = int(valid.sum())
        res = {"envs": n, "env_days": days, "rollout_record_ms": 1e3 * (t1 - t0), "loss_and_backward_ms": 1e3 * (t2 - t1),
               "total_ms": 1e3 * (t2 - t0), "ns_per_env_day": 1e9 * (t2 - t0) / days}
        del tr, obs, qsa, loss, y, nxt, nxt_online
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1 << 20)
    ap.add_argument("--torch-envs", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gamma", type=float, default=0.99)
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

    def net(n_out):
        dims = [ct.n_obs, 64, 64, n_out]
        return [((rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32),
                 (rng.standard_normal(dims[i + 1]) * 0.3).astype(np.float32)) for i in range(3)]

    qd, td = (dict(kind="mlp", layers=net(2), activation="relu") for _ in range(2))
    qp, tparams = policy.check_q_net(qd, td, ct.n_obs, n, ct.obs_slot, dev)
    vp = policy.check_mlp_policy(dict(kind="mlp", layers=net(1), activation="relu"), ct.n_obs, n, ct.obs_slot, dev)

    def struct(params, width, n_layers):
        mp = _ffi.MlpPolicy()
        mp.params, mp.group, mp.order = params.data_ptr(), None, None
        mp.n_groups, mp.n_layers, mp.width, mp.activation = 1, n_layers, width, _ffi.MLP_ACTIVATIONS["relu"]
        mp.sample, mp.require_budget, mp.seed = 0, 0, 0
        return mp

    q_s, t_s, v_s = struct(qp.params, qp.width, qp.n_layers), struct(tparams, qp.width, qp.n_layers), struct(vp.params, vp.width, vp.n_layers)
    q_blocks = torch.empty((1, policy.mlp_heads_stride(qp.width, qp.n_layers)), dtype=torch.float32, device=dev)
    v_blocks = torch.empty((1, policy.mlp_stride(vp.width, vp.n_layers)), dtype=torch.float32, device=dev)
    f32 = lambda: torch.empty(n, dtype=torch.float32, device=dev)  # noqa: E731
    loss, ret = f32(), f32()
    days = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(max(lib.w2a_q_gradient_mlp_workspace_bytes(n, ct.T, 1, qp.width, qp.n_layers),
                         lib.w2a_value_gradient_mlp_workspace_bytes(n, ct.T, 1, vp.width, vp.n_layers)),
                     dtype=torch.uint8, device=dev)
    obs, T = env._obs.data_ptr(), ct.T

    def qg(target):
        return lambda: lib.w2a_q_gradient_mlp(
            h, C.byref(q_s), target, mask.data_ptr(), words, None, T, obs, q_blocks.data_ptr(), loss.data_ptr(),
            days.data_ptr(), ret.data_ptr(), args.gamma, 1, _ffi.Q_LOSSES["huber"], 1.0, 0, None, None, ws.data_ptr(),
            ws.numel(), stream)

    calls = {
        "value_gradient [64,64]": lambda: lib.w2a_value_gradient_mlp(
            h, C.byref(v_s), mask.data_ptr(), words, None, T, obs, v_blocks.data_ptr(), loss.data_ptr(), days.data_ptr(),
            ret.data_ptr(), None, ws.data_ptr(), ws.numel(), stream),
        "q_gradient [64,64] double, target net": qg(C.byref(t_s)),
        "q_gradient [64,64] double, own target": qg(None),
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
    env_days = int(days.sum())
    res = {"envs": n, "days": ct.T, "env_days": env_days, "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "ms": {}}
    for k, v in ms.items():
        res["ms"][k] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print(f"{k:40s} {statistics.median(v):9.3f} ms/call  (min {min(v):.3f}, max {max(v):.3f})")
    base = res["ms"]["value_gradient [64,64]"]["median"]
    kern = res["ms"]["q_gradient [64,64] double, target net"]["median"]
    res["q_over_value_gradient"] = kern / base
    res["q_own_target_over_value_gradient"] = res["ms"]["q_gradient [64,64] double, own target"]["median"] / base
    res["q_gradient_ns_per_env_day"] = 1e6 * kern / env_days
    env.close()
    del ws, mask
    res["torch_route"] = torch_route(ct, args.torch_envs, dev, args.gamma)
    res["torch_over_q_gradient_per_env_day"] = res["torch_route"]["ns_per_env_day"] / res["q_gradient_ns_per_env_day"]
    print(f"q_gradient / value_gradient = {res['q_over_value_gradient']:.3f} (own target "
          f"{res['q_own_target_over_value_gradient']:.3f}); per env-day: q_gradient {res['q_gradient_ns_per_env_day']:.2f} ns, "
          f"torch route {res['torch_route']['ns_per_env_day']:.2f} ns at {args.torch_envs} envs "
          f"(x {res['torch_over_q_gradient_per_env_day']:.1f})")
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
