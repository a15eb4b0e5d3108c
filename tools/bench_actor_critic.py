#!/usr/bin/env python3
"""ms per call of actor_critic_gradient()'s library entry point over one whole 153-day episode at a [64, 64] tanh net of
1 048 576 envs on the BASELINE configs[2] workload (weights/linear shape, S = 746, similar_climate_counties=True), against
the two calls it replaces, all in one process, alternating, timed with device events:
  epoch             w2a_actor_critic_mlp with advantage, value_target and old_log_prob given (one row rebuild, one forward
                    and one backward pass per env-day for both losses)
  value + surrogate w2a_value_gradient_mlp_gae(target=) and w2a_surrogate_gradient_mlp(old_log_prob=) on two one-head
                    [64, 64] nets: the yardstick, unchanged by the actor-critic kernels
  collect           w2a_actor_critic_mlp with nothing given, with the gradient and with grad = NULL (gradient=False)
The ratio epoch / (value + surrogate) is the figure README.md and DESIGN.md quote.
usage: python tools/bench_actor_critic.py [--envs N] [--reps 10] [--warmup 3] [--json PATH]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from weather2alert_amd import HeatAlertVecEnv, _ffi, compile_from_synth, policy, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sd = synth.make_synth("linear", years=list(range(2006, 2017)), n_samples=100, seed=0, extra_confounder_fips=60)
    ct = compile_from_synth(sd)
    n, dev, T = args.envs, torch.device("cuda:0"), ct.T
    print(f"envs {n}  days {T}  obs columns {ct.n_obs}  device {torch.cuda.get_device_name(0)}")
    env = HeatAlertVecEnv(n, tables=ct, similar_climate_counties=True, autoreset="disabled")
    env.reset(seed=0)
    lib, h, stream = env._lib, env._h, env._stream()
    words = (T + 31) // 32
    rng = np.random.default_rng(0)

    def net(n_out):
        dims = [ct.n_obs, 64, 64, n_out]
        return [((rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32),
                 (rng.standard_normal(dims[i + 1]) * 0.3).astype(np.float32)) for i in range(3)]

    two = net(2)
    one = lambda row: two[:-1] + [(two[-1][0][row:row + 1], two[-1][1][row:row + 1])]  # noqa: E731
    ac = policy.check_actor_critic_net(dict(kind="mlp", layers=two, activation="tanh"), ct.n_obs, n, ct.obs_slot, dev)
    actor = policy.check_mlp_policy(dict(kind="mlp", layers=one(0), activation="tanh"), ct.n_obs, n, ct.obs_slot, dev)
    critic = policy.check_mlp_policy(dict(kind="mlp", layers=one(1), activation="tanh"), ct.n_obs, n, ct.obs_slot, dev)

    def struct(p):
        mp = _ffi.MlpPolicy()
        mp.params, mp.group, mp.order = p.params.data_ptr(), None, None
        mp.n_groups, mp.n_layers, mp.width, mp.activation = 1, p.n_layers, p.width, _ffi.MLP_ACTIVATIONS["tanh"]
        mp.sample, mp.require_budget, mp.seed = 0, 0, 0
        return mp

    ac_s, actor_s, critic_s = struct(ac), struct(actor), struct(critic)
    # the schedule: the net's own sampled rollout (what a PPO iteration collects), then the env back at its start
    sched = env.rollout(dict(kind="mlp", layers=one(0), activation="tanh", sample=True, seed=1), alert_mask=True)["alert_days"]
    env.reset(seed=0)
    mask = policy.pack_alert_days(sched, words)
    del sched
    ac_blocks = torch.empty((1, policy.mlp_heads_stride(64, 2)), dtype=torch.float32, device=dev)
    one_blocks = torch.empty((1, policy.mlp_stride(64, 2)), dtype=torch.float32, device=dev)
    f32 = lambda *s: torch.empty(s or (n,), dtype=torch.float32, device=dev)  # noqa: E731
    i32 = lambda: torch.empty(n, dtype=torch.int32, device=dev)  # noqa: E731
    sur, vl, kl, ent, ret, sq = f32(), f32(), f32(), f32(), f32(), f32()
    cl, days = i32(), i32()
    adv, vt, lp = f32(T, n), f32(T, n), f32(T, n)
    ws = torch.empty(max(lib.w2a_actor_critic_mlp_workspace_bytes(n, T, 1, 64, 2),
                         lib.w2a_value_gradient_mlp_gae_workspace_bytes(n, T, 1, 64, 2),
                         lib.w2a_surrogate_gradient_mlp_workspace_bytes(n, T, 1, 64, 2)), dtype=torch.uint8, device=dev)
    obs = env._obs.data_ptr()
    per_env = (sur.data_ptr(), vl.data_ptr(), cl.data_ptr(), kl.data_ptr(), ent.data_ptr(), days.data_ptr())
    tail = (ws.data_ptr(), ws.numel(), stream, None, 0)

    def collect(grad):
        return lambda: lib.w2a_actor_critic_mlp(
            h, C.byref(ac_s), mask.data_ptr(), words, None, None, 0, None, 0, None, 0, 0.2, 0.5, 0.01, 0.99, 0.95, 0, T, obs,
            grad, *per_env, ret.data_ptr(), adv.data_ptr(), vt.data_ptr(), lp.data_ptr(), *tail)

    with torch.cuda.device(dev):  # the epoch's inputs are a collect call's outputs
        _ffi.check(collect(ac_blocks.data_ptr())(), "collect")
        torch.cuda.synchronize()
    adv_in = ((adv - adv.mean()) / (adv.std() + 1e-8)).contiguous()
    vt_in, lp_in = vt.clone(), (lp - 0.05 * torch.rand_like(lp)).clamp_(max=0.0)  # ratios on either side of 1
    ins = (adv_in.data_ptr(), T, vt_in.data_ptr(), T, lp_in.data_ptr(), T)
    calls = {
        "epoch: actor_critic [64,64]": lambda: lib.w2a_actor_critic_mlp(
            h, C.byref(ac_s), mask.data_ptr(), words, None, *ins, 0.2, 0.5, 0.01, 1.0, 1.0, 0, T, obs,
            ac_blocks.data_ptr(), *per_env, None, None, None, None, *tail),
        "epoch: value_gradient(target=) [64,64]": lambda: lib.w2a_value_gradient_mlp_gae(
            h, C.byref(critic_s), mask.data_ptr(), words, None, T, obs, one_blocks.data_ptr(), sq.data_ptr(),
            days.data_ptr(), ret.data_ptr(), None, 1.0, 1.0, 0, None, vt_in.data_ptr(), T, ws.data_ptr(), ws.numel(), stream),
        "epoch: surrogate_gradient(old_log_prob=) [64,64]": lambda: lib.w2a_surrogate_gradient_mlp(
            h, C.byref(actor_s), mask.data_ptr(), words, None, adv_in.data_ptr(), T, lp_in.data_ptr(), T, 0.2, 0.01, T, obs,
            one_blocks.data_ptr(), sur.data_ptr(), cl.data_ptr(), kl.data_ptr(), ent.data_ptr(), days.data_ptr(), None,
            ws.data_ptr(), ws.numel(), stream),
        "collect: actor_critic [64,64]": collect(ac_blocks.data_ptr()),
        "collect: actor_critic, gradient=False": collect(None),
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
    res = {"envs": n, "days": T, "scored_env_days": env_days, "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "ms": {}}
    for k, v in ms.items():
        res["ms"][k] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print(f"{k:52s} {statistics.median(v):9.3f} ms/call  (min {min(v):.3f}, max {max(v):.3f})")
    med = lambda k: res["ms"][k]["median"]  # noqa: E731
    two_calls = med("epoch: value_gradient(target=) [64,64]") + med("epoch: surrogate_gradient(old_log_prob=) [64,64]")
    res["two_calls_ms"] = two_calls
    res["epoch_over_two_calls"] = med("epoch: actor_critic [64,64]") / two_calls
    res["collect_first_pass_share"] = med("collect: actor_critic, gradient=False") / med("collect: actor_critic [64,64]")
    print(f"epoch: actor_critic / (value_gradient + surrogate_gradient) = {res['epoch_over_two_calls']:.3f} "
          f"({med('epoch: actor_critic [64,64]'):.1f} ms against {two_calls:.1f} ms); collect without the gradient is "
          f"{res['collect_first_pass_share']:.3f} of collect with it")
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    env.close()


if __name__ == "__main__":
    main()
