#!/usr/bin/env python3
"""ms per call of the *_gae entry points of value_gradient() at 1 048 576 envs over one whole 153-day episode, next to
the existing entry points of the same kind, in one process (the protocol of tools/bench_value_gradient.py):
  linear        w2a_value_gradient_linear_gae   gamma 0.99, lambda 0.95, advantage + value_target   and   target=
                against  w2a_value_gradient_linear with advantage
  [64,64] tanh  w2a_value_gradient_mlp_gae      the same two forms
                against  w2a_value_gradient_mlp with advantage
The schedule is the hindsight optimum of the episodes. Every figure is the library call alone (preallocated outputs and
workspace, HIP events on the launch stream). The calls alternate inside every repetition; medians, minima and maxima of
--reps after --warmup rounds, and per repetition the ratio to the existing call of the same kind in that repetition.
The targets of the target= form are the value_target rows of a GAE call made before the timing starts. There is no pass
bar: nobody has measured these before.
usage: python tools/bench_gae.py [--envs N] [--reps 10] [--warmup 3] [--json PATH]"""
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
    sq, ret = f32(), f32()
    days = torch.empty(n, dtype=torch.int32, device=dev)
    day_rows = lambda: torch.empty((ct.T, n), dtype=torch.float32, device=dev)  # noqa: E731
    adv, vt, tg_lin, tg_mlp = day_rows(), day_rows(), day_rows(), day_rows()
    ws_lin = torch.empty(lib.w2a_value_gradient_linear_gae_workspace_bytes(n, ct.T), dtype=torch.uint8, device=dev)
    assert ws_lin.numel() >= lib.w2a_value_gradient_linear_workspace_bytes(n, ct.T)  # serves the existing call too
    ws_mlp = torch.empty(lib.w2a_value_gradient_mlp_gae_workspace_bytes(n, ct.T, 1, mlp.width, mlp.n_layers),
                         dtype=torch.uint8, device=dev)
    obs, T = env._obs.data_ptr(), ct.T
    front = (mask.data_ptr(), words, None, T, obs)

    def lin_gae(a, v, target, gamma=0.99, lam=0.95):
        tail = (gamma, lam, 0, v, target, T if target else 0)
        return lambda: lib.w2a_value_gradient_linear_gae(
            h, C.byref(lp), *front, rows.data_ptr(), sq.data_ptr(), days.data_ptr(), ret.data_ptr(), a, *tail,
            ws_lin.data_ptr(), ws_lin.numel(), stream)

    def mlp_gae(a, v, target, gamma=0.99, lam=0.95):
        tail = (gamma, lam, 0, v, target, T if target else 0)
        return lambda: lib.w2a_value_gradient_mlp_gae(
            h, C.byref(mp), *front, blocks.data_ptr(), sq.data_ptr(), days.data_ptr(), ret.data_ptr(), a, *tail,
            ws_mlp.data_ptr(), ws_mlp.numel(), stream)

    with torch.cuda.device(dev):  # the targets of the target= form: each kind's own lambda-returns
        _ffi.check(lin_gae(None, tg_lin.data_ptr(), None)(), "targets linear")
        _ffi.check(mlp_gae(None, tg_mlp.data_ptr(), None)(), "targets mlp")
        torch.cuda.synchronize()
    calls = {
        "value linear + advantage": lambda: lib.w2a_value_gradient_linear(
            h, C.byref(lp), *front, rows.data_ptr(), sq.data_ptr(), days.data_ptr(), ret.data_ptr(), adv.data_ptr(),
            ws_lin.data_ptr(), ws_lin.numel(), stream),
        "gae linear + advantage + value_target": lin_gae(adv.data_ptr(), vt.data_ptr(), None),
        "gae linear target=": lin_gae(None, None, tg_lin.data_ptr(), 1.0, 1.0),
        "value [64,64] tanh + advantage": lambda: lib.w2a_value_gradient_mlp(
            h, C.byref(mp), *front, blocks.data_ptr(), sq.data_ptr(), days.data_ptr(), ret.data_ptr(), adv.data_ptr(),
            ws_mlp.data_ptr(), ws_mlp.numel(), stream),
        "gae [64,64] tanh + advantage + value_target": mlp_gae(adv.data_ptr(), vt.data_ptr(), None),
        "gae [64,64] tanh target=": mlp_gae(None, None, tg_mlp.data_ptr(), 1.0, 1.0),
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
    res = {"envs": n, "days": ct.T, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "ms": {}, "ratio": {}}
    for k, v in ms.items():
        res["ms"][k] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print(f"{k:46s} {statistics.median(v):9.3f} ms/call  (min {min(v):.3f}, max {max(v):.3f}, spread {max(v) - min(v):.3f})")
    for kind in ("linear", "[64,64] tanh"):
        base = ms[f"value {kind} + advantage"]
        for form in ("+ advantage + value_target", "target="):
            r = [x / b for x, b in zip(ms[f"gae {kind} {form}"], base)]  # per repetition, against the same repetition
            res["ratio"][f"gae {kind} {form}"] = dict(median=statistics.median(r), min=min(r), max=max(r), per_rep=r)
            print(f"gae {kind} {form} / value {kind} + advantage: median {statistics.median(r):.3f}  "
                  f"(min {min(r):.3f}, max {max(r):.3f})")
    env.close()
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
