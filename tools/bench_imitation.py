#!/usr/bin/env python3
"""ms per call of imitation_gradient()'s library entry points at 1 048 576 envs over one whole 153-day episode, next to
the policy-gradient entry points they are the supervised counterparts of, in one process:
  linear        w2a_imitation_gradient_linear   against  w2a_policy_gradient_linear ("no_alert" baseline)
  [64,64] tanh  w2a_imitation_gradient_mlp      against  w2a_policy_gradient_mlp    ("no_alert" baseline)
The schedule is the hindsight optimum of the episodes. Every figure is the library call alone (preallocated outputs and
workspace, HIP events on the launch stream), so the host-side group mean of the linear kinds is in neither. The four
calls alternate inside every repetition; medians, minima and maxima of --reps after --warmup rounds. Expectation: each
new call is no slower than its counterpart (it runs a strict subset of that work) beyond the counterpart's own
run-to-run spread (max - min over the repetitions); the tool prints whether that held and writes the numbers as JSON.
usage: python tools/bench_imitation.py [--envs N] [--reps 10] [--warmup 3] [--json PATH]   (one ROCm GPU)"""
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
    lin = policy.check_linear_policy(dict(kind="linear", weight=W, bias=np.zeros(1, np.float32), sample=True, seed=1),
                                     ct.n_obs, n, ct.obs_slot, dev)
    dims = [ct.n_obs, 64, 64, 1]
    layers = [((rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32),
               (rng.standard_normal(dims[i + 1]) * 0.3).astype(np.float32)) for i in range(3)]
    mlp = policy.check_mlp_policy(dict(kind="mlp", layers=layers, activation="tanh", sample=True, seed=1), ct.n_obs, n,
                                  ct.obs_slot, dev)
    lp = _ffi.LinearPolicy()
    lp.weight, lp.bias, lp.group = lin.weight_slots.data_ptr(), lin.bias.data_ptr(), None
    lp.n_groups, lp.sample, lp.require_budget, lp.seed = 1, 1, 0, 1
    mp = _ffi.MlpPolicy()
    mp.params, mp.group, mp.order = mlp.params.data_ptr(), None, None
    mp.n_groups, mp.n_layers, mp.width, mp.activation = 1, mlp.n_layers, mlp.width, _ffi.MLP_ACTIVATIONS["tanh"]
    mp.sample, mp.require_budget, mp.seed = 1, 0, 1
    rows = torch.empty((ct.n_obs + 1, n), dtype=torch.float32, device=dev)
    blocks = torch.empty((1, policy.mlp_stride(mlp.width, mlp.n_layers)), dtype=torch.float32, device=dev)
    ll = torch.empty(n, dtype=torch.float32, device=dev)
    days = torch.empty(n, dtype=torch.int32, device=dev)
    ws_lin = torch.empty(lib.w2a_policy_gradient_workspace_bytes(n, ct.T), dtype=torch.uint8, device=dev)
    ws_mlp = torch.empty(lib.w2a_policy_gradient_mlp_workspace_bytes(n, ct.T, 1, mlp.width, mlp.n_layers),
                         dtype=torch.uint8, device=dev)
    assert ws_mlp.numel() == lib.w2a_imitation_gradient_mlp_workspace_bytes(n, ct.T, 1, mlp.width, mlp.n_layers)
    obs, T = env._obs.data_ptr(), ct.T
    calls = {
        "imitation linear": lambda: lib.w2a_imitation_gradient_linear(
            h, C.byref(lp), mask.data_ptr(), words, None, T, obs, rows.data_ptr(), ll.data_ptr(), days.data_ptr(), stream),
        "policy_gradient linear": lambda: lib.w2a_policy_gradient_linear(
            h, C.byref(lp), _ffi.PG_BASELINES["no_alert"], T, obs, rows.data_ptr(), ws_lin.data_ptr(), ws_lin.numel(), stream),
        "imitation [64,64] tanh": lambda: lib.w2a_imitation_gradient_mlp(
            h, C.byref(mp), mask.data_ptr(), words, None, T, obs, blocks.data_ptr(), ll.data_ptr(), days.data_ptr(),
            ws_mlp.data_ptr(), ws_mlp.numel(), stream),
        "policy_gradient [64,64] tanh": lambda: lib.w2a_policy_gradient_mlp(
            h, C.byref(mp), _ffi.PG_BASELINES["no_alert"], T, obs, blocks.data_ptr(), ws_mlp.data_ptr(), ws_mlp.numel(), stream),
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
        print(f"{k:30s} {statistics.median(v):9.3f} ms/call  (min {min(v):.3f}, max {max(v):.3f}, spread {max(v) - min(v):.3f})")
    res["holds"] = {}
    for kind in ("linear", "[64,64] tanh"):
        new, old = res["ms"][f"imitation {kind}"], res["ms"][f"policy_gradient {kind}"]
        ok = new["median"] <= old["median"] + (old["max"] - old["min"])
        res["holds"][kind] = bool(ok)
        print(f"{kind:13s} imitation / policy_gradient = {new['median'] / old['median']:.3f}   "
              f"no slower within the counterpart's spread: {'yes' if ok else 'NO'}")
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    env.close()


if __name__ == "__main__":
    main()
