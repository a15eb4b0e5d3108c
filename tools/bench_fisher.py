#!/usr/bin/env python3
"""ms per call of fisher_vector_product()'s library entry points at 1 048 576 envs over one whole 153-day episode, next to
surrogate_gradient()'s on the same episodes, in one process:
  linear        w2a_fisher_vector_product_linear   against  w2a_surrogate_gradient_linear
  [64,64] tanh  w2a_fisher_vector_product_mlp      against  w2a_surrogate_gradient_mlp
The surrogate call differs only in the first pass (one dot product / one network forward per env-day where the product
runs two / the forward with its tangent; the count, scan, second pass and reduction of the MLP kind are the same
kernels), so it is the yardstick. The schedule is the hindsight optimum of the episodes, the vector a standard normal
draw in the policy's shapes, the surrogate's advantage a standard normal draw and its old_log_prob NULL. Every figure is
the library call alone (preallocated outputs and workspace, HIP events on the launch stream), so the host-side group
mean of the linear kinds is in none of them. The calls alternate inside every repetition; medians, minima and maxima of
--reps after --warmup rounds. There is no pass bar: nobody has measured these before.
usage: python tools/bench_fisher.py [--envs N] [--reps 10] [--warmup 3] [--json PATH]   (one ROCm GPU)"""
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
    dims = [ct.n_obs, 64, 64, 1]
    W = (rng.standard_normal((1, ct.n_obs)) * 0.2).astype(np.float32)
    layers = [((rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32),
               (rng.standard_normal(dims[i + 1]) * 0.3).astype(np.float32)) for i in range(3)]
    lin = policy.check_linear_policy(dict(kind="linear", weight=W, bias=np.zeros(1, np.float32)), ct.n_obs, n, ct.obs_slot, dev)
    mlp = policy.check_mlp_policy(dict(kind="mlp", layers=layers, activation="tanh"), ct.n_obs, n, ct.obs_slot, dev)
    vlin = policy.check_fisher_args("linear", {"weight": rng.standard_normal((1, ct.n_obs)).astype(np.float32),
                                               "bias": rng.standard_normal(1).astype(np.float32)}, lin, ct.n_obs, ct.obs_slot, dev)
    vmlp = policy.check_fisher_args("mlp", {"layers": [(rng.standard_normal(Wl.shape).astype(np.float32),
                                                        rng.standard_normal(bl.shape).astype(np.float32)) for Wl, bl in layers]},
                                    mlp, ct.n_obs, ct.obs_slot, dev)
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
    i32 = lambda: torch.empty(n, dtype=torch.int32, device=dev)  # noqa: E731
    quad, surr, kl, ent, days, clipped = f32(), f32(), f32(), f32(), i32(), i32()
    T = ct.T
    adv = torch.randn((T, n), dtype=torch.float32, device=dev, generator=torch.Generator(dev).manual_seed(0))
    ws = torch.empty(lib.w2a_fisher_vector_product_mlp_workspace_bytes(n, T, 1, mlp.width, mlp.n_layers), dtype=torch.uint8,
                     device=dev)
    assert ws.numel() == lib.w2a_surrogate_gradient_mlp_workspace_bytes(n, T, 1, mlp.width, mlp.n_layers)
    obs = env._obs.data_ptr()
    calls = {
        "surrogate linear": lambda: lib.w2a_surrogate_gradient_linear(
            h, C.byref(lp), mask.data_ptr(), words, None, adv.data_ptr(), T, None, 0, 0.2, 0.0, T, obs, rows.data_ptr(),
            surr.data_ptr(), clipped.data_ptr(), kl.data_ptr(), ent.data_ptr(), days.data_ptr(), None, stream),
        "fisher linear": lambda: lib.w2a_fisher_vector_product_linear(
            h, C.byref(lp), vlin[0].data_ptr(), vlin[1].data_ptr(), mask.data_ptr(), words, None, T, obs, rows.data_ptr(),
            quad.data_ptr(), days.data_ptr(), stream, None, 0),
        "surrogate [64,64] tanh": lambda: lib.w2a_surrogate_gradient_mlp(
            h, C.byref(mp), mask.data_ptr(), words, None, adv.data_ptr(), T, None, 0, 0.2, 0.0, T, obs, blocks.data_ptr(),
            surr.data_ptr(), clipped.data_ptr(), kl.data_ptr(), ent.data_ptr(), days.data_ptr(), None, ws.data_ptr(),
            ws.numel(), stream),
        "fisher [64,64] tanh": lambda: lib.w2a_fisher_vector_product_mlp(
            h, C.byref(mp), vmlp.data_ptr(), mask.data_ptr(), words, None, T, obs, blocks.data_ptr(), quad.data_ptr(),
            days.data_ptr(), ws.data_ptr(), ws.numel(), stream, None, 0),
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
    res = {"envs": n, "days": T, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "ms": {}, "ratio": {}}
    for k, v in ms.items():
        res["ms"][k] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print(f"{k:26s} {statistics.median(v):9.3f} ms/call  (min {min(v):.3f}, max {max(v):.3f}, spread {max(v) - min(v):.3f})")
    for kind in ("linear", "[64,64] tanh"):
        base, mine = ms[f"surrogate {kind}"], ms[f"fisher {kind}"]
        per_rep = [a / b for a, b in zip(mine, base)]  # the two calls of one repetition, back to back
        r = res["ratio"][f"fisher {kind}"] = dict(median=statistics.median(mine) / statistics.median(base), min=min(per_rep),
                                                  max=max(per_rep))
        print(f"fisher {kind:14s} / surrogate = {r['median']:.3f}   (per repetition: min {r['min']:.3f}, max {r['max']:.3f}, "
              f"spread {r['max'] - r['min']:.3f})")
    env.close()
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
