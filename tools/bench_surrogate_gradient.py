#!/usr/bin/env python3
"""ms per call of surrogate_gradient()'s library entry points at 1 048 576 envs over one whole 153-day episode, next to
the weighted imitation calls at the same shape, in one process:
  linear        w2a_surrogate_gradient_linear (log_prob off / on)   against  w2a_imitation_gradient_linear_weighted
  [64,64] tanh  w2a_surrogate_gradient_mlp    (log_prob off / on)   against  w2a_imitation_gradient_mlp_weighted
The difference is one more 4-B stream per env-day (old_log_prob, next to the advantage both read), the fp64 ratio, clip
test and entropy terms per scored day, and the log_prob stores. The schedule is the hindsight optimum of the episodes,
the advantage a standard normal draw, old_log_prob the log_prob output of the same policy moved by 5 % -- so that a
share of the days is clipped, printed with the timings. Every figure is the library call alone (preallocated outputs
and workspace, HIP events on the launch stream), so the host-side group mean of the linear kinds is in none of them.
The calls alternate inside every repetition; medians, minima and maxima of --reps after --warmup rounds. There is no
pass bar: nobody has measured these before.
usage: python tools/bench_surrogate_gradient.py [--envs N] [--reps 10] [--warmup 3] [--json PATH]   (one ROCm GPU)"""
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
    ap.add_argument("--clip", type=float, default=0.2)
    ap.add_argument("--entropy-coef", type=float, default=0.01)
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

    def structs(scale):
        """(LinearPolicy, MlpPolicy, the checked policies that own the device memory) of the parameters times `scale`"""
        lin = policy.check_linear_policy(dict(kind="linear", weight=W * scale, bias=np.zeros(1, np.float32)), ct.n_obs, n,
                                         ct.obs_slot, dev)
        mlp = policy.check_mlp_policy(dict(kind="mlp", layers=[(Wl * scale, bl * scale) for Wl, bl in layers],
                                           activation="tanh"), ct.n_obs, n, ct.obs_slot, dev)
        lp = _ffi.LinearPolicy()
        lp.weight, lp.bias, lp.group = lin.weight_slots.data_ptr(), lin.bias.data_ptr(), None
        lp.n_groups, lp.sample, lp.require_budget, lp.seed = 1, 0, 0, 0
        mp = _ffi.MlpPolicy()
        mp.params, mp.group, mp.order = mlp.params.data_ptr(), None, None
        mp.n_groups, mp.n_layers, mp.width, mp.activation = 1, mlp.n_layers, mlp.width, _ffi.MLP_ACTIVATIONS["tanh"]
        mp.sample, mp.require_budget, mp.seed = 0, 0, 0
        return lp, mp, (lin, mlp)

    lp, mp, keep = structs(np.float32(1.0))
    mlp = keep[1]
    rows = torch.empty((ct.n_obs + 1, n), dtype=torch.float32, device=dev)
    blocks = torch.empty((1, policy.mlp_stride(mlp.width, mlp.n_layers)), dtype=torch.float32, device=dev)
    f32 = lambda: torch.empty(n, dtype=torch.float32, device=dev)  # noqa: E731
    i32 = lambda: torch.empty(n, dtype=torch.int32, device=dev)  # noqa: E731
    ll, surr, kl, ent, days, clipped = f32(), f32(), f32(), f32(), i32(), i32()
    T = ct.T
    adv = torch.randn((T, n), dtype=torch.float32, device=dev, generator=torch.Generator(dev).manual_seed(0))
    old = {k: torch.empty((T, n), dtype=torch.float32, device=dev) for k in ("linear", "mlp")}
    lp_out = torch.empty((T, n), dtype=torch.float32, device=dev)
    ws = torch.empty(lib.w2a_surrogate_gradient_mlp_workspace_bytes(n, T, 1, mlp.width, mlp.n_layers), dtype=torch.uint8,
                     device=dev)
    assert ws.numel() == lib.w2a_imitation_gradient_mlp_workspace_bytes(n, T, 1, mlp.width, mlp.n_layers)
    obs = env._obs.data_ptr()
    clip, beta = args.clip, args.entropy_coef

    def sg_lin(pol, oldp, out):
        return lambda: lib.w2a_surrogate_gradient_linear(
            h, C.byref(pol), mask.data_ptr(), words, None, adv.data_ptr(), T, oldp, T if oldp else 0, clip, beta, T, obs,
            rows.data_ptr(), surr.data_ptr(), clipped.data_ptr(), kl.data_ptr(), ent.data_ptr(), days.data_ptr(), out, stream)

    def sg_mlp(pol, oldp, out):
        return lambda: lib.w2a_surrogate_gradient_mlp(
            h, C.byref(pol), mask.data_ptr(), words, None, adv.data_ptr(), T, oldp, T if oldp else 0, clip, beta, T, obs,
            blocks.data_ptr(), surr.data_ptr(), clipped.data_ptr(), kl.data_ptr(), ent.data_ptr(), days.data_ptr(), out,
            ws.data_ptr(), ws.numel(), stream)

    # epoch 0 under the policy moved by 5 %: the old log-probabilities of the timed calls
    lp_old, mp_old, keep_old = structs(np.float32(1.05))
    share = {}
    with torch.cuda.device(dev):
        _ffi.check(sg_lin(lp_old, None, old["linear"].data_ptr())(), "epoch 0 linear")
        _ffi.check(sg_mlp(mp_old, None, old["mlp"].data_ptr())(), "epoch 0 mlp")
        for k, fn in (("linear", sg_lin(lp, old["linear"].data_ptr(), None)), ("[64,64] tanh", sg_mlp(mp, old["mlp"].data_ptr(), None))):
            _ffi.check(fn(), k)
            share[k] = float(clipped.sum()) / max(float(days.sum()), 1.0)
    del keep_old
    print("clipped share of the scored days: " + ", ".join(f"{k} {v:.3f}" for k, v in share.items()))
    calls = {
        "imitation weighted linear": lambda: lib.w2a_imitation_gradient_linear_weighted(
            h, C.byref(lp), mask.data_ptr(), words, None, adv.data_ptr(), T, T, obs, rows.data_ptr(), ll.data_ptr(),
            days.data_ptr(), stream),
        "surrogate linear": sg_lin(lp, old["linear"].data_ptr(), None),
        "surrogate linear + log_prob": sg_lin(lp, old["linear"].data_ptr(), lp_out.data_ptr()),
        "imitation weighted [64,64] tanh": lambda: lib.w2a_imitation_gradient_mlp_weighted(
            h, C.byref(mp), mask.data_ptr(), words, None, adv.data_ptr(), T, T, obs, blocks.data_ptr(), ll.data_ptr(),
            days.data_ptr(), ws.data_ptr(), ws.numel(), stream),
        "surrogate [64,64] tanh": sg_mlp(mp, old["mlp"].data_ptr(), None),
        "surrogate [64,64] tanh + log_prob": sg_mlp(mp, old["mlp"].data_ptr(), lp_out.data_ptr()),
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
    res = {"envs": n, "days": T, "reps": args.reps, "warmup": args.warmup, "clip": clip, "entropy_coef": beta,
           "clipped_share": share, "device": torch.cuda.get_device_name(0), "ms": {}, "ratio": {}}
    for k, v in ms.items():
        res["ms"][k] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print(f"{k:34s} {statistics.median(v):9.3f} ms/call  (min {min(v):.3f}, max {max(v):.3f}, spread {max(v) - min(v):.3f})")
    for kind in ("linear", "[64,64] tanh"):
        base = ms[f"imitation weighted {kind}"]
        for name in (f"surrogate {kind}", f"surrogate {kind} + log_prob"):
            per_rep = [a / b for a, b in zip(ms[name], base)]  # the two calls of one repetition, back to back
            res["ratio"][name] = dict(median=statistics.median(ms[name]) / statistics.median(base), min=min(per_rep),
                                      max=max(per_rep))
            r = res["ratio"][name]
            print(f"{name:34s} / imitation weighted = {r['median']:.3f}   (per repetition: min {r['min']:.3f}, "
                  f"max {r['max']:.3f}, spread {r['max'] - r['min']:.3f})")
    env.close()
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
