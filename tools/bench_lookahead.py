#!/usr/bin/env python3
"""What policy["lookahead"] costs: ms per 153-day episode of rollout(linear) and rollout(mlp [64, 64]) at 1 048 576
envs on the BASELINE configs[2] workload (weights/linear shape, S = 746, similar_climate_counties=True), with and
without the key, for D = 3 and D = 10, all in one process. The yardstick is the same call without the key in the same
run: it runs the LOOK = false instantiation, whose statements did not change.
Each figure: HIP events around whole episodes on the launch stream (the episode's reset and visiting order included on
both sides), median of --reps after one warm-up episode; the two sides of a ratio are timed back to back. The
parameters are device tensors, so no host-to-device copy of weights sits inside a timed call; the host-side checks of
the policy dict remain on both sides.
usage: python tools/bench_lookahead.py [--envs N] [--days 3 10] [--reps 7]    (needs one ROCm GPU)"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, synth  # noqa: E402


def timed(fn, reps):
    out = []
    for i in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i:
            out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1 << 20)
    ap.add_argument("--days", type=int, nargs="+", default=[3, 10])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    sd = synth.make_synth("linear", years=list(range(2006, 2017)), n_samples=100, seed=args.seed, extra_confounder_fips=60)
    ct = compile_from_synth(sd)
    n = args.envs
    print(f"envs {n}  days {ct.T}  obs columns {ct.n_obs}  S {ct.S}  device {torch.cuda.get_device_name(0)}")
    env = HeatAlertVecEnv(n, tables=ct, similar_climate_counties=True)
    env.reset(seed=0)
    rng = np.random.default_rng(1)
    result = {}
    for D in args.days:
        spec = {"feature": "heat_qi", "days": D}
        W = (rng.standard_normal((1, ct.n_obs + D)) * 0.4).astype(np.float32)
        b = (rng.standard_normal(1) * 0.5).astype(np.float32)
        W, b = torch.as_tensor(W, device=env.device), torch.as_tensor(b, device=env.device)
        lin = dict(kind="linear", weight=W, bias=b, lookahead=spec)
        lin0 = dict(kind="linear", weight=W[:, :ct.n_obs].contiguous(), bias=b)
        dims = [ct.n_obs + D, 64, 64, 1]
        layers = [((rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32),
                   np.zeros(dims[i + 1], np.float32)) for i in range(3)]
        layers = [(torch.as_tensor(Wl, device=env.device), torch.as_tensor(bl, device=env.device)) for Wl, bl in layers]
        mlp = dict(kind="mlp", layers=layers, activation="tanh", lookahead=spec)
        mlp0 = dict(kind="mlp", layers=[(layers[0][0][:, :ct.n_obs].contiguous(), layers[0][1])] + layers[1:], activation="tanh")
        for name, with_key, without in (("linear", lin, lin0), ("mlp64x64", mlp, mlp0)):
            base = timed(lambda: env.rollout(without), args.reps)
            look = timed(lambda: env.rollout(with_key), args.reps)
            print(f"rollout({name:8s}) D={D:<2d}  without {base[0]:8.3f} ms (min {base[1]:.3f}, max {base[2]:.3f})   "
                  f"with {look[0]:8.3f} ms (min {look[1]:.3f}, max {look[2]:.3f})   ratio {look[0] / base[0]:.3f}   "
                  f"kernel {env.last_rollout_kernel}")
            result[f"{name}_D{D}"] = {"without_ms": round(base[0], 4), "with_ms": round(look[0], 4),
                                      "ratio": round(look[0] / base[0], 4)}
    env.close()
    print(json.dumps({"bench": "lookahead", "envs": n, "reps": args.reps, **result}))


if __name__ == "__main__":
    main()
