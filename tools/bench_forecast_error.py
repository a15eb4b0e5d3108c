#!/usr/bin/env python3
"""What the forecast error of policy["lookahead"] costs: ms per 153-day episode of rollout(linear) and
rollout(mlp [64, 64]) at 1 048 576 envs on the BASELINE configs[2] workload (weights/linear shape, S = 746,
similar_climate_counties=True), for D = 3 and D = 10, with the lookahead key alone and with "error" added, all in one
process. The yardstick is the same lookahead policy without "error" in the same run: it runs the LOOK instantiation,
whose statements did not change. What "error" adds per env-day is ceil(D / 2) 64-bit hashes, D f32 fmas and selects.
Measured as tools/bench_lookahead.py measures: HIP events around whole episodes on the launch stream (the episode's
reset and visiting order included on both sides), median of --reps after one warm-up episode, the two sides of a ratio
back to back, parameters as device tensors.
usage: python tools/bench_forecast_error.py [--envs N] [--days 3 10] [--reps 7]    (needs one ROCm GPU)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_lookahead import timed  # noqa: E402
from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, synth  # noqa: E402


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
        noisy = dict(spec, error=[0.03 * (2.0 + 0.5 * k) for k in range(1, D + 1)], error_seed=1)
        W = torch.as_tensor((rng.standard_normal((1, ct.n_obs + D)) * 0.4).astype(np.float32), device=env.device)
        b = torch.as_tensor((rng.standard_normal(1) * 0.5).astype(np.float32), device=env.device)
        dims = [ct.n_obs + D, 64, 64, 1]
        layers = [((rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32),
                   np.zeros(dims[i + 1], np.float32)) for i in range(3)]
        layers = [(torch.as_tensor(Wl, device=env.device), torch.as_tensor(bl, device=env.device)) for Wl, bl in layers]
        for name, pol in (("linear", dict(kind="linear", weight=W, bias=b)),
                          ("mlp64x64", dict(kind="mlp", layers=layers, activation="tanh"))):
            base = timed(lambda: env.rollout(dict(pol, lookahead=spec)), args.reps)
            err = timed(lambda: env.rollout(dict(pol, lookahead=noisy)), args.reps)
            print(f"rollout({name:8s}) D={D:<2d}  lookahead {base[0]:8.3f} ms (min {base[1]:.3f}, max {base[2]:.3f})   "
                  f"with error {err[0]:8.3f} ms (min {err[1]:.3f}, max {err[2]:.3f})   ratio {err[0] / base[0]:.3f}   "
                  f"kernel {env.last_rollout_kernel}")
            result[f"{name}_D{D}"] = {"without_ms": round(base[0], 4), "with_ms": round(err[0], 4),
                                      "ratio": round(err[0] / base[0], 4)}
    env.close()
    print(json.dumps({"bench": "forecast_error", "envs": n, "reps": args.reps, **result}))


if __name__ == "__main__":
    main()
