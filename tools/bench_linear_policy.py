#!/usr/bin/env python3
"""ms per 153-day episode of a linear policy at 1 048 576 envs (G parameter rows, random groups), three ways:
  rollout(linear)      k_rollout_linear, the whole episode in one launch (plus the episode's reset and visiting order)
  step loop (graph)    the same policy as `policy(obs) -> step()` recorded into a hipGraph (record_steps), fp64 logits
  rollout(threshold)   the built-in threshold policy on the same batch (k_rollout64 / k_rollout_mfma), for reference
Each figure: HIP events around whole episodes on the launch stream, median of --reps after one warm-up episode.
usage: python tools/bench_linear_policy.py [--envs N] [--groups 1 1024] [--reps 5]    (needs one ROCm GPU)"""
import argparse
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
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 1024])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=20, seed=0, extra_confounder_fips=6)
    ct = compile_from_synth(data)
    n, T = args.envs, ct.T
    print(f"envs {n}  days {T}  obs columns {ct.n_obs}  device {torch.cuda.get_device_name(0)}")
    env = HeatAlertVecEnv(n, tables=ct, similar_climate_counties=True)
    env.reset(seed=0)
    thr = dict(kind="threshold", feature="heat_qi", threshold=0.9, require_budget=True)
    ms = timed(lambda: env.rollout(thr), args.reps)
    print(f"rollout(threshold)            {ms[0]:8.3f} ms/episode  (min {ms[1]:.3f}, max {ms[2]:.3f})  kernel "
          f"{env.last_rollout_kernel}")
    for G in args.groups:
        rng = np.random.default_rng(G)
        W = (rng.standard_normal((G, ct.n_obs)) * 0.4).astype(np.float32)
        b = (rng.standard_normal(G) * 0.5).astype(np.float32)
        g = torch.as_tensor(rng.integers(0, G, n), dtype=torch.int32, device=env.device)
        pol = dict(kind="linear", weight=W, bias=b, group=g)
        ms = timed(lambda: env.rollout(pol), args.reps)
        out = env.rollout(pol)
        print(f"rollout(linear) G={G:<5d}       {ms[0]:8.3f} ms/episode  (min {ms[1]:.3f}, max {ms[2]:.3f})  kernel "
              f"{env.last_rollout_kernel}  alerts/env {float(out['alerts'].float().mean()):.2f}")
        # the same policy as a recorded step() loop (episodes restart inside the step kernel: lockstep=False)
        se = HeatAlertVecEnv(n, tables=ct, similar_climate_counties=True, lockstep=False)
        obs, _ = se.reset(seed=0)
        W64 = torch.as_tensor(W, dtype=torch.float64, device=se.device)[g.long()]
        b64 = torch.as_tensor(b, dtype=torch.float64, device=se.device)[g.long()]
        act = torch.empty(n, dtype=torch.int32, device=se.device)

        def one_day():
            act.copy_((obs.double() * W64).sum(dim=1) + b64 > 0)
            se.step(act)

        rec = se.record_steps(one_day, T)
        ms = timed(rec.replay, args.reps)
        rec.finish()
        print(f"step loop (graph) G={G:<5d}     {ms[0]:8.3f} ms/episode  (min {ms[1]:.3f}, max {ms[2]:.3f})  step kernel "
              f"{se.last_step_kernel}")
        se.close()
    env.close()


if __name__ == "__main__":
    main()
