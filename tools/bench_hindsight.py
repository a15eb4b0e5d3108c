#!/usr/bin/env python3
"""The hindsight optimum at 1 048 576 envs on bench.py's configs[2] tables (similar_climate_counties=True), one whole
episode from reset:
  hindsight_optimum()       w2a_hindsight_optimum end to end (plan, histogram to the host, counting sort, one DP launch
                            per budget bin), HIP events, median of --reps after one warm-up
  rollout(linear)           one episode without and with hindsight=True
and the distribution of DP states per day ((U + 1)(U + 4) / 2, U = min(budget - used, H)) over the envs. The DP kernels'
own time comes from a run under `rocprofv3 --kernel-trace --stats` (k_hs_dp<false> / <true>).
usage: python tools/bench_hindsight.py [--envs N] [--reps 5]    (needs one ROCm GPU)"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, synth  # noqa: E402

TARGET_MS = 20.0


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
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    sd = synth.make_synth("linear", years=list(range(2006, 2017)), n_samples=100, seed=0, extra_confounder_fips=60)
    ct = compile_from_synth(sd)
    n, T = args.envs, ct.T
    print(f"envs {n}  days {T}  device {torch.cuda.get_device_name(0)}")
    env = HeatAlertVecEnv(n, tables=ct, similar_climate_counties=True, autoreset="disabled")
    env.reset(seed=0)
    st0 = {k: v.clone() for k, v in env.state().items()}

    U = np.minimum(np.maximum(st0["budget"].cpu().numpy() - st0["used"].cpu().numpy(), 0),
                   st0["n_days"].cpu().numpy() - st0["t"].cpu().numpy()).astype(np.int64)
    ns = (U + 1) * (U + 4) // 2
    H = (st0["n_days"] - st0["t"]).cpu().numpy().astype(np.int64)
    evals = int((H * ns).sum())  # states x days, each with one or two actions
    print(f"U = budget - used: min {U.min()}  mean {U.mean():.2f}  max {U.max()}")
    print(f"states per day: mean {ns.mean():.1f}  p50 {int(np.median(ns))}  p90 {int(np.percentile(ns, 90))}  "
          f"max {ns.max()}  (64-lane chunks per day: mean {np.mean((ns + 63) // 64):.2f}, lane use "
          f"{ns.sum() / (64 * ((ns + 63) // 64)).sum():.1%})")
    hist = np.bincount(U)
    print("envs per U: " + "  ".join(f"{u}:{c}" for u, c in enumerate(hist) if c))
    print(f"state-days {evals:.3e}")

    ms = timed(lambda: env.hindsight_optimum(st0), args.reps)
    verdict = "meets" if ms[0] <= TARGET_MS else "misses"
    print(f"hindsight_optimum()        {ms[0]:8.3f} ms/episode  (min {ms[1]:.3f}, max {ms[2]:.3f})  {verdict} the "
          f"<= {TARGET_MS:.0f} ms target;  {evals / ms[0] / 1e6:.2f} G state-days/s")
    hs = env.hindsight_optimum(st0)
    print(f"mean optimum {hs['return'].double().mean().item():.4f}  mean alerts {hs['alerts'].double().mean().item():.3f}")

    rng = np.random.default_rng(1)
    W = (rng.standard_normal((1, ct.n_obs)) * 0.4).astype(np.float32)
    W[:, ct.feature_names.index("remaining_budget")] *= 0.1
    pol = dict(kind="linear", weight=W, bias=np.asarray([-0.5], np.float32))

    def ro(hindsight):
        env.reset(seed=0)
        return env.rollout(pol, hindsight=hindsight)

    ms0 = timed(lambda: ro(False), args.reps)
    ms1 = timed(lambda: ro(True), args.reps)
    print(f"reset + rollout(linear)            {ms0[0]:8.3f} ms  (min {ms0[1]:.3f}, max {ms0[2]:.3f})")
    print(f"reset + rollout(linear, hindsight) {ms1[0]:8.3f} ms  (min {ms1[1]:.3f}, max {ms1[2]:.3f})  "
          f"+{ms1[0] - ms0[0]:.3f} ms")
    out = ro(True)
    regret = (out["hindsight_return"].double() - out["return"].double())
    print(f"linear policy: mean return {out['return'].double().mean().item():.4f}  mean regret "
          f"{regret.mean().item():.4f}  min regret {regret.min().item():.3e}")
    env.close()


if __name__ == "__main__":
    main()
