#!/usr/bin/env python3
"""Returns under every posterior draw at 1 048 576 envs on BASELINE configs[2]'s synthetic tables (n_samples = 100):
  kernel               w2a_posterior_returns alone on one episode's start state and alert bitmap (k_posterior_returns)
  rollout(linear)      one 153-day episode of a greedy linear policy, without and with posterior_returns=True
  forced-draw replay   what a user does without it: K resets with explicit episode tuples (sample = k), K rollouts
Each figure: HIP events around the work on the launch stream, median of --reps after one warm-up (the replay: --replay-reps).
usage: python tools/bench_posterior_returns.py [--envs N] [--reps 5] [--replay-reps 1]    (needs one ROCm GPU)"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--replay-reps", type=int, default=1)
    args = ap.parse_args()
    sd = synth.make_synth("linear", years=list(range(2006, 2017)), n_samples=100, seed=0, extra_confounder_fips=60)
    ct = compile_from_synth(sd)
    n, T, K = args.envs, ct.T, ct.n_samples
    print(f"envs {n}  days {T}  draws {K}  device {torch.cuda.get_device_name(0)}")
    rng = np.random.default_rng(1)
    W = (rng.standard_normal((1, ct.n_obs)) * 0.4).astype(np.float32)
    W[:, ct.feature_names.index("remaining_budget")] *= 0.1
    pol = dict(kind="linear", weight=W, bias=np.asarray([-0.5], np.float32))
    env = HeatAlertVecEnv(n, tables=ct, similar_climate_counties=True)  # lock step, same_step autoreset
    env.reset(seed=0)

    # the kernel alone, on one episode's start state and bitmap
    st0 = {k: v.clone() for k, v in env.state().items()}
    out = env.rollout(pol, alert_mask=True)
    words = (T + 31) // 32
    bits = out["alert_days"].to(torch.int32)
    bits = torch.nn.functional.pad(bits, (0, words * 32 - T)).view(n, words, 32)
    mask = (bits << torch.arange(32, dtype=torch.int32, device=env.device)).sum(-1, dtype=torch.int32).contiguous()
    ms = timed(lambda: env._posterior_returns_packed(st0, mask, words, T), args.reps)
    fma = n * T * K * 60
    print(f"kernel k_posterior_returns      {ms[0]:8.3f} ms/episode  (min {ms[1]:.3f}, max {ms[2]:.3f})  "
          f"{2 * fma / ms[0] / 1e9:.1f} fp64 TFLOP/s of useful FMAs (spec peak 78.6)")

    # end to end: the rollout with and without the per-draw returns (consecutive episodes of the lock-step batch)
    ms0 = timed(lambda: env.rollout(pol), args.reps)
    ms1 = timed(lambda: env.rollout(pol, posterior_returns=True), args.reps)
    print(f"rollout(linear)                 {ms0[0]:8.3f} ms/episode  (min {ms0[1]:.3f}, max {ms0[2]:.3f})  kernel "
          f"{env.last_rollout_kernel}")
    print(f"rollout(linear, posterior)      {ms1[0]:8.3f} ms/episode  (min {ms1[1]:.3f}, max {ms1[2]:.3f})  "
          f"+{ms1[0] - ms0[0]:.3f} ms")
    env.close()

    # the K forced-draw replay: reset every env to its episode with sample = k, roll out, K times
    rp = HeatAlertVecEnv(n, tables=ct, similar_climate_counties=True, autoreset="disabled")
    rp.reset(seed=0)
    s = {k: v.clone() for k, v in rp.state().items()}
    tup = {k: s[k].cpu().numpy() for k in ("county_w", "year_i", "coef_col", "budget")}
    R = torch.empty((n, K), dtype=torch.float32, device=rp.device)

    def replay():
        for k in range(K):
            rp.reset(options={"episodes": dict(tup, sample=np.full(n, k, np.int32))})
            R[:, k] = rp.rollout(pol)["return"]

    msr = timed(replay, args.replay_reps)
    print(f"forced-draw replay (K={K})     {msr[0]:8.3f} ms/episode  (min {msr[1]:.3f}, max {msr[2]:.3f})  "
          f"{msr[0] / ms1[0]:.1f}x the rollout with posterior_returns")
    # the replay and the kernel agree (the replay's rollouts run the same linear kernel on the same bitmaps)
    rp.reset(options={"episodes": dict(tup, sample=s["sample"].cpu().numpy())})
    o = rp.rollout(pol, posterior_returns=True)
    diff = (o["posterior_returns"].double() - R.double()).abs().max().item()
    print(f"max |posterior_returns - forced-draw replay| = {diff:.3e}  (bit-identical: {bool(diff == 0.0)})")
    rp.close()


if __name__ == "__main__":
    main()
