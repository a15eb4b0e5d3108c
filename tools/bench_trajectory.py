#!/usr/bin/env python3
"""ms per 153-day episode of rollout(record=True) at 1 048 576 envs, G = 1, against the same call without recording:
  linear, [16] tanh and [64, 64] tanh    rollout(pol) and rollout(pol, record=True) on the same batch
  [16] tanh at G = 1024                   groups keep the group-major visiting order: the direct store design
  step loop (graph)                       the linear policy as `policy(obs) -> step()` recorded into a hipGraph that
                                          also copies obs, action, reward and done into preallocated [S, N, .] buffers
plus the bytes each recorded episode writes, the effective write rate, and the box's device-to-device copy rate.
Each figure: HIP events around whole episodes on the launch stream (the call, its reset, the visiting order and, with
record=True, the per-call allocation from torch's cache and the flags -> bool split), median of --reps after one
warm-up episode. Kernel-only times: run under `rocprofv3 --kernel-trace --stats` (profiles/r09/).
usage: python tools/bench_trajectory.py [--envs N] [--reps 5] [--no-loop]    (needs one ROCm GPU)"""
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


def net(n_obs, hidden, seed):
    rng = np.random.default_rng(seed)
    dims = [n_obs] + list(hidden) + [2]
    return [((rng.standard_normal((dims[i + 1], dims[i])) * (1.5 / np.sqrt(dims[i]))).astype(np.float32),
             (rng.standard_normal(dims[i + 1]) * 0.5).astype(np.float32)) for i in range(len(dims) - 1)]


def copy_rate():
    """GB/s of a 4 GiB device-to-device copy, counting the bytes written (read + write = twice that)."""
    src = torch.empty(1 << 30, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    ms = timed(lambda: dst.copy_(src), 5)[0]
    del src, dst
    return 4 * (1 << 30) / ms / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-loop", action="store_true", help="skip the recorded step-loop baseline")
    args = ap.parse_args()
    data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=20, seed=0, extra_confounder_fips=6)
    ct = compile_from_synth(data)
    n, T = args.envs, ct.T
    per_day = 4 * ct.n_obs + 4 + 4 + 1 + 1
    traj_bytes = T * n * per_day + n * ct.n_obs * 4
    print(f"envs {n}  days {T}  obs columns {ct.n_obs}  device {torch.cuda.get_device_name(0)}")
    rate = copy_rate()
    print(f"copy rate (4 GiB d2d)         {rate:8.0f} GB/s written ({2 * rate:.0f} GB/s read + write)")
    print(f"trajectory bytes / episode    {traj_bytes / 1e9:8.2f} GB  ({per_day} B per env-day + one obs slab)")
    rng = np.random.default_rng(1)
    W = (rng.standard_normal((1, ct.n_obs)) * 0.4).astype(np.float32)
    b = (rng.standard_normal(1) * 0.5).astype(np.float32)
    pols = [("linear", dict(kind="linear", weight=W, bias=b, sample=True, seed=3))]
    for hidden in ((16,), (64, 64)):
        pols.append((f"{list(hidden)} tanh".replace(" ", ""), dict(kind="mlp", layers=net(ct.n_obs, hidden, 2),
                                                                      activation="tanh", sample=True, seed=3)))
    g1024 = torch.as_tensor(np.random.default_rng(2).integers(0, 1024, n), dtype=torch.int32, device="cuda")
    layers = [(np.repeat(W_[None], 1024, axis=0), np.repeat(b_[None], 1024, axis=0)) for W_, b_ in net(ct.n_obs, (16,), 2)]
    pols.append(("[16]tanh G=1024", dict(kind="mlp", layers=layers, activation="tanh", group=g1024, sample=True, seed=3)))
    for name, pol in pols:
        env = HeatAlertVecEnv(n, tables=ct, similar_climate_counties=True)
        env.reset(seed=0)
        plain = timed(lambda: env.rollout(pol), args.reps)
        rec = timed(lambda: env.rollout(pol, record=True), args.reps)
        extra = rec[0] - plain[0]
        print(f"{name:16s} plain  {plain[0]:8.3f} ms/episode  (min {plain[1]:.3f})   record {rec[0]:8.3f} ms/episode "
              f"(min {rec[1]:.3f})   +{extra:.3f} ms  x{rec[0] / plain[0]:.2f}   "
              f"{traj_bytes / rec[0] / 1e6:6.0f} GB/s over the recorded call, "
              f"{traj_bytes / max(extra, 1e-3) / 1e6:6.0f} GB/s over the extra time")
        env.close()
        torch.cuda.empty_cache()
    if args.no_loop:
        return
    # the same linear policy (deterministic here: the loop has no in-kernel uniform) as a recorded step loop that
    # collects the trajectory into preallocated buffers
    se = HeatAlertVecEnv(n, tables=ct, similar_climate_counties=True, lockstep=False)
    obs, _ = se.reset(seed=0)
    W64 = torch.as_tensor(W, dtype=torch.float64, device=se.device)[0]
    b64 = float(b[0])
    act = torch.empty(n, dtype=torch.uint8, device=se.device)
    bo = torch.empty((T + 1, n, ct.n_obs), dtype=torch.float32, device=se.device)
    ba = torch.empty((T, n), dtype=torch.uint8, device=se.device)
    br = torch.empty((T, n), dtype=torch.float32, device=se.device)
    bd = torch.empty((T, n), dtype=torch.bool, device=se.device)
    day = [0]

    def one_day():
        s = day[0] % T
        day[0] += 1
        bo[s].copy_(obs)
        torch.gt((obs.double() * W64).sum(dim=1) + b64, 0, out=bd[s])
        act.copy_(bd[s])
        _, r, d, _, _ = se.step(act)
        ba[s].copy_(act)
        br[s].copy_(r)
        bd[s].copy_(d)

    rec = se.record_steps(one_day, T)
    ms = timed(rec.replay, args.reps)
    rec.finish()
    print(f"step loop (graph) + copies    {ms[0]:8.3f} ms/episode  (min {ms[1]:.3f}, max {ms[2]:.3f})  step kernel "
          f"{se.last_step_kernel}")
    se.close()


if __name__ == "__main__":
    main()
