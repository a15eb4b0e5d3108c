#!/usr/bin/env python3
"""ms per 153-day episode of a sampled linear policy at 1 048 576 envs (G parameter rows, random groups), three ways:
  (a) rollout(linear, sample=True)                 the plain rollout (k_rollout_linear)
  (b) the same with policy_gradient="none" / "no_alert"   k_policy_gradient_linear + k_rollout_linear + the group mean
  (c) rollout(record=True) + the estimator in torch on the recorded tensors, "none" baseline, closed form (no autograd):
      the only route to the same numbers without the keyword
Each figure: HIP events around whole calls on the launch stream, in one process; the variants alternate inside every
repetition (a, b-none, b-no_alert, c, a, ...), medians of --reps after one warm-up round. (c) - (a) and (b) - (a) are the
prices of the two gradient routes. The kernels of one repetition without (c):
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_policy_gradient.py --reps 2 --skip-torch
usage: python tools/bench_policy_gradient.py [--envs N] [--groups 1 1024] [--reps 5] [--skip-torch]   (one ROCm GPU)"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, policy, synth  # noqa: E402


def torch_estimator(out, g, G):
    """the "none"-baseline estimator from a recorded trajectory: recorded logits, f32, one pass over the rows"""
    tr = out["trajectory"]
    valid = tr["valid"]
    delta = torch.where(valid, tr["action"].float() - torch.sigmoid(tr["logit"]), torch.zeros_like(tr["logit"]))
    adv = torch.where(valid, tr["reward"], torch.zeros_like(tr["reward"]))
    q = torch.flip(torch.cumsum(torch.flip(adv, [0]), 0), [0])
    c = delta * q
    per_env = torch.cat([torch.einsum("sn,snj->nj", c, tr["obs"][:-1]), c.sum(0)[:, None]], dim=1)
    return policy.group_mean_columns(per_env.T.contiguous(), g, G)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1 << 20)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true", help="leave route (c) out (profiling runs)")
    args = ap.parse_args()
    data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=20, seed=0, extra_confounder_fips=6)
    ct = compile_from_synth(data)
    n = args.envs
    print(f"envs {n}  days {ct.T}  obs columns {ct.n_obs}  device {torch.cuda.get_device_name(0)}")
    env = HeatAlertVecEnv(n, tables=ct, similar_climate_counties=True)
    env.reset(seed=0)
    for G in args.groups:
        rng = np.random.default_rng(G)
        W = (rng.standard_normal((G, ct.n_obs)) * 0.4).astype(np.float32)
        b = (rng.standard_normal(G) * 0.5).astype(np.float32)
        g = torch.as_tensor(rng.integers(0, G, n), dtype=torch.int32, device=env.device) if G > 1 else None
        pol = dict(kind="linear", weight=W, bias=b, sample=True, seed=1)
        if g is not None:
            pol["group"] = g
        keep = {}

        def c_route():
            keep["c"] = torch_estimator(env.rollout(pol, record=True), g, G)

        def b_route(bl):
            keep[bl] = env.rollout(pol, policy_gradient=bl)["policy_gradient"]

        variants = {"(a) rollout": lambda: env.rollout(pol),
                    "(b) policy_gradient=none": lambda: b_route("none"),
                    "(b) policy_gradient=no_alert": lambda: b_route("no_alert")}
        if not args.skip_torch:
            variants["(c) record + torch, none"] = c_route
        ms = {k: [] for k in variants}
        for rep in range(args.reps + 1):
            for k, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if rep:
                    ms[k].append(e0.elapsed_time(e1))
        for k, v in ms.items():
            print(f"G={G:<5d} {k:32s} {statistics.median(v):9.3f} ms/episode  (min {min(v):.3f}, max {max(v):.3f})")
        a = statistics.median(ms["(a) rollout"])
        bn = statistics.median(ms["(b) policy_gradient=none"])
        print(f"G={G:<5d} price of the gradient (b none) - (a): {bn - a:.3f} ms; "
              f"(b no_alert) - (a): {statistics.median(ms['(b) policy_gradient=no_alert']) - a:.3f} ms")
        if not args.skip_torch:
            c = statistics.median(ms["(c) record + torch, none"])
            print(f"G={G:<5d} (c) / (b none) = {c / bn:.2f}x")
            # the two routes estimate the same thing on different episodes (the env restarts between calls); on equal
            # episodes they are compared by tests/test_policy_gradient_gpu.py
            print(f"G={G:<5d} |g| (b none) {float(keep['none']['weight'].norm()):.4e}   (c) {float(keep['c'][:, :-1].norm()):.4e}")
        keep.clear()
        torch.cuda.empty_cache()
    env.close()


if __name__ == "__main__":
    main()
