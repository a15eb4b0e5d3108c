#!/usr/bin/env python3
"""ms per 153-day episode of a sampled MLP policy at 1 048 576 envs, for [16] tanh, [64, 64] tanh and [64, 64] ReLU at
G = 1 and G = 1024 parameter blocks (group = env id // (N / G)), three ways:
  (a) rollout(mlp, sample=True)                      the plain rollout (k_rollout_mlp)
  (b) the same with policy_gradient="none"           k_pgm_pass1 / k_pgm_pass2 / k_pgm_reduce + k_rollout_mlp
  (c) rollout(record=True) + the same estimator ("none" baseline) by torch autograd in f32 on the recorded rows, in
      chunks of days (the recorded observations alone are 126 B per env-day)
Each figure: HIP events around whole calls on the launch stream, in one process; the variants alternate inside every
repetition, medians of --reps after one warm-up round. The kernels of one repetition without (c):
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_policy_gradient_mlp.py --reps 2 --skip-torch
usage: python tools/bench_policy_gradient_mlp.py [--envs N] [--groups 1 1024] [--reps 5] [--skip-torch]   (one ROCm GPU)"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from weather2alert_amd import HeatAlertVecEnv, _ffi, compile_from_synth, policy, synth  # noqa: E402

NETS = {"[16] tanh": ((16,), "tanh"), "[64,64] tanh": ((64, 64), "tanh"), "[64,64] relu": ((64, 64), "relu")}


def torch_estimator(out, layers, act, g, G, chunk=16):
    """autograd of sum Q_s log pi(a_s | o_s) / N_g over the recorded trajectory, f32, `chunk` days at a time"""
    tr = out["trajectory"]
    valid = tr["valid"]
    adv = torch.where(valid, tr["reward"], torch.zeros_like(tr["reward"]))
    q = torch.flip(torch.cumsum(torch.flip(adv, [0]), 0), [0])
    P = [(W.clone().requires_grad_(), b.clone().requires_grad_()) for W, b in layers]
    gi = torch.zeros(valid.shape[1], dtype=torch.long, device=valid.device) if g is None else g.long()
    cnt = torch.bincount(gi, minlength=G).float()
    f = torch.tanh if act == "tanh" else torch.relu
    for s0 in range(0, valid.shape[0], chunk):
        sl = slice(s0, min(s0 + chunk, valid.shape[0]))
        h = tr["obs"][sl]
        for W, b in P[:-1]:
            h = f(torch.einsum("snj,nuj->snu", h, W[gi]) + b[gi][None]) if G > 1 else f(h @ W[0].T + b[0])
        Wo, bo = P[-1]
        z = (h * Wo[gi][None, :, 0]).sum(-1) + bo[gi][None, :, 0] if G > 1 else h @ Wo[0, 0] + bo[0, 0]
        lp = policy.action_log_prob(z, tr["action"][sl])
        (q[sl] * torch.where(valid[sl], lp, torch.zeros_like(lp)) / cnt[gi][None]).sum().backward()
    return [(W.grad, b.grad) for W, b in P]


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
    lib = _ffi.load(build_if_missing=False)
    for name, (hidden, act) in NETS.items():
        for G in args.groups:
            rng = np.random.default_rng(G)
            dims = [ct.n_obs] + list(hidden) + [1]
            layers = [(torch.as_tensor((rng.standard_normal((G, dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32), device=env.device),
                       torch.as_tensor((rng.standard_normal((G, dims[i + 1])) * 0.3).astype(np.float32), device=env.device))
                      for i in range(len(dims) - 1)]
            g = (torch.arange(n, device=env.device) // max(n // G, 1)).clamp_max(G - 1).to(torch.int32) if G > 1 else None
            pol = dict(kind="mlp", layers=layers, activation=act, sample=True, seed=1)
            if g is not None:
                pol["group"] = g
            keep = {}
            variants = {"(a) rollout": lambda: env.rollout(pol),
                        "(b) policy_gradient=none": lambda: keep.__setitem__("b", env.rollout(pol, policy_gradient="none")["policy_gradient"])}
            if not args.skip_torch:
                variants["(c) record + torch autograd"] = lambda: keep.__setitem__(
                    "c", torch_estimator(env.rollout(pol, record=True), layers, act, g, G))
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
            w = policy.mlp_width(hidden)
            ws = lib.w2a_policy_gradient_mlp_workspace_bytes(n, ct.T, G, w, len(hidden))
            for k, v in ms.items():
                print(f"{name:13s} G={G:<5d} {k:32s} {statistics.median(v):9.3f} ms/episode  (min {min(v):.3f}, max {max(v):.3f})")
            a, b = statistics.median(ms["(a) rollout"]), statistics.median(ms["(b) policy_gradient=none"])
            line = f"{name:13s} G={G:<5d} (b) - (a) = {b - a:.3f} ms   workspace {ws / 2**20:.0f} MiB (pass 1's scratch {9 * n * ct.T / 2**20:.0f})"
            if not args.skip_torch:
                line += f"   (c) / (b) = {statistics.median(ms['(c) record + torch autograd']) / b:.2f}x"
            print(line)
            keep.clear()
            torch.cuda.empty_cache()
    env.close()


if __name__ == "__main__":
    main()
