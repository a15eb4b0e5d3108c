#!/usr/bin/env python3
"""ms per 153-day episode of MLP policies at 1 048 576 envs (G parameter blocks, random groups), three ways:
  rollout(mlp)         k_rollout_mlp, the whole episode in one launch (plus the episode's reset and visiting order)
  step loop (graph)    the same network in fp32 torch as `policy(obs) -> step()` recorded into a hipGraph (record_steps);
                       torch's best case: each group's envs contiguous, one batched matmul per layer
  rollout(linear)      k_rollout_linear on the same batch, for reference
for [64, 64] tanh, [64, 64] ReLU and [16] tanh, each at G = 1 and G = 1024. Each figure: HIP events around whole
episodes on the launch stream, median of --reps after one warm-up episode.
usage: python tools/bench_mlp_policy.py [--envs N] [--groups 1 1024] [--reps 5] [--no-torch]   (needs one ROCm GPU)"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, synth  # noqa: E402

NETS = [((64, 64), "tanh"), ((64, 64), "relu"), ((16,), "tanh")]


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


def net(n_obs, hidden, G, scale, seed):
    rng = np.random.default_rng(seed)
    dims = [n_obs] + list(hidden) + [2]
    layers = []
    for i in range(len(dims) - 1):
        W = rng.standard_normal((G, dims[i + 1], dims[i])) * (1.5 / np.sqrt(dims[i]))
        if i == 0:
            W = W / scale[None, None, :]
        layers.append((W.astype(np.float32), (rng.standard_normal((G, dims[i + 1])) * 0.5).astype(np.float32)))
    return layers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1 << 20)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch step loops (kernel-only profiling runs)")
    args = ap.parse_args()
    data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=20, seed=0, extra_confounder_fips=6)
    ct = compile_from_synth(data)
    n, T = args.envs, ct.T
    print(f"envs {n}  days {T}  obs columns {ct.n_obs}  device {torch.cuda.get_device_name(0)}")
    env = HeatAlertVecEnv(n, tables=ct, similar_climate_counties=True)
    env.reset(seed=0)
    scale = env._obs.std(dim=0).clamp_min(0.1).cpu().numpy().astype(np.float64)
    for G in args.groups:
        rng = np.random.default_rng(G)
        g = torch.as_tensor(rng.integers(0, G, n), dtype=torch.int32, device=env.device)
        W = (rng.standard_normal((G, ct.n_obs)) * 0.4 / scale).astype(np.float32)
        b = (rng.standard_normal(G) * 0.5).astype(np.float32)
        lin = dict(kind="linear", weight=W, bias=b, group=g)
        ms_lin = timed(lambda: env.rollout(lin), args.reps)
        print(f"rollout(linear)        G={G:<5d} {ms_lin[0]:8.3f} ms/episode  (min {ms_lin[1]:.3f}, max {ms_lin[2]:.3f})")
        for hidden, act in NETS:
            name = f"[{','.join(map(str, hidden))}] {act}"
            layers = net(ct.n_obs, hidden, G, scale, seed=G + len(hidden))
            pol = dict(kind="mlp", layers=layers, activation=act, group=g)
            ms = timed(lambda: env.rollout(pol), args.reps)
            out = env.rollout(pol)
            print(f"rollout(mlp) {name:12s} G={G:<5d} {ms[0]:8.3f} ms/episode  (min {ms[1]:.3f}, max {ms[2]:.3f})  kernel "
                  f"{env.last_rollout_kernel}  alerts/env {float(out['alerts'].float().mean()):.2f}  "
                  f"x{ms[0] / ms_lin[0]:.2f} of rollout(linear)")
            if args.no_torch:
                continue
            # the same network in fp32 torch as a recorded step() loop (episodes restart inside the step kernel)
            se = HeatAlertVecEnv(n, tables=ct, similar_climate_counties=True, lockstep=False)
            obs, _ = se.reset(seed=0)
            # torch's best case: the envs of a group are contiguous and equally many (one batched matmul per layer)
            assert n % G == 0
            tl = [(torch.as_tensor(Wl, device=se.device).transpose(1, 2).contiguous(),
                   torch.as_tensor(bl, device=se.device).unsqueeze(1)) for Wl, bl in layers]
            actf = torch.tanh if act == "tanh" else torch.relu
            a_out = torch.empty(n, dtype=torch.int32, device=se.device)

            def one_day():
                h = obs.view(G, n // G, -1)
                for i, (Wt, bl) in enumerate(tl):
                    h = torch.baddbmm(bl, h, Wt)
                    if i < len(tl) - 1:
                        h = actf(h)
                h = h.view(n, 2)
                a_out.copy_(h[:, 1] > h[:, 0])
                se.step(a_out)

            rec = se.record_steps(one_day, T)
            mt = timed(rec.replay, args.reps)
            rec.finish()
            se.close()
            print(f"step loop (graph) {name:12s} G={G:<5d} {mt[0]:8.3f} ms/episode  (min {mt[1]:.3f}, max {mt[2]:.3f})  "
                  f"rollout(mlp) is x{mt[0] / ms[0]:.1f} faster")
    env.close()


if __name__ == "__main__":
    main()
