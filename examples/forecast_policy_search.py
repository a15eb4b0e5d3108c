#!/usr/bin/env python3
"""Forecast-aware linear alert policies, searched and cloned inside the kernels.

1. Cross-entropy-method search over linear policies, once on the observation alone and once with
   ``"lookahead": {"feature": "heat_qi", "days": D}`` -- D more inputs h(r + k) - h(r), the coming days' heat index
   relative to the held row's (the older reference env's forecast inputs, zero forecast error). Same batch, same
   iterations; prints the elite mean return of both per iteration.
2. Behaviour cloning of hindsight_optimum()["alert_days"] (schedules that depend on future weather) with
   imitation_gradient(), with and without the lookahead inputs: the log-likelihood the forecast-aware policy reaches.
3. With ``--forecast-error E`` (one MAE in the feature's units for every lead, or ``reference`` for the older
   reference env's profile 2.5, 3.0, .., 7.0, which suits a feature in degrees) the search also runs with
   ``"error": E`` in the key -- forecasts perturbed by U(-1, 1) * MAE[k] -- and the 2 x 2 table is printed: searched
   without / with error, each evaluated without / with error. How much of the gain survives realistic forecast error,
   and does searching under error buy robustness?

    python examples/forecast_policy_search.py [--days 3] [--forecast-error 0.1 --error-seed 1]   # needs one ROCm GPU
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, synth

ap = argparse.ArgumentParser()
ap.add_argument("--days", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--groups", type=int, default=128)
ap.add_argument("--per", type=int, default=2048)
ap.add_argument("--clone-steps", type=int, default=60)
ap.add_argument("--forecast-error", default=None, help="a number (one MAE for every lead) or 'reference'")
ap.add_argument("--error-seed", type=int, default=0)
args = ap.parse_args()
D, G, per = args.days, args.groups, args.per
spec = {"feature": "heat_qi", "days": D}
noisy = None
if args.forecast_error is not None:
    mae = [2.0 + 0.5 * k for k in range(1, D + 1)] if args.forecast_error == "reference" else float(args.forecast_error)
    noisy = dict(spec, error=mae, error_seed=args.error_seed)

data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=20, seed=0, extra_confounder_fips=6)
tables = compile_from_synth(data)
n, k = G * per, tables.n_obs
env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True)  # lock step: every rollout is a fresh episode
obs0, _ = env.reset(seed=0)
group = torch.arange(n, device=env.device, dtype=torch.int32) // per
# search in units of each input's spread (the lookahead inputs' from lookahead_features() on the first rows)
scale_obs = obs0.std(dim=0).clamp_min(0.1).cpu().numpy().astype(np.float64)
scale_look = env.lookahead_features(spec).std(dim=0).clamp_min(1e-3).cpu().numpy().astype(np.float64)


def cem(look, seed=0):
    """look: False, or the "lookahead" value to search with. Returns the elite means and the final mean policy."""
    width = k + (D if look else 0)
    scale = np.concatenate([scale_obs, scale_look]) if look else scale_obs
    rng = np.random.default_rng(seed)
    mu, sd = np.zeros(width + 1), np.ones(width + 1)
    mu[width] = -1.0  # start near "rarely alert"
    elite, hist = max(G // 10, 2), []
    for _ in range(args.iters):
        theta = mu + sd * rng.standard_normal((G, width + 1))
        pol = {"kind": "linear", "weight": (theta[:, :width] / scale).astype(np.float32),
               "bias": theta[:, width].astype(np.float32), "group": group, "require_budget": True}
        if look:
            pol["lookahead"] = look
        score = env.rollout(pol)["group_mean_return"].cpu().numpy()
        top = np.argsort(score)[-elite:]
        mu, sd = theta[top].mean(axis=0), theta[top].std(axis=0) + 0.05
        hist.append(score[top].mean())
    return hist, ((mu[:width] / scale).astype(np.float32)[None, :], mu[width:].astype(np.float32))


(plain, _), (aware, best_clean) = cem(False), cem(spec)
print(f"CEM, {G} candidates x {per} envs, elite mean return per iteration (lookahead: {spec})")
for it, (a, b) in enumerate(zip(plain, aware)):
    print(f"  iter {it:2d}   observation only {a:9.3f}   with lookahead {b:9.3f}")

if noisy is not None:
    _, best_noisy = cem(noisy)
    print(f"searched / evaluated with forecast error {noisy['error']} (seed {noisy['error_seed']}): mean return")
    print(f"  {'':24s} {'evaluated clean':>16s} {'evaluated noisy':>16s}")
    for name, (w, b) in (("searched without error", best_clean), ("searched with error", best_noisy)):
        row = [float(env.rollout({"kind": "linear", "weight": w, "bias": b, "require_budget": True,
                                  "lookahead": la})["return"].mean()) for la in (spec, noisy)]
        print(f"  {name:24s} {row[0]:16.3f} {row[1]:16.3f}")

# ---- cloning the hindsight optimum: one group, normalised gradient ascent on the mean log-likelihood
clone = HeatAlertVecEnv(8192, tables=tables, similar_climate_counties=True, autoreset="disabled")
obs1, _ = clone.reset(seed=1)
sched = clone.hindsight_optimum()["alert_days"]
s_obs = obs1.std(dim=0).clamp_min(0.1)
s_look = clone.lookahead_features(spec).std(dim=0).clamp_min(1e-3)
for look in (False, True):
    s = torch.cat([s_obs, s_look]) if look else s_obs
    theta = torch.zeros(1, s.numel(), device=clone.device)  # in units of each input's spread
    b = torch.full((1,), -2.0, device=clone.device)
    for _ in range(args.clone_steps):
        pol = {"kind": "linear", "weight": theta / s, "bias": b, "require_budget": True}
        if look:
            pol["lookahead"] = spec
        out = clone.imitation_gradient(pol, sched)
        # normalised ascent: the inputs are not centred, so the raw gradient's size varies by orders of magnitude
        gw, gb = out["policy_gradient"]["weight"] / s, out["policy_gradient"]["bias"]
        step = 0.05 / torch.cat([gw.flatten(), gb.flatten()]).abs().max().clamp_min(1e-12)
        theta += step * gw
        b += step * gb
    ll = float(out["log_likelihood"].sum() / out["days"].sum())
    print(f"cloning hindsight_optimum, {'with lookahead   ' if look else 'observation only '}: "
          f"log-likelihood per scored day {ll:8.4f}")
clone.close()
env.close()
