#!/usr/bin/env python3
"""Where would the alerts have paid most? One batch of episodes, the hindsight optimum of every env for EVERY budget
0 .. B in one sweep (hindsight_budget_curve), the mean return-versus-budget curve of every county, and the split of the
batch's own total number of alerts over counties that maximises the summed curves (an exact knapsack DP) -- against the
tables' default budgets: first the hindsight value of both, then the regret of the same threshold policy rolled out
under each.

--draw-blind: the split is decided before anyone knows which posterior draw a county's episode gets, so it also
allocates from the draw-blind curves (hindsight_posterior_budget_curve: the optimum of the reward averaged over all
draws) and prints both allocations and their values under the draw-mean, read off the draw-blind curves.

    python examples/budget_allocation.py [--draw-blind]           # needs one ROCm GPU
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, stats, synth

ap = argparse.ArgumentParser()
ap.add_argument("--draw-blind", action="store_true")
args = ap.parse_args()

data = synth.make_synth("linear", n_fips=64, years=[2006, 2007, 2008], n_samples=100, seed=0, extra_confounder_fips=6)
tables = compile_from_synth(data)
n = 1 << 14
env = HeatAlertVecEnv(n, tables=tables, similar_climate_counties=True, autoreset="disabled")

# 1. one batch of episodes and its curves: column b is the optimum had the env's budget been b
env.reset(seed=123)
st0 = {k: v.clone() for k, v in env.state().items()}
own = st0["budget"] - st0["used"]
B = int(own.max())
curve = env.hindsight_budget_curve(B, start_state=st0)
rows = torch.arange(n, device=env.device)
assert torch.equal(curve["return"][rows, own.long()], env.hindsight_optimum(st0)["return"])  # the env's own column

# 2. the mean curve of every county (fp64; NaN rows would be skipped and counted)
county = st0["county_w"].long()
by = stats.budget_curve_by_group(curve["return"], county, tables.S_w)
assert int(by["skipped"].sum()) == 0

# 3. the batch's own total, split over counties: every env of a county gets the county's budget
total = int(own.sum())
alloc = stats.allocate_budget(by["curve"], total, group_size=by["count"])
new = alloc["budget"].to(env.device)[county].to(torch.int32)
print(f"{n} episodes in {int((by['count'] > 0).sum())} counties, {total} alerts in all (default budgets 0..{B})")
print("county budgets, default (mean) -> allocated:")
mean_own = stats.budget_curve_by_group(own.double()[:, None], county, tables.S_w)["curve"][:, 0]
print("  " + "  ".join(f"{float(mean_own[g]):.1f}->{int(alloc['budget'][g])}" for g in range(tables.S_w)
                      if int(by["count"][g])))

# 4. the hindsight value of both splits, read off the same curves
v_def = curve["return"][rows, own.long()].double().mean().item()
v_new = curve["return"][rows, new.long()].double().mean().item()
assert abs(v_new * n - alloc["value"]) <= 1e-6 * abs(alloc["value"]) and alloc["spent"] <= total
print(f"hindsight value per episode: default budgets {v_def:.3f}, allocated {v_new:.3f} "
      f"({alloc['spent']} of {total} alerts spent)")

# 4b. the same split from the draw-blind curves, and all three splits scored under the draw-mean
if args.draw_blind:
    blind = env.hindsight_posterior_budget_curve(B, start_state=st0)
    assert torch.equal(blind["own_budget"], own)
    by_b = stats.budget_curve_by_group(blind["return"], county, tables.S_w)
    alloc_b = stats.allocate_budget(by_b["curve"], total, group_size=by_b["count"])
    new_b = alloc_b["budget"].to(env.device)[county].to(torch.int32)
    print(f"draw-blind curves: {env.last_hindsight_posterior_keys} distinct problems among {n} episodes")
    print("county budgets, own-draw allocation -> draw-blind allocation:")
    print("  " + "  ".join(f"{int(alloc['budget'][g])}->{int(alloc_b['budget'][g])}" for g in range(tables.S_w)
                          if int(by["count"][g])))
    moved = int((alloc["budget"] != alloc_b["budget"])[(by["count"] > 0).cpu()].sum())
    print(f"{moved} of {int((by['count'] > 0).sum())} counties get another budget")
    for name, bud in (("default", own), ("own-draw allocation", new), ("draw-blind allocation", new_b)):
        v = blind["return"][rows, bud.long()].double().mean().item()
        print(f"draw-mean value per episode, {name:22s}: {v:9.3f} ({int(bud.sum())} alerts)")
    v_b = blind["return"][rows, new_b.long()].double().mean().item()
    assert abs(v_b * n - alloc_b["value"]) <= 1e-6 * abs(alloc_b["value"]) and alloc_b["spent"] <= total
    assert v_b >= blind["return"][rows, new.long()].double().mean().item() - 1e-9  # the optimum of these curves

# 5. the same threshold policy under each split: its return, and its regret against the curve's column
policy = {"kind": "threshold", "feature": "heat_qi", "threshold": 0.9, "require_budget": True}
ep = {k: st0[k].cpu().numpy() for k in ("county_w", "year_i", "coef_col", "sample")}
for name, budget in (("default", own), ("allocated", new)):
    env.reset(options={"episodes": dict(ep, budget=budget.cpu().numpy())})
    assert torch.equal(env.state()["budget"], budget.to(torch.int32))
    ret = env.rollout(policy)["return"]
    opt = curve["return"][rows, budget.long()]
    reg = (opt - ret).double()
    assert bool((reg >= -2e-6 * ret.abs()).all())
    print(f"{name:10s} budgets: threshold policy return {ret.double().mean().item():9.3f}, optimum "
          f"{opt.double().mean().item():9.3f}, regret {reg.mean().item():8.3f}")
env.close()
