#!/usr/bin/env python3
"""Where would the alerts have paid most? One batch of episodes, the hindsight optimum of every env for EVERY budget
0 .. B in one sweep (hindsight_budget_curve), the mean return-versus-budget curve of every county, and the split of the
batch's own total number of alerts over counties that maximises the summed curves (an exact knapsack DP) -- against the
tables' default budgets: first the hindsight value of both, then the regret of the same threshold policy rolled out
under each.

--draw-blind: the split is decided before anyone knows which posterior draw a county's episode gets, so it also
allocates from the draw-blind curves (hindsight_posterior_budget_curve: the optimum of the reward averaged over all
draws) and prints both allocations and their values under the draw-mean, read off the draw-blind curves.

--policy: the split should maximise what the policy that will actually run earns, so it also allocates from that
policy's own curves (policy_budget_curve: rollout(linear) for every budget in one sweep -- here the linear form of the
threshold policy below) and prints them next to the hindsight and draw-blind ones, with the policy's share of the
hindsight optimum per budget.

    python examples/budget_allocation.py [--draw-blind] [--policy]           # needs one ROCm GPU
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from weather2alert_amd import HeatAlertVecEnv, compile_from_synth, stats, synth

ap = argparse.ArgumentParser()
ap.add_argument("--draw-blind", action="store_true")
ap.add_argument("--policy", action="store_true")
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

# 4c. the split on the curves of the policy that will run: heat_qi > 0.9 with budget left, as a linear policy
if args.policy:
    w = torch.zeros((1, tables.n_obs), dtype=torch.float32)
    w[0, tables.feature_names.index("heat_qi")] = 1.0
    lin = {"kind": "linear", "weight": w, "bias": [-torch.tensor(0.9, dtype=torch.float32).item()], "require_budget": True}
    pcv = env.policy_budget_curve(lin, B)  # the env is as reset() left it: its own state, its own observation rows
    assert torch.equal(pcv["own_budget"], own) and not bool(pcv["attempts_over_budget"].any())
    by_p = stats.budget_curve_by_group(pcv["return"], county, tables.S_w)
    alloc_p = stats.allocate_budget(by_p["curve"], total, group_size=by_p["count"])
    new_p = alloc_p["budget"].to(env.device)[county].to(torch.int32)
    blind_p = env.hindsight_posterior_budget_curve(B, start_state=st0)["return"].double().mean(0)
    hs_p, po_p = curve["return"].double().mean(0), pcv["return"].double().mean(0)
    print("budget: mean return of the hindsight optimum / the draw-blind optimum / the policy (policy / hindsight)")
    for b in range(B + 1):
        print(f"  {b:3d}: {hs_p[b].item():9.3f} {blind_p[b].item():9.3f} {po_p[b].item():9.3f}   "
              f"({(po_p[b] / hs_p[b]).item():.4f})")
    print("county budgets, hindsight allocation -> policy allocation:")
    print("  " + "  ".join(f"{int(alloc['budget'][g])}->{int(alloc_p['budget'][g])}" for g in range(tables.S_w)
                          if int(by["count"][g])))
    for name, bud in (("default", own), ("hindsight allocation", new), ("policy allocation", new_p)):
        v = pcv["return"][rows, bud.long()].double().mean().item()
        print(f"policy's return per episode, {name:22s}: {v:9.3f} ({int(bud.sum())} alerts)")
    v_p = pcv["return"][rows, new_p.long()].double().mean().item()
    assert abs(v_p * n - alloc_p["value"]) <= 1e-6 * abs(alloc_p["value"]) and alloc_p["spent"] <= total
    assert v_p >= pcv["return"][rows, new.long()].double().mean().item() - 1e-9  # the optimum of these curves

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
