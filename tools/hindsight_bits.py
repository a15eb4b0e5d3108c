#!/usr/bin/env python3
"""Every output tensor of the hindsight family on fixed inputs, written to one .npz -- the yardstick of a change that
must not move a bit of k_hs_dp / k_hs_along / k_hs_curve / k_hs_pm_dp or of their host side. Run it on two trees, then
compare:
    python tools/hindsight_bits.py before.npz            (on the tree before the change)
    python tools/hindsight_bits.py after.npz             (on the tree after it)
    python tools/hindsight_bits.py --compare before.npz after.npz [report.txt]
The inputs are the tables of tests/test_hindsight_gpu.py and 96 envs at budgets 8, 40 (DP in LDS) and 200 (DP in the
workspace pool), from reset and mid-episode with some envs finished and one start outside the tables, each with and
without allowed_days. The comparison is on raw bytes (np.array_equal of uint8 views), so NaNs and the sign of zeros
count; it exits 1 if an array differs or is missing."""
import sys

import numpy as np

N, BUDGETS, MID_DAYS, CURVE_BUDGETS = 96, (8, 40, 200), 25, (8, 70)


def collect(path):
    import torch

    from weather2alert_amd import HeatAlertVecEnv, synth, tables

    dev = torch.device("cuda:0")
    ct = tables.compile_from_synth(synth.make_synth("linear", n_fips=30, years=[2006, 2007], n_samples=6, seed=17,
                                                      extra_confounder_fips=3))
    gate = torch.as_tensor(np.random.default_rng(5).random((N, ct.T)) < 0.5, device=dev)
    sched = torch.as_tensor(np.random.default_rng(6).random((N, ct.T)) < 0.3, device=dev)
    out = {}

    def keep(tag, res):
        for k, v in res.items():
            out[f"{tag}/{k}"] = v.cpu().numpy()

    for budget in BUDGETS:
        env = HeatAlertVecEnv(N, tables=ct, device=dev, similar_climate_counties=True, autoreset="disabled")
        env.reset(seed=3, options={"budget": budget})
        starts = {"reset": {k: v.clone() for k, v in env.state().items()}}
        g = torch.Generator(device=dev).manual_seed(budget)
        for _ in range(MID_DAYS):
            env.step((torch.rand(N, generator=g, device=dev) < 0.35).to(torch.int32))
        mid = {k: v.clone() for k, v in env.state().items()}
        mid["finished"][5:9] = 1
        mid["coef_col"][0] = ct.S + 3  # a start outside the tables: NaN
        starts["mid"] = mid
        for where, st in starts.items():
            for gname, allowed in (("open", None), ("gated", gate)):
                tag = f"b{budget}/{where}/{gname}"
                hs = env.hindsight_optimum(st, allowed_days=allowed)
                keep(f"{tag}/optimum", hs)
                keep(f"{tag}/optimum17", env.hindsight_optimum(st, n_steps=17, allowed_days=allowed))
                keep(f"{tag}/values_own", env.hindsight_values(hs["alert_days"], st, allowed_days=allowed, value=True,
                                                               loss=True))
                keep(f"{tag}/values", env.hindsight_values(sched, st, allowed_days=allowed, value=True, loss=True))
                for B in CURVE_BUDGETS:
                    keep(f"{tag}/curve{B}", env.hindsight_budget_curve(B, st, allowed_days=allowed, schedules=True))
                keep(f"{tag}/posterior", env.hindsight_posterior_optimum(st, allowed_days=allowed, share=False))
        assert env.check_status() == 0
        env.close()
    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path}")


def compare(a_path, b_path, report=None):
    a, b = np.load(a_path), np.load(b_path)
    lines, bad = [f"{a_path} against {b_path}: raw bytes of every array"], 0
    for k in sorted(set(a.files) | set(b.files)):
        if k not in a.files or k not in b.files:
            verdict = "MISSING in " + (a_path if k not in a.files else b_path)
        else:
            x, y = a[k], b[k]
            same = x.shape == y.shape and x.dtype == y.dtype and \
                np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
            verdict = "equal" if same else "DIFFERENT"
        bad += verdict != "equal"
        shape = a[k].shape if k in a.files else b[k].shape
        dtype = a[k].dtype if k in a.files else b[k].dtype
        lines.append(f"{k:44s} {str(dtype):8s} {str(tuple(shape)):18s} {verdict}")
    lines.append(f"{len(lines) - 1} arrays, {bad} not equal")
    text = "\n".join(lines)
    print(text)
    if report:
        with open(report, "w") as f:
            f.write(text + "\n")
    return bad


if __name__ == "__main__":
    sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
    if sys.argv[1:2] == ["--compare"]:
        sys.exit(1 if compare(*sys.argv[2:5]) else 0)
    collect(sys.argv[1])
