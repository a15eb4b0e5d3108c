"""Round-10 capture from the *unmodified* reference HeatAlertEnv: per-day rewards under EVERY posterior draw.

Runs ONLY in the build container (needs /root/reference); output committed: tests/golden/posterior_draws.npz.
Same import recipe as make_golden.py (a throw-away `gymnasium` stand-in on sys.path, `hf_hub_download` re-pointed at
the committed tests/golden/mini and tests/golden/mini64 data sets; the env code is untouched, nothing of it is copied).

For each episode: one reference env per posterior draw k (n_samples of them), all reset with the same seed and kwargs
(so the same county, year, coefficient column and budget), then `env.coef_index = k` -- the draw the reward reads
(env.py:209,216) -- and every env stepped with the same actions until done. Recorded: the per-day rewards [T, K] (f64,
NaN after the terminal day), the actions and the alerts actually issued, the reset tuple, and the draw reset() chose.
These pin the per-draw rewards and their mean (tests/test_posterior_returns_cpu.py, tests/test_posterior_returns_gpu.py)."""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import ROOT, T, import_reference, make_actions, patch_hub  # noqa: E402

sys.path.insert(0, ROOT)


def scenarios():
    """(data set, ctor kwargs, reset kwargs, action spec): plain and augmented episodes, budgets 0 / 1 / 5 and the
    table default, mixed, all-0 and all-1 actions; several hit their budget."""
    return [
        ("mini", {}, dict(seed=3), ("bern", 0.3, 7001)),
        ("mini", {}, dict(location="06037", seed=4), ("zeros",)),
        ("mini", {}, dict(location="06037", similar_climate_counties=True, seed=21), ("bern", 0.3, 7002)),
        ("mini", dict(similar_climate_counties=True), dict(seed=31), ("bern", 0.25, 7003)),
        ("mini", {}, dict(seed=40, budget=0), ("ones",)),
        ("mini", {}, dict(seed=41, budget=1), ("bern", 0.5, 7004)),
        ("mini", {}, dict(location="06037", seed=45, budget=5), ("ones",)),
        ("mini", {}, dict(seed=46), ("ones",)),
        ("mini", {}, dict(seed=47, budget=5, similar_climate_counties=True), ("bern", 0.4, 7005)),
        ("mini64", {}, dict(seed=40), ("bern", 0.3, 7006)),
        ("mini64", dict(similar_climate_counties=True), dict(seed=50, budget=4), ("bern", 0.4, 7007)),
        ("mini64", {}, dict(location="06037", seed=2, budget=T), ("ones",)),
    ]


def main():
    tmp = tempfile.mkdtemp(prefix="w2a_golden_r10_")
    refenv = import_reference(os.path.join(tmp, "shim"))
    rec = []
    for di, (data, ctor, reset, aspec) in enumerate(scenarios()):
        root = os.path.join(HERE, data)
        patch_hub(refenv, root)
        actions = make_actions(aspec, T)
        probe = refenv.HeatAlertEnv(weights="linear", data_dir=root, **ctor)
        probe.reset(**reset)
        K = int(probe.n_samples)
        R = np.full((T, K), np.nan, np.float64)
        A = np.zeros(T, np.int64)
        head = None
        for k in range(K):
            env = refenv.HeatAlertEnv(weights="linear", data_dir=root, **ctor)
            obs, info = env.reset(**reset)
            h = dict(episode_index=info["episode_index"], location_index=int(info["location_index"]),
                     coef_index=int(env.coef_index), budget=int(env.budget), n_days=int(env.n_days))
            assert head is None or h == head, (h, head)  # every env of the episode drew the same episode
            head = h
            env.coef_index = k
            for t in range(env.n_days):
                obs, r, done, trunc, info = env.step(int(actions[t]))
                R[t, k] = r
                if k == 0:
                    A[t] = env.actual_alert_buffer[-1]
                if done:
                    break
        nd = head["n_days"]
        print(f"episode {di} ({data}): {head['episode_index']} column {head['location_index']} own draw "
              f"{head['coef_index']} budget {head['budget']} n_days {nd} alerts {int(A.sum())}/{int(actions[:nd].sum())} "
              f"return range {np.nansum(R, 0).min():.4f}..{np.nansum(R, 0).max():.4f}")
        rec.append(dict(data=data, ctor=ctor, reset=reset, K=K, reward=R, actions=actions, actual=A, **head))
    import numpy
    import pandas
    import scipy

    Kmax = max(e["K"] for e in rec)
    reward = np.full((len(rec), T, Kmax), np.nan, np.float64)
    for i, e in enumerate(rec):
        reward[i, :, : e["K"]] = e["reward"]
    arr = dict(reward=reward,
               actions=np.stack([e["actions"] for e in rec]).astype(np.int8),
               actual=np.stack([e["actual"] for e in rec]).astype(np.int8),
               n_samples=np.asarray([e["K"] for e in rec], np.int32),
               **{k: np.asarray([e[k] for e in rec], np.int32)
                  for k in ("location_index", "coef_index", "budget", "n_days")})
    meta = dict(versions={"numpy": numpy.__version__, "pandas": pandas.__version__, "scipy": scipy.__version__},
                episodes=[dict(data=e["data"], ctor=e["ctor"], reset=e["reset"], episode_index=e["episode_index"])
                          for e in rec])
    path = os.path.join(HERE, "posterior_draws.npz")
    np.savez_compressed(path, meta_json=np.asarray(json.dumps(meta)), **arr)
    print("wrote", path, os.path.getsize(path), "bytes;", len(rec), "episodes")


if __name__ == "__main__":
    main()
