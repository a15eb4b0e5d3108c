"""CPU twin of the policy budget curve (w2a_policy_curve_linear), shared by tests/test_policy_curve_cpu.py and
tests/test_policy_curve_gpu.py: for every budget b the vector oracle is put into the start state with budget = used + b
and stepped through its own step(), `a = policy(obs); step(a)`, with the policy's fp64 logit in the kernel's order --
the bias first, then the observation columns in slot order (the product of two f32 values is exact in fp64, so
``z + x * w`` is the kernel's fma). Column b reads float(b) in the remaining_budget column of the row the agent holds.
Nothing here touches the GPU or the library."""
from __future__ import annotations

import numpy as np

from oracle import heatalert_oracle as O


def put_state(V, start, budget, held):
    """the oracle in `start` (arrays of a state() dict) with the given budgets, holding the rows `held` [N, n_obs]"""
    V.reset(start["county_w"], start["year_i"], start["coef_col"], start["sample"], budget)
    n = len(V.t)
    V.t = np.asarray(start["t"], np.int64).copy()
    V.used = np.asarray(start["used"], np.int64).copy()
    V.streak = np.asarray(start["streak"], np.int64).copy()
    h = np.asarray(start["hist14"], np.int64)
    V.hist = ((h[:, None] >> np.arange(13, -1, -1)[None, :]) & 1).astype(np.int64)  # newest last
    V.last_actual = (h & 1).astype(np.int64)
    V.at_budget = V.used == V.budget
    V.obs = np.asarray(held, np.float64).copy()
    V._finished = (np.asarray(start["finished"]) != 0) | (V.t >= V.n_days)
    assert V.obs.shape == (n, V.C + 1)


def policy_curve_fp64(V, ct, start, held, weight, bias, group, n_steps, max_budget, sample=False, seed=0, gid0=0,
                      require_budget=False, gate=None):
    """dict of "return" fp64 [N, B + 1], "alerts" / "attempts_over_budget" i64 [N, B + 1], "alert_days" /
    "attempt_days" bool [N, B + 1, T] and "tie" bool [N, B + 1]: some decision of that (env, budget) sat within rounding
    of its threshold, so an f32 sigmoid or another summation order may decide otherwise.
    held: the rows the agents hold in `start` (None: every live env is at t == 0 with nothing used, and the rows are the
    oracle's after reset). gate: optional bool [N, T] of allowed days."""
    n, T, B = len(np.asarray(start["t"])), ct.T, int(max_budget)
    order = np.argsort(np.asarray(ct.obs_slot[: ct.n_obs]), kind="stable")  # observation columns in slot order
    g = np.zeros(n, np.int64) if group is None else np.asarray(group, np.int64)
    W64 = np.asarray(weight, np.float32).astype(np.float64)[g]
    b64 = np.asarray(bias, np.float32).astype(np.float64)[g]
    i_rem = ct.feature_names.index("remaining_budget")
    used = np.asarray(start["used"], np.int64)
    out = dict(alerts=np.zeros((n, B + 1), np.int64), attempts_over_budget=np.zeros((n, B + 1), np.int64),
               alert_days=np.zeros((n, B + 1, T), bool), attempt_days=np.zeros((n, B + 1, T), bool),
               tie=np.zeros((n, B + 1), bool))
    out["return"] = np.zeros((n, B + 1))
    rows = np.arange(n)
    for b in range(B + 1):
        if held is None:
            V.reset(start["county_w"], start["year_i"], start["coef_col"], start["sample"], used + b)
            rebuilt = V.obs.copy()
            put_state(V, start, used + b, rebuilt)
        else:
            row = np.asarray(held, np.float64).copy()
            row[:, i_rem] = float(b)
            put_state(V, start, used + b, row)
        for _ in range(int(n_steps)):
            live = ~V._finished
            if not live.any():
                break
            z, mag = b64.copy(), np.abs(b64)
            for j in order:
                x = V.obs[:, j].astype(np.float32).astype(np.float64)
                z = z + x * W64[:, j]
                mag = mag + np.abs(x * W64[:, j])
            if sample:
                s = 1.0 / (1.0 + np.exp(-z))
                u = O.devrng_policy_uniform_vec(seed, gid0 + rows, np.asarray(start["episode_no"]), V.t).astype(np.float64)
                act = u < s
                out["tie"][:, b] |= live & (np.abs(s - u) <= 1e-6)
            else:
                act = z > 0
                out["tie"][:, b] |= live & (np.abs(z) <= 1e-9 * mag)
            if require_budget:
                act &= (V.budget - V.used) > 0
            if gate is not None:
                act &= gate[rows, np.minimum(V.t, T - 1)]
            act = (act & live).astype(np.int64)
            tday, atb = V.t.copy(), V.used == V.budget
            _, r, done, actual = V.step(act)
            out["return"][:, b] += np.where(live, r, 0.0)
            out["alerts"][:, b] += np.where(live, actual, 0)
            out["attempts_over_budget"][:, b] += np.where(live & (act == 1) & atb, 1, 0)
            out["alert_days"][rows[live & (actual == 1)], b, tday[live & (actual == 1)]] = True
            out["attempt_days"][rows[live & (act == 1)], b, tday[live & (act == 1)]] = True
            V._finished = V._finished | (live & done)
    return out
