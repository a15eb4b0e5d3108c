"""NumPy restatement of the hindsight budget curve (w2a_hindsight_curve), shared by tests/test_budget_curve_cpu.py and
tests/test_budget_curve_gpu.py: one fp64 DP over (r = alerts remaining, family, m) per env and a backtrack per starting
budget that re-adds the chosen rewards in f32 in day order, on the reward of tests/hindsight_restatement.py.

States at r remaining, B = max_budget: family 0 holds the streaks m = 0 .. B - r begun inside the horizon, family 1 the
start streak still unbroken, s0 + m. Transitions (r, f, m) -a=0-> (r, 0, 0) and (r, f, m) -a=1-> (r - 1, f, m + 1), the
alert only while r > 0 on an allowed day and only if strictly better. Column b starts in (b, 1, 0)."""
from __future__ import annotations

import numpy as np

from hindsight_restatement import _env, _sigmoid, horizon
from posterior_restatement import SLOTS


def budget_curve_fp64(X, W, n_samples, Y, start, n_steps, max_budget, gate=None):
    """dict of  "value" fp64 [N, B + 1] (V_0(b, s0)), "return32" f32 [N, B + 1] (the schedule's rewards rounded to f32
    and added in f32 in day order), "alert_days" bool [N, B + 1, T], "alerts" i64 [N, B + 1], "margin" fp64 [N, B + 1]
    (the smallest |q1 - q0| over the days of budget b's path on which an alert was possible; inf if there was none) and
    "H" i64 [N]. gate: optional bool [N, T] of allowed days. The env's own budget and used are not read."""
    X = np.asarray(X)
    W = np.asarray(W, np.float64).reshape(-1, 2, 32)
    T = X.shape[0]
    N = len(np.asarray(start["t"]))
    B = int(max_budget)
    assert not W[:, :, 27].any(), "the DP needs a zero slot-27 coefficient"
    out = dict(value=np.zeros((N, B + 1)), return32=np.zeros((N, B + 1), np.float32),
               alert_days=np.zeros((N, B + 1, T), bool), alerts=np.zeros((N, B + 1), np.int64),
               margin=np.full((N, B + 1), np.inf), H=np.zeros(N, np.int64))
    rt = [24, 25, 26, 27]
    fixed = [q for q in range(SLOTS) if q not in rt]
    rr, ff, mm = np.meshgrid(np.arange(B + 1), np.arange(2), np.arange(B + 1), indexing="ij")
    for e in range(N):
        st = _env(start, e)
        H = horizon(st, n_steps)
        out["H"][e] = H
        if H == 0:
            continue
        t0, s0 = st["t"], st["streak"]
        row = st["county_w"] * int(Y) + st["year_i"]
        w = W[st["coef_col"] * int(n_samples) + st["sample"]]
        s = np.where(ff == 1, s0 + mm, mm).astype(np.float64)

        def reward(d, a):
            x = X[t0 + d, row].astype(np.float64)
            x24 = a if t0 + d > 0 else 0
            z = [x[fixed] @ w[h, fixed] + x24 * w[h, 24] + s * w[h, 25] + (rr - a) * w[h, 26] for h in (0, 1)]
            eff = _sigmoid(z[1]) * (x[30] > 0.5)
            return -1000.0 / 152.0 * _sigmoid(z[0]) * (1.0 - eff * a)

        Vn = np.zeros((B + 1, 2, B + 1))
        dec = np.zeros((H, B + 1, 2, B + 1), bool)
        gap = np.full((H, B + 1, 2, B + 1), np.inf)
        rew = np.zeros((H, 2, B + 1, 2, B + 1))
        for d in range(H - 1, -1, -1):
            rew[d, 0], rew[d, 1] = reward(d, 0), reward(d, 1)
            q0 = rew[d, 0] + Vn[:, :1, :1]
            q1 = np.full_like(q0, -np.inf)
            if gate is None or gate[e, t0 + d]:
                q1[1:, :, :B] = rew[d, 1][1:, :, :B] + Vn[:-1, :, 1:]
            dec[d] = q1 > q0
            gap[d] = np.where(np.isfinite(q1), np.abs(q1 - q0), np.inf)
            Vn = np.where(dec[d], q1, q0)
        out["value"][e] = Vn[:, 1, 0]
        for b in range(B + 1):
            r, f, m = b, 1, 0
            acc = np.float32(0.0)
            for d in range(H):
                a = int(dec[d, r, f, m])
                out["margin"][e, b] = min(out["margin"][e, b], gap[d, r, f, m])
                acc = np.float32(acc + np.float32(rew[d, a, r, f, m]))
                if a:
                    out["alert_days"][e, b, t0 + d] = True
                    out["alerts"][e, b] += 1
                    r, m = r - 1, m + 1
                else:
                    f, m = 0, 0
            out["return32"][e, b] = acc
    return out


def twin(start, b):
    """the start whose remaining budget is b: budget = used + b"""
    st = {k: np.array(v) for k, v in start.items()}
    st["budget"] = st["used"] + b
    return st
