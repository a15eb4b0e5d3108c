"""NumPy fp64 restatement of hindsight_values() (w2a_hindsight_along), shared by tests/test_hindsight_values_cpu.py and
tests/test_hindsight_values_gpu.py: the DP of tests/hindsight_restatement.py (the same states, transitions, strict
comparison and fp64 rewards), kept for EVERY state, then read along a given schedule of attempts.

For the state (j, streak) the schedule reaches on call-day s: Q0 = r0 + V_{s+1}(j, 0), Q1 = r1 + V_{s+1}(j + 1,
streak + 1) (only while used + j < budget on an allowed day), value = max(Q0, Q1), expert bit = Q1 > Q0, loss = value -
Q(alert issued), regret = the sum of the losses. Also `walk`, the schedule's integer states and issued alerts."""
from __future__ import annotations

import numpy as np

from hindsight_restatement import _env, _sigmoid, horizon
from posterior_restatement import SLOTS


def walk(st, H, attempts_row, allowed_row=None):
    """(issued [H], j [H], streak [H]) of one env: the schedule's bits are attempts; a closed day is 0 before the budget
    test, an attempt without budget left is a no-op. j = alerts issued before the day, streak = the streak held."""
    t0, rem0 = st["t"], st["budget"] - st["used"]
    issued, js, ss = np.zeros(H, np.int64), np.zeros(H, np.int64), np.zeros(H, np.int64)
    j, s = 0, st["streak"]
    for d in range(H):
        a = int(attempts_row[t0 + d])
        if allowed_row is not None and not allowed_row[t0 + d]:
            a = 0
        if j >= rem0:
            a = 0
        issued[d], js[d], ss[d] = a, j, s
        j, s = j + a, (s + 1 if a else 0)
    return issued, js, ss


def hindsight_values_fp64(X, W, n_samples, Y, start, n_steps, alert_days, allowed_days=None, envs=None):
    """dict of fp64 arrays by call-day and env, [S, N] with S = min(n_steps, T): "q0", "q1" (NaN where no alert is
    possible, and both NaN for s >= H_e), "gain" = q1 - q0, "value", "loss" (0 for s >= H_e), "issued" (i64); and
    "expert" bool [N, T], "regret" [N], "H" [N]. `envs`: restate these env ids only (the others keep the fill values;
    a budget of 200 costs about 0.15 s per env here)."""
    X = np.asarray(X)
    W = np.asarray(W, np.float64).reshape(-1, 2, 32)
    T = X.shape[0]
    N = len(np.asarray(start["t"]))
    S = min(int(n_steps), T)
    assert not W[:, :, 27].any(), "the DP needs a zero slot-27 coefficient"
    alert_days = np.asarray(alert_days, bool)
    out = {k: np.full((S, N), np.nan) for k in ("q0", "q1", "gain")}
    out.update(value=np.zeros((S, N)), loss=np.zeros((S, N)), issued=np.zeros((S, N), np.int64),
               expert=np.zeros((N, T), bool), regret=np.zeros(N), H=np.zeros(N, np.int64))
    rt = [24, 25, 26, 27]
    fixed = [q for q in range(SLOTS) if q not in rt]
    for e in (range(N) if envs is None else envs):
        st = _env(start, e)
        H = horizon(st, n_steps)
        out["H"][e] = H
        if H == 0:
            continue
        t0, used, s0, budget = st["t"], st["used"], st["streak"], st["budget"]
        rem0 = budget - used
        U = max(0, min(rem0, H))
        row = st["county_w"] * int(Y) + st["year_i"]
        w = W[st["coef_col"] * int(n_samples) + st["sample"]]
        jj, kk = np.meshgrid(np.arange(U + 1), np.arange(U + 2), indexing="ij")
        s = np.where(kk == jj + 1, s0 + jj, kk).astype(np.float64)
        gate = None if allowed_days is None else np.asarray(allowed_days, bool)[e]

        def reward(d, a):
            x = X[t0 + d, row].astype(np.float64)
            x24 = a if t0 + d > 0 else 0
            z = [x[fixed] @ w[h, fixed] + x24 * w[h, 24] + s * w[h, 25] + (budget - used - jj - a) * w[h, 26]
                 for h in (0, 1)]
            eff = _sigmoid(z[1]) * (x[30] > 0.5)
            return -1000.0 / 152.0 * _sigmoid(z[0]) * (1.0 - eff * a)

        issued, js, ss = walk(st, H, alert_days[e], gate)
        Vn = np.zeros((U + 2, U + 3))  # padded: row U + 1 / column U + 2 are never chosen
        losses = np.zeros(H)
        for d in range(H - 1, -1, -1):
            allowed = (jj < rem0) & (True if gate is None else bool(gate[t0 + d]))
            q0 = reward(d, 0) + Vn[:U + 1, :1]
            q1 = reward(d, 1) + Vn[1:U + 2, 1:U + 3]
            a = allowed & (q1 > q0)
            V = np.zeros_like(Vn)
            V[:U + 1, :U + 2] = np.where(a, q1, q0)
            Vn = V
            # the schedule's state: slot j + 1 of row j is the start streak, unbroken since (j alerts on days 0..d-1)
            j = int(js[d])
            k = j + 1 if (s0 > 0 and j == d) else int(ss[d])
            assert s[j, k] == ss[d]
            out["q0"][d, e] = q0[j, k]
            out["value"][d, e] = V[j, k]
            if allowed[j, k]:
                out["q1"][d, e] = q1[j, k]
                out["gain"][d, e] = q1[j, k] - out["q0"][d, e]
            out["expert"][e, t0 + d] = a[j, k]
            out["issued"][d, e] = issued[d]
            assert not issued[d] or allowed[j, k]
            losses[d] = V[j, k] - (q1[j, k] if issued[d] else out["q0"][d, e])
            out["loss"][d, e] = losses[d]
        out["regret"][e] = losses.sum()
    return out
