"""NumPy fp64 restatement of hindsight_posterior_values() (w2a_hindsight_posterior_along), shared by
tests/test_hindsight_posterior_values_cpu.py and tests/test_hindsight_posterior_values_gpu.py: the DP of
tests/hindsight_posterior_restatement.py (the same states, transitions, strict comparison and draw-mean fp64 rewards),
kept for EVERY state, then read along a given schedule of attempts as tests/hindsight_values_restatement.py reads the
own-draw DP. Nothing here reads `sample`."""
from __future__ import annotations

import numpy as np

from hindsight_restatement import _env, _sigmoid, horizon
from hindsight_values_restatement import walk
from posterior_restatement import SLOTS


def hindsight_posterior_values_fp64(X, W, n_samples, Y, start, n_steps, alert_days, allowed_days=None, envs=None):
    """The keys of hindsight_values_fp64 -- fp64 [S, N] by call-day and env with S = min(n_steps, T): "q0", "q1" (NaN
    where no alert is possible, both NaN for s >= H_e), "gain" = q1 - q0, "value", "loss" (0 for s >= H_e), "issued"
    (i64); "expert" bool [N, T], "regret" [N], "H" [N] -- and "abs_reward" [N]: the draw-mean of the sum over the env's
    days of |r_d| on the issued path. `envs`: restate these env ids only (the others keep the fill values)."""
    X = np.asarray(X)
    W = np.asarray(W, np.float64).reshape(-1, 2, 32)
    T, K = X.shape[0], int(n_samples)
    N = len(np.asarray(start["t"]))
    S = min(int(n_steps), T)
    assert not W[:, :, 27].any(), "the DP needs a zero slot-27 coefficient"
    alert_days = np.asarray(alert_days, bool)
    out = {k: np.full((S, N), np.nan) for k in ("q0", "q1", "gain")}
    out.update(value=np.zeros((S, N)), loss=np.zeros((S, N)), issued=np.zeros((S, N), np.int64),
               expert=np.zeros((N, T), bool), regret=np.zeros(N), H=np.zeros(N, np.int64), abs_reward=np.zeros(N))
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
        w = W[st["coef_col"] * K:(st["coef_col"] + 1) * K]  # [K, 2, 32]: every draw of the column
        jj, kk = np.meshgrid(np.arange(U + 1), np.arange(U + 2), indexing="ij")
        s = np.where(kk == jj + 1, s0 + jj, kk).astype(np.float64)
        gate = None if allowed_days is None else np.asarray(allowed_days, bool)[e]

        def rewards(d, a):  # [K, U + 1, U + 2]: every draw's reward in every state
            x = X[t0 + d, row].astype(np.float64)
            x24 = a if t0 + d > 0 else 0
            z = [(w[:, h, fixed] @ x[fixed] + x24 * w[:, h, 24])[:, None, None] + s[None] * w[:, h, 25, None, None]
                 + (budget - used - jj - a)[None] * w[:, h, 26, None, None] for h in (0, 1)]
            eff = _sigmoid(z[1]) * (x[30] > 0.5)
            return -1000.0 / 152.0 * _sigmoid(z[0]) * (1.0 - eff * a)

        issued, js, ss = walk(st, H, alert_days[e], gate)
        Vn = np.zeros((U + 2, U + 3))  # padded: row U + 1 / column U + 2 are never chosen
        losses = np.zeros(H)
        absr = np.zeros(H)
        for d in range(H - 1, -1, -1):
            allowed = (jj < rem0) & (True if gate is None else bool(gate[t0 + d]))
            r0, r1 = rewards(d, 0), rewards(d, 1)
            q0 = r0.mean(axis=0) + Vn[:U + 1, :1]
            q1 = r1.mean(axis=0) + Vn[1:U + 2, 1:U + 3]
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
            absr[d] = np.abs((r1 if issued[d] else r0)[:, j, k]).mean()
        out["regret"][e] = losses.sum()
        out["abs_reward"][e] = absr.sum()
    return out
