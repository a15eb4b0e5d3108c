"""NumPy fp64 restatement of the returns under every posterior draw (w2a_posterior_returns), shared by
tests/test_posterior_returns_cpu.py and tests/test_posterior_returns_gpu.py.

From the compiled tables (X [T][S_w*Y][32], W [S*n_samples][2][32]), a start state and the bitmap of alerts issued, every
active day rebuilds the 32-slot row -- table row of day t, run-time slots 24..27 = alert_lag1 (today's alert, 0 on day
0), the pre-update alert_streak, remaining_budget after today's alert, alert_2wks (alerts of the last 14 days, today's
included) -- and applies the reference's _get_reward (env.py:197-226) per draw in float64: sigmoid of the two dot
products over slots 0..29, the effectiveness gated by heat_qi > 0.5 (slot 30 of the compiled row holds that decision),
reward = -1000/152 * baseline * (1 - effectiveness * actual)."""
from __future__ import annotations

import numpy as np

SLOTS = 30


def posterior_returns_fp64(X, W, n_samples, Y, start, alert_days, n_steps, per_day=False, chunk=512):
    """fp64 [N, n_samples] returns (and with per_day=True also [N, n_steps, n_samples] rewards, NaN where the env did
    not step). start: dict of int arrays [N] (t, used, streak, hist14, budget, n_days, county_w, year_i, coef_col,
    finished); Y: years per weather county (feature row = county_w * Y + year_i); alert_days bool [N, >= T]."""
    X = np.asarray(X)
    W = np.asarray(W, np.float64).reshape(-1, 2, 32)
    N = len(start["t"])
    K = int(n_samples)
    out = np.zeros((N, K), np.float64)
    days = np.full((N, n_steps, K), np.nan) if per_day else None
    for c0 in range(0, N, chunk):
        sl = slice(c0, min(N, c0 + chunk))
        st = {k: np.asarray(v)[sl].astype(np.int64) for k, v in start.items()}
        n = sl.stop - sl.start
        t, used, streak, hist = st["t"].copy(), st["used"].copy(), st["streak"].copy(), st["hist14"].copy() & 0x3FFF
        active = (st["finished"] == 0) & (t < st["n_days"])
        ep_row = st["county_w"] * int(Y) + st["year_i"]
        wr = st["coef_col"][:, None] * K + np.arange(K)[None, :]
        wb = W[wr, 0, :SLOTS]  # [n, K, 30]
        we = W[wr, 1, :SLOTS]
        ad = np.asarray(alert_days)[sl]
        acc = np.zeros((n, K), np.float64)
        for s in range(n_steps):
            if not active.any():
                break
            tt = np.where(active, t, 0)
            actual = ad[np.arange(n), tt].astype(np.int64) * active
            used2 = used + actual
            hist2 = ((hist << 1) | actual) & 0x3FFF
            x = X[tt, ep_row].astype(np.float64)  # [n, 32]
            x[:, 24] = np.where(tt > 0, actual, 0)
            x[:, 25] = streak
            x[:, 26] = st["budget"] - used2
            x[:, 27] = np.array([bin(int(h)).count("1") for h in hist2])
            zb = np.einsum("nks,ns->nk", wb, x[:, :SLOTS])
            ze = np.einsum("nks,ns->nk", we, x[:, :SLOTS])
            base = 1.0 / (1.0 + np.exp(-zb))
            eff = (1.0 / (1.0 + np.exp(-ze))) * (x[:, 30:31] > 0.5)
            r = -1000.0 / 152.0 * base * (1.0 - eff * actual[:, None])
            r = np.where(active[:, None], r, 0.0)
            acc += r
            if per_day:
                days[sl][:, s] = np.where(active[:, None], r, np.nan)
            done = t + 1 >= st["n_days"]
            used = np.where(active, used2, used)
            hist = np.where(active, hist2, hist)
            adv = active & ~done
            streak = np.where(adv, np.where(actual == 1, streak + 1, 0), streak)
            t = np.where(adv, t + 1, t)
            active = adv
        out[sl] = acc
    return (out, days) if per_day else out
