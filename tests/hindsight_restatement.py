"""NumPy fp64 restatement of the hindsight optimum (w2a_hindsight_optimum), shared by tests/test_hindsight_cpu.py and
tests/test_hindsight_gpu.py: an exact DP over (alerts issued j, current streak s) and a brute-force enumerator of every
feasible schedule, valued with tests/posterior_restatement.py::posterior_returns_fp64.

Under the faithful semantics the reward of day d depends on the agent through slots 24 (today's alert, 0 on day 0),
25 (the pre-update streak), 26 (budget - used after today's alert) and 27 (the agent's 14-day count, whose coefficient
must be zero here). States (j, k) of row j: k <= j is a streak that began inside the horizon, k = j + 1 the start
streak s0 still unbroken (s = s0 + j); transitions (j, k) -a=0-> (j, 0) and (j, k) -a=1-> (j + 1, k + 1), the alert
allowed only while used + j < budget, taken only if strictly better."""
from __future__ import annotations

import itertools

import numpy as np

from posterior_restatement import SLOTS, posterior_returns_fp64

_FIELDS = ("t", "used", "streak", "budget", "n_days", "county_w", "year_i", "coef_col", "sample", "finished")


def _sigmoid(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z))


def _env(start, e):
    return {k: int(np.asarray(start[k])[e]) for k in _FIELDS}


def horizon(st, n_steps):
    if st["finished"] or st["t"] >= st["n_days"]:
        return 0
    return min(int(n_steps), st["n_days"] - st["t"])


def hindsight_fp64(X, W, n_samples, Y, start, n_steps):
    """(value fp64 [N], alert_days bool [N, T], alerts i64 [N]) of the exact DP, rewards in fp64 (env.py:197-226)."""
    X = np.asarray(X)
    W = np.asarray(W, np.float64).reshape(-1, 2, 32)
    T = X.shape[0]
    N = len(np.asarray(start["t"]))
    assert not W[:, :, 27].any(), "the DP needs a zero slot-27 coefficient"
    value = np.zeros(N)
    days = np.zeros((N, T), bool)
    alerts = np.zeros(N, np.int64)
    for e in range(N):
        st = _env(start, e)
        H = horizon(st, n_steps)
        if H == 0:
            continue
        t0, used, s0, budget = st["t"], st["used"], st["streak"], st["budget"]
        rem0 = budget - used
        U = max(0, min(rem0, H))
        row = st["county_w"] * int(Y) + st["year_i"]
        w = W[st["coef_col"] * int(n_samples) + st["sample"]]
        jj, kk = np.meshgrid(np.arange(U + 1), np.arange(U + 2), indexing="ij")
        s = np.where(kk == jj + 1, s0 + jj, kk).astype(np.float64)

        rt = [24, 25, 26, 27]
        fixed = [q for q in range(SLOTS) if q not in rt]

        def reward(d, a):
            x = X[t0 + d, row].astype(np.float64)
            x24 = a if t0 + d > 0 else 0
            z = [x[fixed] @ w[h, fixed] + x24 * w[h, 24] + s * w[h, 25] + (budget - used - jj - a) * w[h, 26]
                 for h in (0, 1)]
            eff = _sigmoid(z[1]) * (x[30] > 0.5)
            return -1000.0 / 152.0 * _sigmoid(z[0]) * (1.0 - eff * a)

        allowed = jj < rem0
        Vn = np.zeros((U + 2, U + 3))  # padded: row U + 1 / column U + 2 are never chosen
        dec = np.zeros((H, U + 1, U + 2), bool)
        for d in range(H - 1, -1, -1):
            q0 = reward(d, 0) + Vn[:U + 1, :1]
            q1 = reward(d, 1) + Vn[1:U + 2, 1:U + 3]
            a = allowed & (q1 > q0)
            dec[d] = a
            V = np.zeros_like(Vn)
            V[:U + 1, :U + 2] = np.where(a, q1, q0)
            Vn = V
        j, k = 0, (1 if s0 > 0 else 0)
        value[e] = Vn[j, k]
        for d in range(H):
            a = int(dec[d, j, k])
            if a:
                days[e, t0 + d] = True
                alerts[e] += 1
            j, k = j + a, (k + 1 if a else 0)
    return value, days, alerts


def own_draw_returns(X, W, n_samples, Y, start, alert_days, n_steps):
    """fp64 [N]: each env's return under its own draw (column `sample`) for the schedule alert_days."""
    pr = posterior_returns_fp64(X, W, n_samples, Y, {k: start[k] for k in start if k != "sample"} | {"hist14": _hist(start)},
                                alert_days, n_steps)
    return pr[np.arange(len(pr)), np.asarray(start["sample"])]


def _hist(start):
    return np.asarray(start["hist14"]) if "hist14" in start else np.zeros(len(np.asarray(start["t"])), np.int32)


def brute_force_fp64(X, W, n_samples, Y, start, n_steps, e):
    """(best value, best alert_days row [T]) over every feasible schedule of env e: 2^H alert patterns on the stretch's
    days with at most budget - used alerts."""
    st = _env(start, e)
    T = np.asarray(X).shape[0]
    H = horizon(st, n_steps)
    cap = max(0, st["budget"] - st["used"])
    pats = [p for p in itertools.product((0, 1), repeat=H) if sum(p) <= cap]
    M = len(pats)
    ad = np.zeros((M, T), bool)
    if H:
        ad[:, st["t"]:st["t"] + H] = np.asarray(pats, bool)
    rep = {k: np.full(M, np.asarray(start[k])[e]) for k in start}
    vals = own_draw_returns(X, W, n_samples, Y, rep, ad, n_steps)
    i = int(np.argmax(vals))
    return float(vals[i]), ad[i]
