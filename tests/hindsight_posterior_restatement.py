"""NumPy fp64 restatements of the hindsight optimum with the draw unknown (w2a_hindsight_posterior), shared by
tests/test_hindsight_posterior_cpu.py and tests/test_hindsight_posterior_gpu.py:

* hindsight_posterior_fp64: the DP of tests/hindsight_restatement.py -- the same states (j, k), transitions, budget test
  and strict comparison -- with the reward of every state replaced by the mean over all n_samples draws of the env's
  coefficient column of the fp64 rewards; an optional gate restricts the alert to allowed days;
* brute_force_posterior_fp64: every feasible schedule of one env, valued by
  tests/posterior_restatement.py::posterior_returns_fp64(...).mean(axis=1).
Nothing here reads `sample`."""
from __future__ import annotations

import itertools

import numpy as np

from hindsight_restatement import _env, _hist, _sigmoid, horizon
from posterior_restatement import SLOTS, posterior_returns_fp64


def hindsight_posterior_fp64(X, W, n_samples, Y, start, n_steps, gate=None):
    """(value fp64 [N], alert_days bool [N, T], alerts i64 [N]); gate: optional bool [N, T] of allowed days."""
    X = np.asarray(X)
    W = np.asarray(W, np.float64).reshape(-1, 2, 32)
    T, K = X.shape[0], int(n_samples)
    N = len(np.asarray(start["t"]))
    assert not W[:, :, 27].any(), "the DP needs a zero slot-27 coefficient"
    value = np.zeros(N)
    days = np.zeros((N, T), bool)
    alerts = np.zeros(N, np.int64)
    rt = [24, 25, 26, 27]
    fixed = [q for q in range(SLOTS) if q not in rt]
    for e in range(N):
        st = _env(start, e)
        H = horizon(st, n_steps)
        if H == 0:
            continue
        t0, used, s0, budget = st["t"], st["used"], st["streak"], st["budget"]
        rem0 = budget - used
        U = max(0, min(rem0, H))
        row = st["county_w"] * int(Y) + st["year_i"]
        w = W[st["coef_col"] * K:(st["coef_col"] + 1) * K]  # [K, 2, 32]: every draw of the column
        jj, kk = np.meshgrid(np.arange(U + 1), np.arange(U + 2), indexing="ij")
        s = np.where(kk == jj + 1, s0 + jj, kk).astype(np.float64)

        def reward(d, a):
            x = X[t0 + d, row].astype(np.float64)
            x24 = a if t0 + d > 0 else 0
            z = [(w[:, h, fixed] @ x[fixed] + x24 * w[:, h, 24])[:, None, None] + s[None] * w[:, h, 25, None, None]
                 + (budget - used - jj - a)[None] * w[:, h, 26, None, None] for h in (0, 1)]
            eff = _sigmoid(z[1]) * (x[30] > 0.5)
            return (-1000.0 / 152.0 * _sigmoid(z[0]) * (1.0 - eff * a)).mean(axis=0)

        allowed = jj < rem0
        Vn = np.zeros((U + 2, U + 3))  # padded: row U + 1 / column U + 2 are never chosen
        dec = np.zeros((H, U + 1, U + 2), bool)
        for d in range(H - 1, -1, -1):
            q0 = reward(d, 0) + Vn[:U + 1, :1]
            q1 = reward(d, 1) + Vn[1:U + 2, 1:U + 3]
            a = allowed & (q1 > q0)
            if gate is not None and not gate[e, t0 + d]:
                a[:] = False
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


def posterior_mean_returns(X, W, n_samples, Y, start, alert_days, n_steps):
    """fp64 [N]: the mean over draws of each env's return for the schedule alert_days."""
    st = {k: start[k] for k in start if k != "sample"} | {"hist14": _hist(start)}
    return posterior_returns_fp64(X, W, n_samples, Y, st, alert_days, n_steps).mean(axis=1)


def brute_force_posterior_fp64(X, W, n_samples, Y, start, n_steps, e, gate=None):
    """(best value, best alert_days row [T]) over every feasible schedule of env e: 2^H alert patterns on the stretch's
    (allowed) days with at most budget - used alerts."""
    st = _env(start, e)
    T = np.asarray(X).shape[0]
    H = horizon(st, n_steps)
    cap = max(0, st["budget"] - st["used"])
    pats = [p for p in itertools.product((0, 1), repeat=H) if sum(p) <= cap]
    ad = np.zeros((len(pats), T), bool)
    if H:
        ad[:, st["t"]:st["t"] + H] = np.asarray(pats, bool)
    if gate is not None:
        ad = ad[~(ad & ~np.asarray(gate)[e][None]).any(axis=1)]
    rep = {k: np.full(len(ad), np.asarray(start[k])[e]) for k in start}
    vals = posterior_mean_returns(X, W, n_samples, Y, rep, ad, n_steps)
    i = int(np.argmax(vals))
    return float(vals[i]), ad[i]
