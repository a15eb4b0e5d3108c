"""NumPy fp64 restatements of the draw-blind hindsight budget curve (w2a_hindsight_posterior_curve), shared by
tests/test_hindsight_posterior_curve_cpu.py and tests/test_hindsight_posterior_curve_gpu.py:

* posterior_curve_fp64: THE reference -- column b is tests/hindsight_posterior_restatement.py::hindsight_posterior_fp64
  run on the twin whose budget is used + b, B + 1 runs in all;
* posterior_curve_direct_fp64: one fp64 DP over (r = alerts remaining, family, m) per env, the states and transitions
  of tests/budget_curve_restatement.py with the reward of every state replaced by the mean over all n_samples draws of
  the env's coefficient column, and a backtrack per starting budget. Checked against the twin runs on the CPU.
Nothing here reads `sample`, and the direct DP reads neither `budget` nor `used`."""
from __future__ import annotations

import numpy as np

from budget_curve_restatement import twin
from hindsight_posterior_restatement import hindsight_posterior_fp64
from hindsight_restatement import _env, _sigmoid, horizon
from posterior_restatement import SLOTS


def posterior_curve_fp64(X, W, n_samples, Y, start, n_steps, max_budget, gate=None):
    """dict of "value" fp64 [N, B + 1], "alert_days" bool [N, B + 1, T] and "alerts" i64 [N, B + 1]: the twins' DPs."""
    cols = [hindsight_posterior_fp64(X, W, n_samples, Y, twin(start, b), n_steps, gate) for b in range(int(max_budget) + 1)]
    return dict(value=np.stack([c[0] for c in cols], 1), alert_days=np.stack([c[1] for c in cols], 1),
                alerts=np.stack([c[2] for c in cols], 1))


def posterior_curve_direct_fp64(X, W, n_samples, Y, start, n_steps, max_budget, gate=None):
    """posterior_curve_fp64's dict from one DP per env; also "H" i64 [N]."""
    X = np.asarray(X)
    W = np.asarray(W, np.float64).reshape(-1, 2, 32)
    T, K = X.shape[0], int(n_samples)
    N = len(np.asarray(start["t"]))
    B = int(max_budget)
    assert not W[:, :, 27].any(), "the DP needs a zero slot-27 coefficient"
    out = dict(value=np.zeros((N, B + 1)), alert_days=np.zeros((N, B + 1, T), bool), alerts=np.zeros((N, B + 1), np.int64),
               H=np.zeros(N, np.int64))
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
        w = W[st["coef_col"] * K:(st["coef_col"] + 1) * K]  # [K, 2, 32]: every draw of the column
        s = np.where(ff == 1, s0 + mm, mm).astype(np.float64)

        def reward(d, a):
            x = X[t0 + d, row].astype(np.float64)
            x24 = a if t0 + d > 0 else 0
            z = [(w[:, h, fixed] @ x[fixed] + x24 * w[:, h, 24])[:, None, None, None]
                 + s[None] * w[:, h, 25, None, None, None] + (rr - a)[None] * w[:, h, 26, None, None, None] for h in (0, 1)]
            eff = _sigmoid(z[1]) * (x[30] > 0.5)
            return (-1000.0 / 152.0 * _sigmoid(z[0]) * (1.0 - eff * a)).mean(axis=0)

        Vn = np.zeros((B + 1, 2, B + 1))
        dec = np.zeros((H, B + 1, 2, B + 1), bool)
        for d in range(H - 1, -1, -1):
            q0 = reward(d, 0) + Vn[:, :1, :1]
            q1 = np.full_like(q0, -np.inf)
            if gate is None or gate[e, t0 + d]:
                q1[1:, :, :B] = reward(d, 1)[1:, :, :B] + Vn[:-1, :, 1:]
            dec[d] = q1 > q0
            Vn = np.where(dec[d], q1, q0)
        out["value"][e] = Vn[:, 1, 0]
        for b in range(B + 1):
            r, f, m = b, 1, 0
            for d in range(H):
                if dec[d, r, f, m]:
                    out["alert_days"][e, b, t0 + d] = True
                    out["alerts"][e, b] += 1
                    r, m = r - 1, m + 1
                else:
                    f, m = 0, 0
    return out
