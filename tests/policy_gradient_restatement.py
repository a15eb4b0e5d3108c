"""NumPy fp64 restatement of the reward-to-go score-function gradient of rollout(policy_gradient=...)
(w2a_policy_gradient_linear, include/w2a.h), shared by tests/test_policy_gradient_cpu.py and
tests/test_policy_gradient_gpu.py. From a recorded trajectory -- the rows held before every decision, the policy's
draws, which days were forced by require_budget, the per-day rewards and the per-day no-alert rewards -- per env e

    g_e = sum_s delta_s Q_s (o_s, 1),  delta_s = m_s (a_s - sigmoid(z_s)),  Q_s = sum_{s' >= s, valid} (r_s' - beta_s'),

z_s = W[g] . o_s + b[g] in fp64, and per group the mean of g_e over its envs (NaN for a group without envs). Next to
it the bar the GPU tests hold the kernel to: 1e-5 per reward and day, so 2e-5 per advantage, and the f32 sigmoid within
~1e-7 of fp64 taken x 10:

    bound[g, j] = mean_e sum_s |o_sj| (|delta_s| 2e-5 (valid days from s on) + 1e-6 |Q_s|)      (o_s,n_obs = 1: the bias)
"""
from __future__ import annotations

import numpy as np


def forced_days(require_budget, budget, used0, alert, valid):
    """bool [S, N]: the days on which require_budget forced the action to 0 (no budget left before the decision), from
    the start state and the alerts issued."""
    alert = (np.asarray(alert).astype(bool) & np.asarray(valid).astype(bool)).astype(np.int64)
    if not require_budget:
        return np.zeros(alert.shape, bool)
    used_before = np.asarray(used0, np.int64)[None, :] + np.cumsum(alert, axis=0) - alert
    return (np.asarray(budget, np.int64)[None, :] - used_before) <= 0


def policy_gradient_fp64(obs, action, valid, forced, reward, baseline_reward, W, b, group, n_groups=None):
    """obs [>= S, N, n_obs] (slab s: the row held before decision s), action / valid / forced [S, N], reward [S, N],
    baseline_reward [S, N] or None (the "none" baseline), W [G, n_obs], b [G], group int [N] or None.
    Returns dict(weight fp64 [G, n_obs], bias fp64 [G], per_env fp64 [N, n_obs + 1], bound fp64 [G, n_obs + 1],
    delta, Q fp64 [S, N])."""
    action, valid = np.asarray(action).astype(np.float64), np.asarray(valid).astype(bool)
    S, N = valid.shape
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64).reshape(-1)
    G = W.shape[0] if n_groups is None else int(n_groups)
    g = np.zeros(N, np.int64) if group is None else np.asarray(group, np.int64)
    o = np.asarray(obs, np.float64)[:S]
    z = np.einsum("snj,nj->sn", o, W[g]) + b[g][None, :]
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-z))
    m = valid & ~np.asarray(forced).astype(bool)
    delta = np.where(m, action - p, 0.0)
    with np.errstate(invalid="ignore"):  # entries of days an env did not step are unspecified (any bits)
        A = np.asarray(reward, np.float64) - (0.0 if baseline_reward is None else np.asarray(baseline_reward, np.float64))
    A = np.where(valid, A, 0.0)
    Q = np.cumsum(A[::-1], axis=0)[::-1]
    days_left = np.cumsum(valid[::-1].astype(np.float64), axis=0)[::-1]
    o1 = np.concatenate([np.where(valid[:, :, None], o, 0.0), valid[:, :, None].astype(np.float64)], axis=2)
    per_env = np.einsum("sn,snj->nj", delta * Q, o1)
    per_env_bound = np.einsum("sn,snj->nj", np.abs(delta) * 2e-5 * days_left + 1e-6 * np.abs(Q) * valid, np.abs(o1))
    grad = np.full((G, o1.shape[2]), np.nan)
    bound = np.full((G, o1.shape[2]), np.nan)
    for k in range(G):
        if (g == k).any():
            grad[k] = per_env[g == k].mean(axis=0)
            bound[k] = per_env_bound[g == k].mean(axis=0)
    return dict(weight=grad[:, :-1], bias=grad[:, -1], per_env=per_env, bound=bound, delta=delta, Q=Q)
