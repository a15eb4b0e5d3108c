"""NumPy fp64 restatement of value_gradient(gamma=, gae_lambda=, bootstrap=, value_target=, target=)
(w2a_value_gradient_linear_gae / _mlp_gae, include/w2a.h), shared by tests/test_gae_cpu.py and tests/test_gae_gpu.py.
From the rows held before every decision (S + 1 slabs: the last is the row the call leaves behind), the per-day
rewards, which days were stepped (valid), which envs are still running after the call (alive_after) and a weight per env:

    V_s     = z(o_s)
    Vn_s    = z(o_{s+1}) while the env holds a row after day s inside the call; 0 on the episode's last day; on the
              call's last day of an unfinished episode z(o_S) with bootstrap, else 0
    delta_s = r_s + gamma Vn_s - V_s,   A_s = delta_s + gamma lambda A_{s+1}  (A = 0 past the env's last day),
    R_s     = A_s + V_s,   c_s = A_s,   or   c_s = target[s, e] - V_s   with targets given
    g_e     = w_e sum_s c_s dV_s/dtheta,   per group the mean over its envs,   sq_e = sum_s c_s^2,   ret_e = sum_s r_s.

z as tests/value_gradient_restatement.py has it (whose _mlp_core, _front and _group_loss are used: the forward pass, the
backward pass and the second pass's bound terms are the critic's, with another per-day coefficient).

The bounds, with u = 2^-24 and k = gamma lambda. Nothing here was fitted to a kernel's output.

    reward     1e-5 per reward and day (the project's reward bar) enters delta_s once.
    e_V,s      the kernel's V_s against the restated one. linear: both are fp64 chains of 31 terms in another order,
               1e-12 M_s holds that with orders of magnitude to spare (M_s = |b| + sum_j |W_j| |o_sj|). mlp: e_z M_s, the
               f32 logit's distance from the fp64 one as policy_gradient_mlp_restatement.py derives it.
    e_d,s      of delta_s: 1e-5 + e_V,s + gamma e_Vn,s, where e_Vn,s is e_V of the row Vn_s was read on (0 where Vn_s is
               0). mlp only: the scratch holds delta_s as f32, one rounding of the value the kernel formed, which is
               within e_d of the restated one:  + u (|delta_s| + 1e-5 + e_V,s + gamma e_Vn,s).
    e_A,s      = e_d,s + k e_A,s+1: the errors of the residuals enter A_s with the weights of the recursion itself, so
               they accumulate geometrically, e_A,s = sum_{s' >= s} k^(s' - s) e_d,s'. The kernel's recursion is one
               fp64 fma per day: 1e-12 sum_{s' >= s} k^(s' - s) |delta_s'| holds its roundings with room to spare.
    e_c,s      = e_A,s;   with targets: e_V,s + 1e-12 |c_s| (the f32 target is an input, exact in both).
    advantage  e_A,s + 2^-23 |A_s|                       (one rounding to f32)
    value_target  e_A,s + e_V,s + 2^-23 |R_s|            (the sum of two held values, one rounding)
    sq         sum_s (2 |c_s| e_c,s + e_c,s^2) + 2^-23 sq_e
    ret        1e-5 days_e + 2^-23 |ret_e|               (the suite's return bar; undiscounted)
    linear  bound[g, j] = mean_e sum_s |o_sj| (|w_e| e_c,s + 2^-23 |w_e c_s|)
    mlp     _mlp_core's bound with the coefficient w_e c_s and its error |w_e| e_c,s + eps |w_e c_s|: w_e c_s is rounded
            to f32 once, then the second pass, its sums and the reduction are the critic's, run unchanged.
            eps = u (K2 + 8 + 16 S) counts the S days pass 2 sums, not the extra row a bootstrap evaluates.
    group_loss  as tests/value_gradient_restatement.py.

`mutant` builds one fault in (tests/test_gae_cpu.py): "gamma_dropped" leaves gamma out of Vn_s, "lambda_only" decays the
recursion by lambda alone, "terminal_bootstrap" reads the row after the episode's last day as Vn_s, "call_end_start"
starts the recursion at the call's last day and so reads records an env that stopped earlier never wrote."""
from __future__ import annotations

import numpy as np

from policy_gradient_mlp_restatement import U
from value_gradient_restatement import _front, _group_loss, _mlp_core


def sb3_style_gae(reward, V, V_last, valid, alive_after, gamma, lam, bootstrap):
    """An independently written backward loop in the manner of stable-baselines3's compute_returns_and_advantage
    (last_gae_lam, next_non_terminal), per env over its own stepped days. reward, V, valid [S, N]; V_last [N] the value
    of the row the call leaves behind. Returns (advantage, returns) [S, N], zero where the env does not step."""
    S, N = valid.shape
    adv, ret = np.zeros((S, N)), np.zeros((S, N))
    for e in range(N):
        days = int(valid[:, e].sum())
        assert valid[:days, e].all()
        last_gae_lam = 0.0
        for step in reversed(range(days)):
            if step == days - 1:
                truncated = bool(alive_after[e])  # the call ended, the episode did not
                next_non_terminal = 1.0 if (truncated and bootstrap) else 0.0
                next_value = V_last[e]
            else:
                next_non_terminal = 1.0
                next_value = V[step + 1, e]
            delta = reward[step, e] + gamma * next_value * next_non_terminal - V[step, e]
            last_gae_lam = delta + gamma * lam * next_non_terminal * last_gae_lam
            adv[step, e] = last_gae_lam
        ret[:days, e] = adv[:days, e] + V[:days, e]
    return adv, ret


def _next_rows(valid, alive_after, bootstrap):
    """bool [S, N]: day s's Vn_s is the value of slab s + 1"""
    S = valid.shape[0]
    nxt = np.zeros_like(valid)
    nxt[:-1] = valid[1:]  # the env steps again inside the call: it holds a row after day s
    if bootstrap:
        nxt[S - 1] = valid[S - 1] & np.asarray(alive_after).astype(bool)
    return nxt


def gae_rows(r, V, M, valid, alive_after, gamma, lam, bootstrap, e_scale, f32_delta, target=None, mutant=None):
    """The estimator and the bounds of its per-day scalars. r, valid [S, N]; V, M [S + 1, N] (the value of every slab
    and the magnitude sum behind it; slab S is looked at only where bootstrap reads it). e_scale: e_V,s = e_scale M_s.
    Returns dict(A, R, delta, c, e_c, e_A, e_R) [S, N], zero where the env does not step."""
    valid = np.asarray(valid).astype(bool)
    S, N = valid.shape
    nxt = _next_rows(valid, alive_after, bootstrap)
    if mutant == "terminal_bootstrap":  # the row after the env's last stepped day, episode over or not
        nxt = valid.copy()
    Vs, Ms = np.where(valid, V[:S], 0.0), np.where(valid, M[:S], 0.0)
    Vn, Mn = np.where(nxt, V[1:S + 1], 0.0), np.where(nxt, M[1:S + 1], 0.0)
    eV, eVn = e_scale * Ms, e_scale * Mn
    if target is not None:
        c = np.where(valid, np.asarray(target, np.float64)[:S] - Vs, 0.0)
        zero = np.zeros((S, N))
        return dict(A=zero, R=zero, delta=zero, c=c, e_c=(eV + 1e-12 * np.abs(c)) * valid, e_A=zero, e_R=zero)
    g_vn = 1.0 if mutant == "gamma_dropped" else gamma
    k = lam if mutant == "lambda_only" else gamma * lam
    delta = np.where(valid, r + g_vn * Vn - Vs, 0.0)
    e_d = (1e-5 + eV + gamma * eVn) * valid
    if f32_delta:
        e_d = e_d + U * (np.abs(delta) + e_d) * valid
    A, e_A, acc_d = np.zeros((S, N)), np.zeros((S, N)), np.zeros((S, N))
    a, ea, ad = np.zeros(N), np.zeros(N), np.zeros(N)
    # what a sweep from the call's last day reads past the env's own: the scratch is not written there, so it holds
    # what an earlier call left -- taken here as the env's own last record, repeated
    last_day = np.maximum(valid.sum(axis=0) - 1, 0)
    stale = np.where(valid, delta, delta[last_day, np.arange(N)][None, :] * valid.any(axis=0)[None, :])
    for s in range(S - 1, -1, -1):
        live = valid[s]
        if mutant == "call_end_start":  # one recursion for the whole wave, from the call's last day
            a = stale[s] + k * a
        else:
            a = np.where(live, delta[s] + k * a, 0.0)
        ea = np.where(live, e_d[s] + k * ea, 0.0)
        ad = np.where(live, np.abs(delta[s]) + k * ad, 0.0)
        A[s], e_A[s], acc_d[s] = np.where(live, a, 0.0), ea, ad
    e_A = e_A + 1e-12 * acc_d
    R = np.where(valid, A + Vs, 0.0)
    return dict(A=A, R=R, delta=delta, c=A, e_c=e_A, e_A=e_A, e_R=(e_A + eV) * valid)


def _per_env(rows, r, valid, days_left, target):
    c, e_c = rows["c"], rows["e_c"]
    sq = (c * c).sum(axis=0)
    ret = r.sum(axis=0)
    out = dict(advantage=rows["A"], adv_bound=(rows["e_A"] + 2.0 ** -23 * np.abs(rows["A"])) * valid,
               value_target=rows["R"], vt_bound=(rows["e_R"] + 2.0 ** -23 * np.abs(rows["R"])) * valid,
               delta=rows["delta"], coef=c, sq=sq, sq_bound=(2.0 * np.abs(c) * e_c + e_c * e_c).sum(axis=0) + 2.0 ** -23 * sq,
               days=valid.sum(axis=0))
    if target is None:
        out.update(ret=ret, ret_bound=1e-5 * days_left[0] + 2.0 ** -23 * np.abs(ret))
    return out


def gae_linear_fp64(obs, valid, reward, alive_after, weights, W, b, group, n_groups=None, gamma=1.0, lam=1.0,
                    bootstrap=False, target=None, mutant=None):
    """obs [>= S + 1, N, n_obs] (slab s: the row held before decision s; slab S: the row the call leaves behind),
    valid / reward [S, N], alive_after bool [N], weights [N] or None, W [G, n_obs], b [G], group int [N] or None.
    Returns dict(weight, bias, per_env, bound, V, advantage, adv_bound, value_target, vt_bound, sq, sq_bound, ret,
    ret_bound, days, group_loss, group_loss_bound)."""
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64).reshape(-1)
    valid, S, N, w, G, g, r, _, days_left = _front(valid, reward, weights, group, n_groups, W.shape[0])
    o_all = np.asarray(obs, np.float64)[:S + 1]
    V = np.einsum("snj,nj->sn", o_all, W[g]) + b[g][None, :]
    M = np.einsum("snj,nj->sn", np.abs(o_all), np.abs(W[g])) + np.abs(b[g])[None, :]
    rows = gae_rows(r, V, M, valid, alive_after, gamma, lam, bootstrap, 1e-12, False, target, mutant)
    o = np.where(valid[:, :, None], o_all[:S], 0.0)
    c = w[None, :] * rows["c"]
    o1 = np.concatenate([o, valid[:, :, None].astype(np.float64)], axis=2)
    per_env = np.einsum("sn,snj->nj", c, o1)
    per_env_bound = np.einsum("sn,snj->nj", np.abs(w)[None, :] * rows["e_c"] + 2.0 ** -23 * np.abs(c), np.abs(o1))
    grad, bound = np.full((G, o1.shape[2]), np.nan), np.full((G, o1.shape[2]), np.nan)
    for k in range(G):
        if (g == k).any():
            grad[k], bound[k] = per_env[g == k].mean(axis=0), per_env_bound[g == k].mean(axis=0)
    out = _per_env(rows, r, valid, days_left, target)
    out["group_loss"], out["group_loss_bound"] = _group_loss(w, out["sq"], out["sq_bound"], g, G)
    out.update(weight=grad[:, :-1], bias=grad[:, -1], per_env=per_env, bound=bound, V=np.where(valid, V[:S], 0.0),
               V_last=V[S])
    return out


def gae_mlp_fp64(obs, valid, reward, alive_after, weights, layers, activation, group, n_groups=None, gamma=1.0, lam=1.0,
                 bootstrap=False, target=None, mutant=None):
    """As gae_linear_fp64 for layers [(W, b), ...] (torch Linear convention, optional leading G) and an activation.
    Returns dict(layers=[(dW, db), ...], bound=[(.., ..), ...], V, advantage, ..., near_kink)."""
    G_params = max((np.asarray(W).shape[0] if np.asarray(W).ndim == 3 else 1) for W, _ in layers)
    valid, S, N, w_all, G, g, r, _, days_left = _front(valid, reward, weights, group, n_groups, G_params)
    alive = np.asarray(alive_after).astype(bool)
    # slab S joins the forward pass with a zero coefficient wherever some env's Vn is read on it
    last = valid[S - 1] & alive if (bootstrap or mutant == "terminal_bootstrap") else np.zeros(N, bool)
    if mutant == "terminal_bootstrap":
        last = valid[S - 1].copy()
    ext = np.concatenate([valid, last[None, :]], axis=0)
    keys = ("A", "R", "delta", "c", "e_c", "e_A", "e_R")
    full = {k: np.zeros((S, N)) for k in keys}
    V_all = np.zeros((S + 1, N))

    def coef(sel, z, M, e_z, eps):
        vk = ext[:, sel]
        Vk, Mk = np.where(vk, z, 0.0), np.where(vk, M, 0.0)
        rows = gae_rows(r[:, sel], Vk, Mk, valid[:, sel], alive[sel], gamma, lam, bootstrap, e_z, True,
                        None if target is None else np.asarray(target, np.float64)[:S, sel], mutant)
        for k in keys:
            full[k][:, sel] = rows[k]
        V_all[:, sel] = Vk
        wk = w_all[sel]
        c = rows["c"] * wk[None, :]
        cb = np.abs(wk)[None, :] * rows["e_c"] + (eps - 16 * U) * np.abs(c)  # eps counted S + 1 rows: pass 2 sums S
        zero = np.zeros((1, c.shape[1]))
        return np.concatenate([c, zero], axis=0), np.concatenate([cb, zero], axis=0)

    grads, bounds, near = _mlp_core(layers, activation, np.asarray(obs, np.float64)[:S + 1], ext,
                                    g if group is not None else None, G, coef)
    out = _per_env(full, r, valid, days_left, target)
    out["group_loss"], out["group_loss_bound"] = _group_loss(w_all, out["sq"], out["sq_bound"], g, G)
    out.update(layers=grads, bound=bounds, V=V_all[:S] * valid, V_last=V_all[S], near_kink=near)
    return out
