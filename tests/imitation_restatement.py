"""NumPy fp64 restatement of imitation_gradient() (w2a_imitation_gradient_linear / _mlp, include/w2a.h), shared by
tests/test_imitation_cpu.py and tests/test_imitation_gpu.py. From the rows held before every decision, the schedule's
attempted actions a*_s, which days were stepped (valid) and which were forced by require_budget, and a weight per env:

    delta_s = m_s (a*_s - sigmoid(z_s)),   m_s = valid_s and not forced_s
    ll_e    = sum_s m_s log pi(a*_s | o_s) = -sum_s m_s softplus(-z_s or z_s)
    g_e     = w_e sum_s delta_s dz_s/dtheta,   per group the mean of g_e over its envs (NaN for a group without envs)

z_s = W[g] . o_s + b[g] (linear) or the network's fp64 logit on the f32 parameters (mlp; a two-row output folded into
row1 - row0 and rounded to f32 once, as the host does, the gradient going back as +g on row 1 and -g on row 0).

The bounds are those of tests/policy_gradient_restatement.py and tests/policy_gradient_mlp_restatement.py with the
reward-to-go Q_s replaced by |w_e| and the reward term (2e-5 per advantage) dropped -- rewards do not enter:

    linear  bound[g, j] = mean_e |w_e| sum_s m_s |o_sj| 1e-6      (the project's f32-sigmoid bar: ~1e-7, taken x 10)
            ll:  2^-23 |ll_e| + 1e-9 days_e       (the kernel's fp64 chain is the restated one up to the order of its sum,
                                                   each term then within far less than 1e-9; one rounding to f32)
    mlp     bound_theta = mean_e sum_s ( |dz_s/dtheta|_abs eps_s |w_e| + |c_s| (|dz_s/dtheta|_abs,err - |dz_s/dtheta|_abs) )
            with eps_s, e_h, the tanh' term and the near-kink ReLU rule exactly as policy_gradient_mlp_restatement.py
            derives them (S there = the call's days), c_s = w_e delta_s
            ll:  sum_s m_s e_z M_s + 2^-23 |ll_e|     (log-sigmoid is 1-Lipschitz in z; e_z M_s bounds the f32 logit)
No number here was fitted to a kernel's output. `near_kink` reports the fraction of ReLU unit-days within the kink rule
(no case is excluded: the rule widens the bound)."""
from __future__ import annotations

import numpy as np

from policy_gradient_mlp_restatement import U, _fold


def log_pi(z, a):
    """log pi(a | z) of pi(1) = sigmoid(z), stable: -softplus(-z) for a = 1, -softplus(z) for a = 0"""
    x = np.where(np.asarray(a).astype(bool), -z, z)
    return -(np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x))))


def attempts_from_schedule(alert_days, t0, valid):
    """a*_s [S, N]: the schedule's bit at the day every env is on at call-day s (it advances one day per valid step)"""
    valid = np.asarray(valid).astype(bool)
    S, N = valid.shape
    tt = np.asarray(t0, np.int64)[None, :] + np.cumsum(valid, axis=0) - valid  # day of the episode before decision s
    tt = np.minimum(tt, alert_days.shape[1] - 1)
    return np.asarray(alert_days).astype(bool)[np.arange(N)[None, :], tt] & valid


def group_ll_bound(w, ll, ll_bound, g, G):
    """bound of "group_log_likelihood": the mean of |w_e| times each env's ll bound, and 2^-22 of the mean |w_e ll_e|
    (the host takes the mean of f32 values in fp64 and rounds it to f32: two roundings at most per value)"""
    out = np.full(G, np.nan)
    for k in range(G):
        if (g == k).any():
            out[k] = (np.abs(w) * ll_bound)[g == k].mean() + 2.0 ** -22 * np.abs(w * ll)[g == k].mean()
    return out


def _front(labels, valid, forced, weights, group, n_groups, G_params):
    valid = np.asarray(valid).astype(bool)
    S, N = valid.shape
    m = valid & ~np.asarray(forced).astype(bool)
    a = np.asarray(labels).astype(np.float64)
    w = np.ones(N) if weights is None else np.asarray(weights, np.float64)
    G = G_params if n_groups is None else int(n_groups)
    g = np.zeros(N, np.int64) if group is None else np.asarray(group, np.int64)
    return valid, S, N, m, a, w, G, g


def imitation_linear_fp64(obs, labels, valid, forced, weights, W, b, group, n_groups=None, use_m=True, use_w=True):
    """obs [>= S, N, n_obs] (slab s: the row held before decision s), labels / valid / forced [S, N], weights [N] or
    None, W [G, n_obs], b [G], group int [N] or None. use_m / use_w = False build the CPU test's mutants.
    Returns dict(weight [G, n_obs], bias [G], per_env [N, n_obs + 1], bound [G, n_obs + 1], ll [N], ll_bound [N],
    days [N], group_ll [G])."""
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64).reshape(-1)
    valid, S, N, m, a, w, G, g = _front(labels, valid, forced, weights, group, n_groups, W.shape[0])
    if not use_m:
        m = valid
    if not use_w:
        w = np.ones(N)
    o = np.where(valid[:, :, None], np.asarray(obs, np.float64)[:S], 0.0)
    z = np.einsum("snj,nj->sn", o, W[g]) + b[g][None, :]
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-z))
    delta = np.where(m, a - p, 0.0)
    o1 = np.concatenate([o, valid[:, :, None].astype(np.float64)], axis=2)
    per_env = w[:, None] * np.einsum("sn,snj->nj", delta, o1)
    per_env_bound = np.abs(w)[:, None] * np.einsum("sn,snj->nj", m.astype(np.float64), np.abs(o1)) * 1e-6
    ll = np.where(m, log_pi(z, a), 0.0).sum(axis=0)
    days = m.sum(axis=0)
    grad, bound, gll = np.full((G, o1.shape[2]), np.nan), np.full((G, o1.shape[2]), np.nan), np.full(G, np.nan)
    ll_bound = 2.0 ** -23 * np.abs(ll) + 1e-9 * days
    for k in range(G):
        if (g == k).any():
            grad[k], bound[k] = per_env[g == k].mean(axis=0), per_env_bound[g == k].mean(axis=0)
            gll[k] = (w * ll)[g == k].mean()
    return dict(weight=grad[:, :-1], bias=grad[:, -1], per_env=per_env, bound=bound, ll=ll, ll_bound=ll_bound,
                days=days, group_ll=gll, group_ll_bound=group_ll_bound(w, ll, ll_bound, g, G))


def imitation_mlp_fp64(obs, labels, valid, forced, weights, layers, activation, group, n_groups=None, use_m=True,
                       use_w=True):
    """As imitation_linear_fp64 for layers [(W, b), ...] (torch Linear convention, optional leading G) and an activation.
    Returns dict(layers=[(dW [G, out, in], db [G, out]), ...], bound=[(.., ..), ...], ll, ll_bound, days, group_ll,
    near_kink)."""
    L, n_out = _fold(layers)
    nl = len(L) - 1
    valid, S, N, m_all, a_all, w_all, G, g = _front(labels, valid, forced, weights, group, n_groups,
                                                    max(W.shape[0] for W, _ in L))
    if not use_m:
        m_all = valid
    if not use_w:
        w_all = np.ones(N)
    x_all = np.where(valid[:, :, None], np.asarray(obs, np.float64)[:S], 0.0)
    act = np.tanh if activation == "tanh" else (lambda v: np.maximum(v, 0.0))
    dact = (lambda h, pre: 1.0 - h * h) if activation == "tanh" else (lambda h, pre: (pre > 0).astype(np.float64))
    grads = [(np.full((G,) + W.shape[1:], np.nan), np.full((G,) + b.shape[1:], np.nan)) for W, b in L]
    bounds = [(np.full((G,) + W.shape[1:], np.nan), np.full((G,) + b.shape[1:], np.nan)) for W, b in L]
    ll, ll_bound, gll = np.zeros(N), np.zeros(N), np.full(G, np.nan)
    kink_n = kink_d = 0
    for k in range(G):
        sel = g == k
        n_k = int(sel.sum())
        if n_k == 0:
            continue
        P = [(W[k if W.shape[0] > 1 else 0], b[k if b.shape[0] > 1 else 0]) for W, b in L]
        x, vk, mk, wk = x_all[:, sel], valid[:, sel], m_all[:, sel], w_all[sel]
        hs, pres, mags = [x], [], [np.abs(x)]
        for W, b in P[:-1]:
            pres.append(np.einsum("snj,uj->snu", hs[-1], W) + b)
            mags.append(np.einsum("snj,uj->snu", mags[-1], np.abs(W)) + np.abs(b))
            hs.append(act(pres[-1]))
        wo, bo = P[-1][0][0], P[-1][1][0]
        z = hs[-1] @ wo + bo
        M = mags[-1] @ np.abs(wo) + abs(bo)
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-z))
        delta = np.where(mk, a_all[:, sel] - p, 0.0)
        c = delta * wk[None, :]
        K = [P[i][0].shape[1] + 1 for i in range(nl)] + [len(wo) + 3]
        e_z = U * (sum(K) + 2 * nl)
        eps = 1e-6 + e_z * M / 4 + U * ((K[1] if nl == 2 else 0) + 8 + 16 * S)
        cb = eps * np.abs(wk)[None, :] * mk
        ll[sel] = np.where(mk, log_pi(z, a_all[:, sel]), 0.0).sum(axis=0)
        ll_bound[sel] = (e_z * M * mk).sum(axis=0) + 2.0 ** -23 * np.abs(ll[sel])
        gll[k] = (wk * ll[sel]).mean()
        da, da_plain, da_err, h_abs, h_err = [], [], [], [np.abs(x)], [np.abs(x)]
        kacc = 0
        for i in range(nl):
            d = dact(hs[i + 1], pres[i])
            kacc += K[i] + 2
            eh = kacc * U * mags[i + 1]  # |h_f32 - h_64| of layer i + 1
            if activation == "tanh":
                extra = 2.0 * np.abs(hs[i + 1]) * eh
            else:
                near = np.abs(pres[i]) <= 1e-5 * mags[i + 1]
                kink_n += int((near & vk[:, :, None]).sum())
                kink_d += int(vk.sum()) * pres[i].shape[2]
                extra = near.astype(np.float64)
            da.append(d)
            da_plain.append(np.abs(d))
            da_err.append(np.abs(d) + extra)
            h_abs.append(np.abs(hs[i + 1]))
            h_err.append(np.abs(hs[i + 1]) + eh)

        def absolute(coef, dacts, hin):
            """the backward pass with absolute values throughout, weighted per env-day by coef"""
            out = [None] * (nl + 1)
            out[nl] = (np.einsum("sn,snu->u", coef, hin[nl]) / n_k, coef.sum() / n_k)
            dh_a = coef[:, :, None] * np.abs(wo)[None, None, :] * dacts[-1]
            for i in range(nl - 1, -1, -1):
                out[i] = (np.einsum("snu,snj->uj", dh_a, hin[i]) / n_k, dh_a.sum(axis=(0, 1)) / n_k)
                if i > 0:
                    dh_a = np.einsum("snu,uj->snj", dh_a, np.abs(P[i][0])) * dacts[i - 1]
            return out

        rel = absolute(cb, da_plain, h_abs)
        hi_, lo_ = absolute(np.abs(c), da_err, h_err), absolute(np.abs(c), da_plain, h_abs)
        for i in range(nl + 1):
            bW, bb = rel[i][0] + (hi_[i][0] - lo_[i][0]), rel[i][1] + (hi_[i][1] - lo_[i][1])
            if i == nl:
                bounds[i][0][k, 0], bounds[i][1][k, 0] = bW, bb
            else:
                bounds[i][0][k], bounds[i][1][k] = bW, bb
        dh = c[:, :, None] * wo[None, None, :] * da[-1]
        grads[-1][0][k, 0], grads[-1][1][k, 0] = np.einsum("sn,snu->u", c, hs[-1]) / n_k, c.sum() / n_k
        for i in range(nl - 1, -1, -1):
            grads[i][0][k] = np.einsum("snu,snj->uj", dh, hs[i]) / n_k
            grads[i][1][k] = dh.sum(axis=(0, 1)) / n_k
            if i > 0:
                dh = np.einsum("snu,uj->snj", dh, P[i][0]) * da[i - 1]
    if n_out == 2:  # the adjoint of the fold: +g on row 1, -g on row 0
        for arr, sign in ((grads, -1.0), (bounds, 1.0)):
            W, b = arr[-1]
            arr[-1] = (np.concatenate([sign * W, W], axis=1), np.concatenate([sign * b, b], axis=1))
    return dict(layers=grads, bound=bounds, ll=ll, ll_bound=ll_bound, days=m_all.sum(axis=0), group_ll=gll,
                group_ll_bound=group_ll_bound(w_all, ll, ll_bound, g, G), near_kink=(kink_n / kink_d if kink_d else 0.0))
