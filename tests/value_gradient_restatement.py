"""NumPy fp64 restatement of value_gradient() (w2a_value_gradient_linear / _mlp, include/w2a.h), shared by
tests/test_value_gradient_cpu.py and tests/test_value_gradient_gpu.py. From the rows held before every decision, the
per-day rewards, which days were stepped (valid) and a weight per env:

    Q_s = sum_{s' >= s, valid} r_s',   V_s = z(o_s),   A_s = Q_s - V_s  (the "advantage"),
    g_e = w_e sum_s A_s dV_s/dtheta,   per group the mean of g_e over its envs (NaN for a group without envs),
    sq_e = sum_s A_s^2,   ret_e = Q_0,   group_loss = mean_e 1/2 w_e sq_e.

z = W[g] . o + b[g] (linear) or the network's fp64 logit on the f32 parameters (mlp; a two-row output folded into
row1 - row0 and rounded to f32 once, as the host does, the gradient going back as +g on row 1 and -g on row 0).
`residual` replaces A_s (the CPU test's mutants: telescoped() with a fault built in).
weighted_imitation_*_fp64 restate imitation_gradient(day_weight=...): tests/imitation_restatement.py's estimator and
bound with w_e replaced by w_e d_{s,e} on every day.

The kernels take A_s as total - prefix_s of the one-step residuals y_s = r_s + V_{s+1} - V_s (V := 0 past the env's last
stepped day); telescoped() restates that route so that the CPU test can hold it to Q_s - V_s.

The bounds are those of tests/policy_gradient_restatement.py, tests/policy_gradient_mlp_restatement.py and
tests/imitation_restatement.py with the per-day coefficient c_s = w_e A_s. u = 2^-24. The error e_A of A_s:

    reward      1e-5 per reward and day (the project's reward bar), so 1e-5 (valid days from s on) for Q_s
    V_s         linear: the kernel's chain is fp64 like the restated sum, in another order: 31 terms, <= 31 2^-53 M_s;
                the fp64 sums of y over <= S days likewise. 1e-12 (M_s + sum_{s' >= s} |y_s'|) holds both with orders of
                magnitude to spare for any S the tables allow.
                mlp: e_z M_s, the f32 logit's distance from the fp64 one as policy_gradient_mlp_restatement.py derives it
                (M_s = |b_out| + |w_out| . m_last, e_z = u (K1 + K2 + K_out + 2 L)).
    y in f32    (mlp only: the scratch holds y_s as f32) the kernel's total is the fp64 sum of the ROUNDED y_s, so
                total - prefix_s is exactly the sum of the stored residuals from day s on: each is within u |y_s'| of the
                unrounded one, and the unrounded ones telescope. |y_s'| is taken from the restatement plus its own
                first-order error e_y = 1e-5 + e_z (M_s' + M_s'+1):   u sum_{s' >= s} (|y_s'| + e_y,s')
    linear  e_A,s = 1e-5 days_s + 1e-12 (M_s + sum_{s' >= s} |y_s'|)
    mlp     e_A,s = 1e-5 days_s + e_z M_s + u sum_{s' >= s} (|y_s'| + e_y,s')

    linear  bound[g, j] = mean_e sum_s |o_sj| (|w_e| e_A,s + 2^-23 |c_s|)     (g_e and the group mean are each rounded to
                                                                              f32 once: 2^-24 of the terms' magnitudes)
    mlp     bound_theta = mean_e sum_s ( |dV_s/dtheta|_abs (|w_e| e_A,s + eps |c_s|)
                                         + |c_s| (|dV_s/dtheta|_abs,err - |dV_s/dtheta|_abs) )
            eps = u (K2 + 8 + 16 S): c_s rounded to f32 once, the f32 backward pass and the f32 sums over a tile's days,
            and the second term (f32 activations, tanh' formed from them, the near-kink ReLU rule), exactly as
            policy_gradient_mlp_restatement.py derives them
    adv     e_A,s + 2^-23 |A_s|                      (one rounding to f32)
    sq      sum_s (2 |A_s| e_A,s + e_A,s^2) + 2^-23 sq_e
    ret     1e-5 days_e + 2^-23 |ret_e|              (the suite's return bar)
    group_loss   the mean of |w_e| / 2 times each env's sq bound, and 2^-22 of the mean |w_e sq_e| / 2 (the host takes
                 the mean of f32 values in fp64 and rounds it to f32: two roundings at most per value)
_mlp_core is the third copy of the forward pass, the backward pass and the bound terms of
policy_gradient_mlp_restatement.py and imitation_restatement.py (those files are fixed yardsticks and offer no
coefficient hook, so it could not be shared from here): a change to the derivation has to be made in all three until
they are factored into one core that takes the per-day coefficient and its error as a callback, as _mlp_core does.
No number here was fitted to a kernel's output. `near_kink` reports the fraction of ReLU unit-days within the kink rule
(no case is excluded: the rule widens the bound)."""
from __future__ import annotations

import numpy as np

from policy_gradient_mlp_restatement import U, _fold


def _suffix(x):
    """sum over s' >= s along axis 0"""
    return np.cumsum(x[::-1], axis=0)[::-1]


def telescoped(reward, V, valid, drop_next=False, bootstrap=None):
    """A_s [S, N] by the kernels' route: y_s = r_s + V_{s+1} - V_s, V_{s+1} := 0 when the env does not step on call-day
    s + 1 (its episode ended, or the call did); total = sum_s y_s; A_s = total - sum_{s' < s} y_s'. Also returns y.
    Mutants: drop_next leaves V_{s+1} out; bootstrap [N] (the value of the row the call leaves behind) is used as V past
    the call's last day for envs still running -- bootstrapping past a truncated chunk."""
    valid = np.asarray(valid).astype(bool)
    S, N = valid.shape
    r, V = np.where(valid, np.asarray(reward, np.float64), 0.0), np.where(valid, np.asarray(V, np.float64), 0.0)
    nxt = np.concatenate([V[1:], np.zeros((1, N))], axis=0)  # V is already 0 where the env does not step
    if bootstrap is not None:
        nxt[S - 1] = np.where(valid[S - 1], np.asarray(bootstrap, np.float64), 0.0)
    if drop_next:
        nxt = np.zeros_like(nxt)
    y = np.where(valid, r + nxt - V, 0.0)
    total = y.sum(axis=0)
    prefix = np.cumsum(y, axis=0) - y
    return np.where(valid, total[None, :] - prefix, 0.0), y


def _front(valid, reward, weights, group, n_groups, G_params):
    valid = np.asarray(valid).astype(bool)
    S, N = valid.shape
    w = np.ones(N) if weights is None else np.asarray(weights, np.float64)
    G = G_params if n_groups is None else int(n_groups)
    g = np.zeros(N, np.int64) if group is None else np.asarray(group, np.int64)
    with np.errstate(invalid="ignore"):
        r = np.where(valid, np.asarray(reward, np.float64), 0.0)
    return valid, S, N, w, G, g, r, _suffix(r), _suffix(valid.astype(np.float64))


def _per_env(A, eA, Q, days_left, valid):
    sq = (A * A).sum(axis=0)
    ret = Q[0]
    return dict(advantage=A, adv_bound=(eA + 2.0 ** -23 * np.abs(A)) * valid, sq=sq,
                sq_bound=(2.0 * np.abs(A) * eA + eA * eA).sum(axis=0) + 2.0 ** -23 * sq, ret=ret,
                ret_bound=1e-5 * days_left[0] + 2.0 ** -23 * np.abs(ret), days=valid.sum(axis=0))


def _group_loss(w, sq, sq_bound, g, G):
    loss, bound = np.full(G, np.nan), np.full(G, np.nan)
    for k in range(G):
        if (g == k).any():
            loss[k] = (0.5 * w * sq)[g == k].mean()
            bound[k] = (0.5 * np.abs(w) * sq_bound)[g == k].mean() + 2.0 ** -22 * np.abs(0.5 * w * sq)[g == k].mean()
    return loss, bound


def value_linear_fp64(obs, valid, reward, weights, W, b, group, n_groups=None, residual=None):
    """obs [>= S, N, n_obs] (slab s: the row held before decision s), valid / reward [S, N], weights [N] or None,
    W [G, n_obs], b [G], group int [N] or None. Returns dict(weight [G, n_obs], bias [G], per_env [N, n_obs + 1], bound
    [G, n_obs + 1], V, advantage, adv_bound [S, N], sq, sq_bound, ret, ret_bound, days [N], group_loss,
    group_loss_bound [G])."""
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64).reshape(-1)
    valid, S, N, w, G, g, r, Q, days_left = _front(valid, reward, weights, group, n_groups, W.shape[0])
    o = np.where(valid[:, :, None], np.asarray(obs, np.float64)[:S], 0.0)
    V = np.where(valid, np.einsum("snj,nj->sn", o, W[g]) + b[g][None, :], 0.0)
    M = np.where(valid, np.einsum("snj,nj->sn", np.abs(o), np.abs(W[g])) + np.abs(b[g])[None, :], 0.0)
    A = np.where(valid, Q - V, 0.0) if residual is None else np.asarray(residual, np.float64)
    y = telescoped(r, V, valid)[1]
    eA = (1e-5 * days_left + 1e-12 * (M + _suffix(np.abs(y)))) * valid
    c = w[None, :] * A
    o1 = np.concatenate([o, valid[:, :, None].astype(np.float64)], axis=2)
    per_env = np.einsum("sn,snj->nj", c, o1)
    per_env_bound = np.einsum("sn,snj->nj", np.abs(w)[None, :] * eA + 2.0 ** -23 * np.abs(c), np.abs(o1))
    grad, bound = np.full((G, o1.shape[2]), np.nan), np.full((G, o1.shape[2]), np.nan)
    for k in range(G):
        if (g == k).any():
            grad[k], bound[k] = per_env[g == k].mean(axis=0), per_env_bound[g == k].mean(axis=0)
    out = _per_env(A, eA, Q, days_left, valid)
    out["group_loss"], out["group_loss_bound"] = _group_loss(w, out["sq"], out["sq_bound"], g, G)
    out.update(weight=grad[:, :-1], bias=grad[:, -1], per_env=per_env, bound=bound, V=V)
    return out


def _mlp_core(layers, activation, obs, valid, group, n_groups, coef):
    """The forward pass, the coefficient rule `coef(sel, z, M, e_z, eps) -> (c, cb)` per group (c_s the per-day
    coefficient of dz_s/dtheta, cb_s the bound of its error including eps |c_s|) and the backward pass with its bound,
    exactly as policy_gradient_mlp_restatement.py lays them out. Returns (grads, bounds, near_kink)."""
    L, n_out = _fold(layers)
    nl = len(L) - 1
    valid = np.asarray(valid).astype(bool)
    S, N = valid.shape
    G = max(W.shape[0] for W, _ in L) if n_groups is None else int(n_groups)
    g = np.zeros(N, np.int64) if group is None else np.asarray(group, np.int64)
    x_all = np.where(valid[:, :, None], np.asarray(obs, np.float64)[:S], 0.0)
    act = np.tanh if activation == "tanh" else (lambda v: np.maximum(v, 0.0))
    dact = (lambda h, pre: 1.0 - h * h) if activation == "tanh" else (lambda h, pre: (pre > 0).astype(np.float64))
    grads = [(np.full((G,) + W.shape[1:], np.nan), np.full((G,) + b.shape[1:], np.nan)) for W, b in L]
    bounds = [(np.full((G,) + W.shape[1:], np.nan), np.full((G,) + b.shape[1:], np.nan)) for W, b in L]
    kink_n = kink_d = 0
    for k in range(G):
        sel = g == k
        n_k = int(sel.sum())
        if n_k == 0:
            continue
        P = [(W[k if W.shape[0] > 1 else 0], b[k if b.shape[0] > 1 else 0]) for W, b in L]
        x, vk = x_all[:, sel], valid[:, sel]
        hs, pres, mags = [x], [], [np.abs(x)]
        for W, b in P[:-1]:
            pres.append(np.einsum("snj,uj->snu", hs[-1], W) + b)
            mags.append(np.einsum("snj,uj->snu", mags[-1], np.abs(W)) + np.abs(b))
            hs.append(act(pres[-1]))
        wo, bo = P[-1][0][0], P[-1][1][0]
        z = hs[-1] @ wo + bo
        M = mags[-1] @ np.abs(wo) + abs(bo)
        K = [P[i][0].shape[1] + 1 for i in range(nl)] + [len(wo) + 3]
        e_z = U * (sum(K) + 2 * nl)
        eps = U * ((K[1] if nl == 2 else 0) + 8 + 16 * S)
        c, cb = coef(sel, z, M, e_z, eps)
        c, cb = c * vk, cb * vk
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

        def absolute(coef_, dacts, hin):
            """the backward pass with absolute values throughout, weighted per env-day by coef_"""
            out = [None] * (nl + 1)
            out[nl] = (np.einsum("sn,snu->u", coef_, hin[nl]) / n_k, coef_.sum() / n_k)
            dh_a = coef_[:, :, None] * np.abs(wo)[None, None, :] * dacts[-1]
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
    return grads, bounds, (kink_n / kink_d if kink_d else 0.0)


def value_mlp_fp64(obs, valid, reward, weights, layers, activation, group, n_groups=None, residual=None):
    """As value_linear_fp64 for layers [(W, b), ...] (torch Linear convention, optional leading G) and an activation.
    Returns dict(layers=[(dW [G, out, in], db [G, out]), ...], bound=[(.., ..), ...], V, advantage, ..., near_kink)."""
    G_params = max((np.asarray(W).shape[0] if np.asarray(W).ndim == 3 else 1) for W, _ in layers)
    valid, S, N, w_all, G, g, r, Q, days_left = _front(valid, reward, weights, group, n_groups, G_params)
    V_all, A_all, eA_all = np.zeros((S, N)), np.zeros((S, N)), np.zeros((S, N))

    def coef(sel, z, M, e_z, eps):
        vk, wk = valid[:, sel], w_all[sel]
        V, M = np.where(vk, z, 0.0), np.where(vk, M, 0.0)
        A = np.where(vk, Q[:, sel] - V, 0.0) if residual is None else np.asarray(residual, np.float64)[:, sel]
        y = telescoped(r[:, sel], V, vk)[1]
        M_next = np.concatenate([M[1:], np.zeros((1, M.shape[1]))], axis=0)
        e_y = (1e-5 + e_z * (M + M_next)) * vk
        eA = (1e-5 * days_left[:, sel] + e_z * M + U * _suffix(np.abs(y) + e_y)) * vk
        V_all[:, sel], A_all[:, sel], eA_all[:, sel] = V, A, eA
        c = A * wk[None, :]
        return c, np.abs(wk)[None, :] * eA + eps * np.abs(c)

    grads, bounds, near = _mlp_core(layers, activation, obs, valid, g if group is not None else None, G, coef)
    out = _per_env(A_all, eA_all, Q, days_left, valid)
    out["group_loss"], out["group_loss_bound"] = _group_loss(w_all, out["sq"], out["sq_bound"], g, G)
    out.update(layers=grads, bound=bounds, V=V_all, near_kink=near)
    return out


def weighted_imitation_linear_fp64(obs, labels, valid, forced, weights, day_weight, W, b, group, n_groups=None):
    """imitation_linear_fp64 (tests/imitation_restatement.py) with a weight per env-day: g_e = w_e sum_s d_{s,e} delta_s
    (o_s, 1); its bound with |w_e| replaced by |w_e d_{s,e}|. day_weight [>= S, N] or None (= 1). Returns dict(weight,
    bias, bound)."""
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64).reshape(-1)
    valid = np.asarray(valid).astype(bool)
    S, N = valid.shape
    m = valid & ~np.asarray(forced).astype(bool)
    w = np.ones(N) if weights is None else np.asarray(weights, np.float64)
    d = np.ones((S, N)) if day_weight is None else np.asarray(day_weight, np.float64)[:S]
    G = W.shape[0] if n_groups is None else int(n_groups)
    g = np.zeros(N, np.int64) if group is None else np.asarray(group, np.int64)
    o = np.where(valid[:, :, None], np.asarray(obs, np.float64)[:S], 0.0)
    z = np.einsum("snj,nj->sn", o, W[g]) + b[g][None, :]
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-z))
    wd = w[None, :] * np.where(m, d, 0.0)
    c = np.where(m, np.asarray(labels).astype(np.float64) - p, 0.0) * wd
    o1 = np.concatenate([o, valid[:, :, None].astype(np.float64)], axis=2)
    per_env = np.einsum("sn,snj->nj", c, o1)
    per_env_bound = np.einsum("sn,snj->nj", np.abs(wd), np.abs(o1)) * 1e-6
    grad, bound = np.full((G, o1.shape[2]), np.nan), np.full((G, o1.shape[2]), np.nan)
    for k in range(G):
        if (g == k).any():
            grad[k], bound[k] = per_env[g == k].mean(axis=0), per_env_bound[g == k].mean(axis=0)
    return dict(weight=grad[:, :-1], bias=grad[:, -1], bound=bound)


def weighted_imitation_mlp_fp64(obs, labels, valid, forced, weights, day_weight, layers, activation, group,
                                n_groups=None):
    """imitation_mlp_fp64 with a weight per env-day: c_s = w_e d_{s,e} delta_s, and its bound with |w_e| replaced by
    |w_e d_{s,e}| (eps_s of imitation_restatement.py: 1e-6 + e_z M_s / 4 for delta, the relative terms on top).
    Returns dict(layers, bound, near_kink)."""
    valid = np.asarray(valid).astype(bool)
    S, N = valid.shape
    m = valid & ~np.asarray(forced).astype(bool)
    w = np.ones(N) if weights is None else np.asarray(weights, np.float64)
    d = np.ones((S, N)) if day_weight is None else np.asarray(day_weight, np.float64)[:S]
    a = np.asarray(labels).astype(np.float64)

    def coef(sel, z, M, e_z, eps):
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-z))
        wd = w[sel][None, :] * np.where(m[:, sel], d[:, sel], 0.0)
        return np.where(m[:, sel], a[:, sel] - p, 0.0) * wd, (1e-6 + e_z * M / 4 + eps) * np.abs(wd)

    grads, bounds, near = _mlp_core(layers, activation, obs, valid, group, n_groups, coef)
    return dict(layers=grads, bound=bounds, near_kink=near)
