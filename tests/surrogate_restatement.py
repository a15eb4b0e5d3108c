"""NumPy fp64 restatement of surrogate_gradient() (w2a_surrogate_gradient_linear / _mlp, include/w2a.h), shared by
tests/test_surrogate_cpu.py and tests/test_surrogate_gpu.py. From the rows held before every decision, the schedule's
attempted actions a_s, which days were stepped (valid) and which were forced by require_budget, a weight per env, the
advantage A [S, N] and the old log-probabilities [S, N] (or None), on the scored days m_s = valid_s and not forced_s:

    lp_s   = log pi(a_s | z_s),   rho_s = exp(lp_s - old_s)   (1 for old = None),   p_s = sigmoid(z_s)
    live_s = not ((A_s > 0 and rho_s > hi) or (A_s < 0 and rho_s < lo)),   lo, hi = 1 - clip, 1 + clip
    L_e    = sum_s min(rho_s A_s, clamp(rho_s, lo, hi) A_s)
    c_s    = w_e (live_s rho_s A_s (a_s - p_s) + beta (-z_s p_s (1 - p_s)))
    g_e    = sum_s c_s dz_s/dtheta,   per group the mean of g_e over its envs (NaN for a group without envs)
    kl_e   = sum_s (rho_s - 1) - log rho_s,   H_e = sum_s H(p_s),   clipped_e = sum_s not live_s,   days_e = sum_s m_s

z_s as tests/imitation_restatement.py takes it (linear: W[g] . o_s + b[g]; mlp: the network's fp64 logit on the f32
parameters, a two-row output folded and rounded to f32 once as the host does).

The bounds, u = 2^-24. `old` is an INPUT of the call (an f32 array both sides read), so it carries no error here; the f32
rounding of a stored log-probability is the bound of the "log_prob" OUTPUT.
    e_zabs   |z_kernel - z_s|: linear 1e-12 (M_s + 1) (the kernel's fp64 chain is the restated sum in another order:
             31 terms, <= 31 2^-53 M_s, and the fp64 exp / log1p that follow, a few 2^-53 (|lp_s| + 1), as
             value_gradient_restatement.py takes the linear critic's); mlp e_z M_s, the f32 logit's distance from the
             fp64 one as policy_gradient_mlp_restatement.py derives it
    e_lp     = e_zabs: log pi is 1-Lipschitz in z
    e_rho    = rho_s expm1(e_lp)  (0 for old = None: both sides hold rho = 1 exactly)
    e_delta  linear 1e-6, mlp 1e-6 + e_z M_s / 4: the f32 sigmoid, as imitation_restatement.py
    e_dH     = (1 + |z_s|) / 4 e_zabs + 1e-15:  |d(z p q)/dz| = |p q (1 + z (q - p))| <= (1 + |z|) / 4
    cb_s     = |w_e| (live_s |A_s| (e_rho |delta_s| + rho_s e_delta) + |beta| e_dH)
    linear   bound[g, j] = mean_e sum_s |o_sj| (cb_s + 2^-23 |c_s|)   (g_e and the group mean each rounded to f32 once)
    mlp      bound_theta = mean_e sum_s (|dz_s/dtheta|_abs (cb_s + eps |c_s|) + |c_s| (|dz_s/dtheta|_abs,err - |..|_abs)),
             eps and the second term exactly as value_gradient_restatement._mlp_core lays them out (c_s rounded to f32
             once, the f32 backward pass, the f32 sums over a tile's days, the near-kink ReLU rule)
    L        sum_s |A_s| e_rho + 2^-23 |L_e| + 1e-15 sum_s |rho_s A_s|: min(rho A, clamp(rho) A) is continuous in rho with
             slope 0 or A, so the clip edge needs no extra slack here (tighter than |A| clip per ambiguous day)
    kl       sum_s ((|rho_s - 1| + e_rho) e_lp + 1e-15) + 2^-23 kl_e:  d/dd (e^d - 1 - d) = e^d - 1
    H        sum_s (e_zabs / 4 + 1e-15) + 2^-23 H_e:  |dH/dz| = |z p q| < 1/4
    lp       e_lp + 2^-23 |lp_s|
    group_surrogate  as imitation_restatement.group_ll_bound
The clip edge is a discontinuity of live_s. A scored day is AMBIGUOUS when |rho_s - edge| <= rho_s e_lp for the edge that
matters for the sign of A_s (hi for A_s > 0, lo for A_s < 0; never for old = None). No day is left out: an ambiguous day
adds its whole term |w_e rho_s A_s delta_s| to cb_s and 1 to the tolerance of clipped_e. `ambiguous_share` is the
ambiguous days' share of the scored days; every comparison asserts it is at most AMBIGUOUS_CAP, so the rule cannot
swallow a failure.
`mutant` builds the CPU test's faults: "clip_rho_only" (clipping on rho alone, whatever the sign of A), "swap_sign" (the
clip test with the signs of A swapped), "no_rho" (rho dropped from the coefficient), "entropy_sign" (+z p q).
No number here was fitted to a kernel's output."""
from __future__ import annotations

import numpy as np

from imitation_restatement import group_ll_bound, log_pi
from policy_gradient_mlp_restatement import U  # noqa: F401  (2^-24, the name the other restatements use)
from value_gradient_restatement import _mlp_core

AMBIGUOUS_CAP = 0.01


def entropy(z):
    """H(sigmoid(z)) = softplus(z) - z sigmoid(z), stable for either sign"""
    p, q = _pq(z)
    return -(p * log_pi(z, 1) + q * log_pi(z, 0))


def _pq(z):
    e = np.exp(-np.abs(z))
    r = 1.0 / (1.0 + e)
    return np.where(z >= 0, r, e * r), np.where(z >= 0, e * r, r)


def _days(z, e_zabs, e_delta, a, m, w, A, old, clip, beta, mutant):
    """every per-day quantity of the estimator and of its bound for one block of env-days [S, n]; w [n]"""
    lo, hi = 1.0 - clip, 1.0 + clip
    a = np.asarray(a).astype(bool)
    lp = log_pi(z, a)
    d = np.zeros_like(z) if old is None else lp - old
    with np.errstate(over="ignore"):
        rho = np.exp(d)
    p, q = _pq(z)
    delta = a.astype(np.float64) - p
    e_lp = e_zabs
    e_rho = np.zeros_like(z) if old is None else rho * np.expm1(e_lp)
    clip_hi, clip_lo = rho > hi, rho < lo
    As = -A if mutant == "swap_sign" else A
    if mutant == "clip_rho_only":
        live = ~(clip_hi | clip_lo)
    else:
        live = ~(((As > 0) & clip_hi) | ((As < 0) & clip_lo))
    if old is None:
        amb = np.zeros(z.shape, bool)
    else:
        amb = m & (((A > 0) & (np.abs(rho - hi) <= rho * e_lp)) | ((A < 0) & (np.abs(rho - lo) <= rho * e_lp)))
    dH = -z * p * q
    pg = np.where(live, (A if mutant == "no_rho" else rho * A) * delta, 0.0)
    c = np.where(m, w[None, :] * (pg + beta * (-dH if mutant == "entropy_sign" else dH)), 0.0)
    e_dH = 0.25 * (1.0 + np.abs(z)) * e_zabs + 1e-15
    cb = np.abs(w)[None, :] * (live * np.abs(A) * (e_rho * np.abs(delta) + rho * e_delta) + abs(beta) * e_dH)
    cb = np.where(m, cb + amb * np.abs(w[None, :] * rho * A * delta), 0.0)
    mf = m.astype(np.float64)
    L = (mf * np.minimum(rho * A, np.clip(rho, lo, hi) * A)).sum(axis=0)
    kl = (mf * ((rho - 1.0) - d)).sum(axis=0)
    H = (mf * entropy(z)).sum(axis=0)
    return dict(
        m=m, c=c, cb=cb, lp=np.where(m, lp, 0.0), lp_bound=np.where(m, e_lp + 2.0 ** -23 * np.abs(lp), 0.0), rho=np.where(m, rho, 1.0),
        live=live | ~m, ambiguous=amb, L=L,
        L_bound=(mf * (np.abs(A) * e_rho + 1e-15 * np.abs(rho * A))).sum(axis=0) + 2.0 ** -23 * np.abs(L), kl=kl,
        kl_bound=(mf * ((np.abs(rho - 1.0) + e_rho) * e_lp + 1e-15)).sum(axis=0) + 2.0 ** -23 * np.abs(kl), H=H,
        H_bound=(mf * (0.25 * e_zabs + 1e-15)).sum(axis=0) + 2.0 ** -23 * np.abs(H),
        clipped=(m & ~live).sum(axis=0), clipped_tol=amb.sum(axis=0), days=m.sum(axis=0))


_PER_DAY = ("m", "c", "cb", "lp", "lp_bound", "rho", "live", "ambiguous")
_PER_ENV = ("L", "L_bound", "kl", "kl_bound", "H", "H_bound", "clipped", "clipped_tol", "days")


def _front(labels, valid, forced, weights, advantage, old, group, n_groups, G_params):
    valid = np.asarray(valid).astype(bool)
    S, N = valid.shape
    m = valid & ~np.asarray(forced).astype(bool)
    a = np.asarray(labels).astype(bool)
    w = np.ones(N) if weights is None else np.asarray(weights, np.float64)
    A = np.asarray(advantage, np.float64)[:S]
    o = None if old is None else np.asarray(old, np.float64)[:S]
    G = G_params if n_groups is None else int(n_groups)
    g = np.zeros(N, np.int64) if group is None else np.asarray(group, np.int64)
    return valid, S, N, m, a, w, A, o, G, g


def _finish(out, w, g, G):
    scored = int(out["days"].sum())
    out["ambiguous_share"] = float(out["ambiguous"].sum()) / scored if scored else 0.0
    gs = np.full(G, np.nan)
    for k in range(G):
        if (g == k).any():
            gs[k] = (w * out["L"])[g == k].mean()
    out["group_surrogate"], out["group_surrogate_bound"] = gs, group_ll_bound(w, out["L"], out["L_bound"], g, G)
    return out


def surrogate_linear_fp64(obs, labels, valid, forced, weights, advantage, old_log_prob, clip, beta, W, b, group,
                          n_groups=None, mutant=None):
    """obs [>= S, N, n_obs] (slab s: the row held before decision s), labels / valid / forced [S, N], weights [N] or
    None, advantage [>= S, N], old_log_prob [>= S, N] or None, W [G, n_obs], b [G], group int [N] or None.
    Returns dict(weight [G, n_obs], bias [G], bound [G, n_obs + 1], the per-day arrays m, c, cb, lp, lp_bound, rho, live,
    ambiguous [S, N], the per-env L, kl, H, clipped, days and their bounds [N], group_surrogate(_bound) [G],
    ambiguous_share)."""
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64).reshape(-1)
    valid, S, N, m, a, w, A, old, G, g = _front(labels, valid, forced, weights, advantage, old_log_prob, group, n_groups,
                                                W.shape[0])
    o = np.where(valid[:, :, None], np.asarray(obs, np.float64)[:S], 0.0)
    z = np.einsum("snj,nj->sn", o, W[g]) + b[g][None, :]
    M = np.einsum("snj,nj->sn", np.abs(o), np.abs(W[g])) + np.abs(b[g])[None, :]
    out = _days(z, 1e-12 * (M + 1.0), 1e-6, a, m, w, A, old, clip, beta, mutant)
    o1 = np.concatenate([o, valid[:, :, None].astype(np.float64)], axis=2)
    per_env = np.einsum("sn,snj->nj", out["c"], o1)
    per_env_bound = np.einsum("sn,snj->nj", out["cb"] + 2.0 ** -23 * np.abs(out["c"]), np.abs(o1))
    grad, bound = np.full((G, o1.shape[2]), np.nan), np.full((G, o1.shape[2]), np.nan)
    for k in range(G):
        if (g == k).any():
            grad[k], bound[k] = per_env[g == k].mean(axis=0), per_env_bound[g == k].mean(axis=0)
    out.update(weight=grad[:, :-1], bias=grad[:, -1], bound=bound, per_env=per_env)
    return _finish(out, w, g, G)


def surrogate_mlp_fp64(obs, labels, valid, forced, weights, advantage, old_log_prob, clip, beta, layers, activation,
                       group, n_groups=None, mutant=None):
    """As surrogate_linear_fp64 for layers [(W, b), ...] (torch Linear convention, optional leading G) and an activation.
    Returns dict(layers=[(dW [G, out, in], db [G, out]), ...], bound=[(.., ..), ...], near_kink, and the rest as above)."""
    G_params = max((np.asarray(W).shape[0] if np.asarray(W).ndim == 3 else 1) for W, _ in layers)
    valid, S, N, m, a, w, A, old, G, g = _front(labels, valid, forced, weights, advantage, old_log_prob, group, n_groups,
                                                G_params)
    out = {k: np.zeros((S, N), bool if k in ("m", "live", "ambiguous") else np.float64) for k in _PER_DAY}
    out.update({k: np.zeros(N, np.int64 if k in ("clipped", "clipped_tol", "days") else np.float64) for k in _PER_ENV})

    def coef(sel, z, M, e_z, eps):
        r = _days(z, e_z * M, 1e-6 + e_z * M / 4, a[:, sel], m[:, sel], w[sel], A[:, sel],
                  None if old is None else old[:, sel], clip, beta, mutant)
        for k in _PER_DAY:
            out[k][:, sel] = r[k]
        for k in _PER_ENV:
            out[k][sel] = r[k]
        return r["c"], r["cb"] + eps * np.abs(r["c"])

    grads, bounds, near = _mlp_core(layers, activation, obs, valid, g if group is not None else None, G, coef)
    out.update(layers=grads, bound=bounds, near_kink=near)
    return _finish(out, w, g, G)
