"""NumPy fp64 restatement of fisher_vector_product() (w2a_fisher_vector_product_linear / _mlp, include/w2a.h), shared by
tests/test_fisher_cpu.py and tests/test_fisher_gpu.py. The interface is tests/surrogate_restatement.py's: from the rows
held before every decision, the schedule's attempted actions (they enter only through the states visited), which days
were stepped (valid) and which were forced (by require_budget or closed by "allowed_days"), a weight per env and the
vector v in the shape of the policy's parameters, on the scored days m_s = valid_s and not forced_s:

    z_s   the policy's logit on o_s,   p_s = sigmoid(z_s),   J_s = dz_s/dtheta,   u_s = J_s . v_g
    c_s   = w_e p_s (1 - p_s) u_s
    Fv_e  = sum_s m_s c_s J_s^T,        per group the mean of Fv_e over its envs (NaN for a group without envs)
    q_e   = sum_s m_s p_s (1 - p_s) u_s^2  (unweighted),   days_e = sum_s m_s
    group_quadratic[g] = mean over the group's envs of w_e q_e  ( = <v_g, F_g v> )

z_s as tests/imitation_restatement.py takes it (linear: W[g] . o_s + b[g]; mlp: the network's fp64 logit on the f32
parameters, a two-row output folded and rounded to f32 once as the host does). The vector goes the policy's way: a
two-row output block of v is folded into row1 - row0 and rounded to f32 once, and the product comes back as +g on row 1
and -g on row 0. u_s of the MLP kind is the forward-mode tangent
    adot_1 = V1 x + vb1,  hdot_1 = act'(h_1) adot_1,  adot_2 = W2 hdot_1 + V2 h_1 + vb2,  ...,  u = w_o . hdot + v_o . h + vb_o
with act' taken from the activation's value (tanh: 1 - h^2; ReLU: 1 where the pre-activation is positive, 0 at 0).

The bounds, U = 2^-24, by first-order propagation as the other restatements take it.
    e_zabs   |z_kernel - z_s|: linear 1e-12 (M_s + 1) (the kernel's fp64 chain is the restated sum in another order, as
             surrogate_restatement.py); mlp e_z M_s, the f32 logit's distance from the fp64 one as
             policy_gradient_mlp_restatement.py derives it (M_s = |b_out| + |w_out| . m_last, m_i = |b_i| + |W_i| m_{i-1})
    e_pq     = 0.1 e_zabs:  d(p q)/dz = p q (q - p), and |p q (q - p)| <= 1 / (6 sqrt 3) < 0.0963. The kernels form p and
             q = 1 - p in fp64 from exp(-|z|) without cancellation: a few 2^-53 relative, far inside the 1e-15 below
    e_u      |u_kernel - u_s|
             linear: 1e-12 (Mu_s + 1), Mu_s = |vb| + |v| . |o_s|: a second fp64 chain, bounded as z's
             mlp: the f32 tangent. Per layer i (h_0 = x exact, hdot_0 = 0), with e_h,i = U (sum_{j <= i} (K_j + 2)) m_i the
             error of an f32 activation (policy_gradient_mlp_restatement.py) and K_j = fan-in + 1:
               adot_i is one k-ordered f32 fmaf chain of Kd_i = 2 fan-in + 1 terms (vb_i first; a first layer has fan-in
               + 1: hdot_0 = 0 adds no term), so within Kd_i U md_i of the exact sum of its f32 inputs, where
                   md_i = |vb_i| + |W_i| md_{i-1} + |V_i| m_{i-1}          (|hdot| <= |adot| <= md since |act'| <= 1)
               and its inputs carry e_hdot,i-1 and e_h,i-1:
                   e_adot,i = Kd_i U md_i + |W_i| e_hdot,i-1 + |V_i| e_h,i-1
               act' is formed from the f32 activation: tanh' = fma(-h, h, 1) is off by e_d,i = 2 |h_i| e_h,i + U (the
               fma's own rounding, of a value <= 1); ReLU' is exact unless the unit is near its kink (the rule of
               policy_gradient_mlp_restatement.py: |pre| <= 1e-5 m_i), where it may be the other branch: e_d,i = 1
               hdot_i = act' adot_i, one f32 product:
                   e_hdot,i = |act'_i| e_adot,i + e_d,i (|adot_i| + e_adot,i) + U |hdot_i|
             the output is one f32 fmaf chain of 2 fan-in + 1 terms and two adds across lanes (Kd_o = 2 fan-in + 3):
                   e_u = Kd_o U mu + |w_o| . e_hdot,L + |v_o| . e_h,L,    mu = |vb_o| + |w_o| . md_L + |v_o| . m_L
    cb_s     = |w_e| (e_pq |u_s| + p_s q_s e_u) + 1e-15 |c_s|        (c_s is formed in fp64 from z_s and u_s)
    linear   bound[g, j] = mean_e sum_s |o_sj| (cb_s + 2^-23 |c_s|)   (Fv_e and the group mean each rounded to f32 once)
    mlp      bound_theta = mean_e sum_s (|dz_s/dtheta|_abs (cb_s + eps |c_s|) + |c_s| (|dz_s/dtheta|_abs,err - |..|_abs)),
             eps and the second term exactly as value_gradient_restatement._mlp_core lays them out (c_s rounded to f32
             once, the f32 backward pass, the f32 sums over a tile's days, the near-kink ReLU rule): the second pass is
             the kernels of w2a_policy_gradient_mlp, run unchanged
    q        sum_s m_s (e_pq u_s^2 + p_s q_s (2 |u_s| e_u + e_u^2) + 1e-15 p_s q_s u_s^2) + 2^-23 q_e
    group_quadratic  as imitation_restatement.group_ll_bound
A ReLU unit-day near its kink is the only discontinuity. No day is left out: such a unit adds its whole tangent to e_u
(e_d = 1 above) and its whole contribution to the backward pass's bound (_mlp_core). `near_kink` is the share of such
unit-days; every comparison asserts it is at most AMBIGUOUS_CAP, so the rule cannot swallow a failure.
`mutant` builds the CPU test's faults: "no_q" (p instead of p (1 - p)), "no_bias" (the bias components of v dropped from
u), "quad_weighted" (q_e carrying w_e), "dact_pre" (act' = 1 for the tangent: the activation's derivative left out).
No number here was fitted to a kernel's output."""
from __future__ import annotations

import numpy as np

from imitation_restatement import group_ll_bound
from policy_gradient_mlp_restatement import U, _fold
from surrogate_restatement import AMBIGUOUS_CAP, _pq  # noqa: F401  (the cap the comparisons assert)
from value_gradient_restatement import _mlp_core

PQ_SLOPE = 0.1  # >= max |p q (q - p)| = 1 / (6 sqrt 3)


def _front(valid, forced, weights, group, n_groups, G_params):
    valid = np.asarray(valid).astype(bool)
    S, N = valid.shape
    m = valid & ~np.asarray(forced).astype(bool)
    w = np.ones(N) if weights is None else np.asarray(weights, np.float64)
    G = G_params if n_groups is None else int(n_groups)
    g = np.zeros(N, np.int64) if group is None else np.asarray(group, np.int64)
    return valid, S, N, m, w, G, g


def _days(z, e_zabs, u, e_u, m, w, mutant=None):
    """c_s, its bound and the per-env quadratic form with its bound, for one block of env-days [S, n]; w [n]"""
    p, q = _pq(z)
    pq = p if mutant == "no_q" else p * q
    e_pq = PQ_SLOPE * e_zabs
    c = np.where(m, w[None, :] * pq * u, 0.0)
    cb = np.where(m, np.abs(w)[None, :] * (e_pq * np.abs(u) + pq * e_u) + 1e-15 * np.abs(c), 0.0)
    mf = m.astype(np.float64)
    quad = (mf * pq * u * u).sum(axis=0)
    if mutant == "quad_weighted":
        quad = quad * w
    quad_bound = (mf * (e_pq * u * u + pq * (2.0 * np.abs(u) * e_u + e_u * e_u) + 1e-15 * pq * u * u)).sum(axis=0) \
        + 2.0 ** -23 * np.abs(quad)
    return c, cb, quad, quad_bound


def _finish(out, w, g, G):
    gq = np.full(G, np.nan)
    for k in range(G):
        if (g == k).any():
            gq[k] = (w * out["quadratic"])[g == k].mean()
    out["group_quadratic"] = gq
    out["group_quadratic_bound"] = group_ll_bound(w, out["quadratic"], out["quadratic_bound"], g, G)
    return out


def fisher_linear_fp64(obs, labels, valid, forced, weights, W, b, vW, vb, group, n_groups=None, mutant=None):
    """obs [>= S, N, n_obs] (slab s: the row held before decision s), labels / valid / forced [S, N] (labels are not
    read: the schedule enters through the rows), weights [N] or None, W, vW [G, n_obs], b, vb [G], group int [N] or
    None. Returns dict(weight [G, n_obs], bias [G], bound [G, n_obs + 1], per_env [N, n_obs + 1], the per-day m, c, u
    [S, N], quadratic, quadratic_bound, days [N], group_quadratic(_bound) [G], near_kink = 0)."""
    del labels
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64).reshape(-1)
    vW, vb = np.asarray(vW, np.float64), np.asarray(vb, np.float64).reshape(-1)
    valid, S, N, m, w, G, g = _front(valid, forced, weights, group, n_groups, W.shape[0])
    o = np.where(valid[:, :, None], np.asarray(obs, np.float64)[:S], 0.0)
    z = np.einsum("snj,nj->sn", o, W[g]) + b[g][None, :]
    M = np.einsum("snj,nj->sn", np.abs(o), np.abs(W[g])) + np.abs(b[g])[None, :]
    vb_used = np.zeros_like(vb) if mutant == "no_bias" else vb
    u = np.einsum("snj,nj->sn", o, vW[g]) + vb_used[g][None, :]
    Mu = np.einsum("snj,nj->sn", np.abs(o), np.abs(vW[g])) + np.abs(vb[g])[None, :]
    c, cb, quad, quad_bound = _days(z, 1e-12 * (M + 1.0), u, 1e-12 * (Mu + 1.0), m, w, mutant)
    o1 = np.concatenate([o, valid[:, :, None].astype(np.float64)], axis=2)
    per_env = np.einsum("sn,snj->nj", c, o1)
    per_env_bound = np.einsum("sn,snj->nj", cb + 2.0 ** -23 * np.abs(c), np.abs(o1))
    grad, bound = np.full((G, o1.shape[2]), np.nan), np.full((G, o1.shape[2]), np.nan)
    for k in range(G):
        if (g == k).any():
            grad[k], bound[k] = per_env[g == k].mean(axis=0), per_env_bound[g == k].mean(axis=0)
    out = dict(weight=grad[:, :-1], bias=grad[:, -1], bound=bound, per_env=per_env, m=m, c=c, u=np.where(m, u, 0.0),
               quadratic=quad, quadratic_bound=quad_bound, days=m.sum(axis=0), near_kink=0.0)
    return _finish(out, w, g, G)


def mlp_tangent_fp64(layers, vector, activation, x, mutant=None):
    """One group's fp64 forward pass with its forward-mode tangent, and the bound of the f32 tangent's error.
    layers / vector: [(W [out, in], b [out]), ...] with the output already folded to one row; x [S, n, n_obs].
    Returns (z, u, e_u) [S, n]."""
    nl = len(layers) - 1
    act = np.tanh if activation == "tanh" else (lambda v: np.maximum(v, 0.0))
    h, hd = x, np.zeros_like(x)
    mag, magd = np.abs(x), np.zeros_like(x)
    e_h, e_hd = np.zeros_like(x), np.zeros_like(x)
    kacc = 0
    for i in range(nl):
        (W, b), (V, vb) = layers[i], vector[i]
        if mutant == "no_bias":
            vb = np.zeros_like(vb)
        fan_in = W.shape[1]
        pre = np.einsum("snj,uj->snu", h, W) + b
        ad = np.einsum("snj,uj->snu", hd, W) + np.einsum("snj,uj->snu", h, V) + vb
        mag_n = np.einsum("snj,uj->snu", mag, np.abs(W)) + np.abs(b)
        magd_n = np.einsum("snj,uj->snu", magd, np.abs(W)) + np.einsum("snj,uj->snu", mag, np.abs(V)) + np.abs(vb)
        Kd = (fan_in if i == 0 else 2 * fan_in) + 1
        e_ad = Kd * U * magd_n + np.einsum("snj,uj->snu", e_hd, np.abs(W)) + np.einsum("snj,uj->snu", e_h, np.abs(V))
        h_n = act(pre)
        kacc += fan_in + 1 + 2
        e_h_n = kacc * U * mag_n
        if activation == "tanh":
            d = 1.0 - h_n * h_n
            e_d = 2.0 * np.abs(h_n) * e_h_n + U
        else:
            d = (pre > 0).astype(np.float64)
            e_d = (np.abs(pre) <= 1e-5 * mag_n).astype(np.float64)
        if mutant == "dact_pre":
            d = np.ones_like(d)
        hd_n = d * ad
        e_hd = np.abs(d) * e_ad + e_d * (np.abs(ad) + e_ad) + U * np.abs(hd_n)
        h, hd, mag, magd, e_h = h_n, hd_n, mag_n, magd_n, e_h_n
    (Wo, bo), (Vo, vbo) = layers[-1], vector[-1]
    wo, vo, vbo = Wo[0], Vo[0], (0.0 if mutant == "no_bias" else vbo[0])
    z = h @ wo + bo[0]
    u = hd @ wo + h @ vo + vbo
    mu = magd @ np.abs(wo) + mag @ np.abs(vo) + abs(vbo)
    e_u = (2 * len(wo) + 3) * U * mu + e_hd @ np.abs(wo) + e_h @ np.abs(vo)
    return z, u, e_u


def fisher_mlp_fp64(obs, labels, valid, forced, weights, layers, vector, activation, group, n_groups=None, mutant=None):
    """As fisher_linear_fp64 for layers and vector [(W, b), ...] (torch Linear convention, optional leading G) and an
    activation. Returns dict(layers=[(FvW [G, out, in], Fvb [G, out]), ...], bound=[(.., ..), ...], near_kink, and the
    rest as above)."""
    del labels
    L, _ = _fold(layers)
    Lv, _ = _fold(vector)
    assert [(W.shape[1:], b.shape[1:]) for W, b in L] == [(W.shape[1:], b.shape[1:]) for W, b in Lv]
    G_params = max(W.shape[0] for W, _ in L)
    valid, S, N, m, w, G, g = _front(valid, forced, weights, group, n_groups, G_params)
    x_all = np.where(valid[:, :, None], np.asarray(obs, np.float64)[:S], 0.0)
    u_all, eu_all = np.zeros((S, N)), np.zeros((S, N))
    for k in range(G):
        sel = g == k
        if not sel.any():
            continue
        pick = lambda arr: [(W[k if W.shape[0] > 1 else 0], b[k if b.shape[0] > 1 else 0]) for W, b in arr]  # noqa: E731
        _, u_all[:, sel], eu_all[:, sel] = mlp_tangent_fp64(pick(L), pick(Lv), activation, x_all[:, sel], mutant)
    out = dict(m=m, c=np.zeros((S, N)), u=np.where(m, u_all, 0.0), quadratic=np.zeros(N), quadratic_bound=np.zeros(N),
               days=m.sum(axis=0))

    def coef(sel, z, M, e_z, eps):
        c, cb, quad, quad_bound = _days(z, e_z * M, u_all[:, sel], eu_all[:, sel], m[:, sel], w[sel], mutant)
        out["c"][:, sel], out["quadratic"][sel], out["quadratic_bound"][sel] = c, quad, quad_bound
        return c, cb + eps * np.abs(c)

    grads, bounds, near = _mlp_core(layers, activation, obs, valid, g if group is not None else None, G, coef)
    out.update(layers=grads, bound=bounds, near_kink=near)
    return _finish(out, w, g, G)
