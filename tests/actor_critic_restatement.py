"""NumPy fp64 restatement of actor_critic_gradient() (w2a_actor_critic_mlp, include/w2a.h), shared by
tests/test_actor_critic_cpu.py and tests/test_actor_critic_gpu.py, in the manner of tests/q_restatement.py. From a stepped
twin's rows (slab s: the row held before decision s, slab S the row the call leaves behind), the schedule's bit on every
day (labels), which days were stepped (valid), which ended the episode (terminal), the per-day rewards, which days were
forced (no budget left before the day under require_budget, or closed by the gate) and a weight per env:

    z_s, V_s   rows 0 and 1 of the net's output layer in fp64 on its f32 parameters (one trunk)
    m_s      = valid_s and not forced_s                                                      (the scored days)
    collect:   delta_s = r_s + gamma Vn_s - V_s,  A_s = delta_s + gamma lambda A_{s+1},  T_s = A_s + V_s,  rho_s = 1
               (tests/gae_restatement.py: gae_rows on row 1)
    epoch:     A_s, T_s and old_s are inputs; rho_s = exp(lp_s - old_s), live_s as tests/surrogate_restatement.py
    c_pi,s   = m_s w_e (live_s rho_s A_s (a_s - p_s) + beta dH_s/dz)         c_v,s = valid_s w_e vf_coef (T_s - V_s)
    g_e      = sum_s c_pi,s dz_s/dtheta + c_v,s dV_s/dtheta, per group the mean over its envs (NaN for a group without)
    L_e, kl_e, H_e, clipped_e, days_e  as surrogate_restatement;   vl_e = sum_s 1/2 (T_s - V_s)^2
    group_objective = mean_e w_e (L_e + beta H_e - vf_coef vl_e)

The gradient runs through value_gradient_restatement._mlp_core once per output row -- the one-output net made of the
hidden layers and that row, with that row's coefficient -- and the hidden layers' gradients and bounds of the two runs
add, as q_restatement does for its two heads. So the forward pass, the backward pass and every bound term of the second
pass are the ones the other restatements use.

The bounds, U = 2^-24, with the constants of those files (nothing here was fitted to a kernel's output):
    rows     |z_kernel - z| <= e_z M_z, |V_kernel - V| <= e_z M_v: each row is mlp_logit's chain (q_restatement.heads_fp64)
    collect  e_A,s and e_T,s from gae_rows (row 1, delta_s stored as f32). The policy coefficient sees A_s with that
             error: cb_pi += |w_e| rho_s (|delta_s| + e_delta) e_A,s, and L's bound += sum_s m_s e_A,s
             c_v = w_e vf A_s: cb_v = |w_e| vf e_A,s;   vl: sum_s (|A_s| e_A,s + e_A,s^2 / 2) + 2^-23 vl_e
    epoch    the three arrays are INPUTS (f32 both sides read): cb_pi is surrogate_restatement._days' as it stands;
             T_s - V_s: e_dv = e_z M_v + 1e-15 |T_s - V_s|, cb_v = |w_e| vf e_dv, vl as above with e_dv
    second   both coefficients are rounded to f32 once and enter ONE backward pass: dh_last = (c_pi w_out0 + c_v w_out1)
    pass     act' is one more f32 product-sum than the one-row pass has, 2 U of its terms' magnitudes: eps + 2 U in place
             of _mlp_core's eps on either row's coefficient. Everything after dh_last is linear in it, so the two rows'
             bounds add.
    outputs  advantage, value_target as gae_restatement; log_prob, L, kl, H, clipped, days as surrogate_restatement
    group_objective  mean_e |w_e| (L_bound + |beta| H_bound + vf vl_bound) + 2^-22 mean_e |w_e obj_e|  (the host's fp64
             mean of f32 values, rounded to f32 once)
`adv_err`, `target_err` and `old_err` (epoch only, [S, N]) widen the bound for inputs that are themselves only known to
that error: the test that feeds an epoch a collect call's own outputs compares with the collect reference this way.
A day inside the clip edge's error band is AMBIGUOUS exactly as in surrogate_restatement (its whole term joins the
bound, clipped_e gets a tolerance of 1); `ambiguous_share` and `near_kink` are held under AMBIGUOUS_CAP by every
comparison. There is no argmax here, so no near-tie rule: near_tie is 0 and reported for symmetry.
`mutant` builds the CPU test's faults: "value_on_scored_only" (the value term dropped on forced days), "no_half" (the
value coefficient doubled), "swap_rows" (row 0 read as the value)."""
from __future__ import annotations

import numpy as np

from gae_restatement import gae_rows
from policy_gradient_mlp_restatement import U
from q_restatement import _as_groups, heads_fp64
from surrogate_restatement import AMBIGUOUS_CAP, _days  # noqa: F401  (the cap the comparisons assert)
from value_gradient_restatement import _mlp_core


def ac_fp64(obs, labels, valid, forced, terminal, reward, weights, layers, activation, group, n_groups=None,
            advantage=None, value_target=None, old_log_prob=None, clip=0.2, vf_coef=0.5, beta=0.0, gamma=1.0, lam=1.0,
            bootstrap=False, adv_err=None, target_err=None, old_err=None, mutant=None):
    """obs [S + 1, N, n_obs] (slab S is read only with bootstrap), labels / valid / forced / terminal bool [S, N]
    (forced: the budget the twin held before the day was used up under require_budget, or the gate closed the day),
    reward f64 [S, N] (not read in an epoch), weights [N] or None, layers
    [(W, b), ...] (torch Linear convention, optional leading G, two output rows), group int [N] or None.
    Returns dict(layers, bound, advantage, adv_bound, value_target, vt_bound, lp, lp_bound, L, L_bound, kl, kl_bound, H,
    H_bound, vl, vl_bound, ret, ret_bound, clipped, clipped_tol, days, stepped, group_objective,
    group_objective_bound, c_pi, c_v [S, N], m, ambiguous_share, near_kink, near_tie)."""
    L = _as_groups(layers)
    if mutant == "swap_rows":
        L = L[:-1] + [(L[-1][0][:, ::-1], L[-1][1][:, ::-1])]
    valid = np.asarray(valid).astype(bool)
    S, N = valid.shape
    G = max(W.shape[0] for W, _ in L) if n_groups is None else int(n_groups)
    g = np.zeros(N, np.int64) if group is None else np.asarray(group, np.int64)
    w = np.ones(N) if weights is None else np.asarray(weights, np.float64)
    term = np.asarray(terminal).astype(bool)
    a = np.asarray(labels).astype(bool)
    m = valid & ~np.asarray(forced).astype(bool)
    epoch = advantage is not None
    assert epoch == (value_target is not None) == (old_log_prob is not None)
    x = np.asarray(obs, np.float64)
    alive_after = valid[S - 1] & ~term[S - 1]
    rows_valid = np.concatenate([valid, alive_after[None, :]], axis=0)
    if x.shape[0] == S:
        assert not bootstrap, "the bootstrap reads slab S"
        x = np.concatenate([x, np.zeros_like(x[:1])], axis=0)
    x = np.where(rows_valid[:, :, None], x[:S + 1], 0.0)
    Q, M = np.zeros((S + 1, N, 2)), np.zeros((S + 1, N, 2))
    e_z = 0.0
    for k in range(G):
        sel = g == k
        if sel.any():
            P = [(W[k if W.shape[0] > 1 else 0], b[k if b.shape[0] > 1 else 0]) for W, b in L]
            Q[:, sel], M[:, sel], e_z = heads_fp64(P, activation, x[:, sel])
    z, Mz, V, Mv = Q[:S, :, 0], M[:S, :, 0], Q[..., 1], M[..., 1]
    e_zabs = e_z * Mz
    zero = np.zeros((S, N))
    out = {}
    if epoch:
        A = np.where(valid, np.asarray(advantage, np.float64)[:S], 0.0)
        T = np.where(valid, np.asarray(value_target, np.float64)[:S], 0.0)
        old = np.asarray(old_log_prob, np.float64)[:S]
        e_A = zero if adv_err is None else np.asarray(adv_err, np.float64)[:S] * valid
        e_T = zero if target_err is None else np.asarray(target_err, np.float64)[:S] * valid
        e_old = zero if old_err is None else np.asarray(old_err, np.float64)[:S] * m
        dv = np.where(valid, T - V[:S], 0.0)
        e_dv = (e_z * Mv[:S] + 1e-15 * np.abs(dv) + e_T) * valid
    else:
        with np.errstate(invalid="ignore"):
            r = np.where(valid, np.asarray(reward, np.float64), 0.0)
        rows = gae_rows(r, np.where(rows_valid, V, 0.0), np.where(rows_valid, Mv, 0.0), valid, alive_after, gamma, lam,
                        bootstrap, e_z, True)
        A, e_A, T = rows["A"], rows["e_A"], rows["R"]
        old, e_old = None, zero
        dv, e_dv = A, e_A
        ret = r.sum(axis=0)
        out.update(advantage=A, adv_bound=(e_A + 2.0 ** -23 * np.abs(A)) * valid, value_target=T,
                   vt_bound=(rows["e_R"] + 2.0 ** -23 * np.abs(T)) * valid, ret=ret,
                   ret_bound=1e-5 * valid.sum(axis=0) + 2.0 ** -23 * np.abs(ret))
    d = _days(z, e_zabs + e_old, 1e-6 + e_zabs / 4, a, m, w, A, old, clip, beta, None)
    # the policy coefficient's view of an advantage known to e_A only
    with np.errstate(over="ignore"):
        p_delta = np.abs(a.astype(np.float64) - 1.0 / (1.0 + np.exp(-z))) + 1e-6 + e_zabs / 4
    cb_pi = d["cb"] + np.where(m, np.abs(w)[None, :] * d["rho"] * p_delta * e_A, 0.0)
    amb = d["ambiguous"]
    if epoch and adv_err is not None:  # the sign of A_s decides which edge clips: unknown inside the input's error
        lo, hi = 1.0 - clip, 1.0 + clip
        flip = m & (np.abs(A) <= e_A) & ((d["rho"] > hi) | (d["rho"] < lo))
        cb_pi = cb_pi + flip * np.abs(w[None, :] * d["rho"] * (np.abs(A) + e_A) * p_delta)
        amb = amb | flip
    c_pi = d["c"]
    on_v = m if mutant == "value_on_scored_only" else valid
    k_v = vf_coef * (2.0 if mutant == "no_half" else 1.0)
    c_v = np.where(on_v, w[None, :] * k_v * dv, 0.0)
    cb_v = np.where(valid, np.abs(w)[None, :] * vf_coef * e_dv, 0.0)
    vl = (0.5 * dv * dv * valid).sum(axis=0)
    vl_bound = ((np.abs(dv) * e_dv + 0.5 * e_dv * e_dv) * valid).sum(axis=0) + 2.0 ** -23 * vl
    L_bound = d["L_bound"] + (m * np.maximum(d["rho"], 1.0 + clip) * e_A).sum(axis=0)
    grads = bounds = None
    near = 0.0
    for head, (ck_all, cbk_all) in enumerate(((c_pi, cb_pi), (c_v, cb_v))):
        one = [(W, b) for W, b in L[:-1]] + [(L[-1][0][:, head:head + 1], L[-1][1][:, head:head + 1])]

        def coef(sel, z_, M_, e_z_, eps, ck_all=ck_all, cbk_all=cbk_all):
            ck = ck_all[:, sel]
            return ck, cbk_all[:, sel] + (eps + 2.0 * U) * np.abs(ck)

        gr, bd, near = _mlp_core(one, activation, x[:S], valid, g if group is not None else None, G, coef)
        if grads is None:
            grads, bounds = gr, bd
        else:
            cat = lambda P_, Q_: (np.concatenate([P_[0], Q_[0]], axis=1), np.concatenate([P_[1], Q_[1]], axis=1))  # noqa: E731
            grads = [(A_ + B_, a_ + b_) for (A_, a_), (B_, b_) in zip(grads[:-1], gr[:-1])] + [cat(grads[-1], gr[-1])]
            bounds = [(A_ + B_, a_ + b_) for (A_, a_), (B_, b_) in zip(bounds[:-1], bd[:-1])] + [cat(bounds[-1], bd[-1])]
    obj = w * (d["L"] + beta * d["H"] - vf_coef * vl)
    obj_b = np.abs(w) * (L_bound + abs(beta) * d["H_bound"] + vf_coef * vl_bound)
    go, gob = np.full(G, np.nan), np.full(G, np.nan)
    for k in range(G):
        if (g == k).any():
            go[k] = obj[g == k].mean()
            gob[k] = obj_b[g == k].mean() + 2.0 ** -22 * np.abs(obj)[g == k].mean()
    scored = int(m.sum())
    out.update(layers=grads, bound=bounds, lp=d["lp"], lp_bound=d["lp_bound"], L=d["L"], L_bound=L_bound, kl=d["kl"],
               kl_bound=d["kl_bound"], H=d["H"], H_bound=d["H_bound"], vl=vl, vl_bound=vl_bound, clipped=d["clipped"],
               clipped_tol=amb.sum(axis=0), days=d["days"], stepped=valid.sum(axis=0), group_objective=go,
               group_objective_bound=gob, c_pi=c_pi, c_v=c_v, m=m, rho=d["rho"], live=d["live"],
               ambiguous_share=float(amb.sum()) / scored if scored else 0.0, near_kink=near, near_tie=0.0)
    return out


def objective_torch(obs, labels, valid, m, weights, layers, activation, group, n_groups, A, T, old, clip, vf_coef, beta):
    """J_g of include/w2a.h as a torch fp64 graph over `layers` (leaf tensors [G, out, in] / [G, out]): returns the
    list of per-group objectives (None for a group without envs). A, T and old are constants; old = None is a collect
    call (rho = exp(lp - lp.detach()) = 1 with the gradient of lp)."""
    import torch

    x = torch.as_tensor(np.asarray(obs, np.float64))
    S, N = valid.shape
    g = np.zeros(N, np.int64) if group is None else np.asarray(group, np.int64)
    w = torch.as_tensor(np.ones(N) if weights is None else np.asarray(weights, np.float64))
    act = torch.tanh if activation == "tanh" else torch.relu
    out = []
    for k in range(n_groups):
        sel = np.nonzero(g == k)[0]
        if len(sel) == 0:
            out.append(None)
            continue
        h = x[:S, sel]
        for W, b in layers[:-1]:
            h = act(h @ W[k].T + b[k])
        o = h @ layers[-1][0][k].T + layers[-1][1][k]
        z, V = o[..., 0], o[..., 1]
        a = torch.as_tensor(np.asarray(labels)[:, sel].astype(np.float64))
        lp = -torch.nn.functional.softplus(torch.where(a > 0, -z, z))
        rho = torch.exp(lp - (lp.detach() if old is None else torch.as_tensor(np.asarray(old, np.float64)[:S, sel])))
        Ak = torch.as_tensor(np.asarray(A, np.float64)[:S, sel])
        Tk = torch.as_tensor(np.asarray(T, np.float64)[:S, sel])
        Lc = torch.minimum(rho * Ak, torch.clamp(rho, 1.0 - clip, 1.0 + clip) * Ak)
        H = torch.nn.functional.softplus(z) - z * torch.sigmoid(z)
        mk, vk = torch.as_tensor(m[:, sel].astype(np.float64)), torch.as_tensor(valid[:, sel].astype(np.float64))
        per_env = (mk * (Lc + beta * H) - vk * 0.5 * vf_coef * (Tk - V) ** 2).sum(dim=0)
        out.append((w[sel] * per_env).mean())
    return out
