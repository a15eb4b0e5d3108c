"""NumPy fp64 restatement of q_gradient() (w2a_q_gradient_mlp, include/w2a.h), shared by tests/test_q_gradient_cpu.py
and tests/test_q_gradient_gpu.py, in the manner of tests/value_gradient_restatement.py. From a stepped twin's rows (slab
s: the row held before decision s, slab S the row the call leaves behind), the alerts ISSUED, the per-day rewards, which
days were stepped (valid), which ended the episode (terminal), the budget left after every day and a weight per env:

    Q(o, a), Qt(o, a)   the two output rows of the online and the target net in fp64 on their f32 parameters
    N_s      = 0 where the env holds no row after day s that enters (terminal day; the call's last day unless bootstrap)
               else max_a' Qt(o_{s+1}, a'), or (double) Qt(o_{s+1}, a*), a* = 1 iff Q(o_{s+1}, 1) > Q(o_{s+1}, 0);
               with require_budget the choice is a' = 0 where no budget is left after day s
    y_s      = r_s + gamma N_s,   delta_s = y_s - Q(o_s, a_s),   c_s = delta_s or clamp(delta_s, +-huber_delta)
    g_e      = w_e sum_s c_s dQ(o_s, a_s)/dtheta,  per group the mean over its envs (NaN for a group without envs)
    loss_e   = sum_s l(delta_s),  l = delta^2 / 2, or Huber's (delta^2 / 2 inside, hd (|delta| - hd / 2) outside)
    ret_e    = sum_s r_s,   group_loss = mean_e w_e loss_e

The gradient runs through value_gradient_restatement._mlp_core once per head: the one-output net made of the hidden
layers and output row a, with the coefficient w_e c_s on the days where a_s = a and 0 elsewhere. The hidden layers'
gradients and bounds of the two runs add; the output layer's rows sit side by side. So the forward pass, the backward
pass and every bound term of the second pass are the ones the other restatements use.

The bounds, U = 2^-24, with the constants of those files (nothing here was fitted to a kernel's output):
    heads    |Q_kernel - Q| <= e_z M_a, M_a = |b_out,a| + |w_out,a| . m_last and e_z = U (K1 + K2 + K_out + 2 L) as
             policy_gradient_mlp_restatement.py derives them: each head is mlp_logit's chain for its own row
    N_s      max is 1-Lipschitz in each argument: e_N = max(e_t0, e_t1) (masked: e_t0). Double: e_N = e_t,a* when
             the online choice is clear; when |Q(., 1) - Q(., 0)| <= e_o0 + e_o1 the kernel may take either row:
             e_N = |Qt(., 1) - Qt(., 0)| + max(e_t0, e_t1)  -- the bound is WIDENED, the day stays in
    y_s      e_y = 1e-5 (the project's reward bar) + gamma e_N;   delta_s: e_d = e_y + e_z M_{a_s}(o_s)
    c_s      the clamp is 1-Lipschitz: e_c = e_d, also where |delta_s| is within e_d of huber_delta (c is continuous
             there; such days are counted in near_tie all the same); fp64 arithmetic on top: 1e-15 relative
    theta    mean_e sum_s ( |dQ/dtheta|_abs (|w_e| e_c + eps |w_e c_s|) + |w_e c_s| (|dQ/dtheta|_abs,err - |..|_abs) )
             exactly as _mlp_core lays it out (w_e c_s rounded to f32 once, the f32 backward pass, the f32 sums over a
             tile's days, the near-kink ReLU rule, which widens by the unit's whole contribution)
    td_error e_d + 2^-23 |delta_s|;   td_target  e_y + 2^-23 |y_s|                  (one rounding to f32)
    loss     sum_s (|c_s| + e_d) e_d + 2^-23 loss_e          (l' = c)
    ret      1e-5 days_e + 2^-23 |ret_e|;   group_loss as value_gradient_restatement._group_loss without the 1/2
`near_tie` is the share of stepped days whose next-row choice (max or argmax) lies inside the forward error bound or
whose |delta_s| is within e_d of huber_delta; `near_kink` the share of ReLU unit-days within the kink rule. No case is
dropped; every comparison asserts near_tie + near_kink <= AMBIGUOUS_CAP, so the widening cannot swallow a failure.
`mutant` builds the CPU test's faults: "attempted" (the head of the schedule's bit, not of the alert issued -- pass
`attempted`), "no_mask" (require_budget ignored), "online_target" (the online net valued as its own target)."""
from __future__ import annotations

import numpy as np

from policy_gradient_mlp_restatement import U
from surrogate_restatement import AMBIGUOUS_CAP  # noqa: F401  (the cap the comparisons assert)
from value_gradient_restatement import _mlp_core


def _as_groups(layers):
    """fp64 layers with a leading G"""
    out = []
    for W, b in layers:
        W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
        out.append((W[None] if W.ndim == 2 else W, b[None] if b.ndim == 1 else b))
    assert out[-1][0].shape[1] == 2, "a Q-net has two output rows"
    return out


def heads_fp64(P, activation, x):
    """One group's fp64 forward pass: P [(W [out, in], b [out]), ...] with a two-row output, x [R, n, n_obs].
    Returns (Q [R, n, 2], M [R, n, 2] the magnitudes |b_out,a| + |w_out,a| . m_last, e_z)."""
    act = np.tanh if activation == "tanh" else (lambda v: np.maximum(v, 0.0))
    h, mag = x, np.abs(x)
    for W, b in P[:-1]:
        h, mag = act(np.einsum("snj,uj->snu", h, W) + b), np.einsum("snj,uj->snu", mag, np.abs(W)) + np.abs(b)
    Wo, bo = P[-1]
    nl = len(P) - 1
    K = [P[i][0].shape[1] + 1 for i in range(nl)] + [Wo.shape[1] + 3]
    return h @ Wo.T + bo, mag @ np.abs(Wo).T + np.abs(bo), U * (sum(K) + 2 * nl)


def q_fp64(obs, issued, valid, terminal, reward, left_after, weights, layers, target_layers, activation, group,
           n_groups=None, gamma=0.99, double=False, loss="huber", huber_delta=1.0, bootstrap=False, require_budget=False,
           mutant=None, attempted=None):
    """obs [S + 1, N, n_obs] (slab S is read only with bootstrap), issued / valid / terminal bool [S, N], reward f64
    [S, N], left_after int [S, N] (budget - used after day s), weights [N] or None, layers / target_layers [(W, b), ...]
    (torch Linear convention, optional leading G, two output rows; target_layers None = the online net), group int [N] or
    None. Returns dict(layers=[(dW [G, out, in], db [G, out]), ...], bound=[...], loss, loss_bound, ret, ret_bound, days
    [N], group_loss, group_loss_bound [G], td_error, td_error_bound, td_target, td_target_bound, c [S, N], masked,
    has_next [S, N] bool, near_tie, near_kink)."""
    L = _as_groups(layers)
    Lt = L if target_layers is None or mutant == "online_target" else _as_groups(target_layers)
    valid = np.asarray(valid).astype(bool)
    S, N = valid.shape
    G = max(W.shape[0] for W, _ in L) if n_groups is None else int(n_groups)
    g = np.zeros(N, np.int64) if group is None else np.asarray(group, np.int64)
    w = np.ones(N) if weights is None else np.asarray(weights, np.float64)
    a = np.asarray(attempted if mutant == "attempted" else issued).astype(bool) & valid
    term = np.asarray(terminal).astype(bool)
    with np.errstate(invalid="ignore"):
        r = np.where(valid, np.asarray(reward, np.float64), 0.0)
    x = np.asarray(obs, np.float64)
    rows_valid = np.concatenate([valid, (valid[-1:] & ~term[-1:])], axis=0)  # slab s + 1 holds a row the env was given
    if x.shape[0] == S:
        assert not bootstrap, "the bootstrap reads slab S"
        x = np.concatenate([x, np.zeros_like(x[:1])], axis=0)
    x = np.where(rows_valid[:, :, None], x[:S + 1], 0.0)
    last = np.zeros((S, 1), bool)
    last[S - 1] = True
    has_next = valid & ~term & (~last | bool(bootstrap))
    masked = has_next & bool(require_budget and mutant != "no_mask") & (np.asarray(left_after) <= 0)
    Qo, Mo, Qt, Mt = (np.zeros((S + 1, N, 2)) for _ in range(4))
    e_z = 0.0
    for k in range(G):
        sel = g == k
        if not sel.any():
            continue
        pick = lambda arr: [(W[k if W.shape[0] > 1 else 0], b[k if b.shape[0] > 1 else 0]) for W, b in arr]  # noqa: E731
        Qo[:, sel], Mo[:, sel], e_z = heads_fp64(pick(L), activation, x[:, sel])
        Qt[:, sel], Mt[:, sel], _ = (Qo[:, sel], Mo[:, sel], 0) if Lt is L else heads_fp64(pick(Lt), activation, x[:, sel])
    on, tn, e_on, e_tn = Qo[1:], Qt[1:], e_z * Mo[1:], e_z * Mt[1:]
    e_tmax = np.maximum(e_tn[..., 0], e_tn[..., 1])
    gap_o, gap_t = on[..., 1] - on[..., 0], tn[..., 1] - tn[..., 0]
    if double:
        pick1 = gap_o > 0
        tie = np.abs(gap_o) <= e_on[..., 0] + e_on[..., 1]
        Nv = np.where(pick1, tn[..., 1], tn[..., 0])
        eN = np.where(tie, np.abs(gap_t) + e_tmax, np.where(pick1, e_tn[..., 1], e_tn[..., 0]))
    else:
        tie = np.abs(gap_t) <= e_tn[..., 0] + e_tn[..., 1]
        Nv, eN = np.maximum(tn[..., 0], tn[..., 1]), e_tmax
    Nv, eN, tie = np.where(masked, tn[..., 0], Nv), np.where(masked, e_tn[..., 0], eN), tie & ~masked
    Nv, eN, tie = np.where(has_next, Nv, 0.0), np.where(has_next, eN, 0.0), tie & has_next
    y = np.where(valid, r + gamma * Nv, 0.0)
    e_y = np.where(valid, 1e-5 + gamma * eN, 0.0)
    qsa = np.where(a, Qo[:S, :, 1], Qo[:S, :, 0])
    delta = np.where(valid, y - qsa, 0.0)
    e_d = np.where(valid, e_y + e_z * np.where(a, Mo[:S, :, 1], Mo[:S, :, 0]), 0.0)
    if loss == "huber":
        c = np.clip(delta, -huber_delta, huber_delta)
        l = np.where(np.abs(delta) <= huber_delta, 0.5 * delta * delta, huber_delta * (np.abs(delta) - 0.5 * huber_delta))
        near_hd = valid & (np.abs(np.abs(delta) - huber_delta) <= e_d)
    else:
        c, l, near_hd = delta, 0.5 * delta * delta, np.zeros_like(valid)
    e_c = e_d + 1e-15 * np.abs(c)
    wc, wcb = w[None, :] * c, np.abs(w)[None, :] * e_c
    grads = bounds = None
    near = 0.0
    for head in (0, 1):
        on_head = valid & (a == bool(head))
        one = [(W, b) for W, b in L[:-1]] + [(L[-1][0][:, head:head + 1], L[-1][1][:, head:head + 1])]

        def coef(sel, z, M, e_z_, eps, on_head=on_head):
            ck = np.where(on_head[:, sel], wc[:, sel], 0.0)
            return ck, np.where(on_head[:, sel], wcb[:, sel], 0.0) + eps * np.abs(ck)

        gr, bd, near = _mlp_core(one, activation, x[:S], valid, g if group is not None else None, G, coef)
        if grads is None:
            grads, bounds = gr, bd
        else:
            grads = [(A + B, a_ + b_) for (A, a_), (B, b_) in zip(grads[:-1], gr[:-1])] + \
                [(np.concatenate([grads[-1][0], gr[-1][0]], axis=1), np.concatenate([grads[-1][1], gr[-1][1]], axis=1))]
            bounds = [(A + B, a_ + b_) for (A, a_), (B, b_) in zip(bounds[:-1], bd[:-1])] + \
                [(np.concatenate([bounds[-1][0], bd[-1][0]], axis=1), np.concatenate([bounds[-1][1], bd[-1][1]], axis=1))]
    loss_e = l.sum(axis=0)
    loss_bound = ((np.abs(c) + e_d) * e_d).sum(axis=0) + 2.0 ** -23 * loss_e
    ret = r.sum(axis=0)
    days = valid.sum(axis=0)
    gl, glb = np.full(G, np.nan), np.full(G, np.nan)
    for k in range(G):
        if (g == k).any():
            gl[k] = (w * loss_e)[g == k].mean()
            glb[k] = (np.abs(w) * loss_bound)[g == k].mean() + 2.0 ** -22 * np.abs(w * loss_e)[g == k].mean()
    n_days = max(int(valid.sum()), 1)
    return dict(layers=grads, bound=bounds, loss=loss_e, loss_bound=loss_bound, ret=ret,
                ret_bound=1e-5 * days + 2.0 ** -23 * np.abs(ret), days=days, group_loss=gl, group_loss_bound=glb,
                td_error=delta, td_error_bound=(e_d + 2.0 ** -23 * np.abs(delta)) * valid, td_target=y,
                td_target_bound=(e_y + 2.0 ** -23 * np.abs(y)) * valid, c=np.where(valid, c, 0.0), masked=masked,
                has_next=has_next, near_tie=float((tie | near_hd).sum()) / n_days, near_kink=near)
