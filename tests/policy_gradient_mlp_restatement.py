"""NumPy fp64 restatement of rollout(mlp, policy_gradient=...) (w2a_policy_gradient_mlp, include/w2a.h), shared by
tests/test_policy_gradient_mlp_cpu.py and tests/test_policy_gradient_mlp_gpu.py. Inputs as policy_gradient_fp64
(tests/policy_gradient_restatement.py) takes them -- the rows held before every decision, the policy's draws, the
forced days, the per-day rewards and no-alert rewards -- plus the layers and the activation. Per env e of group g

    g_e = sum_s delta_s Q_s dz_s/dtheta,  delta_s = m_s (a_s - sigmoid(z_s)),  Q_s = sum_{s' >= s, valid} (r_s' - beta_s'),

z_s the network's logit in fp64 on the f32 parameters (a two-row output folded into row1 - row0 and rounded to f32 once,
as the host does; its gradient goes back as +g on row 1 and -g on row 0), dz/dtheta the manual backward pass (ReLU' = 0
at a pre-activation of exactly 0), everything as einsums over [S, N]; per group the mean over its envs.

The bound, of the linear bar's form:

    bound_theta = mean_e sum_s |dz_s/dtheta|_abs (|delta_s| 2e-5 (valid days from s on) + eps_s |Q_s|)

|dz/dtheta|_abs is the backward pass with absolute values throughout (|w|, |x|, |h|, |act'|): outer products, so no
per-sample parameter array is formed. 2e-5 per advantage is the reward bar (1e-5 per reward and day, twice).

eps_s, from the numerics DESIGN.md documents for k_rollout_mlp (u = 2^-24; nothing here was fitted to a kernel's output):
  * every pre-activation is a k-ordered f32 fmaf chain, bias first: a chain of K terms is within K u (|b| + sum |w x|)
    of the exact sum. tanhf is within 2 ulp (<= 2 u |h|), ReLU is exact, both are 1-Lipschitz, |act(v)| <= |v|. So with
    the magnitudes m1 = |b1| + |W1| |x|, m2 = |b2| + |W2| m1, M_s = |b_out| + |w_out| . m_last, the f32 logit is within
    e_z M_s of the fp64 one, e_z = u (K1 + K2 + K_out + 2 L), K = fan-in + 1 (K_out + 2 for the two adds across lanes).
  * delta: the f32 sigmoid is within ~1e-7 of fp64, taken x 10 as in the linear bar (1e-6); sigmoid' <= 1/4, so
    |delta - delta_64| <= 1e-6 + e_z M_s / 4.
  * the backward pass multiplies f32 factors (c = delta Q rounded once, w_out, act', a chain over <= 64 units per layer
    through W2): (K2 + 8) u relative.
  * every weight-gradient element is summed in f32 over the env-days of one 64-env tile (the f32 matrix-core instruction
    is a k-ordered fmaf chain, 4 envs per instruction: 16 instructions per day and tile, one chain of <= 64 S terms, S
    the call's days) before the tiles are added in fp64. The term allowed for it is 16 S u relative to the sum of the
    terms' magnitudes: one u per instruction. That is NOT the deterministic worst case of a sequential sum (64 S u, every
    rounding in the same direction); round-to-nearest errors of a chain of n terms grow like sqrt(n), and
    tests/test_policy_gradient_mlp_cpu.py::test_f32_chain_emulation replays the kernel's exact order on the CPU (numpy
    f32 fmaf per env, days of a tile, fp64 across tiles) and asserts the measured error under a tenth of this term.
  Together eps_s = 1e-6 + u (K1 + K2 + K_out + 2 L) M_s / 4 + u (K2 + 8 + 16 S).
Errors of dz/dtheta that are NOT relative to it get a second term, weighted by the full |c_s| = |delta_s Q_s|:
  * an f32 activation of layer i is off by <= e_h = u (sum of K_j + 2 over the layers up to i) m_i (its chain, tanhf's
    2 ulp, and the same carried in from the layer before), however small |h| is;
  * tanh' = 1 - h^2 is formed from that h: off by <= 2 |h| e_h, however small tanh' is (a saturated unit).
  The term is the absolute backward pass with |h| + e_h and |act'| + 2 |h| e_h minus the same pass with |h| and |act'|:
  everything that holds at least one of these errors.
    bound_theta = mean_e sum_s ( |dz_s/dtheta|_abs (|delta_s| 2e-5 days + eps_s |Q_s|) + |c_s| (|dz_s/dtheta|_abs,err - |dz_s/dtheta|_abs) )
ReLU: a unit whose fp64 pre-activation lies within 1e-5 (|b| + sum |w x|) of zero may take the other branch in f32; its
whole absolute contribution is added to the bound (|act'| + 1 in the second term's pass, times |c_s|). No case is
excluded; `near_kink` reports the fraction of such unit-days."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24


def _fold(layers):
    """fp64 layers with a leading G: hidden layers as given, the output folded to one row (rounded to f32 once)"""
    L = []
    for W, b in layers:
        W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
        L.append((W[None] if W.ndim == 2 else W, b[None] if b.ndim == 1 else b))
    Wo, bo = L[-1]
    n_out = Wo.shape[1]
    if n_out == 2:
        Wo, bo = Wo[:, 1:] - Wo[:, :1], bo[:, 1:] - bo[:, :1]
    L[-1] = (Wo.astype(np.float32).astype(np.float64), bo.astype(np.float32).astype(np.float64))
    return L, n_out


def policy_gradient_mlp_fp64(obs, action, valid, forced, reward, baseline_reward, layers, activation, group,
                             n_groups=None, q_shift=0, drop_act2=False, w2_untransposed=False):
    """obs [>= S, N, n_obs], action / valid / forced / reward [S, N], baseline_reward [S, N] or None, layers [(W, b), ...]
    (torch Linear convention, optional leading G), group int [N] or None. The three last keywords build the perturbed
    gradients of the CPU test (Q shifted by a day, act' of the second layer omitted, W2 untransposed in the backward).
    Returns dict(layers=[(dW [G, out, in], db [G, out]), ...], bound=[(.., ..), ...], bound_second (the part of bound that
    is its second term), near_kink=fraction, delta, Q)."""
    L, n_out = _fold(layers)
    nl = len(L) - 1
    action, valid = np.asarray(action).astype(np.float64), np.asarray(valid).astype(bool)
    S, N = valid.shape
    G = max(W.shape[0] for W, _ in L) if n_groups is None else int(n_groups)
    g = np.zeros(N, np.int64) if group is None else np.asarray(group, np.int64)
    x_all = np.where(valid[:, :, None], np.asarray(obs, np.float64)[:S], 0.0)
    with np.errstate(invalid="ignore"):
        A = np.asarray(reward, np.float64) - (0.0 if baseline_reward is None else np.asarray(baseline_reward, np.float64))
    A = np.where(valid, A, 0.0)
    Q = np.cumsum(A[::-1], axis=0)[::-1]
    if q_shift:
        Q = Q + np.concatenate([np.zeros((1, N)), A[:-1]], axis=0) * valid  # includes the day before
    days_left = np.cumsum(valid[::-1].astype(np.float64), axis=0)[::-1]
    m = valid & ~np.asarray(forced).astype(bool)
    act = np.tanh if activation == "tanh" else (lambda v: np.maximum(v, 0.0))
    dact = (lambda h, pre: 1.0 - h * h) if activation == "tanh" else (lambda h, pre: (pre > 0).astype(np.float64))
    grads = [(np.full((G,) + W.shape[1:], np.nan), np.full((G,) + b.shape[1:], np.nan)) for W, b in L]
    bounds = [(np.full((G,) + W.shape[1:], np.nan), np.full((G,) + b.shape[1:], np.nan)) for W, b in L]
    second = [(np.zeros((G,) + W.shape[1:]), np.zeros((G,) + b.shape[1:])) for W, b in L]  # the bound's second term
    delta_all = np.zeros((S, N))
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
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-z))
        delta = np.where(m[:, sel], action[:, sel] - p, 0.0)
        delta_all[:, sel] = delta
        c = delta * Q[:, sel]
        K = [P[i][0].shape[1] + 1 for i in range(nl)] + [len(wo) + 3]
        e_z = U * (sum(K) + 2 * nl)
        eps = 1e-6 + e_z * M / 4 + U * ((K[1] if nl == 2 else 0) + 8 + 16 * S)
        cb = (np.abs(delta) * 2e-5 * days_left[:, sel] + eps * np.abs(Q[:, sel])) * vk
        # errors of dz/dtheta that are not relative to it: the f32 activations (chain and tanhf's 2 ulp, carried
        # through the layers), tanh' formed from them, and the whole unit for a ReLU near its kink
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

        # relative part (the formula above) + |c| times what the absolute errors add to |dz/dtheta|_abs
        rel = absolute(cb, da_plain, h_abs)
        hi_, lo_ = absolute(np.abs(c) * vk, da_err, h_err), absolute(np.abs(c) * vk, da_plain, h_abs)
        for i in range(nl + 1):
            bW, bb = rel[i][0] + (hi_[i][0] - lo_[i][0]), rel[i][1] + (hi_[i][1] - lo_[i][1])
            if i == nl:
                bounds[i][0][k, 0], bounds[i][1][k, 0] = bW, bb
                second[i][0][k, 0], second[i][1][k, 0] = hi_[i][0] - lo_[i][0], hi_[i][1] - lo_[i][1]
            else:
                bounds[i][0][k], bounds[i][1][k] = bW, bb
                second[i][0][k], second[i][1][k] = hi_[i][0] - lo_[i][0], hi_[i][1] - lo_[i][1]
        # backward: dz/dh_last = w_out
        dh = c[:, :, None] * wo[None, None, :] * (1.0 if (drop_act2 and nl == 2) else da[-1])
        grads[-1][0][k, 0], grads[-1][1][k, 0] = np.einsum("sn,snu->u", c, hs[-1]) / n_k, c.sum() / n_k
        for i in range(nl - 1, -1, -1):
            grads[i][0][k] = np.einsum("snu,snj->uj", dh, hs[i]) / n_k
            grads[i][1][k] = dh.sum(axis=(0, 1)) / n_k
            if i > 0:
                W = P[i][0]  # [out u, in j]: dh_in[j] = sum_u W[u, j] dh[u]
                dh = np.einsum("snu,ju->snj" if w2_untransposed else "snu,uj->snj", dh, W) * da[i - 1]
    if n_out == 2:  # the adjoint of the fold: +g on row 1, -g on row 0
        for arr, sign in ((grads, -1.0), (bounds, 1.0), (second, 1.0)):
            W, b = arr[-1]
            arr[-1] = (np.concatenate([sign * W, W], axis=1), np.concatenate([sign * b, b], axis=1))
    return dict(layers=grads, bound=bounds, bound_second=second, near_kink=(kink_n / kink_d if kink_d else 0.0), delta=delta_all, Q=Q)
