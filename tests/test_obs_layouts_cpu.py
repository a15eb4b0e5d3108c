"""The observation layouts of tests/obs_layouts.py without a GPU: the table compiler puts every column on the slot
tables._assign_slots specifies (written out by hand below), the name-driven oracle's rows are the gather of the
slot-driven tables' row model, the host helpers that move parameters and gradients between the two orders
(policy.slot_map, to_slot_order, pack_mlp, unpack_mlp_grad) are right on every layout, the fp64 restatements the GPU
file holds the gradient kernels to are the autograd gradients on rows of 5, 8, 28 and 29 columns, and the references
alone stay inside the near-tie cap the GPU file asserts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import obs_layouts as L  # noqa: E402
import table_edges as E  # noqa: E402
from imitation_restatement import imitation_linear_fp64, imitation_mlp_fp64  # noqa: E402
from policy_gradient_mlp_restatement import policy_gradient_mlp_fp64  # noqa: E402
from policy_gradient_restatement import policy_gradient_fp64  # noqa: E402

from weather2alert_amd import policy  # noqa: E402

# weighted table columns first in column order, then the unweighted ones, run-time columns on 24 / 25 / 26, the 25th
# table column on 28, `alert_2wks` last on 27
OBS_SLOT = {
    # columns 1 and 5 and the two last table columns (significance, issued_in_advance) carry no coefficient
    "permuted": [0, 21, 1, 2, 3, 22, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 23, 28, 26, 25, 24, 19, 20, 27],
    # column 2 and significance carry none; 24 table columns: slot 28 stays empty
    "n28": [0, 1, 22, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 24, 25, 26, 21, 23, 27],
    "n8": [3, 0, 1, 24, 2, 25, 26, 27],
    "narrow": [0, 26, 25, 24, 27],
}
MLP_NETS = {"tanh7x13": ((7, 13), "tanh", 1), "relu33": ((33,), "relu", 1), "tanh64_o2": ((64,), "tanh", 2)}


@pytest.fixture(scope="module")
def tabs():
    return L.make_layouts()


@pytest.fixture(scope="module")
def recorded(tabs):
    """layout -> the oracle's recorded episode of 70 envs under the sampled linear policy, G = 5 interleaved groups, and
    the rewards of the same envs stepped with no alerts (computed once, shared, left unchanged)"""
    out = {}
    for name in L.LAYOUTS:
        tb, n = tabs[name], L.N_SMALL
        ct, tup, g = tb.ct, L.host_tuples(tb, n), E.groups(n)
        V = tb.oracle()
        E.oracle_reset(V, tup)
        beta = np.zeros((ct.T, n))
        for s in range(ct.T):
            r, _, _, live = E.oracle_step(V, np.zeros(n, np.int64))
            beta[s] = np.where(live, r, 0.0)
        pol, fn, ties = L.make_policy(tb, "linear_sampled", g)
        E.oracle_reset(V, tup)
        R = E.oracle_record(V, fn, ct.T, ties, uniform=L.policy_uniform(tb, n))
        assert R["alert"].any() and (R["action"] == 0).any()
        out[name] = dict(R=R, beta=beta, g=g, ct=ct, pol=pol)
    return out


# ------------------------------------------------------------------ the table compiler
@pytest.mark.parametrize("name", L.LAYOUTS)
def test_compiler_puts_every_column_on_its_slot(tabs, name):
    tb = tabs[name]
    ct, sd = tb.ct, tb.sd
    assert ct.n_obs == L.N_OBS[name] == len(OBS_SLOT[name])
    assert list(ct.obs_slot) == OBS_SLOT[name]
    assert ct.feature_names[-1] == "alert_2wks" and ct.slot_of["heat_qi"] == OBS_SLOT[name][ct.columns.index("heat_qi")]
    Xv = ct.X.reshape(ct.T, ct.S_w, ct.Y, 32)
    exo, endo = sd.meta["exo_cols"], sd.meta["endo_cols"]
    assert ct.columns == list(exo) + list(endo)
    for j, c in enumerate(ct.columns):
        if c in ("alert_lag1", "alert_streak", "remaining_budget"):
            continue
        src = sd.exo[..., j] if j < len(exo) else np.asarray(getattr(sd, c), np.float32)
        np.testing.assert_array_equal(Xv[..., ct.slot_of[c]], np.moveaxis(src, 2, 0), err_msg=c)
    used = set(OBS_SLOT[name]) | {29, 30}
    for s in set(range(32)) - used:
        assert not Xv[..., s].any(), s
    if name.startswith("permuted"):
        assert sum(s != c for c, s in enumerate(OBS_SLOT[name][:23])) > 15
    assert tabs["permuted_ragged"].ct.obs_slot == OBS_SLOT["permuted"] and tabs["n8_ragged"].ct.obs_slot == OBS_SLOT["n8"]


@pytest.mark.parametrize("name", L.LAYOUTS + L.RAGGED)
def test_oracle_rows_are_the_gather_of_the_row_model(tabs, name):
    """after reset and after each of three steps: the oracle's observation (columns by name) equals the 32-slot row
    X[day] with slots 24..27 patched from the oracle's integer state, read through obs_slot"""
    tb, n = tabs[name], L.N_SMALL
    ct, tup = tb.ct, L.host_tuples(tb, n)
    V = tb.oracle()
    E.oracle_reset(V, tup)
    rows = tup["county_w"] * ct.Y + tup["year_i"]
    slot = np.asarray(ct.obs_slot)

    def model(t, lag, streak):
        r = ct.X[t, rows].astype(np.float64)
        r[:, 24], r[:, 25], r[:, 26], r[:, 27] = lag, streak, V.budget - V.used, V.hist.sum(axis=1)
        return r[:, slot]

    np.testing.assert_array_equal(V.obs, model(V.t, 0, 0))
    rng = np.random.default_rng(2)
    for _ in range(3):
        live = ~V._finished
        t0, streak0 = V.t.copy(), V.streak.copy()
        keep = V.obs.copy()
        _, done, actual, _ = E.oracle_step(V, (rng.random(n) < 0.5).astype(np.int64))
        # the row a step returns: the table row of the day just played with the counters after the action and the
        # streak before it (the reference's observation); a terminal step and a finished env keep the row they had
        moved = live & ~done
        want = model(t0, np.where(t0 > 0, actual, 0), streak0)
        np.testing.assert_array_equal(V.obs[moved], want[moved])
        np.testing.assert_array_equal(V.obs[~moved], keep[~moved])
    assert moved.any() and (name in L.LAYOUTS or (~moved).any())


# ------------------------------------------------------------------ the host helpers
def _forward32(P, w, nl, act, x32, g):
    """fp64 forward pass of the packed f32 blocks (w2a.h: w2a_mlp_policy) on 32-slot rows"""
    P = P.double().numpy()
    f = np.tanh if act == "tanh" else (lambda v: np.maximum(v, 0.0))
    z = np.empty(len(x32))
    for k in range(P.shape[0]):
        p, off = P[k], 0
        W1 = p[off:off + 32 * w].reshape(32, w); off += 32 * w  # noqa: E702
        b1 = p[off:off + w]; off += w  # noqa: E702
        h = f(x32[g == k] @ W1 + b1)
        if nl == 2:
            W2 = p[off:off + w * w].reshape(w, w); off += w * w  # noqa: E702
            b2 = p[off:off + w]; off += w  # noqa: E702
            h = f(h @ W2 + b2)
        z[g == k] = h @ p[off:off + w] + p[off + w]
    return z


@pytest.mark.parametrize("name", L.LAYOUTS)
def test_parameters_in_slot_order_give_the_same_logit(recorded, name):
    c = recorded[name]
    ct, g = c["ct"], c["g"]
    obs = c["R"]["obs"][:4].reshape(-1, ct.n_obs).astype(np.float64)
    gg = np.tile(g, 4)
    x32 = L.row32(ct, obs)
    s = policy.slot_map(ct.obs_slot, ct.n_obs)
    assert s.tolist() == OBS_SLOT[name]
    W, _ = E.linear_params(ct)
    Ws = policy.to_slot_order(torch.as_tensor(W), ct.obs_slot, ct.n_obs)
    assert Ws.shape == (E.G, 32) and Ws.dtype == torch.float32
    Ws = Ws.double().numpy()
    np.testing.assert_allclose((x32 * Ws[gg]).sum(1), (obs * W.astype(np.float64)[gg]).sum(1), rtol=1e-12, atol=1e-12)
    for j in range(ct.n_obs):  # column by column: exactly the values, nothing else anywhere
        np.testing.assert_array_equal(Ws[:, OBS_SLOT[name][j]], W[:, j].astype(np.float64))
    assert not Ws[:, sorted(set(range(32)) - set(OBS_SLOT[name]))].any()
    # a matrix whose column j is the constant j: a transposed or inverse permutation cannot hide behind random values
    const = np.tile(np.arange(ct.n_obs, dtype=np.float32), (2, 1))
    Cs = policy.to_slot_order(torch.as_tensor(const), ct.obs_slot, ct.n_obs).numpy()
    for j in range(ct.n_obs):
        assert (Cs[:, OBS_SLOT[name][j]] == j).all()
    for net, (hidden, act, n_out) in MLP_NETS.items():
        layers = E.net(ct, hidden, n_out, seed=5)
        P, w, nl, G = policy.pack_mlp(layers, ct.obs_slot, ct.n_obs)
        assert (w, nl, G) == (policy.mlp_width(hidden), len(hidden), E.G)
        z, _ = E.mlp64(layers, act, obs.astype(np.float32), gg)
        np.testing.assert_allclose(_forward32(P, w, nl, act, x32, gg), z, rtol=1e-12, atol=1e-12, err_msg=net)


@pytest.mark.parametrize("name", L.LAYOUTS)
def test_unpack_mlp_grad_inverts_pack_mlp_on_the_first_layer(tabs, name):
    ct = tabs[name].ct
    for net, (hidden, act, n_out) in MLP_NETS.items():
        layers = E.net(ct, hidden, n_out, seed=6)
        h0 = hidden[0]
        const = np.broadcast_to(np.arange(ct.n_obs, dtype=np.float32), (E.G, h0, ct.n_obs)).copy()
        ones = np.ones((E.G, h0, ct.n_obs), np.float32)
        for W1 in (layers[0][0], const, ones):
            P, w, nl, _ = policy.pack_mlp([(W1, layers[0][1])] + layers[1:], ct.obs_slot, ct.n_obs)
            back = policy.unpack_mlp_grad(P, ct.obs_slot, ct.n_obs, hidden, n_out)
            assert back[0][0].shape == (E.G, h0, ct.n_obs)
            for j in range(ct.n_obs):
                np.testing.assert_array_equal(back[0][0][:, :, j].numpy(), W1[:, :, j], err_msg=f"{net} column {j}")
            np.testing.assert_array_equal(back[0][1].numpy(), layers[0][1])
            blk = P[:, :32 * w].reshape(E.G, 32, w).numpy()
            for j in range(ct.n_obs):  # the packed block holds column j on the slot written out above
                np.testing.assert_array_equal(blk[:, OBS_SLOT[name][j], :h0], W1[:, :, j])
        # ones: a zero in the unpacked first layer would be a slot the gather missed
        assert (back[0][0] == 1).all()
        # the adjoint: a block that is 1 on one slot unpacks to 1 on that slot's column alone
        for j in (0, ct.n_obs // 2, ct.n_obs - 1):
            Pz = torch.zeros_like(P)
            Pz[:, :32 * w].view(E.G, 32, w)[:, OBS_SLOT[name][j], :] = 1.0
            dW = policy.unpack_mlp_grad(Pz, ct.obs_slot, ct.n_obs, hidden, n_out)[0][0]
            assert (dW[:, :, j] == 1).all() and dW.sum() == E.G * h0


# ------------------------------------------------------------------ the restatements against autograd
def _surrogate_grad(c, layers, act, coef, m, cnt_w):
    """torch fp64 autograd of sum_e sum_s coef[s, e] m[s, e] log pi(a_s | o_s) / N_g for a linear policy (layers =
    [(W [G, 1, n_obs], b [G, 1])], act None) or a net: [(dW, db), ...]"""
    R, g = c["R"], c["g"]
    valid = R["valid"]
    S = valid.shape[0]
    P = [(torch.tensor(np.asarray(W, np.float64), requires_grad=True), torch.tensor(np.asarray(b, np.float64), requires_grad=True))
         for W, b in layers]
    gt = torch.as_tensor(g)
    h = torch.as_tensor(np.where(valid[:, :, None], R["obs"][:S].astype(np.float64), 0.0))
    f = torch.tanh if act == "tanh" else torch.relu
    for W, b in P[:-1]:
        h = f(torch.einsum("snj,nuj->snu", h, W[gt]) + b[gt][None])
    Wo, bo = P[-1]
    if Wo.shape[1] == 2:  # the host's fold, rounded to f32 once (straight-through for the gradient)
        wo, b0 = Wo[:, 1] - Wo[:, 0], bo[:, 1] - bo[:, 0]
        wo = wo + (wo.detach().float().double() - wo.detach())
        b0 = b0 + (b0.detach().float().double() - b0.detach())
    else:
        wo, b0 = Wo[:, 0], bo[:, 0]
    z = (h * wo[gt][None]).sum(-1) + b0[gt][None]
    lp = policy.action_log_prob(z, torch.as_tensor(R["action"]))
    cnt = torch.as_tensor(np.bincount(g, minlength=E.G).astype(np.float64))
    (torch.as_tensor(coef) * torch.where(torch.as_tensor(m), lp, torch.zeros_like(lp)) / cnt[gt][None]).sum().backward()
    return [(W.grad.numpy(), b.grad.numpy()) for W, b in P]


def _close(got, want, what):
    scale = max(np.abs(x).max() for wb in want for x in wb)
    assert scale > 0, what
    for (dW, db), (aW, ab) in zip(got, want):
        assert dW.shape == aW.shape and db.shape == ab.shape, what
        assert max(np.abs(dW - aW).max(), np.abs(db - ab).max()) <= 1e-10 * scale, what


@pytest.mark.parametrize("name", L.LAYOUTS)
def test_restatements_are_the_autograd_gradients_on_every_layout(recorded, name):
    """policy_gradient_fp64, policy_gradient_mlp_fp64, imitation_linear_fp64 and imitation_mlp_fp64 on the oracle's rows
    of this layout against torch autograd in fp64, to 1e-10 relative (tests/test_policy_gradient_mlp_cpu.py)"""
    c = recorded[name]
    R, g, ct, n = c["R"], c["g"], c["ct"], L.N_SMALL
    valid = R["valid"]
    forced = np.zeros_like(valid)
    forced[::3] = True  # some days masked
    m = valid & ~forced
    w = np.random.default_rng(8).standard_normal(n)
    A = np.where(valid, R["reward"] - c["beta"], 0.0)
    Q = np.cumsum(A[::-1], axis=0)[::-1].copy()
    ones = np.ones_like(Q)
    W, b = c["pol"]["weight"], c["pol"]["bias"]
    lin = [(W[:, None, :], b[:, None])]
    ref = policy_gradient_fp64(R["obs"], R["action"], valid, forced, R["reward"], c["beta"], W, b, g, E.G)
    assert ref["weight"].shape == (E.G, ct.n_obs)
    _close([(ref["weight"][:, None, :], ref["bias"][:, None])], _surrogate_grad(c, lin, None, Q, m, None), "pg linear")
    ref = imitation_linear_fp64(R["obs"], R["action"], valid, forced, w, W, b, g, E.G)
    assert ref["weight"].shape == (E.G, ct.n_obs)
    _close([(ref["weight"][:, None, :], ref["bias"][:, None])], _surrogate_grad(c, lin, None, ones * w[None, :], m, None),
           "imitation linear")
    for net, (hidden, act, n_out) in MLP_NETS.items():
        layers = E.net(ct, hidden, n_out, seed=7)
        ref = policy_gradient_mlp_fp64(R["obs"], R["action"], valid, forced, R["reward"], c["beta"], layers, act, g, E.G)
        assert ref["layers"][0][0].shape == (E.G, hidden[0], ct.n_obs)
        _close(ref["layers"], _surrogate_grad(c, layers, act, Q, m, None), f"pg {net}")
        ref = imitation_mlp_fp64(R["obs"], R["action"], valid, forced, w, layers, act, g, E.G)
        _close(ref["layers"], _surrogate_grad(c, layers, act, ones * w[None, :], m, None), f"imitation {net}")


# ------------------------------------------------------------------ the near-tie cap
@pytest.mark.parametrize("name", L.LAYOUTS + L.RAGGED)
def test_near_tie_share_of_the_references(tabs, name):
    """every policy of table_edges.POLICIES at the env counts of the GPU file: the share of envs with a decision inside
    the near-tie band anywhere in the episode stays below the 1 % the GPU file asserts, and every policy decides"""
    tb = tabs[name]
    ct = tb.ct
    for n in (L.N_ENVS, L.N_SMALL):
        tup, g = L.host_tuples(tb, n), E.groups(n)
        for pol_name in E.POLICIES:
            pol, fn, ties = L.make_policy(tb, pol_name, g)
            V = tb.oracle()
            E.oracle_reset(V, tup)
            R = E.oracle_record(V, fn, ct.T, ties, uniform=L.policy_uniform(tb, n) if pol["sample"] else None)
            assert R["tie"].mean() < 0.01, (name, pol_name, n, int(R["tie"].sum()))
            assert R["action"][R["valid"]].any() and not R["action"][R["valid"]].all(), (name, pol_name, n)
            assert V._finished.all()
