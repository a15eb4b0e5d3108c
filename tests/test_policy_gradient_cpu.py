"""The estimator of rollout(policy_gradient=...) without a GPU: the fp64 restatement the GPU tests compare the kernel
with (tests/policy_gradient_restatement.py) is the gradient of the REINFORCE surrogate, points the way the exact one-day
gradient points, its baseline does not depend on the policy, and every refusal of the keyword is a ValueError before
anything could be launched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402
from policy_gradient_restatement import forced_days, policy_gradient_fp64  # noqa: E402

from oracle import heatalert_oracle as O  # noqa: E402
from weather2alert_amd import _ffi, build, policy, tables  # noqa: E402


@pytest.fixture(scope="module")
def tabs():
    return E.make_tables()


def _mini(golden_dir, mini_root, n=200):
    """(ct, oracle, episode tuples) on the committed mini data set"""
    ct = tables.CompiledTables.load_npz(os.path.join(golden_dir, "mini_compiled.npz"))
    V = O.VectorOracle(O.RefData.from_files(mini_root, weights="linear", split="65k"), ct.fips_weather, ct.years)
    rng = np.random.default_rng(4)
    cols = np.nonzero(np.asarray(ct.fips_to_weather) >= 0)[0]
    cc = rng.choice(cols, n)
    cw = np.asarray(ct.fips_to_weather)[cc].astype(np.int64)
    yi = rng.integers(0, len(ct.years), n)
    tup = dict(county_w=cw, coef_col=cc.astype(np.int64), year_i=yi, sample=rng.integers(0, ct.n_samples, n),
               budget=rng.integers(0, 9, n), n_days=np.asarray(ct.n_days)[cw * len(ct.years) + yi].astype(np.int64))
    return ct, V, tup


def _no_alert_rewards(V, tup, S):
    """per-day rewards [S, n] of the same episodes stepped with no alert from the start"""
    E.oracle_reset(V, tup)
    out = np.zeros((S, len(tup["budget"])))
    for s in range(S):
        r, _, _, live = E.oracle_step(V, np.zeros(len(tup["budget"]), np.int64))
        out[s] = np.where(live, r, 0.0)
    return out


def _record(V, ct, tup, g, seed=E.POLICY_SEED, S=None):
    n = len(tup["budget"])
    W, b = E.linear_params(ct)
    W64, b64 = W.astype(np.float64)[g], b.astype(np.float64)[g]

    def fn(obs):
        prod = obs.astype(np.float64) * W64
        return prod.sum(axis=1) + b64, np.abs(prod).sum(axis=1) + np.abs(b64)

    uni = lambda t: O.devrng_policy_uniform_vec(seed, E.GID0 + np.arange(n), np.zeros(n, np.int64), t)  # noqa: E731
    E.oracle_reset(V, tup)
    return E.oracle_record(V, fn, ct.T if S is None else S, (1e-9, 1e-6), uniform=uni, T=ct.T), W, b


def _surrogate_grad(R, forced, beta, W, b, g, G):
    """torch.autograd of sum_e sum_s stopgrad(Q_s) m_s log pi(a_s | o_s) in fp64, divided by each group's env count"""
    valid = R["valid"]
    A = np.where(valid, R["reward"] - (0.0 if beta is None else beta), 0.0)
    Q = torch.as_tensor(np.cumsum(A[::-1], axis=0)[::-1].copy())
    Wt = torch.tensor(W.astype(np.float64), requires_grad=True)
    bt = torch.tensor(b.astype(np.float64), requires_grad=True)
    gt = torch.as_tensor(g)
    S = valid.shape[0]
    o = torch.as_tensor(R["obs"][:S].astype(np.float64))
    z = (o * Wt[gt][None]).sum(-1) + bt[gt][None]
    m = torch.as_tensor(valid & ~forced)
    lp = policy.action_log_prob(z, torch.as_tensor(R["action"]))
    (Q * torch.where(m, lp, torch.zeros_like(lp))).sum().backward()
    cnt = np.bincount(g, minlength=G).astype(np.float64)
    return Wt.grad.numpy() / cnt[:, None], bt.grad.numpy() / cnt


def _check_surrogate(V, ct, tup, what):
    n = len(tup["budget"])
    g = E.groups(n)
    R, W, b = _record(V, ct, tup, g)
    S = R["valid"].shape[0]
    beta = _no_alert_rewards(V, tup, S)
    # any mask of forced days must drop out of both sides: the days require_budget would have forced
    forced = forced_days(True, tup["budget"], np.zeros(n, np.int64), R["alert"], R["valid"])
    assert forced[R["valid"]].any() and R["alert"].any()
    for bl in (None, beta):
        for f in (np.zeros_like(forced), forced):
            ref = policy_gradient_fp64(R["obs"], R["action"], R["valid"], f, R["reward"], bl, W, b, g, E.G)
            gw, gb = _surrogate_grad(R, f, bl, W, b, g, E.G)
            scale = max(np.abs(gw).max(), np.abs(gb).max())
            assert scale > 0
            err = max(np.abs(ref["weight"] - gw).max(), np.abs(ref["bias"] - gb).max())
            assert err <= 1e-12 * scale, (what, err, scale)


def test_restatement_is_the_gradient_of_the_surrogate_mini(golden_dir, mini_root):
    ct, V, tup = _mini(golden_dir, mini_root)
    _check_surrogate(V, ct, tup, "mini")


@pytest.mark.parametrize("name", ["ragged", "slot27", "ragged27"])
def test_restatement_is_the_gradient_of_the_surrogate_edges(tabs, name):
    tb = tabs[name]
    _check_surrogate(tb.oracle(), tb.ct, E.host_tuples(tb, 300), name)


@pytest.mark.parametrize("baseline", ["none", "no_alert"])
def test_one_day_gradient_points_the_right_way(tabs, baseline):
    """n_steps = 1: the exact gradient of the expected reward is sigma (1 - sigma) (r1 - r0) (o, 1). The restatement
    averaged over K independent uniforms agrees within 5 standard errors, K doubled until the standard error is under
    10 % of the exact norm."""
    tb = tabs["slot27"]
    ct, n = tb.ct, 48
    tup = E.host_tuples(tb, n)
    assert (tup["budget"] > 0).all()
    V = tb.oracle()
    W, b = E.linear_params(ct)
    g = np.zeros(n, np.int64)
    r = {}
    for a in (0, 1):
        E.oracle_reset(V, tup)
        obs = V.obs.astype(np.float32).astype(np.float64)
        r[a] = E.oracle_step(V, np.full(n, a, np.int64))[0]
    z = obs @ W[0].astype(np.float64) + float(b[0])
    p = 1.0 / (1.0 + np.exp(-z))
    o1 = np.concatenate([obs, np.ones((n, 1))], axis=1)
    exact = ((p * (1 - p) * (r[1] - r[0]))[:, None] * o1).mean(axis=0)
    beta = r[0] if baseline == "no_alert" else None  # one day from the start state: the no-alert reward is r0
    rng = np.random.default_rng(12)
    K = 1 << 10
    while True:
        per_draw = np.zeros((K, n))
        u = rng.random((K, n))
        act = (u < p[None, :]).astype(np.uint8)
        for lo in range(0, K, 256):  # the restatement itself, 256 draws at a time stacked as envs
            a_ = act[lo:lo + 256].reshape(1, -1)
            k_ = a_.shape[1] // n
            rew = np.where(a_ == 1, np.tile(r[1], k_)[None], np.tile(r[0], k_)[None])
            ref = policy_gradient_fp64(np.tile(obs, (k_, 1))[None], a_, np.ones_like(a_, bool), np.zeros_like(a_, bool),
                                       rew, None if beta is None else np.tile(beta, k_)[None], W[:1], b[:1], None, 1)
            per_draw[lo:lo + k_] = ref["per_env"][:, -1].reshape(k_, n)  # bias column: delta_s Q_s itself
        c_mean, c_var = per_draw.mean(axis=0), per_draw.var(axis=0, ddof=1)
        est = (c_mean[:, None] * o1).mean(axis=0)
        se = np.sqrt((c_var[:, None] * o1 ** 2).sum(axis=0) / K) / n
        if np.linalg.norm(se) < 0.1 * np.linalg.norm(exact) or K >= 1 << 18:
            break
        K *= 4
    assert np.linalg.norm(se) < 0.1 * np.linalg.norm(exact), (K, np.linalg.norm(se), np.linalg.norm(exact))
    assert (np.abs(est - exact) <= 5 * se + 1e-15).all(), (K, np.abs(est - exact) / np.maximum(se, 1e-300))
    assert est @ exact > 0


def test_forced_day_has_zero_gradient(tabs):
    """require_budget with no budget left: the action is off the policy's distribution, the gradient exactly 0"""
    tb = tabs["slot27"]
    ct, n = tb.ct, 16
    tup = E.host_tuples(tb, n)
    tup["budget"] = np.zeros(n, np.int64)
    V = tb.oracle()
    E.oracle_reset(V, tup)
    obs = V.obs.astype(np.float32)[None]
    r = E.oracle_step(V, np.zeros(n, np.int64))[0][None]
    W, b = E.linear_params(ct)
    valid = np.ones((1, n), bool)
    forced = forced_days(True, tup["budget"], np.zeros(n, np.int64), np.zeros((1, n), bool), valid)
    assert forced.all()
    ref = policy_gradient_fp64(obs, np.zeros((1, n), np.uint8), valid, forced, r, None, W[:1], b[:1], None, 1)
    assert not ref["weight"].any() and not ref["bias"].any() and not ref["per_env"].any()


def test_baseline_is_action_independent(tabs):
    """the no-alert rewards of the same episodes under two policy seeds (different actions) are equal bit for bit"""
    tb = tabs["ragged27"]
    ct = tb.ct
    tup = E.host_tuples(tb, 200)
    g = E.groups(200)
    V = tb.oracle()
    runs = []
    for seed in (1, 2):
        R, _, _ = _record(V, ct, tup, g, seed=seed)
        runs.append((R["action"].copy(), _no_alert_rewards(V, tup, ct.T)))
    assert (runs[0][0] != runs[1][0]).any()
    np.testing.assert_array_equal(runs[0][1], runs[1][1])


def test_policy_gradient_keyword_checks():
    ok = policy.check_policy_gradient
    assert ok(False, "linear", True) is None and ok(False, "never", False, "posterior_mean", {"lag"}, True) is None
    assert ok(True, "linear", True) == "no_alert" and ok("no_alert", "linear", True, "sampled", {"budget"}) == "no_alert"
    assert ok("none", "linear", np.bool_(True)) == "none"
    for args in ((True, "linear", False), (True, "mlp", True), (True, "never", True), (True, "bernoulli", True),
                 (True, "threshold", True), (True, "table", True), ("none", "linear", True, "posterior_mean"),
                 ("none", "linear", True, "sampled", {"lag"}), ("none", "linear", True, "sampled", {"budget", "obs"}),
                 ("critic", "linear", True), (1, "linear", True), ("none", "linear", True, "sampled", (), True),
                 ("none", "linear", 1)):
        with pytest.raises(ValueError):
            ok(*args)


def test_policy_gradient_entry_refuses_bad_arguments_without_gpu():
    build.build_lib()
    lib = _ffi.load()
    assert {"w2a_policy_gradient_linear", "w2a_policy_gradient_workspace_bytes"} <= set(_ffi.SYMBOLS)
    assert lib.w2a_policy_gradient_workspace_bytes(1000, 153) >= 9 * 1000 * 153
    assert lib.w2a_policy_gradient_workspace_bytes(0, 5) == 0 and lib.w2a_policy_gradient_workspace_bytes(5, 0) == 0
    w, b, obs, grad = (C.c_float * 32)(), (C.c_float * 1)(), (C.c_float * 29)(), (C.c_float * 30)()
    ws = (C.c_char * 1024)()
    ws_p = (C.addressof(ws) + 255) & ~255

    def pol(**kw):
        p = _ffi.LinearPolicy()
        p.weight, p.bias, p.group, p.n_groups, p.sample, p.require_budget, p.seed = (
            C.cast(w, C.c_void_p), C.cast(b, C.c_void_p), None, 1, 1, 0, 0)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def call(p, baseline=1, n_steps=10, ob=obs, gr=grad, wsp=ws_p):
        return lib.w2a_policy_gradient_linear(None, None if p is None else C.byref(p), baseline, n_steps,
                                              None if ob is None else C.cast(ob, C.c_void_p),
                                              None if gr is None else C.cast(gr, C.c_void_p), wsp, 512, None)

    for kw, msg in ((dict(p=None), b"NULL policy"), (dict(p=pol(), n_steps=0), b"n_steps"),
                    (dict(p=pol(weight=None)), b"NULL weight"), (dict(p=pol(n_groups=0)), b"n_groups"),
                    (dict(p=pol(sample=0)), b"sample must be 1"), (dict(p=pol(require_budget=2)), b"require_budget"),
                    (dict(p=pol(), baseline=2), b"baseline"), (dict(p=pol(), ob=None), b"NULL obs"),
                    (dict(p=pol(), gr=None), b"NULL grad"), (dict(p=pol(), wsp=None), b"NULL grad or workspace"),
                    (dict(p=pol(), wsp=ws_p + 4), b"256-B aligned"), (dict(p=pol()), b"NULL handle")):
        assert call(**kw) == -1
        assert msg in lib.w2a_last_error(), (msg, lib.w2a_last_error())


def test_group_mean_columns_equals_group_mean():
    rng = np.random.default_rng(0)
    v = torch.as_tensor(rng.standard_normal((5000, 7)).astype(np.float32))
    g = torch.as_tensor(rng.integers(0, 11, 5000))
    a, b_ = policy.group_mean(v, g, 13), policy.group_mean_columns(v.T.contiguous(), g, 13)
    assert b_.shape == (13, 7) and b_.dtype == torch.float32
    np.testing.assert_allclose(a[:11].numpy(), b_[:11].numpy(), rtol=1e-6, atol=1e-7)
    assert torch.isnan(b_[11:]).all()
    np.testing.assert_allclose(policy.group_mean_columns(v.T.contiguous(), None, 1).numpy(),
                               v.double().mean(0, keepdim=True).numpy(), rtol=1e-6)
    assert torch.equal(b_.nan_to_num(0.0), policy.group_mean_columns(v.T.contiguous(), g, 13).nan_to_num(0.0))
