"""policy["lookahead"] on the GPU: the LOOK forms of k_rollout_linear, k_rollout_mlp, k_policy_gradient_linear and
k_imitation_linear against the restatement (tests/lookahead_restatement.py: the inputs from the tables' host copy and a
twin env's state, the twin stepped day by day with a = policy(cat(obs, f))). N = 193 envs (no multiple of 64), G = 3.
Comparison rules: tests/test_linear_policy_gpu.py and tests/test_mlp_policy_gpu.py (near-tie envs set aside, < 1 %)."""
import numpy as np
import pytest
import torch

import lookahead_cases as C
import lookahead_restatement as LR
import policy_gradient_mlp_cases as M
import table_edges as E
from imitation_restatement import imitation_linear_fp64
from lookahead_cases import FEATURE, G, GID0, MLP_CASES, N, SEED
from policy_gradient_restatement import policy_gradient_fp64
from weather2alert_amd import HeatAlertVecEnv

pytestmark = pytest.mark.gpu

RETURN_RTOL, RETURN_ATOL = 2e-6, 2e-5  # as tests/test_linear_policy_gpu.py
# the twin's side: every env's state as its own last live step left it (lookahead_restatement.twin_loop)
INT_STATE = ("t", "used", "streak", "last_actual", "at_budget", "hist14", "finished")
_groups, _spec, _linear, _mlp = C.groups, C.spec, C.linear, C.mlp  # the cases the CPU file walks on the host oracle


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def TB():
    """name -> (compiled tables, reset seed, reset options): the golden mini tables and table_edges' ragged one"""
    return {k: (ct, cfg["seed"], cfg["opts"]) for k, (ct, cfg, _) in C.make_tables().items()}


def _env(dev, tb, **kw):
    ct, seed, opts = tb
    env = HeatAlertVecEnv(N, tables=ct, device=dev, autoreset="disabled", env_gid0=GID0, similar_climate_counties=True, **kw)
    env.reset(seed=seed, options=dict(opts))
    return env


def _without(pol, ct):
    p = {k: v for k, v in pol.items() if k != "lookahead"}
    if p["kind"] == "linear":
        p["weight"] = pol["weight"][:, :ct.n_obs]
    else:
        p["layers"] = [(pol["layers"][0][0][..., :ct.n_obs], pol["layers"][0][1])] + list(pol["layers"][1:])
    return p


def _zeroed(pol, ct):
    p = dict(pol)
    if p["kind"] == "linear":
        p["weight"] = pol["weight"].copy()
        p["weight"][:, ct.n_obs:] = 0
    else:
        W1 = pol["layers"][0][0].copy()
        W1[..., ct.n_obs:] = 0
        p["layers"] = [(W1, pol["layers"][0][1])] + list(pol["layers"][1:])
    return p


def _same_outputs(a, b, keys=("return", "alerts", "attempts_over_budget", "alert_days", "attempt_days", "final_return", "done")):
    for k in keys:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(torch.nan_to_num(a["return_snapshot"], nan=-7.0), torch.nan_to_num(b["return_snapshot"], nan=-7.0))


def _same_env(A, B):
    sa, sb = A.state(), B.state()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(A._obs, B._obs)


def _against_twin(A, B, ct, out, acc, ok):
    assert acc["tie"].mean() < LR.TIE_CAP, acc["tie"].sum()
    assert acc["alerts"][ok].sum() > 0 and (~acc["days"][ok]).any()  # a policy that decides
    np.testing.assert_array_equal(out["alerts"].cpu().numpy()[ok], acc["alerts"][ok])
    np.testing.assert_array_equal(out["attempts_over_budget"].cpu().numpy()[ok], acc["over"][ok])
    np.testing.assert_array_equal(out["alert_days"].cpu().numpy()[ok], acc["days"][ok])
    np.testing.assert_array_equal(out["attempt_days"].cpu().numpy()[ok], acc["att"][ok])
    np.testing.assert_allclose(out["return"].cpu().numpy()[ok], acc["ret"][ok], rtol=RETURN_RTOL, atol=RETURN_ATOL)
    sa = LR.host_state(A)
    for k in INT_STATE:
        np.testing.assert_array_equal(sa[k][ok], acc["state"][k][ok], err_msg=k)
    np.testing.assert_array_equal(A._obs.cpu().numpy()[ok], acc["obs"][ok])


# ------------------------------------------------------------------ 1: a rule on the weather alone, exact
@pytest.mark.parametrize("table,D,k", [("mini", 1, 1), ("mini", 3, 1), ("mini", 10, 1), ("ragged", 3, 3), ("ragged", 10, 10)])
def test_weather_only_rule_is_exact(dev, TB, table, D, k):
    """observation weights 0, weight 1 on lookahead input k, bias -c with c between two table values of h(r+k) - h(r):
    alert_days is the schedule the table and the budget rule give, bit for bit; past the end the logit is the bias."""
    ct = TB[table][0]
    c = LR.midpoint_threshold(ct, FEATURE, k)
    W = np.zeros((G, ct.n_obs + D), np.float32)
    W[:, ct.n_obs + k - 1] = 1.0
    env = _env(dev, TB[table])
    st = LR.host_state(env)
    out = env.rollout(dict(kind="linear", weight=W, bias=np.full(G, -c, np.float32), group=_groups(), lookahead=_spec(D)),
                      alert_mask=True)
    assert env.last_rollout_kernel == "k_rollout_linear" and env.check_status() == 0
    h = LR.series(ct, FEATURE)
    row = st["county_w"].astype(np.int64) * ct.Y + st["year_i"]
    want, att = np.zeros((N, ct.T), bool), np.zeros((N, ct.T), bool)
    for e in range(N):
        used = 0
        for t in range(int(st["n_days"][e])):
            r = max(t - 1, 0)
            f = np.float32(h[row[e], r + k] - h[row[e], r]) if r + k < st["n_days"][e] else np.float32(0)
            att[e, t] = f > c
            want[e, t] = att[e, t] and used < st["budget"][e]
            used += want[e, t]
    assert want.any() and att.sum() > want.sum() and not want.all()  # the rule fires, and the budget binds somewhere
    np.testing.assert_array_equal(out["alert_days"].cpu().numpy(), want)
    np.testing.assert_array_equal(out["attempt_days"].cpu().numpy(), att)
    if table == "ragged":  # the last k held rows of every env see 0: no attempt on their decisions
        nd = st["n_days"]
        for e in range(N):
            assert not att[e, max(int(nd[e]) - k + 1, 1):int(nd[e])].any()
    env.close()


# ------------------------------------------------------------------ 2: step equivalence
@pytest.mark.parametrize("table,D,sample", C.LINEAR_CASES)
def test_linear_rollout_equals_the_stepped_twin(dev, TB, table, D, sample):
    ct = TB[table][0]
    A, B = _env(dev, TB[table]), _env(dev, TB[table])
    pol = _linear(ct, D, sample)
    st0 = LR.host_state(B)
    uni = LR.policy_uniform(SEED, GID0, st0) if sample else None
    out = A.rollout(pol, alert_mask=True)
    acc = LR.twin_loop(B, ct, _spec(D), lambda x: LR.linear_logit(pol["weight"], pol["bias"], pol["group"], x), ct.T,
                       "linear", uniform=uni)
    assert A.check_status() == 0 and out["done"].all()
    _against_twin(A, B, ct, out, acc, ~acc["tie"])
    A.close(), B.close()


@pytest.mark.parametrize("name,D,sample", MLP_CASES)
def test_mlp_rollout_equals_the_stepped_twin(dev, TB, name, D, sample):
    """all six <WIDTH, LAYERS> instantiations (tests/policy_gradient_mlp_cases.py: MATRIX), the first layer D wider"""
    table = C.mlp_table(D)
    ct = TB[table][0]
    A, B = _env(dev, TB[table]), _env(dev, TB[table])
    pol = _mlp(ct, name, D, sample)
    st0 = LR.host_state(B)
    uni = LR.policy_uniform(SEED, GID0, st0) if sample else None
    out = A.rollout(pol, alert_mask=True)
    assert A.last_rollout_kernel == "k_rollout_mlp"
    acc = LR.twin_loop(B, ct, _spec(D), lambda x: E.mlp64(pol["layers"], pol["activation"], x, pol["group"]), ct.T,
                       "mlp", uniform=uni)
    assert A.check_status() == 0 and out["done"].all()
    _against_twin(A, B, ct, out, acc, ~acc["tie"])
    A.close(), B.close()


def test_all_six_mlp_instantiations_are_covered():
    assert {M.MATRIX[n][0] for n, _, _ in MLP_CASES} == {(w, l) for w in (16, 32, 64) for l in (1, 2)}


# ------------------------------------------------------------------ 3: zero lookahead columns change no bit
@pytest.mark.parametrize("kind,D", [("linear", 3), ("linear", 10), ("mlp", 1), ("mlp", 10)])
def test_zero_lookahead_columns_give_the_bits_of_the_call_without_the_key(dev, TB, kind, D):
    ct = TB["ragged"][0]
    pol = _zeroed(_linear(ct, D, sample=True) if kind == "linear" else _mlp(ct, "relu40x64", D, sample=True), ct)
    A, B = _env(dev, TB["ragged"]), _env(dev, TB["ragged"])
    oa = A.rollout(pol, n_steps=40, alert_mask=True)
    ob = B.rollout(_without(pol, ct), n_steps=40, alert_mask=True)
    _same_outputs(oa, ob)
    _same_env(A, B)
    oa, ob = A.rollout(pol, alert_mask=True), B.rollout(_without(pol, ct), alert_mask=True)
    _same_outputs(oa, ob)
    _same_env(A, B)
    A.close(), B.close()


# ------------------------------------------------------------------ 4: chunking
@pytest.mark.parametrize("kind,D,k", [("linear", 3, 1), ("linear", 10, -4), ("mlp", 10, 1), ("mlp", 3, -2)])
def test_two_calls_equal_one(dev, TB, kind, D, k):
    """k days then the rest equal one call, bit for bit: the state (the episode's running return included), the
    observation buffer, the bitmaps and the counters. k < 0: T + k days, so the second call starts inside the last D."""
    ct = TB["mini"][0]
    k = k if k > 0 else ct.T + k
    pol = _linear(ct, D, sample=True) if kind == "linear" else _mlp(ct, "tanh29x9", D, sample=True)
    A, B = _env(dev, TB["mini"]), _env(dev, TB["mini"])
    whole = A.rollout(pol, alert_mask=True)
    first = B.rollout(pol, n_steps=k, alert_mask=True)
    second = B.rollout(pol, alert_mask=True)
    _same_env(A, B)
    for key in ("alerts", "attempts_over_budget"):
        assert torch.equal(whole[key], first[key] + second[key]), key
    for key in ("alert_days", "attempt_days"):
        assert torch.equal(whole[key], first[key] | second[key]), key
    assert torch.equal(whole["final_return"], second["final_return"]) and second["done"].all()
    A.close(), B.close()


# ------------------------------------------------------------------ 5: with a gate
@pytest.mark.parametrize("kind,D", C.GATE_CASES)
def test_gate_and_lookahead_equal_the_gated_twin(dev, TB, kind, D):
    ct = TB["ragged"][0]
    A, B = _env(dev, TB["ragged"]), _env(dev, TB["ragged"])
    gate = A.alert_gate(FEATURE, C.GATE_THRESHOLD)
    g = gate.cpu().numpy()
    assert g.any() and not g.all()
    pol = (_linear(ct, D) if kind == "linear" else _mlp(ct, C.GATE_NET, D))
    fn = (lambda x: LR.linear_logit(pol["weight"], pol["bias"], pol["group"], x)) if kind == "linear" else \
        (lambda x: E.mlp64(pol["layers"], pol["activation"], x, pol["group"]))
    out = A.rollout(dict(pol, allowed_days=gate), alert_mask=True)
    acc = LR.twin_loop(B, ct, _spec(D), fn, ct.T, kind, gate=g)
    assert not (out["alert_days"].cpu().numpy() & ~g).any() and not (out["attempt_days"].cpu().numpy() & ~g).any()
    _against_twin(A, B, ct, out, acc, ~acc["tie"])
    A.close(), B.close()


# ------------------------------------------------------------------ 6: lookahead_features()
@pytest.mark.parametrize("table", ["mini", "ragged"])
def test_lookahead_features_equal_the_restatement(dev, TB, table):
    ct = TB[table][0]
    env = _env(dev, TB[table])
    tab = env.lookahead_table(FEATURE)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (ct.S_w * ct.Y, ct.T) and tab.is_contiguous()
    assert env.lookahead_table(FEATURE) is tab  # built once
    np.testing.assert_array_equal(tab.cpu().numpy(), LR.series(ct, FEATURE))

    def check():
        for D in (1, 3, 10):
            f = env.lookahead_features(_spec(D))
            assert f.dtype == torch.float32 and tuple(f.shape) == (N, D)
            np.testing.assert_array_equal(f.cpu().numpy(), LR.inputs(ct, FEATURE, D, LR.host_state(env)))

    check()
    for _ in range(2):
        env.step(torch.ones(N, dtype=torch.int32, device=dev))
        check()
    env.rollout(_linear(ct, 3), n_steps=17)
    check()
    env.rollout(_linear(ct, 3))  # every env on its last day: mostly zeros
    check()
    with pytest.raises(ValueError):
        env.lookahead_features({"feature": "remaining_budget", "days": 2})
    for bad in ("no_such_column", "remaining_budget"):
        with pytest.raises(ValueError, match="lookahead_table"):
            env.lookahead_table(bad)
    env.close()
    assert env._look_tables == {}  # close() drops the series tables


# ------------------------------------------------------------------ 7: gradients, linear
def _grad(out):
    g = out["policy_gradient"]
    return np.concatenate([g["weight"].double().cpu().numpy(), g["bias"].double().cpu().numpy()[:, None]], axis=1)


def _within(got, ref, what):
    want = np.concatenate([ref["weight"], ref["bias"][:, None]], axis=1)
    diff = np.abs(got - want)
    ratio = float(np.where(ref["bound"] > 0, diff / np.where(ref["bound"] > 0, ref["bound"], 1.0), 0.0).max())
    print(f"{what}: max |g - g_ref| / bound = {ratio:.3e}   (max |g_ref| = {np.abs(want).max():.3e})")
    assert np.isfinite(got).all() and (diff <= ref["bound"]).all(), (what, ratio)


@pytest.mark.parametrize("table,D", C.GRADIENT_CASES)
def test_policy_gradient_matches_the_restatement(dev, TB, table, D):
    """both baselines against policy_gradient_fp64 on the rows cat(obs, f) of the stepped twin (the bounds of
    tests/policy_gradient_restatement.py); beta from a third twin stepped with no alerts"""
    ct = TB[table][0]
    pol = _linear(ct, D, sample=True)
    A1, A2, B, C = (_env(dev, TB[table]) for _ in range(4))
    st0 = LR.host_state(B)
    got = {"none": A1.rollout(pol, policy_gradient="none"), "no_alert": A2.rollout(pol, policy_gradient="no_alert")}
    assert tuple(got["none"]["policy_gradient"]["weight"].shape) == (G, ct.n_obs + D)
    acc = LR.twin_loop(B, ct, _spec(D), lambda x: LR.linear_logit(pol["weight"], pol["bias"], pol["group"], x), ct.T,
                       "linear", uniform=LR.policy_uniform(SEED, GID0, st0))
    # the group means hold every env, so a near-tie of the twin's own draws would spoil the comparison: the seeds
    # above give none (a property of the restatement alone, not of the kernel)
    assert not acc["tie"].any(), acc["tie"].sum()
    tr = acc["traj"]
    beta = np.zeros_like(tr["reward"])
    for s in range(ct.T):
        beta[s] = C.step(torch.zeros(N, dtype=torch.int32, device=dev))[1].cpu().numpy()
    for bl in ("none", "no_alert"):
        ref = policy_gradient_fp64(tr["x"], tr["action"], tr["valid"], np.zeros_like(tr["valid"]), tr["reward"],
                                   beta if bl == "no_alert" else None, pol["weight"], pol["bias"][:G], pol["group"], G)
        _within(_grad(got[bl]), ref, f"{table} D={D} {bl}")
    for e in (A1, A2, B, C):
        e.close()


@pytest.mark.parametrize("table,D", [("mini", 3), ("ragged", 10)])
def test_imitation_gradient_along_the_hindsight_optimum(dev, TB, table, D):
    ct = TB[table][0]
    pol = _linear(ct, D)
    A, B = _env(dev, TB[table]), _env(dev, TB[table])
    sched = A.hindsight_optimum()["alert_days"]
    out = A.imitation_gradient(pol, sched)
    again = A.imitation_gradient(pol, sched)
    for k in ("weight", "bias"):
        assert torch.equal(out["policy_gradient"][k], again["policy_gradient"][k])  # deterministic
    assert tuple(out["policy_gradient"]["weight"].shape) == (G, ct.n_obs + D)
    acc = LR.twin_loop(B, ct, _spec(D), lambda x: LR.linear_logit(pol["weight"], pol["bias"], pol["group"], x), ct.T,
                       "linear", schedule=sched.cpu().numpy())
    tr = acc["traj"]
    ref = imitation_linear_fp64(tr["x"], tr["action"], tr["valid"], np.zeros_like(tr["valid"]), None, pol["weight"],
                                pol["bias"], pol["group"], G)
    np.testing.assert_array_equal(out["days"].cpu().numpy(), ref["days"])
    assert (np.abs(out["log_likelihood"].double().cpu().numpy() - ref["ll"]) <= ref["ll_bound"]).all()
    _within(_grad(out), ref, f"imitation {table} D={D}")
    assert np.abs(ref["weight"][:, ct.n_obs:]).min() > 0  # the lookahead columns carry a gradient
    A.close(), B.close()


@pytest.mark.parametrize("D", [3, 10])
def test_gradients_with_zero_lookahead_weights_keep_the_other_columns_bits(dev, TB, D):
    ct = TB["ragged"][0]
    pol = _zeroed(_linear(ct, D, sample=True), ct)
    A, B = _env(dev, TB["ragged"]), _env(dev, TB["ragged"])
    for bl in ("none", "no_alert"):
        ga = A.rollout(pol, n_steps=60, policy_gradient=bl)["policy_gradient"]
        gb = B.rollout(_without(pol, ct), n_steps=60, policy_gradient=bl)["policy_gradient"]
        assert torch.equal(ga["weight"][:, :ct.n_obs], gb["weight"]) and torch.equal(ga["bias"], gb["bias"]), bl
        assert ga["weight"][:, ct.n_obs:].abs().sum() > 0
        _same_env(A, B)
    A2, B2 = _env(dev, TB["ragged"]), _env(dev, TB["ragged"])
    g1 = A2.rollout(pol, policy_gradient="no_alert")["policy_gradient"]
    g2 = B2.rollout(pol, policy_gradient="no_alert")["policy_gradient"]
    assert torch.equal(g1["weight"], g2["weight"]) and torch.equal(g1["bias"], g2["bias"])  # identical calls, identical bits
    C, D_ = _env(dev, TB["ragged"]), _env(dev, TB["ragged"])
    days = C.hindsight_optimum()["alert_days"]
    ia = C.imitation_gradient(pol, days)
    ib = D_.imitation_gradient(_without(pol, ct), days)
    assert torch.equal(ia["policy_gradient"]["weight"][:, :ct.n_obs], ib["policy_gradient"]["weight"])
    assert torch.equal(ia["policy_gradient"]["bias"], ib["policy_gradient"]["bias"])
    assert torch.equal(ia["log_likelihood"], ib["log_likelihood"]) and torch.equal(ia["days"], ib["days"])
    for e in (A, B, A2, B2, C, D_):
        e.close()


# ------------------------------------------------------------------ 8: the refusals, on the GPU build
def test_refusals_on_a_live_env(dev, TB):
    ct = TB["mini"][0]
    env = _env(dev, TB["mini"])
    lin, mlp = _linear(ct, 3, sample=True), _mlp(ct, "tanh7x13", 3, sample=True)
    days = torch.zeros((N, ct.T), dtype=torch.bool, device=dev)
    adv = torch.zeros((ct.T, N), device=dev)
    before = {k: v.clone() for k, v in env.state().items()}
    with pytest.raises(ValueError, match="lookahead"):
        env.rollout(lin, record=True)
    with pytest.raises(ValueError, match="lookahead"):
        env.rollout(mlp, policy_gradient="none")
    with pytest.raises(ValueError, match="lookahead"):
        env.imitation_gradient(mlp, days)
    for pol in (lin, mlp):
        with pytest.raises(ValueError, match="lookahead"):
            env.surrogate_gradient(pol, days, adv)
        with pytest.raises(ValueError, match="lookahead"):
            env.fisher_vector_product(pol, days, {})
        with pytest.raises(ValueError, match="lookahead"):
            env.value_gradient(pol, days)
    with pytest.raises(ValueError, match="lookahead"):
        env.q_gradient(mlp, days)
    with pytest.raises(ValueError, match="unknown|no observation column"):
        env.rollout(dict(lin, lookahead={"feature": "nope", "days": 3}))
    after = env.state()
    for k in before:
        assert torch.equal(before[k], after[k]), k
    env.close()
