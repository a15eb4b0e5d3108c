"""policy["lookahead"] on other tables and layouts, on the GPU (tests/lookahead_layout_cases.py): the LOOK forms of
k_rollout_linear, k_rollout_mlp, k_policy_gradient_linear and k_imitation_linear, lookahead_table() and
lookahead_features(), on observation layouts whose columns sit on slots that are not their index (n_obs 29, 28, 8, 5 and
the ragged variants), with features other than heat_qi, D on both sides of every first-layer k-step of four, and on the
slot-27 tables. Every comparison is against the stepped twin (lookahead_restatement.twin_loop: step() driven by the fp64
logit on cat(obs, restated f)) or an fp64 restatement, never against another lookahead kernel; the bounds are those of
tests/test_lookahead_gpu.py and of the restatements. N = 193 envs, G = 3 groups, T <= 60 days.
tests/test_lookahead_layouts_cpu.py holds the input conditions of every case without a GPU."""
import dataclasses

import numpy as np
import pytest
import torch

import lookahead_layout_cases as K
import lookahead_restatement as LR
import obs_layouts as L
import policy_gradient_mlp_cases as M
from imitation_restatement import imitation_linear_fp64
from lookahead_cases import groups, logit_fn
from lookahead_layout_cases import G, GID0, N
from policy_gradient_restatement import policy_gradient_fp64
from weather2alert_amd import HeatAlertVecEnv

pytestmark = pytest.mark.gpu

RETURN_RTOL, RETURN_ATOL = 2e-6, 2e-5  # tests/test_lookahead_gpu.py (as tests/test_linear_policy_gpu.py), unchanged
INT_STATE = ("t", "used", "streak", "last_actual", "at_budget", "hist14", "finished")  # tests/test_lookahead_gpu.py
FEATURE_DAYS = (4, 5, 9)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tabs():
    return K.make_tables()


def _env(dev, tb, ct=None, options=None, **kw):
    cfg = K.reset_cfg(tb.name)
    env = HeatAlertVecEnv(N, tables=tb.ct if ct is None else ct, device=dev, autoreset="disabled", env_gid0=GID0,
                          similar_climate_counties=True, **kw)
    env.reset(seed=cfg["seed"], options=dict(cfg["opts"]) if options is None else options)
    return env


def _same_outputs(a, b, keys=("return", "alerts", "attempts_over_budget", "alert_days", "attempt_days", "final_return", "done")):
    for k in keys:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(torch.nan_to_num(a["return_snapshot"], nan=-7.0), torch.nan_to_num(b["return_snapshot"], nan=-7.0))


def _same_env(A, B):
    sa, sb = A.state(), B.state()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(A._obs, B._obs)


def _against_twin(A, out, acc, ok):
    """tests/test_lookahead_gpu.py's comparison: near-tie envs set aside (< 1 %), everything else bit for bit, the
    return within that file's bound"""
    assert acc["tie"].mean() < LR.TIE_CAP, acc["tie"].sum()
    assert acc["alerts"][ok].sum() > 0 and (~acc["days"][ok]).any()  # a policy that decides
    np.testing.assert_array_equal(out["alerts"].cpu().numpy()[ok], acc["alerts"][ok])
    np.testing.assert_array_equal(out["attempts_over_budget"].cpu().numpy()[ok], acc["over"][ok])
    np.testing.assert_array_equal(out["alert_days"].cpu().numpy()[ok], acc["days"][ok])
    np.testing.assert_array_equal(out["attempt_days"].cpu().numpy()[ok], acc["att"][ok])
    ret = out["return"].double().cpu().numpy()
    err = np.abs(ret - acc["ret"])[ok]
    print(f"    max |return - twin| = {err.max():.2e}, worst ratio to the bound "
          f"{(err / (RETURN_ATOL + RETURN_RTOL * np.abs(acc['ret'][ok]))).max():.2e}")
    np.testing.assert_allclose(ret[ok], acc["ret"][ok], rtol=RETURN_RTOL, atol=RETURN_ATOL)
    sa = LR.host_state(A)
    for k in INT_STATE:
        np.testing.assert_array_equal(sa[k][ok], acc["state"][k][ok], err_msg=k)
    np.testing.assert_array_equal(A._obs.cpu().numpy()[ok], acc["obs"][ok])


def _uniform(pol, B):
    return LR.policy_uniform(pol["seed"], GID0, LR.host_state(B)) if pol["sample"] else None


# ------------------------------------------------------------------ 1: lookahead_table() / lookahead_features()
def _features(ct):
    feats = ["heat_qi"]
    c = L.offset_column(ct)
    if c is not None:
        feats.append(ct.feature_names[c])
    if "alerts_2wks" in ct.feature_names:
        feats.append("alerts_2wks")
    return feats


@pytest.mark.parametrize("table", K.LAYOUT_TABLES)
def test_lookahead_table_and_features_equal_the_restatement(dev, tabs, table):
    """the series of a feature is the table column of its SLOT (obs_slot[column index]), not of its column index:
    lookahead_table() and lookahead_features() bit-equal to lookahead_restatement.series / inputs at reset, after 7
    days of step() (the 1-, 2- and 3-day episodes of the ragged tables are over by then) and at every episode's end"""
    tb = tabs[table]
    ct = tb.ct
    env = _env(dev, tb)
    feats = _features(ct)
    assert table == "narrow" or len(feats) >= 2
    for f in feats:
        col = ct.feature_names.index(f)
        if f != "alerts_2wks" and table != "narrow":
            assert ct.obs_slot[col] != col  # the layouts put these columns on other slots than their index
        tab = env.lookahead_table(f)
        assert tab.dtype == torch.float32 and tuple(tab.shape) == (ct.S_w * ct.Y, ct.T) and tab.is_contiguous()
        np.testing.assert_array_equal(tab.cpu().numpy(), LR.series(ct, f), err_msg=f)

    def check(when):
        st = LR.host_state(env)
        for f in feats:
            for D in FEATURE_DAYS:
                got = env.lookahead_features(K.spec(f, D))
                assert got.dtype == torch.float32 and tuple(got.shape) == (N, D)
                np.testing.assert_array_equal(got.cpu().numpy(), LR.inputs(ct, f, D, st), err_msg=f"{f} D={D} {when}")

    check("at reset")
    rng = np.random.default_rng(4)
    for _ in range(7):
        fin = env.state()["finished"].cpu().numpy().astype(bool)
        env.step(torch.as_tensor(np.where(fin, 0, rng.random(N) < 0.3).astype(np.int32), device=dev))
    if tb.ragged:
        assert (LR.host_state(env)["finished"] == 1).any()
    check("after 7 days")
    env.rollout(dict(kind="linear", weight=np.zeros((1, ct.n_obs), np.float32), bias=np.array([-1.0], np.float32)))
    assert (LR.host_state(env)["finished"] == 1).all()
    check("at the end")
    env.close()


def test_lookahead_table_refuses_the_run_time_columns(dev, tabs):
    ct = tabs["permuted"].ct
    env = _env(dev, tabs["permuted"])
    for bad in K.RUN_TIME_COLUMNS:
        assert 24 <= ct.obs_slot[ct.feature_names.index(bad)] <= 27
        with pytest.raises(ValueError, match="table-sourced"):
            env.lookahead_table(bad)
        with pytest.raises(ValueError, match="table-sourced"):
            env.lookahead_features(K.spec(bad, 4))
    assert env.lookahead_table("alerts_2wks").shape == (ct.S_w * ct.Y, ct.T)  # the table's own count is a table column
    env.close()


# ------------------------------------------------------------------ 2: a rule on the weather alone, exact
@pytest.mark.parametrize("table,feature,D,k", K.WEATHER_RULE_CASES)
def test_weather_only_rule_is_exact(dev, tabs, table, feature, D, k):
    """observation weights 0, weight 1 on lookahead input k, bias -c with c between two table values of h(r + k) - h(r):
    alert_days and attempt_days are the schedule the table and the budget rule give, bit for bit, for every env (there
    is no near-tie by construction). A series read from the wrong slot gives another schedule."""
    tb = tabs[table]
    ct = tb.ct
    W, b, c = K.weather_rule(ct, feature, D, k)
    env = _env(dev, tb)
    st = LR.host_state(env)
    out = env.rollout(dict(kind="linear", weight=W, bias=b, group=groups(), lookahead=K.spec(feature, D)), alert_mask=True)
    assert env.last_rollout_kernel == "k_rollout_linear" and env.check_status() == 0
    want, att = K.weather_rule_schedule(ct, feature, k, c, st)
    assert want.any() and att.sum() > want.sum() and not want.all()  # the rule fires, and the budget binds somewhere
    np.testing.assert_array_equal(out["alert_days"].cpu().numpy(), want)
    np.testing.assert_array_equal(out["attempt_days"].cpu().numpy(), att)
    env.close()


# ------------------------------------------------------------------ 3: step equivalence
def _twin_case(dev, tb, pol, kind, kernel, gate=None):
    ct = tb.ct
    A, B = _env(dev, tb), _env(dev, tb)
    uni = _uniform(pol, B)
    g = None
    if gate is not None:
        mask = A.alert_gate(gate[0], gate[1])
        g = mask.cpu().numpy()
        assert g.any() and not g.all()
        pol = dict(pol, allowed_days=mask)
    out = A.rollout(pol, alert_mask=True)
    assert A.last_rollout_kernel == kernel
    acc = LR.twin_loop(B, ct, pol["lookahead"], logit_fn(pol), ct.T, kind, uniform=uni, gate=g)
    assert A.check_status() == 0 and out["done"].all()
    if g is not None:  # no alert and no attempt on a closed day
        assert not (out["alert_days"].cpu().numpy() & ~g).any() and not (out["attempt_days"].cpu().numpy() & ~g).any()
    _against_twin(A, out, acc, ~acc["tie"])
    A.close(), B.close()


@pytest.mark.parametrize("table,feature,D,sample", K.LINEAR_CASES)
def test_linear_rollout_equals_the_stepped_twin(dev, tabs, table, feature, D, sample):
    """On slot27 / ragged27 the returns are compared for every env that is no near-tie, not only for those whose
    coefficient column has no slot-27 coefficient: the reference is the twin's step(), which carries slot 27 and is
    itself held to fp64 there (tests/test_table_edges_gpu.py, tests/test_env_gpu.py)."""
    tb = tabs[table]
    _twin_case(dev, tb, K.linear(tb, feature, D, sample), "linear", "k_rollout_linear")


@pytest.mark.parametrize("table,feature,D,sample,net", K.MLP_CASES)
def test_mlp_rollout_equals_the_stepped_twin(dev, tabs, table, feature, D, sample, net):
    """all six <WIDTH, LAYERS> instantiations with the first layer's slot block mostly empty (n_obs = 5, 8) or full
    (28, 29), and D = 2, 4, 5, 8, 9: zero, one and two whole first-layer k-steps with and without a partial one.
    Returns on ragged27 as in the linear test."""
    tb = tabs[table]
    _twin_case(dev, tb, K.mlp(tb, feature, net, D, sample), "mlp", "k_rollout_mlp")


def test_all_six_mlp_instantiations_are_covered():
    assert {M.MATRIX[n][0] for *_, n in K.MLP_CASES} == {(w, l) for w in (16, 32, 64) for l in (1, 2)}
    assert {D for _, _, D, _, _ in K.MLP_CASES} >= {2, 4, 5, 8, 9}


# ------------------------------------------------------------------ 4: with a gate
@pytest.mark.parametrize("kind,table,feature,D,gate_feature,net", K.GATE_CASES)
def test_gate_and_lookahead_equal_the_gated_twin(dev, tabs, kind, table, feature, D, gate_feature, net):
    tb = tabs[table]
    pol = K.linear(tb, feature, D) if kind == "linear" else K.mlp(tb, feature, net, D)
    _twin_case(dev, tb, pol, kind, "k_rollout_linear" if kind == "linear" else "k_rollout_mlp",
               gate=(gate_feature, K.gate_threshold(tb.ct, gate_feature)))


# ------------------------------------------------------------------ 5: chunking
@pytest.mark.parametrize("kind,table,D", [("mlp", "n8", 5), ("linear", "permuted_ragged", 9)])
@pytest.mark.parametrize("k", [3, -2])
def test_two_calls_equal_one(dev, tabs, kind, table, D, k):
    """k days then the rest equal one call, bit for bit: the state, the observation buffer, the bitmaps and the
    counters. k = -2: T - 2 days, so the second call starts inside the last D days."""
    tb = tabs[table]
    ct = tb.ct
    k = k if k > 0 else ct.T + k
    pol = K.linear(tb, "heat_qi", D, sample=True) if kind == "linear" else K.mlp(tb, "heat_qi", "tanh29x9", D, sample=True)
    A, B = _env(dev, tb), _env(dev, tb)
    whole = A.rollout(pol, alert_mask=True)
    first = B.rollout(pol, n_steps=k, alert_mask=True)
    second = B.rollout(pol, alert_mask=True)
    _same_env(A, B)
    for key in ("alerts", "attempts_over_budget"):
        assert torch.equal(whole[key], first[key] + second[key]), key
    for key in ("alert_days", "attempt_days"):
        assert torch.equal(whole[key], first[key] | second[key]), key
    assert torch.equal(whole["final_return"], second["final_return"]) and second["done"].all()
    assert whole["alerts"].sum() > 0 and A.check_status() == 0 and B.check_status() == 0
    A.close(), B.close()


# ------------------------------------------------------------------ 6: zero lookahead columns change no bit
@pytest.mark.parametrize("kind,table,D", [("linear", "n8", 4), ("mlp", "narrow", 8)])
def test_zero_lookahead_columns_give_the_bits_of_the_call_without_the_key(dev, tabs, kind, table, D):
    tb = tabs[table]
    ct = tb.ct
    full = K.linear(tb, "heat_qi", D, sample=True) if kind == "linear" else K.mlp(tb, "heat_qi", "relu40x64", D, sample=True)
    pol = K.zeroed(full, ct)
    A, B = _env(dev, tb), _env(dev, tb)
    oa = A.rollout(pol, n_steps=17, alert_mask=True)
    ob = B.rollout(K.without(pol, ct), n_steps=17, alert_mask=True)
    _same_outputs(oa, ob)
    _same_env(A, B)
    oa, ob = A.rollout(pol, alert_mask=True), B.rollout(K.without(pol, ct), alert_mask=True)
    _same_outputs(oa, ob)
    _same_env(A, B)
    assert oa["alerts"].sum() > 0
    A.close(), B.close()


# ------------------------------------------------------------------ 7: gradients, linear
def _grad(out):
    g = out["policy_gradient"]
    return np.concatenate([g["weight"].double().cpu().numpy(), g["bias"].double().cpu().numpy()[:, None]], axis=1)


def _within(got, ref, what):
    """got, and the restatement's weight / bias / bound, in the order: the n_obs observation COLUMNS, the D lookahead
    inputs k = 1..D, the bias (the bound is that of the restatement, unchanged)"""
    want = np.concatenate([ref["weight"], ref["bias"][:, None]], axis=1)
    diff = np.abs(got - want)
    ratio = float(np.where(ref["bound"] > 0, diff / np.where(ref["bound"] > 0, ref["bound"], 1.0), 0.0).max())
    print(f"{what}: max |g - g_ref| / bound = {ratio:.3e}   (max |g_ref| = {np.abs(want).max():.3e})")
    assert np.isfinite(got).all() and (diff <= ref["bound"]).all(), (what, ratio)


@pytest.mark.parametrize("table,feature,D", K.GRADIENT_CASES)
def test_policy_gradient_matches_the_restatement(dev, tabs, table, feature, D):
    """both baselines against policy_gradient_fp64 on the rows cat(obs, f) of the stepped twin, whose columns are the
    observation columns in the layout's own order (not slot order) and then k = 1..D; beta from a third twin stepped
    with no alerts"""
    tb = tabs[table]
    ct = tb.ct
    pol = K.linear(tb, feature, D, sample=True)
    A1, A2, B, Z = (_env(dev, tb) for _ in range(4))
    uni = _uniform(pol, B)
    got = {"none": A1.rollout(pol, policy_gradient="none"), "no_alert": A2.rollout(pol, policy_gradient="no_alert")}
    assert tuple(got["none"]["policy_gradient"]["weight"].shape) == (G, ct.n_obs + D)
    acc = LR.twin_loop(B, ct, pol["lookahead"], logit_fn(pol), ct.T, "linear", uniform=uni)
    assert not acc["tie"].any(), acc["tie"].sum()  # tests/test_lookahead_layouts_cpu.py holds this without a GPU
    tr = acc["traj"]
    beta = np.zeros_like(tr["reward"])
    for s in range(ct.T):
        beta[s] = Z.step(torch.zeros(N, dtype=torch.int32, device=dev))[1].cpu().numpy()
    for bl in ("none", "no_alert"):
        ref = policy_gradient_fp64(tr["x"], tr["action"], tr["valid"], np.zeros_like(tr["valid"]), tr["reward"],
                                   beta if bl == "no_alert" else None, pol["weight"], pol["bias"][:G], pol["group"], G)
        assert np.abs(ref["weight"][:, ct.n_obs:]).min() > 0  # every lookahead column carries a gradient
        _within(_grad(got[bl]), ref, f"{table} {feature} D={D} {bl}")
    assert A1.check_status() == 0 and A2.check_status() == 0
    for e in (A1, A2, B, Z):
        e.close()


@pytest.mark.parametrize("table,feature,D", K.IMITATION_CASES)
def test_imitation_gradient_along_a_bernoulli_schedule(dev, tabs, table, feature, D):
    tb = tabs[table]
    ct = tb.ct
    pol = K.linear(tb, feature, D)
    A, B = _env(dev, tb), _env(dev, tb)
    sched = K.imitation_schedule(ct)
    out = A.imitation_gradient(pol, torch.as_tensor(sched, device=dev))
    assert tuple(out["policy_gradient"]["weight"].shape) == (G, ct.n_obs + D)
    acc = LR.twin_loop(B, ct, pol["lookahead"], logit_fn(pol), ct.T, "linear", schedule=sched)
    tr = acc["traj"]
    ref = imitation_linear_fp64(tr["x"], tr["action"], tr["valid"], np.zeros_like(tr["valid"]), None, pol["weight"],
                                pol["bias"], pol["group"], G)
    np.testing.assert_array_equal(out["days"].cpu().numpy(), ref["days"])
    assert (np.abs(out["log_likelihood"].double().cpu().numpy() - ref["ll"]) <= ref["ll_bound"]).all()
    _within(_grad(out), ref, f"imitation {table} {feature} D={D}")
    # the lookahead columns carry a gradient, but for an input that is 0 on every row (weekend: f_7 = 0 on all days)
    live = (tr["x"][:, :, ct.n_obs:] != 0).any(axis=(0, 1))
    assert live.sum() >= D - 1 and ((ref["weight"][:, ct.n_obs:] != 0) == live[None, :]).all()
    assert A.check_status() == 0
    A.close(), B.close()


def _probe_env(dev, tb, X):
    """n8's schema on a hand-made feature table, every env with a budget of 0: no alert is ever issued, so the four
    run-time columns stay 0 and an observation row holds what X holds and nothing else"""
    tup = K.host_tuples(tb)
    ep = {k: tup[k] for k in ("county_w", "year_i", "coef_col", "sample")}
    ep["budget"] = np.zeros(N, np.int64)
    return _env(dev, tb, ct=dataclasses.replace(tb.ct, X=X), options={"episodes": ep})


def _one_hot(out, ref, col, n_cols, what):
    """exactly one input column has a nonzero fp64 gradient, and it is the one that comes back nonzero"""
    got = out["policy_gradient"]["weight"].double().cpu().numpy()
    assert got.shape == (G, n_cols)
    others = np.delete(np.arange(n_cols), col)
    assert (ref["weight"][:, col] != 0).all() and not ref["weight"][:, others].any(), what
    assert (got[:, col] != 0).all() and not got[:, others].any(), (what, np.nonzero(got.any(axis=0))[0])
    _within(_grad(out), ref, what)


def test_gradient_rows_are_observation_columns_then_bias_then_k(dev, tabs):
    """One-hot probes of the output order of the linear gradient on n8 (hi_max: column 0 on slot 3; heat_qi: column 1 on
    slot 0; dos: column 2 on slot 1; alerts_2wks: column 4 on slot 2), along a Bernoulli schedule with imitation_gradient.
    (a) X is 1 in the slot of one table-sourced column and 0 elsewhere, the lookahead reads another (all-zero) column:
        gradient column j < n_obs must be the only nonzero one for observation column j -- not slot j.
    (b) X is 0 but for a pulse h(d*) = 1 on one day in the lookahead feature's slot; the env is stepped to day t0 and one
        day is scored (n_steps = 1): the held row is day r = t0 - 1, so f_k = 1 exactly for k = d* - r and every other
        input is 0: gradient column n_obs + k - 1 must be the only nonzero one, for every k = 1..D."""
    tb = tabs["n8"]
    ct = tb.ct
    D = 5
    assert [ct.obs_slot[ct.feature_names.index(f)] for f in ("hi_max", "heat_qi", "dos", "alerts_2wks")] == [3, 0, 1, 2]
    sched = K.imitation_schedule(ct)
    sched_t = torch.as_tensor(sched, device=dev)
    rows = np.arange(N)
    for name, other in (("hi_max", "heat_qi"), ("heat_qi", "dos"), ("dos", "hi_max"), ("alerts_2wks", "hi_max")):
        j = ct.feature_names.index(name)
        X = np.zeros_like(np.asarray(ct.X))
        X[:, :, ct.obs_slot[j]] = 1.0
        ct2 = dataclasses.replace(ct, X=X)
        pol = K.linear(tb, other, D)
        env = _probe_env(dev, tb, X)
        st = LR.host_state(env)
        out = env.imitation_gradient(pol, sched_t)
        x = np.zeros((ct.T, N, ct.n_obs + D), np.float32)
        x[:, :, j] = 1.0
        np.testing.assert_array_equal(env._obs.cpu().numpy(), x[0, :, :ct.n_obs])
        assert not LR.inputs(ct2, other, D, st).any()
        valid = np.arange(ct.T)[:, None] < st["n_days"][None, :]
        ref = imitation_linear_fp64(x, sched.T & valid, valid, np.zeros_like(valid), None, pol["weight"], pol["bias"],
                                    pol["group"], G)
        _one_hot(out, ref, j, ct.n_obs + D, f"observation column {name}")
        env.close()
    d_star = 6
    X = np.zeros_like(np.asarray(ct.X))
    X[d_star, :, ct.obs_slot[ct.feature_names.index("hi_max")]] = 1.0
    ct2 = dataclasses.replace(ct, X=X)
    pol = K.linear(tb, "hi_max", D)
    env = _probe_env(dev, tb, X)
    seen = []
    for t0 in range(1, d_star + 1):
        env.step(torch.zeros(N, dtype=torch.int32, device=dev))
        st = LR.host_state(env)
        assert (st["t"] == t0).all()
        k = d_star - (t0 - 1)
        if k > D:
            continue
        out = env.imitation_gradient(pol, sched_t, n_steps=1)
        x = np.concatenate([env._obs.cpu().numpy(), LR.inputs(ct2, "hi_max", D, st)], axis=1)[None]
        want = np.zeros((1, N, ct.n_obs + D), np.float32)
        want[0, :, ct.n_obs + k - 1] = 1.0
        np.testing.assert_array_equal(x, want)
        valid = np.ones((1, N), bool)
        ref = imitation_linear_fp64(x, sched[rows, t0][None], valid, np.zeros_like(valid), None, pol["weight"],
                                    pol["bias"], pol["group"], G)
        _one_hot(out, ref, ct.n_obs + k - 1, ct.n_obs + D, f"lookahead input k={k}")
        seen.append(k)
    assert seen == [5, 4, 3, 2, 1]
    assert env.check_status() == 0
    env.close()


def test_gradients_with_zero_lookahead_weights_keep_the_other_columns_bits(dev, tabs):
    tb = tabs["n8"]
    ct = tb.ct
    D = 4
    pol = K.zeroed(K.linear(tb, "hi_max", D, sample=True), ct)
    for bl in ("none", "no_alert"):  # whole episodes: the gradient is that of the episodes the call finishes
        A, B = _env(dev, tb), _env(dev, tb)
        ga = A.rollout(pol, policy_gradient=bl)["policy_gradient"]
        gb = B.rollout(K.without(pol, ct), policy_gradient=bl)["policy_gradient"]
        assert torch.equal(ga["weight"][:, :ct.n_obs], gb["weight"]) and torch.equal(ga["bias"], gb["bias"]), bl
        assert gb["weight"].abs().sum() > 0 and ga["weight"][:, ct.n_obs:].abs().sum() > 0
        _same_env(A, B)
        A.close(), B.close()
    E1, E2 = _env(dev, tb), _env(dev, tb)
    days = torch.as_tensor(K.imitation_schedule(ct), device=dev)
    ia = E1.imitation_gradient(pol, days)
    ib = E2.imitation_gradient(K.without(pol, ct), days)
    assert torch.equal(ia["policy_gradient"]["weight"][:, :ct.n_obs], ib["policy_gradient"]["weight"])
    assert torch.equal(ia["policy_gradient"]["bias"], ib["policy_gradient"]["bias"])
    assert torch.equal(ia["log_likelihood"], ib["log_likelihood"]) and torch.equal(ia["days"], ib["days"])
    assert ia["policy_gradient"]["weight"][:, ct.n_obs:].abs().sum() > 0
    E1.close(), E2.close()
