"""policy["lookahead"] with "error" on the GPU: the NOISE forms of k_rollout_linear, k_rollout_mlp,
k_policy_gradient_linear and k_imitation_linear, and k_lookahead_features, against the restatement
(tests/forecast_error_restatement.py). The batch, tables and policies are tests/test_lookahead_gpu.py's (N = 193 envs,
G = 3, the mini and ragged tables); tests/test_forecast_error_cpu.py shows on the host that no case meets a near-tie, so
no env is set aside in any comparison here."""
import numpy as np
import pytest
import torch

import forecast_error_cases as FC
import forecast_error_restatement as FR
import lookahead_cases as C
import lookahead_restatement as LR
from forecast_error_cases import FEATURE, G, GID0, N, SEED
from imitation_restatement import imitation_linear_fp64
from policy_gradient_restatement import policy_gradient_fp64
from weather2alert_amd import HeatAlertVecEnv

pytestmark = pytest.mark.gpu

RETURN_RTOL, RETURN_ATOL = 2e-6, 2e-5  # as tests/test_lookahead_gpu.py
INT_STATE = ("t", "used", "streak", "last_actual", "at_budget", "hist14", "finished")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def TB():
    return {k: (ct, cfg["seed"], cfg["opts"]) for k, (ct, cfg, _) in C.make_tables().items()}


def _env(dev, tb, n=N, gid0=GID0, **kw):
    ct, seed, opts = tb
    env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", env_gid0=gid0, similar_climate_counties=True, **kw)
    env.reset(seed=seed, options=dict(opts))
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


def _against_twin(A, out, acc):
    assert not acc["tie"].any(), acc["tie"].sum()  # shown on the host alone by the CPU file
    assert acc["alerts"].sum() > 0 and (~acc["days"]).any()
    np.testing.assert_array_equal(out["alerts"].cpu().numpy(), acc["alerts"])
    np.testing.assert_array_equal(out["attempts_over_budget"].cpu().numpy(), acc["over"])
    np.testing.assert_array_equal(out["alert_days"].cpu().numpy(), acc["days"])
    np.testing.assert_array_equal(out["attempt_days"].cpu().numpy(), acc["att"])
    np.testing.assert_allclose(out["return"].cpu().numpy(), acc["ret"], rtol=RETURN_RTOL, atol=RETURN_ATOL)
    sa = LR.host_state(A)
    for k in INT_STATE:
        np.testing.assert_array_equal(sa[k], acc["state"][k], err_msg=k)
    np.testing.assert_array_equal(A._obs.cpu().numpy(), acc["obs"])


# ------------------------------------------------------------------ 1: lookahead_features(spec), bit for bit
@pytest.mark.parametrize("table", ["mini", "ragged"])
def test_noisy_features_equal_the_restatement_bit_for_bit(dev, TB, table):
    ct = TB[table][0]
    env = _env(dev, TB[table])
    shift = 50
    other = _env(dev, TB[table], n=N - shift, gid0=GID0 + shift)  # the same global ids under another env_gid0
    sa, so = LR.host_state(env), LR.host_state(other)
    for k in ("county_w", "year_i", "n_days"):  # the device reset draws by global id: the same episodes
        np.testing.assert_array_equal(sa[k][shift:], so[k])
    if table == "ragged":
        assert len(np.unique(sa["n_days"])) > 3

    def check(e=env, gid0=GID0):
        st = LR.host_state(e)
        for D in FC.FEATURE_DAYS:
            for row in (True, False):
                spec = FC.spec(D, row)
                f = e.lookahead_features(spec)
                assert f.dtype == torch.float32 and tuple(f.shape) == (e.num_envs, D)
                want = FR.inputs(ct, spec, st, gid0)
                np.testing.assert_array_equal(f.cpu().numpy().view(np.uint32), want.view(np.uint32))
                clean = e.lookahead_features(FR.clean(spec)).cpu().numpy()
                mae = FR.error_row(spec["error"], D)[None, :]
                ulp = np.spacing(np.maximum(np.abs(want), np.abs(clean)))
                assert (np.abs(want.astype(np.float64) - clean) <= mae + ulp).all()
        return want

    check()
    check(other, GID0 + shift)
    a = env.lookahead_features(FC.spec(10)).cpu().numpy()
    b = other.lookahead_features(FC.spec(10)).cpu().numpy()
    np.testing.assert_array_equal(a[shift:].view(np.uint32), b.view(np.uint32))
    assert (a != env.lookahead_features(FR.clean(FC.spec(10))).cpu().numpy()).mean() > 0.5
    env.rollout(FC.linear(ct, 3), n_steps=17)
    check()
    env.rollout(FC.linear(ct, 3))  # every env on its last day: +0 everywhere but the held row's own leads
    last = check()
    st = LR.host_state(env)
    assert (st["t"] == st["n_days"] - 1).all()
    assert (last[:, 1:].view(np.uint32) == 0).all()  # r = n_days - 2: lead 1 is the last day, every later lead is past it
    env.close(), other.close()


# ------------------------------------------------------------------ 2, 3: step equivalence
@pytest.mark.parametrize("table,D,sample,row", FC.LINEAR_CASES)
def test_linear_rollout_equals_the_stepped_twin(dev, TB, table, D, sample, row):
    ct = TB[table][0]
    A, B = _env(dev, TB[table]), _env(dev, TB[table])
    pol = FC.linear(ct, D, sample, row, key=("linear", table, D))
    uni = LR.policy_uniform(SEED, GID0, LR.host_state(B)) if sample else None
    out = A.rollout(pol, alert_mask=True)
    assert A.last_rollout_kernel == "k_rollout_linear" and A.check_status() == 0 and out["done"].all()
    acc = FR.twin_loop(B, ct, pol["lookahead"], GID0, C.logit_fn(pol), ct.T, "linear", uniform=uni)
    _against_twin(A, out, acc)
    # the twin's policy can as well read its inputs from lookahead_features(): the first decision's rows agree
    C0 = _env(dev, TB[table])
    np.testing.assert_array_equal(C0.lookahead_features(pol["lookahead"]).cpu().numpy(), acc["traj"]["x"][0][:, ct.n_obs:])
    for e in (A, B, C0):
        e.close()


@pytest.mark.parametrize("name,D,sample", FC.MLP_CASES)
def test_mlp_rollout_equals_the_stepped_twin(dev, TB, name, D, sample):
    """all six <WIDTH, LAYERS> instantiations; D = 4, 5, 10: the k-step boundaries of the first layer's extra steps"""
    table = C.mlp_table(D)
    ct = TB[table][0]
    A, B = _env(dev, TB[table]), _env(dev, TB[table])
    pol = FC.mlp(ct, name, D, sample, key=("mlp", name, D))
    uni = LR.policy_uniform(SEED, GID0, LR.host_state(B)) if sample else None
    out = A.rollout(pol, alert_mask=True)
    assert A.last_rollout_kernel == "k_rollout_mlp" and A.check_status() == 0 and out["done"].all()
    acc = FR.twin_loop(B, ct, pol["lookahead"], GID0, C.logit_fn(pol), ct.T, "mlp", uniform=uni)
    _against_twin(A, out, acc)
    A.close(), B.close()


# ------------------------------------------------------------------ 4: a zero error changes no bit
@pytest.mark.parametrize("kind,D,zero", [("linear", 3, 0.0), ("linear", 10, [0.0] * 10), ("mlp", 4, [0, 0, 0, 0]),
                                         ("mlp", 10, 0)])
def test_zero_error_gives_the_bits_of_the_call_without_the_key(dev, TB, kind, D, zero):
    ct = TB["ragged"][0]
    base = C.linear(ct, D, sample=True) if kind == "linear" else C.mlp(ct, "relu40x64", D, sample=True)
    pol = FC.with_error(base, zero, error_seed=5)
    A, B = _env(dev, TB["ragged"]), _env(dev, TB["ragged"])
    for steps in (40, None):
        oa, ob = A.rollout(pol, n_steps=steps, alert_mask=True), B.rollout(base, n_steps=steps, alert_mask=True)
        _same_outputs(oa, ob)
        _same_env(A, B)
    A.close(), B.close()


def test_zero_error_gives_the_gradients_bits(dev, TB):
    ct = TB["ragged"][0]
    base = C.linear(ct, 10, sample=True)
    pol = FC.with_error(base, [0.0] * 10)
    A, B = _env(dev, TB["ragged"]), _env(dev, TB["ragged"])
    sched = A.hindsight_optimum()["alert_days"]
    ia, ib = A.imitation_gradient(pol, sched), B.imitation_gradient(base, sched)
    for k in ("weight", "bias"):
        assert torch.equal(ia["policy_gradient"][k], ib["policy_gradient"][k]), k
    assert torch.equal(ia["log_likelihood"], ib["log_likelihood"]) and torch.equal(ia["days"], ib["days"])
    for bl in ("none", "no_alert"):
        ga = A.rollout(pol, n_steps=60, policy_gradient=bl)
        gb = B.rollout(base, n_steps=60, policy_gradient=bl)
        for k in ("weight", "bias"):
            assert torch.equal(ga["policy_gradient"][k], gb["policy_gradient"][k]), (bl, k)
        assert torch.equal(ga["return"], gb["return"])
        _same_env(A, B)
    A.close(), B.close()


# ------------------------------------------------------------------ 5: chunking and the visiting order
@pytest.mark.parametrize("kind,D,k", [("linear", 3, 1), ("linear", 10, -4), ("mlp", 10, 1), ("mlp", 4, -2)])
def test_two_calls_equal_one(dev, TB, kind, D, k):
    ct = TB["mini"][0]
    k = k if k > 0 else ct.T + k
    pol = FC.linear(ct, D, sample=True) if kind == "linear" else FC.mlp(ct, "tanh29x9", D, sample=True)
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


@pytest.mark.parametrize("kind", ["linear", "mlp"])
def test_the_visiting_order_changes_no_result(dev, TB, kind):
    ct = TB["ragged"][0]
    pol = FC.linear(ct, 5, sample=True) if kind == "linear" else FC.mlp(ct, "tanh17", 5, sample=True)
    # linear: the handle's feature-row order against the identity; mlp: the group-major order against a fixed
    # non-identity permutation of the policy's own
    A, B = _env(dev, TB["ragged"]), _env(dev, TB["ragged"], rollout_order=(kind == "mlp"))
    polb = dict(pol, order=np.random.default_rng(2).permutation(N)) if kind == "mlp" else pol
    oa, ob = A.rollout(pol, alert_mask=True), B.rollout(polb, alert_mask=True)
    _same_outputs(oa, ob)
    _same_env(A, B)
    A.close(), B.close()


# ------------------------------------------------------------------ 6: seeds
def test_error_seed_moves_the_features_and_the_policy_seed_does_not(dev, TB):
    ct = TB["mini"][0]
    A, B = _env(dev, TB["mini"]), _env(dev, TB["mini"])
    pol = FC.linear(ct, 5, sample=True)
    o1, o2 = A.rollout(pol, n_steps=30, alert_mask=True), B.rollout(pol, n_steps=30, alert_mask=True)
    _same_outputs(o1, o2)
    _same_env(A, B)
    spec = pol["lookahead"]
    f = A.lookahead_features(spec)
    assert torch.equal(f, A.lookahead_features(spec)) and torch.equal(f, B.lookahead_features(spec))
    assert (f != A.lookahead_features(dict(spec, error_seed=spec["error_seed"] + 1))).float().mean() > 0.9
    # another policy seed: other Bernoulli draws, so other states -- but the inputs of a GIVEN state do not move
    C1, C2 = _env(dev, TB["mini"]), _env(dev, TB["mini"])
    sched = o1["alert_days"]
    g1 = C1.imitation_gradient(pol, sched)
    g2 = C2.imitation_gradient(dict(pol, seed=SEED + 1), sched)
    assert torch.equal(g1["log_likelihood"], g2["log_likelihood"])
    g3 = C2.imitation_gradient(FC.with_error(pol, spec["error"], error_seed=spec["error_seed"] + 1), sched)
    assert not torch.equal(g1["log_likelihood"], g3["log_likelihood"])
    for e in (A, B, C1, C2):
        e.close()


# ------------------------------------------------------------------ 7: with a gate
@pytest.mark.parametrize("kind,D", FC.GATE_CASES)
def test_gate_and_error_equal_the_gated_twin(dev, TB, kind, D):
    ct = TB["ragged"][0]
    A, B = _env(dev, TB["ragged"]), _env(dev, TB["ragged"])
    gate = A.alert_gate(FEATURE, C.GATE_THRESHOLD)
    g = gate.cpu().numpy()
    assert g.any() and not g.all()
    pol = FC.linear(ct, D, key=("gate", kind, D)) if kind == "linear" else FC.mlp(ct, FC.GATE_NET, D, key=("gate", kind, D))
    out = A.rollout(dict(pol, allowed_days=gate), alert_mask=True)
    acc = FR.twin_loop(B, ct, pol["lookahead"], GID0, C.logit_fn(pol), ct.T, kind, gate=g)
    assert not (out["alert_days"].cpu().numpy() & ~g).any() and not (out["attempt_days"].cpu().numpy() & ~g).any()
    _against_twin(A, out, acc)
    A.close(), B.close()


# ------------------------------------------------------------------ 8: gradients, linear
def _grad(out):
    g = out["policy_gradient"]
    return np.concatenate([g["weight"].double().cpu().numpy(), g["bias"].double().cpu().numpy()[:, None]], axis=1)


def _within(got, ref, what):
    want = np.concatenate([ref["weight"], ref["bias"][:, None]], axis=1)
    diff = np.abs(got - want)
    ratio = float(np.where(ref["bound"] > 0, diff / np.where(ref["bound"] > 0, ref["bound"], 1.0), 0.0).max())
    print(f"{what}: max |g - g_ref| / bound = {ratio:.3e}   (max |g_ref| = {np.abs(want).max():.3e})")
    assert np.isfinite(got).all() and (diff <= ref["bound"]).all(), (what, ratio)


@pytest.mark.parametrize("table,D", FC.GRADIENT_CASES)
def test_policy_gradient_matches_the_restatement(dev, TB, table, D):
    """as tests/test_lookahead_gpu.py: both baselines against policy_gradient_fp64 on the rows cat(obs, noisy f) of the
    stepped twin, with that file's bounds"""
    ct = TB[table][0]
    pol = FC.linear(ct, D, sample=True, key=("gradient", table, D))
    A1, A2, B, Z = (_env(dev, TB[table]) for _ in range(4))
    st0 = LR.host_state(B)
    got = {"none": A1.rollout(pol, policy_gradient="none"), "no_alert": A2.rollout(pol, policy_gradient="no_alert")}
    assert tuple(got["none"]["policy_gradient"]["weight"].shape) == (G, ct.n_obs + D)
    acc = FR.twin_loop(B, ct, pol["lookahead"], GID0, C.logit_fn(pol), ct.T, "linear",
                       uniform=LR.policy_uniform(SEED, GID0, st0))
    assert not acc["tie"].any(), acc["tie"].sum()
    np.testing.assert_array_equal(got["none"]["alerts"].cpu().numpy(), acc["alerts"])  # the rollout of the same call
    tr = acc["traj"]
    beta = np.zeros_like(tr["reward"])
    for s in range(ct.T):
        beta[s] = Z.step(torch.zeros(N, dtype=torch.int32, device=dev))[1].cpu().numpy()
    for bl in ("none", "no_alert"):
        ref = policy_gradient_fp64(tr["x"], tr["action"], tr["valid"], np.zeros_like(tr["valid"]), tr["reward"],
                                   beta if bl == "no_alert" else None, pol["weight"], pol["bias"][:G], pol["group"], G)
        _within(_grad(got[bl]), ref, f"{table} D={D} {bl}")
    for e in (A1, A2, B, Z):
        e.close()


@pytest.mark.parametrize("table,D", FC.IMITATION_CASES)
def test_imitation_gradient_along_the_hindsight_optimum(dev, TB, table, D):
    ct = TB[table][0]
    pol = FC.linear(ct, D)
    A, B = _env(dev, TB[table]), _env(dev, TB[table])
    sched = A.hindsight_optimum()["alert_days"]
    out = A.imitation_gradient(pol, sched)
    again = A.imitation_gradient(pol, sched)
    for k in ("weight", "bias"):
        assert torch.equal(out["policy_gradient"][k], again["policy_gradient"][k])
    acc = FR.twin_loop(B, ct, pol["lookahead"], GID0, C.logit_fn(pol), ct.T, "linear", schedule=sched.cpu().numpy())
    tr = acc["traj"]
    ref = imitation_linear_fp64(tr["x"], tr["action"], tr["valid"], np.zeros_like(tr["valid"]), None, pol["weight"],
                                pol["bias"], pol["group"], G)
    np.testing.assert_array_equal(out["days"].cpu().numpy(), ref["days"])
    assert (np.abs(out["log_likelihood"].double().cpu().numpy() - ref["ll"]) <= ref["ll_bound"]).all()
    _within(_grad(out), ref, f"imitation {table} D={D}")
    clean = A.imitation_gradient(FC.without_error(pol), sched)
    assert not torch.equal(out["log_likelihood"], clean["log_likelihood"])  # the error reaches the logits
    A.close(), B.close()


def test_imitation_along_a_rollouts_schedule_reproduces_its_decisions(dev, TB):
    """a deterministic rollout's alert_days are its own greedy choices: scored along them, every day the policy was free
    on has the sign of its logit on the schedule's side, so log-likelihood > days * log(1/2) env by env -- which holds
    only if imitation_gradient() sees the noisy inputs the rollout acted on"""
    ct = TB["mini"][0]
    pol = FC.linear(ct, 10)
    A, B = _env(dev, TB["mini"]), _env(dev, TB["mini"])
    out = A.rollout(dict(pol, require_budget=True), alert_mask=True)
    im = B.imitation_gradient(dict(pol, require_budget=True), out["attempt_days"])
    ll, days = im["log_likelihood"].double().cpu().numpy(), im["days"].cpu().numpy()
    assert (days > 0).all() and (ll > days * np.log(0.5)).all()
    other = B.imitation_gradient(dict(FC.with_error(pol, pol["lookahead"]["error"], error_seed=99), require_budget=True),
                                 out["attempt_days"])
    assert (other["log_likelihood"].double().cpu().numpy() < ll).mean() > 0.5  # another noise: another policy's choices
    A.close(), B.close()


# ------------------------------------------------------------------ 9: the refusals, on the GPU build
def test_refusals_on_a_live_env(dev, TB):
    ct = TB["mini"][0]
    env = _env(dev, TB["mini"])
    lin, mlp = FC.linear(ct, 3, sample=True), FC.mlp(ct, "tanh7x13", 3, sample=True)
    days = torch.zeros((N, ct.T), dtype=torch.bool, device=dev)
    adv = torch.zeros((ct.T, N), device=dev)
    before = {k: v.clone() for k, v in env.state().items()}
    obs = env._obs.clone()
    with pytest.raises(ValueError, match="lookahead"):
        env.rollout(lin, record=True)
    with pytest.raises(ValueError, match="lookahead"):
        env.rollout(mlp, policy_gradient="none")
    with pytest.raises(ValueError, match="lookahead"):
        env.imitation_gradient(mlp, days)
    with pytest.raises(ValueError, match="lookahead"):
        env.imitation_gradient(lin, days, labels=days)
    for pol in (lin, mlp):
        with pytest.raises(ValueError, match="lookahead"):
            env.surrogate_gradient(pol, days, adv)
        with pytest.raises(ValueError, match="lookahead"):
            env.fisher_vector_product(pol, days, {})
        with pytest.raises(ValueError, match="lookahead"):
            env.value_gradient(pol, days)
        with pytest.raises(ValueError, match="lookahead"):
            env.rollout(FC.with_error(pol, -0.5))
        with pytest.raises(ValueError, match="lookahead"):
            env.rollout(FC.with_error(pol, [0.1] * 4))
        with pytest.raises(ValueError, match="lookahead"):
            env.rollout(dict(pol, lookahead=dict(C.spec(3), error_seed=1)))
    with pytest.raises(ValueError, match="lookahead"):
        env.q_gradient(mlp, days)
    with pytest.raises(ValueError, match="lookahead"):
        env.policy_budget_curve(lin, 3)
    with pytest.raises(ValueError, match="lookahead"):
        env.lookahead_features(dict(C.spec(3), error=float("nan")))
    after = env.state()
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert torch.equal(obs, env._obs)
    env.close()
