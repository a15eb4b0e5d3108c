"""Alert gates on the GPU: alert_gate() (k_alert_gate) against a twin stepped through step(), and "allowed_days" in the
linear and mlp kinds' rollout(), rollout(policy_gradient=...), imitation_gradient(), surrogate_gradient() and in
hindsight_optimum() against the ungated calls, the stepped twin and tests/alert_gate_restatement.py. The inputs are
tests/alert_gate_restatement.py's make_case(): 257 envs (a partial wave), groups 0 and 2 of 3 (group 1 empty), per-env
thresholds, on the synthetic tables of the imitation tests and on tests/table_edges.py's ragged table."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alert_gate_restatement as G  # noqa: E402
import table_edges as E  # noqa: E402
import test_imitation_gpu as TI  # noqa: E402  (its twin walk and its checks against the bounds: the existing tolerances)
import test_surrogate_gpu as TS  # noqa: E402
from imitation_restatement import imitation_linear_fp64, imitation_mlp_fp64  # noqa: E402
from policy_gradient_restatement import policy_gradient_fp64  # noqa: E402
from surrogate_restatement import surrogate_linear_fp64, surrogate_mlp_fp64  # noqa: E402

KINDS = ("linear", "mlp")

pytestmark = pytest.mark.gpu

REWARD_TOL = 1e-5  # the suite's per-day bar (tests/test_trajectory_gpu.py:15, tests/test_env_gpu.py:19)
RETURN_RTOL, RETURN_ATOL = 2e-6, 2e-5  # tests/test_linear_policy_gpu.py:15 (as tests/test_env_gpu.py:23)
DAY_BAR = 1e-5  # tests/test_hindsight_gpu.py:22


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in ("synth", "ragged"):
        ct = G.make_tables(name)
        case = G.make_case(ct)
        case["allowed"] = G.check_case(ct, case)  # the issue's conditions, asserted on the test's own inputs
        out[name] = (ct, case)
    return out


def _make(dev, ct, case, **kw):
    from weather2alert_amd import HeatAlertVecEnv

    env = HeatAlertVecEnv(G.N_ENVS, tables=ct, device=dev, autoreset="disabled", **kw)
    env.reset(options={"episodes": case["ep"]})
    return env


def _policy(ct, case, sample, rb=False, seed=11, kind="linear"):
    rng = np.random.default_rng(3)
    if kind == "mlp":  # two hidden layers, 13 and 7 units (padded to 16), tanh, one block per group
        dims = [ct.n_obs, 13, 7, 1]
        layers = []
        for i in range(3):
            W = rng.standard_normal((G.N_GROUPS, dims[i + 1], dims[i])) * (1.5 / np.sqrt(dims[i]))
            if i == 0:
                W *= E._col_scale(ct)[None, None, :]
            layers.append((W.astype(np.float32), (rng.standard_normal((G.N_GROUPS, dims[i + 1])) * 0.5).astype(np.float32)))
        return dict(kind="mlp", layers=layers, activation="tanh", group=case["group"], sample=sample, seed=seed,
                    require_budget=rb)
    W = (rng.standard_normal((G.N_GROUPS, ct.n_obs)) * 0.4).astype(np.float32)
    W[:, ct.feature_names.index("remaining_budget")] *= 0.1
    b = (rng.standard_normal(G.N_GROUPS) * 0.5 + 0.3).astype(np.float32)
    return dict(kind="linear", weight=W, bias=b, group=case["group"], sample=sample, seed=seed, require_budget=rb)


def _twin_gate(env, col, tau, S):
    """obs[:, col] >= tau gathered from `env` stepped day by day with no alerts, every env on its own days: bool [N, T]"""
    n, T = env.num_envs, env.ct.T
    out = torch.zeros((n, T), dtype=torch.bool, device=env.device)
    rows = torch.arange(n, device=env.device)
    fin = env.state()["finished"].bool()
    tau_t = torch.as_tensor(tau, dtype=torch.float32, device=env.device)
    zero = torch.zeros(n, dtype=torch.int32, device=env.device)
    for _ in range(S):
        if bool(fin.all()):
            break
        t = env.state()["t"].long()
        live = ~fin
        out[rows[live], t[live]] = (env._obs[:, col] >= tau_t)[live]
        fin = fin | env.step(zero)[2].bool()
    return out


@pytest.mark.parametrize("name", ["synth", "ragged"])
def test_alert_gate_equals_stepped_twin(dev, cases, name):
    """Bit for bit, from reset and to the end; with n_steps < T from a mid-episode state with finished envs; and a
    scalar threshold."""
    ct, case = cases[name]
    col = ct.feature_names.index(G.FEATURE)
    A, B = _make(dev, ct, case), _make(dev, ct, case)
    got = A.alert_gate(G.FEATURE, torch.as_tensor(case["tau"]))
    assert got.dtype == torch.bool and got.shape == (G.N_ENVS, ct.T)
    np.testing.assert_array_equal(got.cpu().numpy(), case["allowed"])
    assert torch.equal(got, _twin_gate(B, col, case["tau"], ct.T))
    A.close()
    B.close()
    A, B = _make(dev, ct, case), _make(dev, ct, case)
    g = torch.Generator(device=dev).manual_seed(5)
    for _ in range(25):  # ragged: the short episodes finish
        a = (torch.rand(G.N_ENVS, generator=g, device=dev) < 0.3).to(torch.int32)
        A.step(a)
        B.step(a)
    st = A.state()
    assert name != "ragged" or (bool(st["finished"].any()) and not bool(st["finished"].all()))
    for tau in (torch.as_tensor(case["tau"]), 0.5):
        got = A.alert_gate(G.FEATURE, tau, n_steps=40)
        assert not bool(got[st["finished"].bool()].any()) and not bool(got[:, :24].any())
        sd = B.state_dict()
        want = _twin_gate(B, col, case["tau"] if torch.is_tensor(tau) else np.full(G.N_ENVS, tau, np.float32), 40)
        B.load_state_dict(sd)
        assert torch.equal(got, want)
    # (bit 4, W2A_ST_STEP_AFTER_DONE, is this test's own: the 25 step() calls above went on past the short episodes)
    assert torch.equal(A.state()["t"], st["t"]) and (A.check_status() & ~4) == 0
    with pytest.raises(ValueError, match="table-sourced"):
        A.alert_gate("remaining_budget", 0.5)
    with pytest.raises(ValueError):
        A.alert_gate(G.FEATURE, torch.zeros(3))
    A.close()
    B.close()


def test_alert_gate_with_the_obs_fix(dev, cases):
    """One handle with the Q6 fix: step() returns the next day's row, so day t is gated on table row t."""
    ct, case = cases["synth"]
    col = ct.feature_names.index(G.FEATURE)
    A, B = _make(dev, ct, case, fixes={"obs"}), _make(dev, ct, case, fixes={"obs"})
    got = A.alert_gate(G.FEATURE, torch.as_tensor(case["tau"]))
    np.testing.assert_array_equal(got.cpu().numpy(),
                                  G.gate_fp32(ct.X, ct.Y, case["slot"], case["start"], case["tau"], lag=False))
    assert torch.equal(got, _twin_gate(B, col, case["tau"], ct.T))
    assert not torch.equal(got, torch.as_tensor(case["allowed"], device=dev))
    A.close()
    B.close()


def _same(a, b, what):
    if isinstance(a, dict) and "valid" in a:  # a trajectory: entries where valid is False are unspecified
        v = a["valid"]
        assert torch.equal(v, b["valid"]) and set(a) == set(b), what
        for k in a:
            if k == "obs":
                assert torch.equal(a[k][:-1][v], b[k][:-1][v]) and torch.equal(a[k][-1], b[k][-1]), f"{what}.obs"
            else:
                assert torch.equal(a[k][v], b[k][v]), f"{what}.{k}"
    elif isinstance(a, dict):
        assert set(a) == set(b), what
        for k in a:
            _same(a[k], b[k], f"{what}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    elif torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        assert torch.equal(torch.nan_to_num(a.float(), nan=12345.0) if a.is_floating_point() else a,
                           torch.nan_to_num(b.float(), nan=12345.0) if b.is_floating_point() else b), what
    else:
        assert a == b, what


def _shifted(pol):
    """the policy with its output bias lowered by 0.2: the "old" policy of the surrogate's ratios"""
    if pol["kind"] == "linear":
        return dict(pol, bias=pol["bias"] - 0.2)
    (Wo, bo) = pol["layers"][-1]
    return dict(pol, layers=list(pol["layers"][:-1]) + [(Wo, bo - 0.2)])


def _grad_rows(pg):
    """the gradient's tensors, each with the group as its first axis"""
    return [pg["weight"], pg["bias"]] if "weight" in pg else [x for wb in pg["layers"] for x in wb]


def _calls(env, pol, case, ct, sample):
    """every call of the issue's section 2 on a fresh env, in a fixed order"""
    sched = torch.as_tensor(case["sched"], device=env.device)
    adv = torch.as_tensor(np.random.default_rng(2).standard_normal((ct.T, G.N_ENVS)).astype(np.float32), device=env.device)
    out = {}
    out["im"] = env.imitation_gradient(pol, sched)
    out["im_w"] = env.imitation_gradient(pol, sched, day_weight=adv.abs(), n_steps=50)
    lp0 = env.surrogate_gradient(_shifted(pol), sched, adv, log_prob=True)
    out["sg"] = env.surrogate_gradient(pol, sched, adv, old_log_prob=lp0["log_prob"], entropy_coef=0.01, log_prob=True)
    out["hs"] = env.hindsight_optimum(allowed_days=pol.get("allowed_days"))
    kw = dict(policy_gradient="no_alert") if sample else dict(record=True)
    out["roll"] = env.rollout(pol, n_steps=70, alert_mask=True, hindsight=True, posterior_returns=True, **kw)
    out["roll2"] = env.rollout(pol, alert_mask=True, record=True)
    out["state"] = env.state()
    out["obs"] = env._obs.clone()
    assert env.check_status() == 0
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sample", [False, True])
def test_all_ones_mask_gives_the_ungated_bits(dev, cases, sample, kind):
    """every call that takes the gate, sampled and greedy, every output including the trajectory and the state left"""
    ct, case = cases["synth"]
    pol = _policy(ct, case, sample, kind=kind)
    ones = torch.ones((G.N_ENVS, ct.T), dtype=torch.bool, device=dev)
    A, B = _make(dev, ct, case), _make(dev, ct, case)
    a = _calls(A, pol, case, ct, sample)
    b = _calls(B, dict(pol, allowed_days=ones), case, ct, sample)
    _same(a, b, "out")
    assert int(a["roll"]["alerts"].sum()) > 0 and int(a["roll"]["attempts_over_budget"].sum()) > 0
    A.close()
    B.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sample", [False, True])
def test_all_zero_mask(dev, cases, sample, kind):
    """returns and alerts of {"kind": "never"} on the same episodes; nothing over budget, no scored day, exactly zero
    gradients, log_prob 0"""
    ct, case = cases["ragged"]
    zeros = torch.zeros((G.N_ENVS, ct.T), dtype=torch.bool, device=dev)
    pol = dict(_policy(ct, case, sample, kind=kind), allowed_days=zeros)
    A, B = _make(dev, ct, case), _make(dev, ct, case)
    o = _calls(A, pol, case, ct, sample)
    never = B.rollout({"kind": "never"}, n_steps=70, alert_mask=True)
    for k in ("alerts", "attempts_over_budget", "alert_days", "attempt_days", "done"):
        assert torch.equal(o["roll"][k], never[k]), k
    torch.testing.assert_close(o["roll"]["return"], never["return"], rtol=RETURN_RTOL, atol=RETURN_ATOL)
    assert int(o["roll"]["alerts"].sum()) == 0 and int(o["roll"]["attempts_over_budget"].sum()) == 0
    assert int(o["roll2"]["trajectory"]["action"].sum()) == 0 and bool((o["roll2"]["trajectory"]["logit"] != 0).any())
    for k in ("im", "im_w", "sg"):
        assert int(o[k]["days"].abs().sum()) == 0, k
        for x in _grad_rows(o[k]["policy_gradient"]):  # groups 0 and 2 hold envs, group 1 none
            assert bool((x[[0, 2]] == 0).all()) and bool(torch.isnan(x[1]).all()), k
    assert bool((o["im"]["log_likelihood"] == 0).all())
    assert bool((o["sg"]["log_prob"] == 0).all()) and int(o["sg"]["clipped_days"].sum()) == 0
    for k in ("surrogate", "approx_kl", "entropy"):
        assert bool((o["sg"][k] == 0).all()), k
    if sample:
        for x in _grad_rows(o["roll"]["policy_gradient"]):
            assert bool((x[[0, 2]] == 0).all())
    assert int(o["hs"]["alerts"].sum()) == 0 and int(o["roll"]["hindsight_return"].ne(o["roll"]["return"]).sum()) == 0
    A.close()
    B.close()


def _replay(B, actions, S):
    """the twin stepped with actions [S, N] (every env on its own days): rewards [S, N] and the state it ends in"""
    n, dv = B.num_envs, B.device
    rew = torch.zeros((S, n), dtype=torch.float32, device=dv)
    fin = B.state()["finished"].bool()
    for s in range(S):
        if bool(fin.all()):
            break
        _, r, term, _, _ = B.step(torch.where(fin, 0, actions[s].to(torch.int32)))
        rew[s] = torch.where(fin, torch.zeros_like(r), r)
        fin = fin | term.bool()
    return rew, B.state()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,sample", [("synth", False), ("ragged", False), ("synth", True)])
def test_rollout_under_a_mixed_mask_against_the_twin(dev, cases, name, sample, kind):
    """Greedy: the twin's action is (logit > 0) & allowed from the recorded logits; integer outputs exact, returns within
    the bar of the rollout-vs-twin tests. Sampled: action == 0 wherever the bit is clear, and the recorded actions
    replayed through the twin reproduce reward and state. The draws do not move: on allowed days the sampled actions
    are those of u < sigmoid(logit) with the ungated call's uniforms."""
    ct, case = cases[name]
    allowed = torch.as_tensor(case["allowed"], device=dev)
    pol = dict(_policy(ct, case, sample, kind=kind), allowed_days=allowed)
    A, B = _make(dev, ct, case), _make(dev, ct, case)
    out = A.rollout(pol, alert_mask=True, record=True)
    assert A.check_status() == 0 and A.last_rollout_kernel == "k_rollout_" + kind
    tr = out["trajectory"]
    S = ct.T
    v = tr["valid"]
    t0 = torch.zeros(G.N_ENVS, dtype=torch.int64, device=dev)
    open_ = torch.as_tensor(G.by_call_day(case["allowed"], t0.cpu().numpy(), S), device=dev)
    act = tr["action"].bool()
    assert not bool((act & ~open_ & v).any())                       # action == 0 wherever the bit is clear
    assert bool(((tr["logit"] > 0) & ~open_ & v).any())             # ... although the policy asked
    if not sample:
        assert torch.equal(act & v, (tr["logit"] > 0) & open_ & v)  # the twin's action, from the recorded logits
    rew, stB = _replay(B, act & v, S)
    torch.testing.assert_close(tr["reward"][v], rew[v], rtol=REWARD_TOL, atol=REWARD_TOL)
    torch.testing.assert_close(out["return"], rew.sum(0), rtol=RETURN_RTOL, atol=RETURN_ATOL)
    stA = A.state()
    # the twin's step() goes on shifting the 14-day window, the streak and the last action of the envs of a ragged batch
    # that finished earlier: those fields are compared on the envs with the longest episode
    longest = torch.as_tensor(case["start"]["n_days"] == case["start"]["n_days"].max(), device=dev)
    for k in ("t", "used", "streak", "hist14", "finished", "last_actual", "at_budget"):
        if k in stA:
            m = longest if k in ("hist14", "streak", "last_actual", "at_budget") else slice(None)
            assert torch.equal(stA[k][m], stB[k][m]), k
    # the integer bookkeeping of the recorded actions, restated
    walk = G.gated_walk(_by_day(act & v, ct.T), case["allowed"], case["start"]["t"], case["start"]["used"],
                        case["start"]["budget"], case["start"]["n_days"], case["start"]["finished"], S)
    np.testing.assert_array_equal(out["alerts"].cpu().numpy(), walk["alert"].sum(0))
    np.testing.assert_array_equal(out["attempts_over_budget"].cpu().numpy(), walk["over"].sum(0))
    np.testing.assert_array_equal(out["alert_days"].cpu().numpy(), _by_day(torch.as_tensor(walk["alert"]), ct.T))
    np.testing.assert_array_equal(out["attempt_days"].cpu().numpy(), _by_day(torch.as_tensor(walk["attempt"]), ct.T))
    assert not bool((out["alert_days"] & ~allowed).any()) and int(out["attempts_over_budget"].sum()) > 0
    assert torch.equal(A._obs, B._obs)
    A.close()
    B.close()


def _by_day(x, T):
    """[S, N] by call-day from day 0 -> numpy bool [N, T]"""
    x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    out = np.zeros((x.shape[1], T), bool)
    out[:, : x.shape[0]] = x.T[:, :T]
    return out


def test_sampled_draws_do_not_move(dev, cases):
    """Two gated sampled rollouts under different masks agree with the ungated one on every day until their schedules
    first differ -- and on the logit-vs-uniform outcome of every later allowed day whose logit is the same bits."""
    ct, case = cases["synth"]
    pol = _policy(ct, case, True)
    allowed = torch.as_tensor(case["allowed"], device=dev)
    A, B = _make(dev, ct, case), _make(dev, ct, case)
    a = A.rollout(pol, record=True)["trajectory"]
    b = B.rollout(dict(pol, allowed_days=allowed), record=True)["trajectory"]
    open_ = torch.as_tensor(G.by_call_day(case["allowed"], np.zeros(G.N_ENVS, np.int64), ct.T), device=dev)
    same = (a["logit"] == b["logit"]) & a["valid"] & b["valid"] & open_
    assert int(same.sum()) > 1000
    assert torch.equal(a["action"][same], b["action"][same])  # same logit, same day, same uniform: same draw
    A.close()
    B.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rb", [False, True])
def test_gradients_equal_the_ungated_calls_on_the_gated_schedule(dev, cases, rb, kind):
    """imitation_gradient(pol | allowed, sched) == imitation_gradient(pol, sched & allowed, day_weight=allowed) and
    surrogate_gradient(pol | allowed, sched, A, old, entropy_coef=0) == surrogate_gradient(pol, sched & allowed,
    A * allowed, old): in the gradient, exactly -- the ungated kernels add products with a zero coefficient on the closed
    days, the gated ones add nothing (so no tolerance is needed; the existing tests' bound is not used). days,
    log-likelihood, log_prob and the diagnostics against the restatement's bookkeeping."""
    ct, case = cases["synth"]
    n, T = G.N_ENVS, ct.T
    allowed = torch.as_tensor(case["allowed"], device=dev)
    sched = torch.as_tensor(case["sched"], device=dev)
    pol = _policy(ct, case, False, rb=rb, kind=kind)
    open_ = torch.as_tensor(G.by_call_day(case["allowed"], np.zeros(n, np.int64), T), device=dev)
    adv = torch.as_tensor(np.random.default_rng(2).standard_normal((T, n)).astype(np.float32), device=dev)
    A = _make(dev, ct, case)
    gated = A.imitation_gradient(dict(pol, allowed_days=allowed), sched)
    plain = A.imitation_gradient(pol, sched & allowed, day_weight=open_.float())
    _same(gated["policy_gradient"], plain["policy_gradient"], "imitation")
    st = case["start"]
    walk = G.gated_walk(case["sched"], case["allowed"], st["t"], st["used"], st["budget"], st["n_days"], st["finished"], T, rb)
    scored = walk["valid"] & ~walk["forced"]
    np.testing.assert_array_equal(gated["days"].cpu().numpy(), scored.sum(0))
    assert bool((gated["days"] < plain["days"]).any()) and bool((gated["log_likelihood"] >= plain["log_likelihood"]).all())
    lp0 = A.surrogate_gradient(dict(_shifted(pol), allowed_days=allowed), sched, adv, log_prob=True)
    old = lp0["log_prob"]
    sc = torch.as_tensor(scored, device=dev)
    assert bool((old[~sc] == 0).all()) and bool((old[sc] <= 0).all()) and bool((old[sc] < 0).any())
    sg = A.surrogate_gradient(dict(pol, allowed_days=allowed), sched, adv, old_log_prob=old, entropy_coef=0.0)
    sp = A.surrogate_gradient(pol, sched & allowed, adv * open_.float(), old_log_prob=old, entropy_coef=0.0)
    _same(sg["policy_gradient"], sp["policy_gradient"], "surrogate")
    np.testing.assert_array_equal(sg["days"].cpu().numpy(), scored.sum(0))
    assert bool((sg["clipped_days"] <= sg["days"]).all())
    # entropy_coef > 0: the entropy sums over the scored days only -- the gated call on the all-ones advantage equals
    # the ungated call less the closed days' entropy, so it is strictly smaller where a day is closed
    se = A.surrogate_gradient(dict(pol, allowed_days=allowed), sched, adv, old_log_prob=old, entropy_coef=0.01, log_prob=True)
    su = A.surrogate_gradient(pol, sched & allowed, adv, entropy_coef=0.01)
    closed_days = torch.as_tensor((walk["valid"] & walk["forced"]).sum(0), device=dev)
    assert bool((se["entropy"] <= su["entropy"]).all()) and bool((se["entropy"][closed_days > 0] < su["entropy"][closed_days > 0]).any())
    assert bool((se["log_prob"][~sc] == 0).all())
    assert A.check_status() == 0
    A.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rb", [False, True])
def test_imitation_and_surrogate_against_the_restatements(dev, cases, rb, kind):
    """The gated calls against tests/imitation_restatement.py and tests/surrogate_restatement.py with
    forced = closed day | no budget left, on rows from a twin stepped through step() along the gated schedule: gradient,
    log-likelihood and days (tests/test_imitation_gpu.py's _check_linear / _check_mlp), and with entropy_coef > 0,
    old_log_prob and log_prob=True the gradient, surrogate, approx_kl, entropy, clipped_days, days and log_prob
    (tests/test_surrogate_gpu.py's _check): the existing tests' own checks, so their bounds."""
    ct, case = cases["synth"]
    n, T = G.N_ENVS, ct.T
    allowed = torch.as_tensor(case["allowed"], device=dev)
    sched = torch.as_tensor(case["sched"], device=dev)
    pol = _policy(ct, case, False, rb=rb, kind=kind)
    gated = dict(pol, allowed_days=allowed)
    w = TI._weights(n, "mixed")
    A, B = _make(dev, ct, case), _make(dev, ct, case)
    # the twin attempts what the gate lets through; closed days are then marked forced for the restatement
    R, _ = TI._step_reference(B, sched & allowed, T, rb)
    closed = ~G.by_call_day(case["allowed"], np.zeros(n, np.int64), T) & R["valid"]
    asked = G.by_call_day(case["sched"], np.zeros(n, np.int64), T) & R["valid"]
    assert (asked & closed & ~R["forced"]).any()  # the schedule asks on closed days while budget is left
    forced = R["forced"] | closed
    g, Gn = case["group"], G.N_GROUPS
    what = f"{kind} rb={rb}"
    out = A.imitation_gradient(gated, sched, env_weight=w)
    if kind == "linear":
        ref = imitation_linear_fp64(R["obs"], asked, R["valid"], forced, w, pol["weight"], pol["bias"], g, Gn)
        TI._check_linear(out, ref, Gn, ct.n_obs, "imitation " + what)
    else:
        ref = imitation_mlp_fp64(R["obs"], asked, R["valid"], forced, w, pol["layers"], "tanh", g, Gn)
        # TI._check_mlp's comparison (|g - g_ref| <= bound for every component) on the groups that hold envs; the
        # empty group's rows are NaN on both sides, which that helper's own cases never have
        for (dW, db), (rW, rb_), (bW, bb) in zip(out["policy_gradient"]["layers"], ref["layers"], ref["bound"]):
            for x, r, bd in ((dW, rW, bW), (db, rb_, bb)):
                x = x.double().cpu().numpy()
                assert x.shape == r.shape and np.isnan(x[1]).all() and np.isnan(r[1]).all(), what
                assert (np.abs(x - r)[[0, 2]] <= bd[[0, 2]]).all(), ("imitation " + what, TI._ratio(np.abs(x - r)[[0, 2]], bd[[0, 2]]))
        assert ref["near_kink"] < 0.01
        TI._check_ll(out, ref, "imitation " + what)
    adv = TS._advantage(T, n)
    clip, beta = 0.2, 0.01
    lp0 = A.surrogate_gradient(dict(_shifted(pol), allowed_days=allowed), sched, adv, env_weight=w, log_prob=True)["log_prob"]
    sg = A.surrogate_gradient(gated, sched, adv, old_log_prob=lp0, clip=clip, entropy_coef=beta, env_weight=w, log_prob=True)
    old = lp0.double().cpu().numpy()
    if kind == "linear":
        ref = surrogate_linear_fp64(R["obs"], asked, R["valid"], forced, w, adv, old, clip, beta, pol["weight"],
                                    pol["bias"], g, Gn)
    else:
        ref = surrogate_mlp_fp64(R["obs"], asked, R["valid"], forced, w, adv, old, clip, beta, pol["layers"], "tanh", g, Gn)
    TS._check(sg, ref, pol, "surrogate " + what)
    assert (ref["days"] < R["valid"].sum(0)).any()
    assert kind != "linear" or int(ref["clipped"].sum()) > 0  # (this net's ratios stay inside the clip range)
    assert A.check_status() == 0
    A.close()
    B.close()


@pytest.mark.parametrize("kind", KINDS)
def test_policy_gradient_against_the_restatement(dev, cases, kind):
    """rollout(policy_gradient="none") under a mixed mask against tests/policy_gradient_restatement.py (mlp:
    tests/policy_gradient_mlp_restatement.py) with the gate's days as forced days, from a recorded twin; the
    restatement's own bound, as tests/test_policy_gradient_gpu.py and tests/test_policy_gradient_mlp_gpu.py (_within)."""
    ct, case = cases["synth"]
    allowed = torch.as_tensor(case["allowed"], device=dev)
    pol = dict(_policy(ct, case, True, rb=True, kind=kind), allowed_days=allowed)
    A, B = _make(dev, ct, case), _make(dev, ct, case)
    out = A.rollout(pol, policy_gradient="none")
    tr = B.rollout(pol, record=True)["trajectory"]
    S, n = ct.T, G.N_ENVS
    valid = tr["valid"].cpu().numpy()
    st = case["start"]
    # the sampled draw a_s of the policy on scored days is the recorded action; forced days carry m_s = 0
    draws = tr["action"].bool().cpu().numpy()
    alert = tr["alert"].cpu().numpy()
    used_before = np.cumsum(alert, axis=0) - alert
    forced = (~G.by_call_day(case["allowed"], st["t"], S) | ((st["budget"][None, :] - used_before) <= 0)) & valid
    assert (forced & (st["budget"][None, :] - used_before > 0)).any() and (valid & ~forced).any()
    if kind == "mlp":
        from policy_gradient_mlp_restatement import policy_gradient_mlp_fp64
        from test_policy_gradient_mlp_gpu import _layers, _within

        ref = policy_gradient_mlp_fp64(tr["obs"][:-1].double().cpu().numpy(), draws, valid, forced,
                                       tr["reward"].double().cpu().numpy(), None, pol["layers"], "tanh", case["group"],
                                       G.N_GROUPS)
        got = _layers(out)
        assert all(np.isnan(x[1]).all() for wb in got for x in wb)  # the empty group
        _within(got, ref, "mlp policy gradient under a gate", rows=[0, 2])
        A.close()
        B.close()
        return
    ref = policy_gradient_fp64(tr["obs"][:-1].double().cpu().numpy(), draws, valid, forced,
                               tr["reward"].double().cpu().numpy(), np.zeros((S, n)), pol["weight"], pol["bias"],
                               case["group"], G.N_GROUPS)
    g = out["policy_gradient"]
    got = np.concatenate([g["weight"].double().cpu().numpy(), g["bias"].double().cpu().numpy()[:, None]], axis=1)
    want = np.concatenate([ref["weight"], ref["bias"][:, None]], axis=1)
    have = ~np.isnan(want).all(axis=1)
    assert np.isnan(got[~have]).all()
    diff = np.abs(got - want)[have]
    bd = ref["bound"][have]
    print("policy gradient under a gate: max |g - g_ref| / bound =", float((diff[bd > 0] / bd[bd > 0]).max()))
    assert (diff <= ref["bound"][have]).all()
    A.close()
    B.close()


def _twin_pays(dev, ct, tup, schedules, n_steps):
    """a twin batch with one env per candidate schedule (bool [M, T]), all on the episode `tup`, stepped n_steps days
    through step(): the f32 return the env pays for each, added in day order"""
    from weather2alert_amd import HeatAlertVecEnv

    M = len(schedules)
    env = HeatAlertVecEnv(M, tables=ct, device=dev, autoreset="disabled")
    env.reset(options={"episodes": {k: np.full(M, v) for k, v in tup.items()}})
    sch = torch.as_tensor(schedules, device=dev)
    ret = torch.zeros(M, dtype=torch.float32, device=dev)
    for d in range(n_steps):
        ret += env.step(sch[:, d].to(torch.int32))[1]
    env.close()
    return ret.cpu().numpy()


def test_hindsight_under_the_restriction(dev, cases):
    """Short stretches (budget <= 3, n_steps = 12): every schedule on allowed days within the budget is paid for by a
    twin stepped through step(); the kernel's return is the twin's payment for the kernel's schedule (2e-6 relative,
    tests/test_hindsight_gpu.py::test_bit_identity's replay rule) and at least the best payment less H day bars (the
    rule of its test_brute_force). Full length: only allowed days, the return is the env's own (posterior_returns, bit
    for bit), <= the unrestricted optimum; and in like sums -- fp64 sums of the f32 rewards a twin pays per day, what the
    DP maximises -- >= the gated greedy policy on the same episodes."""
    import itertools

    ct, case = cases["synth"]
    n = G.N_ENVS
    allowed = torch.as_tensor(case["allowed"], device=dev)
    ep = dict(case["ep"], budget=np.minimum(case["ep"]["budget"], 3))
    A = _make(dev, ct, dict(case, ep=ep))
    hs = A.hindsight_optimum(n_steps=12, allowed_days=allowed)
    days = hs["alert_days"].cpu().numpy()
    got = hs["return"].cpu().numpy()
    assert not (days & ~case["allowed"]).any() and not days[:, 12:].any()
    assert (days.sum(1) <= ep["budget"]).all() and int(hs["alerts"].sum()) > 0
    for e in range(0, n, 16):
        open_ = case["allowed"][e, :12]
        pats = [p for p in itertools.product((0, 1), repeat=12)
                if sum(p) <= ep["budget"][e] and not (np.asarray(p, bool) & ~open_).any()]
        cand = np.zeros((len(pats) + 1, ct.T), bool)
        cand[:-1, :12] = np.asarray(pats, bool)
        cand[-1] = days[e]  # the kernel's own schedule, last
        paid = _twin_pays(dev, ct, {k: int(v[e]) for k, v in ep.items()}, cand, 12)
        np.testing.assert_allclose(got[e], paid[-1], rtol=2e-6, atol=0)
        assert got[e] >= paid[:-1].max() - 12 * DAY_BAR, (e, got[e], paid[:-1].max())
    A.close()
    # full length
    A, B, C = _make(dev, ct, case), _make(dev, ct, case), _make(dev, ct, case)
    st0 = {k: v.clone() for k, v in A.state().items()}
    full = A.hindsight_optimum(allowed_days=allowed)
    free = A.hindsight_optimum()
    assert not bool((full["alert_days"] & ~allowed).any())
    pr = A.posterior_returns(st0, full["alert_days"])
    assert torch.equal(pr.gather(1, st0["sample"].long()[:, None])[:, 0], full["return"])
    assert bool((full["return"] <= free["return"]).all()) and bool((full["return"] < free["return"]).any())
    out = A.rollout(dict(_policy(ct, case, False), allowed_days=allowed), hindsight=True, alert_mask=True)
    assert torch.equal(out["hindsight_return"], full["return"])
    assert out["group_hindsight_return"].shape == (G.N_GROUPS,)
    best_days = _replay(B, full["alert_days"].T.contiguous(), ct.T)[0].double().sum(0)
    greedy_days = _replay(C, out["alert_days"].T.contiguous(), ct.T)[0].double().sum(0)
    assert bool((best_days >= greedy_days).all()) and bool((best_days > greedy_days).any())
    for e_ in (A, B, C):
        e_.close()
