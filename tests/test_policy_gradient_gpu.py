"""rollout(policy_gradient=...) (k_policy_gradient_linear, w2a_policy_gradient_linear) against the fp64 restatement
(tests/policy_gradient_restatement.py), which is fed by references that never touch the kernel under test: the recorded
trajectory of an identical twin (rollout(record=True)), the rewards of a third twin that never alerts, the vector oracle
stepped with the twin's recorded actions, and the fp64 table restatement of the reward (tests/posterior_restatement.py).

The bar (policy_gradient_restatement.py): 1e-5 per reward and day -> 2e-5 per advantage; the f32 sigmoid within ~1e-7 of
fp64, taken x 10:  |g - g_ref|_j <= mean_e sum_s |o_sj| (|delta_s| 2e-5 (valid days from s on) + 1e-6 |Q_s|).
Every test prints the largest observed ratio to that bound."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402
from policy_gradient_restatement import forced_days, policy_gradient_fp64  # noqa: E402
from posterior_restatement import posterior_returns_fp64  # noqa: E402

from oracle import heatalert_oracle as O  # noqa: E402
from weather2alert_amd import synth, tables  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PR_KEYS = ("t", "used", "streak", "hist14", "budget", "n_days", "county_w", "year_i", "coef_col", "finished")
BASELINES = ("none", "no_alert")
SEED = 11


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sd():
    return synth.make_synth("linear", n_fips=30, years=[2006, 2007], n_samples=6, seed=17, extra_confounder_fips=3)


@pytest.fixture(scope="module")
def data(sd):
    """name -> (compiled tables, env keywords)"""
    return {"synth": (tables.compile_from_synth(sd), dict(similar_climate_counties=True)),
            "mini": (tables.CompiledTables.load_npz(os.path.join(GOLDEN, "mini_compiled.npz")), {})}


@pytest.fixture(scope="module")
def tabs():
    return E.make_tables()


def _params(ct, G, seed=3, scale=0.4):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((G, ct.n_obs)) * scale).astype(np.float32)
    W[:, ct.feature_names.index("remaining_budget")] *= 0.1
    return W, (rng.standard_normal(G) * 0.5).astype(np.float32)


def _policy(ct, G, g, require_budget=False, seed=SEED):
    W, b = _params(ct, G)
    pol = dict(kind="linear", weight=W, bias=b, sample=True, seed=seed, require_budget=require_budget)
    if G > 1:
        pol["group"] = g
    return pol


def _never(ct):
    """a linear policy whose logit is -1 on every row: the twin that is stepped with no alerts, day by day"""
    return dict(kind="linear", weight=np.zeros((1, ct.n_obs), np.float32), bias=np.array([-1.0], np.float32))


def _npd(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _grad(out):
    g = out["policy_gradient"]
    assert g["weight"].dtype == torch.float32 and g["bias"].dtype == torch.float32
    return np.concatenate([g["weight"].double().cpu().numpy(), g["bias"].double().cpu().numpy()[:, None]], axis=1)


def _within(got, ref, what):
    """got [G, n_obs + 1] against the restatement's gradient within its bound; returns the largest ratio"""
    want = np.concatenate([ref["weight"], ref["bias"][:, None]], axis=1)
    bound = ref["bound"]
    assert np.isfinite(got).all() and np.isfinite(want).all(), what
    diff = np.abs(got - want)
    ratio = float(np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), 0.0).max())
    print(f"{what}: max |g - g_ref| / bound = {ratio:.3e}   (max |g_ref| = {np.abs(want).max():.3e})")
    assert (diff <= bound).all(), (what, ratio)
    return ratio


def _restate_twin(st0, tr, beta, pol, baseline, g, G):
    """the restatement on a twin's recorded trajectory: logits recomputed in fp64 from the recorded rows, the forced
    days from require_budget and the start state, beta from the no-alert twin"""
    forced = forced_days(pol["require_budget"], st0["budget"], st0["used"], tr["alert"], tr["valid"])
    # a forced day records action 0 whatever the draw, and an unforced day records the policy's own draw
    return policy_gradient_fp64(tr["obs"], tr["action"], tr["valid"], forced, tr["reward"],
                                beta if baseline == "no_alert" else None, pol["weight"], pol["bias"], g, G)


def _twin_case(dev, ct, make_env, pol, g, G, prefix, n_steps, what):
    """check 5 for both baselines from one start: A1 / A2 take the gradient, B records, C is stepped with no alerts.
    Returns what check 6 needs: (B's start state, prefix actions, recorded trajectory, the two gradients)."""
    envs = [make_env() for _ in range(4)]
    A = dict(zip(BASELINES, envs[:2]))
    B, C = envs[2], envs[3]
    pre = None
    if prefix:
        for e_ in envs[:2] + [C]:
            e_.rollout(pol, n_steps=prefix)
        pre = _npd(B.rollout(pol, n_steps=prefix, record=True)["trajectory"])
    st0 = {k: v.cpu().numpy().astype(np.int64) for k, v in B.state().items()}
    tr = _npd(B.rollout(pol, n_steps=n_steps, record=True)["trajectory"])
    trc = _npd(C.rollout(_never(ct), n_steps=n_steps, record=True)["trajectory"])
    np.testing.assert_array_equal(trc["valid"], tr["valid"])
    assert not trc["alert"].any() and tr["alert"].any() and tr["valid"].any()
    got = {}
    for bl in BASELINES:
        out = A[bl].rollout(pol, n_steps=n_steps, policy_gradient=bl)
        assert A[bl].check_status() == 0
        assert out["policy_gradient"]["weight"].shape == (G, ct.n_obs) and out["policy_gradient"]["bias"].shape == (G,)
        got[bl] = _grad(out)
        _within(got[bl], _restate_twin(st0, tr, trc["reward"], pol, bl, g, G), f"{what} twin {bl}")
    assert np.abs(got["none"] - got["no_alert"]).max() > 0  # the baseline is in
    for e_ in envs:
        e_.close()
    return st0, pre, tr, got


def _oracle_replay(V, st_reset, pre, actions, S):
    """V reset to the episodes of `st_reset`, the prefix's recorded actions replayed, then `actions` [S, N] (None: no
    alerts): fp64 rows held before every decision, rewards and valid flags of the S days."""
    V.reset(st_reset["county_w"], st_reset["year_i"], st_reset["coef_col"], st_reset["sample"], st_reset["budget"])
    n = len(st_reset["t"])
    V._finished = np.zeros(n, bool)
    if pre is not None:
        for s in range(pre["action"].shape[0]):
            E.oracle_step(V, pre["action"][s].astype(np.int64))
    obs = np.zeros((S, n, V.obs.shape[1]))
    rew, valid = np.zeros((S, n)), np.zeros((S, n), bool)
    for s in range(S):
        obs[s] = V.obs
        act = np.zeros(n, np.int64) if actions is None else actions[s].astype(np.int64)
        r, _, _, live = E.oracle_step(V, act)
        rew[s], valid[s] = np.where(live, r, 0.0), live
    return obs, rew, valid


SPANS = {"whole": (0, None), "n17": (0, 17), "mid": (9, 40)}


@pytest.mark.parametrize("span", list(SPANS))
@pytest.mark.parametrize("require_budget", [False, True])
@pytest.mark.parametrize("G", [1, 5])
@pytest.mark.parametrize("name", ["mini", "synth"])
def test_gradient_against_recorded_twin_and_oracle(dev, sd, data, name, G, require_budget, span):
    """Checks 5 and 6: identical twins from one seed, a batch that is no multiple of 64, both baselines. (5) the
    restatement on the twin's recorded trajectory, beta from a twin stepped with no alerts. (6) the same with every
    float recomputed in fp64: on the synthetic table by the vector oracle stepped with the recorded actions, on the
    mini goldens (whose oracle needs a parquet engine the GPU machines do not have) by the fp64 table restatement of
    the reward fed the recorded alerts."""
    from weather2alert_amd import HeatAlertVecEnv

    ct, kw = data[name]
    n = 1500 + 29
    g = E.groups(n) if G > 1 else None
    pol = _policy(ct, G, g, require_budget)
    prefix, n_steps = SPANS[span]

    def make_env():
        env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", env_gid0=100, **kw)
        env.reset(seed=5, options={"budget": 10})
        return env

    probe = make_env()
    st_reset = {k: v.cpu().numpy().astype(np.int64) for k, v in probe.state().items()}
    probe.close()
    what = f"{name} G={G} rb={require_budget} {span}"
    st0, pre, tr, got = _twin_case(dev, ct, make_env, pol, g, G, prefix, n_steps, what)
    if require_budget:
        assert forced_days(True, st0["budget"], st0["used"], tr["alert"], tr["valid"])[tr["valid"]].any() or span == "n17"
    S = tr["valid"].shape[0]
    forced = forced_days(require_budget, st0["budget"], st0["used"], tr["alert"], tr["valid"])
    if name == "synth":
        V = O.VectorOracle(O.RefData.from_synth(sd), sd.fips_weather, sd.years)
        obs, rew, valid = _oracle_replay(V, st_reset, pre, tr["action"], S)
        _, beta, valid0 = _oracle_replay(V, st_reset, pre, None, S)
        np.testing.assert_array_equal(valid, tr["valid"])
        np.testing.assert_array_equal(valid0, tr["valid"])
        np.testing.assert_array_equal(obs[valid].astype(np.float32), tr["obs"][:S][valid])
    else:
        obs, valid = tr["obs"][:S].astype(np.float64), tr["valid"]
        days = np.zeros((n, ct.T), bool)
        tt = st0["t"][None, :] + np.cumsum(valid, axis=0) - 1
        ss, ee = np.nonzero(tr["alert"])
        days[ee, tt[ss, ee]] = True
        start = {k: st0[k] for k in PR_KEYS}
        own = st0["sample"]
        rew = posterior_returns_fp64(ct.X, ct.W, ct.n_samples, len(ct.years), start, days, S, per_day=True)[1]
        beta = posterior_returns_fp64(ct.X, ct.W, ct.n_samples, len(ct.years), start, np.zeros_like(days), S, per_day=True)[1]
        rew = np.nan_to_num(rew[np.arange(n), :, own].T)
        beta = np.nan_to_num(beta[np.arange(n), :, own].T)
    for bl in BASELINES:
        ref = policy_gradient_fp64(obs, tr["action"], valid, forced, rew, beta if bl == "no_alert" else None,
                                   pol["weight"], pol["bias"], g, G)
        _within(got[bl], ref, f"{what} fp64 {bl}")


@pytest.mark.parametrize("name", ["ragged", "slot27", "ragged27"])
def test_gradient_on_table_edges(dev, tabs, name):
    """Check 7: check 5 on the table edges (ragged episode lengths down to 1 day inside one wave, slot-27 coefficient
    rows), whole episodes and a mid-episode start after alerts: on the slot-27 tables the no-alert fork then has to use
    the decayed 14-day window of the start state."""
    from weather2alert_amd import HeatAlertVecEnv

    tb = tabs[name]
    ct, n = tb.ct, E.N_ENVS[name]
    g = E.groups(n)

    def make_env():
        env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", env_gid0=E.GID0,
                              similar_climate_counties=True)
        env.reset(seed=E.RESET[name]["seed"], options=dict(E.RESET[name]["opts"]))
        return env

    for rb in (False, True):
        W, b = E.linear_params(ct)
        pol = dict(kind="linear", weight=W, bias=b, group=g, sample=True, seed=E.POLICY_SEED, require_budget=rb)
        for span, (prefix, n_steps) in (("whole", (0, None)), ("mid", (9, 30))):
            st0, _, tr, _ = _twin_case(dev, ct, make_env, pol, g, E.G, prefix, n_steps, f"{name} rb={rb} {span}")
            if span == "mid":  # alerts inside the 14-day window of the start state
                assert ((st0["hist14"] != 0) & (st0["finished"] == 0)).any()


def _equal(a, b, what):
    if a.is_floating_point():
        a, b = a.nan_to_num(7.0), b.nan_to_num(7.0)
    assert torch.equal(a, b), what


@pytest.mark.parametrize("mode", ["disabled", "lockstep_same_step", "order"])
def test_gradient_changes_nothing_else(dev, data, mode):
    """Check 8a: with and without the keyword, identical twins: every other key, the observation buffer, state(),
    final_return and the next reset() / rollout() bit-identical (alert_mask, posterior_returns and hindsight on); two
    identical gradient calls are bit-identical."""
    from weather2alert_amd import HeatAlertVecEnv

    ct, _ = data["synth"]
    n, G = 3000 + 7, 3
    kw = dict(tables=ct, device=dev)
    if mode == "disabled":
        kw.update(autoreset="disabled")
    elif mode == "order":
        kw.update(lockstep=False, autoreset="disabled", rollout_order=True)
    envs = [HeatAlertVecEnv(n, **kw) for _ in range(3)]
    for e_ in envs:
        e_.reset(seed=4, options={"budget": 5})
    A, A2, B = envs
    g = np.random.default_rng(5).integers(0, G, n)
    pol = _policy(ct, G, g, require_budget=True, seed=2)
    for steps in (37, None, None):
        extra = dict(alert_mask=True, posterior_returns=True, hindsight=True)
        oa = A.rollout(pol, n_steps=steps, policy_gradient=True, **extra)
        oa2 = A2.rollout(pol, n_steps=steps, policy_gradient="no_alert", **extra)
        ob = B.rollout(pol, n_steps=steps, **extra)
        assert set(oa) - set(ob) == {"policy_gradient"} and not [k for k in oa if k.startswith("_")]
        for k, v in ob.items():
            _equal(oa[k], v, k)
        for k in ("weight", "bias"):
            _equal(oa["policy_gradient"][k], oa2["policy_gradient"][k], k)
        sa, sb = A.state(), B.state()
        for k in sb:
            assert torch.equal(sa[k], sb[k]), k
        assert torch.equal(A._obs, B._obs) and torch.equal(A._final_return, B._final_return)
        assert A.check_status() == 0 and B.check_status() == 0
        if mode != "lockstep_same_step" and steps is None:
            oa_, ob_ = A.reset(seed=9)[0], B.reset(seed=9)[0]
            A2.reset(seed=9)
            assert torch.equal(oa_, ob_)
    for e_ in envs:
        e_.close()


def test_gradient_group_layout(dev, data):
    """Check 8b: permuting the group labels permutes the gradient rows, and a group's gradient does not change when envs
    of other groups are added to the batch -- both within the bar of the fp64 reference (they are in fact far closer:
    an env's row does not depend on its neighbours)."""
    from weather2alert_amd import HeatAlertVecEnv

    ct, kw = data["synth"]
    n, G = 1500 + 29, 5
    g = E.groups(n)
    W, b = _params(ct, G)
    perm = np.array([3, 0, 4, 1, 2])  # new label of old group k

    def run(n_, W_, b_, g_):
        env = HeatAlertVecEnv(n_, tables=ct, device=dev, autoreset="disabled", env_gid0=100, **kw)
        env.reset(seed=5, options={"budget": 6})
        st0 = {k: v.cpu().numpy().astype(np.int64) for k, v in env.state().items()}
        pol = dict(kind="linear", weight=W_, bias=b_, group=g_, sample=True, seed=SEED)
        out = env.rollout(pol, policy_gradient="no_alert")
        env.close()
        return _grad(out), st0, pol

    base, st0, pol = run(n, W, b, g)
    Wp, bp = np.empty_like(W), np.empty_like(b)
    Wp[perm], bp[perm] = W, b
    permuted, _, _ = run(n, Wp, bp, perm[g])
    # the reference of `base`: the recorded twin
    B = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", env_gid0=100, **kw)
    C = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", env_gid0=100, **kw)
    B.reset(seed=5, options={"budget": 6})
    C.reset(seed=5, options={"budget": 6})
    tr = _npd(B.rollout(pol, record=True)["trajectory"])
    beta = _npd(C.rollout(_never(ct), record=True)["trajectory"])["reward"]
    B.close()
    C.close()
    ref = _restate_twin(st0, tr, beta, dict(pol, require_budget=False), "no_alert", g, G)
    _within(base, ref, "group layout: base")
    _within(permuted[perm], ref, "group layout: labels permuted")
    # the first n envs keep their groups; 700 more envs (the same global ids as before for the first n) join groups 1..4
    n2 = n + 700
    g2 = np.concatenate([g, 1 + np.arange(700) % 4])
    bigger, _, _ = run(n2, W, b, g2)
    ref0 = dict(weight=ref["weight"][:1], bias=ref["bias"][:1], bound=ref["bound"][:1])
    _within(bigger[:1], ref0, "group layout: other groups grown")
    print(f"group 0, bigger batch vs base: max abs diff {np.abs(bigger[0] - base[0]).max():.3e}")


def test_gradient_refusals(dev, data):
    """The refusals come before anything is launched: the env's state is untouched."""
    from weather2alert_amd import HeatAlertVecEnv

    ct, _ = data["synth"]
    n = 300
    env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled")
    env.reset(seed=1)
    before = {k: v.clone() for k, v in env.state().items()}
    W, b = _params(ct, 1)
    lin = dict(kind="linear", weight=W, bias=b, sample=True)
    for pol, kw in ((dict(lin, sample=False), dict(policy_gradient=True)), (lin, dict(policy_gradient="critic")),
                    (lin, dict(policy_gradient=True, record=True)), ({"kind": "never"}, dict(policy_gradient=True)),
                    ({"kind": "bernoulli", "p": 0.1}, dict(policy_gradient="none"))):
        with pytest.raises(ValueError):
            env.rollout(pol, **kw)
    for k, v in env.state().items():
        assert torch.equal(v, before[k]), k
    assert "policy_gradient" not in env.rollout(lin, n_steps=3, policy_gradient=False)
    env.close()


def test_gradient_full_size(dev, sd, data):
    """Check 9: 1 048 576 envs, G = 1024 (group = env id // 1024), one whole episode: finite everywhere, and 16 groups at
    a stride of 64 against check 6's reference -- each such group's 1024 envs rebuilt as a small batch with the same
    global env ids (the episode draw and the policy's uniforms are keyed by them), recorded, and replayed by the oracle."""
    from weather2alert_amd import HeatAlertVecEnv

    ct, kw = data["synth"]
    n, G, per = 1 << 20, 1024, 1024
    g = np.arange(n) // per
    W, b = _params(ct, G, seed=8)
    env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", **kw)
    env.reset(seed=77)
    out = env.rollout(dict(kind="linear", weight=W, bias=b, group=g, sample=True, seed=SEED), policy_gradient="no_alert")
    assert env.check_status() == 0 and out["done"].all()
    got = _grad(out)
    assert got.shape == (G, ct.n_obs + 1) and np.isfinite(got).all()
    del out
    env.close()
    V = O.VectorOracle(O.RefData.from_synth(sd), sd.fips_weather, sd.years)
    worst = 0.0
    for k in range(0, G, 64):
        polk = dict(kind="linear", weight=W[k:k + 1], bias=b[k:k + 1], sample=True, seed=SEED, require_budget=False)
        B = HeatAlertVecEnv(per, tables=ct, device=dev, autoreset="disabled", env_gid0=k * per, **kw)
        B.reset(seed=77)
        st0 = {kk: v.cpu().numpy().astype(np.int64) for kk, v in B.state().items()}
        tr = _npd(B.rollout(polk, record=True)["trajectory"])
        B.close()
        S = tr["valid"].shape[0]
        obs, rew, valid = _oracle_replay(V, st0, None, tr["action"], S)
        _, beta, _ = _oracle_replay(V, st0, None, None, S)
        np.testing.assert_array_equal(valid, tr["valid"])
        ref = policy_gradient_fp64(obs, tr["action"], valid, np.zeros_like(valid), rew, beta, polk["weight"],
                                   polk["bias"], None, 1)
        worst = max(worst, _within(got[k:k + 1], ref, f"full size, group {k}"))
    print(f"full size: worst ratio {worst:.3e}")
