"""rollout(kind="linear") on the GPU (k_rollout_linear): against the vector oracle's `a = policy(obs); step(a)` loop,
against the env's own step() loop, against the built-in policies it contains as special cases, its refusals, and at
full size.
Uniform tables only; the same kernel on ragged episode lengths and slot-27 coefficient rows:
tests/test_table_edges_gpu.py."""
import numpy as np
import pytest
import torch

from oracle import heatalert_oracle as O
from weather2alert_amd import synth, tables

pytestmark = pytest.mark.gpu

RETURN_RTOL, RETURN_ATOL = 2e-6, 2e-5  # as tests/test_env_gpu.py
INT_STATE = ("t", "used", "streak", "last_actual", "at_budget")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sd():
    return synth.make_synth("linear", n_fips=30, years=[2006, 2007], n_samples=6, seed=17, extra_confounder_fips=3)


@pytest.fixture(scope="module")
def ct(sd):
    return tables.compile_from_synth(sd)


def _params(ct, G, seed, scale=0.4):
    """Random parameters with a sensible alert rate: scaled per column by the table's spread."""
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((G, ct.n_obs)) * scale).astype(np.float32)
    W[:, ct.feature_names.index("remaining_budget")] *= 0.1
    b = (rng.standard_normal(G) * 0.5).astype(np.float32)
    return W, b


def _oracle_for_env(env, V, idx=None):
    st = {k: v.cpu().numpy() for k, v in env.state().items()}
    if idx is not None:
        st = {k: v[idx] for k, v in st.items()}
    V.reset(st["county_w"], st["year_i"], st["coef_col"], st["sample"], st["budget"])
    V._finished = np.zeros(len(st["t"]), bool)
    return st


def _oracle_linear(V, W, b, g, n_steps, T, require_budget=False, uniform=None, acc=None):
    """`a = policy(V.obs); V.step(a)` with fp64 logits; accumulates into acc (ret, alerts, over, alert/attempt days, tie)."""
    n = len(V.t)
    if acc is None:
        acc = dict(ret=np.zeros(n), alerts=np.zeros(n, np.int64), over=np.zeros(n, np.int64),
                   days=np.zeros((n, T), bool), att=np.zeros((n, T), bool), tie=np.zeros(n, bool))
    W64, b64 = W.astype(np.float64)[g], b.astype(np.float64)[g]
    for _ in range(n_steps):
        live = ~V._finished
        if not live.any():
            break
        prod = V.obs * W64
        z = prod.sum(axis=1) + b64
        if uniform is None:
            act = z > 0
            acc["tie"] |= live & (np.abs(z) <= 1e-9 * np.abs(prod).sum(axis=1))
        else:
            s = 1.0 / (1.0 + np.exp(-z))
            u = uniform(V.t).astype(np.float64)
            act = u < s
            acc["tie"] |= live & (np.abs(s - u) <= 1e-6)
        if require_budget:
            act &= (V.budget - V.used) > 0
        act = (act & live).astype(np.int64)
        tday, atb = V.t.copy(), V.used == V.budget
        _, r, done, actual = V.step(act)
        acc["ret"] += np.where(live, r, 0.0)
        acc["alerts"] += np.where(live, actual, 0)
        acc["over"] += np.where(live & (act == 1) & atb, 1, 0)
        rows = np.arange(n)
        acc["days"][rows[live & (actual == 1)], tday[live & (actual == 1)]] = True
        acc["att"][rows[live & (act == 1)], tday[live & (act == 1)]] = True
        V._finished = V._finished | (live & done)
    return acc


def _add(tot, out):
    for k in ("return", "alerts", "attempts_over_budget"):
        tot[k] = out[k].cpu().numpy() + tot.get(k, 0)
    for k in ("alert_days", "attempt_days"):
        if k in out:
            tot[k] = out[k].cpu().numpy() | tot.get(k, False)
    return tot


@pytest.mark.parametrize("sample", [False, True])
def test_linear_rollout_matches_oracle_policy_loop(dev, sd, ct, sample):
    """40 days of rollout(linear), 10 step() days with random actions, the rest of the episode by rollout(linear), G = 5
    groups by an explicit map: integers, day bitmaps and the env's observation buffer exact against the oracle's loop
    (envs with a near-tie logit excepted, < 1 %), returns to the suite's tolerance."""
    from weather2alert_amd import HeatAlertVecEnv

    V = O.VectorOracle(O.RefData.from_synth(sd), sd.fips_weather, sd.years)
    n, gid0, G, seed = 2000 + 37, 300, 5, 11
    env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", env_gid0=gid0, similar_climate_counties=True)
    env.reset(seed=5, options={"budget": 8})
    st = _oracle_for_env(env, V)
    np.testing.assert_array_equal(env._obs.cpu().numpy(), V.obs.astype(np.float32))
    W, b = _params(ct, G, 3)
    g = np.random.default_rng(1).integers(0, G, n)
    pol = dict(kind="linear", weight=W, bias=b, group=g, sample=sample, seed=seed)
    uni = (lambda t: O.devrng_policy_uniform_vec(seed, gid0 + np.arange(n), st["episode_no"], t)) if sample else None
    tot = {}
    out = env.rollout(pol, n_steps=40, alert_mask=True)
    assert env.last_rollout_kernel == "k_rollout_linear" and env.check_status() == 0
    assert out["group_mean_return"].shape == (G,)
    np.testing.assert_allclose(out["group_mean_return"].cpu().numpy(),
                               [out["return"].cpu().numpy()[g == k].mean() for k in range(G)], rtol=1e-5)
    _add(tot, out)
    acc = _oracle_linear(V, W, b, g, 40, ct.T, uniform=uni)
    rng = np.random.default_rng(9)
    for _ in range(10):
        a = (rng.random(n) < 0.3).astype(np.int32)
        env.step(torch.as_tensor(a, device=dev))
        _, r, _, actual = V.step(a)
    out = env.rollout(pol, alert_mask=True)
    _add(tot, out)
    acc_b = _oracle_linear(V, W, b, g, ct.T, ct.T, uniform=uni)
    assert env.check_status() == 0
    assert out["done"].all() and V._finished.all()
    tie = acc["tie"] | acc_b["tie"]
    assert tie.mean() < 0.01, tie.sum()
    ok = ~tie
    alerts_o = acc["alerts"] + acc_b["alerts"]
    assert alerts_o[ok].sum() > 0.05 * n and (alerts_o[ok] < acc["days"].shape[1]).any()  # a policy that decides
    np.testing.assert_array_equal(tot["alerts"][ok], alerts_o[ok])
    np.testing.assert_array_equal(tot["attempts_over_budget"][ok], (acc["over"] + acc_b["over"])[ok])
    # the bitmaps of the last call cover its own days (the first call's are in acc)
    np.testing.assert_array_equal(out["alert_days"].cpu().numpy()[ok], acc_b["days"][ok])
    np.testing.assert_array_equal(out["attempt_days"].cpu().numpy()[ok], acc_b["att"][ok])
    np.testing.assert_allclose(tot["return"][ok], (acc["ret"] + acc_b["ret"])[ok], rtol=RETURN_RTOL, atol=RETURN_ATOL)
    s = {k: v.cpu().numpy() for k, v in env.state().items()}
    for k, v in (("t", V.t), ("used", V.used), ("streak", V.streak), ("last_actual", V.last_actual),
                 ("at_budget", V.at_budget.astype(np.int64))):
        np.testing.assert_array_equal(s[k][ok], v[ok], err_msg=k)
    np.testing.assert_array_equal(env._obs.cpu().numpy()[ok], V.obs.astype(np.float32)[ok])
    env.close()


def _step_loop(env, W, b, g, days, dev):
    """The env's own `policy(obs) -> step()` loop with fp64 logits; returns the summed rewards."""
    W64 = torch.as_tensor(W, dtype=torch.float64, device=dev)[torch.as_tensor(g, device=dev).long()]
    b64 = torch.as_tensor(b, dtype=torch.float64, device=dev)[torch.as_tensor(g, device=dev).long()]
    ret = torch.zeros(env.num_envs, dtype=torch.float64, device=dev)
    for _ in range(days):
        z = (env._obs.double() * W64).sum(dim=1) + b64
        _, r, _, _, _ = env.step((z > 0).to(torch.int32))
        ret += r.double()
    return ret.float()


@pytest.mark.parametrize("mode", ["order", "no_order", "lockstep_same_step", "disabled", "next_step"])
def test_linear_rollout_equals_the_envs_step_loop(dev, ct, mode):
    """Two envs from one seed: rollout(linear) on one, a torch `policy(obs) -> step()` loop on the other. Returns, alerts,
    integer state and the final observation agree -- with and without the visiting order, in lock-step same_step mode over
    two consecutive episodes, with autoreset "disabled" and "next_step"."""
    from weather2alert_amd import HeatAlertVecEnv

    n, G = 4096 + 5, 4
    kw = dict(tables=ct, device=dev)
    if mode in ("order", "no_order"):
        kw.update(lockstep=False, autoreset="disabled", rollout_order=(mode == "order"))
    elif mode == "disabled":
        kw.update(autoreset="disabled")
    elif mode == "next_step":
        kw.update(autoreset="next_step")
    A, B = HeatAlertVecEnv(n, **kw), HeatAlertVecEnv(n, **kw)
    A.reset(seed=8)
    B.reset(seed=8)
    W, b = _params(ct, G, 4)
    g = np.random.default_rng(2).integers(0, G, n)
    pol = dict(kind="linear", weight=W, bias=b, group=g)
    episodes = 2 if mode in ("lockstep_same_step", "next_step") else 1
    for ep in range(episodes):
        if mode == "next_step" and ep == 1:
            B.step(torch.zeros(n, dtype=torch.int32, device=dev))  # the restart call: actions ignored, reward 0
        ua0 = A.state()["used"]
        oa = A.rollout(pol, n_steps=50)
        ob = A.rollout(pol)
        ret_b = _step_loop(B, W, b, g, ct.T, dev)
        assert A.last_rollout_kernel == "k_rollout_linear"
        torch.testing.assert_close(oa["return"] + ob["return"], ret_b, rtol=RETURN_RTOL, atol=RETURN_ATOL)
        if mode in ("order", "no_order", "disabled"):  # nothing reset the batch after the terminal day
            sa, sb = A.state(), B.state()
            for k in INT_STATE + ("hist14", "finished"):
                assert torch.equal(sa[k], sb[k]), k
            assert torch.equal((oa["alerts"] + ob["alerts"]), sa["used"] - ua0)
        assert torch.equal(A._obs, B._obs)
        assert A.check_status() == 0 and B.check_status() == 0
    A.close()
    B.close()


@pytest.mark.parametrize("order", [True, False])
def test_builtin_policies_are_special_cases(dev, ct, order):
    """G = 1: W = 0 with b = -1 / +1 is `never` / `always`; W = e_heat_qi with b = -float32(0.8) is threshold(heat_qi,
    0.8, lag 1) -- the fp64 sign of x + b for two f32 values is the f32 comparison x > 0.8f -- with and without
    require_budget: integers exact against whichever built-in kernel rollout() picks (k_rollout64 / k_rollout_mfma)."""
    from weather2alert_amd import HeatAlertVecEnv

    n = 3000 + 11
    zero = np.zeros((1, ct.n_obs), np.float32)
    e_hq = zero.copy()
    e_hq[0, ct.feature_names.index("heat_qi")] = 1.0
    cases = [(dict(weight=zero, bias=[-1.0]), dict(kind="never")),
             (dict(weight=zero, bias=[1.0]), dict(kind="always")),
             (dict(weight=e_hq, bias=[-np.float32(0.8)]), dict(kind="threshold", feature="heat_qi", threshold=0.8)),
             (dict(weight=e_hq, bias=[-np.float32(0.8)], require_budget=True),
              dict(kind="threshold", feature="heat_qi", threshold=0.8, require_budget=True))]
    for lin, builtin in cases:
        A = HeatAlertVecEnv(n, tables=ct, device=dev, rollout_order=order, similar_climate_counties=True)
        B = HeatAlertVecEnv(n, tables=ct, device=dev, rollout_order=order, similar_climate_counties=True)
        A.reset(seed=2, options={"budget": 6})
        B.reset(seed=2, options={"budget": 6})
        alerts = 0
        for steps in (30, None):
            oa = A.rollout(dict(kind="linear", **lin), n_steps=steps, alert_mask=True)
            alerts = alerts + oa["alerts"]
            ob = B.rollout(builtin, n_steps=steps, alert_mask=True)
            for k in ("alerts", "attempts_over_budget", "alert_days", "attempt_days", "done"):
                assert torch.equal(oa[k], ob[k]), (builtin, steps, k)
            torch.testing.assert_close(oa["return"], ob["return"], rtol=3e-6, atol=3e-5)
            if steps:
                sa, sb = A.state(), B.state()
                for k in INT_STATE + ("hist14",):
                    assert torch.equal(sa[k], sb[k]), (builtin, k)
        assert bool((alerts > 0).any()) == (builtin["kind"] != "never")
        assert A.check_status() == 0
        A.close()
        B.close()


def test_linear_rollout_refusals(dev, ct):
    from weather2alert_amd import HeatAlertVecEnv

    n = 512
    W, b = _params(ct, 2, 5)
    g = np.arange(n) % 2
    pol = dict(kind="linear", weight=W, bias=b, group=g)
    pm = HeatAlertVecEnv(n, tables=ct, device=dev, reward_mode="posterior_mean", autoreset="disabled")
    pm.reset(seed=1)
    with pytest.raises(ValueError, match="sampled"):
        pm.rollout(pol)
    pm.close()
    fx = HeatAlertVecEnv(n, tables=ct, device=dev, fixes=("lag",))
    fx.reset(seed=1)
    with pytest.raises(ValueError, match="faithful"):
        fx.rollout(pol)
    fx.close()
    ok = HeatAlertVecEnv(n, tables=ct, device=dev, fixes=("budget",), autoreset="disabled")
    ok.reset(seed=1)
    ok.rollout(pol, n_steps=3)
    assert ok.check_status() == 0
    for bad in (dict(weight=W[:, :-1]), dict(bias=b[:1]), dict(group=g[:-1]), dict(group=g + 1),
                dict(weight=np.where(W > 0, np.inf, W).astype(np.float32))):
        with pytest.raises(ValueError):
            ok.rollout({**pol, **bad})
    ok.rollout(pol, n_steps=3)
    assert ok.check_status() == 0
    # a built-in rollout stopped mid-episode writes no observation rows: the buffer is stale until step() / reset()
    ok.rollout(dict(kind="always"), n_steps=5)
    with pytest.raises(RuntimeError, match="observation buffer"):
        ok.rollout(pol)
    ok.step(torch.zeros(n, dtype=torch.int32, device=dev))
    ok.rollout(pol, n_steps=2)
    sd_ = ok.state_dict()
    ok.load_state_dict(sd_)
    with pytest.raises(RuntimeError, match="observation buffer"):
        ok.rollout(pol)
    ok.reset(seed=2)
    ok.rollout(pol, n_steps=2)
    assert ok.check_status() == 0
    ok.close()
    no = HeatAlertVecEnv(n, tables=ct, device=dev, write_obs=False)
    no.reset(seed=1)
    with pytest.raises(RuntimeError, match="observation buffer"):
        no.rollout(pol)
    no.close()


def test_linear_rollout_full_size(dev, sd, ct):
    """1 048 576 envs, G = 1024 groups: a strided sample (the last env included) against the oracle's loop."""
    from weather2alert_amd import HeatAlertVecEnv

    n, G = 1 << 20, 1024
    env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", similar_climate_counties=True)
    env.reset(seed=77)
    idx = np.unique(np.concatenate([np.arange(0, n, 509), [n - 1]]))
    V = O.VectorOracle(O.RefData.from_synth(sd), sd.fips_weather, sd.years)
    _oracle_for_env(env, V, idx)
    W, b = _params(ct, G, 6)
    g = np.random.default_rng(3).integers(0, G, n)
    pol = dict(kind="linear", weight=W, bias=b, group=torch.as_tensor(g, device=dev))
    o1 = env.rollout(pol, n_steps=100)
    o2 = env.rollout(pol)
    assert env.check_status() == 0 and o2["done"].all()
    acc = _oracle_linear(V, W, b, g[idx], ct.T, ct.T)
    ok = ~acc["tie"]
    assert acc["tie"].mean() < 0.01 and ok[-1]
    np.testing.assert_array_equal((o1["alerts"] + o2["alerts"]).cpu().numpy()[idx][ok], acc["alerts"][ok])
    np.testing.assert_allclose((o1["return"] + o2["return"]).cpu().numpy()[idx][ok], acc["ret"][ok], rtol=RETURN_RTOL,
                               atol=RETURN_ATOL)
    s = {k: v.cpu().numpy()[idx] for k, v in env.state().items()}
    for k, v in (("t", V.t), ("used", V.used), ("streak", V.streak), ("last_actual", V.last_actual)):
        np.testing.assert_array_equal(s[k][ok], v[ok], err_msg=k)
    np.testing.assert_array_equal(env._obs.cpu().numpy()[idx][ok], V.obs.astype(np.float32)[ok])
    gm = o2["group_mean_return"].cpu().numpy()
    ret2 = o2["return"].cpu().numpy()
    np.testing.assert_allclose(gm[:3], [ret2[g == k].mean() for k in range(3)], rtol=1e-5)
    env.close()
