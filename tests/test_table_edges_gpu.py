"""Every kernel with its own copy of the env's day loop -- k_rollout_linear, k_rollout_mlp (plain and record=True),
k_posterior_returns, k_hs_dp -- on the table edges that until now only step() and the built-in rollout kernels met
(tests/table_edges.py): ragged episode lengths inside one wave (20..153 days and the shortest there are: 1, 2, 3),
coefficient rows with a term on slot 27 (the agent's 14-day alert count) and with the large heat_qi / bias pair, and
both together. References: the vector oracle's fp64 `a = policy(obs); step(a)` loop, the fp64 restatements
(tests/posterior_restatement.py, tests/hindsight_restatement.py) and the env's own step() on a twin batch -- never the
kernel under test. tests/test_table_edges_cpu.py checks the references themselves (near-tie share, that the policies
decide, lengths per wave) without a GPU.

A new kernel with a day loop of its own belongs in this matrix ("Table edges")."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402
from hindsight_restatement import brute_force_fp64, hindsight_fp64, horizon, own_draw_returns  # noqa: E402
from posterior_restatement import posterior_returns_fp64  # noqa: E402

pytestmark = pytest.mark.gpu

REWARD_TOL = DAY_BAR = 1e-5  # the suite's per-day bar against fp64 (tests/test_env_gpu.py)
RETURN_RTOL, RETURN_ATOL = 2e-6, 2e-5  # as tests/test_env_gpu.py
INT_STATE = ("t", "used", "streak", "last_actual", "at_budget", "hist14", "finished")
PR_KEYS = ("t", "used", "streak", "hist14", "budget", "n_days", "county_w", "year_i", "coef_col", "finished")
HS_KEYS = PR_KEYS + ("sample",)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tabs():
    """the three tables, built once"""
    return E.make_tables()


def _env(tb, dev, n=None, reset=True, **kw):
    """A fresh env on the table's batch (tests/table_edges.py: RESET, N_ENVS); its tuples are the host restatement's."""
    from weather2alert_amd import HeatAlertVecEnv

    n = E.N_ENVS[tb.name] if n is None else n
    env = HeatAlertVecEnv(n, tables=tb.ct, device=dev, autoreset="disabled", env_gid0=E.GID0,
                          similar_climate_counties=True, **kw)
    assert env._lockstep == (not tb.ragged)
    if reset:
        env.reset(seed=E.RESET[tb.name]["seed"], options=dict(E.RESET[tb.name]["opts"]))
    return env


def _np(d, keys=None):
    return {k: d[k].cpu().numpy().astype(np.int64) for k in (keys or d)}


def _clone(st):
    return {k: v.clone() for k, v in st.items()}


def _check_tuples(env, tup):
    st = _np(env.state())
    for k, v in tup.items():
        np.testing.assert_array_equal(st[k], v, err_msg=k)
    return st


def _own(pr, st0):
    return pr.gather(1, st0["sample"].long()[:, None])[:, 0]


def _restate(ct, st, alert_days, n_steps, per_day=False):
    ad = alert_days.cpu().numpy() if torch.is_tensor(alert_days) else alert_days
    return posterior_returns_fp64(ct.X, ct.W, ct.n_samples, ct.Y, {k: st[k] for k in PR_KEYS}, ad, n_steps, per_day=per_day)


def _step_replay(env, attempt_days, T):
    """The env's own step() driven by a schedule of attempts from day 0. step() has no notion of "this env is over" in
    a batch that is not in lock step (it raises W2A_ST_STEP_AFTER_DONE and goes on shifting the history), so every env
    is read on its own days only: (summed rewards f64 [n], integer state and observation rows as its terminal step left
    them, the status bits the replay raised)."""
    n, dev = env.num_envs, env.device
    acc = torch.zeros(n, dtype=torch.float64, device=dev)
    fin = torch.zeros(n, dtype=torch.bool, device=dev)
    snap, obs_snap = _clone(env.state()), env._obs.clone()
    for t in range(T):
        if bool(fin.all()):
            break
        a = torch.where(fin, torch.zeros_like(attempt_days[:, t]), attempt_days[:, t]).to(torch.int32)
        _, r, term, _, _ = env.step(a)
        acc += torch.where(fin, torch.zeros_like(acc), r.double())
        st = env.state()
        for k in snap:
            snap[k] = torch.where(fin, snap[k], st[k])
        obs_snap = torch.where(fin[:, None], obs_snap, env._obs)
        fin = fin | term.bool()
    assert bool(fin.all())
    return acc, snap, obs_snap, env.check_status()


# ------------------------------------------------------------------ k_rollout_linear, k_rollout_mlp
@pytest.mark.parametrize("name", ["ragged", "slot27", "ragged27"])
@pytest.mark.parametrize("pol_name", list(E.POLICIES))
def test_policy_rollouts_on_table_edges(dev, tabs, name, pol_name):
    """A whole episode in one call (A), the same in two calls of k days and the rest (B), and step() driven by A's
    attempts (C), three envs from one seed. Against the oracle's fp64 loop (near-tie envs excepted, < 1 %): alerts,
    attempts over budget, both day bitmaps, the integer state, `done`, the observation buffer exact; returns to the
    suite's bars against the oracle (where it knows the coefficients), against the fp64 restatement fed A's alert days
    (every env, slot 27 included) and against step(); the own-draw column of posterior_returns bit for bit."""
    tb = tabs[name]
    ct, n = tb.ct, E.N_ENVS[name]
    tup = E.host_tuples(tb, n)
    g = E.groups(n)
    pol, fn, ties = E.make_policy(ct, pol_name, g)
    kernel = "k_rollout_linear" if pol["kind"] == "linear" else "k_rollout_mlp"
    V = tb.oracle()
    E.oracle_reset(V, tup)
    R = E.oracle_record(V, fn, ct.T, ties, uniform=E.policy_uniform(n) if pol["sample"] else None)
    tie, ok = R["tie"], ~R["tie"]
    assert tie.mean() < 0.01, tie.sum()
    known = ~tb.a2w[tup["coef_col"]]
    A, B, Cenv = _env(tb, dev), _env(tb, dev), _env(tb, dev)
    st0 = _clone(A.state())
    _check_tuples(A, tup)
    entry = A._obs.cpu().numpy()
    np.testing.assert_array_equal(entry, R["obs"][0])

    oa = A.rollout(pol, alert_mask=True, posterior_returns=True)
    assert A.last_rollout_kernel == kernel and A.check_status() == 0
    k = 7 if tb.ct.T < 100 else 41
    ob1 = B.rollout(pol, n_steps=k, alert_mask=True)
    mid = _np(B.state())
    ob2 = B.rollout(pol, alert_mask=True)
    assert B.last_rollout_kernel == kernel and B.check_status() == 0
    # a call of k days stops every env after min(k, its own length) days
    np.testing.assert_array_equal(mid["finished"], tup["n_days"] <= k)
    np.testing.assert_array_equal(mid["t"], np.minimum(k, tup["n_days"] - 1))

    got = {kk: oa[kk].cpu().numpy() for kk in ("return", "alerts", "attempts_over_budget", "alert_days", "attempt_days")}
    assert oa["done"].all() and ob2["done"].all()
    for kk, ref in (("alerts", R["alerts"]), ("attempts_over_budget", R["over"]), ("alert_days", R["days"]),
                    ("attempt_days", R["att"])):
        np.testing.assert_array_equal(got[kk][ok], ref[ok], err_msg=kk)
    sa, so = _np(A.state()), E.oracle_state(V)
    for kk in INT_STATE:
        np.testing.assert_array_equal(sa[kk][ok], so[kk][ok], err_msg=kk)
    np.testing.assert_array_equal(sa["t"], tup["n_days"] - 1)
    np.testing.assert_array_equal(A._obs.cpu().numpy()[ok], R["obs"][ct.T][ok])
    # nothing past an env's last day: no bitmap bit at or beyond n_days, one-day episodes keep the row of the reset
    past = np.arange(ct.T)[None, :] >= tup["n_days"][:, None]
    assert not (got["alert_days"] & past).any() and not (got["attempt_days"] & past).any()
    np.testing.assert_array_equal(A._obs.cpu().numpy()[tup["n_days"] == 1], entry[tup["n_days"] == 1])
    assert (got["alerts"][tup["budget"] == 0] == 0).all()
    # returns: the oracle where it knows the coefficients, the restatement (slot 27 in fp64) for every env
    ret = got["return"].astype(np.float64)
    print(f"{name}/{pol_name}: max |return - oracle| = {np.abs(ret - R['ret'])[ok & known].max():.2e}")
    np.testing.assert_allclose(ret[ok & known], R["ret"][ok & known], rtol=RETURN_RTOL, atol=RETURN_ATOL)
    pr64 = _restate(ct, _np(st0), got["alert_days"], ct.T)
    own64 = pr64[np.arange(n), tup["sample"]]
    print(f"{name}/{pol_name}: max |return - restatement| = {np.abs(ret - own64).max():.2e}")
    np.testing.assert_allclose(ret, own64, rtol=RETURN_RTOL, atol=RETURN_ATOL)
    if tb.slot27:  # the slot-27 coefficients act: the oracle, which has none, is off on those columns
        assert np.abs(ret - R["ret"])[ok & ~known].max() > 1e-4
    # posterior_returns of the same call: the own draw bit for bit, every column against the restatement
    assert torch.equal(_own(oa["posterior_returns"], st0), oa["return"])
    np.testing.assert_allclose(oa["posterior_returns"].double().cpu().numpy(), pr64, rtol=RETURN_RTOL, atol=RETURN_ATOL)
    gm = oa["group_mean_return"].double().cpu().numpy()
    np.testing.assert_allclose(gm, [ret[g == j].mean() for j in range(E.G)], rtol=1e-5)
    # the split call: every integer output and the final state and buffer as the whole call's, bit for bit
    for kk in ("alerts", "attempts_over_budget"):
        assert torch.equal(ob1[kk] + ob2[kk], oa[kk]), kk
    for kk in ("alert_days", "attempt_days"):
        assert torch.equal(ob1[kk] | ob2[kk], oa[kk]), kk
        assert not (ob1[kk] & ob2[kk]).any()
    sb = B.state()
    for kk, v in A.state().items():
        assert torch.equal(v, sb[kk]), kk
    assert torch.equal(A._obs, B._obs) and torch.equal(oa["final_return"], ob2["final_return"])
    np.testing.assert_allclose((ob1["return"].double() + ob2["return"].double()).cpu().numpy(), own64, rtol=RETURN_RTOL,
                               atol=RETURN_ATOL)
    # step() driven by A's attempts pays the same and leaves the same state and buffer
    acc, sc, obs_c, bits = _step_replay(Cenv, oa["attempt_days"], ct.T)
    assert bits == (4 if tb.ragged else 0)  # W2A_ST_STEP_AFTER_DONE: step() went on past the shorter episodes
    torch.testing.assert_close(oa["return"].double(), acc, rtol=RETURN_RTOL, atol=RETURN_ATOL)
    for kk in INT_STATE + ("n_days", "budget"):
        assert torch.equal(A.state()[kk], sc[kk]), kk
    assert torch.equal(A._obs, obs_c)
    for e in (A, B):
        assert e.check_status() == 0
    for e in (A, B, Cenv):
        e.close()


# ------------------------------------------------------------------ record=True
@pytest.mark.parametrize("name", ["ragged", "ragged27"])
@pytest.mark.parametrize("pol_name", ["linear_sampled", "mlp16", "mlp64x64_sampled"])
def test_recorded_trajectories_on_ragged_tables(dev, tabs, name, pol_name):
    """Nine step() days with random actions (the shortest episodes are over on entry), then the rest recorded in one
    call: obs bit-equal with the bootstrap row obs[S], actions and flags exact, every env recorded for exactly the days
    it had left, rewards and logits within their bars; what the contract says of entries the env did not step (flags 0;
    the row after a terminal step repeats the one before; obs[S] is the buffer for every env); recording changes no
    other output."""
    tb = tabs[name]
    ct, n = tb.ct, E.N_ENVS[name]
    tup = E.host_tuples(tb, n)
    g = E.groups(n)
    pol, fn, ties = E.make_policy(ct, pol_name, g)
    V = tb.oracle()
    E.oracle_reset(V, tup)
    A, B = _env(tb, dev), _env(tb, dev)
    rng = np.random.default_rng(9)
    for _ in range(9):
        a = np.where(V._finished, 0, rng.random(n) < 0.3).astype(np.int32)
        for e in (A, B):
            e.step(torch.as_tensor(a, device=dev))
        E.oracle_step(V, a)
    for e in (A, B):  # step() went on past the shortest episodes (it shifts their history; nothing else moves)
        assert e.check_status() == 4  # W2A_ST_STEP_AFTER_DONE
    st0 = _clone(A.state())
    s0 = _np(st0)
    fin0 = s0["finished"] == 1
    for kk, v in E.oracle_state(V).items():
        sel = ~fin0 if kk in ("hist14", "last_actual", "at_budget") else np.ones(n, bool)
        np.testing.assert_array_equal(s0[kk][sel], v[sel], err_msg=kk)
    assert fin0.any() and (s0["hist14"] != 0).any()
    S = ct.T
    R = E.oracle_record(V, fn, S, ties, uniform=E.policy_uniform(n) if pol["sample"] else None, T=ct.T)
    ok = ~R["tie"]
    assert R["tie"].mean() < 0.01, R["tie"].sum()
    entry = A._obs.clone()
    oa = A.rollout(pol, record=True, alert_mask=True)
    ob = B.rollout(pol, alert_mask=True)
    assert A.check_status() == 0 and oa["done"].all()
    tr = {k: v.cpu().numpy() for k, v in oa["trajectory"].items()}
    assert tr["obs"].shape == (S + 1, n, ct.n_obs)
    left = np.where(s0["finished"] == 1, 0, s0["n_days"] - s0["t"])
    np.testing.assert_array_equal(tr["valid"].sum(0), left)  # every env: exactly the days it had left, no more
    assert (tr["valid"] == (np.arange(S)[:, None] < left[None, :])).all()
    np.testing.assert_array_equal(tr["terminated"].sum(0), (left > 0).astype(np.int64))
    v = R["valid"][:, ok]
    for k in ("valid", "terminated", "alert", "action"):
        np.testing.assert_array_equal(tr[k][:, ok] * (v if k == "action" else 1), R[k][:, ok], err_msg=k)
    assert R["alert"][:, ok].any() and (R["alert"][:, ok] < v).any()  # a policy that decides
    assert not (tr["terminated"] & ~tr["valid"]).any() and not (tr["alert"] & ~tr["valid"]).any()
    np.testing.assert_array_equal(tr["obs"][:-1, ok][v], R["obs"][:-1, ok][v])
    # the contract's other rows: slab 0 and slab S for EVERY env; the row after a terminal step repeats the one before
    np.testing.assert_array_equal(tr["obs"][0], entry.cpu().numpy())
    np.testing.assert_array_equal(tr["obs"][S], A._obs.cpu().numpy())
    np.testing.assert_array_equal(tr["obs"][S][ok & ~fin0], R["obs"][S][ok & ~fin0])
    sT, eT = np.nonzero(tr["terminated"])
    np.testing.assert_array_equal(tr["obs"][sT + 1, eT], tr["obs"][sT, eT])
    np.testing.assert_array_equal(tr["obs"][S][fin0], entry.cpu().numpy()[fin0])
    # rewards: the restatement's per-day rewards of the env's own draw (slot 27 in fp64), and the oracle where it knows
    _, days = _restate(ct, s0, oa["alert_days"], S, per_day=True)
    r64 = days[np.arange(n), :, s0["sample"]].T  # [S, n]
    va = tr["valid"]
    assert not np.isnan(r64[va]).any() and np.isnan(r64[~va]).all()
    print(f"{name}/{pol_name}: max per-day |reward - restatement| = {np.abs(tr['reward'][va] - r64[va]).max():.2e}")
    np.testing.assert_allclose(tr["reward"][va], r64[va], rtol=REWARD_TOL, atol=REWARD_TOL)
    known = ~tb.a2w[tup["coef_col"]]
    kn = (ok & known)
    np.testing.assert_allclose(tr["reward"][:, kn][R["valid"][:, kn]], R["reward"][:, kn][R["valid"][:, kn]],
                               rtol=REWARD_TOL, atol=REWARD_TOL)
    lg, z, mag = tr["logit"][:, ok][v].astype(np.float64), R["logit"][:, ok][v], R["mag"][:, ok][v]
    if pol["kind"] == "linear":  # the fp64 logit rounded to f32
        assert (np.abs(lg - z) <= 1e-6 * np.abs(z) + 1e-9 * mag).all()
    else:  # the f32 network, within the near-tie band of include/w2a.h
        assert (np.abs(lg - z) <= 1e-5 * mag).all()
    # recording changes nothing else
    assert set(oa) - set(ob) == {"trajectory"}
    for k, x in ob.items():
        y = oa[k]
        if x.is_floating_point():
            x, y = x.nan_to_num(7.0), y.nan_to_num(7.0)
        assert torch.equal(x, y), k
    sb = B.state()
    for k, x in A.state().items():
        assert torch.equal(x, sb[k]), k
    assert torch.equal(A._obs, B._obs) and torch.equal(A._final_return, B._final_return)
    ret = torch.zeros(n, dtype=torch.float32, device=dev)
    t_ = oa["trajectory"]
    for s in range(S):
        ret = torch.where(t_["valid"][s], ret + t_["reward"][s], ret)
    assert torch.equal(ret, oa["return"])
    for e in (A, B):
        assert e.check_status() == 0
        e.close()


# ------------------------------------------------------------------ k_posterior_returns
@pytest.mark.parametrize("name", ["slot27", "ragged", "ragged27"])
def test_posterior_returns_on_table_edges(dev, tabs, name):
    """Arbitrary start states -- random days inside each env's own episode, random NONZERO 14-day words, counters,
    finished flags -- and random bitmaps, for 1, 17 and T days: every column against the fp64 restatement. The own
    draw of a built-in kind on k_rollout64 bit for bit; chained partial calls sum to one call."""
    tb = tabs[name]
    ct, n = tb.ct, E.N_ENVS[name]
    B = _env(tb, dev, rollout_mfma=False)
    rng = np.random.default_rng(4)
    base = B.state()
    st = _np(base, PR_KEYS)
    st["t"] = (rng.random(n) * st["n_days"]).astype(np.int64)  # mid-episode, the last day included
    st["t"][::5] = st["n_days"][::5] - 1
    st["used"] = rng.integers(0, 4, n)
    st["streak"] = rng.integers(0, 3, n)
    st["hist14"] = rng.integers(1, 1 << 14, n)
    st["hist14"][::3] |= 1 << 13  # the window's oldest day set: it leaves the window on the first day
    st["finished"] = (rng.random(n) < 0.1).astype(np.int64)
    ad = rng.random((n, ct.T)) < 0.25
    dst = {k: torch.as_tensor(v, dtype=torch.int32, device=dev) for k, v in st.items()}
    for steps in (1, 17, ct.T):
        got = B.posterior_returns(dst, torch.as_tensor(ad, device=dev), n_steps=steps).double().cpu().numpy()
        ref = _restate(ct, st, ad, steps)
        print(f"{name}: {steps} days, max |posterior_returns - restatement| = {np.abs(got - ref).max():.2e}")
        np.testing.assert_allclose(got, ref, rtol=RETURN_RTOL, atol=RETURN_ATOL)
        assert (got[st["finished"] == 1] == 0).all()
    if tb.slot27:  # the window acts: without the start word the slot-27 columns' returns differ
        c27 = tb.a2w[st["coef_col"]] & (st["finished"] == 0)
        ref0 = _restate(ct, {**st, "hist14": np.zeros(n, np.int64)}, ad, 1)
        assert np.abs(ref0 - _restate(ct, st, ad, 1))[c27].max() > 1e-4
    # a built-in kind on k_rollout64, in three chained calls; a twin runs the episode in one
    A = _env(tb, dev, rollout_mfma=False)
    pol = dict(kind="bernoulli", p=0.3, seed=2)
    st0 = _clone(A.state())
    parts = []
    for k in (5, 9, None):
        s_k = _clone(A.state())
        o = A.rollout(pol, n_steps=k, posterior_returns=True, alert_mask=True)
        assert A.last_rollout_kernel == "k_rollout64"
        assert torch.equal(_own(o["posterior_returns"], s_k), o["return"])
        np.testing.assert_allclose(o["posterior_returns"].double().cpu().numpy(),
                                   _restate(ct, _np(s_k), o["alert_days"], k or ct.T), rtol=RETURN_RTOL, atol=RETURN_ATOL)
        parts.append(o)
    whole = B.rollout(pol, posterior_returns=True, alert_mask=True)
    assert torch.equal(whole["alert_days"], parts[0]["alert_days"] | parts[1]["alert_days"] | parts[2]["alert_days"])
    assert torch.equal(_own(whole["posterior_returns"], st0), whole["return"])
    np.testing.assert_allclose(sum(p["posterior_returns"].double() for p in parts).cpu().numpy(),
                               whole["posterior_returns"].double().cpu().numpy(), rtol=2e-6, atol=1e-5)
    for e in (A, B):
        assert e.check_status() == 0
        e.close()


# ------------------------------------------------------------------ k_hs_dp
def test_hindsight_on_ragged_table(dev, tabs):
    """The ragged table with every shortest episode and the full-length one injected, a third of the envs each on budget
    0, the tables' default and 40 (beyond most remaining horizons, and all of the shortest episodes'), from reset and
    mid-episode, to the end and for 4 days: feasibility inside each env's own horizon, the value against the fp64 DP
    and (horizons of at most 4 days) brute force, bit-identity with posterior_returns, step() paying the schedule, and
    dominance over linear, mlp and threshold rollouts of the same batch."""
    from weather2alert_amd import HeatAlertVecEnv

    tb = tabs["ragged"]
    ct, n = tb.ct, 384 + 5
    Y, K = ct.Y, ct.n_samples
    rng = np.random.default_rng(21)
    col = rng.integers(0, ct.S, n)
    cw, yi = ct.fips_to_weather[col].astype(np.int64), rng.integers(0, Y, n)
    nd_tab = np.asarray(ct.n_days).reshape(-1, Y)
    pairs = [tuple(p) for d in E.SHORTEST + (ct.T,) for p in np.argwhere(nd_tab == d)[:1]]
    for i in range(24):  # six envs on each of the four edge lengths, two per budget kind
        cw[i], yi[i] = pairs[i % 4]
    default = np.asarray(ct.B0)[cw * Y + yi]
    budget = np.where(np.arange(n) % 3 == 0, 0, np.where(np.arange(n) % 3 == 1, default, 40))
    ep = dict(county_w=cw, year_i=yi, coef_col=col, sample=rng.integers(0, K, n), budget=budget)
    kw = dict(tables=ct, device=dev, autoreset="disabled", env_gid0=E.GID0)
    env = HeatAlertVecEnv(n, **kw)
    env.reset(options={"episodes": ep})
    g = torch.Generator(device=dev).manual_seed(3)
    for days in (0, 13):
        for _ in range(days):
            a = (torch.rand(n, generator=g, device=dev) < 0.35) & (env.state()["finished"] == 0)
            env.step(a.to(torch.int32))
        assert env.check_status() == (4 if days else 0)  # W2A_ST_STEP_AFTER_DONE: step() past the shortest episodes
        st0 = _clone(env.state())
        st = _np(st0, HS_KEYS)
        nd = st["n_days"]
        np.testing.assert_array_equal(st["budget"], budget)
        assert set(E.SHORTEST + (ct.T,)) <= set(nd.tolist()) and len(np.unique(nd)) > 40
        for steps in (None, 4):
            n_steps = steps or ct.T
            hs = env.hindsight_optimum(st0, n_steps=steps)
            days_g, alerts_g = hs["alert_days"].cpu().numpy(), hs["alerts"].cpu().numpy()
            H = np.array([horizon({k: int(st[k][e]) for k in st}, n_steps) for e in range(n)])
            assert (H == np.where(st["finished"] == 1, 0, np.minimum(n_steps, nd - st["t"]))).all()
            assert (days_g.sum(1) == alerts_g).all() and (alerts_g <= np.maximum(0, st["budget"] - st["used"])).all()
            inside = (np.arange(ct.T)[None, :] >= st["t"][:, None]) & (np.arange(ct.T)[None, :] < (st["t"] + H)[:, None])
            assert not (days_g & ~inside).any()
            mine = own_draw_returns(ct.X, ct.W, K, Y, st, days_g, n_steps)
            val, _, _ = hindsight_fp64(ct.X, ct.W, K, Y, st, n_steps)
            assert (mine >= val - H * DAY_BAR).all()
            err = np.abs(hs["return"].double().cpu().numpy() - val)
            print(f"day {days}, {n_steps} days: max |return - fp64 DP| / H = {(err / np.maximum(H, 1)).max():.2e}")
            assert (err <= H * DAY_BAR).all()
            assert (hs["return"].cpu().numpy()[H == 0] == 0).all() and (alerts_g[H == 0] == 0).all()
            for e in np.nonzero((H > 0) & (H <= 4))[0][:96]:
                best, _ = brute_force_fp64(ct.X, ct.W, K, Y, st, n_steps, e)
                assert mine[e] >= best - H[e] * DAY_BAR, (e, mine[e], best)
            pr = env.posterior_returns(st0, hs["alert_days"], n_steps=steps)
            assert torch.equal(_own(pr, st0), hs["return"]), (days, steps)
            assert alerts_g[budget == 0].sum() == 0 and (alerts_g <= H).all()
            if steps is None:
                assert alerts_g[budget == 40].sum() > alerts_g[budget != 40].sum() > 0
    assert env.check_status() == 0
    env.close()
    # step() pays the schedule from reset; rollout(hindsight=True) dominates each kind's own return on the same batch
    A = HeatAlertVecEnv(n, **kw)
    A.reset(options={"episodes": ep})
    hs = A.hindsight_optimum()
    acc, sc, _, _ = _step_replay(A, hs["alert_days"], ct.T)
    np.testing.assert_allclose(acc.cpu().numpy(), hs["return"].double().cpu().numpy(), rtol=2e-6, atol=0)
    assert torch.equal(sc["used"], hs["alerts"])
    gmap = E.groups(n)
    pols = [E.make_policy(ct, "linear", gmap)[0], E.make_policy(ct, "mlp64x64_sampled", gmap)[0],
            dict(kind="threshold", feature="heat_qi", threshold=0.8, require_budget=True)]
    for pol in pols:
        A.reset(options={"episodes": ep})
        out = A.rollout(pol, hindsight=True)
        assert torch.equal(out["hindsight_return"], hs["return"]), pol["kind"]
        slack = 2e-6 * out["return"].abs()
        assert bool((out["hindsight_return"] >= out["return"] - slack).all()), pol["kind"]
        assert int(out["alerts"].sum()) > 0
    assert A.check_status() == 0
    A.close()


@pytest.mark.parametrize("name", ["slot27", "ragged27"])
def test_hindsight_refuses_slot27_tables_through_rollout(dev, tabs, name):
    tb = tabs[name]
    env = _env(tb, dev, n=200 + 3)
    g = E.groups(env.num_envs)
    before = env.state_dict()
    for pol_name in ("linear", "mlp16"):
        with pytest.raises(ValueError, match="slot-27"):
            env.rollout(E.make_policy(tb.ct, pol_name, g)[0], hindsight=True)
    with pytest.raises(ValueError, match="slot-27"):
        env.hindsight_optimum()
    after = env.state_dict()
    for k in ("state", "obs", "final_return"):
        assert torch.equal(before[k], after[k]), k
    out = env.rollout(E.make_policy(tb.ct, "linear", g)[0])  # the refusal left the env usable
    assert out["done"].all() and env.check_status() == 0
    env.close()


# ------------------------------------------------------------------ everything in one call
def test_all_features_in_one_call_on_ragged_table(dev, tabs):
    """rollout(mlp, record=True, posterior_returns=True, hindsight=True, alert_mask=True) in two chained calls equals
    the four single-feature calls on twin envs bit for bit."""
    tb = tabs["ragged"]
    n = E.N_ENVS["ragged"]
    pol = E.make_policy(tb.ct, "mlp64x64_sampled", E.groups(n))[0]
    feats = (dict(record=True), dict(posterior_returns=True), dict(hindsight=True), dict(alert_mask=True))
    A = _env(tb, dev)
    twins = [_env(tb, dev) for _ in feats]
    for steps in (30, None):
        oa = A.rollout(pol, n_steps=steps, record=True, posterior_returns=True, hindsight=True, alert_mask=True)
        seen = set()
        for env, kw in zip(twins, feats):
            ob = env.rollout(pol, n_steps=steps, **kw)
            for k, v in ob.items():
                seen.add(k)
                if k == "trajectory":
                    val = v["valid"]
                    for kk in ("valid", "terminated", "alert"):
                        assert torch.equal(oa[k][kk], v[kk]), kk
                    for kk in ("action", "logit", "reward"):
                        assert torch.equal(oa[k][kk][val], v[kk][val]), kk
                    assert torch.equal(oa[k]["obs"][0], v["obs"][0]) and torch.equal(oa[k]["obs"][-1], v["obs"][-1])
                    assert torch.equal(oa[k]["obs"][1:-1][val[:-1]], v["obs"][1:-1][val[:-1]])
                    continue
                a_ = oa[k]
                if v.is_floating_point():
                    a_, v = a_.nan_to_num(7.0), v.nan_to_num(7.0)
                assert torch.equal(a_, v), (k, kw)
            sa, sb = A.state(), env.state()
            for k in sa:
                assert torch.equal(sa[k], sb[k]), k
            assert torch.equal(A._obs, env._obs) and torch.equal(A._final_return, env._final_return)
            assert env.check_status() == 0
        assert seen == set(oa)
    assert A.check_status() == 0 and oa["done"].all()
    for e in [A] + twins:
        e.close()
