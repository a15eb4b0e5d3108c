"""Every kernel that evaluates a policy inside the day loop, and step() itself, on observation layouts other than the
generator's own (tests/obs_layouts.py): columns on slots that are not their index, empty slots, n_obs of 29, 28, 8 and 5,
run-time columns in reverse order and interleaved with table columns, and the ragged variants of two of them. The
references never touch the kernel under test: the name-driven vector oracle (tests/table_edges.py), the fp64
restatements of the gradients fed by the oracle's rows, and step() on a twin. Every bound is the one the existing test
of that kernel uses. tests/test_obs_layouts_cpu.py checks the references themselves without a GPU."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import obs_layouts as L  # noqa: E402
import table_edges as E  # noqa: E402
from imitation_restatement import imitation_linear_fp64, imitation_mlp_fp64  # noqa: E402
from policy_gradient_mlp_cases import MATRIX, net as case_net  # noqa: E402
from policy_gradient_mlp_restatement import policy_gradient_mlp_fp64  # noqa: E402
from policy_gradient_restatement import forced_days, policy_gradient_fp64  # noqa: E402

from oracle import heatalert_oracle as O  # noqa: E402
from weather2alert_amd import policy  # noqa: E402

pytestmark = pytest.mark.gpu

REWARD_TOL = 1e-5  # the suite's per-day bar against fp64 (tests/test_env_gpu.py)
RETURN_RTOL, RETURN_ATOL = 2e-6, 2e-5  # as tests/test_env_gpu.py
INT_STATE = ("t", "used", "streak", "last_actual", "at_budget", "hist14", "finished")
BASELINES = ("none", "no_alert")
ALL = L.LAYOUTS + L.RAGGED
# nets of the instantiation matrix that between them reach widths 16, 32 and 64 and both layer counts
PG_NETS = ("tanh7x13", "relu29_o2", "relu40x64")
IM_NETS = ("tanh1_o2", "tanh64x33_o2")  # <16, 1> and <64, 2>
WORST = {}


def _worst(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))
    print(f"    worst ratio to the bound so far, {key}: {WORST[key]:.3e}")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tabs():
    return L.make_layouts()


def _env(tb, dev, n=L.N_ENVS, reset=True, **kw):
    from weather2alert_amd import HeatAlertVecEnv

    kw.setdefault("autoreset", "disabled")
    env = HeatAlertVecEnv(n, tables=tb.ct, device=dev, env_gid0=E.GID0, similar_climate_counties=True, **kw)
    if reset:
        env.reset(seed=L.RESET[tb.name]["seed"], options=dict(L.RESET[tb.name]["opts"]))
    return env


def _np(d, keys=None):
    return {k: d[k].cpu().numpy().astype(np.int64) for k in (keys or d) if k != "episode_return"}


def _npd(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _check_tuples(env, tup):
    st = _np(env.state())
    for k, v in tup.items():
        np.testing.assert_array_equal(st[k], v, err_msg=k)
    return st


def _ratio(diff, bound):
    return float(np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff > 0, np.inf, 0.0)).max())


# ------------------------------------------------------------------ a. reset() / step()
@pytest.mark.parametrize("n", [L.N_ENVS, 7])
@pytest.mark.parametrize("mode", ["wide", "classic", "posterior_mean"])
@pytest.mark.parametrize("name", ALL)
def test_step_parity(dev, tabs, name, mode, n):
    """reset() and T days of step() with random actions (none for an env that is over): the observation rows bit-equal
    to the oracle's f32 rows every day on each env's own days (the row a terminal step leaves included), rewards within
    1e-5, `done` and the integer state equal. n = 333 and 7: the last wave is ragged; on the ragged variants part of a
    wave has finished and keeps its row (write_me false). posterior_mean (the wide kernel only): the same, the rewards
    against the oracle's mean over every draw and the fp64 restatement."""
    tb = tabs[name]
    ct = tb.ct
    tup = L.host_tuples(tb, n)
    pm = mode == "posterior_mean"
    kw = dict(reward_mode="posterior_mean", pm_kernel="vector") if pm else dict(step_kernel=mode)
    env = _env(tb, dev, n, **kw)
    assert env._obs.shape == (n, L.N_OBS[name])
    _check_tuples(env, tup)
    V = tb.oracle("posterior_mean" if pm else "sampled")
    E.oracle_reset(V, tup)
    np.testing.assert_array_equal(env._obs.cpu().numpy(), V.obs.astype(np.float32))
    rng = np.random.default_rng(12)
    alert_days = np.zeros((n, ct.T), bool)
    rew, lives = np.zeros((ct.T, n)), np.zeros((ct.T, n), bool)
    worst, held = 0.0, 0
    for s in range(ct.T):
        act = np.where(V._finished, 0, rng.random(n) < 0.3).astype(np.int32)
        tday = V.t.copy()
        obs, r, done, _, _ = env.step(torch.as_tensor(act, device=dev))
        r64, d64, actual, live = E.oracle_step(V, act)
        alert_days[np.arange(n)[live & (actual == 1)], tday[live & (actual == 1)]] = True
        assert live.any()
        o = obs.cpu().numpy()
        np.testing.assert_array_equal(o[live], V.obs.astype(np.float32)[live], err_msg=f"day {s}")
        held += int((~live).sum())
        np.testing.assert_array_equal(done.cpu().numpy()[live], d64[live])
        rew[s], lives[s] = r.double().cpu().numpy(), live
        err = float(np.abs(rew[s] - r64)[live].max())
        worst = max(worst, err)
        assert err <= REWARD_TOL, (s, err)
        if (live & d64).any() or s == ct.T - 1:
            st, so = _np(env.state()), E.oracle_state(V)
            sel = live & d64
            for k in ("t", "used", "streak", "finished"):
                np.testing.assert_array_equal(st[k][sel], so[k][sel], err_msg=k)
    assert V._finished.all() and (held > 0) == tb.ragged
    print(f"{name} [{mode}] n={n}: max per-day |reward - oracle| = {worst:.2e}")
    _worst("step reward / 1e-5", worst / REWARD_TOL)
    if pm:
        r64, _ = E.pm_rewards_fp64(ct, E.start_state(tup), alert_days, ct.T)
        assert np.isnan(r64[~lives]).all()
        assert np.abs(rew - r64)[lives].max() <= REWARD_TOL
    assert env.check_status() == (4 if tb.ragged else 0)  # W2A_ST_STEP_AFTER_DONE on the ragged variants
    env.close()


@pytest.mark.parametrize("name", L.RAGGED)
def test_in_kernel_autoreset_step(dev, tabs, name):
    """autoreset="same_step" on a batch that is not in lock step: the terminal step of the 1-day episodes restarts them
    inside the step kernel; the row it returns is the first row of episode 1's tuple, in this layout's column order."""
    tb, n = tabs[name], L.N_ENVS
    ct, cfg = tb.ct, L.RESET[name]
    tup = L.host_tuples(tb, n)
    env = _env(tb, dev, n, autoreset="same_step")
    assert env._dev_auto
    V = tb.oracle()
    E.oracle_reset(V, tup)
    act = (np.arange(n) % 3 == 0).astype(np.int32)
    obs, r, done, _, _ = env.step(torch.as_tensor(act, device=dev))
    r64, d64, _, _ = E.oracle_step(V, act)
    one = tup["n_days"] == 1
    assert one.any() and not one.all()
    np.testing.assert_array_equal(done.cpu().numpy(), d64)
    np.testing.assert_array_equal(d64, one)
    assert np.abs(r.double().cpu().numpy() - r64).max() <= REWARD_TOL
    o = obs.cpu().numpy()
    np.testing.assert_array_equal(o[~one], V.obs.astype(np.float32)[~one])
    rows = [O.devrng_reset_tuple(cfg["seed"], E.GID0 + i, 1, ct.S, ct.Y, ct.n_samples, ct.fips_to_weather, ct.sim_ptr,
                                 ct.sim_cnt, True, lambda cw, yi: int(ct.B0[cw * ct.Y + yi]), -1, cfg["opts"]["budget"], 0)
            for i in np.nonzero(one)[0].tolist()]
    cw, cc, yi, sm, b = (np.array(c, np.int64) for c in zip(*rows))
    st = _np(env.state())
    for k, v in (("county_w", cw), ("coef_col", cc), ("year_i", yi), ("sample", sm), ("budget", b)):
        np.testing.assert_array_equal(st[k][one], v, err_msg=k)
    assert (st["episode_no"][one] == 1).all() and (st["t"][one] == 0).all() and (st["episode_no"][~one] == 0).all()
    V2 = tb.oracle()
    first = V2.reset(cw, yi, cc, sm, b)
    np.testing.assert_array_equal(o[one], first.astype(np.float32))
    assert env.check_status() == 0
    env.close()


@pytest.mark.parametrize("name", ["narrow", "n8"])
def test_drop_in_env(dev, tabs, name):
    """HeatAlertEnv(tables=...): its host record is cut at offsets computed from n_obs. Observation, reward, done and
    the decoded fields against the scalar oracle for a short episode."""
    from weather2alert_amd import HeatAlertEnv

    tb = tabs[name]
    env = HeatAlertEnv(tables=tb.ct, device=str(dev))
    ref = O.OracleEnv(tb.ref)
    fips = tb.ct.fips_list[3]
    obs, info = env.reset(location=fips, seed=31, budget=3)
    obs_o, info_o = ref.reset(location=fips, seed=31, budget=3)
    assert obs.shape == (L.N_OBS[name],) and obs.dtype == np.float32
    np.testing.assert_array_equal(obs, obs_o.astype(np.float32))
    assert info == info_o and env.feat_names == ref.feat_names
    rng = np.random.default_rng(1)
    for t in range(tb.ct.T):
        a = int(rng.random() < 0.4)
        obs, r, done, trunc, info = env.step(a)
        obs_o, r_o, done_o, _, info_o = ref.step(a)
        np.testing.assert_array_equal(obs, obs_o.astype(np.float32), err_msg=f"day {t}")
        assert abs(r - r_o) <= REWARD_TOL and done == done_o and trunc is False and info == info_o, t
        assert (env.t, env.alert_streak, env.remaining_budget, env.at_budget, env.n_days, env.coef_index) == \
            (ref.t, ref.alert_streak, ref.remaining_budget, ref.at_budget, ref.n_days, ref.coef_index), t
    assert done
    env.close()


# ------------------------------------------------------------------ b. policy rollouts
def _policy_cases():
    out = []
    for name in ALL:
        for pol_name in E.POLICIES:
            if name.replace("_ragged", "") in ("narrow", "n8") and pol_name == "mlp64x64":
                continue  # the [64, 64] net on the two narrow layouts in its sampled form only
            out.append((name, pol_name))
    return out


@pytest.mark.parametrize("name,pol_name", _policy_cases())
def test_policy_rollouts(dev, tabs, name, pol_name):
    """A whole episode in one call (A) and in two calls with a step() day in between (B: the row the first call wrote
    back is read by step(), and the row step() wrote by the second call's day-0 logit, through slot_obs). Against the
    oracle's fp64 loop, near-tie envs excepted (< 1 %): alerts, attempts over budget, both day bitmaps, the integer
    state and the observation buffer exact, returns to the suite's bars."""
    tb, n = tabs[name], L.N_ENVS
    ct = tb.ct
    tup, g = L.host_tuples(tb, n), E.groups(n)
    pol, fn, ties = L.make_policy(tb, pol_name, g)
    kernel = "k_rollout_linear" if pol["kind"] == "linear" else "k_rollout_mlp"
    uni = L.policy_uniform(tb, n) if pol["sample"] else None
    V = tb.oracle()
    E.oracle_reset(V, tup)
    R = E.oracle_record(V, fn, ct.T, ties, uniform=uni)
    ok = ~R["tie"]
    assert R["tie"].mean() < 0.01, R["tie"].sum()
    A, B = _env(tb, dev), _env(tb, dev)
    _check_tuples(A, tup)
    np.testing.assert_array_equal(A._obs.cpu().numpy(), R["obs"][0])
    oa = A.rollout(pol, alert_mask=True)
    assert A.last_rollout_kernel == kernel and A.check_status() == 0 and oa["done"].all()
    got = {k: oa[k].cpu().numpy() for k in ("return", "alerts", "attempts_over_budget", "alert_days", "attempt_days")}
    for k, ref in (("alerts", R["alerts"]), ("attempts_over_budget", R["over"]), ("alert_days", R["days"]),
                   ("attempt_days", R["att"])):
        np.testing.assert_array_equal(got[k][ok], ref[ok], err_msg=k)
    sa, so = _np(A.state()), E.oracle_state(V)
    for k in INT_STATE:
        np.testing.assert_array_equal(sa[k][ok], so[k][ok], err_msg=k)
    np.testing.assert_array_equal(A._obs.cpu().numpy()[ok], R["obs"][ct.T][ok])
    ret = got["return"].astype(np.float64)
    err = np.abs(ret - R["ret"])[ok]
    print(f"{name}/{pol_name}: max |return - oracle| = {err.max():.2e}")
    _worst("return / (2e-6 |ret| + 2e-5)", (err / (RETURN_ATOL + RETURN_RTOL * np.abs(R["ret"][ok]))).max())
    np.testing.assert_allclose(ret[ok], R["ret"][ok], rtol=RETURN_RTOL, atol=RETURN_ATOL)
    assert got["alerts"][ok].sum() > 0
    # B: k days, one step() day with the oracle policy's own decision, the rest
    k = 7
    V2 = tb.oracle()
    E.oracle_reset(V2, tup)
    R1 = E.oracle_record(V2, fn, k, ties, uniform=uni, T=ct.T)
    z, mag = fn(V2.obs.astype(np.float32))
    if uni is None:
        act, tie_mid = z > 0, np.abs(z) <= ties[0] * mag
    else:
        sg, u = 1.0 / (1.0 + np.exp(-z)), uni(V2.t).astype(np.float64)
        act, tie_mid = u < sg, np.abs(sg - u) <= ties[1]
    fin_mid = V2._finished.copy()  # step() goes on shifting the history of an env that is over; nothing else moves
    act = (act & ~fin_mid).astype(np.int32)
    ob1 = B.rollout(pol, n_steps=k, alert_mask=True)
    np.testing.assert_array_equal(B._obs.cpu().numpy()[~R1["tie"]], V2.obs.astype(np.float32)[~R1["tie"]])
    B.step(torch.as_tensor(act, device=dev))
    assert B.check_status() == (4 if tb.ragged else 0)  # the step() day went past the shortest episodes
    E.oracle_step(V2, act)
    R2 = E.oracle_record(V2, fn, ct.T, ties, uniform=uni, T=ct.T)
    ob2 = B.rollout(pol, alert_mask=True)
    ok2 = ~(R1["tie"] | R2["tie"] | (tie_mid & (R1["valid"].sum(0) == k)))
    assert B.last_rollout_kernel == kernel and ok2.mean() > 0.98 and ob2["done"].all()
    sb, so2 = _np(B.state()), E.oracle_state(V2)
    for kk in INT_STATE:
        sel = ok2 & ~fin_mid if kk in ("hist14", "last_actual", "at_budget") else ok2
        np.testing.assert_array_equal(sb[kk][sel], so2[kk][sel], err_msg=kk)
    np.testing.assert_array_equal(B._obs.cpu().numpy()[ok2], V2.obs.astype(np.float32)[ok2])
    days_b = (ob1["alert_days"] | ob2["alert_days"]).cpu().numpy()
    np.testing.assert_array_equal(days_b[ok2], (R1["days"] | R2["days"])[ok2])  # the step() day is in neither bitmap
    np.testing.assert_array_equal(ob1["alerts"].cpu().numpy()[ok2], R1["alerts"][ok2])
    np.testing.assert_array_equal(ob2["alerts"].cpu().numpy()[ok2], R2["alerts"][ok2])
    np.testing.assert_allclose(ob1["return"].double().cpu().numpy()[ok2], R1["ret"][ok2], rtol=RETURN_RTOL, atol=RETURN_ATOL)
    np.testing.assert_allclose(ob2["return"].double().cpu().numpy()[ok2], R2["ret"][ok2], rtol=RETURN_RTOL, atol=RETURN_ATOL)
    # whole and split agree with each other wherever both agree with the oracle
    for kk in INT_STATE:
        both = ok & ok2 & ~fin_mid if kk in ("hist14", "last_actual", "at_budget") else ok & ok2
        np.testing.assert_array_equal(sa[kk][both], sb[kk][both], err_msg=kk)
    assert B.check_status() == 0
    A.close()
    B.close()


@pytest.mark.parametrize("name", L.LAYOUTS)
def test_threshold_policy_finds_its_column(dev, tabs, name):
    """kind="threshold" looks its feature's observation column up in obs_slot (w2a_rollout and the per-day
    w2a_policy_actions path of a posterior_mean env on the fp64 matrix kernel): heat_qi, and a table column whose
    observation column differs from its slot on this layout, against the oracle's built-in rollout."""
    tb, n = tabs[name], L.N_ENVS
    ct = tb.ct
    tup = L.host_tuples(tb, n)
    feats = ["heat_qi"]
    c = L.offset_column(ct)
    if c is not None:
        feats.append(ct.columns[c])
    assert name == "narrow" or len(feats) == 2
    if name == "n8":
        assert ct.columns.index("heat_qi") == 1 and ct.obs_slot[1] == 0
    for feat in feats:
        col = ct.columns.index(feat)
        vals = ct.X[:, :, ct.obs_slot[col]]
        thr = float(np.quantile(vals, 0.7))
        pol = dict(kind="threshold", feature=feat, threshold=thr, require_budget=True)
        V = tb.oracle()
        E.oracle_reset(V, tup)
        ref = E.oracle_builtin_rollout(V, dict(pol, col=col), ct.T)
        Vp = tb.oracle("posterior_mean")
        E.oracle_reset(Vp, tup)
        refp = E.oracle_builtin_rollout(Vp, dict(pol, col=col), ct.T)
        assert ref["alerts"].sum() > 0
        for pm in (False, True):
            kw = dict(reward_mode="posterior_mean", pm_kernel="matrix") if pm else {}
            env = _env(tb, dev, **kw)
            out = env.rollout(pol, alert_mask=True)
            if pm:
                assert env.last_pm_rollout == "per_day"
            want = refp if pm else ref
            np.testing.assert_array_equal(out["alerts"].cpu().numpy(), want["alerts"], err_msg=feat)
            np.testing.assert_array_equal(out["alert_days"].cpu().numpy(), want["days"], err_msg=feat)
            np.testing.assert_array_equal(out["attempts_over_budget"].cpu().numpy(), want["over"], err_msg=feat)
            np.testing.assert_allclose(out["return"].double().cpu().numpy(), want["ret"], rtol=RETURN_RTOL, atol=RETURN_ATOL)
            assert env.check_status() == 0
            env.close()


# ------------------------------------------------------------------ c. recorded trajectories
GUARD = 64 * 32  # floats behind the trajectory's last row


@pytest.mark.parametrize("design", ["staged", "direct"])
@pytest.mark.parametrize("pol_name", ["linear_sampled", "mlp16"])
@pytest.mark.parametrize("name", ALL)
def test_recorded_trajectories(dev, tabs, name, pol_name, design, monkeypatch):
    """Four step() days with random actions (the shortest episodes of the ragged variants are over on entry), then the
    rest recorded in one call, with the staged store (identity visiting order) and the direct one (rollout_order=True,
    lockstep=False): obs bit-equal to the oracle's rows wherever the contract defines it, actions and flags exact,
    rewards and logits within their bars. Staged: the trajectory tensor is a view into a larger buffer whose patterned
    guard region behind the last row must stay untouched (the last wave's tile holds min(left, 64) * n_obs floats)."""
    tb, n = tabs[name], L.N_ENVS
    ct = tb.ct
    tup, g = L.host_tuples(tb, n), E.groups(n)
    pol, fn, ties = L.make_policy(tb, pol_name, g)
    kw = dict(rollout_order=True, lockstep=False) if design == "direct" else {}
    A = _env(tb, dev, **kw)
    V = tb.oracle()
    E.oracle_reset(V, tup)
    rng = np.random.default_rng(9)
    for _ in range(4):
        a = np.where(V._finished, 0, rng.random(n) < 0.3).astype(np.int32)
        A.step(torch.as_tensor(a, device=dev))
        E.oracle_step(V, a)
    assert A.check_status() == (4 if tb.ragged else 0)
    s0 = _np(A.state())
    fin0 = s0["finished"] == 1
    assert fin0.any() == tb.ragged and (s0["hist14"] != 0).any()
    S = ct.T
    R = E.oracle_record(V, fn, S, ties, uniform=L.policy_uniform(tb, n) if pol["sample"] else None, T=ct.T)
    ok = ~R["tie"]
    assert R["tie"].mean() < 0.01, R["tie"].sum()
    entry = A._obs.cpu().numpy()
    bufs = []
    real_empty = torch.empty

    def guarded_empty(*size, **kwargs):
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        if shape == (S + 1, n, ct.n_obs) and kwargs.get("dtype") == torch.float32:
            numel = (S + 1) * n * ct.n_obs
            buf = real_empty(numel + GUARD, **kwargs)
            buf[numel:] = torch.arange(GUARD, dtype=torch.float32, device=buf.device) + 0.5
            bufs.append((buf, numel))
            return buf[:numel].view(shape)
        return real_empty(*size, **kwargs)

    monkeypatch.setattr(torch, "empty", guarded_empty)
    oa = A.rollout(pol, record=True, alert_mask=True)
    monkeypatch.setattr(torch, "empty", real_empty)
    assert A.check_status() == 0 and oa["done"].all()
    assert len(bufs) == 1
    buf, numel = bufs[0]
    assert torch.equal(buf[numel:], torch.arange(GUARD, dtype=torch.float32, device=buf.device) + 0.5)
    tr = _npd(oa["trajectory"])
    assert tr["obs"].shape == (S + 1, n, ct.n_obs)
    left = np.where(fin0, 0, s0["n_days"] - s0["t"])
    assert (tr["valid"] == (np.arange(S)[:, None] < left[None, :])).all()
    np.testing.assert_array_equal(tr["terminated"].sum(0), (left > 0).astype(np.int64))
    v = R["valid"][:, ok]
    for k in ("valid", "terminated", "alert", "action"):
        np.testing.assert_array_equal(tr[k][:, ok] * (v if k == "action" else 1), R[k][:, ok], err_msg=k)
    assert R["alert"][:, ok].any() and (R["alert"][:, ok] < v).any()
    assert not (tr["terminated"] & ~tr["valid"]).any() and not (tr["alert"] & ~tr["valid"]).any()
    np.testing.assert_array_equal(tr["obs"][:-1, ok][v], R["obs"][:-1, ok][v])
    np.testing.assert_array_equal(tr["obs"][0], entry)
    np.testing.assert_array_equal(tr["obs"][S], A._obs.cpu().numpy())
    np.testing.assert_array_equal(tr["obs"][S][ok & ~fin0], R["obs"][S][ok & ~fin0])
    sT, eT = np.nonzero(tr["terminated"])
    np.testing.assert_array_equal(tr["obs"][sT + 1, eT], tr["obs"][sT, eT])  # the row after a terminal step repeats
    np.testing.assert_array_equal(tr["obs"][S][fin0], entry[fin0])
    rv = R["valid"][:, ok]
    err = np.abs(tr["reward"][:, ok][rv] - R["reward"][:, ok][rv])
    print(f"{name}/{pol_name}/{design}: max per-day |reward - oracle| = {err.max():.2e}")
    _worst("recorded reward / 1e-5", (err / (REWARD_TOL + REWARD_TOL * np.abs(R["reward"][:, ok][rv]))).max())
    np.testing.assert_allclose(tr["reward"][:, ok][rv], R["reward"][:, ok][rv], rtol=REWARD_TOL, atol=REWARD_TOL)
    lg, z, mag = tr["logit"][:, ok][v].astype(np.float64), R["logit"][:, ok][v], R["mag"][:, ok][v]
    if pol["kind"] == "linear":  # the fp64 logit rounded to f32
        assert (np.abs(lg - z) <= 1e-6 * np.abs(z) + 1e-9 * mag).all()
    else:  # the f32 network, within the near-tie band of include/w2a.h
        assert (np.abs(lg - z) <= 1e-5 * mag).all()
    A.close()


# ------------------------------------------------------------------ d. policy_gradient
def _never(ct):
    return dict(kind="linear", weight=np.zeros((1, ct.n_obs), np.float32), bias=np.array([-1.0], np.float32))


def _oracle_replay(V, tup, pre, actions, S):
    """V reset to the batch's episodes, the prefix's actions replayed, then `actions` [S, N] (None: no alerts): fp64
    rows held before every decision, rewards and valid flags of the S days."""
    E.oracle_reset(V, tup)
    n = len(tup["budget"])
    for a in ([] if pre is None else pre):
        E.oracle_step(V, a.astype(np.int64))
    obs, rew, valid = np.zeros((S, n, V.obs.shape[1])), np.zeros((S, n)), np.zeros((S, n), bool)
    for s in range(S):
        obs[s] = V.obs
        act = np.zeros(n, np.int64) if actions is None else actions[s].astype(np.int64)
        r, _, _, live = E.oracle_step(V, np.where(V._finished, 0, act))
        rew[s], valid[s] = np.where(live, r, 0.0), live
    return obs, rew, valid


def _pg_case(dev, tb, pol, prefix, what):
    """the recorded-twin scheme with every float from the oracle: B records (the prefix too), the oracle replays B's
    actions for the rows and rewards and runs once more with no alerts for the baseline; A1 / A2 take the gradient.
    Returns baseline -> (out, fp64 inputs of the restatement)."""
    n = L.N_ENVS
    ct, tup = tb.ct, L.host_tuples(tb, n)
    envs = [_env(tb, dev) for _ in range(3)]
    A, B = dict(zip(BASELINES, envs[:2])), envs[2]
    pre = None
    if prefix:
        for e_ in envs[:2]:
            e_.rollout(pol, n_steps=prefix)
        pre = _npd(B.rollout(pol, n_steps=prefix, record=True)["trajectory"])["action"]
    st0 = _np(B.state())
    tr = _npd(B.rollout(pol, record=True)["trajectory"])
    S = tr["valid"].shape[0]
    V = tb.oracle()
    obs, rew, valid = _oracle_replay(V, tup, pre, tr["action"] * tr["valid"], S)
    _, beta, valid0 = _oracle_replay(V, tup, pre, None, S)
    np.testing.assert_array_equal(valid, tr["valid"])
    np.testing.assert_array_equal(valid0, tr["valid"])
    np.testing.assert_array_equal(obs[valid].astype(np.float32), tr["obs"][:S][valid])
    assert tr["alert"].any() and valid.any()
    forced = forced_days(pol.get("require_budget", False), st0["budget"], st0["used"], tr["alert"], tr["valid"])
    out = {}
    for bl in BASELINES:
        o = A[bl].rollout(pol, policy_gradient=bl)
        assert A[bl].check_status() == 0
        np.testing.assert_array_equal(o["alerts"].cpu().numpy(), (tr["alert"] & tr["valid"]).sum(axis=0))
        out[bl] = o
    for e_ in envs:
        e_.close()
    return out, dict(obs=obs, action=tr["action"], valid=valid, forced=forced, rew=rew, beta=beta)


def _lin_within(out, ref, G, n_obs, what, key):
    g = out["policy_gradient"]
    assert g["weight"].shape == (G, n_obs) and g["bias"].shape == (G,) and g["weight"].dtype == torch.float32
    got = np.concatenate([g["weight"].double().cpu().numpy(), g["bias"].double().cpu().numpy()[:, None]], axis=1)
    want = np.concatenate([ref["weight"], ref["bias"][:, None]], axis=1)
    assert np.isfinite(got).all() and np.isfinite(want).all(), what
    diff = np.abs(got - want)
    r = _ratio(diff, ref["bound"])
    print(f"{what}: max |g - g_ref| / bound = {r:.3e}   (max |g_ref| = {np.abs(want).max():.3e})")
    _worst(key, r)
    assert (diff <= ref["bound"]).all(), (what, r)
    return got


def _mlp_within(out, ref, layers, what, key):
    got = [(dW.double().cpu().numpy(), db.double().cpu().numpy()) for dW, db in out["policy_gradient"]["layers"]]
    assert [(a.shape, b.shape) for a, b in got] == [(W.shape, b.shape) for W, b in layers], what
    ratio = 0.0
    for (dW, db), (rW, rb), (bW, bb) in zip(got, ref["layers"], ref["bound"]):
        for x, r, bd in ((dW, rW, bW), (db, rb, bb)):
            assert np.isfinite(x).all() and np.isfinite(r).all(), what
            diff = np.abs(x - r)
            ratio = max(ratio, _ratio(diff, bd))
            assert (diff <= bd).all(), (what, ratio)
    print(f"{what}: max |g - g_ref| / bound = {ratio:.3e}")
    _worst(key, ratio)
    return got


@pytest.mark.parametrize("prefix", [0, 9])
@pytest.mark.parametrize("name", L.LAYOUTS)
def test_policy_gradient_linear(dev, tabs, name, prefix):
    """k_policy_gradient_linear, G = 5 interleaved groups, both baselines, from reset and after a 9-day prefix: shape
    [G, n_obs], every component inside the restatement's bound on the oracle's fp64 rows and rewards."""
    tb = tabs[name]
    ct, g = tb.ct, E.groups(L.N_ENVS)
    W, b = E.linear_params(ct)
    pol = dict(kind="linear", weight=W, bias=b, group=g, sample=True, seed=L.policy_seed(name), require_budget=prefix > 0)
    out, x = _pg_case(dev, tb, pol, prefix, name)
    got = {}
    for bl in BASELINES:
        ref = policy_gradient_fp64(x["obs"], x["action"], x["valid"], x["forced"], x["rew"],
                                   x["beta"] if bl == "no_alert" else None, W, b, g, E.G)
        got[bl] = _lin_within(out[bl], ref, E.G, ct.n_obs, f"{name} prefix={prefix} {bl}", "policy_gradient linear")
    assert np.abs(got["none"] - got["no_alert"]).max() > 0


def _single_columns(ct):
    """a table column whose slot differs from its index, a run-time column, and `alert_2wks`"""
    c = L.offset_column(ct)
    cols = [] if c is None else [c]
    return cols + [ct.feature_names.index("alert_streak"), ct.n_obs - 1]


@pytest.mark.parametrize("name", L.LAYOUTS)
def test_policy_on_one_column_alone(dev, tabs, name):
    """A linear policy whose weight is zero except on one observation column c must act, pay and differentiate as the
    reference evaluated with that column alone: logit = w obs[:, c] + b computed from the oracle's named column. Pins
    the identity of the column, with no random matrix to hide behind."""
    tb, n = tabs[name], L.N_ENVS
    ct = tb.ct
    tup = L.host_tuples(tb, n)
    for c in _single_columns(ct):
        cname = ct.feature_names[c]
        col = ct.X[:, :, ct.obs_slot[c]].ravel() if ct.obs_slot[c] < 24 else np.array([0.0, 1.0, 2.0])
        scale = 2.0 / max(float(col.max() - col.min()), 1e-3)
        W = np.zeros((1, ct.n_obs), np.float32)
        W[0, c] = scale
        b = np.array([-scale * float(np.median(col)) - 0.3], np.float32)
        pol = dict(kind="linear", weight=W, bias=b, sample=True, seed=L.policy_seed(name))
        w64, b64 = float(W[0, c]), float(b[0])

        def fn(obs, c=c, w64=w64, b64=b64):
            x = obs[:, c].astype(np.float64)
            return w64 * x + b64, np.abs(w64 * x) + abs(b64)

        V = tb.oracle()
        E.oracle_reset(V, tup)
        R = E.oracle_record(V, fn, ct.T, (1e-9, 1e-6), uniform=L.policy_uniform(tb, n))
        ok = ~R["tie"]
        assert R["tie"].mean() < 0.01 and R["alert"].any(), cname
        assert np.ptp(R["logit"][R["valid"]]) > 0.1, cname  # the column moves the logit
        A, B = _env(tb, dev), _env(tb, dev)
        oa = A.rollout(pol, alert_mask=True, policy_gradient="none")
        np.testing.assert_array_equal(oa["alerts"].cpu().numpy()[ok], R["alerts"][ok], err_msg=cname)
        np.testing.assert_array_equal(oa["attempt_days"].cpu().numpy()[ok], R["att"][ok], err_msg=cname)
        np.testing.assert_allclose(oa["return"].double().cpu().numpy()[ok], R["ret"][ok], rtol=RETURN_RTOL, atol=RETURN_ATOL)
        np.testing.assert_array_equal(A._obs.cpu().numpy()[ok], R["obs"][ct.T][ok])
        if ok.all():  # the gradient averages over every env: only when none is a near-tie
            only = R["obs"][:ct.T].astype(np.float64)[:, :, c:c + 1]
            ref1 = policy_gradient_fp64(only, R["action"], R["valid"], np.zeros_like(R["valid"]), R["reward"], None,
                                        W[:, c:c + 1], b, None, 1)
            full = policy_gradient_fp64(R["obs"][:ct.T].astype(np.float64), R["action"], R["valid"], np.zeros_like(R["valid"]),
                                        R["reward"], None, W, b, None, 1)
            pg = oa["policy_gradient"]
            gc = float(pg["weight"][0, c].double())
            assert abs(gc - ref1["weight"][0, 0]) <= ref1["bound"][0, 0], cname
            assert abs(float(pg["bias"][0].double()) - ref1["bias"][0]) <= ref1["bound"][0, 1], cname
            _lin_within(oa, full, 1, ct.n_obs, f"{name} column {cname} alone", "policy_gradient linear")
        # the same column through imitation_gradient along the oracle's own attempts
        sched = torch.as_tensor(R["att"], device=dev)
        out = B.imitation_gradient(dict(kind="linear", weight=W, bias=b), sched)
        lab = R["action"].astype(bool) & R["valid"]
        refi = imitation_linear_fp64(R["obs"][:ct.T].astype(np.float64), lab, R["valid"], np.zeros_like(R["valid"]), None,
                                     W, b, None, 1)
        gi = out["policy_gradient"]["weight"].double().cpu().numpy()
        assert (np.abs(gi - refi["weight"]) <= refi["bound"][:, :-1]).all(), cname  # a given schedule: no near-ties
        assert abs(gi[0, c]) > 0
        A.close()
        B.close()


@pytest.mark.parametrize("net", PG_NETS)
@pytest.mark.parametrize("name", L.LAYOUTS)
def test_policy_gradient_mlp(dev, tabs, name, net):
    """k_pgm_pass1 / k_pgm_pass2 with the first layer's fan-in at the layout's n_obs: dW of the first layer has shape
    [G, h, n_obs]; every parameter inside the restatement's bound, both baselines, from reset (one-layer nets) or after
    a 9-day prefix (two-layer nets)."""
    pair, hidden, act, n_out = MATRIX[net]
    assert (policy.mlp_width(hidden), len(hidden)) == pair
    tb = tabs[name]
    ct, g = tb.ct, E.groups(L.N_ENVS)
    layers = case_net(ct, net, hidden, n_out)
    assert layers[0][0].shape == (E.G, hidden[0], ct.n_obs)
    prefix = 9 if len(hidden) == 2 else 0
    pol = dict(kind="mlp", layers=layers, activation=act, group=g, sample=True, seed=L.policy_seed(name),
               require_budget=net == "relu29_o2")
    out, x = _pg_case(dev, tb, pol, prefix, f"{name} {net}")
    got = {}
    for bl in BASELINES:
        ref = policy_gradient_mlp_fp64(x["obs"], x["action"], x["valid"], x["forced"], x["rew"],
                                       x["beta"] if bl == "no_alert" else None, layers, act, g, E.G)
        got[bl] = _mlp_within(out[bl], ref, layers, f"{name} {net} prefix={prefix} {bl}", "policy_gradient mlp")
        assert got[bl][0][0].shape == (E.G, hidden[0], ct.n_obs)
    assert max(np.abs(a - b_).max() for (a, _), (b_, _) in zip(got["none"], got["no_alert"])) > 0


# ------------------------------------------------------------------ e. imitation_gradient
def _step_reference(env, sched, S, require_budget):
    """`env` stepped through step() along `sched` for at most S days; every env read on its own days only (as
    tests/test_imitation_gpu.py). Returns numpy obs f64 [S, n, n_obs], labels / valid / forced [S, n]."""
    n, dv = env.num_envs, env.device
    rows = torch.arange(n, device=dv)
    fin = env.state()["finished"].bool()
    R = dict(obs=torch.zeros((S, n, env._obs.shape[1]), dtype=torch.float64, device=dv),
             labels=torch.zeros((S, n), dtype=torch.bool, device=dv), valid=torch.zeros((S, n), dtype=torch.bool, device=dv),
             forced=torch.zeros((S, n), dtype=torch.bool, device=dv))
    for s in range(S):
        if bool(fin.all()):
            break
        st = env.state()
        R["obs"][s] = env._obs.double()
        R["valid"][s] = ~fin
        R["labels"][s] = sched[rows, st["t"].long().clamp(max=sched.shape[1] - 1)] & ~fin
        if require_budget:
            R["forced"][s] = ((st["budget"] - st["used"]) <= 0) & ~fin
        term = env.step((R["labels"][s] & ~R["forced"][s]).to(torch.int32))[2]
        fin = fin | term.bool()
    return {k: v.cpu().numpy() for k, v in R.items()}


def _check_ll(out, ref, what):
    ll, days = out["log_likelihood"].double().cpu().numpy(), out["days"].cpu().numpy()
    np.testing.assert_array_equal(days, ref["days"], err_msg=what)
    diff = np.abs(ll - ref["ll"])
    assert (diff <= ref["ll_bound"]).all(), (what, _ratio(diff, ref["ll_bound"]))
    _worst("imitation log-likelihood", _ratio(diff, ref["ll_bound"]))


IM_CASES = {"random_rb": ("random", True), "ones": ("ones", False)}


@pytest.mark.parametrize("case", list(IM_CASES))
@pytest.mark.parametrize("kind", ["linear"] + list(IM_NETS))
@pytest.mark.parametrize("name", L.LAYOUTS)
def test_imitation_gradient(dev, tabs, name, kind, case):
    """k_imitation_linear and k_im_pass1 + the second pass of the MLP gradient (<16, 1> and <64, 2>) against a twin
    stepped through step() along the schedule -- whose rows test_step_parity holds to the oracle on this layout -- after a
    5-day prefix: a random schedule with require_budget and the all-ones schedule without, mixed weights."""
    sched_kind, rb = IM_CASES[case]
    tb, n = tabs[name], 193
    ct = tb.ct
    A, B = _env(tb, dev, n), _env(tb, dev, n)
    rng = np.random.default_rng(13)
    for _ in range(5):
        a = torch.as_tensor((rng.random(n) < 0.4).astype(np.int32), device=dev)
        A.step(a)
        B.step(a)
    g = E.groups(n)
    sched = (torch.ones((n, ct.T), dtype=torch.bool, device=dev) if sched_kind == "ones"
             else torch.as_tensor(np.random.default_rng(21).random((n, ct.T)) < 0.35, device=dev))
    w = np.random.default_rng(8).standard_normal(n).astype(np.float32)
    w[::5] = 0.0
    what = f"{name} {kind} {case}"
    if kind == "linear":
        W, b = E.linear_params(ct)
        out = A.imitation_gradient(dict(kind="linear", weight=W, bias=b, group=g, require_budget=rb), sched, env_weight=w)
    else:
        _, hidden, act, n_out = MATRIX[kind]
        layers = case_net(ct, kind, hidden, n_out)
        out = A.imitation_gradient(dict(kind="mlp", layers=layers, activation=act, group=g, require_budget=rb), sched, env_weight=w)
    assert A.check_status() == 0
    R = _step_reference(B, sched, ct.T, rb)
    assert R["valid"].any() and (R["forced"].any() == rb)
    if sched_kind == "ones":
        assert (R["labels"] & R["valid"]).sum() > R["valid"][0].sum() * 6  # attempts over the budget of 6
    if kind == "linear":
        ref = imitation_linear_fp64(R["obs"], R["labels"], R["valid"], R["forced"], w, W, b, g, E.G)
        gd = out["policy_gradient"]
        assert gd["weight"].shape == (E.G, ct.n_obs)
        got = np.concatenate([gd["weight"].double().cpu().numpy(), gd["bias"].double().cpu().numpy()[:, None]], axis=1)
        want = np.concatenate([ref["weight"], ref["bias"][:, None]], axis=1)
        diff = np.abs(got - want)
        r = _ratio(diff, ref["bound"])
        print(f"{what}: max |g - g_ref| / bound = {r:.3e}")
        _worst("imitation linear", r)
        assert (diff <= ref["bound"]).all(), (what, r)
    else:
        ref = imitation_mlp_fp64(R["obs"], R["labels"], R["valid"], R["forced"], w, layers, act, g, E.G)
        assert ref["near_kink"] < 0.01
        _mlp_within(out, ref, layers, what, "imitation mlp")
    _check_ll(out, ref, what)
    A.close()
    B.close()


# ------------------------------------------------------------------ f. refusals
def test_layouts_the_policy_kernels_cannot_serve_are_refused(dev, tabs):
    """An observation column on slot 30: step() serves it (the row is a gather of 32 slots); every policy entry refuses
    it (rollout, the gradient and imitation calls, value_gradient on both its paths, surrogate_gradient,
    fisher_vector_product and q_gradient) -- the host check of policy.slot_map first, and with that check out of the way the
    library's own schema error -- and nothing is written. An obs_slot that is not injective is refused by w2a_create."""
    from weather2alert_amd import HeatAlertVecEnv, _ffi

    tb, n = tabs["narrow"], 70
    ct = tb.ct
    bad = dataclasses.replace(ct, obs_slot=[0, 26, 25, 24, 30])  # `alert_2wks` reads the gate flag's slot
    env = HeatAlertVecEnv(n, tables=bad, device=dev, autoreset="disabled", env_gid0=E.GID0, similar_climate_counties=True)
    env.reset(seed=L.RESET["narrow"]["seed"], options=dict(L.RESET["narrow"]["opts"]))
    tup = L.host_tuples(tb, n)
    V = tb.oracle()
    E.oracle_reset(V, tup)
    for s in range(3):
        a = (np.arange(n) % 2 == s % 2).astype(np.int32)
        obs, r, _, _, _ = env.step(torch.as_tensor(a, device=dev))
        r64 = E.oracle_step(V, a)[0]
        o = obs.cpu().numpy()
        np.testing.assert_array_equal(o[:, :4], V.obs.astype(np.float32)[:, :4])
        rows = tup["county_w"] * ct.Y + tup["year_i"]
        np.testing.assert_array_equal(o[:, 4], ct.X[s, rows, 30])  # the slot-30 value of the day just played
        assert np.abs(r.double().cpu().numpy() - r64).max() <= REWARD_TOL
    g = E.groups(n)
    W, b = E.linear_params(ct)
    lin = dict(kind="linear", weight=W, bias=b, group=g, sample=True)
    layers = E.net(ct, (16,), 1, seed=4)
    mlp = dict(kind="mlp", layers=layers, activation="tanh", group=g, sample=True)
    sched = torch.zeros((n, ct.T), dtype=torch.bool, device=dev)
    calls = [lambda: env.rollout(lin), lambda: env.rollout(mlp), lambda: env.rollout(lin, record=True),
             lambda: env.rollout(lin, policy_gradient=True), lambda: env.rollout(mlp, policy_gradient=True),
             lambda: env.imitation_gradient(lin, sched), lambda: env.imitation_gradient(mlp, sched)]
    # the critic, PPO, Fisher and Q entry points, linear and MLP where both exist, the plain and the GAE path of the critic
    adv = np.zeros((ct.T, n), np.float32)
    vec_lin = {"weight": np.ones_like(W), "bias": np.ones_like(b)}
    vec_mlp = {"layers": [(np.ones_like(Wl), np.ones_like(bl)) for Wl, bl in layers]}
    qnet = dict(kind="mlp", layers=E.net(ct, (16,), 2, seed=4), activation="tanh", group=g)
    gae = dict(gamma=0.97, gae_lambda=0.9, bootstrap=True, n_steps=7)
    lin2, mlp2 = ({k: v for k, v in p.items() if k != "sample"} for p in (lin, mlp))
    calls += [lambda: env.value_gradient(lin2, sched), lambda: env.value_gradient(mlp2, sched),
              lambda: env.value_gradient(lin2, sched, **gae), lambda: env.value_gradient(mlp2, sched, **gae),
              lambda: env.surrogate_gradient(lin2, sched, adv), lambda: env.surrogate_gradient(mlp2, sched, adv),
              lambda: env.fisher_vector_product(lin2, sched, vec_lin), lambda: env.fisher_vector_product(mlp2, sched, vec_mlp),
              lambda: env.q_gradient(qnet, sched), lambda: env.q_gradient(qnet, sched, target_net=dict(qnet), double=True)]
    before = env.state_dict()
    obs0 = env._obs.clone()
    for call in calls:
        with pytest.raises(ValueError, match="one-to-one into slots 0..29"):
            call()
    env.ct = ct  # the host's check sees a layout it accepts; the handle still holds slot 30
    for call in calls:
        with pytest.raises(_ffi.W2AError, match="slot 30 or 31"):
            call()
    env.ct = bad
    after = env.state_dict()
    for k in ("state", "obs", "final_return"):
        assert torch.equal(before[k], after[k]), k
    assert torch.equal(env._obs, obs0) and env.check_status() == 0
    env.step(torch.zeros(n, dtype=torch.int32, device=dev))  # the refusals left the env usable
    env.close()
    twice = dataclasses.replace(ct, obs_slot=[0, 26, 25, 24, 26])
    with pytest.raises(_ffi.W2AError, match="injective"):
        HeatAlertVecEnv(n, tables=twice, device=dev, autoreset="disabled")
