"""reward_mode="posterior_mean" on the table edges of tests/table_edges.py. About a third of the library's kernels serve
that mode -- k_pm_prep, k_posterior_mean_v, k_posterior_mean<7|8>, k_posterior_mean_i8, the one-launch rollouts
k_pm_rollout and k_pm_rollout_i8 (each with its own copy of the env's day loop) and the per-day sequence
k_policy_actions -> reward kernel -> w2a_step(REWARD_GIVEN | SKIP_FINISHED) -- and until now they only met uniform
episode lengths and a zero coefficient on slot 27 (the agent's 14-day alert count). Here: ragged lengths inside one
tile (20..153 days and 1, 2, 3), coefficient columns with a slot-27 term next to columns with the large heat_qi / bias
pair (the int8 kernels then run their matrix-core path and their exact fp64 path in ONE launch: E.pi8_flagged_columns),
both together, mid-episode entry with a live 14-day window, and the fixed-point ranges of the run-time slots.

The reference is E.pm_rewards_fp64: the draw-mean of the fp64 restatement's per-day rewards
(tests/posterior_restatement.py), slot 27 included -- the posterior-mean oracle has no slot-27 key and is right only
on the `known` envs; it is held next to the restatement there and serves every decision (tests/test_table_edges_cpu.py
checks both references without a GPU). The built-in policy kinds decide on table-sourced columns, the remaining budget
and the device RNG, which the oracle restates exactly: no env is excepted anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402

pytestmark = pytest.mark.gpu

REWARD_TOL = 1e-5  # the suite's per-day bar against fp64 (tests/test_env_gpu.py)
RETURN_RTOL, RETURN_ATOL = 2e-6, 2e-5  # as tests/test_env_gpu.py
INT_STATE = ("t", "used", "streak", "last_actual", "at_budget", "hist14", "finished")
INT_OUT = ("alerts", "attempts_over_budget", "alert_days", "attempt_days")
NAMES = ["ragged", "slot27", "ragged27"]
# pm_kernel -> ((pm_rollout_kernel, what last_pm_rollout must say), ...): the fp64 matrix kernel has no one-launch form,
# rollout() falls through to the per-day calls by itself
PATHS = {"vector": ((True, "k_pm_rollout"), (False, "per_day")), "matrix": ((True, "per_day"),),
         "matrix_i8": ((True, "k_pm_rollout_i8"), (False, "per_day"))}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tabs():
    """the three tables, built once"""
    return E.make_tables()


@pytest.fixture(scope="module")
def refs(tabs):
    """host references, each computed once and shared (never written to): ("step", table) -> E.pm_step_reference,
    ("roll", table, kind) -> the posterior-mean oracle's policy loop over whole episodes"""
    cache = {}

    def get(what, name, kind=None):
        key = (what, name, kind)
        if key not in cache:
            tb = tabs[name]
            n = E.N_ENVS[name]
            if what == "step":
                cache[key] = E.pm_step_reference(tb, n)
            else:
                V = tb.oracle("posterior_mean")
                E.oracle_reset(V, E.host_tuples(tb, n))
                pol = E.builtin_policies(tb.ct)[kind]
                cache[key] = E.oracle_builtin_rollout(V, E.oracle_policy(tb.ct, pol), tb.ct.T, E.PolicyStream(n))
                cache[key]["t"] = V.t.copy()
        return cache[key]
    return get


def _env(tb, dev, pm_kernel=None, one_launch=True, reset=True):
    """A fresh env on the table's batch (tests/table_edges.py: RESET, N_ENVS); pm_kernel=None: the sampled-reward twin."""
    from weather2alert_amd import HeatAlertVecEnv

    kw = dict(reward_mode="posterior_mean", pm_kernel=pm_kernel) if pm_kernel else {}
    env = HeatAlertVecEnv(E.N_ENVS[tb.name], tables=tb.ct, device=dev, autoreset="disabled", env_gid0=E.GID0,
                          similar_climate_counties=True, **kw)
    env.pm_rollout_kernel = one_launch
    if pm_kernel:
        assert env.pm_kernel_choice == pm_kernel and env.last_pm_rollout is None
    if reset:
        env.reset(seed=E.RESET[tb.name]["seed"], options=dict(E.RESET[tb.name]["opts"]))
    return env


def _np(d, keys=None):
    return {k: d[k].cpu().numpy().astype(np.int64) for k in (keys or d) if k != "episode_return"}


def _check_tuples(env, tup):
    st = _np(env.state())
    for k, v in tup.items():
        np.testing.assert_array_equal(st[k], v, err_msg=k)
    return st


def _bars(got, ref, what):
    np.testing.assert_allclose(np.asarray(got, np.float64), ref, rtol=RETURN_RTOL, atol=RETURN_ATOL, err_msg=what)


# ------------------------------------------------------------------ a. step() on every reward kernel
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("pm_kernel", ["vector", "matrix", "matrix_i8"])
def test_step_rewards_on_table_edges(dev, tabs, refs, pm_kernel, name):
    """k_pm_prep + each reward kernel + w2a_step(REWARD_GIVEN), ct.T days of random actions (p = 0.3, none for an env
    that is over) on a posterior_mean env and a sampled twin from one seed: every day every live env's reward within
    1e-5 of the fp64 reference (and of the oracle where it knows the coefficients); observation rows, `done` and the
    integer state bit-equal to the twin on each env's own days; episode_return within the return bars."""
    tb = tabs[name]
    ct, n = tb.ct, E.N_ENVS[name]
    R = refs("step", name)
    known = R["known"]
    pm, sm = _env(tb, dev, pm_kernel), _env(tb, dev)
    for e in (pm, sm):
        _check_tuples(e, R["tup"])
    assert torch.equal(pm._obs, sm._obs)
    worst = worst_o = 0.0
    er = np.zeros(n)
    for s in range(ct.T):
        live = R["live"][s]
        assert live.any()
        lt = torch.as_tensor(live, device=dev)
        at = torch.as_tensor(R["actions"][s], device=dev)
        obs, r, done, _, _ = pm.step(at)
        obs_s, _, done_s, _, _ = sm.step(at)
        r64 = r.double().cpu().numpy()
        err = float(np.abs(r64 - R["reward"][s])[live].max())
        worst = max(worst, err)
        assert err <= REWARD_TOL, (s, err)
        if (live & known).any():
            err_o = float(np.abs(r64 - R["oracle"][s])[live & known].max())
            worst_o = max(worst_o, err_o)
            assert err_o <= REWARD_TOL, (s, err_o)
        assert torch.equal(obs[lt], obs_s[lt]) and torch.equal(done[lt], done_s[lt]), s
        np.testing.assert_array_equal(done.cpu().numpy()[live], R["done"][s][live])
        last = R["done"][s]
        if last.any() or s % 16 == 15:  # the integer state on the envs' own days; the return as the terminal step left it
            s1, s2 = pm.state(), sm.state()
            for k in INT_STATE:
                assert torch.equal(s1[k][lt], s2[k][lt]), (s, k)
            er[last] = s1["episode_return"].double().cpu().numpy()[last]
            if last.any():
                fin = _np(s1, INT_STATE)
                for k in ("t", "used", "streak", "hist14", "finished"):
                    np.testing.assert_array_equal(fin[k][last], R["state"][k][last], err_msg=k)
    print(f"step() [{pm_kernel}] on {name}: max per-day |reward - fp64| = {worst:.2e}, |reward - oracle| (known) = {worst_o:.2e}")
    _bars(er, R["ret"], "episode_return")
    _bars(er[known], R["oracle"].sum(0)[known], "episode_return vs oracle")
    if tb.slot27:
        assert np.abs(er - R["oracle"].sum(0))[~known].max() > 1e-4
    # W2A_ST_STEP_AFTER_DONE: step() went on past the shorter episodes
    assert pm.check_status() == sm.check_status() == (4 if tb.ragged else 0)
    pm.close()
    sm.close()


# ------------------------------------------------------------------ b. whole episodes on every path
def _check_episode(tb, env, out, ref, st0, entry, want):
    """one whole-episode rollout(alert_mask=True) against the oracle's loop (decisions, exact) and the fp64 reference
    (returns, every env)"""
    ct, n = tb.ct, env.num_envs
    assert env.last_pm_rollout == want, env.last_pm_rollout
    assert env.check_status() == 0
    got = {k: out[k].cpu().numpy() for k in INT_OUT + ("return", "final_return")}
    for k, rk in zip(INT_OUT, ("alerts", "over", "days", "att")):
        np.testing.assert_array_equal(got[k], ref[rk], err_msg=k)
    nd, budget = st0["n_days"], st0["budget"]
    past = np.arange(ct.T)[None, :] >= nd[:, None]
    assert not (got["alert_days"] & past).any() and not (got["attempt_days"] & past).any()
    assert (got["alerts"][budget == 0] == 0).all()
    assert bool(out["done"].all())
    st = _np(env.state())
    np.testing.assert_array_equal(st["t"], nd - 1)
    np.testing.assert_array_equal(st["t"], ref["t"])
    np.testing.assert_array_equal(st["used"], got["alerts"])
    assert (st["finished"] == 1).all()
    # one-day episodes: the day counter, the streak and the observation row stay as the reset left them (the terminal
    # step advances neither); used / hist14 / last_actual hold that one day's grant
    one = nd == 1
    if tb.ragged:
        assert one.any()
    for k in ("t", "streak"):
        assert (st[k][one] == 0).all(), k
    for k in ("hist14", "last_actual"):
        np.testing.assert_array_equal(st[k][one], got["alerts"][one], err_msg=k)
    assert torch.equal(env._obs, entry)  # built-in kinds write no observation rows
    _, ret64 = E.pm_rewards_fp64(ct, st0, got["alert_days"], ct.T)
    known = ~tb.a2w[st0["coef_col"]]
    for k in ("return", "final_return"):
        _bars(got[k], ret64, k)
        _bars(got[k][known], ref["ret"][known], k + " vs oracle")
        if tb.slot27:
            assert np.abs(got[k] - ref["ret"])[~known].max() > 1e-4
    return float(np.abs(got["return"] - ret64).max())


KINDS = [(name, kind) for name in NAMES for kind in ("bernoulli", "threshold", "table")] + [("ragged", "always"),
                                                                                            ("slot27", "always")]


@pytest.mark.parametrize("name,kind", KINDS)
@pytest.mark.parametrize("pm_kernel", list(PATHS))
def test_whole_episode_rollouts_on_table_edges(dev, tabs, refs, pm_kernel, name, kind):
    """Every path of a reward kernel -- the one-launch kernel and the per-day sequence -- on twin envs: decisions exact
    against the oracle's loop, returns of every env against the fp64 reference, and the two paths against each other
    (integer outputs and state() bit-equal, floats within the return bars)."""
    tb = tabs[name]
    ct = tb.ct
    ref = refs("roll", name, kind)
    pol = E.builtin_policies(ct)[kind]
    runs = []
    for one_launch, want in PATHS[pm_kernel]:
        env = _env(tb, dev, pm_kernel, one_launch)
        st0 = _check_tuples(env, E.host_tuples(tb, env.num_envs))
        entry = env._obs.clone()
        out = env.rollout(pol, alert_mask=True)
        worst = _check_episode(tb, env, out, ref, st0, entry, want)
        print(f"rollout [{pm_kernel}, {want}] {kind} on {name}: max |return - fp64| = {worst:.2e}")
        runs.append((env, out))
    if len(runs) == 2:
        (ea, oa), (eb, ob) = runs
        assert set(oa) == set(ob)
        for k, x in oa.items():
            y = ob[k]
            if x.is_floating_point():
                assert torch.equal(x.isnan(), y.isnan()), k
                torch.testing.assert_close(x.nan_to_num(0.0).double(), y.nan_to_num(0.0).double(), rtol=RETURN_RTOL,
                                           atol=RETURN_ATOL, msg=k)
            else:
                assert torch.equal(x, y), k
        sa, sb = ea.state(), eb.state()
        for k in sa:
            if k == "episode_return":
                torch.testing.assert_close(sa[k].double(), sb[k].double(), rtol=RETURN_RTOL, atol=RETURN_ATOL)
            else:
                assert torch.equal(sa[k], sb[k]), k
    for env, _ in runs:
        assert env.check_status() == 0
        env.close()


# ------------------------------------------------------------------ c. mid-episode entry with a live window
@pytest.mark.parametrize("name", ["slot27", "ragged27"])
@pytest.mark.parametrize("pm_kernel,one_launch,want", [("vector", True, "k_pm_rollout"), ("matrix_i8", True, "k_pm_rollout_i8"),
                                                       ("matrix", True, "per_day")])
def test_mid_episode_entry_with_a_live_window(dev, tabs, pm_kernel, one_launch, want, name):
    """rollout(n_steps=7), five step() days, then the rest -- the second entry finds alerts inside the 14-day window of
    envs on slot-27 columns. A twin runs the episode in one call; the step() days take the twin's attempts of those
    days (the bernoulli kind's, so random), hence the three parts' integer outputs sum / OR to the twin's exactly.
    Every part's rewards against the fp64 reference started from the state() read before that part."""
    tb = tabs[name]
    ct, n = tb.ct, E.N_ENVS[name]
    pol = E.builtin_policies(ct)["bernoulli"]
    A, W = _env(tb, dev, pm_kernel, one_launch), _env(tb, dev, pm_kernel, one_launch)
    whole = W.rollout(pol, alert_mask=True)
    assert W.last_pm_rollout == want and bool(whole["done"].all())
    att_w = whole["attempt_days"].cpu().numpy()
    rows = np.arange(n)

    s0 = _np(A.state())
    o1 = A.rollout(pol, n_steps=7, alert_mask=True)
    assert A.last_pm_rollout == want and A.check_status() == 0
    _, ref1 = E.pm_rewards_fp64(ct, s0, o1["alert_days"].cpu().numpy(), 7)
    _bars(o1["return"].cpu().numpy(), ref1, "part 1")
    s1 = _np(A.state())
    np.testing.assert_array_equal(s1["finished"], s0["n_days"] <= 7)
    np.testing.assert_array_equal(s1["t"], np.minimum(7, s0["n_days"] - 1))

    mid = {k: np.zeros_like(att_w) for k in ("alert_days", "attempt_days")}
    mid_alerts, mid_over = np.zeros(n, np.int64), np.zeros(n, np.int64)
    got_r, cur, worst, past_done = [], s1, 0.0, False
    for _ in range(5):
        live = cur["finished"] == 0
        past_done |= bool((~live).any())
        a = np.where(live, att_w[rows, cur["t"]], False).astype(np.int32)
        _, r, _, _, _ = A.step(torch.as_tensor(a, device=dev))
        got_r.append(r.double().cpu().numpy())
        nxt = _np(A.state())
        granted = (nxt["used"] - cur["used"]).astype(bool) & live
        assert not (granted & (a == 0)).any()
        mid["attempt_days"][rows[live & (a == 1)], cur["t"][live & (a == 1)]] = True
        mid["alert_days"][rows[granted], cur["t"][granted]] = True
        mid_alerts += granted
        mid_over += live & (a == 1) & ~granted
        cur = nxt
    r2, ref2 = E.pm_rewards_fp64(ct, s1, mid["alert_days"], 5)
    for d in range(5):
        lv = ~np.isnan(r2[d])
        if lv.any():
            worst = max(worst, float(np.abs(got_r[d] - r2[d])[lv].max()))
    print(f"mid-episode [{pm_kernel}, {want}] on {name}: max per-day |reward - fp64| of the step() days = {worst:.2e}")
    assert worst <= REWARD_TOL
    assert A.check_status() == (4 if past_done else 0)  # W2A_ST_STEP_AFTER_DONE: step() past the episodes already over

    s2 = cur
    col27 = tb.a2w[s2["coef_col"]]
    assert ((s2["finished"] == 0) & (s2["hist14"] != 0) & col27).any()  # a live window on a slot-27 column
    o3 = A.rollout(pol, alert_mask=True)
    assert A.last_pm_rollout == want and A.check_status() == 0 and bool(o3["done"].all())
    np.testing.assert_array_equal(o3["first_day"].cpu().numpy(), s2["t"])
    _, ref3 = E.pm_rewards_fp64(ct, s2, o3["alert_days"].cpu().numpy(), ct.T)
    _bars(o3["return"].cpu().numpy(), ref3, "part 3")
    # without the window the slot-27 columns' reference differs: the entry state matters
    _, ref3_0 = E.pm_rewards_fp64(ct, {**s2, "hist14": np.zeros(n, np.int64)}, o3["alert_days"].cpu().numpy(), ct.T)
    assert np.abs(ref3 - ref3_0)[col27].max() > 1e-4
    # final_return is the return at an env's terminal step; the episodes over before the step() days took theirs in
    # part 1 (step() on a finished env is the caller's error, flagged above, and goes on adding to it)
    early = s1["finished"] == 1
    _bars(o1["final_return"].cpu().numpy()[early], ref1[early], "final_return of part 1")
    _bars(o3["final_return"].cpu().numpy()[~early], (ref1 + ref2 + ref3)[~early], "final_return")
    _bars(whole["final_return"].cpu().numpy(), ref1 + ref2 + ref3, "the twin's final_return")
    g = {k: whole[k].cpu().numpy() for k in INT_OUT}
    np.testing.assert_array_equal(o1["alerts"].cpu().numpy() + mid_alerts + o3["alerts"].cpu().numpy(), g["alerts"])
    np.testing.assert_array_equal(o1["attempts_over_budget"].cpu().numpy() + mid_over + o3["attempts_over_budget"].cpu().numpy(),
                                  g["attempts_over_budget"])
    for k in ("alert_days", "attempt_days"):
        p1, p3 = o1[k].cpu().numpy(), o3[k].cpu().numpy()
        np.testing.assert_array_equal(p1 | mid[k] | p3, g[k], err_msg=k)
        assert not (p1 & mid[k]).any() and not (p1 & p3).any() and not (mid[k] & p3).any(), k
    sa, sw = _np(A.state()), _np(W.state())
    for k in sa:  # step() shifted the history of the episodes that were over before the step() days
        sel = ~early if k in ("hist14", "last_actual", "at_budget") else np.ones(n, bool)
        np.testing.assert_array_equal(sa[k][sel], sw[k][sel], err_msg=k)
    for e in (A, W):
        assert e.check_status() == 0
        e.close()


# ------------------------------------------------------------------ d. fixed-point ranges of the run-time slots
# case -> (reset options, masked second reset or None, exponent of slot 27's range: 2^e > min(14, largest budget))
RANGES = {"budget3": ({"budget": 3}, None, 2), "budget12": ({"budget": 12}, None, 4), "budget40": ({"budget": 40}, None, 4),
          "less_than": ({"sample_budget": True, "sample_budget_type": "less_than"}, None, 4),
          "masked_3_to_12": ({"budget": 3}, {"budget": 12}, 4)}


@pytest.mark.parametrize("case", list(RANGES))
def test_int8_fixed_point_ranges_of_the_runtime_slots(dev, tabs, case):
    """The int8 kernels turn the run-time slots into fixed point by ranges taken from the episode's largest budget B
    (k_pi8_scales: streak min(T, B), remaining budget B, 14-day count min(14, B)). On slot27, budgets 3, 12 and 40 (the
    remaining budget at 2^6), drawn budgets with zeros, and a masked reset that raises B from 3 to 12 (the scales are
    per episode and must follow): per-day rewards of k_pm_rollout_i8 (one-day rollouts) and of step() on a twin fed the
    same attempts within 1e-5 of the fp64 reference, whole episodes of an always-alert policy (the streak and the
    14-day count run to their limits) within the return bars. The slot-27 columns stay on the matrix-core path in every
    case (E.pi8_flagged_columns), next to the flagged third on the exact path."""
    tb = tabs["slot27"]
    ct, n = tb.ct, E.N_ENVS["slot27"]
    opts, second, e27 = RANGES[case]
    envs = [_env(tb, dev, "matrix_i8", True, reset=False) for _ in range(3)]
    for e in envs:
        e.reset(seed=15, options=dict(opts))
        if second:  # the same episodes again for every other env, on the larger budget (a drawn reset would keep the
            # budget of the first one: the reference's sticky budget)
            ep = {k: v.cpu().numpy() for k, v in e.state().items() if k in ("county_w", "year_i", "coef_col", "sample")}
            e.reset(options={"episodes": dict(ep, budget=second["budget"]), "mask": np.arange(n) % 2 == 1})
    A, B, C = envs
    st0 = _np(A.state())
    bmax = int(st0["budget"].max())
    assert bmax == {"budget3": 3, "budget12": 12, "budget40": 40, "less_than": int(np.asarray(ct.B0).max()),
                    "masked_3_to_12": 12}[case]
    if case == "less_than":
        assert (st0["budget"] == 0).any()
    if second:
        assert set(np.unique(st0["budget"])) == {3, 12} and (st0["t"] == 0).all()
    assert np.frexp(min(14.0, float(bmax)))[1] == e27
    flag = E.pi8_flagged_columns(ct, bmax)
    assert np.array_equal(flag, tb.big) and not flag[tb.a2w].any()  # slot-27 columns: matrix cores; the big third: exact
    on_mfma = ~flag[st0["coef_col"]]
    assert (on_mfma & tb.a2w[st0["coef_col"]]).any() and (~on_mfma).any()
    pol = dict(kind="bernoulli", p=0.8, seed=E.POLICY_SEED)
    days = np.zeros((n, ct.T), bool)
    ra, rb = np.zeros((ct.T, n)), np.zeros((ct.T, n))
    for t in range(ct.T):
        out = A.rollout(pol, n_steps=1, alert_mask=True)
        assert A.last_pm_rollout == "k_pm_rollout_i8", (t, A.last_pm_rollout)
        days |= out["alert_days"].cpu().numpy()
        _, r_b, _, _, _ = B.step(out["attempt_days"][:, t].to(torch.int32))
        ra[t], rb[t] = out["return"].double().cpu().numpy(), r_b.double().cpu().numpy()
    assert bool(out["done"].all())
    r64, ret64 = E.pm_rewards_fp64(ct, st0, days, ct.T)
    assert not np.isnan(r64).any()
    top = days.cumsum(1)
    win = top - np.pad(top, ((0, 0), (14, 0)))[:, : ct.T]
    assert win.max() == min(14, bmax)  # the 14-day count reaches the top of its range
    wa, wb = float(np.abs(ra - r64).max()), float(np.abs(rb - r64).max())
    print(f"int8 ranges, {case}: max per-day |reward - fp64|: one-day rollouts {wa:.2e}, step() {wb:.2e}")
    assert wa <= REWARD_TOL and wb <= REWARD_TOL
    sa, sb = A.state(), B.state()
    for k in INT_STATE:
        assert torch.equal(sa[k], sb[k]), k
    for s in (sa, sb):
        _bars(s["episode_return"].cpu().numpy(), ret64, "episode_return")
    whole = C.rollout(dict(kind="always"), alert_mask=True)
    assert C.last_pm_rollout == "k_pm_rollout_i8" and bool(whole["done"].all())
    np.testing.assert_array_equal(whole["alerts"].cpu().numpy(), np.minimum(st0["budget"], ct.T))
    np.testing.assert_array_equal(C.state()["streak"].cpu().numpy(), np.where(st0["budget"] >= ct.T, ct.T - 1, 0))
    _, ret_c = E.pm_rewards_fp64(ct, st0, whole["alert_days"].cpu().numpy(), ct.T)
    for k in ("return", "final_return"):
        _bars(whole[k].cpu().numpy(), ret_c, k)
    for e in envs:
        assert e.check_status() == 0
        e.close()
