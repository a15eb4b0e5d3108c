"""The draw-blind hindsight budget curve on the GPU (w2a_hindsight_posterior_curve, k_hs_pm_curve): every column
against hindsight_posterior_optimum() of the twin with budget = used + b, bit for bit (from reset, mid-episode, under a
gate, on a truncated horizon; 6 and 67 draws and the ragged table); past 64 budgets on the workspace path; sharing; one
draw against hindsight_budget_curve(); the fp64 restatement (tests/hindsight_posterior_curve_restatement.py); a
reward_mode="posterior_mean" env stepped along a column's schedule; edges, determinism, no side effects; refusals."""
import os
import sys

import numpy as np
import pytest
import torch

from weather2alert_amd import _ffi, synth, tables

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402
from budget_curve_restatement import twin  # noqa: E402
from hindsight_posterior_curve_restatement import posterior_curve_fp64  # noqa: E402
from hindsight_posterior_restatement import posterior_mean_returns  # noqa: E402
from hindsight_restatement import horizon  # noqa: E402

pytestmark = pytest.mark.gpu

DAY_BAR = 1e-5  # per-day reward bar of the f32 epilogue against fp64 (tests/test_hindsight_posterior_gpu.py)
KEYS = ("t", "used", "streak", "hist14", "budget", "n_days", "county_w", "year_i", "coef_col", "sample", "finished")
B = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _synth(n_samples):
    return tables.compile_from_synth(synth.make_synth("linear", n_fips=30, years=[2006, 2007], n_samples=n_samples,
                                                      seed=17, extra_confounder_fips=3))


@pytest.fixture(scope="module")
def tabs():
    """name -> compiled tables (made once for the module)"""
    return {"k6": _synth(6), "k67": _synth(67), "ragged": E.make_tables()["ragged"].ct}


def _make(n, ct, dev, **kw):
    from weather2alert_amd import HeatAlertVecEnv

    return HeatAlertVecEnv(n, tables=ct, device=dev, similar_climate_counties=True, autoreset="disabled", **kw)


def _env(dev, tabs, table, n, days=0, seed=11, budget=6, p=0.3):
    """a fresh env on the table, stepped `days` days with Bernoulli(p) attempts (none on finished envs)"""
    ct = tabs[table]
    if table == "ragged":  # the shortest episodes and the full-length one are among the envs
        rng = np.random.default_rng(21)
        col = rng.integers(0, ct.S, n)
        cw, yi = ct.fips_to_weather[col].astype(np.int64), rng.integers(0, ct.Y, n)
        nd_tab = np.asarray(ct.n_days).reshape(-1, ct.Y)
        for i, d in enumerate(E.SHORTEST + (ct.T,)):
            cw[i], yi[i] = np.argwhere(nd_tab == d)[0]
        ep = dict(county_w=cw, year_i=yi, coef_col=col, sample=rng.integers(0, ct.n_samples, n),
                  budget=np.where(np.arange(n) % 3 == 0, 0, np.where(np.arange(n) % 3 == 1, 4, 40)))
        from weather2alert_amd import HeatAlertVecEnv

        env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", env_gid0=E.GID0)
        env.reset(options={"episodes": ep})
    else:
        env = _make(n, ct, dev)
        env.reset(seed=seed, options={"budget": budget})
    acts = torch.as_tensor((np.random.default_rng(seed).random((days, n)) < p).astype(np.int32), device=dev)
    for d in range(days):
        env.step(acts[d] * (env.state()["finished"] == 0).to(torch.int32))
    return env


def _clone(st):
    return {k: v.clone() for k, v in st.items()}


def _np(st):
    return {k: st[k].cpu().numpy().astype(np.int64) for k in KEYS}


def _bits(x):
    return x.contiguous().view(torch.int32) if x.is_floating_point() else x


def _twin(st0, b):
    tw = _clone(st0)
    tw["budget"] = tw["used"] + b
    return tw


def _check_twins(env, st0, max_budget, budgets, n_steps=None, gate=None, share=True):
    """columns `budgets` of the curve against hindsight_posterior_optimum(share=False) of the twins; returns the curve"""
    cv = env.hindsight_posterior_budget_curve(max_budget, start_state=st0, n_steps=n_steps, allowed_days=gate,
                                              schedules=True, share=share)
    n, T = env.num_envs, env.ct.T
    assert cv["return"].shape == cv["alerts"].shape == (n, max_budget + 1) and cv["return"].dtype == torch.float32
    assert cv["alert_days"].shape == (n, max_budget + 1, T) and cv["alert_days"].dtype == torch.bool
    assert cv["alerts"].dtype == cv["own_budget"].dtype == torch.int32
    assert torch.equal(cv["own_budget"], st0["budget"] - st0["used"])
    for b in budgets:
        hs = env.hindsight_posterior_optimum(_twin(st0, b), n_steps=n_steps, allowed_days=gate, share=False)
        assert torch.equal(_bits(cv["return"][:, b]), _bits(hs["return"])), b
        assert torch.equal(cv["alerts"][:, b], hs["alerts"]), b
        assert torch.equal(cv["alert_days"][:, b], hs["alert_days"]), b
    assert torch.equal(cv["alert_days"].sum(-1).to(torch.int32), cv["alerts"])
    return cv


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("case", ["reset", "mid", "gate", "steps12"])
@pytest.mark.parametrize("table", ["k6", "k67", "ragged"])
def test_twins_bit_for_bit(dev, tabs, table, case):
    """every column 0 .. 8 is the twin's optimum; the env's own column is hindsight_posterior_optimum() of the env as
    it is. 67 draws wrap the lanes-over-draws loops; the ragged table's shortest episodes end inside the horizon."""
    n = 192
    env = _env(dev, tabs, table, n, days=40, budget=16, p=0.35) if case == "mid" else _env(dev, tabs, table, n)
    st0 = _clone(env.state())
    if case == "mid":  # running streaks, spent budgets, some finished (the synth episodes are longer than 40 days)
        st0["finished"][3::50] = 1
        assert (st0["streak"] > 0).any() and (st0["used"] > 0).any() and (st0["finished"] != 0).any()
    gate = env.alert_gate("heat_qi", 0.8) if case == "gate" else None
    n_steps = 12 if case == "steps12" else None
    cv = _check_twins(env, st0, B, range(B + 1), n_steps=n_steps, gate=gate)
    if gate is not None:
        assert not (cv["alert_days"] & ~gate[:, None, :]).any()
    own = env.hindsight_posterior_optimum(st0, n_steps=n_steps, allowed_days=gate)
    ob = cv["own_budget"].long()
    inside = (ob >= 0) & (ob <= B)
    col = ob.clamp(0, B)
    assert int(inside.sum()) >= n // 3
    assert torch.equal(_bits(cv["return"].gather(1, col[:, None])[:, 0][inside]), _bits(own["return"][inside]))
    assert torch.equal(cv["alerts"].gather(1, col[:, None])[:, 0][inside], own["alerts"][inside])
    pick = cv["alert_days"][torch.arange(n, device=dev), col]
    assert torch.equal(pick[inside], own["alert_days"][inside])
    assert int(cv["alerts"].sum()) > 0 and not cv["alert_days"][:, 0].any()
    env.close()


# ------------------------------------------------------------------ 2
def test_past_64_budgets_on_the_pool_path(dev, tabs):
    """B = 70: the backtrack's second chunk of budgets, V and the decision words in the workspace (GLOBAL = true)"""
    n, steps, big = 64, 25, 70
    env = _env(dev, tabs, "k6", n, days=6)
    lib = env._lib
    assert lib.w2a_hindsight_posterior_curve_workspace_bytes(env._h, steps, B, 1) == 256
    assert lib.w2a_hindsight_posterior_curve_workspace_bytes(env._h, steps, big, 1) > 256
    cv = _check_twins(env, _clone(env.state()), big, (0, 1, 63, 64, 65, 70), n_steps=steps)
    assert int(cv["alerts"][:, 64:].max()) > 1
    env.close()


# ------------------------------------------------------------------ 3
def test_sharing(dev, tabs):
    """share=True is share=False bit for bit; from one reset the 192 envs are at most 60 x 30 (county-year, column)
    problems with repeats among them; with allowed_days nothing is shared"""
    n = 192
    env = _env(dev, tabs, "k6", n)
    st0 = _clone(env.state())
    st0["finished"][5] = 1
    st0["coef_col"][7] = tabs["k6"].S + 3   # outside the tables: NaN
    st0["sample"][9] = tabs["k6"].n_samples  # this one alone
    st0["budget"][::2] += 3                  # the env's own budget is no part of the problem
    a = env.hindsight_posterior_budget_curve(B, start_state=st0, schedules=True, share=True)
    keys = env.last_hindsight_posterior_keys
    b = env.hindsight_posterior_budget_curve(B, start_state=st0, schedules=True, share=False)
    assert keys < n and env.last_hindsight_posterior_keys == n
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert torch.isnan(a["return"][7]).all() and torch.isnan(a["return"][9]).all() and (a["return"][5] == 0).all()
    assert int(torch.isnan(a["return"]).any(1).sum()) == 2
    gate = torch.ones((n, tabs["k6"].T), dtype=torch.bool, device=dev)
    g = env.hindsight_posterior_budget_curve(B, start_state=st0, schedules=True, allowed_days=gate)
    assert env.last_hindsight_posterior_keys == n
    for k in a:  # an all-true gate is the ungated call
        assert torch.equal(_bits(a[k]), _bits(g[k])), k
    env.close()


# ------------------------------------------------------------------ 4
def test_one_draw_is_the_own_draw_curve(dev):
    """n_samples = 1: alerts and schedules are hindsight_budget_curve()'s bit for bit; the return to f32 rounding (one
    rounding of the fp64 sum against T f32 roundings of partial sums: the bound of
    tests/test_hindsight_posterior_gpu.py::test_n_samples_edges)"""
    ct1 = _synth(1)
    env = _make(96, ct1, dev)
    env.reset(seed=4, options={"budget": 6})
    g = torch.Generator(device=dev).manual_seed(20)
    for days in (0, 20):
        for _ in range(days):
            env.step((torch.rand(96, device=dev, generator=g) < 0.3).to(torch.int32))
        st0 = _clone(env.state())
        a = env.hindsight_posterior_budget_curve(B, start_state=st0, schedules=True)
        c = env.hindsight_budget_curve(B, start_state=st0, schedules=True)
        assert torch.equal(a["alerts"], c["alerts"]) and torch.equal(a["alert_days"], c["alert_days"])
        assert torch.equal(a["own_budget"], c["own_budget"])
        np.testing.assert_allclose(a["return"].cpu().numpy(), c["return"].cpu().numpy(), rtol=(ct1.T + 1) * 2.0 ** -24)
        assert int(a["alerts"].sum()) > 0
    env.close()


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("table,days", [("k6", 0), ("k6", 30), ("ragged", 5)])
def test_against_the_fp64_restatement(dev, tabs, table, days):
    """|return - fp64 optimum| <= max(H, 1) day bars per column, and the kernel's schedule earns the fp64 optimum less
    H day bars in fp64 (the DAY_BAR conditions of tests/test_hindsight_posterior_gpu.py)"""
    n, b_max, steps = 32, 4, 25
    ct = tabs[table]
    env = _env(dev, tabs, table, n, days=days)
    st0 = _clone(env.state())
    st = _np(st0)
    cv = env.hindsight_posterior_budget_curve(b_max, start_state=st0, n_steps=steps, schedules=True)
    ref = posterior_curve_fp64(ct.X, ct.W, ct.n_samples, len(ct.years), st, steps, b_max)
    H = np.array([horizon({k: int(st[k][e]) for k in st}, steps) for e in range(n)])
    ret, sched = cv["return"].double().cpu().numpy(), cv["alert_days"].cpu().numpy()
    for b in range(b_max + 1):
        val = ref["value"][:, b]
        mine = posterior_mean_returns(ct.X, ct.W, ct.n_samples, len(ct.years), twin(st, b), sched[:, b], steps)
        print(f"b = {b}: max |return - fp64| / H = {(np.abs(ret[:, b] - val) / np.maximum(H, 1)).max():.2e}, "
              f"max (fp64 optimum - schedule's fp64 value) / H = {((val - mine) / np.maximum(H, 1)).max():.2e}")
        assert (np.abs(ret[:, b] - val) <= np.maximum(H, 1) * DAY_BAR).all(), b
        assert (mine >= val - H * DAY_BAR).all(), b
    assert (H > 0).any() and int(cv["alerts"].sum()) > 0
    env.close()


# ------------------------------------------------------------------ 6
@pytest.mark.parametrize("b", [2, 5])
def test_paid_by_a_posterior_mean_env(dev, tabs, b):
    """a reward_mode="posterior_mean" env whose budget is used + b, stepped along column b's schedule, pays "return"
    (the bound of tests/test_hindsight_posterior_gpu.py::test_posterior_mean_twin); such an env is accepted"""
    n, ct = 128, tabs["k6"]
    pm = _make(n, ct, dev, reward_mode="posterior_mean")
    pm.reset(seed=6, options={"budget": b})
    st0 = _clone(pm.state())
    assert (st0["budget"] - st0["used"] == b).all()
    cv = pm.hindsight_posterior_budget_curve(B, start_state=st0, schedules=True)
    ad = cv["alert_days"][:, b]
    acc = torch.zeros(n, dtype=torch.float64, device=dev)
    for t in range(ct.T):
        _, r, term, _, _ = pm.step(ad[:, t].to(torch.int32))
        acc += r.double()
        if bool(term.all()):
            break
    err = (acc - cv["return"][:, b].double()).abs().max().item()
    print(f"b = {b}: max |stepped posterior-mean return - return| = {err:.2e}")
    assert err <= ct.T * DAY_BAR and int(cv["alerts"][:, b].sum()) > 0
    assert torch.equal(pm.state()["used"] - st0["used"], cv["alerts"][:, b])
    pm.close()


# ------------------------------------------------------------------ 7
def test_edges(dev, tabs):
    """B = 0, finished envs and starts outside the tables, determinism, no side effects, packed words"""
    n, ct = 100, tabs["k6"]
    env = _env(dev, tabs, "k6", n, days=5)
    before, obs_before, status = env.state_dict(), env._obs.clone(), env.status_word.clone()
    st_before = _clone(env.state())
    st = _clone(env.state())
    st["coef_col"][:5] = ct.S + 3
    st["sample"][5] = ct.n_samples
    st["finished"][6:9] = 1
    st["t"][9] = st["n_days"][9]
    for share in (True, False):
        a = env.hindsight_posterior_budget_curve(B, start_state=st, schedules=True, share=share)
        b = env.hindsight_posterior_budget_curve(B, start_state=st, schedules=True, share=share)
        for k in a:
            assert torch.equal(_bits(a[k]), _bits(b[k])), k
        assert torch.isnan(a["return"][:6]).all() and (a["return"][6:10] == 0).all()
        assert torch.isfinite(a["return"][10:]).all()
        assert (a["alerts"][:10] == 0).all() and not a["alert_days"][:10].any()
    # B = 0: one column, empty schedules, the no-alert draw-mean of the twin with no budget left
    z = env.hindsight_posterior_budget_curve(0, start_state=st, schedules=True)
    assert z["return"].shape == (n, 1) and torch.equal(_bits(z["return"][:, 0]), _bits(a["return"][:, 0]))
    assert not z["alert_days"].any() and (z["alerts"] == 0).all()
    inside = {**st, "coef_col": st_before["coef_col"], "sample": st_before["sample"], "budget": st["used"]}
    empty = torch.zeros((n, ct.T), dtype=torch.bool, device=dev)
    never = env.posterior_returns(inside, empty).double().mean(1)
    np.testing.assert_allclose(z["return"][10:, 0].double().cpu().numpy(), never[10:].cpu().numpy(), rtol=2e-6)
    # without schedules: the same returns and counts; packed words unpack to the bool array
    c = env.hindsight_posterior_budget_curve(B, start_state=st)
    assert set(c) == {"return", "alerts", "own_budget"}
    assert torch.equal(_bits(c["return"]), _bits(a["return"])) and torch.equal(c["alerts"], a["alerts"])
    pk = env.hindsight_posterior_budget_curve(B, start_state=st, schedules=True, packed=True)["alert_days"]
    words = (ct.T + 31) // 32
    assert pk.shape == (n, B + 1, words) and pk.dtype == torch.int32
    days = torch.arange(ct.T, device=dev)
    unpacked = ((pk[:, :, days >> 5] >> (days & 31)) & 1).bool()
    assert torch.equal(unpacked, a["alert_days"])
    # the handle: state, observation buffer, status word and bookkeeping untouched; the default start is the state
    cur = env.hindsight_posterior_budget_curve(B)
    assert torch.equal(cur["own_budget"], st_before["budget"] - st_before["used"])
    after = env.state_dict()
    for k in ("state", "obs", "final_return", "reward", "done"):
        assert torch.equal(before[k], after[k]), k
    assert before["host"] == after["host"] and torch.equal(obs_before, env._obs)
    assert torch.equal(status, env.status_word) and env.check_status() == 0
    for k, x in env.state().items():
        assert torch.equal(x, st_before[k]), k
    env.close()


def test_refusals_come_before_any_output(dev, tabs):
    """fixes other than "budget", a stream capture, slot-27 tables and an n_samples beyond the per-draw arrays (658 at
    153 days; the workspace size is then 0): Python's and the C entry's refusals, nothing written"""
    import ctypes as C

    from weather2alert_amd import HeatAlertVecEnv

    def c_call(env, ct, steps):
        n, st, v = env.num_envs, env.state(), _ffi.StateView()
        for k in _ffi.STATE_FIELDS:
            setattr(v, k, st[k].data_ptr())
        ret = torch.full((n, B + 1), 5.0, dtype=torch.float32, device=dev)
        cnt = torch.full((n, B + 1), 9, dtype=torch.int32, device=dev)
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
        rc = env._lib.w2a_hindsight_posterior_curve(env._h, C.byref(v), steps, B, ret.data_ptr(), cnt.data_ptr(), None, 0,
                                                    ws.data_ptr(), 1 << 20, None)
        torch.cuda.synchronize()
        return rc, bool((ret == 5.0).all() and (cnt == 9).all()), env._lib.w2a_last_error()

    ct = tabs["k6"]
    env = HeatAlertVecEnv(64, tables=ct, device=dev, fixes={"lag"})
    env.reset(seed=1)
    with pytest.raises(ValueError, match=r"hindsight_posterior_budget_curve\(\) needs faithful semantics"):
        env.hindsight_posterior_budget_curve(B)
    rc, untouched, msg = c_call(env, ct, ct.T)
    assert rc == -1 and untouched and b"w2a_hindsight_posterior_curve: not available with corrected-semantics" in msg
    env.close()
    ok = HeatAlertVecEnv(64, tables=ct, device=dev, fixes={"budget"}, autoreset="disabled")
    ok.reset(seed=1)
    st = _clone(ok.state())
    with pytest.raises(_ffi.W2AError, match="recording a hipGraph"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            ok.hindsight_posterior_budget_curve(B, st)
    assert ok.hindsight_posterior_budget_curve(B, st)["return"].shape == (64, B + 1) and ok.check_status() == 0
    ok.close()
    s27 = E.make_tables()["slot27"].ct
    bad = HeatAlertVecEnv(64, tables=s27, device=dev)
    bad.reset(seed=1)
    with pytest.raises(ValueError, match="slot-27"):
        bad.hindsight_posterior_budget_curve(B)
    rc, untouched, msg = c_call(bad, s27, s27.T)
    assert rc == -1 and untouched and b"w2a_hindsight_posterior_curve: a coefficient row has a nonzero slot-27" in msg
    bad.close()
    big = _synth(658)
    env = HeatAlertVecEnv(64, tables=big, device=dev)
    env.reset(seed=1)
    f = env._lib.w2a_hindsight_posterior_curve_workspace_bytes
    assert f(env._h, big.T, B, 1) == 0 and f(env._h, 30, B, 1) > 256 and f(None, 30, B, 1) == 0  # (30 days: the pool)
    with pytest.raises(_ffi.W2AError, match="n_samples is too large"):
        env.hindsight_posterior_budget_curve(B)
    rc, untouched, msg = c_call(env, big, big.T)
    assert rc == -1 and untouched and b"w2a_hindsight_posterior_curve: the tables' n_samples is too large" in msg
    assert env.hindsight_posterior_budget_curve(B, n_steps=30)["return"].shape == (64, B + 1)  # 16 x 30 + 96 x 658 B fit
    env.close()
