"""The hindsight optimum on the GPU (w2a_hindsight_optimum): schedules against brute force and the fp64 DP
restatement (tests/hindsight_restatement.py), bit-identity of the return with posterior_returns and agreement with
step() driven by the schedule, dominance over every policy kind at full size, budget 0 and budgets far beyond the
tables' defaults, no side effects, refusals.
Uniform tables only; the same kernel on ragged episode lengths and slot-27 coefficient rows:
tests/test_table_edges_gpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from weather2alert_amd import _ffi, synth, tables

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hindsight_restatement import brute_force_fp64, hindsight_fp64, horizon, own_draw_returns  # noqa: E402

pytestmark = pytest.mark.gpu

DAY_BAR = 1e-5  # per-day reward bar of the f32 epilogue against fp64 (tests/test_env_gpu.py)
KEYS = ("t", "used", "streak", "hist14", "budget", "n_days", "county_w", "year_i", "coef_col", "sample", "finished")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ct():
    return tables.compile_from_synth(synth.make_synth("linear", n_fips=30, years=[2006, 2007], n_samples=6, seed=17,
                                                      extra_confounder_fips=3))


def _np(st):
    return {k: st[k].cpu().numpy().astype(np.int64) for k in KEYS}


def _own(pr, st0):
    return pr.gather(1, st0["sample"].long()[:, None])[:, 0]


def _mid_episode(env, days, seed, p=0.35):
    """step random actions for `days` days: varied alerts used, streaks and remaining budgets"""
    g = torch.Generator(device=env.device).manual_seed(seed)
    for _ in range(days):
        env.step((torch.rand(env.num_envs, generator=g, device=env.device) < p).to(torch.int32))
    return {k: v.clone() for k, v in env.state().items()}


def _feasible(ct, st, hs, n_steps):
    days = hs["alert_days"].cpu().numpy()
    alerts = hs["alerts"].cpu().numpy()
    assert (days.sum(1) == alerts).all()
    for e in range(len(alerts)):
        H = horizon({k: int(st[k][e]) for k in st}, n_steps)
        t0 = int(st["t"][e])
        assert alerts[e] <= max(0, st["budget"][e] - st["used"][e])
        assert not days[e, :t0].any() and not days[e, t0 + H:].any()


@pytest.mark.parametrize("n_steps", [1, 5, 12])
def test_brute_force(dev, ct, n_steps):
    """~512 envs at random mid-episode states: the fp64 value of the GPU schedule is at least the best of every feasible
    schedule less H day bars (brute force on all envs for n_steps <= 5, on a strided 48 for 12; the fp64 DP on all)."""
    from weather2alert_amd import HeatAlertVecEnv

    n = 512
    env = HeatAlertVecEnv(n, tables=ct, device=dev, similar_climate_counties=True, autoreset="disabled")
    env.reset(seed=3, options={"budget": 8})
    st0 = _mid_episode(env, 12 + n_steps, seed=n_steps)
    st = _np(st0)
    assert (st["streak"] > 0).any() and (st["used"] == st["budget"]).any() and (st["used"] < st["budget"]).any()
    hs = env.hindsight_optimum(st0, n_steps=n_steps)
    _feasible(ct, st, hs, n_steps)
    Y, K = len(ct.years), ct.n_samples
    days = hs["alert_days"].cpu().numpy()
    mine = own_draw_returns(ct.X, ct.W, K, Y, st, days, n_steps)
    val, _, _ = hindsight_fp64(ct.X, ct.W, K, Y, st, n_steps)
    H = np.array([horizon({k: int(st[k][e]) for k in st}, n_steps) for e in range(n)])
    assert (mine >= val - H * DAY_BAR).all()
    np.testing.assert_allclose(hs["return"].double().cpu().numpy(), mine, rtol=0, atol=n_steps * DAY_BAR)
    for e in (range(n) if n_steps <= 5 else range(0, n, n // 48)):
        best, _ = brute_force_fp64(ct.X, ct.W, K, Y, st, n_steps, e)
        assert mine[e] >= best - H[e] * DAY_BAR, (e, mine[e], best)
    assert int(hs["alerts"].sum()) > 0
    env.close()


def test_bit_identity(dev, ct):
    """"return" == posterior_returns(st0, alert_days)[e, sample_e] bit for bit (mid-episode and from reset), and step()
    driven by the schedule pays it (2e-6 relative) on a small lock-step batch. Stretches of 1 and 17 days and to the end."""
    from weather2alert_amd import HeatAlertVecEnv

    n = 700
    env = HeatAlertVecEnv(n, tables=ct, device=dev, similar_climate_counties=True, autoreset="disabled")
    env.reset(seed=9)
    for days in (0, 33):
        st0 = _mid_episode(env, days, seed=days) if days else {k: v.clone() for k, v in env.state().items()}
        for steps in (None, 17, 1):
            hs = env.hindsight_optimum(st0, n_steps=steps)
            pr = env.posterior_returns(st0, hs["alert_days"], n_steps=steps)
            assert torch.equal(_own(pr, st0), hs["return"]), (days, steps)
    # step() replay from the state reached above
    st0 = {k: v.clone() for k, v in env.state().items()}
    hs = env.hindsight_optimum(st0)
    ad = hs["alert_days"]
    acc = torch.zeros(n, dtype=torch.float32, device=dev)
    t = int(st0["t"][0])
    assert (st0["t"] == t).all()
    while True:
        _, r, term, _, _ = env.step(ad[:, t].to(torch.int32))
        acc += r
        if bool(term.all()):
            break
        t += 1
    np.testing.assert_allclose(acc.double().cpu().numpy(), hs["return"].double().cpu().numpy(), rtol=2e-6, atol=0)
    assert torch.equal(env.state()["used"] - st0["used"], hs["alerts"])
    env.close()


def test_dominance_full_size(dev):
    """1 048 576 envs on bench.py's configs[2] tables, one episode from reset: the optimum is at least every policy
    kind's return (2e-6 relative, for k_rollout_mfma), and rollout(hindsight=True) returns hindsight_optimum(st0)."""
    from weather2alert_amd import HeatAlertVecEnv

    sd = synth.make_synth("linear", years=list(range(2006, 2017)), n_samples=100, seed=0, extra_confounder_fips=60)
    cth = tables.compile_from_synth(sd)
    n, G = 1 << 20, 8
    env = HeatAlertVecEnv(n, tables=cth, device=dev, similar_climate_counties=True, autoreset="disabled")
    env.reset(seed=0)
    st0 = {k: v.clone() for k, v in env.state().items()}
    hs = env.hindsight_optimum(st0)
    opt = hs["return"]
    assert torch.isfinite(opt).all() and (hs["alerts"] <= st0["budget"]).all()
    rng = np.random.default_rng(4)
    W = (rng.standard_normal((G, cth.n_obs)) * 0.3).astype(np.float32)
    b = (rng.standard_normal(G) * 0.5).astype(np.float32)
    pols = [dict(kind="never"), dict(kind="always", require_budget=True),
            dict(kind="threshold", feature="heat_qi", threshold=0.85, require_budget=True),
            dict(kind="bernoulli", p=0.1, seed=2), dict(kind="linear", weight=W, bias=b, group=rng.integers(0, G, n))]
    for pol in pols:
        env.reset(seed=0)
        out = env.rollout(pol, hindsight=True)
        assert torch.equal(out["hindsight_return"], opt), pol["kind"]
        ret = out["return"]
        slack = 2e-6 * ret.abs()
        assert bool((opt >= ret - slack).all()), (pol["kind"], float((ret - opt).max()))
        if pol["kind"] == "linear":
            assert out["group_hindsight_return"].shape == (G,)
    env.close()


def test_budget_cases(dev, ct):
    """Budget 0: an empty schedule whose return is posterior_returns of the empty schedule bit for bit. Budgets 40
    (several 64-state chunks per day, in LDS) and 200 (the workspace path), from reset and mid-episode: against the
    fp64 DP restatement. One env per budget: the faithful env keeps the budget of its first reset (quirk Q9)."""
    from weather2alert_amd import HeatAlertVecEnv

    n = 96
    env = HeatAlertVecEnv(n, tables=ct, device=dev, similar_climate_counties=True, autoreset="disabled")
    env.reset(seed=5, options={"budget": 0})
    st0 = {k: v.clone() for k, v in env.state().items()}
    hs = env.hindsight_optimum(st0)
    assert (hs["alerts"] == 0).all() and not hs["alert_days"].any()
    empty = torch.zeros((n, ct.T), dtype=torch.bool, device=dev)
    assert torch.equal(_own(env.posterior_returns(st0, empty), st0), hs["return"])
    env.close()
    Y, K = len(ct.years), ct.n_samples
    for budget in (40, 200):
        env = HeatAlertVecEnv(n, tables=ct, device=dev, similar_climate_counties=True, autoreset="disabled")
        env.reset(seed=6, options={"budget": budget})
        assert (env.state()["budget"] == budget).all()
        for days in (0, 25):
            st0 = _mid_episode(env, days, seed=budget + days, p=0.6) if days else \
                {k: v.clone() for k, v in env.state().items()}
            st = _np(st0)
            hs = env.hindsight_optimum(st0)
            _feasible(ct, st, hs, ct.T)
            assert int(hs["alerts"].max()) > 14  # the budget is really used beyond the tables' defaults
            val, _, _ = hindsight_fp64(ct.X, ct.W, K, Y, st, ct.T)
            mine = own_draw_returns(ct.X, ct.W, K, Y, st, hs["alert_days"].cpu().numpy(), ct.T)
            H = st["n_days"] - st["t"]
            assert (mine >= val - H * DAY_BAR).all(), budget
            np.testing.assert_allclose(hs["return"].double().cpu().numpy(), val, rtol=0, atol=ct.T * DAY_BAR)
            pr = env.posterior_returns(st0, hs["alert_days"])
            assert torch.equal(_own(pr, st0), hs["return"])
        if budget == 40:
            env.close()
    # a workspace sized for the tables' default budgets is refused for this batch, before any output is written
    lib = env._lib
    small = lib.w2a_hindsight_workspace_bytes(env._h, ct.T, 14, 1)
    assert small < lib.w2a_hindsight_workspace_bytes(env._h, ct.T, 200, 1)
    st = env.state()
    st["finished"][: n // 2] = 1  # envs without a DP: their outputs must stay untouched too
    v = _ffi.StateView()
    for k in _ffi.STATE_FIELDS:
        setattr(v, k, st[k].data_ptr())
    words = (ct.T + 31) // 32
    ret = torch.full((n,), 5.0, dtype=torch.float32, device=dev)
    mask = torch.full((n, words), 7, dtype=torch.int32, device=dev)
    cnt = torch.full((n,), 9, dtype=torch.int32, device=dev)
    ws = torch.empty(small, dtype=torch.uint8, device=dev)
    rc = lib.w2a_hindsight_optimum(env._h, C.byref(v), ct.T, ret.data_ptr(), mask.data_ptr(), words, cnt.data_ptr(),
                                   ws.data_ptr(), small, None)
    assert rc == -1 and b"workspace too small" in lib.w2a_last_error()
    assert (ret == 5.0).all() and (mask == 7).all() and (cnt == 9).all()
    env.close()


def test_ties_do_not_alert(dev, ct):
    """Coefficient rows where an alert changes nothing -- the effectiveness logit so low that its f32 sigmoid is exactly 0
    and no baseline term on the alert, streak or budget slots -- make every alert a tie: the schedule is empty, and the
    return is posterior_returns of the empty schedule bit for bit, as in the fp64 restatement."""
    from weather2alert_amd import HeatAlertVecEnv

    W = np.array(ct.W, np.float32).reshape(-1, 2, 32)
    W[:, 1, :] = 0.0
    W[:, 1, 29] = -1000.0  # slot 29 is the bias input (1.0): sigmoid(-1000) = 0 in f32 and in fp64
    W[:, 0, 24:28] = 0.0
    ctt = tables.CompiledTables(**{**ct.__dict__, "W": W.reshape(ct.W.shape)})
    n = 512
    env = HeatAlertVecEnv(n, tables=ctt, device=dev, similar_climate_counties=True, autoreset="disabled")
    env.reset(seed=4)
    st0 = _mid_episode(env, 20, seed=4)
    assert (st0["used"] < st0["budget"]).any()
    hs = env.hindsight_optimum(st0)
    assert int(hs["alerts"].sum()) == 0 and not hs["alert_days"].any()
    empty = torch.zeros((n, ct.T), dtype=torch.bool, device=dev)
    assert torch.equal(_own(env.posterior_returns(st0, empty), st0), hs["return"])
    val, days, _ = hindsight_fp64(ctt.X, ctt.W, ctt.n_samples, len(ctt.years), _np(st0), ct.T)
    assert not days.any()
    out_never = env.rollout(dict(kind="never"), hindsight=True)
    assert torch.equal(out_never["hindsight_return"], hs["return"])
    env.close()


@pytest.mark.parametrize("kind", ["linear", "threshold"])
def test_no_side_effects(dev, ct, kind):
    from weather2alert_amd import HeatAlertVecEnv

    n = 3001
    g = np.random.default_rng(1).integers(0, 2, n)
    rng = np.random.default_rng(3)
    pol = dict(kind="linear", weight=(rng.standard_normal((2, ct.n_obs)) * 0.3).astype(np.float32),
               bias=np.zeros(2, np.float32), group=g) if kind == "linear" else \
        dict(kind="threshold", feature="heat_qi", threshold=0.7)
    A = HeatAlertVecEnv(n, tables=ct, device=dev, similar_climate_counties=True)
    B = HeatAlertVecEnv(n, tables=ct, device=dev, similar_climate_counties=True)
    A.reset(seed=2)
    B.reset(seed=2)
    for steps in (50, None, 30):
        kw = dict(alert_mask=True, posterior_returns=True) if kind == "threshold" else {}
        oa = A.rollout(pol, n_steps=steps, hindsight=True, **kw)
        ob = B.rollout(pol, n_steps=steps, **kw)
        extra = {"hindsight_return"} | ({"group_hindsight_return"} if kind == "linear" else set())
        assert set(oa) - set(ob) == extra and not set(ob) - set(oa)
        for k, v in ob.items():
            a_ = oa[k]
            if v.is_floating_point():
                a_, v = a_.nan_to_num(7.0), v.nan_to_num(7.0)
            assert torch.equal(a_, v), k
        sa, sb = A.state_dict(), B.state_dict()
        for k in ("state", "obs", "final_return", "reward", "done"):
            assert torch.equal(sa[k], sb[k]), k
        assert sa["host"] == sb["host"]
    before = A.state_dict()
    A.hindsight_optimum()
    A.hindsight_optimum(n_steps=9)
    after = A.state_dict()
    for k in ("state", "obs", "final_return", "reward", "done"):
        assert torch.equal(before[k], after[k]), k
    assert before["host"] == after["host"] and A.check_status() == 0
    A.close()
    B.close()


def test_refusals(dev, ct):
    from weather2alert_amd import HeatAlertVecEnv

    env = HeatAlertVecEnv(64, tables=ct, device=dev, fixes={"lag"})
    env.reset(seed=1)
    with pytest.raises(ValueError, match="lag"):
        env.hindsight_optimum()
    with pytest.raises(ValueError, match="lag"):
        env.rollout(dict(kind="never"), hindsight=True)
    st = env.state()
    v = _ffi.StateView()
    for k in _ffi.STATE_FIELDS:
        setattr(v, k, st[k].data_ptr())
    words = (ct.T + 31) // 32
    ret = torch.empty(64, dtype=torch.float32, device=dev)
    mask = torch.empty((64, words), dtype=torch.int32, device=dev)
    cnt = torch.empty(64, dtype=torch.int32, device=dev)
    ws_bytes = env._lib.w2a_hindsight_workspace_bytes(env._h, ct.T, 1 << 20, 1)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def call(e, steps=ct.T, words=words, nbytes=ws_bytes):
        return e._lib.w2a_hindsight_optimum(e._h, C.byref(v), steps, ret.data_ptr(), mask.data_ptr(), words,
                                           cnt.data_ptr(), ws.data_ptr(), nbytes, None)

    assert call(env) == -1 and b"corrected-semantics" in env._lib.w2a_last_error()
    env.close()
    pm = HeatAlertVecEnv(64, tables=ct, device=dev, reward_mode="posterior_mean")
    pm.reset(seed=1)
    with pytest.raises(ValueError, match="posterior_mean"):
        pm.hindsight_optimum()
    with pytest.raises(ValueError, match="posterior_mean"):
        pm.rollout(dict(kind="never"), hindsight=True)
    pm.close()
    # a table whose slot-27 coefficient is nonzero: refused by Python and by the C entry
    W27 = np.array(ct.W, np.float32).reshape(-1, 2, 32)
    W27[3, 0, 27] = 0.25
    ct27 = tables.CompiledTables(**{**ct.__dict__, "W": W27.reshape(ct.W.shape)})
    bad = HeatAlertVecEnv(64, tables=ct27, device=dev)
    bad.reset(seed=1)
    with pytest.raises(ValueError, match="slot-27"):
        bad.hindsight_optimum()
    with pytest.raises(ValueError, match="slot-27"):
        bad.rollout(dict(kind="never"), hindsight=True)
    st = bad.state()
    for k in _ffi.STATE_FIELDS:
        setattr(v, k, st[k].data_ptr())
    assert call(bad) == -1 and b"slot-27" in bad._lib.w2a_last_error()
    bad.close()
    ok = HeatAlertVecEnv(64, tables=ct, device=dev, fixes={"budget"})
    ok.reset(seed=1)
    st = ok.state()
    for k in _ffi.STATE_FIELDS:
        setattr(v, k, st[k].data_ptr())
    assert call(ok, words=words - 1) == -1 and b"ceil(T/32)" in ok._lib.w2a_last_error()
    assert call(ok, nbytes=1024) == -1 and b"workspace" in ok._lib.w2a_last_error()
    assert call(ok) == 0 and ok.rollout(dict(kind="always"), hindsight=True)["hindsight_return"].shape == (64,)
    with pytest.raises(ValueError, match="shape"):
        ok.hindsight_optimum({k: x[:63] for k, x in st.items()})
    with pytest.raises(KeyError, match="sample"):
        ok.hindsight_optimum({k: x for k, x in st.items() if k != "sample"})
    with pytest.raises(ValueError, match="n_steps"):
        ok.hindsight_optimum(st, n_steps=0)
    st = {k: x.clone() for k, x in ok.state().items()}
    with pytest.raises(_ffi.W2AError, match="recording a hipGraph"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            ok.hindsight_optimum(st)
    assert ok.hindsight_optimum(st)["return"].shape == (64,) and ok.check_status() == 0
    ok.close()
