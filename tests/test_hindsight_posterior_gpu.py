"""The hindsight optimum with the draw unknown on the GPU (w2a_hindsight_posterior, k_hs_pm_dp): returns against brute
force and the fp64 DP restatement (tests/hindsight_posterior_restatement.py), against the draw-mean of
posterior_returns() and against a reward_mode="posterior_mean" env stepped along the schedule; n_samples 1 and 67;
optimality against hindsight_optimum() both ways; budgets 0, beyond the episode and beyond LDS; ties; allowed_days;
sharing; the suffix property; no side effects, determinism; the ragged and slot-27 tables of tests/table_edges.py;
refusals."""
import os
import sys

import numpy as np
import pytest
import torch

from weather2alert_amd import _ffi, synth, tables

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402
from hindsight_posterior_restatement import (brute_force_posterior_fp64, hindsight_posterior_fp64,  # noqa: E402
                                             posterior_mean_returns)
from hindsight_restatement import hindsight_fp64, horizon  # noqa: E402

pytestmark = pytest.mark.gpu

DAY_BAR = 1e-5  # per-day reward bar of the f32 epilogue against fp64 (tests/test_env_gpu.py)
KEYS = ("t", "used", "streak", "hist14", "budget", "n_days", "county_w", "year_i", "coef_col", "sample", "finished")
OUT = ("return", "alert_days", "alerts")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _synth(n_samples):
    return tables.compile_from_synth(synth.make_synth("linear", n_fips=30, years=[2006, 2007], n_samples=n_samples,
                                                      seed=17, extra_confounder_fips=3))


@pytest.fixture(scope="module")
def ct():
    return _synth(6)


def _make(n, ct, dev, **kw):
    from weather2alert_amd import HeatAlertVecEnv

    return HeatAlertVecEnv(n, tables=ct, device=dev, similar_climate_counties=True, autoreset="disabled", **kw)


def _np(st):
    return {k: st[k].cpu().numpy().astype(np.int64) for k in KEYS}


def _clone(st):
    return {k: v.clone() for k, v in st.items()}


def _mid_episode(env, days, seed, p=0.35):
    """step random actions for `days` days: varied alerts used, streaks and remaining budgets"""
    g = torch.Generator(device=env.device).manual_seed(seed)
    for _ in range(days):
        env.step((torch.rand(env.num_envs, generator=g, device=env.device) < p).to(torch.int32))
    return _clone(env.state())


def _horizons(st, n_steps):
    return np.array([horizon({k: int(st[k][e]) for k in st}, n_steps) for e in range(len(st["t"]))])


def _feasible(st, out, n_steps, gate=None):
    days, alerts = out["alert_days"].cpu().numpy(), out["alerts"].cpu().numpy()
    H = _horizons(st, n_steps)
    assert (days.sum(1) == alerts).all() and (alerts <= np.maximum(0, st["budget"] - st["used"])).all()
    d = np.arange(days.shape[1])[None, :]
    assert not (days & ~((d >= st["t"][:, None]) & (d < (st["t"] + H)[:, None]))).any()
    if gate is not None:
        assert not (days & ~gate).any()
    return days, H


def _against_dp(ct, st, out, n_steps, gate=None):
    """the schedule is feasible, earns the fp64 DP's value less H day bars (in fp64), and "return" is that value"""
    days, H = _feasible(st, out, n_steps, gate)
    Y, K = len(ct.years), ct.n_samples
    val, _, _ = hindsight_posterior_fp64(ct.X, ct.W, K, Y, st, n_steps, gate)
    mine = posterior_mean_returns(ct.X, ct.W, K, Y, st, days, n_steps)
    ret = out["return"].double().cpu().numpy()
    print(f"max |return - fp64 DP| / H = {(np.abs(ret - val) / np.maximum(H, 1)).max():.2e}, "
          f"max (DP - schedule's fp64 value) / H = {((val - mine) / np.maximum(H, 1)).max():.2e}")
    assert (mine >= val - H * DAY_BAR).all()
    assert (np.abs(ret - val) <= np.maximum(H, 1) * DAY_BAR).all()
    return val, days, H


def _equal(a, b):
    for k in OUT:
        x, y = a[k], b[k]
        if x.is_floating_point():  # NaN marks a start outside the tables: equal bits
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), k


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("n_steps", [1, 5, 12])
def test_brute_force(dev, ct, n_steps):
    """64 envs at random mid-episode states: "return" is the best draw-mean return over every feasible schedule, within
    n_steps day bars; the schedule is feasible"""
    n = 64
    env = _make(n, ct, dev)
    env.reset(seed=3, options={"budget": 8})
    st0 = _mid_episode(env, 12 + n_steps, seed=n_steps, p=0.15)
    st = _np(st0)
    assert (st["streak"] > 0).any() and (st["used"] < st["budget"]).any()
    out = env.hindsight_posterior_optimum(st0, n_steps=n_steps)
    _against_dp(ct, st, out, n_steps)
    ret = out["return"].double().cpu().numpy()
    for e in range(n):
        best, _ = brute_force_posterior_fp64(ct.X, ct.W, ct.n_samples, len(ct.years), st, n_steps, e)
        print(f"env {e}: return - brute force = {ret[e] - best:.2e}")
        assert abs(ret[e] - best) <= n_steps * DAY_BAR, (e, ret[e], best)
    assert int(out["alerts"].sum()) > 0
    env.close()


# ------------------------------------------------------------------ 2
def test_mean_of_posterior_returns(dev, ct):
    """whole episodes: "return" is the draw-mean of posterior_returns() on the schedule, rtol 2e-6; "alerts" is the
    popcount; posterior_returns=True returns that tensor"""
    n = 300
    env = _make(n, ct, dev)
    env.reset(seed=9)
    st0 = _clone(env.state())
    out = env.hindsight_posterior_optimum(st0, posterior_returns=True)
    pr = env.posterior_returns(st0, out["alert_days"])
    assert torch.equal(pr, out["posterior_returns"]) and pr.shape == (n, ct.n_samples)
    np.testing.assert_allclose(out["return"].double().cpu().numpy(), pr.double().mean(1).cpu().numpy(), rtol=2e-6, atol=0)
    assert torch.equal(out["alerts"], out["alert_days"].sum(1).to(torch.int32)) and int(out["alerts"].sum()) > 0
    dflt = env.hindsight_posterior_optimum(posterior_returns=True)  # the current state, which is st0
    _equal(dflt, out)
    assert torch.equal(dflt["posterior_returns"], pr)
    env.close()


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("n_samples", [1, 67])
def test_n_samples_edges(dev, n_samples):
    """one draw: the schedule and the count are hindsight_optimum()'s bit for bit, the return to f32 rounding; 67 draws:
    past one 64-lane chunk of draws. Both against the fp64 DP."""
    ctk = _synth(n_samples)
    n = 96
    env = _make(n, ctk, dev)
    env.reset(seed=4, options={"budget": 6})
    for days in (0, 20):
        st0 = _mid_episode(env, days, seed=days) if days else _clone(env.state())
        out = env.hindsight_posterior_optimum(st0)
        _against_dp(ctk, _np(st0), out, ctk.T)
        if n_samples == 1:
            hs = env.hindsight_optimum(st0)
            assert torch.equal(hs["alert_days"], out["alert_days"]) and torch.equal(hs["alerts"], out["alerts"])
            # one rounding of the fp64 sum against T f32 roundings of partial sums below |return|
            np.testing.assert_allclose(out["return"].cpu().numpy(), hs["return"].cpu().numpy(), rtol=(ctk.T + 1) * 2.0 ** -24)
        assert int(out["alerts"].sum()) > 0
    env.close()


# ------------------------------------------------------------------ 4
def test_optimality_both_ways(dev, ct):
    """A the new optimum, B hindsight_optimum()'s schedule: A's draw-mean is at least B's, B's own-draw return at least
    A's, and the two differ on far more than 10 % of the envs -- in the fp64 restatements alone as well"""
    n = 128
    env = _make(n, ct, dev)
    env.reset(seed=11, options={"budget": 8})
    st0 = _clone(env.state())
    st = _np(st0)
    Y, K = len(ct.years), ct.n_samples
    ref_a = hindsight_posterior_fp64(ct.X, ct.W, K, Y, st, ct.T)[1]
    ref_b = hindsight_fp64(ct.X, ct.W, K, Y, st, ct.T)[1]
    ref_share = float((ref_a != ref_b).any(1).mean())
    A = env.hindsight_posterior_optimum(st0)
    B = env.hindsight_optimum(st0)
    share = float((A["alert_days"] != B["alert_days"]).any(1).float().mean())
    print(f"schedules differ on {share:.3f} of the envs (restatements: {ref_share:.3f})")
    assert ref_share >= 0.10 and share >= 0.10
    pa, pb = env.posterior_returns(st0, A["alert_days"]).double(), env.posterior_returns(st0, B["alert_days"]).double()
    bar = ct.T * DAY_BAR
    assert bool((pa.mean(1) >= pb.mean(1) - bar).all())
    own = st0["sample"].long()[:, None]
    assert bool((pb.gather(1, own) >= pa.gather(1, own) - bar).all())
    # the value of knowing the draw is really there
    assert float((pa.mean(1) - pb.mean(1)).max()) > bar and float((pb.gather(1, own) - pa.gather(1, own)).max()) > bar
    env.close()


# ------------------------------------------------------------------ 5
def test_posterior_mean_twin(dev, ct):
    """a reward_mode="posterior_mean" env stepped along the schedule pays "return"; hindsight_optimum() on it still
    raises"""
    n = 200
    pm = _make(n, ct, dev, reward_mode="posterior_mean")
    pm.reset(seed=6)
    with pytest.raises(ValueError, match="posterior_mean"):
        pm.hindsight_optimum()
    st0 = _clone(pm.state())
    out = pm.hindsight_posterior_optimum(st0)
    _against_dp(ct, _np(st0), out, ct.T)
    ad = out["alert_days"]
    acc = torch.zeros(n, dtype=torch.float64, device=dev)
    for t in range(ct.T):
        _, r, term, _, _ = pm.step(ad[:, t].to(torch.int32))
        acc += r.double()
        if bool(term.all()):
            break
    err = (acc - out["return"].double()).abs().max().item()
    print(f"max |stepped posterior-mean return - return| = {err:.2e}")
    assert err <= ct.T * DAY_BAR and int(out["alerts"].sum()) > 0
    assert torch.equal(pm.state()["used"] - st0["used"], out["alerts"])
    pm.close()


# ------------------------------------------------------------------ 6
@pytest.mark.parametrize("budget", [0, 40, 160])
def test_budgets(dev, ct, budget):
    """budget 0 (an empty schedule), 40 (several 64-state chunks per day, in LDS) and 160 (>= n_days = 153, and beyond
    LDS: V and the decision words in the workspace pool): against the fp64 DP, from reset and mid-episode. Few envs at
    160: the restatement's cost grows with the square of the budget."""
    n = 6 if budget > 40 else 24
    env = _make(n, ct, dev)
    env.reset(seed=5, options={"budget": budget})
    assert (env.state()["budget"] == budget).all() and (budget <= 40 or budget >= ct.T)
    lib = env._lib
    base = lib.w2a_hindsight_posterior_workspace_bytes(n, ct.T, ct.n_samples, ct.T, 0, 1)
    assert (lib.w2a_hindsight_posterior_workspace_bytes(n, ct.T, ct.n_samples, ct.T, budget, 1) > base) == (budget > 40)
    for days in (0, 25):
        st0 = _mid_episode(env, days, seed=budget + days, p=0.6) if days else _clone(env.state())
        out = env.hindsight_posterior_optimum(st0)
        _against_dp(ct, _np(st0), out, ct.T)
        if budget == 0:
            assert not out["alert_days"].any() and (out["alerts"] == 0).all()
            empty = torch.zeros((n, ct.T), dtype=torch.bool, device=dev)
            np.testing.assert_allclose(out["return"].double().cpu().numpy(),
                                       env.posterior_returns(st0, empty).double().mean(1).cpu().numpy(), rtol=2e-6)
        else:
            assert int(out["alerts"].max()) > 14  # the budget is really used beyond the tables' defaults
    env.close()


def test_ties_do_not_alert(dev, ct):
    """coefficient rows where an alert changes nothing (tests/test_hindsight_gpu.py::test_ties_do_not_alert): every
    alert is a tie under every draw, so under their mean: the schedule is empty"""
    W = np.array(ct.W, np.float32).reshape(-1, 2, 32)
    W[:, 1, :] = 0.0
    W[:, 1, 29] = -1000.0  # slot 29 is the bias input (1.0): sigmoid(-1000) = 0 in f32 and in fp64
    W[:, 0, 24:28] = 0.0
    ctt = tables.CompiledTables(**{**ct.__dict__, "W": W.reshape(ct.W.shape)})
    n = 128
    env = _make(n, ctt, dev)
    env.reset(seed=4)
    st0 = _mid_episode(env, 20, seed=4)
    assert (st0["used"] < st0["budget"]).any()
    out = env.hindsight_posterior_optimum(st0)
    assert int(out["alerts"].sum()) == 0 and not out["alert_days"].any()
    _against_dp(ctt, _np(st0), out, ct.T)
    assert not hindsight_posterior_fp64(ctt.X, ctt.W, ctt.n_samples, len(ctt.years), _np(st0), ct.T)[1].any()
    env.close()


# ------------------------------------------------------------------ 7
def test_allowed_days(dev, ct):
    """the best schedule under a restriction against the restatement under it; an all-true mask is the ungated call
    bit for bit; an all-false mask gives the no-alert return"""
    n = 96
    env = _make(n, ct, dev)
    env.reset(seed=8, options={"budget": 6})
    st0 = _mid_episode(env, 10, seed=1)
    st = _np(st0)
    gate = torch.rand((n, ct.T), generator=torch.Generator(device=dev).manual_seed(2), device=dev) < 0.4
    out = env.hindsight_posterior_optimum(st0, allowed_days=gate)
    _against_dp(ct, st, out, ct.T, gate.cpu().numpy())
    free = env.hindsight_posterior_optimum(st0, share=False)
    assert int(out["alerts"].sum()) > 0 and bool((free["return"] >= out["return"] - ct.T * DAY_BAR).all())
    assert not torch.equal(free["alert_days"], out["alert_days"])
    _equal(env.hindsight_posterior_optimum(st0, allowed_days=torch.ones_like(gate)), free)
    none = env.hindsight_posterior_optimum(st0, allowed_days=torch.zeros_like(gate))
    assert not none["alert_days"].any() and (none["alerts"] == 0).all()
    st_b0 = dict(st0, budget=st0["used"].clone())  # no budget left: the no-alert return of the same states
    # (the remaining budget enters the reward, so the reference is the restatement, not a budget-0 twin)
    val = posterior_mean_returns(ct.X, ct.W, ct.n_samples, len(ct.years), st, np.zeros((n, ct.T), bool), ct.T)
    H = _horizons(st, ct.T)
    assert (np.abs(none["return"].double().cpu().numpy() - val) <= np.maximum(H, 1) * DAY_BAR).all()
    assert not env.hindsight_posterior_optimum(st_b0)["alert_days"].any()
    env.close()


# ------------------------------------------------------------------ 8
def test_sharing(dev, ct):
    """share=True and share=False are bit-identical on a batch whose distinct problems are fewer than half the envs
    (lock-step envs from one reset differ in (county, year, column) only: at most 60 x 30), finished envs and a start
    outside the tables included; the outputs do not change under a permutation of `sample`"""
    n = 512
    env = _make(n, ct, dev)
    env.reset(seed=12, options={"budget": 5})
    st0 = _clone(env.state())
    q, half = n // 4, n // 2  # the other three quarters repeat the first with other draws
    for r in (1, 2, 3):
        for k in KEYS:
            st0[k][r * q:(r + 1) * q] = st0[k][:q] if k != "sample" else (st0[k][:q] + r) % ct.n_samples
    st0["finished"][5] = st0["finished"][half + 5] = 1
    st0["coef_col"][7] = ct.S + 3  # outside the tables: NaN
    st0["sample"][half + 9] = ct.n_samples  # this one alone, not its twin
    a = env.hindsight_posterior_optimum(st0, share=True)
    keys = env.last_hindsight_posterior_keys
    b = env.hindsight_posterior_optimum(st0, share=False)
    assert keys < n // 2 and env.last_hindsight_posterior_keys == n
    assert keys == len(torch.unique(torch.stack([st0[k] for k in KEYS if k not in ("sample", "hist14")], 1), dim=0)) + 1
    _equal(a, b)
    assert torch.isnan(a["return"][7]) and torch.isnan(a["return"][half + 9]) and not torch.isnan(a["return"][9])
    assert int(torch.isnan(a["return"]).sum()) == 2 and float(a["return"][5]) == 0.0 and int(a["alerts"].sum()) > 0
    st1 = _clone(env.state())
    st1["sample"] = st1["sample"][torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(dev)]
    for share in (True, False):
        _equal(env.hindsight_posterior_optimum(st1, share=share), env.hindsight_posterior_optimum(share=share))
    env.close()


# ------------------------------------------------------------------ 9
def test_suffix_property(dev, ct):
    """from the state after k days of the schedule, the call returns the schedule's remaining days bit for bit"""
    n = 128
    env = _make(n, ct, dev)
    env.reset(seed=13, options={"budget": 7})
    out = env.hindsight_posterior_optimum()
    ad = out["alert_days"]
    k = 37
    for t in range(k):
        env.step(ad[:, t].to(torch.int32))
    rest = env.hindsight_posterior_optimum()
    assert not rest["alert_days"][:, :k].any() and torch.equal(rest["alert_days"][:, k:], ad[:, k:])
    assert torch.equal(rest["alerts"], ad[:, k:].sum(1).to(torch.int32)) and int(rest["alerts"].sum()) > 0
    assert int(ad[:, :k].sum()) > 0
    env.close()


# ------------------------------------------------------------------ 10
def test_no_side_effects_and_determinism(dev, ct):
    n = 1000 + 37
    A, B = _make(n, ct, dev), _make(n, ct, dev)
    A.reset(seed=2)
    B.reset(seed=2)
    g = torch.Generator(device=dev).manual_seed(5)
    for day in range(40):
        if day in (0, 17, 39):
            before = A.state_dict()
            x = A.hindsight_posterior_optimum(posterior_returns=True)
            y = A.hindsight_posterior_optimum(n_steps=9, share=False)
            _equal(x, A.hindsight_posterior_optimum())  # identical calls, identical bits
            _equal(y, A.hindsight_posterior_optimum(n_steps=9, share=False))
            after = A.state_dict()
            for k in ("state", "obs", "final_return", "reward", "done"):
                assert torch.equal(before[k], after[k]), k
            assert before["host"] == after["host"]
        act = (torch.rand(n, generator=g, device=dev) < 0.2).to(torch.int32)
        oa, ob = A.step(act), B.step(act)
        for p, q in zip(oa[:4], ob[:4]):
            assert torch.equal(p, q)
    sa, sb = A.state_dict(), B.state_dict()
    for k in ("state", "obs", "final_return", "reward", "done"):
        assert torch.equal(sa[k], sb[k]), k
    assert sa["host"] == sb["host"] and A.check_status() == 0
    A.close()
    B.close()


# ------------------------------------------------------------------ 11
def test_ragged_and_slot27_tables(dev):
    """the ragged table (episodes of 1, 2 and 3 days and the full-length one among 20..153) against the fp64 DP, from
    reset and mid-episode; the slot-27 table is refused by Python and by the C entry, before anything is written"""
    from weather2alert_amd import HeatAlertVecEnv

    tabs = E.make_tables()
    rt = tabs["ragged"].ct
    n = 128 + 5
    rng = np.random.default_rng(21)
    col = rng.integers(0, rt.S, n)
    cw, yi = rt.fips_to_weather[col].astype(np.int64), rng.integers(0, rt.Y, n)
    nd_tab = np.asarray(rt.n_days).reshape(-1, rt.Y)
    for i, d in enumerate(E.SHORTEST + (rt.T,)):
        cw[i], yi[i] = np.argwhere(nd_tab == d)[0]
    ep = dict(county_w=cw, year_i=yi, coef_col=col, sample=rng.integers(0, rt.n_samples, n),
              budget=np.where(np.arange(n) % 3 == 0, 0, np.where(np.arange(n) % 3 == 1, 4, 40)))
    env = HeatAlertVecEnv(n, tables=rt, device=dev, autoreset="disabled", env_gid0=E.GID0)
    env.reset(options={"episodes": ep})
    g = torch.Generator(device=dev).manual_seed(3)
    for days in (0, 13):
        for _ in range(days):
            a = (torch.rand(n, generator=g, device=dev) < 0.35) & (env.state()["finished"] == 0)
            env.step(a.to(torch.int32))
        st0 = _clone(env.state())
        st = _np(st0)
        assert set(E.SHORTEST + (rt.T,)) <= set(st["n_days"].tolist())
        for steps in (None, 4):
            out = env.hindsight_posterior_optimum(st0, n_steps=steps)
            _, _, H = _against_dp(rt, st, out, steps or rt.T)
            assert (out["return"].cpu().numpy()[H == 0] == 0).all()
            _equal(out, env.hindsight_posterior_optimum(st0, n_steps=steps, share=False))
        assert int(out["alerts"].sum()) > 0
    env.close()
    s27 = tabs["slot27"].ct
    bad = HeatAlertVecEnv(64, tables=s27, device=dev)
    bad.reset(seed=1)
    with pytest.raises(ValueError, match="slot-27"):
        bad.hindsight_posterior_optimum()
    rc, ret, mask, cnt = _c_call(bad, s27, dev)
    assert rc == -1 and b"w2a_hindsight_posterior: a coefficient row has a nonzero slot-27" in bad._lib.w2a_last_error()
    assert (ret == 5.0).all() and (mask == 7).all() and (cnt == 9).all()
    bad.close()


def _c_call(env, ct, dev, ws_bytes=None):
    import ctypes as C

    n = env.num_envs
    st = env.state()
    v = _ffi.StateView()
    for k in _ffi.STATE_FIELDS:
        setattr(v, k, st[k].data_ptr())
    words = (ct.T + 31) // 32
    ret = torch.full((n,), 5.0, dtype=torch.float32, device=dev)
    mask = torch.full((n, words), 7, dtype=torch.int32, device=dev)
    cnt = torch.full((n,), 9, dtype=torch.int32, device=dev)
    if ws_bytes is None:
        ws_bytes = max(256, env._lib.w2a_hindsight_posterior_workspace_bytes(n, ct.T, ct.n_samples, ct.T, 1 << 20, 1))
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
    rc = env._lib.w2a_hindsight_posterior(env._h, C.byref(v), ct.T, ret.data_ptr(), mask.data_ptr(), words,
                                          cnt.data_ptr(), ws.data_ptr(), ws_bytes, None)
    torch.cuda.synchronize()
    return rc, ret, mask, cnt


def test_refusals(dev, ct):
    """fixes other than "budget", a stream capture, a workspace sized for small budgets, and tables with more draws than
    the per-draw LDS arrays take (658 at 153 days): each with its message, before anything is written"""
    from weather2alert_amd import HeatAlertVecEnv

    env = HeatAlertVecEnv(64, tables=ct, device=dev, fixes={"lag"})
    env.reset(seed=1)
    with pytest.raises(ValueError, match=r"hindsight_posterior_optimum\(\) needs faithful semantics"):
        env.hindsight_posterior_optimum()
    rc, ret, mask, cnt = _c_call(env, ct, dev)
    assert rc == -1 and b"corrected-semantics" in env._lib.w2a_last_error() and (ret == 5.0).all()
    env.close()
    ok = HeatAlertVecEnv(64, tables=ct, device=dev, fixes={"budget"}, autoreset="disabled")
    ok.reset(seed=1, options={"budget": 200})
    st = _clone(ok.state())
    with pytest.raises(_ffi.W2AError, match="recording a hipGraph"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            ok.hindsight_posterior_optimum(st)
    small = ok._lib.w2a_hindsight_posterior_workspace_bytes(64, ct.T, ct.n_samples, ct.T, 14, 1)
    rc, ret, mask, cnt = _c_call(ok, ct, dev, ws_bytes=small)
    assert rc == -1 and b"workspace too small" in ok._lib.w2a_last_error()
    assert (ret == 5.0).all() and (mask == 7).all() and (cnt == 9).all()
    rc, ret, mask, cnt = _c_call(ok, ct, dev, ws_bytes=1024)
    assert rc == -1 and b"workspace smaller than" in ok._lib.w2a_last_error() and (ret == 5.0).all()
    assert ok.hindsight_posterior_optimum(st)["return"].shape == (64,) and ok.check_status() == 0
    ok.close()
    big = _synth(658)
    env = HeatAlertVecEnv(64, tables=big, device=dev)
    env.reset(seed=1)
    assert env._lib.w2a_hindsight_posterior_workspace_bytes(64, big.T, 658, big.T, 10, 1) == 0
    with pytest.raises(_ffi.W2AError, match="n_samples is too large"):
        env.hindsight_posterior_optimum()
    rc, ret, mask, cnt = _c_call(env, big, dev)
    assert rc == -1 and (ret == 5.0).all() and (mask == 7).all() and (cnt == 9).all()
    assert env.hindsight_posterior_optimum(n_steps=30)["return"].shape == (64,)  # 16 x 30 + 96 x 658 bytes fit
    env.close()
