"""k_step64's phase B after the one-pass change (csrc/w2a_step64.hip.h): the feature and baseline rows of all 8 rounds of a
64-env tile are requested before the first wait, and the effectiveness rows -- needed only by envs that alert today with an
open gate -- are served from a compact per-tile list: a first unconditional round of 8 envs, then a wave-uniform loop.

Every case runs through HeatAlertVecEnv.step() on the forced 64-envs-per-wave kernel (step_kernel="wide") and is checked
day by day against the float64 VectorOracle: observations, done flags and integer state exact, rewards within 1e-5, returns
at the suite's bar. Where the 4-lanes-per-env kernel (step_kernel="classic") serves the same batch, observations and
integer state are also compared with it bit for bit (its rewards differ by the order of the fp64 additions: 1e-6).

The oracle cannot read tests/golden's mini parquet tables where no parquet engine is installed, so the tables here are the
small synthetic ones the sibling step-kernel tests use (20 counties x 3 years x 9 draws, 5-day episodes).

How many envs of a tile need the row is set through the actions: with budget = T every attempt is granted, and on tables
without the gate bitmap (W2A_NO_GATE_BITS, read when the device tables are made) every granted alert fetches its row, so
the list holds EXACTLY the alerting envs; with the bitmap it holds those of them whose gate is open (at most as many)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import obs_layouts as L  # noqa: E402
from oracle import heatalert_oracle as O  # noqa: E402
from weather2alert_amd import synth, tables  # noqa: E402

pytestmark = pytest.mark.gpu

REWARD_TOL = 1e-5
KERNEL_TOL = 1e-6
RETURN_RTOL, RETURN_ATOL = 2e-6, 2e-5
N_DAYS = 5
SIZES = (63, 64, 65, 95, 96, 97, 257, 1023)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def world():
    sd = synth.make_synth("linear", n_fips=20, years=[2006, 2007, 2008], n_samples=9, n_days=N_DAYS, seed=67,
                          extra_confounder_fips=3)
    ct = tables.compile_from_synth(sd)
    gate = np.asarray(ct.X)[:, :, tables.SLOT_GATE] > 0.5
    assert ct.T == N_DAYS and gate.any() and (~gate).any()  # open and closed gates both occur
    return sd, ct


def _oracle(sd, **kw):
    return O.VectorOracle(O.RefData.from_synth(sd), sd.fips_weather, sd.years, **kw)


def _np_state(env):
    return {k: v.cpu().numpy() for k, v in env.state().items()}


def _ints_equal_oracle(env, V):
    st = _np_state(env)
    np.testing.assert_array_equal(st["t"], V.t)
    np.testing.assert_array_equal(st["used"], V.used)
    np.testing.assert_array_equal(st["budget"], V.budget)
    np.testing.assert_array_equal(st["streak"], V.streak)
    np.testing.assert_array_equal(st["hist14"], (V.hist * (1 << np.arange(13, -1, -1))).sum(axis=1))


def _same_ints(A, B, what):
    sa, sb = A.state(), B.state()
    for k in sa:
        if k != "episode_return":
            assert torch.equal(sa[k], sb[k]), (k, what)


def _tuples(ct, n, seed, budget):
    rng = np.random.default_rng(seed)
    county = rng.integers(0, ct.S, n)
    return dict(county_w=np.asarray(ct.fips_to_weather)[county].astype(np.int64), year_i=rng.integers(0, ct.Y, n),
                coef_col=county, sample=rng.integers(0, ct.n_samples, n), budget=np.full(n, budget, np.int64))


def _day(wide, classic, V, a, a_oracle, what, obs_exact=True):
    """one day on the wide env, its classic twin (or None) and the oracle"""
    at = torch.as_tensor(np.asarray(a, np.int32), device=wide.device)
    o1, r1, d1, _, i1 = wide.step(at)
    assert wide.last_step_kernel.startswith("k_step64"), what
    obs_o, r_o, done_o, _ = V.step(np.asarray(a_oracle, np.int64))
    err = float(np.abs(r1.cpu().numpy().astype(np.float64) - r_o).max())
    assert err <= REWARD_TOL, (what, err)
    np.testing.assert_array_equal(d1.cpu().numpy(), done_o)
    if obs_exact and wide.write_obs:
        np.testing.assert_array_equal(o1.cpu().numpy(), obs_o.astype(np.float32))
    if classic is not None:
        o2, r2, d2, _, _ = classic.step(at)
        assert classic.last_step_kernel == "k_step", what
        assert torch.equal(d1, d2), what
        assert torch.allclose(r1, r2, rtol=0, atol=KERNEL_TOL), what
        if wide.write_obs:
            assert torch.equal(o1, o2), what
    return o1, i1, r_o


def _episode(dev, sd, ct, n, act, budget=N_DAYS, classic=True, bad=None, status_ok=True, **kw):
    """One injected episode of N_DAYS days (autoreset off) under the actions act(t) -> int array [n]; `bad`: env indices
    whose action value is sent as 2 on day 1 (counts as 1, raises the bad-action status bit)."""
    from weather2alert_amd import HeatAlertVecEnv

    kw = dict(dict(tables=ct, device=dev, autoreset="disabled"), **kw)
    wide = HeatAlertVecEnv(n, step_kernel="wide", **kw)
    twin = HeatAlertVecEnv(n, step_kernel="classic", **kw) if classic else None
    assert wide.step_kernel_name == "k_step64"
    ep = _tuples(ct, n, n + budget, budget)
    o1, _ = wide.reset(options={"episodes": ep})
    if twin is not None:
        o2, _ = twin.reset(options={"episodes": ep})
        assert torch.equal(o1, o2)
    V = _oracle(sd, **({"fixes": tuple(sorted(kw["fixes"]))} if kw.get("fixes") else {}))
    obs_o = V.reset(ep["county_w"], ep["year_i"], ep["coef_col"], ep["sample"], ep["budget"])
    if wide.write_obs:
        np.testing.assert_array_equal(o1.cpu().numpy(), obs_o.astype(np.float32))
    ret = np.zeros(n)
    for t in range(N_DAYS):
        a = np.asarray(act(t), np.int64)
        sent = a.copy()
        if bad is not None and t == 1:
            sent[bad], a[bad] = 2, 1
        _, _, r_o = _day(wide, twin, V, sent, a, (n, t))
        ret += r_o
        if t == N_DAYS - 2:
            _ints_equal_oracle(wide, V)
            if twin is not None:
                _same_ints(wide, twin, t)
    np.testing.assert_allclose(_np_state(wide)["episode_return"], ret, rtol=RETURN_RTOL, atol=RETURN_ATOL)
    if twin is not None:
        _same_ints(wide, twin, "end")
    if bad is not None:
        with pytest.raises(ValueError):
            wide.check_status()
    elif status_ok:
        assert wide.check_status() == 0
    wide.close()
    if twin is not None:
        twin.close()


@pytest.mark.parametrize("n", SIZES)
def test_batch_edges_two_episodes(dev, world, n):
    """Two whole episodes in lock step on the packed form: the ragged second half-tile (95, 96, 97: the tile's rounds 4..7
    are requested on shadow descriptors and never flushed), the masked flush, padding waves, ten consecutive launches =
    both walk directions on every day."""
    from weather2alert_amd import HeatAlertVecEnv

    sd, ct = world
    kw = dict(tables=ct, device=dev, similar_climate_counties=True, env_gid0=3)
    wide, twin = HeatAlertVecEnv(n, step_kernel="wide", **kw), HeatAlertVecEnv(n, step_kernel="classic", **kw)
    o1, _ = wide.reset(seed=5)
    o2, _ = twin.reset(seed=5)
    assert torch.equal(o1, o2)
    rng = np.random.default_rng(n)
    V = _oracle(sd)
    for episode in range(2):
        st = _np_state(wide)
        assert (st["t"] == 0).all() and (st["episode_no"] == episode).all()
        obs_o = V.reset(st["county_w"], st["year_i"], st["coef_col"], st["sample"], st["budget"])
        np.testing.assert_array_equal(o1.cpu().numpy(), obs_o.astype(np.float32))
        ret = np.zeros(n)
        for t in range(N_DAYS):
            a = (rng.random(n) < 0.5).astype(np.int32)
            # (the terminal step of a lock-step batch returns the next episode's first row: checked above)
            o1, info, r_o = _day(wide, twin, V, a, a, (n, episode, t), obs_exact=t < N_DAYS - 1)
            assert wide.last_step_kernel == "k_step64<packed>"
            ret += r_o
            if t == N_DAYS - 2:
                _ints_equal_oracle(wide, V)
        np.testing.assert_allclose(info["final_return"].cpu().numpy(), ret, rtol=RETURN_RTOL, atol=RETURN_ATOL)
    _same_ints(wide, twin, n)
    assert wide.check_status() == 0 and twin.check_status() == 0
    wide.close()
    twin.close()


def _lanes(name, t):
    """lanes of a 64-env tile that alert on day t"""
    rng = np.random.default_rng(100 + t)
    if name == "none":
        return []
    if name in ("one", "eight", "nine"):
        return rng.choice(64, {"one": 1, "eight": 8, "nine": 9}[name], replace=False)
    if name == "all":
        return np.arange(64)
    if name == "late_rounds":   # every needing env in rounds 4..7 (the second flush's half of the tile), 12 of them
        return 32 + rng.choice(32, 12, replace=False)
    if name == "one_group":     # the 8 envs of one round, another round every day
        return 8 * ((3 + t) % 8) + np.arange(8)
    raise KeyError(name)


@pytest.mark.parametrize("bitmap", [True, False])
@pytest.mark.parametrize("pattern", ["none", "one", "eight", "nine", "all", "late_rounds", "one_group"])
def test_effectiveness_list_lengths(dev, world, monkeypatch, pattern, bitmap):
    """0, 1, 8 (the first list round full), 9 (first trip of the loop), 64 (budget = T, actions all 1: the loop at full
    length, every day) needing envs per tile, and the grouped ones. 3 tiles + a ragged fourth (n = 200), whose clamp lanes
    may stand in the list. Without the bitmap the counts are exact and closed gates act through the -inf logit; with it
    the closed-gate envs are not in the list at all."""
    sd, ct = world
    if not bitmap:
        monkeypatch.setenv("W2A_NO_GATE_BITS", "1")
    n = 200

    def act(t):
        a = np.zeros(n, np.int64)
        for tile0 in range(0, n, 64):
            idx = tile0 + np.asarray(_lanes(pattern, t), np.int64)
            a[idx[idx < n]] = 1
        return a

    _episode(dev, sd, ct, n, act)


@pytest.mark.parametrize("bitmap", [True, False])
def test_closed_gates_and_a_bad_action(dev, world, monkeypatch, bitmap):
    """Half the envs alert every day, so open and closed gates both occur among them (the table has both); on day 1 some
    envs send the action value 2: it counts as an alert and raises the status bit."""
    sd, ct = world
    if not bitmap:
        monkeypatch.setenv("W2A_NO_GATE_BITS", "1")
    n = 257
    rng = np.random.default_rng(9)
    _episode(dev, sd, ct, n, lambda t: (rng.random(n) < 0.5).astype(np.int64), bad=np.arange(5, n, 11))


def test_budget_runs_out_in_the_list(dev, world):
    """budget 2 under an alert every day: from day 2 on nobody is granted one and the list is empty again"""
    sd, ct = world
    _episode(dev, sd, ct, 130, lambda t: np.ones(130, np.int64), budget=2)


def test_reward_only(dev, world):
    """write_obs=False: no tile, no flush (the two-pass body with the list)"""
    sd, ct = world
    rng = np.random.default_rng(4)
    _episode(dev, sd, ct, 257, lambda t: (rng.random(257) < 0.6).astype(np.int64), write_obs=False)


@pytest.mark.parametrize("fixes", [("obs",), ("alert_2wks", "lag", "penalty", "obs")])
def test_fixes_combination(dev, world, fixes):
    """FIXES: the observation's own row (xo) beside the reward's, the 14-day count patched into the list round's row too"""
    sd, ct = world
    rng = np.random.default_rng(6)
    _episode(dev, sd, ct, 257, lambda t: (rng.random(257) < 0.6).astype(np.int64), budget=3, fixes=set(fixes))


def test_in_kernel_autoreset_on_the_restart_day(dev, world):
    """lockstep=False: the AUTORESET instantiation; the envs restart inside the kernel on the terminal day, three times"""
    from weather2alert_amd import HeatAlertVecEnv

    sd, ct = world
    n = 321
    kw = dict(tables=ct, device=dev, autoreset="same_step", lockstep=False, similar_climate_counties=True)
    wide, twin = HeatAlertVecEnv(n, step_kernel="wide", **kw), HeatAlertVecEnv(n, step_kernel="classic", **kw)
    assert wide._dev_auto
    o1, _ = wide.reset(seed=12, options={"budget": 3})
    o2, _ = twin.reset(seed=12, options={"budget": 3})
    assert torch.equal(o1, o2)
    V = _oracle(sd)
    rng = np.random.default_rng(12)
    for episode in range(3):
        st = _np_state(wide)
        assert (st["t"] == 0).all() and (st["episode_no"] == episode).all()
        obs_o = V.reset(st["county_w"], st["year_i"], st["coef_col"], st["sample"], st["budget"])
        np.testing.assert_array_equal(o1.cpu().numpy(), obs_o.astype(np.float32))  # the restart day's row
        for t in range(N_DAYS):
            a = (rng.random(n) < 0.6).astype(np.int32)
            o1, _, _ = _day(wide, twin, V, a, a, ("autoreset", episode, t), obs_exact=t < N_DAYS - 1)
            if t == N_DAYS - 2:
                _ints_equal_oracle(wide, V)
    _same_ints(wide, twin, "autoreset")
    assert wide.check_status() == 0 and twin.check_status() == 0
    wide.close()
    twin.close()


def test_recorded_block_replayed_twice(dev, world):
    """One hipGraph block of three packed steps, replayed twice (an episode boundary inside), equals six eager steps,
    which are checked against the oracle above."""
    from weather2alert_amd import HeatAlertVecEnv

    _, ct = world
    n = 321
    kw = dict(tables=ct, device=dev, similar_climate_counties=True, lockstep=False, step_kernel="wide")
    A, B = HeatAlertVecEnv(n, **kw), HeatAlertVecEnv(n, **kw)
    oa, _ = A.reset(seed=3)
    ob, _ = B.reset(seed=3)
    assert torch.equal(oa, ob)
    g = torch.Generator(device=dev).manual_seed(11)
    acts = [(torch.rand(n, device=dev, generator=g) < 0.6).to(torch.int32) for _ in range(3)]
    A.step(acts[0]); B.step(acts[0])  # (loads the kernels and packs the mirror before the capture)
    assert A.last_step_kernel == "k_step64<packed>"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for a in acts:
            A.step(a)
    for rep in range(2):
        graph.replay()
        for a in acts:
            o, r, d, _, _ = B.step(a)
        torch.cuda.synchronize()
        assert torch.equal(A._obs, o) and torch.equal(A._reward, r) and torch.equal(A._done_bool, d), rep
        assert torch.equal(A._final_return, B._final_return), rep
    sa, sb = A.state(), B.state()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert int(sa["episode_no"].min()) >= 1 and A.check_status() == 0 and B.check_status() == 0
    A.close()
    B.close()


@pytest.fixture(scope="module")
def other_layout():
    tb = L.make_table("n8")  # heat_qi is column 1 on slot 0, run-time columns interleaved with a table column, 40-day episodes
    return tb.sd, tb.ct


@pytest.mark.parametrize("pattern", ["one", "nine", "all"])
def test_other_observation_layout(dev, other_layout, pattern):
    """n_obs = 8 with slots 4..23 empty: the list round requests the env's feature row again whatever the layout"""
    sd, ct = other_layout
    n = 130

    def act(t):
        a = np.zeros(n, np.int64)
        for tile0 in range(0, n, 64):
            idx = tile0 + np.asarray(_lanes(pattern, t), np.int64)
            a[idx[idx < n]] = 1
        return a

    # (40-day episodes: N_DAYS days of them, so no final return yet)
    _episode_prefix(dev, sd, ct, n, act)


def _episode_prefix(dev, sd, ct, n, act):
    from weather2alert_amd import HeatAlertVecEnv

    kw = dict(tables=ct, device=dev, autoreset="disabled")
    wide, twin = HeatAlertVecEnv(n, step_kernel="wide", **kw), HeatAlertVecEnv(n, step_kernel="classic", **kw)
    ep = _tuples(ct, n, 31, N_DAYS)
    o1, _ = wide.reset(options={"episodes": ep})
    o2, _ = twin.reset(options={"episodes": ep})
    assert torch.equal(o1, o2) and o1.shape == (n, ct.n_obs)
    V = _oracle(sd)
    obs_o = V.reset(ep["county_w"], ep["year_i"], ep["coef_col"], ep["sample"], ep["budget"])
    np.testing.assert_array_equal(o1.cpu().numpy(), obs_o.astype(np.float32))
    ret = np.zeros(n)
    for t in range(N_DAYS):
        a = act(t)
        _, _, r_o = _day(wide, twin, V, a, a, ("layout", t))
        ret += r_o
    _ints_equal_oracle(wide, V)
    _same_ints(wide, twin, "layout")
    np.testing.assert_allclose(_np_state(wide)["episode_return"], ret, rtol=RETURN_RTOL, atol=RETURN_ATOL)
    assert wide.check_status() == 0 and twin.check_status() == 0
    wide.close()
    twin.close()
