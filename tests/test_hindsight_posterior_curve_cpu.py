"""CPU checks of the draw-blind hindsight budget curve: the two fp64 restatements
(tests/hindsight_posterior_curve_restatement.py: the B + 1 twin runs and the direct (remaining, streak) DP) against each
other on the mini synth table and on the ragged table of tests/table_edges.py, the one-draw case against
tests/budget_curve_restatement.py, what hindsight_posterior_budget_curve() refuses before it touches a device, the C
ABI of w2a_hindsight_posterior_curve (header, binding, host-side refusals without a GPU), and stats.py on a dict of the
new call's shape."""
import ctypes as C
import inspect
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from weather2alert_amd import HeatAlertVecEnv, _ffi, build, stats, synth, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "w2a.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402
from budget_curve_restatement import budget_curve_fp64  # noqa: E402
from hindsight_posterior_curve_restatement import posterior_curve_direct_fp64, posterior_curve_fp64  # noqa: E402
from test_hindsight_cpu import random_starts  # noqa: E402

P = 4096  # a non-NULL, 256-B aligned address that is never read
B = 4
NAMES = ("w2a_hindsight_posterior_curve_workspace_bytes", "w2a_hindsight_posterior_curve",
         "w2a_hindsight_posterior_curve_gated")


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.load()


def _synth(n_samples):
    return tables.compile_from_synth(synth.make_synth("linear", n_fips=30, years=[2006, 2007], n_samples=n_samples,
                                                      seed=17, extra_confounder_fips=3))


@pytest.fixture(scope="module")
def ct():
    return _synth(6)


def _both_ways(ct, start, n_steps, gate=None):
    Y, K = len(ct.years), ct.n_samples
    a = posterior_curve_fp64(ct.X, ct.W, K, Y, start, n_steps, B, gate)
    b = posterior_curve_direct_fp64(ct.X, ct.W, K, Y, start, n_steps, B, gate)
    np.testing.assert_allclose(b["value"], a["value"], rtol=0, atol=1e-9)
    np.testing.assert_array_equal(b["alert_days"], a["alert_days"])
    np.testing.assert_array_equal(b["alerts"], a["alerts"])
    assert (a["alerts"] <= np.arange(B + 1)[None]).all() and (a["alert_days"].sum(-1) == a["alerts"]).all()
    assert not a["alert_days"][:, 0].any()
    if gate is not None:
        assert not (a["alert_days"] & ~gate[:, None, :]).any()
    return a, b


@pytest.mark.parametrize("n_steps", [7, 25])
def test_restatements_agree_on_the_mini_synth_table(ct, n_steps):
    rng = np.random.default_rng(70 + n_steps)
    start = random_starts(ct, 16, rng, n_steps)
    start["finished"][3] = 1
    a, b = _both_ways(ct, start, n_steps)
    assert a["alerts"].sum() > 0 and (start["streak"] > 0).any()
    assert (a["value"][3] == 0).all() and not a["alert_days"][3].any() and b["H"][3] == 0
    # neither reads `sample`, and the direct DP neither `budget` nor `used`
    other = dict(start, sample=(start["sample"] + 1) % ct.n_samples, budget=start["budget"] + 3, used=start["used"] * 0)
    c = posterior_curve_direct_fp64(ct.X, ct.W, ct.n_samples, len(ct.years), other, n_steps, B)
    assert all(np.array_equal(b[k], c[k]) for k in b)
    gate = rng.random((16, ct.T)) < 0.5
    _both_ways(ct, start, n_steps, gate)


def test_restatements_agree_on_the_ragged_table():
    """episodes of 1, 2 and 3 days and the full-length one among them: the stretch stops after the terminal day"""
    rt = E.make_tables()["ragged"].ct
    n_steps = 8
    rng = np.random.default_rng(61)
    start = random_starts(rt, 12, rng, n_steps)
    nd_tab = np.asarray(rt.n_days).reshape(-1, rt.Y)
    for i, d in enumerate(E.SHORTEST + (rt.T,)):
        cw, yi = np.argwhere(nd_tab == d)[0]
        start["county_w"][i], start["year_i"][i], start["n_days"][i] = cw, yi, d
        start["t"][i] = min(int(start["t"][i]), d - 1)
        start["budget"][i], start["used"][i], start["streak"][i] = 3, 0, 0
    a, b = _both_ways(rt, start, n_steps)
    assert (b["H"][:3] <= np.array(E.SHORTEST)).all() and a["alerts"].sum() > 0


def test_one_draw_is_the_budget_curve():
    """n_samples = 1: the mean over draws is the draw, so the schedules are budget_curve_fp64's"""
    ct1 = _synth(1)
    rng = np.random.default_rng(6)
    for n_steps in (5, 25):
        start = random_starts(ct1, 8, rng, n_steps)
        assert (start["sample"] == 0).all()
        a = posterior_curve_fp64(ct1.X, ct1.W, 1, len(ct1.years), start, n_steps, B)
        d = posterior_curve_direct_fp64(ct1.X, ct1.W, 1, len(ct1.years), start, n_steps, B)
        c = budget_curve_fp64(ct1.X, ct1.W, 1, len(ct1.years), start, n_steps, B)
        for x in (a, d):
            np.testing.assert_array_equal(x["alert_days"], c["alert_days"])
            np.testing.assert_array_equal(x["alerts"], c["alerts"])
            np.testing.assert_allclose(x["value"], c["value"], rtol=0, atol=1e-12)


def test_python_refusals_on_a_bare_env(ct):
    """every refusal is raised before a device or the library is touched; a posterior_mean env is NOT refused"""
    env = object.__new__(HeatAlertVecEnv)
    env.ct, env.num_envs, env.device, env.fixes, env.reward_mode = ct, 4, torch.device("cpu"), set(), "sampled"
    env._needs_reset, env._pm = False, False
    env.dtables = types.SimpleNamespace(_slot27_zero=True)
    sig = inspect.signature(HeatAlertVecEnv.hindsight_posterior_budget_curve)
    assert list(sig.parameters)[1:] == ["max_budget", "start_state", "n_steps", "allowed_days", "schedules", "packed",
                                        "share"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [None, None, None, False, False, True]
    who = r"hindsight_posterior_budget_curve\(\)"
    st = {k: np.zeros(4, np.int32) for k in ("t", "used", "streak", "budget", "n_days", "county_w", "year_i", "coef_col",
                                             "sample", "finished")}
    for pm in (False, True):
        env._pm = pm
        for bad in (-1, 1024, 3.0, "8", None, True):
            with pytest.raises(ValueError, match=who + r": max_budget must be an int in 0\.\.1023"):
                env.hindsight_posterior_budget_curve(bad)
        env.num_envs = 1 << 22
        with pytest.raises(ValueError, match=who + r": the schedules of 4194304 envs x 9 budgets need 6530531328 bytes"):
            env.hindsight_posterior_budget_curve(8, schedules=True)
        with pytest.raises(ValueError, match=r"need 29024583680 bytes"):
            env.hindsight_posterior_budget_curve(345, schedules=True, packed=True)
        env.num_envs = 4
        with pytest.raises(ValueError, match="allowed_days"):
            env.hindsight_posterior_budget_curve(8, allowed_days=np.zeros((3, ct.T), bool))
        with pytest.raises(KeyError, match="sample"):
            env.hindsight_posterior_budget_curve(8, {k: v for k, v in st.items() if k != "sample"})
        with pytest.raises(ValueError, match="shape"):
            env.hindsight_posterior_budget_curve(8, {k: v[:3] for k, v in st.items()})
        with pytest.raises(ValueError, match="n_steps must be positive"):
            env.hindsight_posterior_budget_curve(8, st, n_steps=0)
        for bad in (2.0, "3", True):
            with pytest.raises(ValueError, match=who + ": n_steps must be an int"):
                env.hindsight_posterior_budget_curve(8, st, n_steps=bad)
    env.fixes = {"lag", "budget"}
    with pytest.raises(ValueError, match=who + r" needs faithful semantics; fixes \['lag'\]"):
        env.hindsight_posterior_budget_curve(8)
    env.fixes = {"budget"}
    env.dtables = types.SimpleNamespace(_slot27_zero=False)
    with pytest.raises(ValueError, match=who + ".*slot-27"):
        env.hindsight_posterior_budget_curve(8)
    # the own-draw curve sees what it saw
    env.dtables = types.SimpleNamespace(_slot27_zero=True)
    env._pm = True
    with pytest.raises(ValueError, match=r"hindsight_budget_curve\(\) needs reward_mode='sampled', not 'posterior_mean'"):
        env.hindsight_budget_curve(8)


def test_entry_points_declared_exported_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)

    def args(name):
        m = re.search(r"\b(?:int|size_t) " + name + r"\s*\(([^;]*)\);", text)
        assert m, name
        return re.sub(r"\s+", " ", m.group(1))

    for new, old, n_args in zip(NAMES, ("w2a_hindsight_curve_workspace_bytes", "w2a_hindsight_curve",
                                        "w2a_hindsight_curve_gated"), (4, 11, 13)):
        assert args(new) == args(old)  # w2a_hindsight_curve's arguments
        assert len(args(new).split(",")) == n_args == len(getattr(lib, new).argtypes)
        assert getattr(lib, new).argtypes == getattr(lib, old).argtypes
    assert re.search(r"\bsize_t w2a_hindsight_posterior_curve_workspace_bytes\s*\(", text)
    assert "const uint32_t *allowed_days" in args(NAMES[2])
    header = sorted(set(re.findall(r"\b(w2a_[a-z_0-9]+)\s*\(", text)))
    for s in NAMES:
        assert s in _ffi.SYMBOLS and s in header and hasattr(lib, s)
        assert not s.startswith("w2a_rollout_") and "_gradient_" not in s
    assert header == sorted(_ffi.SYMBOLS)
    assert lib.w2a_hindsight_posterior_curve.restype is C.c_int
    assert lib.w2a_hindsight_posterior_curve_gated.restype is C.c_int
    assert lib.w2a_hindsight_posterior_curve_workspace_bytes.restype is C.c_size_t
    assert lib.w2a_abi_version() == 18 == _ffi.ABI_VERSION


@pytest.mark.parametrize("name", NAMES[1:])
def test_host_side_refusals_without_gpu(lib, name):
    bufs = {k: (C.c_int32 * 4)() for k in _ffi.STATE_FIELDS}

    def view(**null):
        v = _ffi.StateView()
        for k in _ffi.STATE_FIELDS:
            setattr(v, k, None if k in null else C.addressof(bufs[k]))
        return v

    ok = dict(start=view(), n_steps=3, max_budget=8, ret=P, alerts=P, masks=None, mask_words=0, ws=P, ws_bytes=4096,
              stream=None)
    if name.endswith("_gated"):
        ok.update(allowed_days=P, allowed_words=5)

    def call(**bad):
        a = dict(ok, **bad)
        a["start"] = None if a["start"] is None else C.byref(a["start"])
        return getattr(lib, name)(None, *a.values()), lib.w2a_last_error().decode()

    assert call() == (-1, f"{name}: NULL handle")  # alert_masks may be NULL; mask_words is then not read
    assert call(masks=P, mask_words=5) == (-1, f"{name}: NULL handle")
    for k in ("start", "ret", "alerts", "ws"):
        assert call(**{k: None}) == (-1, f"{name}: NULL argument"), k
    for k in ("t", "used", "streak", "budget", "n_days", "county_w", "year_i", "coef_col", "sample", "finished"):
        rc, msg = call(start=view(**{k: 1}))
        assert rc == -1 and msg.startswith(f"{name}: NULL start-state array"), k
    assert call(start=view(hist14=1, episode_return=1)) == (-1, f"{name}: NULL handle")  # not read
    for steps in (0, -2):
        assert call(n_steps=steps) == (-1, f"{name}: n_steps must be positive")
    assert call(masks=P, mask_words=0) == (-1, f"{name}: mask_words must be positive")
    for b in (-1, 1024, 1 << 30):
        assert call(max_budget=b) == (-1, f"{name}: max_budget must lie in 0..1023")
    assert call(max_budget=1023) == (-1, f"{name}: NULL handle")
    # no handle, no size (an n_samples beyond the per-draw arrays needs a handle: tests/test_hindsight_posterior_curve_gpu.py)
    assert lib.w2a_hindsight_posterior_curve_workspace_bytes(None, 10, 5, 1) == 0


def test_stats_take_the_new_output():
    """budget_curve_by_group and allocate_budget on a dict with hindsight_posterior_budget_curve()'s keys, shapes and
    dtypes (a NaN row and a row of 0 among them)"""
    rng = np.random.default_rng(3)
    n, G = 24, 5
    out = {"return": torch.as_tensor(-np.abs(rng.standard_normal((n, B + 1))).cumsum(1).astype(np.float32)),
           "alerts": torch.as_tensor(np.minimum(rng.integers(0, B + 1, (n, B + 1)), np.arange(B + 1)).astype(np.int32)),
           "own_budget": torch.as_tensor(rng.integers(0, 9, n).astype(np.int32))}
    out["return"][4] = float("nan")
    out["return"][7] = 0.0
    group = torch.as_tensor(np.arange(n) % G)
    by = stats.budget_curve_by_group(out["return"], group, G)
    assert by["curve"].shape == (G, B + 1) and by["curve"].dtype == torch.float64
    assert int(by["skipped"].sum()) == 1 and int(by["count"].sum()) == n - 1
    ret = out["return"].double().numpy()
    good = ~np.isnan(ret).any(1)
    for g in range(G):
        np.testing.assert_allclose(by["curve"][g].numpy(), ret[(np.arange(n) % G == g) & good].mean(0), rtol=1e-13)
    got = stats.allocate_budget(by["curve"], 7, by["count"])
    assert got["budget"].shape == (G,) and got["spent"] <= 7 and 0 <= int(got["budget"].min()) <= int(got["budget"].max()) <= B
    val = float((by["count"].double() * by["curve"][torch.arange(G), got["budget"]]).sum())
    assert abs(val - got["value"]) <= 1e-9
    own = float((by["count"].double() * by["curve"][:, 0]).sum())
    assert got["value"] >= own  # spending nothing is among the choices
