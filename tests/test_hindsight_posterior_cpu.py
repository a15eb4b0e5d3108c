"""CPU checks of the hindsight optimum with the draw unknown: the two fp64 restatements
(tests/hindsight_posterior_restatement.py) against each other on the mini synth tables and on the ragged table of
tests/table_edges.py, the n_samples = 1 case against tests/hindsight_restatement.py, what
hindsight_posterior_optimum() refuses before it touches a device, and the C ABI of w2a_hindsight_posterior (header,
binding, host-side refusals and the workspace size without a GPU)."""
import ctypes as C
import inspect
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from weather2alert_amd import HeatAlertVecEnv, _ffi, build, synth, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "w2a.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402
from hindsight_posterior_restatement import (brute_force_posterior_fp64, hindsight_posterior_fp64,  # noqa: E402
                                             posterior_mean_returns)
from hindsight_restatement import hindsight_fp64, horizon  # noqa: E402
from test_hindsight_cpu import random_starts  # noqa: E402

P = 4096  # a non-NULL, 256-B aligned address that is never read
NAMES = ("w2a_hindsight_posterior_workspace_bytes", "w2a_hindsight_posterior", "w2a_hindsight_posterior_gated")


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.load()


@pytest.fixture(scope="module")
def ct():
    return tables.compile_from_synth(synth.make_synth("linear", n_fips=30, years=[2006, 2007], n_samples=6, seed=17,
                                                      extra_confounder_fips=3))


def _check(ct, start, n_steps, gate=None):
    Y, K = len(ct.years), ct.n_samples
    val, days, alerts = hindsight_posterior_fp64(ct.X, ct.W, K, Y, start, n_steps, gate)
    # the DP's own value is what its schedule earns on average over the draws
    np.testing.assert_allclose(posterior_mean_returns(ct.X, ct.W, K, Y, start, days, n_steps), val, rtol=0, atol=1e-12)
    for e in range(len(val)):
        best, _ = brute_force_posterior_fp64(ct.X, ct.W, K, Y, start, n_steps, e, gate)
        assert abs(val[e] - best) <= 1e-12, (e, val[e], best)
        H = horizon({k: int(start[k][e]) for k in start}, n_steps)
        t0 = int(start["t"][e])
        assert alerts[e] == days[e].sum() <= max(0, int(start["budget"][e] - start["used"][e]))
        assert not days[e, :t0].any() and not days[e, t0 + H:].any()
        if gate is not None:
            assert not (days[e] & ~gate[e]).any()
    return val, days, alerts


@pytest.mark.parametrize("n_steps", [1, 5, 8])
def test_dp_equals_brute_force_on_the_mini_synth_tables(ct, n_steps):
    rng = np.random.default_rng(40 + n_steps)
    start = random_starts(ct, 8, rng, n_steps)
    start["budget"][:3] = [0, 1, n_steps + 3]  # budget 0, 1 and >= H are always among them
    start["used"][:3] = 0
    _, days, alerts = _check(ct, start, n_steps)
    assert alerts[0] == 0 and not days[0].any()
    gate = rng.random((8, ct.T)) < 0.5
    _check(ct, start, n_steps, gate)
    start["finished"][:] = 1  # nothing to choose
    val, days, alerts = hindsight_posterior_fp64(ct.X, ct.W, ct.n_samples, len(ct.years), start, n_steps)
    assert (val == 0).all() and not days.any() and (alerts == 0).all()


@pytest.mark.parametrize("n_steps", [1, 5, 8])
def test_dp_equals_brute_force_on_the_ragged_table(n_steps):
    """episodes of 1, 2 and 3 days and the full-length one among them: the stretch stops after the terminal day"""
    rt = E.make_tables()["ragged"].ct
    rng = np.random.default_rng(60 + n_steps)
    start = random_starts(rt, 10, rng, n_steps)
    nd_tab = np.asarray(rt.n_days).reshape(-1, rt.Y)
    for i, d in enumerate(E.SHORTEST + (rt.T,)):
        cw, yi = np.argwhere(nd_tab == d)[0]
        start["county_w"][i], start["year_i"][i], start["n_days"][i] = cw, yi, d
        start["t"][i] = min(int(start["t"][i]), d - 1)
        start["budget"][i], start["used"][i], start["streak"][i] = 3, 0, 0
    _check(rt, start, n_steps)


def test_one_draw_is_the_hindsight_optimum(ct):
    """n_samples = 1: the mean over draws is the draw, so both restatements are one"""
    ct1 = tables.compile_from_synth(synth.make_synth("linear", n_fips=30, years=[2006, 2007], n_samples=1, seed=17,
                                                     extra_confounder_fips=3))
    rng = np.random.default_rng(5)
    for n_steps in (5, 40):
        start = random_starts(ct1, 8, rng, n_steps)
        assert (start["sample"] == 0).all()
        a = hindsight_posterior_fp64(ct1.X, ct1.W, 1, len(ct1.years), start, n_steps)
        b = hindsight_fp64(ct1.X, ct1.W, 1, len(ct1.years), start, n_steps)
        np.testing.assert_allclose(a[0], b[0], rtol=0, atol=1e-12)
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(a[2], b[2])
    # and with several draws it does not read `sample`
    start = random_starts(ct, 8, rng, 9)
    a = hindsight_posterior_fp64(ct.X, ct.W, ct.n_samples, len(ct.years), start, 9)
    start["sample"] = (start["sample"] + 1) % ct.n_samples
    b = hindsight_posterior_fp64(ct.X, ct.W, ct.n_samples, len(ct.years), start, 9)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_python_refusals_on_a_bare_env(ct):
    """every refusal is raised before a device or the library is touched; a posterior_mean env is NOT refused"""
    env = object.__new__(HeatAlertVecEnv)
    env.ct, env.num_envs, env.device, env.fixes, env.reward_mode = ct, 4, torch.device("cpu"), set(), "sampled"
    env._needs_reset, env._pm = False, False
    env.dtables = types.SimpleNamespace(_slot27_zero=True)
    sig = inspect.signature(HeatAlertVecEnv.hindsight_posterior_optimum)
    assert list(sig.parameters)[1:] == ["start_state", "n_steps", "allowed_days", "share", "posterior_returns"]
    assert sig.parameters["share"].default is True and sig.parameters["posterior_returns"].default is False
    who = r"hindsight_posterior_optimum\(\)"
    st = {k: np.zeros(4, np.int32) for k in ("t", "used", "streak", "budget", "n_days", "county_w", "year_i", "coef_col",
                                             "sample", "finished")}
    for pm in (False, True):
        env._pm = pm
        with pytest.raises(ValueError, match="allowed_days"):
            env.hindsight_posterior_optimum(allowed_days=np.zeros((3, ct.T), bool))
        with pytest.raises(KeyError, match="sample"):
            env.hindsight_posterior_optimum({k: v for k, v in st.items() if k != "sample"})
        with pytest.raises(ValueError, match="shape"):
            env.hindsight_posterior_optimum({k: v[:3] for k, v in st.items()})
        with pytest.raises(ValueError, match="n_steps must be positive"):
            env.hindsight_posterior_optimum(st, n_steps=0)
    env.fixes = {"lag", "budget"}
    with pytest.raises(ValueError, match=who + r" needs faithful semantics; fixes \['lag'\]"):
        env.hindsight_posterior_optimum()
    env.fixes = {"budget"}
    env.dtables = types.SimpleNamespace(_slot27_zero=False)
    with pytest.raises(ValueError, match=who + ".*slot-27"):
        env.hindsight_posterior_optimum()
    # the existing calls see what they saw: the posterior_mean refusal between the two shared checks
    env._pm = True
    with pytest.raises(ValueError, match=r"hindsight_optimum\(\) needs reward_mode='sampled', not 'posterior_mean'"):
        env.hindsight_optimum()
    env._pm = False
    with pytest.raises(ValueError, match=r"hindsight_optimum\(\): some coefficient row has a nonzero slot-27"):
        env.hindsight_optimum()


def test_entry_points_declared_exported_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bsize_t w2a_hindsight_posterior_workspace_bytes\s*\(int64_t num_envs, int32_t T, int32_t "
                     r"n_samples, int32_t n_steps,\s*int32_t max_remaining, int32_t big_envs\);", text)
    m = re.search(r"\bint w2a_hindsight_posterior\s*\(([^;]*)\);", text)
    o = re.search(r"\bint w2a_hindsight_optimum\s*\(([^;]*)\);", text)
    assert m and re.sub(r"\s+", " ", m.group(1)) == re.sub(r"\s+", " ", o.group(1))  # w2a_hindsight_optimum's arguments
    assert len(lib.w2a_hindsight_posterior.argtypes) == 10
    g = re.search(r"\bint w2a_hindsight_posterior_gated\s*\(([^;]*)\);", text)
    assert g and len(g.group(1).split(",")) == 12 == len(lib.w2a_hindsight_posterior_gated.argtypes)
    assert "const uint32_t *allowed_days" in g.group(1)
    header = sorted(set(re.findall(r"\b(w2a_[a-z_0-9]+)\s*\(", text)))
    for s in NAMES:
        assert s in _ffi.SYMBOLS and s in header and hasattr(lib, s)
        assert not s.startswith("w2a_rollout_") and "_gradient_" not in s
    assert lib.w2a_hindsight_posterior.restype is C.c_int and lib.w2a_hindsight_posterior_gated.restype is C.c_int
    assert lib.w2a_hindsight_posterior_workspace_bytes.restype is C.c_size_t
    assert lib.w2a_abi_version() == 18 == _ffi.ABI_VERSION


@pytest.mark.parametrize("name", NAMES[1:])
def test_host_side_refusals_without_gpu(lib, name):
    bufs = {k: (C.c_int32 * 4)() for k in _ffi.STATE_FIELDS}

    def view(**null):
        v = _ffi.StateView()
        for k in _ffi.STATE_FIELDS:
            setattr(v, k, None if k in null else C.addressof(bufs[k]))
        return v

    ok = dict(start=view(), n_steps=3, ret=P, mask=P, mask_words=5, alerts=P, ws=P, ws_bytes=4096, stream=None)
    if name.endswith("_gated"):
        ok.update(allowed_days=P, allowed_words=5)

    def call(**bad):
        a = dict(ok, **bad)
        a["start"] = None if a["start"] is None else C.byref(a["start"])
        return getattr(lib, name)(None, *a.values()), lib.w2a_last_error().decode()

    assert call() == (-1, f"{name}: NULL handle")
    for k in ("start", "ret", "mask", "alerts", "ws"):
        assert call(**{k: None}) == (-1, f"{name}: NULL argument"), k
    for k in ("t", "used", "streak", "budget", "n_days", "county_w", "year_i", "coef_col", "sample", "finished"):
        rc, msg = call(start=view(**{k: 1}))
        assert rc == -1 and msg.startswith(f"{name}: NULL start-state array"), k
    assert call(start=view(hist14=1, episode_return=1)) == (-1, f"{name}: NULL handle")  # not read
    for steps in (0, -2):
        assert call(n_steps=steps) == (-1, f"{name}: n_steps must be positive")
    assert call(mask_words=0) == (-1, f"{name}: mask_words must be positive")


def test_workspace_bytes(lib):
    """non-decreasing in the remaining budget and in the days; the pool starts where 16 B per day + 96 B per draw + the
    DP pass 64 KiB; 0 for what the entry refuses"""
    f = lib.w2a_hindsight_posterior_workspace_bytes
    n, T, K = 1000, 153, 100
    base = f(n, T, K, T, 0, 1)
    assert base == 2 * 4096 + 2 * 4096  # 8 B per env (256-B aligned arrays) and the two 1024-bin tables
    prev = 0
    for steps in (1, 2, 30, 152, 153, 154, 1000):
        row = [f(n, T, K, steps, rem, 1) for rem in (-3, 0, 1, 14, 40, 41, 60, 153, 1 << 30)]
        assert all(b >= a for a, b in zip(row, row[1:])), (steps, row)
        assert row[0] == row[1] == base and row[-1] >= prev
        prev = row[-1]
    assert f(n, T, K, 153, 1 << 30, 1) == f(n, T, K, 1000, 153, 1)  # U is capped by the days

    def lds(u, hb, k):  # include/w2a.h: per day, per draw, per state, per day and 64 states
        ns = (u + 1) * (u + 4) // 2
        return 16 * hb + 96 * k + 16 * ns + 8 * hb * ((ns + 63) // 64)

    u_pool = next(u for u in range(T + 1) if lds(u, T, K) > 65536)
    assert f(n, T, K, T, u_pool - 1, 1) == base < f(n, T, K, T, u_pool, 1)
    assert f(n, T, K, T, u_pool, 64) - base == 64 * (f(n, T, K, T, u_pool, 1) - base)
    assert f(n, T, 1, T, u_pool, 1) == base  # fewer draws leave more room for the DP
    # the largest n_samples the per-draw arrays take at 153 days, and one more
    assert (65536 - 16 * 153) // 96 == 657
    assert f(n, T, 657, T, 10, 1) >= base and f(n, T, 658, T, 10, 1) == 0 and f(n, T, 658, 30, 10, 1) >= base
    for bad in ((0, T, K, T, 1, 1), (n, 0, K, T, 1, 1), (n, 1024, K, T, 1, 1), (n, T, 0, T, 1, 1), (n, T, K, 0, 1, 1),
                (n, T, K, T, 1, 0)):
        assert f(*bad) == 0, bad
