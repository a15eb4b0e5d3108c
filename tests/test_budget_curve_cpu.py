"""CPU checks of the hindsight budget curve: the (remaining, streak) restatement (tests/budget_curve_restatement.py)
against tests/hindsight_restatement.py's optimum of every twin with budget = used + b on the mini goldens, what
hindsight_budget_curve() refuses before it touches a device, the C ABI of w2a_hindsight_curve (header, binding,
host-side refusals without a GPU), and the two host helpers of stats.py."""
import ctypes as C
import inspect
import itertools
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from weather2alert_amd import HeatAlertVecEnv, _ffi, build, stats, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "w2a.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from budget_curve_restatement import budget_curve_fp64, twin  # noqa: E402
from hindsight_restatement import hindsight_fp64  # noqa: E402
from test_hindsight_cpu import random_starts  # noqa: E402

P = 4096  # a non-NULL, 256-B aligned address that is never read
B = 8


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.load()


@pytest.fixture(scope="module")
def ct():
    return tables.CompiledTables.load_npz(os.path.join(GOLDEN, "mini_compiled.npz"))


def _check_columns(ct, start, n_steps, gate=None):
    Y, K = len(ct.years), ct.n_samples
    got = budget_curve_fp64(ct.X, ct.W, K, Y, start, n_steps, B, gate)
    n_alerts = 0
    for b in range(B + 1):
        val, days, alerts = hindsight_fp64(ct.X, ct.W, K, Y, twin(start, b), n_steps)
        np.testing.assert_allclose(got["value"][:, b], val, rtol=0, atol=1e-9, err_msg=f"b = {b}")
        np.testing.assert_array_equal(got["alert_days"][:, b], days, err_msg=f"b = {b}")
        np.testing.assert_array_equal(got["alerts"][:, b], alerts, err_msg=f"b = {b}")
        assert (alerts <= b).all()
        # the f32 re-adding: H roundings of sums below sum |r|
        bound = got["H"] * 2.0 ** -24 * np.maximum(np.abs(val), 1.0) * 2
        assert (np.abs(got["return32"][:, b].astype(np.float64) - val) <= bound).all(), b
        n_alerts += int(alerts.sum())
    return got, n_alerts


@pytest.mark.parametrize("n_steps", [9, 40, 153])
def test_columns_equal_the_twins_from_day_0(ct, n_steps):
    rng = np.random.default_rng(n_steps)
    start = random_starts(ct, 6, rng, n_steps)
    for k in ("t", "used", "streak"):
        start[k][:] = 0
    got, n_alerts = _check_columns(ct, start, n_steps)
    assert n_alerts > 0 and not got["alert_days"][:, 0].any()


@pytest.mark.parametrize("n_steps", [9, 153])
def test_columns_equal_the_twins_mid_episode(ct, n_steps):
    """used > 0 and a running start streak: the continuation family carries s0 + m; an env finished on entry and one on
    its last day are among them"""
    rng = np.random.default_rng(100 + n_steps)
    start = random_starts(ct, 8, rng, n_steps)
    start["t"][:6] = rng.integers(20, 120, 6)
    start["used"][:6] = rng.integers(1, 6, 6)
    start["streak"][:6] = [1, 2, 3, 4, 1, 2]
    start["t"][6] = start["n_days"][6] - 1
    start["finished"][7] = 1
    got, n_alerts = _check_columns(ct, start, n_steps)
    assert n_alerts > 0 and (start["streak"] > 0).sum() >= 6
    assert (got["value"][7] == 0).all() and not got["alert_days"][7].any() and got["H"][6] == 1


def test_python_refusals_on_a_bare_env(ct):
    """every refusal is raised before a device or the library is touched"""
    env = object.__new__(HeatAlertVecEnv)
    env.ct, env.num_envs, env.device, env.fixes, env.reward_mode = ct, 4, torch.device("cpu"), set(), "sampled"
    env._needs_reset, env._pm = False, False
    env.dtables = types.SimpleNamespace(_slot27_zero=True)
    sig = inspect.signature(HeatAlertVecEnv.hindsight_budget_curve)
    assert list(sig.parameters)[1:] == ["max_budget", "start_state", "n_steps", "allowed_days", "schedules", "packed"]
    for bad in (-1, 1024, 3.0, "8", None, True):
        with pytest.raises(ValueError, match=r"hindsight_budget_curve\(\): max_budget must be an int in 0\.\.1023"):
            env.hindsight_budget_curve(bad)
    env.num_envs = 1 << 22
    with pytest.raises(ValueError, match=r"schedules of 4194304 envs x 9 budgets need 6530531328 bytes"):
        env.hindsight_budget_curve(8, schedules=True)
    with pytest.raises(ValueError, match=r"need 29024583680 bytes"):
        env.hindsight_budget_curve(345, schedules=True, packed=True)
    env.num_envs = 4
    with pytest.raises(ValueError, match="allowed_days"):
        env.hindsight_budget_curve(8, allowed_days=np.zeros((3, ct.T), bool))
    env._pm = True
    with pytest.raises(ValueError, match=r"hindsight_budget_curve\(\) needs reward_mode='sampled', not 'posterior_mean'"):
        env.hindsight_budget_curve(8)
    env._pm = False
    env.fixes = {"lag", "budget"}
    with pytest.raises(ValueError, match=r"hindsight_budget_curve\(\) needs faithful semantics; fixes \['lag'\]"):
        env.hindsight_budget_curve(8)
    env.fixes = set()
    env.dtables = types.SimpleNamespace(_slot27_zero=False)
    with pytest.raises(ValueError, match="slot-27"):
        env.hindsight_budget_curve(8)


def test_entry_points_declared_exported_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bsize_t w2a_hindsight_curve_workspace_bytes\s*\(const w2a_env \*env, int32_t n_steps, int32_t "
                     r"max_budget, int32_t big_envs\);", text)
    m = re.search(r"\bint w2a_hindsight_curve\s*\(([^;]*)\);", text)
    assert m and len(m.group(1).split(",")) == 11 == len(lib.w2a_hindsight_curve.argtypes)
    assert re.search(r"w2a_env \*env, const w2a_state_view \*start, int32_t n_steps, int32_t max_budget,\s*float "
                     r"\*ret_out,\s*int32_t \*alerts_out, uint32_t \*alert_masks, int32_t mask_words, void \*workspace,"
                     r"\s*size_t workspace_bytes, void \*stream", m.group(1))
    g = re.search(r"\bint w2a_hindsight_curve_gated\s*\(([^;]*)\);", text)
    assert g and len(g.group(1).split(",")) == 13 == len(lib.w2a_hindsight_curve_gated.argtypes)
    assert "const uint32_t *allowed_days" in g.group(1)
    header = sorted(set(re.findall(r"\b(w2a_[a-z_]+)\s*\(", text)))
    for s in ("w2a_hindsight_curve_workspace_bytes", "w2a_hindsight_curve", "w2a_hindsight_curve_gated"):
        assert s in _ffi.SYMBOLS and s in header and hasattr(lib, s)
        assert not s.startswith("w2a_rollout_") and "_gradient_" not in s
    assert header == sorted(_ffi.SYMBOLS)
    assert lib.w2a_hindsight_curve.restype is C.c_int and lib.w2a_hindsight_curve_gated.restype is C.c_int
    assert lib.w2a_hindsight_curve_workspace_bytes.restype is C.c_size_t
    assert lib.w2a_abi_version() == 18


@pytest.mark.parametrize("name", ["w2a_hindsight_curve", "w2a_hindsight_curve_gated"])
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
    assert lib.w2a_hindsight_curve_workspace_bytes(None, 10, 5, 1) == 0


# ------------------------------------------------------------------ stats.py
def test_allocate_budget_equals_brute_force():
    rng = np.random.default_rng(5)
    for trial in range(6):
        curves = rng.standard_normal((4, 6)).cumsum(1)  # not monotone
        size = None if trial % 2 == 0 else rng.integers(1, 4, 4)
        sz = np.ones(4, np.int64) if size is None else size
        for total in (0, 1, 4, 7, 11, 60):
            got = stats.allocate_budget(torch.as_tensor(curves), total, None if size is None else torch.as_tensor(size))
            best, arg = -np.inf, None
            for bs in itertools.product(range(6), repeat=4):  # lexicographic: the first maximum has the smallest budgets
                if (sz * bs).sum() <= total:
                    v = float((sz * curves[np.arange(4), bs]).sum())
                    if v > best + 1e-12:
                        best, arg = v, bs
            assert abs(got["value"] - best) <= 1e-9, (trial, total)
            bud = got["budget"].numpy()
            assert (sz * bud).sum() == got["spent"] <= total
            assert abs(float((sz * curves[np.arange(4), bud]).sum()) - best) <= 1e-9
            assert got["budget"].dtype == torch.int64 and tuple(bud) == arg, (trial, total, bud, arg)


def test_allocate_budget_ties_and_empty_groups():
    flat = torch.zeros((3, 5), dtype=torch.float64)
    assert stats.allocate_budget(flat, 9)["budget"].tolist() == [0, 0, 0]  # ties go to the smaller budget
    curves = torch.tensor([[0.0, 1.0, 1.0], [float("nan")] * 3, [0.0, 0.5, 2.0]], dtype=torch.float64)
    got = stats.allocate_budget(curves, 3)
    assert got["budget"].tolist() == [1, 0, 2] and got["value"] == 3.0 and got["spent"] == 3
    with pytest.raises(ValueError, match="NaN"):
        stats.allocate_budget(torch.tensor([[0.0, float("nan")]]), 1)
    with pytest.raises(ValueError, match="total"):
        stats.allocate_budget(flat, -1)
    with pytest.raises(ValueError, match="group_size"):
        stats.allocate_budget(flat, 2, torch.ones(2, dtype=torch.int64))


def test_budget_curve_by_group_skips_nan_rows():
    rng = np.random.default_rng(2)
    curve = rng.standard_normal((11, 4)).astype(np.float32)
    group = np.array([0, 2, 2, 0, 3, 2, 0, 3, 2, 0, 2])
    curve[3, 1] = np.nan   # group 0
    curve[4] = np.nan      # group 3
    curve[7] = np.nan      # group 3: no row left
    out = stats.budget_curve_by_group(torch.as_tensor(curve), torch.as_tensor(group), 5)
    assert out["curve"].dtype == torch.float64 and out["curve"].shape == (5, 4)
    assert out["count"].tolist() == [3, 0, 5, 0, 0] and out["skipped"].tolist() == [1, 0, 0, 2, 0]
    good = ~np.isnan(curve).any(1)
    for g in (0, 2):
        want = curve[(group == g) & good].astype(np.float64).mean(0)
        np.testing.assert_allclose(out["curve"][g].numpy(), want, rtol=1e-14, atol=1e-15)
    assert torch.isnan(out["curve"][[1, 3, 4]]).all()
    with pytest.raises(ValueError, match="group ids"):
        stats.budget_curve_by_group(torch.as_tensor(curve), torch.as_tensor(group), 3)
