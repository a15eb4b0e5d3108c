"""CPU checks of the policy budget curve: the restatement alone (tests/policy_curve_restatement.py) on the mini golden and
the ragged table, what policy_budget_curve() refuses before it touches a device, the C ABI of w2a_policy_curve_linear
(header, binding, host-side refusals without a GPU), and stats.py taking the restated curves unchanged."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from weather2alert_amd import HeatAlertVecEnv, _ffi, build, stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "w2a.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lookahead_cases as L  # noqa: E402
from policy_curve_restatement import policy_curve_fp64  # noqa: E402

P = 4096  # a non-NULL, 256-B aligned address that is never read
B = 6
N = 48
SYMBOLS = ("w2a_policy_curve_workspace_bytes", "w2a_policy_curve_linear", "w2a_policy_curve_linear_gated")


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.load()


@pytest.fixture(scope="module")
def tabs():
    return L.make_tables()


def _policy(ct, seed=3):
    """one row per group, eager enough to run out of alerts, with a weight on remaining_budget: the columns differ from
    the first day on"""
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((L.G, ct.n_obs)) * 0.4).astype(np.float32)
    W[:, ct.feature_names.index("remaining_budget")] = np.float32(0.15)
    return W, (rng.standard_normal(L.G) * 0.5 + 0.5).astype(np.float32)


def _start(name, tb, n):
    tup = {k: v[:n] for k, v in L.host_tuples(name, tb).items()}
    z = np.zeros(n, np.int64)
    return dict(tup, t=z, used=z, streak=z, hist14=z, finished=z, episode_no=z)


@pytest.fixture(scope="module")
def restated(tabs):
    """name -> (ct, start, weight, bias, group, {case: restated dict}); computed once, shared, left unchanged"""
    out = {}
    for name, tb in tabs.items():
        ct, V = tb[0], tb[2]()
        st = _start(name, tb, N)
        W, b = _policy(ct)
        g = L.groups()[:N]
        gate = np.zeros((N, ct.T), bool)
        gate[:, ::3] = True
        gate[::2, 1::3] = True
        kw = dict(seed=L.SEED, gid0=L.GID0)
        cases = {"plain": policy_curve_fp64(V, ct, st, None, W, b, g, ct.T, B, **kw),
                 "require": policy_curve_fp64(V, ct, st, None, W, b, g, ct.T, B, require_budget=True, **kw),
                 "gate": policy_curve_fp64(V, ct, st, None, W, b, g, ct.T, B, gate=gate, **kw),
                 "sample": policy_curve_fp64(V, ct, st, None, W, b, g, ct.T, B, sample=True, **kw)}
        out[name] = (ct, st, W, b, g, gate, cases)
    return out


@pytest.mark.parametrize("name", ["mini", "ragged"])
def test_restatement_alone(restated, name):
    ct, st, W, b, g, gate, cases = restated[name]
    for case, cv in cases.items():
        assert (cv["alert_days"].sum(-1) == cv["alerts"]).all() and (cv["alerts"] <= np.arange(B + 1)[None, :]).all(), case
        assert not cv["alert_days"][:, 0].any(), case  # column 0 issues no alert
        assert np.isfinite(cv["return"]).all() and (cv["return"] < 0).any(), case
        # nothing outside an env's own days
        days = np.arange(ct.T)[None, None, :] < st["n_days"][:, None, None]
        assert not (cv["alert_days"] & ~days).any() and not (cv["attempt_days"] & ~days).any(), case
    plain = cases["plain"]
    # the weight on remaining_budget: for some env every two columns differ in schedule
    sched = plain["alert_days"]
    pairwise = np.array([all((sched[e, i] != sched[e, j]).any() for i in range(B + 1) for j in range(i))
                         for e in range(N)])
    assert pairwise.any()
    assert (plain["attempts_over_budget"] > 0).any() and (plain["attempts_over_budget"][:, 0] > 0).any()
    assert (plain["attempt_days"].sum(-1) == plain["alerts"] + plain["attempts_over_budget"]).all()
    req = cases["require"]
    assert not req["attempts_over_budget"].any() and (req["attempt_days"] == req["alert_days"]).all()
    assert (req["alerts"] > 0).any()
    gt = cases["gate"]
    assert not (gt["alert_days"] & ~gate[:, None, :]).any() and not (gt["attempt_days"] & ~gate[:, None, :]).any()
    assert (gt["alerts"] > 0).any() and (gt["alert_days"] != plain["alert_days"]).any()
    sm = cases["sample"]
    assert (sm["alerts"] > 0).any() and (sm["alert_days"] != plain["alert_days"]).any()


def test_held_rows_from_a_buffer_equal_the_rebuilt_ones(tabs, restated):
    """from reset the buffer's rows are the rebuilt ones: passing them changes nothing (column b overrides the
    remaining-budget column either way)"""
    ct, st, W, b, g, gate, cases = restated["mini"]
    V = tabs["mini"][2]()
    held = V.reset(st["county_w"], st["year_i"], st["coef_col"], st["sample"], st["budget"])
    cv = policy_curve_fp64(V, ct, st, held, W, b, g, ct.T, B, seed=L.SEED, gid0=L.GID0)
    for k in ("return", "alerts", "attempts_over_budget", "alert_days"):
        np.testing.assert_array_equal(cv[k], cases["plain"][k], err_msg=k)
    # a truncated call: the first days of the whole-episode schedules
    cut = policy_curve_fp64(V, ct, st, None, W, b, g, 7, B, seed=L.SEED, gid0=L.GID0)
    np.testing.assert_array_equal(cut["alert_days"][:, :, :7], cases["plain"]["alert_days"][:, :, :7])
    assert not cut["alert_days"][:, :, 7:].any()


# ------------------------------------------------------------------ stats.py takes the dict unchanged
def test_stats_helpers_take_the_curves_unchanged(restated):
    ct, st, W, b, g, gate, cases = restated["ragged"]
    cv = {k: torch.as_tensor(v) for k, v in cases["plain"].items()}
    by = stats.budget_curve_by_group(cv["return"].float(), g, L.G)
    assert by["curve"].shape == (L.G, B + 1) and int(by["count"].sum()) == N and int(by["skipped"].sum()) == 0
    for k in range(L.G):
        np.testing.assert_allclose(by["curve"][k].numpy(), cases["plain"]["return"][g == k].astype(np.float32).mean(0),
                                   rtol=1e-6)
    size = torch.as_tensor(np.bincount(g, minlength=L.G))
    al = stats.allocate_budget(by["curve"], 2 * N, size)
    assert al["budget"].shape == (L.G,) and al["spent"] <= 2 * N and int((al["budget"] * size).sum()) == al["spent"]
    best = float((by["curve"].gather(1, al["budget"][:, None])[:, 0] * size).sum())
    assert al["value"] == pytest.approx(best, rel=1e-12)


# ------------------------------------------------------------------ the env method's refusals, on a bare object
def _bare_env(ct, n=4):
    """An env object no device ever saw: every refusal below is raised before anything else is read."""
    env = object.__new__(HeatAlertVecEnv)
    env.ct, env.num_envs, env.device, env.fixes, env.reward_mode = ct, n, torch.device("cpu"), set(), "sampled"
    env._needs_reset, env._pm = False, False
    return env


def test_refusals_before_anything_touches_a_device(tabs):
    ct = tabs["mini"][0]
    n = 4
    W, b = _policy(ct)
    lin = dict(kind="linear", weight=W[:1], bias=b[:1])
    env = _bare_env(ct, n)
    mlp = dict(kind="mlp", layers=[(np.zeros((5, ct.n_obs), np.float32), np.zeros(5, np.float32)),
                                   (np.zeros((2, 5), np.float32), np.zeros(2, np.float32))])
    with pytest.raises(ValueError, match=r"policy_budget_curve\(\).*mlp.*later addition"):
        env.policy_budget_curve(mlp, B)
    for pol in (dict(kind="always"), dict(kind="bernoulli", p=0.1), {}, None):
        with pytest.raises(ValueError, match=r"policy_budget_curve\(\).*kind 'linear'"):
            env.policy_budget_curve(pol, B)
    with pytest.raises(ValueError, match=r"policy_budget_curve\(\).*lookahead"):
        env.policy_budget_curve({**lin, "lookahead": {"feature": "heat_qi", "days": 3}}, B)
    for bad in (-1, 1024, 2.0, True, None, "3"):
        with pytest.raises(ValueError, match="max_budget must be an int in 0..1023"):
            env.policy_budget_curve(lin, bad)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="n_steps"):
            env.policy_budget_curve(lin, B, n_steps=bad)
    with pytest.raises(ValueError, match="4294967296|more than"):  # the siblings' 4 GiB cap of the schedules
        big = _bare_env(ct, 1 << 22)
        big.policy_budget_curve(lin, 63, schedules=True)
    pm = _bare_env(ct, n)
    pm._pm, pm.reward_mode = True, "posterior_mean"
    with pytest.raises(ValueError, match="sampled"):
        pm.policy_budget_curve(lin, B)
    for fixes in ({"lag"}, {"budget", "obs"}):
        fx = _bare_env(ct, n)
        fx.fixes = fixes
        with pytest.raises(ValueError, match="faithful"):
            fx.policy_budget_curve(lin, B)
    ok_fix = _bare_env(ct, n)
    ok_fix.fixes = {"budget"}
    cold = _bare_env(ct, n)
    cold._needs_reset = True
    with pytest.raises(ValueError, match="needs a reset"):
        cold.policy_budget_curve(lin, B)
    # whatever rollout(linear) refuses of the policy (the same checks, on the host)
    for e in (env, ok_fix):
        for bad in (dict(weight=W[:1, :-1]), dict(bias=b[:2]), dict(group=np.zeros(n - 1, np.int64)),
                    dict(group=np.ones(n, np.int64)), dict(weight=np.full_like(W[:1], np.inf)),
                    dict(allowed_days=np.ones((n, ct.T - 1), bool)), dict(allowed_days=np.ones((n, ct.T), np.float32))):
            with pytest.raises(ValueError):
                e.policy_budget_curve({**lin, **bad}, B)


# ------------------------------------------------------------------ the C ABI
def test_header_and_binding_agree(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in SYMBOLS:
        assert s in _ffi.SYMBOLS and hasattr(lib, s), s
        m = re.search(r"\b" + s + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, s
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(getattr(lib, s).argtypes), s
        # outside the prefixes tests/test_policy_entry_refusals_cpu.py pins
        assert not s.startswith(("w2a_rollout_linear", "w2a_rollout_mlp", "w2a_policy_gradient_",
                                 "w2a_imitation_gradient_", "w2a_surrogate_gradient_", "w2a_value_gradient_"))
    assert lib.w2a_policy_curve_linear_gated.argtypes[:-2] == lib.w2a_policy_curve_linear.argtypes
    assert lib.w2a_abi_version() == _ffi.ABI_VERSION == 18
    assert lib.w2a_policy_curve_workspace_bytes.restype is C.c_size_t
    assert lib.w2a_policy_curve_workspace_bytes(None, 153, 19) == 0


def _c_call(lib, name="w2a_policy_curve_linear", **bad):
    """one call with a NULL handle and otherwise good arguments, `bad` put in; returns (return code, error text)"""
    pol = _ffi.LinearPolicy(weight=P, bias=P, group=None, n_groups=1, sample=0, require_budget=0, seed=0)
    v = _ffi.StateView(**{k: P for k in _ffi.STATE_FIELDS})
    a = dict(policy=C.byref(pol), start=C.byref(v), n_steps=10, max_budget=B, obs=P, ret=P, alerts=P, over=P, masks=P,
             words=5, ws=P, ws_bytes=256, stream=None)
    for k, x in bad.items():
        if k.startswith("p."):
            setattr(pol, k[2:], x)
        elif k.startswith("v."):
            setattr(v, k[2:], x)
        else:
            a[k] = x
    args = [None] + [a[k] for k in ("policy", "start", "n_steps", "max_budget", "obs", "ret", "alerts", "over", "masks",
                                    "words", "ws", "ws_bytes", "stream")]
    if name.endswith("_gated"):
        args += [P, 5]
    rc = getattr(lib, name)(*args)
    return rc, lib.w2a_last_error().decode()


@pytest.mark.parametrize("name", SYMBOLS[1:])
def test_c_level_refusals_without_a_gpu(lib, name):
    checks = [({"policy": None}, "NULL policy"), ({"n_steps": 0}, "n_steps must be positive"),
              ({"p.weight": None}, "NULL weight or bias"), ({"p.n_groups": 0}, "n_groups must be positive"),
              ({"p.sample": 2}, "sample must be 0 or 1"), ({"p.require_budget": 3}, "require_budget must be 0 or 1"),
              ({"p.weight": P + 4}, "weight must be 16-B aligned"),
              ({"start": None}, "NULL argument"), ({"ret": None}, "NULL argument"), ({"alerts": None}, "NULL argument"),
              ({"over": None}, "NULL argument"),
              ({"v.hist14": None}, "NULL start-state array (t, streak, hist14, n_days, county_w, year_i, coef_col, "
                                   "sample, episode_no and finished are read)"),
              ({"v.episode_no": None}, "NULL start-state array (t, streak, hist14, n_days, county_w, year_i, coef_col, "
                                       "sample, episode_no and finished are read)"),
              ({"words": 0}, "mask_words must be positive"),
              ({"max_budget": -1}, "max_budget must lie in 0..1023"), ({"max_budget": 1024}, "max_budget must lie in 0..1023"),
              ({"ws": None}, "NULL workspace"), ({"ws": P + 16}, "workspace must be 256-B aligned")]
    assert _c_call(lib, name) == (-1, f"{name}: NULL handle")
    # what the kernel does not read may be NULL; without schedules mask_words is not read; a NULL obs asks for the rebuilt rows
    for free in ({"v.used": None, "v.budget": None}, {"masks": None, "words": 0}, {"obs": None}):
        assert _c_call(lib, name, **free) == (-1, f"{name}: NULL handle")
    for bad, text in checks:
        assert _c_call(lib, name, **bad) == (-1, f"{name}: {text}"), bad
    # two bad arguments: the earlier check reports
    for i, (bad1, text1) in enumerate(checks):
        for bad2, _ in checks[i + 1:]:
            if bad1.keys() & bad2.keys() or text1 == _:
                continue
            assert _c_call(lib, name, **{**bad2, **bad1}) == (-1, f"{name}: {text1}"), (bad1, bad2)
