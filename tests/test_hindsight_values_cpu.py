"""CPU checks of hindsight_values(): the fp64 restatement (tests/hindsight_values_restatement.py) against brute force
over all remaining schedules for horizons of at most 6 days, its losses against its regret, the cases' thresholds, and
the C ABI of w2a_hindsight_along / w2a_relabel_imitation_* (header, binding, what they refuse without a GPU)."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

from weather2alert_amd import _ffi, build, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "w2a.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hindsight_values_cases as K  # noqa: E402
from hindsight_restatement import brute_force_fp64, horizon, own_draw_returns  # noqa: E402
from hindsight_values_restatement import hindsight_values_fp64, walk  # noqa: E402
from test_hindsight_cpu import random_starts  # noqa: E402

P = 4096  # a non-NULL, 256-B aligned address that is never read


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.load()


def _one(start, e, **over):
    st = {k: np.array([np.asarray(v)[e]]) for k, v in start.items()}
    for k, v in over.items():
        st[k] = np.array([v])
    return st


@pytest.mark.parametrize("gated", [False, True])
def test_restatement_equals_brute_force(gated):
    """Q0, Q1 and the expert bit in every state a random schedule reaches: r_a of the day (one day of the own-draw
    return) plus the best of every remaining schedule from the next state, by brute_force_fp64. The brute force knows
    no gate: with one, closed days must give no Q1 and no expert bit. In both forms the losses telescope: V_0(start)
    less the regret is what the schedule's issued alerts earn."""
    ct = tables.CompiledTables.load_npz(os.path.join(K.GOLDEN, "mini_compiled.npz"))
    Y, Ks = len(ct.years), ct.n_samples
    rng = np.random.default_rng(12)
    n_alert_states = 0
    for n_steps in (1, 3, 6):
        start = random_starts(ct, 12, rng, n_steps)
        start["budget"][:3] = [0, 1, n_steps + 3]
        start["used"][:3] = 0
        sched = rng.random((12, ct.T)) < 0.5
        gate = (rng.random((12, ct.T)) < 0.5) if gated else None
        ref = hindsight_values_fp64(ct.X, ct.W, Ks, Y, start, n_steps, sched, gate)
        np.testing.assert_allclose(ref["loss"].sum(0), ref["regret"], rtol=0, atol=1e-12)
        assert (ref["loss"] >= 0).all()
        for e in range(12):
            st = {k: int(start[k][e]) for k in start}
            H = horizon(st, n_steps)
            issued, js, ss = walk(st, H, sched[e], None if gate is None else gate[e])
            assert issued.sum() <= max(0, st["budget"] - st["used"])
            # the losses telescope: V_0(start) less what the schedule earns
            row = np.zeros((1, ct.T), bool)
            row[0, st["t"]:st["t"] + H] = issued.astype(bool)
            earned = own_draw_returns(ct.X, ct.W, Ks, Y, _one(start, e), row, n_steps)[0]
            assert abs(ref["value"][0, e] - ref["regret"][e] - earned) <= 1e-9
            if gated:
                closed = ~gate[e, st["t"]:st["t"] + H]
                assert np.isnan(ref["q1"][:H, e][closed]).all() and not ref["expert"][e, st["t"]:st["t"] + H][closed].any()
                continue
            for d in range(H):
                here = _one(start, e, t=st["t"] + d, used=st["used"] + js[d], streak=ss[d])
                can = st["used"] + js[d] < st["budget"]
                q = []
                for a in (0, 1):
                    day = np.zeros((1, ct.T), bool)
                    day[0, st["t"] + d] = bool(a)
                    r = own_draw_returns(ct.X, ct.W, Ks, Y, here, day, 1)[0]
                    last = st["t"] + d + 1 >= st["n_days"] or d + 1 >= n_steps
                    nxt = _one(start, e, t=st["t"] + d + 1, used=st["used"] + js[d] + a, streak=ss[d] + 1 if a else 0)
                    q.append(r + (0.0 if last else brute_force_fp64(ct.X, ct.W, Ks, Y, nxt, n_steps - d - 1, 0)[0]))
                assert abs(ref["q0"][d, e] - q[0]) <= 1e-9
                if can:
                    assert abs(ref["q1"][d, e] - q[1]) <= 1e-9 and abs(ref["gain"][d, e] - (q[1] - q[0])) <= 1e-9
                    if abs(q[1] - q[0]) > 1e-9:
                        assert ref["expert"][e, st["t"] + d] == (q[1] > q[0])
                    n_alert_states += 1
                else:
                    assert np.isnan(ref["q1"][d, e]) and np.isnan(ref["gain"][d, e]) and not ref["expert"][e, st["t"] + d]
                assert abs(ref["value"][d, e] - (max(q) if can else q[0])) <= 1e-9
            assert np.isnan(ref["gain"][H:, e]).all() and (ref["value"][H:, e] == 0).all()
    assert gated or n_alert_states > 20


def test_case_thresholds():
    """the budgets of the cases sit where the kernel changes path: 8 is the last U with one 64-state chunk, 40 needs
    several chunks and fits in LDS at T = 153, 200 does not; 100 days on every DP fits"""
    ns = lambda U: (U + 1) * (U + 4) // 2  # noqa: E731
    assert ns(8) <= 64 < ns(9) and ns(40) > 64
    assert K.lds_fits(40, 153) and not K.lds_fits(153, 153) and K.lds_fits(153 - 100, 153)
    assert K.lds_fits(56, 153) and not K.lds_fits(57, 153)
    s = K.schedule(K.N, 153, 0.5, 1)
    assert s.shape == (K.N, 153) and 0.4 < s.mean() < 0.6


def test_entry_points_declared_exported_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint w2a_hindsight_along\s*\(([^;]*)\);", text)
    assert m and len(m.group(1).split(",")) == 15 == len(lib.w2a_hindsight_along.argtypes)
    for name, sib in (("w2a_relabel_imitation_linear", "w2a_imitation_gradient_linear_gated"),
                      ("w2a_relabel_imitation_mlp", "w2a_imitation_gradient_mlp_gated")):
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", text)
        assert m and "const uint32_t *labels" in m.group(1)
        assert len(m.group(1).split(",")) == len(getattr(lib, name).argtypes) == len(getattr(lib, sib).argtypes) + 1
        assert name in _ffi.SYMBOLS and not name.startswith("w2a_imitation_gradient_")
    assert lib.w2a_abi_version() == 18


def test_hindsight_along_refuses_on_the_host(lib):
    bufs = {k: (C.c_int32 * 4)() for k in _ffi.STATE_FIELDS}
    v = _ffi.StateView()
    for k in _ffi.STATE_FIELDS:
        setattr(v, k, C.addressof(bufs[k]))
    ok = dict(start=C.byref(v), n_steps=3, alert_mask=P, mask_words=5, allowed_days=None, allowed_words=0, gain=P,
              expert=P, regret=P, value=None, loss=None, ws=P, ws_bytes=4096, stream=None)

    def call(**bad):
        a = dict(ok, **bad)
        return lib.w2a_hindsight_along(None, *a.values()), lib.w2a_last_error().decode()

    assert call() == (-1, "w2a_hindsight_along: NULL handle")  # value_out, loss_out and allowed_days may be NULL
    assert call(value=P, loss=P, allowed_days=P) == (-1, "w2a_hindsight_along: NULL handle")
    for k in ("start", "alert_mask", "gain", "expert", "regret", "ws"):
        assert call(**{k: None}) == (-1, "w2a_hindsight_along: NULL argument"), k
    assert call(n_steps=0) == (-1, "w2a_hindsight_along: n_steps must be positive")
    assert call(mask_words=0) == (-1, "w2a_hindsight_along: mask_words must be positive")


@pytest.mark.parametrize("kind", ["linear", "mlp"])
def test_relabel_entry_points_check_the_handle_first(lib, kind):
    """the sibling's checks in the sibling's order (its texts, under the new name), the handle before the labels"""
    name = f"w2a_relabel_imitation_{kind}"
    if kind == "linear":
        pol = _ffi.LinearPolicy(weight=P, bias=P, group=None, n_groups=1, sample=1, require_budget=0, seed=0)
    else:
        pol = _ffi.MlpPolicy(params=P, group=None, order=None, n_groups=1, n_layers=2, width=64, activation=0, sample=1,
                             require_budget=0, seed=0)
    ok = dict(alert_mask=P, mask_words=0, labels=P, env_weight=None, day_weight=None, day_weight_days=0, n_steps=3, obs=P,
              grad=P, loglik=P, days=P)
    if kind == "mlp":
        ok.update(workspace=P, workspace_bytes=1 << 20)
    ok.update(stream=None, allowed_days=None, allowed_words=0)

    def call(**bad):
        a = dict(ok, **bad)
        return getattr(lib, name)(None, C.byref(pol), *a.values()), lib.w2a_last_error().decode()

    assert call() == (-1, f"{name}: NULL handle")
    assert call(labels=None) == (-1, f"{name}: NULL handle")
    assert call(alert_mask=None) == (-1, f"{name}: NULL alert_mask (the schedule to score)")
    assert call(n_steps=0, alert_mask=None) == (-1, f"{name}: n_steps must be positive")
    assert call(obs=None, grad=None) == (-1, f"{name}: NULL obs (the rows the agent holds are the first day's input)")
    assert call(days=None) == (-1, f"{name}: NULL grad, loglik or days")
    assert call(day_weight=P, day_weight_days=2) == (-1, f"{name}: day_weight holds fewer call-days than n_steps")
    if kind == "mlp":
        assert call(workspace=None) == (-1, f"{name}: NULL workspace")


def test_python_signatures():
    from weather2alert_amd import HeatAlertVecEnv

    sig = inspect.signature(HeatAlertVecEnv.hindsight_values)
    assert list(sig.parameters)[1:] == ["alert_days", "start_state", "n_steps", "allowed_days", "value", "loss"]
    assert inspect.signature(HeatAlertVecEnv.imitation_gradient).parameters["labels"].default is None
    import torch
    from weather2alert_amd import policy

    good = torch.zeros((5, 40), dtype=torch.bool)
    assert policy.check_schedule(good, "labels", 5, 40, "cpu", "f()").shape == (5, 2)
    words = torch.zeros((5, 2), dtype=torch.int32)
    assert policy.check_schedule(words, "labels", 5, 40, "cpu", "f()") is not None
    for bad in (None, good[:4], good.float(), good[:, :39], torch.zeros((5, 3), dtype=torch.int32)):
        with pytest.raises(ValueError, match="labels"):
            policy.check_schedule(bad, "labels", 5, 40, "cpu", "f()")
