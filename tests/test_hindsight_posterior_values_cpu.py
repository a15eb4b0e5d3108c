"""CPU checks of hindsight_posterior_values(): the fp64 restatement (tests/hindsight_posterior_values_restatement.py)
along hindsight_posterior_fp64's own schedule, with one draw against hindsight_values_fp64, and against brute force over
every remaining schedule (brute_force_posterior_fp64) on the suffix after each of the first days; what the call refuses
on an env object no device ever saw; the C ABI of w2a_hindsight_posterior_along (header, binding, what it refuses
without a GPU); and the sharing helper's key and inverse on a hand-made batch."""
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
from hindsight_posterior_restatement import (brute_force_posterior_fp64, hindsight_posterior_fp64,  # noqa: E402
                                             posterior_mean_returns)
from hindsight_posterior_values_restatement import hindsight_posterior_values_fp64  # noqa: E402
from hindsight_restatement import horizon  # noqa: E402
from hindsight_values_restatement import hindsight_values_fp64, walk  # noqa: E402
from test_hindsight_cpu import random_starts  # noqa: E402

P = 4096  # a non-NULL, 256-B aligned address that is never read
NAME = "w2a_hindsight_posterior_along"
FIELDS = ("t", "used", "streak", "budget", "n_days", "county_w", "year_i", "coef_col", "sample", "finished")


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


def _one(start, e, **over):
    st = {k: np.array([np.asarray(v)[e]]) for k, v in start.items()}
    for k, v in over.items():
        st[k] = np.array([v])
    return st


# ------------------------------------------------------------------ the restatement alone
@pytest.mark.parametrize("gated", [False, True])
def test_along_the_restated_optimums_own_schedule(ct, gated):
    """the expert bits are the schedule, every loss and the regret are exactly 0, value[0] is the DP's value"""
    Y, K = len(ct.years), ct.n_samples
    rng = np.random.default_rng(3)
    for n_steps in (5, 40):
        start = random_starts(ct, 8, rng, n_steps)
        start["budget"][:3] = [0, 1, n_steps + 3]
        start["used"][:3] = 0
        gate = (rng.random((8, ct.T)) < 0.5) if gated else None
        val, days, alerts = hindsight_posterior_fp64(ct.X, ct.W, K, Y, start, n_steps, gate)
        ref = hindsight_posterior_values_fp64(ct.X, ct.W, K, Y, start, n_steps, days, gate)
        np.testing.assert_array_equal(ref["expert"], days)
        assert (ref["loss"] == 0).all() and (ref["regret"] == 0).all()
        np.testing.assert_array_equal(ref["value"][0], val)
        assert (ref["issued"].sum(0) == alerts).all() and alerts.sum() > 0
        assert set(ref) == set(hindsight_values_fp64(ct.X, ct.W, K, Y, start, n_steps, days, gate)) | {"abs_reward"}


def test_one_draw_is_hindsight_values():
    """K = 1: the mean over draws is the draw, so the two restatements are one; several draws: `sample` is not read"""
    ct1 = _synth(1)
    rng = np.random.default_rng(5)
    for n_steps in (5, 40):
        start = random_starts(ct1, 8, rng, n_steps)
        sched = rng.random((8, ct1.T)) < 0.4
        gate = rng.random((8, ct1.T)) < 0.6
        for g in (None, gate):
            a = hindsight_posterior_values_fp64(ct1.X, ct1.W, 1, len(ct1.years), start, n_steps, sched, g)
            b = hindsight_values_fp64(ct1.X, ct1.W, 1, len(ct1.years), start, n_steps, sched, g)
            for k in b:
                if b[k].dtype == np.float64:
                    np.testing.assert_allclose(a[k], b[k], rtol=0, atol=1e-12, equal_nan=True, err_msg=k)
                else:
                    np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    ct6 = _synth(6)
    start = random_starts(ct6, 8, rng, 9)
    sched = rng.random((8, ct6.T)) < 0.4
    a = hindsight_posterior_values_fp64(ct6.X, ct6.W, 6, len(ct6.years), start, 9, sched)
    start["sample"] = (start["sample"] + 1) % 6
    b = hindsight_posterior_values_fp64(ct6.X, ct6.W, 6, len(ct6.years), start, 9, sched)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


@pytest.mark.parametrize("n_steps", [3, 8])
def test_restatement_equals_brute_force_on_every_suffix(ct, n_steps):
    """In the state a random schedule reaches on each of the first days: Q_a is the draw-mean reward of the day (one
    day of posterior_mean_returns) plus the best draw-mean return of every remaining schedule from the next state
    (brute_force_posterior_fp64). The losses telescope: value[0] less the regret is what the issued alerts earn on
    average over the draws, and abs_reward bounds that in absolute value."""
    Y, K = len(ct.years), ct.n_samples
    rng = np.random.default_rng(20 + n_steps)
    n = 6
    start = random_starts(ct, n, rng, n_steps)
    start["budget"][:3] = [0, 1, n_steps + 3]
    start["used"][:3] = 0
    sched = rng.random((n, ct.T)) < 0.5
    ref = hindsight_posterior_values_fp64(ct.X, ct.W, K, Y, start, n_steps, sched)
    np.testing.assert_allclose(ref["loss"].sum(0), ref["regret"], rtol=0, atol=1e-12)
    assert (ref["loss"] >= 0).all()
    n_alert_states = 0
    for e in range(n):
        st = {k: int(start[k][e]) for k in start}
        H = horizon(st, n_steps)
        issued, js, ss = walk(st, H, sched[e])
        row = np.zeros((1, ct.T), bool)
        row[0, st["t"]:st["t"] + H] = issued.astype(bool)
        earned = posterior_mean_returns(ct.X, ct.W, K, Y, _one(start, e), row, n_steps)[0]
        assert abs(ref["value"][0, e] - ref["regret"][e] - earned) <= 1e-9
        assert ref["abs_reward"][e] >= abs(earned) - 1e-12 and (H == 0) == (ref["abs_reward"][e] == 0)
        for d in range(H):
            here = _one(start, e, t=st["t"] + d, used=st["used"] + js[d], streak=ss[d])
            can = st["used"] + js[d] < st["budget"]
            q = []
            for a in (0, 1):
                day = np.zeros((1, ct.T), bool)
                day[0, st["t"] + d] = bool(a)
                r = posterior_mean_returns(ct.X, ct.W, K, Y, here, day, 1)[0]
                last = st["t"] + d + 1 >= st["n_days"] or d + 1 >= n_steps
                nxt = _one(start, e, t=st["t"] + d + 1, used=st["used"] + js[d] + a, streak=ss[d] + 1 if a else 0)
                q.append(r + (0.0 if last else brute_force_posterior_fp64(ct.X, ct.W, K, Y, nxt, n_steps - d - 1, 0)[0]))
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
    assert n_alert_states > 5


# ------------------------------------------------------------------ the Python refusals
def _bare_env(ct, n=4):
    """An env object no device ever saw: every refusal below is raised before anything else is read."""
    env = object.__new__(HeatAlertVecEnv)
    env.ct, env.num_envs, env.device, env.fixes, env.reward_mode = ct, n, torch.device("cpu"), set(), "sampled"
    env._needs_reset, env._pm = False, False
    env.dtables = types.SimpleNamespace(_slot27_zero=True)
    return env


def test_python_refusals_on_a_bare_env(ct):
    """hindsight_posterior_optimum()'s checks, hindsight_values()'s schedule check and its strict n_steps; a
    posterior_mean env is NOT refused"""
    env = _bare_env(ct)
    sig = inspect.signature(HeatAlertVecEnv.hindsight_posterior_values)
    assert list(sig.parameters)[1:] == ["alert_days", "start_state", "n_steps", "allowed_days", "value", "loss", "share"]
    assert [sig.parameters[k].default for k in ("start_state", "n_steps", "allowed_days", "value", "loss", "share")] == \
        [None, None, None, False, False, True]
    who = r"hindsight_posterior_values\(\)"
    sched = np.zeros((4, ct.T), bool)
    st = {k: np.zeros(4, np.int32) for k in FIELDS}
    for pm in (False, True):
        env._pm = pm
        for bad in (sched[:3], sched[:, :-1], sched.astype(np.float32), None):
            with pytest.raises(ValueError, match=who + ".*alert_days"):
                env.hindsight_posterior_values(bad)
        with pytest.raises(ValueError, match="allowed_days"):
            env.hindsight_posterior_values(sched, allowed_days=np.zeros((3, ct.T), bool))
        with pytest.raises(KeyError, match="sample"):
            env.hindsight_posterior_values(sched, {k: v for k, v in st.items() if k != "sample"})
        with pytest.raises(ValueError, match="shape"):
            env.hindsight_posterior_values(sched, {k: v[:3] for k, v in st.items()})
        with pytest.raises(ValueError, match="n_steps must be positive"):
            env.hindsight_posterior_values(sched, st, n_steps=0)
        for steps in (2.0, True, "3"):
            with pytest.raises(ValueError, match=who + ": n_steps must be an int"):
                env.hindsight_posterior_values(sched, st, n_steps=steps)
    env.fixes = {"lag", "budget"}
    with pytest.raises(ValueError, match=who + r" needs faithful semantics; fixes \['lag'\]"):
        env.hindsight_posterior_values(sched)
    env.fixes = {"budget"}
    env.dtables = types.SimpleNamespace(_slot27_zero=False)
    with pytest.raises(ValueError, match=who + ".*slot-27"):
        env.hindsight_posterior_values(sched)


# ------------------------------------------------------------------ the C ABI
def test_entry_point_declared_exported_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint " + NAME + r"\s*\(([^;]*)\);", text)
    o = re.search(r"\bint w2a_hindsight_along\s*\(([^;]*)\);", text)
    assert m and re.sub(r"\s+", " ", m.group(1)) == re.sub(r"\s+", " ", o.group(1))  # w2a_hindsight_along's arguments
    assert len(m.group(1).split(",")) == 15 == len(lib.w2a_hindsight_posterior_along.argtypes)
    assert lib.w2a_hindsight_posterior_along.restype is C.c_int
    header = sorted(set(re.findall(r"\b(w2a_[a-z_0-9]+)\s*\(", text)))
    assert NAME in _ffi.SYMBOLS and NAME in header and hasattr(lib, NAME)
    assert not NAME.startswith("w2a_rollout_") and "_gradient_" not in NAME
    assert lib.w2a_abi_version() == 18 == _ffi.ABI_VERSION


def test_entry_refuses_on_the_host(lib):
    """w2a_hindsight_posterior's refusals in its order, under the new name: a NULL env is an error, after the NULL
    arguments, the start-state arrays, n_steps and mask_words"""
    bufs = {k: (C.c_int32 * 4)() for k in _ffi.STATE_FIELDS}

    def view(**null):
        v = _ffi.StateView()
        for k in _ffi.STATE_FIELDS:
            setattr(v, k, None if k in null else C.addressof(bufs[k]))
        return v

    ok = dict(start=view(), n_steps=3, alert_mask=P, mask_words=5, allowed_days=None, allowed_words=0, gain=P,
              expert=P, regret=P, value=None, loss=None, ws=P, ws_bytes=4096, stream=None)

    def call(**bad):
        a = dict(ok, **bad)
        a["start"] = None if a["start"] is None else C.byref(a["start"])
        return lib.w2a_hindsight_posterior_along(None, *a.values()), lib.w2a_last_error().decode()

    assert call() == (-1, f"{NAME}: NULL handle")  # value_out, loss_out and allowed_days may be NULL
    assert call(value=P, loss=P, allowed_days=P, allowed_words=5) == (-1, f"{NAME}: NULL handle")
    for k in ("start", "alert_mask", "gain", "expert", "regret", "ws"):
        assert call(**{k: None}) == (-1, f"{NAME}: NULL argument"), k
    for k in FIELDS:
        rc, msg = call(start=view(**{k: 1}))
        assert rc == -1 and msg.startswith(f"{NAME}: NULL start-state array"), k
    for steps in (0, -2):
        assert call(n_steps=steps) == (-1, f"{NAME}: n_steps must be positive")
    assert call(mask_words=0) == (-1, f"{NAME}: mask_words must be positive")


# ------------------------------------------------------------------ sharing
def test_sharing_key_and_inverse_on_a_hand_made_batch(ct):
    """envs 0, 3 and 5 are one problem under three draws; 1 differs in its streak, 2 in one schedule bit, 4 holds a draw
    outside the tables, 6 is env 2 again. The representatives are the lowest env ids, in front, the rest are marked
    finished, and x[:m][inv] gives every env its representative's answer. Without the schedule 2 and 6 join 0."""
    env = _bare_env(ct, 7)
    st = {k: torch.full((7,), 2, dtype=torch.int32) for k in FIELDS}
    st["finished"].zero_()
    st["sample"] = torch.tensor([0, 1, 2, 3, ct.n_samples, 5, 4], dtype=torch.int32)
    st["streak"][1] = 3
    words = (ct.T + 31) // 32
    sched = torch.zeros((7, words), dtype=torch.int32)
    sched[:, 0] = 0b1010
    sched[2, words - 1] = sched[6, words - 1] = 1 << 7
    sched[5, 1] = sched[0, 1] = sched[3, 1] = -(1 << 31)  # bit 31: the words are compared as they are
    rep, inv, first, m = env._hs_posterior_share(st, sched)
    assert m == 4 and sorted(first.tolist()) == [0, 1, 2, 4]
    assert inv[0] == inv[3] == inv[5] and inv[2] == inv[6] and len({int(inv[i]) for i in (0, 1, 2, 4)}) == 4
    assert torch.equal(first[inv], torch.tensor([0, 1, 2, 0, 4, 0, 2]))
    for k in FIELDS:
        assert torch.equal(rep[k][:m], st[k][first]) and rep[k].dtype == torch.int32 and rep[k].shape == (7,)
    assert (rep["finished"][m:] == 1).all() and (rep["finished"][:m] == 0).all()
    ids = torch.arange(7)
    answer = torch.zeros(7, dtype=torch.int64)
    answer[:m] = ids[first]  # what a per-env output of the library holds in front
    assert torch.equal(answer[:m][inv], first[inv])
    rep0, inv0, first0, m0 = env._hs_posterior_share(st)  # hindsight_posterior_optimum()'s key: no schedule
    assert m0 == 3 and sorted(first0.tolist()) == [0, 1, 4] and inv0[2] == inv0[6] == inv0[0]
