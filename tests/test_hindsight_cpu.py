"""CPU checks of the hindsight optimum: the fp64 DP restatement (tests/hindsight_restatement.py) against brute force
over every feasible schedule on the mini goldens -- mid-episode starts with a running streak, budgets 0, 1 and >= H --
and on coefficient rows whose streak and remaining-budget terms dominate; the C ABI of w2a_hindsight_optimum (header,
binding, host-side refusals without a GPU)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from weather2alert_amd import _ffi, build, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "w2a.h")
ERR_ARG = -1
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hindsight_restatement import brute_force_fp64, hindsight_fp64, horizon, own_draw_returns  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.load()


def random_starts(ct, E, rng, n_steps, budgets=None):
    """E start states on table ct: random (county, year, column, draw), day, budget, alerts used and streak; a quarter
    start at day 0 with no history, the rest mid-episode (a streak > 0 on half of those)."""
    rows = np.flatnonzero(ct.n_days > 0)
    row = rng.choice(rows, E)
    Y = len(ct.years)
    nd = ct.n_days[row].astype(np.int32)
    t = np.where(rng.random(E) < 0.25, 0, rng.integers(0, nd)).astype(np.int32)
    budget = (budgets if budgets is not None else rng.integers(0, 2 * n_steps + 2, E)).astype(np.int32)
    used = np.minimum(rng.integers(0, 6, E), budget) * (t > 0)
    streak = np.where((t > 0) & (rng.random(E) < 0.5), rng.integers(1, 5, E), 0) * (used > 0)
    return dict(t=t, used=used.astype(np.int32), streak=streak.astype(np.int32), hist14=np.zeros(E, np.int32),
                budget=budget, n_days=nd, county_w=(row // Y).astype(np.int32), year_i=(row % Y).astype(np.int32),
                coef_col=rng.integers(0, ct.S, E).astype(np.int32),
                sample=rng.integers(0, ct.n_samples, E).astype(np.int32), finished=np.zeros(E, np.int32))


def check_against_brute_force(ct, W, start, n_steps):
    Y, K = len(ct.years), ct.n_samples
    val, days, alerts = hindsight_fp64(ct.X, W, K, Y, start, n_steps)
    # the DP's own value is what its schedule earns
    np.testing.assert_allclose(own_draw_returns(ct.X, W, K, Y, start, days, n_steps), val, rtol=0, atol=1e-9)
    for e in range(len(val)):
        best, _ = brute_force_fp64(ct.X, W, K, Y, start, n_steps, e)
        assert abs(val[e] - best) <= 1e-9, (e, val[e], best)
        H = horizon({k: int(start[k][e]) for k in start}, n_steps)
        t0 = int(start["t"][e])
        assert alerts[e] == days[e].sum() <= max(0, int(start["budget"][e] - start["used"][e]))
        assert not days[e, :t0].any() and not days[e, t0 + H:].any()
    return val, days, alerts


@pytest.mark.parametrize("data", ["mini", "mini64"])
def test_dp_equals_brute_force_on_the_mini_goldens(data):
    ct = tables.CompiledTables.load_npz(os.path.join(GOLDEN, f"{data}_compiled.npz"))
    assert not ct.W.reshape(-1, 2, 32)[:, :, 27].any()
    rng = np.random.default_rng(7 if data == "mini" else 8)
    for n_steps in (1, 2, 5, 9, 12):
        start = random_starts(ct, 10, rng, n_steps)
        # budget 0, budget 1 and budget >= H are always among them
        start["budget"][:3] = [0, 1, n_steps + 3]
        start["used"][:3] = 0
        _, days, alerts = check_against_brute_force(ct, ct.W, start, n_steps)
        assert alerts[0] == 0 and not days[0].any()
    # episode ends inside the horizon: the stretch stops after the terminal day
    start = random_starts(ct, 6, rng, 12)
    start["t"][:] = start["n_days"] - rng.integers(1, 6, 6)
    check_against_brute_force(ct, ct.W, start, 12)
    # finished envs: nothing to choose
    start["finished"][:] = 1
    val, days, alerts = hindsight_fp64(ct.X, ct.W, ct.n_samples, len(ct.years), start, 12)
    assert (val == 0).all() and not days.any() and (alerts == 0).all()


def test_dp_with_dominant_streak_and_budget_terms():
    """Coefficient rows whose streak (slot 25) and remaining-budget (slot 26) terms dominate the logits: the optimum
    then hinges on exactly what the DP state carries."""
    ct = tables.CompiledTables.load_npz(os.path.join(GOLDEN, "mini_compiled.npz"))
    rng = np.random.default_rng(11)
    W = np.array(ct.W, np.float32).reshape(-1, 2, 32)
    n = W.shape[0]
    W[:, 0, 25] = rng.uniform(-0.6, 0.6, n)
    W[:, 1, 25] = rng.uniform(-1.5, 1.5, n)
    W[:, 0, 26] = rng.uniform(-0.4, 0.4, n)
    W[:, 1, 26] = rng.uniform(-0.8, 0.8, n)
    W[:, 0, 24] = rng.uniform(-0.5, 0.5, n)
    W[:, 1, 24] = rng.uniform(-1.0, 1.0, n)
    W = W.reshape(ct.W.shape)
    n_alerts = 0
    for n_steps in (4, 8, 11):
        start = random_starts(ct, 10, rng, n_steps)
        _, days, alerts = check_against_brute_force(ct, W, start, n_steps)
        n_alerts += alerts.sum()
    assert n_alerts > 0


# ------------------------------------------------------------------ C ABI
def test_entry_points_declared_exported_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bsize_t w2a_hindsight_workspace_bytes\s*\(const w2a_env \*env, int32_t n_steps, int32_t "
                     r"max_remaining, int32_t big_envs\);", text)
    assert re.search(r"\bint w2a_hindsight_optimum\s*\(w2a_env \*env, const w2a_state_view \*start, int32_t n_steps, "
                     r"float \*ret_out,\s*uint32_t \*alert_mask, int32_t mask_words, int32_t \*alerts_out, void "
                     r"\*workspace,\s*size_t workspace_bytes, void \*stream\);", text)
    for s in ("w2a_hindsight_workspace_bytes", "w2a_hindsight_optimum"):
        assert s in _ffi.SYMBOLS and hasattr(lib, s)
    assert lib.w2a_hindsight_optimum.restype is C.c_int and len(lib.w2a_hindsight_optimum.argtypes) == 10
    assert lib.w2a_hindsight_workspace_bytes.restype is C.c_size_t
    assert lib.w2a_abi_version() == 18


def test_host_side_refusals_without_gpu(lib):
    bufs = {k: (C.c_int32 * 4)() for k in _ffi.STATE_FIELDS}

    def view(**null):
        v = _ffi.StateView()
        for k in _ffi.STATE_FIELDS:
            setattr(v, k, None if k in null else C.addressof(bufs[k]))
        return v

    v = view()
    mask = (C.c_uint32 * 32)()
    ret = (C.c_float * 4)()
    cnt = (C.c_int32 * 4)()
    ws = (C.c_uint8 * 4096)()

    def call(vw=v, steps=3, r=C.addressof(ret), m=C.addressof(mask), words=5, a=C.addressof(cnt), w=C.addressof(ws)):
        return lib.w2a_hindsight_optimum(None, None if vw is None else C.byref(vw), steps, r, m, words, a, w, 4096, None)

    assert call() == ERR_ARG and b"NULL handle" in lib.w2a_last_error()
    for kw in ({"vw": None}, {"r": None}, {"m": None}, {"a": None}, {"w": None}):
        assert call(**kw) == ERR_ARG and b"NULL argument" in lib.w2a_last_error(), kw
    for k in ("t", "used", "streak", "budget", "n_days", "county_w", "year_i", "coef_col", "sample", "finished"):
        assert call(vw=view(**{k: 1})) == ERR_ARG and b"NULL start-state array" in lib.w2a_last_error(), k
    for k in ("hist14", "last_actual", "at_budget", "sticky_budget", "episode_no", "episode_return"):
        assert call(vw=view(**{k: 1})) == ERR_ARG and b"NULL handle" in lib.w2a_last_error(), k  # not read
    assert call(steps=0) == ERR_ARG and b"n_steps must be positive" in lib.w2a_last_error()
    assert call(steps=-2) == ERR_ARG and b"n_steps must be positive" in lib.w2a_last_error()
    assert call(words=0) == ERR_ARG and b"mask_words must be positive" in lib.w2a_last_error()
    assert lib.w2a_hindsight_workspace_bytes(None, 10, 5, 1) == 0
