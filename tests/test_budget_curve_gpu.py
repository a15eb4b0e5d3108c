"""hindsight_budget_curve() (k_hs_curve) on the GPU. Exact properties first: every column b is, bit for bit,
hindsight_optimum() of the twin whose budget is used + b -- from reset and mid-episode (running streaks, spent budgets,
finished envs), past 64 budgets on the workspace path, under a gate, over a truncated horizon -- then the fp64
restatement (tests/budget_curve_restatement.py), the edges and the C entry's refusals.
Tables: the mini and mini64 goldens (T = 153, uniform) and the ragged table of tests/table_edges.py, whose shortest
episodes end inside a 25-day prefix."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from weather2alert_amd import _ffi, tables

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402
from budget_curve_restatement import budget_curve_fp64  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DAY_BAR = 1e-5  # the bar tests/test_hindsight_gpu.py holds k_hs_dp to against the fp64 DP: H days of it on a return
KEYS = ("t", "used", "streak", "hist14", "budget", "n_days", "county_w", "year_i", "coef_col", "sample", "finished")
B = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tabs():
    """name -> (compiled tables, env keywords)"""
    out = {d: (tables.CompiledTables.load_npz(os.path.join(GOLDEN, f"{d}_compiled.npz")), {}) for d in ("mini", "mini64")}
    out["ragged"] = (E.make_tables()["ragged"].ct, dict(similar_climate_counties=True))
    return out


def _env(dev, tabs, table, n, days=0, p=0.3, seed=11, options=None):
    """a fresh env, stepped `days` days with Bernoulli(p) attempts (none on finished envs)"""
    from weather2alert_amd import HeatAlertVecEnv

    ct, kw = tabs[table]
    env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", env_gid0=E.GID0, **kw)
    env.reset(seed=seed, options=options)
    acts = torch.as_tensor((np.random.default_rng(seed).random((days, n)) < p).astype(np.int32), device=dev)
    for d in range(days):
        env.step(acts[d] * (env.state()["finished"] == 0).to(torch.int32))
    return env


def _clone(st):
    return {k: v.clone() for k, v in st.items()}


def _bits(x):
    return x.view(torch.int32) if x.is_floating_point() else x


def _check_twins(env, st0, max_budget, budgets, n_steps=None, gate=None):
    """columns `budgets` of the curve against hindsight_optimum() of the twins; returns the curve"""
    cv = env.hindsight_budget_curve(max_budget, start_state=st0, n_steps=n_steps, allowed_days=gate, schedules=True)
    n, T = env.num_envs, env.ct.T
    assert cv["return"].shape == cv["alerts"].shape == (n, max_budget + 1) and cv["return"].dtype == torch.float32
    assert cv["alert_days"].shape == (n, max_budget + 1, T) and cv["alert_days"].dtype == torch.bool
    assert cv["alerts"].dtype == cv["own_budget"].dtype == torch.int32
    assert torch.equal(cv["own_budget"], st0["budget"] - st0["used"])
    for b in budgets:
        tw = _clone(st0)
        tw["budget"] = tw["used"] + b
        hs = env.hindsight_optimum(tw, n_steps=n_steps, allowed_days=gate)
        assert torch.equal(_bits(cv["return"][:, b].contiguous()), _bits(hs["return"])), b
        assert torch.equal(cv["alerts"][:, b], hs["alerts"]), b
        assert torch.equal(cv["alert_days"][:, b], hs["alert_days"]), b
    assert torch.equal(cv["alert_days"].sum(-1).to(torch.int32), cv["alerts"])
    return cv


@pytest.mark.parametrize("table", ["mini", "mini64"])
def test_bit_identity_with_the_twins_from_reset(dev, tabs, table):
    env = _env(dev, tabs, table, 192)
    st0 = _clone(env.state())
    assert (st0["streak"] == 0).all() and (st0["used"] == 0).all() and (st0["t"] == 0).all()
    cv = _check_twins(env, st0, B, range(B + 1))
    assert int(cv["alerts"][:, B].max()) == B and not cv["alert_days"][:, 0].any()
    # the env's own column is hindsight_optimum() of the env as it is
    own = cv["own_budget"].long()
    inside = own <= B
    assert bool(inside.any())
    hs = env.hindsight_optimum(st0)
    mine = cv["return"].gather(1, own.clamp(max=B)[:, None])[:, 0]
    assert torch.equal(_bits(mine[inside]), _bits(hs["return"][inside]))
    assert env.check_status() == 0
    env.close()


def test_bit_identity_with_the_twins_mid_episode(dev, tabs):
    """20 days of Bernoulli(0.3) attempts at the ragged table's default budgets: envs mid-streak with alerts used, envs
    whose budget is spent, envs whose episode is over"""
    env = _env(dev, tabs, "ragged", 256, days=20)
    st0 = _clone(env.state())
    live = st0["finished"] == 0
    assert bool((live & (st0["streak"] > 0) & (st0["used"] > 0) & (st0["used"] < st0["budget"])).any())
    assert bool((live & (st0["used"] == st0["budget"])).any()) and bool((~live).any()) and bool(live.any())
    assert bool((live & (st0["streak"] == 0) & (st0["used"] > 0)).any())
    cv = _check_twins(env, st0, B, range(B + 1))
    assert (cv["return"][~live] == 0).all() and (cv["alerts"][~live] == 0).all()
    assert int(cv["alerts"][live].max()) > 2
    env.close()


def test_both_sides_of_64_budgets_on_the_workspace_path(dev, tabs):
    """max_budget = 70: budget chunks of 64 + 7 lanes, 72 x 71 states in 80 chunks per day, beyond LDS"""
    env = _env(dev, tabs, "mini", 8)
    ct = tabs["mini"][0]
    lib = env._lib
    assert lib.w2a_hindsight_curve_workspace_bytes(env._h, ct.T, 40, 1) == 256  # 40 still fits in LDS at T = 153
    assert lib.w2a_hindsight_curve_workspace_bytes(env._h, ct.T, 41, 1) > 256
    per_env = 16 * 71 * 72 + 8 * ct.T * ((71 * 72 + 63) // 64)
    assert 32 * ct.T + per_env > 64 * 1024
    assert lib.w2a_hindsight_curve_workspace_bytes(env._h, ct.T, 70, 3) == 256 + 3 * ((per_env + 255) // 256 * 256)
    st0 = _clone(env.state())
    cv = _check_twins(env, st0, 70, (0, 1, 63, 64, 65, 70))
    assert int(cv["alerts"][:, 70].max()) > 14
    # a pool of one env: eight launches in turn give the same bits
    words = (ct.T + 31) // 32
    ret = torch.empty((8, 71), dtype=torch.float32, device=dev)
    cnt = torch.empty((8, 71), dtype=torch.int32, device=dev)
    one = lib.w2a_hindsight_curve_workspace_bytes(env._h, ct.T, 70, 1)
    ws = torch.empty(one, dtype=torch.uint8, device=dev)
    v = _ffi.StateView()
    for k in _ffi.STATE_FIELDS:
        setattr(v, k, st0[k].data_ptr())
    assert lib.w2a_hindsight_curve(env._h, C.byref(v), ct.T, 70, ret.data_ptr(), cnt.data_ptr(), None, words,
                                   ws.data_ptr(), one, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(ret), _bits(cv["return"])) and torch.equal(cnt, cv["alerts"])
    env.close()


def test_gate(dev, tabs):
    env = _env(dev, tabs, "mini", 128)
    st0 = _clone(env.state())
    gate = None
    for q in (0.8, 0.9, 0.95, 0.98):
        g = env.alert_gate("heat_qi", q)
        days = g.sum(1)
        if bool((days < B).any()) and bool((days > 0).any()):
            gate = g
            break
    assert gate is not None, "no threshold leaves some envs fewer open days than B"
    cv = _check_twins(env, st0, B, range(B + 1), gate=gate)
    open_days = gate.sum(1).to(torch.int32)
    assert (cv["alerts"] <= open_days[:, None]).all() and not (cv["alert_days"] & ~gate[:, None, :]).any()
    assert bool((cv["alerts"][:, B] < B).any()) and int(cv["alerts"].max()) > 0
    # the packed words of the gate and of the schedules
    pk = env.hindsight_budget_curve(B, start_state=st0, allowed_days=env.alert_gate("heat_qi", q, packed=True),
                                    schedules=True, packed=True)
    assert pk["alert_days"].dtype == torch.int32 and pk["alert_days"].shape == (128, B + 1, (env.ct.T + 31) // 32)
    assert torch.equal(_bits(pk["return"]), _bits(cv["return"]))
    from weather2alert_amd import policy as P
    assert torch.equal(P.unpack_alert_days(pk["alert_days"].view(128 * (B + 1), -1), env.ct.T).view(128, B + 1, -1),
                       cv["alert_days"])
    env.close()


def test_truncated_horizon(dev, tabs):
    env = _env(dev, tabs, "mini", 96, days=10)
    st0 = _clone(env.state())
    assert (st0["t"] == 10).all()
    cv = _check_twins(env, st0, B, range(B + 1), n_steps=30)
    assert not cv["alert_days"][:, :, :10].any() and not cv["alert_days"][:, :, 40:].any()
    assert int(cv["alerts"].max()) > 0
    env.close()


@pytest.mark.parametrize("table,days", [("mini", 0), ("mini64", 25)])
def test_against_the_restatement(dev, tabs, table, days):
    """Returns within H_e DAY_BAR of the fp64 restatement's values, over the whole episode and over 30 days. Schedules
    over 30 days: equal wherever no decision on the restatement's path has |q1 - q0| inside that bar. Such (env, budget)
    pairs may be at most 1 % -- asserted here of the restatement alone, on these inputs, before the kernel's schedules
    are read (over the whole episode the restatement's own share is about 3 % on these tables, so schedules are compared
    on the 30-day stretch, where it is 0.1 .. 0.4 %)."""
    n = 64
    env = _env(dev, tabs, table, n, days=days)
    ct = tabs[table][0]
    st0 = _clone(env.state())
    st = {k: st0[k].cpu().numpy().astype(np.int64)[::2] for k in KEYS}  # the kernel runs 64 envs, every 2nd is restated
    for steps in (30, None):
        cv = env.hindsight_budget_curve(B, start_state=st0, n_steps=steps, schedules=True)
        ref = budget_curve_fp64(ct.X, ct.W, ct.n_samples, len(ct.years), st, steps or ct.T, B)
        bar = ref["H"][:, None] * DAY_BAR
        err = np.abs(cv["return"].double().cpu().numpy()[::2] - ref["value"])
        print(f"{table} from day {days}, n_steps {steps}: largest error / bar {float((err / bar).max()):.4f}")
        assert (err <= bar).all(), float((err - bar).max())
        if steps is None:
            continue
        close = ref["margin"] < bar
        print(f"  pairs with a decision inside the bar: {int(close.sum())} of {close.size}")
        assert close.mean() <= 0.01
        same = (cv["alert_days"].cpu().numpy()[::2] == ref["alert_days"]).all(-1)
        assert (same | close).all()
        assert (cv["alerts"].cpu().numpy()[::2] == ref["alerts"])[~close].all()
    env.close()


def test_edges(dev, tabs):
    """a start outside the tables, finished envs, column 0, determinism, no side effects"""
    env = _env(dev, tabs, "mini", 100, days=5)
    ct = tabs["mini"][0]
    before, obs_before = env.state_dict(), env._obs.clone()
    st_before = _clone(env.state())
    st = _clone(env.state())
    st["coef_col"][:5] = ct.S + 3
    st["sample"][5] = ct.n_samples
    st["finished"][6:9] = 1
    st["t"][9] = st["n_days"][9]
    a = env.hindsight_budget_curve(B, start_state=st, schedules=True)
    b = env.hindsight_budget_curve(B, start_state=st, schedules=True)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert torch.isnan(a["return"][:6]).all() and (a["return"][6:10] == 0).all() and torch.isfinite(a["return"][10:]).all()
    assert (a["alerts"][:10] == 0).all() and not a["alert_days"][:10].any()
    # column 0 is what the empty schedule pays the twin with no budget left (slot 26 reads 0 on every day)
    empty = torch.zeros((100, ct.T), dtype=torch.bool, device=dev)
    inside = {**st, "coef_col": st_before["coef_col"], "sample": st_before["sample"],  # (the curve's NaN rows aside)
              "budget": st["used"]}
    pr = env.posterior_returns(inside, empty).gather(1, inside["sample"].long()[:, None])[:, 0]
    assert torch.equal(_bits(a["return"][10:, 0].contiguous()), _bits(pr[10:]))
    never = env.hindsight_optimum({**st, "budget": st["used"]})["return"]
    assert torch.equal(_bits(a["return"][6:, 0].contiguous()), _bits(never[6:]))
    # without schedules: the same returns and counts; max_budget = 0: one column
    c = env.hindsight_budget_curve(B, start_state=st)
    assert set(c) == {"return", "alerts", "own_budget"}
    assert torch.equal(_bits(c["return"]), _bits(a["return"])) and torch.equal(c["alerts"], a["alerts"])
    z = env.hindsight_budget_curve(0, start_state=st, schedules=True)
    assert z["return"].shape == (100, 1) and torch.equal(_bits(z["return"][:, 0]), _bits(a["return"][:, 0]))
    assert not z["alert_days"].any()
    # the handle: state, observation buffer and bookkeeping untouched; the default start is the current state
    cur = env.hindsight_budget_curve(B)
    assert torch.equal(cur["own_budget"], st_before["budget"] - st_before["used"])
    after = env.state_dict()
    for k in ("state", "obs", "final_return", "reward", "done"):
        assert torch.equal(before[k], after[k]), k
    assert before["host"] == after["host"] and torch.equal(obs_before, env._obs) and env.check_status() == 0
    for k, x in env.state().items():
        assert torch.equal(x, st_before[k]), k
    env.close()


def test_refusals_come_before_any_output(dev, tabs):
    from weather2alert_amd import HeatAlertVecEnv

    ct = tabs["mini"][0]
    n, words = 64, (ct.T + 31) // 32
    ret = torch.full((n, B + 1), 5.0, dtype=torch.float32, device=dev)
    cnt = torch.full((n, B + 1), 9, dtype=torch.int32, device=dev)
    mask = torch.full((n, B + 1, words), 7, dtype=torch.int32, device=dev)
    v = _ffi.StateView()

    def call(e, steps=ct.T, budget=B, w=words, nbytes=None, gated=None):
        st = e.state()
        st["finished"][: n // 2] = 1  # envs without a DP: their rows must stay untouched too
        for k in _ffi.STATE_FIELDS:
            setattr(v, k, st[k].data_ptr())
        need = e._lib.w2a_hindsight_curve_workspace_bytes(e._h, steps, max(0, min(budget, 1023)), 1)
        nbytes = need if nbytes is None else nbytes
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        args = (e._h, C.byref(v), steps, budget, ret.data_ptr(), cnt.data_ptr(), mask.data_ptr(), w, ws.data_ptr(),
                nbytes, None)
        rc = e._lib.w2a_hindsight_curve(*args) if gated is None else e._lib.w2a_hindsight_curve_gated(*args, *gated)
        torch.cuda.synchronize()
        return rc, e._lib.w2a_last_error()

    def untouched():
        return bool((ret == 5.0).all()) and bool((cnt == 9).all()) and bool((mask == 7).all())

    env = HeatAlertVecEnv(n, tables=ct, device=dev, fixes={"lag"})
    env.reset(seed=1)
    with pytest.raises(ValueError, match="lag"):
        env.hindsight_budget_curve(B)
    rc, msg = call(env)
    assert rc == -1 and b"corrected-semantics" in msg and untouched()
    env.close()
    W27 = np.array(ct.W, np.float32).reshape(-1, 2, 32)
    W27[3, 0, 27] = 0.25
    bad = HeatAlertVecEnv(n, tables=tables.CompiledTables(**{**ct.__dict__, "W": W27.reshape(ct.W.shape)}), device=dev)
    bad.reset(seed=1)
    with pytest.raises(ValueError, match="slot-27"):
        bad.hindsight_budget_curve(B)
    rc, msg = call(bad)
    assert rc == -1 and b"slot-27" in msg and untouched()
    bad.close()
    ok = HeatAlertVecEnv(n, tables=ct, device=dev, fixes={"budget"})
    ok.reset(seed=1)
    for kw, text in ((dict(w=words - 1), b"ceil(T/32)"), (dict(w=0), b"mask_words must be positive"),
                     (dict(steps=0), b"n_steps must be positive"), (dict(budget=-1), b"max_budget must lie in 0..1023"),
                     (dict(budget=1024), b"max_budget must lie in 0..1023"), (dict(nbytes=128), b"workspace smaller"),
                     (dict(budget=70, nbytes=256), b"workspace smaller"),
                     (dict(gated=(None, words)), b"NULL allowed_days"),
                     (dict(gated=(mask.data_ptr(), words - 1)), b"allowed_days needs ceil(T/32)")):
        rc, msg = call(ok, **kw)
        assert rc == -1 and text in msg and untouched(), kw
    st = _clone(ok.state())
    with pytest.raises(_ffi.W2AError, match="recording a hipGraph"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            ok.hindsight_budget_curve(B, start_state=st)
    with pytest.raises(ValueError, match="shape"):
        ok.hindsight_budget_curve(B, {k: x[:63] for k, x in st.items()})
    with pytest.raises(KeyError, match="sample"):
        ok.hindsight_budget_curve(B, {k: x for k, x in st.items() if k != "sample"})
    with pytest.raises(ValueError, match="n_steps"):
        ok.hindsight_budget_curve(B, st, n_steps=0)
    rc, _ = call(ok)
    assert rc == 0 and (ret[: n // 2] == 0).all() and (cnt[: n // 2] == 0).all() and (mask[: n // 2] == 0).all()
    assert torch.isfinite(ret).all() and not bool((ret[n // 2:] == 5.0).any()) and ok.check_status() == 0
    ok.close()
