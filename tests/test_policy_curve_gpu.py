"""policy_budget_curve() (k_policy_curve_linear) on the GPU. Every assertion is bit equality with rollout(linear) of the
twin env whose budget is used + b -- from reset, mid-episode (the env's own column), under a gate, across the kernel's
budget chunks, over a truncated call -- except against the CPU twin (tests/policy_curve_restatement.py), which is held
to the bars tests/test_linear_policy_gpu.py holds k_rollout_linear to against the oracle's loop.
Tables: the mini and mini64 goldens (T = 153, uniform) and the ragged table of tests/table_edges.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from weather2alert_amd import _ffi, env as envmod, policy as P, tables

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402
from policy_curve_restatement import policy_curve_fp64  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RETURN_RTOL, RETURN_ATOL = 2e-6, 2e-5  # as tests/test_linear_policy_gpu.py (and tests/test_env_gpu.py)
TIE_SHARE = 0.01                       # near-tie decisions excepted there: fewer than 1 %
CHUNK = 64                             # budgets one workgroup of k_policy_curve_linear serves at most
B = 8
G = 3
SEED = 11
KEYS = ("return", "alerts", "attempts_over_budget", "alert_days")


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


def _env(dev, tabs, table, n, days=0, p=0.3, seed=SEED, options=None, twin=False):
    """a fresh env, stepped `days` days with Bernoulli(p) attempts (none on finished envs). twin: an env whose later
    reset(seed, options={"budget": b}) takes b (fixes={"budget"}: without it the first reset's budget is sticky, quirk
    Q9, and a second reset keeps it); the same episodes, the same kernels"""
    from weather2alert_amd import HeatAlertVecEnv

    ct, kw = tabs[table]
    kw = dict(kw, fixes={"budget"}) if twin else kw
    env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", env_gid0=E.GID0, **kw)
    env.reset(seed=seed, options=options)
    acts = torch.as_tensor((np.random.default_rng(seed).random((days, n)) < p).astype(np.int32), device=dev)
    for d in range(days):
        env.step(acts[d] * (env.state()["finished"] == 0).to(torch.int32))
    return env


def _policy(ct, n, sample=False, require_budget=False, seed=3, **kw):
    """G rows, eager enough to run out of alerts, with a weight on remaining_budget: columns differ from day 0 on"""
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((G, ct.n_obs)) * 0.4).astype(np.float32)
    W[:, ct.feature_names.index("remaining_budget")] = np.float32(0.15)
    b = (rng.standard_normal(G) * 0.5 + 0.5).astype(np.float32)
    g = (np.arange(n) * 3 + np.arange(n) // 7) % G
    return dict(kind="linear", weight=W, bias=b, group=g, sample=sample, seed=5, require_budget=require_budget, **kw)


def _clone(st):
    return {k: v.clone() for k, v in st.items()}


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _twin_columns(twin, pol, cv, budgets, n_steps=None, seed=SEED):
    """columns `budgets` of a curve taken right after reset(seed) against rollout() of the twins reset(seed, budget=b)"""
    for b in budgets:
        twin.reset(seed=seed, options={"budget": int(b)})
        ro = twin.rollout(pol, n_steps=n_steps, alert_mask=True)
        for k in KEYS:
            assert torch.equal(_bits(cv[k][:, b].contiguous()), _bits(ro[k])), (b, k)


def _shapes(cv, n, nb, T):
    assert cv["return"].shape == cv["alerts"].shape == cv["attempts_over_budget"].shape == (n, nb + 1)
    assert cv["return"].dtype == torch.float32
    assert cv["alerts"].dtype == cv["attempts_over_budget"].dtype == cv["own_budget"].dtype == torch.int32
    assert cv["alert_days"].shape == (n, nb + 1, T) and cv["alert_days"].dtype == torch.bool
    assert torch.equal(cv["alert_days"].sum(-1).to(torch.int32), cv["alerts"])
    assert (cv["alerts"] <= torch.arange(nb + 1, device=cv["alerts"].device)[None, :]).all()


@pytest.mark.parametrize("require_budget", [False, True])
@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("table", ["mini", "mini64"])
def test_twins_from_reset(dev, tabs, table, sample, require_budget):
    n = 192
    env, twin = _env(dev, tabs, table, n), _env(dev, tabs, table, n, twin=True)
    ct = tabs[table][0]
    pol = _policy(ct, n, sample, require_budget)
    st0 = _clone(env.state())
    assert (st0["used"] == 0).all() and (st0["t"] == 0).all()
    cv = env.policy_budget_curve(pol, B, schedules=True)
    _shapes(cv, n, B, ct.T)
    assert torch.equal(cv["own_budget"], st0["budget"])
    _twin_columns(twin, pol, cv, range(B + 1))
    assert not cv["alert_days"][:, 0].any() and int(cv["alerts"][:, B].max()) == B
    sched = cv["alert_days"]
    assert bool((sched[:, 1:] != sched[:, :-1]).any(-1).all(-1).any())  # some env: neighbouring columns all differ
    if require_budget:
        assert not cv["attempts_over_budget"].any()
    else:
        assert bool((cv["attempts_over_budget"] > 0).any())
    # the env's own column is its own rollout, and the curve left the env as it was
    ro = env.rollout(pol, alert_mask=True)
    own = cv["own_budget"].long()
    inside = own <= B
    assert bool(inside.any())
    for k in KEYS:
        col = cv[k].gather(1, own.clamp(max=B).view(n, 1, *([1] * (cv[k].dim() - 2))).expand(n, 1, *cv[k].shape[2:]))[:, 0]
        assert torch.equal(_bits(col[inside]), _bits(ro[k][inside])), k
    assert env.check_status() == 0
    env.close()
    twin.close()


@pytest.mark.parametrize("sample", [False, True])
def test_own_column_mid_episode(dev, tabs, sample):
    """20 days of Bernoulli(0.3) attempts at the ragged table's default budgets: envs mid-streak with alerts used, envs
    whose budget is spent, envs whose episode is over. The env's own column is its own rollout; every column is the
    CPU twin's; the call leaves the env as it found it."""
    n = 256
    env = _env(dev, tabs, "ragged", n, days=20)
    ct = tabs["ragged"][0]
    pol = _policy(ct, n, sample)
    st0 = _clone(env.state())
    live = st0["finished"] == 0
    assert bool((live & (st0["streak"] > 0) & (st0["used"] > 0) & (st0["used"] < st0["budget"])).any())
    assert bool((live & (st0["used"] == st0["budget"])).any()) and bool((~live).any()) and bool(live.any())
    before, obs_before, status_before = env.state_dict(), env._obs.clone(), env.status_word.clone()
    cv = env.policy_budget_curve(pol, B, schedules=True)
    _shapes(cv, n, B, ct.T)
    after = env.state_dict()
    for k in ("state", "obs", "final_return", "reward", "done"):
        assert torch.equal(before[k], after[k]), k
    # (the status word holds the setup's steps of finished envs; the call leaves it as it was)
    assert before["host"] == after["host"] and torch.equal(obs_before, env._obs)
    assert torch.equal(status_before, env.status_word)
    for k, x in env.state().items():
        assert torch.equal(x, st0[k]), k
    assert torch.equal(cv["own_budget"], st0["budget"] - st0["used"])
    assert (cv["return"][~live] == 0).all() and (cv["alerts"][~live] == 0).all() and not cv["alert_days"][~live].any()
    assert not cv["alert_days"][:, :, :20][live].any()  # nothing before the start day
    # a state() dict equal to the current state is the env's own state
    again = env.policy_budget_curve(pol, B, start_state=st0, schedules=True)
    for k in cv:
        assert torch.equal(_bits(cv[k]), _bits(again[k])), k
    # ---- the CPU twin, all columns
    V = E.make_tables()["ragged"].oracle()
    st = {k: v.cpu().numpy().astype(np.int64) for k, v in st0.items() if k != "episode_return"}
    ref = policy_curve_fp64(V, ct, st, obs_before.cpu().numpy(), pol["weight"], pol["bias"], pol["group"], ct.T, B,
                            sample=sample, seed=pol["seed"], gid0=E.GID0)
    tie = ref["tie"]
    print(f"sample={sample}: near-tie (env, budget) pairs {int(tie.sum())} of {tie.size}")
    assert tie.mean() < TIE_SHARE
    ok = ~tie
    got = {k: cv[k].cpu().numpy() for k in KEYS}
    err = np.abs(got["return"].astype(np.float64) - ref["return"])
    bar = RETURN_ATOL + RETURN_RTOL * np.abs(ref["return"])
    print(f"  largest return error / bar {float((err / bar)[ok].max()):.4f}")
    np.testing.assert_array_equal(got["alerts"][ok], ref["alerts"][ok])
    np.testing.assert_array_equal(got["attempts_over_budget"][ok], ref["attempts_over_budget"][ok])
    np.testing.assert_array_equal(got["alert_days"][ok], ref["alert_days"][ok])
    assert (err <= bar)[ok].all()
    assert ref["alerts"][ok].sum() > 0 and (ref["attempts_over_budget"][ok] > 0).any()
    # ---- the env's own column: the rollout of the env as it is
    ro = env.rollout(pol, alert_mask=True)
    own = cv["own_budget"].long()
    inside = (own <= B) & (own >= 0)
    assert bool((inside & live).any())
    for k in ("return", "alerts", "attempts_over_budget"):
        col = cv[k].gather(1, own.clamp(0, B)[:, None])[:, 0]
        assert torch.equal(_bits(col[inside]), _bits(ro[k][inside])), k
    col = cv["alert_days"].gather(1, own.clamp(0, B)[:, None, None].expand(n, 1, ct.T))[:, 0]
    assert torch.equal(col[inside], ro["alert_days"][inside])
    env.close()


def test_gate(dev, tabs):
    n = 128
    env, twin = _env(dev, tabs, "mini", n), _env(dev, tabs, "mini", n, twin=True)
    ct = tabs["mini"][0]
    gate = q = None
    for q in (0.8, 0.9, 0.95, 0.98):
        g = env.alert_gate("heat_qi", q)
        days = g.sum(1)
        if bool((days < B).any()) and bool((days > 0).any()):
            gate = g
            break
    assert gate is not None, "no threshold leaves some envs fewer open days than B"
    for sample in (False, True):
        pol = _policy(ct, n, sample, allowed_days=gate)
        cv = env.policy_budget_curve(pol, B, schedules=True)
        _shapes(cv, n, B, ct.T)
        _twin_columns(twin, pol, cv, range(B + 1))
        assert not (cv["alert_days"] & ~gate[:, None, :]).any() and int(cv["alerts"].max()) > 0
        free = env.policy_budget_curve(_policy(ct, n, sample), B, schedules=True)
        assert bool((free["alert_days"] != cv["alert_days"]).any())
        # the packed words of the gate and of the schedules
        pk = env.policy_budget_curve(_policy(ct, n, sample, allowed_days=env.alert_gate("heat_qi", q, packed=True)), B,
                                     schedules=True, packed=True)
        assert pk["alert_days"].dtype == torch.int32 and pk["alert_days"].shape == (n, B + 1, (ct.T + 31) // 32)
        for k in ("return", "alerts", "attempts_over_budget"):
            assert torch.equal(_bits(pk[k]), _bits(cv[k])), k
        assert torch.equal(P.unpack_alert_days(pk["alert_days"].view(n * (B + 1), -1), ct.T).view(n, B + 1, -1),
                           cv["alert_days"])
    env.close()
    twin.close()


def _c_args(env, pol, st, nb, ret, cnt, over, masks, obs=True):
    """the arguments of w2a_policy_curve_linear on the env's handle (and what they point to)"""
    lin = envmod._check_learned(env, pol)
    lp = _ffi.LinearPolicy()
    lp.weight, lp.bias = lin.weight_slots.data_ptr(), lin.bias.data_ptr()
    lp.group = None if lin.group is None else lin.group.data_ptr()
    lp.n_groups, lp.sample, lp.require_budget, lp.seed = lin.n_groups, int(lin.sample), int(lin.require_budget), lin.seed
    v = _ffi.StateView()
    for k in _ffi.STATE_FIELDS:
        setattr(v, k, st[k].data_ptr())
    words = (env.ct.T + 31) // 32
    return [env._h, C.byref(lp), C.byref(v), env.ct.T, nb, env._obs.data_ptr() if obs else None, ret.data_ptr(),
            cnt.data_ptr(), over.data_ptr(), None if masks is None else masks.data_ptr(), words], (lin, lp, v)


def test_partial_wave_and_poisoned_outputs(dev, tabs):
    """N = 70: a partial last workgroup at every chunking. Outputs allocated for 6 more envs and poisoned: nothing is
    written past row N - 1."""
    n, extra = 70, 6
    env = _env(dev, tabs, "mini", n)
    ct = tabs["mini"][0]
    words = (ct.T + 31) // 32
    st = _clone(env.state())
    pol = _policy(ct, n, True)
    ws = torch.empty(256, dtype=torch.uint8, device=dev)
    for nb in (0, 3, B, 20, CHUNK):
        want = env.policy_budget_curve(pol, nb, schedules=True, packed=True)
        ret = torch.full((n + extra, nb + 1), 5.0, dtype=torch.float32, device=dev)
        cnt = torch.full((n + extra, nb + 1), 9, dtype=torch.int32, device=dev)
        over = torch.full((n + extra, nb + 1), 8, dtype=torch.int32, device=dev)
        masks = torch.full((n + extra, nb + 1, words), 7, dtype=torch.int32, device=dev)
        args, keep = _c_args(env, pol, st, nb, ret, cnt, over, masks)
        assert env._lib.w2a_policy_curve_linear(*args, ws.data_ptr(), 256, None) == 0, env._lib.w2a_last_error()
        torch.cuda.synchronize()
        assert (ret[n:] == 5.0).all() and (cnt[n:] == 9).all() and (over[n:] == 8).all() and (masks[n:] == 7).all(), nb
        assert torch.equal(_bits(ret[:n]), _bits(want["return"])) and torch.equal(cnt[:n], want["alerts"])
        assert torch.equal(over[:n], want["attempts_over_budget"]) and torch.equal(masks[:n], want["alert_days"])
    env.close()


def test_max_budget_zero_determinism_and_packed(dev, tabs):
    n = 100
    env, twin = _env(dev, tabs, "mini", n), _env(dev, tabs, "mini", n, twin=True)
    ct = tabs["mini"][0]
    pol = _policy(ct, n, True)
    z = env.policy_budget_curve(pol, 0, schedules=True)
    _shapes(z, n, 0, ct.T)
    assert not z["alert_days"].any() and not z["alerts"].any()
    _twin_columns(twin, pol, z, (0,))
    a = env.policy_budget_curve(pol, B, schedules=True)
    b = env.policy_budget_curve(pol, B, schedules=True)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert torch.equal(_bits(z["return"][:, 0]), _bits(a["return"][:, 0]))
    c = env.policy_budget_curve(pol, B)
    assert set(c) == {"return", "alerts", "attempts_over_budget", "own_budget"}
    for k in c:
        assert torch.equal(_bits(c[k]), _bits(a[k])), k
    pk = env.policy_budget_curve(pol, B, schedules=True, packed=True)
    words = (ct.T + 31) // 32
    assert pk["alert_days"].dtype == torch.int32 and pk["alert_days"].shape == (n, B + 1, words)
    assert torch.equal(pk["alert_days"].view(n * (B + 1), words),
                       P.pack_alert_days(a["alert_days"].view(n * (B + 1), ct.T), words))
    env.close()
    twin.close()


@pytest.mark.parametrize("nb", [CHUNK - 1, CHUNK, 2 * CHUNK + 1])
def test_both_sides_of_the_budget_chunk(dev, tabs, nb):
    """max_budget 63: one workgroup of 64 budgets per env; 64: 65 budgets in two chunks of 33; 129: 130 budgets in three
    chunks of 44. Columns around 64 and around the chunks' own borders against the twins."""
    n = 10
    env, twin = _env(dev, tabs, "mini", n), _env(dev, tabs, "mini", n, twin=True)
    ct = tabs["mini"][0]
    pol = _policy(ct, n, True)
    pol["bias"] = pol["bias"] + np.float32(1.5)  # eager: large budgets get used
    cv = env.policy_budget_curve(pol, nb, schedules=True)
    _shapes(cv, n, nb, ct.T)
    chunks = (nb + 1 + CHUNK - 1) // CHUNK
    per = (nb + 1 + chunks - 1) // chunks
    cols = {0, 1, CHUNK - 1, CHUNK, CHUNK + 1, nb}
    for c in range(1, chunks):
        cols |= {c * per - 1, c * per}
    _twin_columns(twin, pol, cv, sorted(c for c in cols if c <= nb))
    assert int(cv["alerts"][:, nb].max()) > 20
    env.close()
    twin.close()


def test_truncated_call_and_the_rest_add_up(dev, tabs):
    """n_steps = 5 is the twins' first five days bit for bit; the rest of the episode from a twin's state after them (its
    own column) adds up to the whole-episode column within the suite's bar for sums of f32 returns."""
    n = 96
    env, twin = _env(dev, tabs, "mini", n), _env(dev, tabs, "mini", n, twin=True)
    ct = tabs["mini"][0]
    pol = _policy(ct, n, True)
    cut = env.policy_budget_curve(pol, B, n_steps=5, schedules=True)
    whole = env.policy_budget_curve(pol, B, schedules=True)
    assert not cut["alert_days"][:, :, 5:].any() and torch.equal(cut["alert_days"][:, :, :5], whole["alert_days"][:, :, :5])
    for b in (0, 3, B):
        twin.reset(seed=SEED, options={"budget": b})
        ro = twin.rollout(pol, n_steps=5, alert_mask=True)
        for k in KEYS:
            assert torch.equal(_bits(cut[k][:, b].contiguous()), _bits(ro[k])), (b, k)
        rest = twin.policy_budget_curve(pol, B)
        own = rest["own_budget"].long()
        assert torch.equal(own, b - ro["alerts"].long())
        tail = rest["return"].gather(1, own[:, None])[:, 0]
        torch.testing.assert_close(cut["return"][:, b] + tail, whole["return"][:, b], rtol=RETURN_RTOL, atol=RETURN_ATOL)
        assert torch.equal(cut["alerts"][:, b] + rest["alerts"].gather(1, own[:, None])[:, 0], whole["alerts"][:, b])
    env.close()
    twin.close()


def test_foreign_start_states(dev, tabs):
    """a start that is not the env's current state: taken from reset (the held rows are rebuilt from day 0's table row),
    refused mid-episode"""
    n = 80
    env = _env(dev, tabs, "ragged", n)
    ct = tabs["ragged"][0]
    pol = _policy(ct, n, True)
    st0 = _clone(env.state())
    want = env.policy_budget_curve(pol, B, schedules=True)
    for d in range(3):
        env.step(torch.ones(n, dtype=torch.int32, device=dev))
    st3, obs3 = _clone(env.state()), env._obs.clone()
    got = env.policy_budget_curve(pol, B, start_state=st0, schedules=True)
    for k in want:
        assert torch.equal(_bits(want[k]), _bits(got[k])), k
    mid = _clone(st3)
    mid["budget"] = mid["budget"] + 1  # not the current state, and not at day 0
    with pytest.raises(ValueError, match="not the env's current state"):
        env.policy_budget_curve(pol, B, start_state=mid)
    assert torch.equal(obs3, env._obs)
    for k, x in env.state().items():
        assert torch.equal(x, st3[k]), k
    # a start outside the tables: a row of NaN, zero counts, nothing read
    bad = _clone(st0)
    bad["coef_col"][:3] = ct.S + 2
    bad["finished"][3:5] = 1
    out = env.policy_budget_curve(pol, B, start_state=bad, schedules=True)
    assert torch.isnan(out["return"][:3]).all() and (out["return"][3:5] == 0).all() and torch.isfinite(out["return"][5:]).all()
    assert (out["alerts"][:5] == 0).all() and not out["alert_days"][:5].any()
    for k in KEYS:
        assert torch.equal(_bits(out[k][5:]), _bits(want[k][5:])), k
    env.close()


def test_c_level_refusals_come_before_any_output(dev, tabs):
    from weather2alert_amd import HeatAlertVecEnv

    ct = tabs["mini"][0]
    n, words = 64, (ct.T + 31) // 32
    ret = torch.full((n, B + 1), 5.0, dtype=torch.float32, device=dev)
    cnt = torch.full((n, B + 1), 9, dtype=torch.int32, device=dev)
    over = torch.full((n, B + 1), 8, dtype=torch.int32, device=dev)
    # poison -1: a word of 32 alert days, which no schedule of at most B alerts holds (7 is days 0, 1 and 2)
    masks = torch.full((n, B + 1, words), -1, dtype=torch.int32, device=dev)
    ws = torch.empty(512, dtype=torch.uint8, device=dev)

    def call(e, name="w2a_policy_curve_linear", handle=True, nbytes=256, w=words, budget=B, ws_ptr=None, gated=()):
        st = e.state()
        args, keep = _c_args(e, _policy(ct, n), st, budget, ret, cnt, over, masks)
        args[10] = w
        if not handle:
            args[0] = None
        rc = getattr(e._lib, name)(*args, ws.data_ptr() if ws_ptr is None else ws_ptr, nbytes, None, *gated)
        torch.cuda.synchronize()
        return rc, e._lib.w2a_last_error()

    def untouched():
        return bool((ret == 5.0).all()) and bool((cnt == 9).all()) and bool((over == 8).all()) and bool((masks == -1).all())

    fx = HeatAlertVecEnv(n, tables=ct, device=dev, fixes={"lag"})
    fx.reset(seed=1)
    with pytest.raises(ValueError, match="faithful"):
        fx.policy_budget_curve(_policy(ct, n), B)
    rc, msg = call(fx)
    assert rc == -1 and msg.startswith(b"w2a_policy_curve_linear: ") and b"corrected-semantics" in msg and untouched()
    fx.close()
    ok = HeatAlertVecEnv(n, tables=ct, device=dev, fixes={"budget"}, autoreset="disabled")
    ok.reset(seed=1)
    g = "w2a_policy_curve_linear_gated"
    for kw, text in ((dict(handle=False), b"w2a_policy_curve_linear: NULL handle"),
                     (dict(nbytes=255), b"workspace smaller than w2a_policy_curve_workspace_bytes(env, n_steps, max_budget)"),
                     (dict(nbytes=0), b"workspace smaller than"),
                     (dict(ws_ptr=ws.data_ptr() + 64), b"workspace must be 256-B aligned"),
                     (dict(w=words - 1), b"alert_masks needs ceil(T/32) words per env and budget"),
                     (dict(w=0), b"mask_words must be positive"),
                     (dict(budget=-1), b"max_budget must lie in 0..1023"),
                     (dict(budget=1024), b"max_budget must lie in 0..1023"),
                     (dict(name=g, handle=False, gated=(masks.data_ptr(), words)), b"w2a_policy_curve_linear_gated: NULL handle"),
                     (dict(name=g, gated=(None, words)), b"NULL allowed_days"),
                     (dict(name=g, gated=(masks.data_ptr(), words - 1)), b"allowed_days needs ceil(T/32)"),
                     (dict(name=g, nbytes=128, gated=(masks.data_ptr(), words)), b"workspace smaller than")):
        rc, msg = call(ok, **kw)
        assert rc == -1 and text in msg and untouched(), (kw, msg)
    assert ok._lib.w2a_policy_curve_workspace_bytes(ok._h, ct.T, B) == 256
    assert ok._lib.w2a_policy_curve_workspace_bytes(ok._h, 0, B) == 0
    assert ok._lib.w2a_policy_curve_workspace_bytes(ok._h, ct.T, 1024) == 0
    st = _clone(ok.state())
    with pytest.raises(_ffi.W2AError, match="recording a hipGraph"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            ok.policy_budget_curve(_policy(ct, n), B, start_state=st)
    with pytest.raises(ValueError, match="shape"):
        ok.policy_budget_curve(_policy(ct, n), B, {k: x[:63] for k, x in st.items()})
    with pytest.raises(KeyError, match="hist14"):
        ok.policy_budget_curve(_policy(ct, n), B, {k: x for k, x in st.items() if k != "hist14"})
    ok.rollout(dict(kind="always"), n_steps=5)  # a built-in rollout writes no observation rows
    with pytest.raises(RuntimeError, match="observation buffer"):
        ok.policy_budget_curve(_policy(ct, n), B)
    ok.reset(seed=1)
    assert untouched()
    rc, _ = call(ok)
    assert rc == 0 and torch.isfinite(ret).all() and not bool((ret == 5.0).any()) and not bool((masks == -1).any())
    assert ok.check_status() == 0
    ok.close()
