"""hindsight_posterior_values() (w2a_hindsight_posterior_along, k_hs_pm_along) on the GPU. The numerics contract of
include/w2a.h first, each item exactly (bit equality, NaNs as bits): along hindsight_posterior_optimum()'s own schedule,
one draw against hindsight_values(), any later start against a twin stepped through step(), attempts, independence of
`sample`, determinism and sharing; then the fp64 restatement (tests/hindsight_posterior_values_restatement.py), the
regret against hindsight_posterior_optimum() less the draw-mean of posterior_returns(), a reward_mode="posterior_mean"
twin, n_steps, no side effects, refusals and the DAgger wiring. N = 193 envs on the synth tables of
tests/test_hindsight_posterior_gpu.py with 1, 6 and 67 draws and on the ragged table of tests/table_edges.py; one twin
and one call per case, shared by the tests."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from weather2alert_amd import _ffi, policy as P, synth, tables

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hindsight_values_cases as K  # noqa: E402
import table_edges as E  # noqa: E402
from hindsight_posterior_values_restatement import hindsight_posterior_values_fp64  # noqa: E402
from policy_gradient_mlp_cases import MATRIX, net as case_net  # noqa: E402

pytestmark = pytest.mark.gpu

# budgets 0, 8 (one 64-state chunk), 40 (several chunks, in LDS) and 200 (the pool path) on the 6-draw table; one draw,
# 67 draws (past one 64-lane chunk of draws) and the ragged table at budget 8
CASES = [("synth6", 0), ("synth6", 8), ("synth6", 40), ("synth6", 200), ("synth1", 8), ("synth67", 8), ("ragged", 8)]
FLOATS = ("alert_gain", "value", "loss")
PM_FIELDS = ("t", "used", "streak", "budget", "n_days", "county_w", "year_i", "coef_col", "finished")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _synth(n_samples):  # tests/test_hindsight_posterior_gpu.py::_synth
    return tables.compile_from_synth(synth.make_synth("linear", n_fips=30, years=[2006, 2007], n_samples=n_samples,
                                                      seed=17, extra_confounder_fips=3))


@pytest.fixture(scope="module")
def tabs():
    t = E.make_tables()
    return {"synth1": _synth(1), "synth6": _synth(6), "synth67": _synth(67), "ragged": t["ragged"].ct,
            "slot27": t["slot27"].ct}


def lds_fits(U, hb, n_samples):
    """w2a_hindsight_posterior's split between LDS and the pool: hs_pm_fixed_bytes (16 B per day + 96 B per draw) plus
    hs_dp_bytes (csrc/w2a_hindsight_posterior.hip.h, csrc/w2a_hindsight.hip.h)"""
    ns = (U + 1) * (U + 4) // 2
    return 16 * hb + 96 * n_samples + 16 * ns + 8 * hb * ((ns + 63) // 64) <= 64 * 1024


def _clone(st):
    return {k: v.clone() for k, v in st.items()}


def _env(dev, tabs, table, budget, start, **kw):
    """a fresh env of the case's batch, stepped `start` days with fixed actions (the same for every twin)"""
    from weather2alert_amd import HeatAlertVecEnv

    env = HeatAlertVecEnv(K.N, tables=tabs[table], device=dev, autoreset="disabled", env_gid0=E.GID0,
                          similar_climate_counties=True, **kw)
    env.reset(seed=11, options={"budget": budget})
    acts = torch.as_tensor(K.prefix_actions(K.N, start, seed=budget + 1), device=dev)
    for d in range(start):
        env.step(acts[d] * (env.state()["finished"] == 0).to(torch.int32))
    return env


def _same(a, b):
    """bit equality of two outputs of hindsight_posterior_values() / hindsight_values() (NaN gains included)"""
    assert set(a) == set(b)
    for k in a:
        x, y = a[k], b[k]
        if x.is_floating_point():
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k
        else:
            assert torch.equal(x, y), k


def _issued(sched, st0, T):
    """the alerts a schedule of attempts ISSUES from st0: the first budget - used attempts from the start day on"""
    rem = (st0["budget"] - st0["used"]).clamp(min=0).long()
    day = torch.arange(T, device=sched.device)[None, :]
    att = sched & (day >= st0["t"].long()[:, None])
    return (att & (att.long().cumsum(1) <= rem[:, None])) | (sched & ~att)


_BUNDLES = {}


def _bundle(dev, tabs, table, budget):
    """per (start, p): the start state, the schedule, hindsight_posterior_values(value, loss, share=False) on env A
    (with the no-side-effect checks), and what a twin stepped through step() along the schedule saw: liveness per
    call-day, the state after k days for the later-start test, and hindsight_posterior_optimum()'s bit of the day at
    hand from the twin's state on every 7th call-day and the last three"""
    key = (table, budget)
    if key in _BUNDLES:
        return _BUNDLES[key]
    ct = tabs[table]
    rows = torch.arange(K.N, device=dev)
    out = []
    for start in K.STARTS:
        A = _env(dev, tabs, table, budget, start)
        st0 = _clone(A.state())
        assert (st0["budget"] == budget).all()
        for p in K.PS:
            sched = torch.as_tensor(K.schedule(K.N, ct.T, p, seed=int(100 * p) + start), device=dev)
            before = A.state_dict()
            obs_before = A._obs.clone()
            hv = A.hindsight_posterior_values(sched, value=True, loss=True, share=False)
            after = A.state_dict()
            for k in ("state", "obs", "final_return", "reward", "done"):  # no side effects
                assert torch.equal(before[k], after[k]), k
            assert before["host"] == after["host"] and torch.equal(obs_before, A._obs)
            B = _env(dev, tabs, table, budget, start)
            S = ct.T - start
            twin = dict(live=torch.zeros((ct.T, K.N), dtype=torch.bool, device=dev), states={}, opt=[], attempts_over=0)
            for s in range(S):
                st = B.state()
                live = st["finished"] == 0
                if not bool(live.any()):
                    break
                t = st["t"].long().clamp(max=ct.T - 1)
                if s in K.CHUNKS:
                    twin["states"][s] = _clone(st)
                if s % 7 == 0 or s >= S - 3:
                    bit = B.hindsight_posterior_optimum()["alert_days"][rows, t]
                    twin["opt"].append((s, live.clone(), t.clone(), bit))
                a = sched[rows, t] & live
                twin["attempts_over"] += int((a & (st["used"] >= st["budget"])).sum())
                B.step(a.to(torch.int32))
                twin["live"][s] = live
            B.close()
            out.append(dict(start=start, p=p, st0=st0, sched=sched, hv=hv, twin=twin))
        assert A.check_status() in (0, 4)  # 4: step() past the ragged table's shortest episodes in the prefix
        A.close()
    _BUNDLES[key] = out
    return out


# ------------------------------------------------------------------ contract 1
@pytest.mark.parametrize("table,budget", CASES)
@pytest.mark.parametrize("gated", [False, True])
def test_along_the_optimums_own_schedule(dev, tabs, table, budget, gated):
    """hindsight_posterior_optimum()["alert_days"], with and without a gate, share on and off: the expert bits are the
    schedule, every loss is +0 bitwise and the regret is +0"""
    ct = tabs[table]
    for start in K.STARTS:
        A = _env(dev, tabs, table, budget, start)
        gate = torch.as_tensor(K.schedule(K.N, ct.T, 0.5, seed=5), device=dev) if gated else None
        hs = A.hindsight_posterior_optimum(allowed_days=gate)
        for share in (True, False):
            hv = A.hindsight_posterior_values(hs["alert_days"], allowed_days=gate, value=True, loss=True, share=share)
            assert torch.equal(hv["expert_alert_days"], hs["alert_days"])
            assert (hv["loss"].view(torch.int32) == 0).all() and (hv["regret"].view(torch.int32) == 0).all()
        assert budget == 0 or bool(hs["alert_days"].any())
        if gated:  # an attempt on a closed day is 0 before the budget test: no output bit changes
            closed = ~gate
            assert not (hv["expert_alert_days"] & closed).any()
            _same(hv, A.hindsight_posterior_values(hs["alert_days"] | closed, allowed_days=gate, value=True, loss=True))
        assert A.check_status() in (0, 4)
        A.close()


# ------------------------------------------------------------------ contract 2
@pytest.mark.parametrize("gated", [False, True])
def test_one_draw_is_hindsight_values_bit_for_bit(dev, tabs, gated):
    """n_samples = 1: 0.0 + (double) r and x / 1.0 are exact, so every output equals hindsight_values()'s"""
    ct = tabs["synth1"]
    gate = torch.as_tensor(K.schedule(K.N, ct.T, 0.6, seed=4), device=dev) if gated else None
    n_bits, regret = 0, 0.0
    for c in _bundle(dev, tabs, "synth1", 8):
        A = _env(dev, tabs, "synth1", 8, c["start"])
        own = A.hindsight_values(c["sched"], allowed_days=gate, value=True, loss=True)
        if gated:
            _same(A.hindsight_posterior_values(c["sched"], allowed_days=gate, value=True, loss=True), own)
        else:
            _same(c["hv"], own)
        n_bits += int(own["expert_alert_days"].sum())
        regret = max(regret, float(own["regret"].max()))
        A.close()
    assert n_bits > 0 and regret > 0  # (after 25 days of the prefix most envs have spent a budget of 8)


# ------------------------------------------------------------------ contract 3, the expert bit
@pytest.mark.parametrize("table,budget", CASES)
def test_expert_bits_equal_the_optimum_of_a_stepped_twin(dev, tabs, table, budget):
    """On every 7th call-day and the last three, hindsight_posterior_optimum() from the twin's state has the same bit
    for the day at hand as "expert_alert_days"; gains are NaN exactly where the env does not step; losses and the regret
    are not negative; days outside the stretch carry no bits. On the 6-draw table at least one expert bit differs from
    hindsight_values()'s: the draw-blind expert is another expert."""
    ct = tabs[table]
    rows = torch.arange(K.N, device=dev)
    n_bits = n_other = 0
    for c in _bundle(dev, tabs, table, budget):
        hv, twin = c["hv"], c["twin"]
        assert len(twin["opt"]) >= 10
        for s, live, t, bit in twin["opt"]:
            mine = hv["expert_alert_days"][rows, t]
            assert torch.equal(mine[live], bit[live]), (c["start"], c["p"], s)
            n_bits += int(bit[live].sum())
        S = hv["alert_gain"].shape[0]
        assert hv["alert_gain"].shape == hv["value"].shape == hv["loss"].shape == (ct.T, K.N)
        live = twin["live"][:S]
        assert torch.isnan(hv["alert_gain"][~live]).all() and (hv["value"][~live] == 0).all()
        assert (hv["loss"] >= 0).all() and (hv["loss"][~live] == 0).all() and (hv["regret"] >= 0).all()
        assert torch.isfinite(hv["value"]).all() and torch.isfinite(hv["regret"]).all()
        t0, nd = c["st0"]["t"].long(), c["st0"]["n_days"].long()
        day = torch.arange(ct.T, device=dev)[None, :]
        inside = (day >= t0[:, None]) & (day < nd[:, None]) & (c["st0"]["finished"] == 0)[:, None]
        assert not (hv["expert_alert_days"] & ~inside).any()
        if budget == 0:  # no alert is ever possible
            assert torch.isnan(hv["alert_gain"]).all() and not hv["expert_alert_days"].any()
            assert (hv["loss"].view(torch.int32) == 0).all() and (hv["regret"].view(torch.int32) == 0).all()
        else:
            assert twin["attempts_over"] > 0 or c["p"] < 0.5 or budget > 40
        if table == "synth6" and budget == 8:
            A = _env(dev, tabs, table, budget, c["start"])
            n_other += int((A.hindsight_values(c["sched"])["expert_alert_days"] != hv["expert_alert_days"]).sum())
            A.close()
    assert n_bits > 0 or budget == 0
    assert n_other > 0 or not (table == "synth6" and budget == 8)


# ------------------------------------------------------------------ contracts 3 (rows), 4 and 5
@pytest.mark.parametrize("table,budget", CASES)
def test_later_starts_attempts_sample_sharing_and_determinism(dev, tabs, table, budget):
    """Rows s >= k of one call equal, bit for bit, the call from the state the schedule reaches after k days (k = 7: the
    U bin of a budget-40 env changes; k = 100: a budget-200 env moves from the pool to LDS); clearing the attempts that
    found no budget changes no output bit; neither does another `sample`; share=True is share=False; two identical
    calls give identical bits."""
    ct = tabs[table]
    A = _env(dev, tabs, table, budget, 0)
    moved = False
    for c in _bundle(dev, tabs, table, budget):
        hv, sched, st0 = c["hv"], c["sched"], c["st0"]
        kw = dict(start_state=st0, value=True, loss=True)
        _same(hv, A.hindsight_posterior_values(sched, share=False, **kw))
        _same(hv, A.hindsight_posterior_values(sched, **kw))
        assert A.last_hindsight_posterior_keys <= K.N
        _same(hv, A.hindsight_posterior_values(_issued(sched, st0, ct.T), **kw))
        other = dict(st0, sample=(st0["sample"] + 1) % ct.n_samples)
        for share in (True, False):
            _same(hv, A.hindsight_posterior_values(sched, share=share, **dict(kw, start_state=other)))
        day = torch.arange(ct.T, device=dev)[None, :]
        for k, stk in c["twin"]["states"].items():
            part = A.hindsight_posterior_values(sched, start_state=stk, value=True, loss=True)
            S = ct.T - k
            for f in FLOATS:
                assert torch.equal(hv[f][k:].view(torch.int32), part[f][:S].view(torch.int32)), (f, k, c["start"], c["p"])
            later = day >= (st0["t"].long() + k)[:, None]
            assert torch.equal(hv["expert_alert_days"] & later, part["expert_alert_days"]), k
            if budget == 200:
                u0 = int((st0["budget"] - st0["used"]).min())
                uk = int(torch.minimum(stk["budget"] - stk["used"], stk["n_days"] - stk["t"]).max())
                moved |= (not lds_fits(min(u0, ct.T - c["start"]), ct.T, ct.n_samples)) and lds_fits(uk, ct.T, ct.n_samples)
            if budget == 40 and k == 7:
                assert bool((stk["used"] > st0["used"]).any())  # U = min(budget - used, H) changed
        assert set(c["twin"]["states"]) == set(K.CHUNKS)
    assert moved or budget != 200
    assert A.check_status() == 0
    A.close()


def test_sharing_on_a_deterministic_learners_batch(dev, tabs):
    """the batch of tests/test_hindsight_posterior_gpu.py::test_sharing with one schedule per problem (what a
    deterministic learner plays): fewer than half the envs run, finished envs and starts outside the tables included,
    and the outputs are share=False's bit for bit. One flipped bit inside an env's stretch gives it a key of its own."""
    ct = tabs["synth6"]
    n = K.N
    env = _env(dev, tabs, "synth6", 5, 0)
    st0 = _clone(env.state())
    q = n // 4
    for r in (1, 2, 3):  # the other three quarters repeat the first with other draws
        for k in st0:
            st0[k][r * q:(r + 1) * q] = st0[k][:q] if k != "sample" else (st0[k][:q] + r) % ct.n_samples
    sched = torch.as_tensor(K.schedule(n, ct.T, 0.2, seed=2), device=dev)
    for r in (1, 2, 3):
        sched[r * q:(r + 1) * q] = sched[:q]
    st0["finished"][5] = st0["finished"][q + 5] = 1
    st0["coef_col"][7] = ct.S + 3  # outside the tables: NaN
    st0["sample"][q + 9] = ct.n_samples  # this one alone, not its twins
    a = env.hindsight_posterior_values(sched, start_state=st0, value=True, loss=True)
    keys = env.last_hindsight_posterior_keys
    b = env.hindsight_posterior_values(sched, start_state=st0, value=True, loss=True, share=False)
    assert env.last_hindsight_posterior_keys == n
    fields = torch.stack([st0[k] for k in PM_FIELDS], 1)
    assert keys == len(torch.unique(torch.cat([fields, P.pack_alert_days(sched, (ct.T + 31) // 32)], 1), dim=0)) + 1
    assert keys <= n - 3 * q + 3 < n // 2  # q problems four times, the last env once, the three marked envs
    _same(a, b)
    assert torch.isnan(a["regret"][7]) and torch.isnan(a["regret"][q + 9]) and not torch.isnan(a["regret"][9])
    assert int(torch.isnan(a["regret"]).sum()) == 2 and torch.isnan(a["value"][:, 7]).all()
    assert float(a["regret"][5]) == 0.0 and torch.isnan(a["alert_gain"][:, 5]).all() and not a["expert_alert_days"][5].any()
    sched[q + 11, 30] ^= True
    env.hindsight_posterior_values(sched, start_state=st0)
    assert env.last_hindsight_posterior_keys == keys + 1
    gate = torch.ones_like(sched)  # under allowed_days nothing is shared; an all-true gate changes no bit
    _same(env.hindsight_posterior_values(sched, start_state=st0, allowed_days=gate),
          env.hindsight_posterior_values(sched, start_state=st0, share=False))
    assert env.last_hindsight_posterior_keys == n
    env.close()


# ------------------------------------------------------------------ the fp64 restatement and the regret (contract 6)
@pytest.mark.parametrize("table,budget", CASES)
def test_against_the_fp64_restatement(dev, tabs, table, budget):
    """"value" within (H_e - s) DAY_BAR of the restatement (a mean of rewards that each meet the per-day bar meets it,
    and so does the maximum over schedules of sums of them), "alert_gain" and "loss" within twice that, equal NaN
    patterns, the expert bit the restatement's wherever its |gain| exceeds its own bound. "regret" >= 0 and against
    hindsight_posterior_optimum(st0)["return"] less the fp64 draw-mean of posterior_returns(st0, issued): the f32
    recursive-summation bound 2 (H_e - 1) 2^-24 abs_reward_e of the per-draw returns plus one f32 rounding (2^-24
    relative) of the optimum's return, of the mean's summands (bounded by abs_reward_e) and of the regret itself.
    The restatement costs K x what hindsight_values_fp64 costs, so it restates every 16th env (67 draws: every 48th;
    budget 200: two envs); the kernel runs all 193 and the exact tests above read all of them."""
    ct = tabs[table]
    envs = [3, 100] if budget == 200 else list(range(0, K.N, 48 if table == "synth67" else 16))
    A = _env(dev, tabs, table, budget, 0)
    worst = dict(value=0.0, alert_gain=0.0, loss=0.0, regret=0.0)
    for c in _bundle(dev, tabs, table, budget):
        hv, st0, sched = c["hv"], c["st0"], c["sched"]
        st = {k: st0[k].cpu().numpy().astype(np.int64) for k in K.HS_KEYS}
        ref = hindsight_posterior_values_fp64(ct.X, ct.W, ct.n_samples, ct.Y, st, ct.T, sched.cpu().numpy(), envs=envs)
        H = ref["H"][envs]
        left = np.maximum(H[None, :] - np.arange(ct.T)[:, None], 0)  # H_e - s
        for f, key, mult in (("value", "value", 1), ("alert_gain", "gain", 2), ("loss", "loss", 2)):
            got, want = hv[f].double().cpu().numpy()[:, envs], ref[key][:, envs]
            assert (np.isnan(got) == np.isnan(want)).all(), f
            err = np.nan_to_num(np.abs(got - want))
            bound = mult * left * K.DAY_BAR
            worst[f] = max(worst[f], float((err / np.maximum(bound, 1e-300))[left > 0].max(initial=0.0)))
            assert (err <= bound).all(), (f, c["start"], c["p"], float((err - bound).max()))
        t0 = st["t"][envs]
        for i, e in enumerate(envs):  # the expert bit where the restatement's gain is beyond its own bound
            g = np.nan_to_num(ref["gain"][:H[i], e])
            sure = np.abs(g) > 2 * left[:H[i], i] * K.DAY_BAR
            mine = hv["expert_alert_days"][e].cpu().numpy()[t0[i]:t0[i] + H[i]]
            assert (mine[sure] == ref["expert"][e, t0[i]:t0[i] + H[i]][sure]).all(), (e, c["start"], c["p"])
        opt = A.hindsight_posterior_optimum(st0)["return"].double().cpu().numpy()[envs]
        mean = A.posterior_returns(st0, _issued(sched, st0, ct.T)).double().mean(1).cpu().numpy()[envs]
        got = hv["regret"].double().cpu().numpy()
        assert (got >= 0).all()
        got, absr = got[envs], ref["abs_reward"][envs]
        bound = 2.0 * np.maximum(H - 1, 0) * 2.0 ** -24 * absr + 2.0 ** -24 * (np.abs(opt) + absr + np.abs(got))
        err = np.abs(got - (opt - mean))
        worst["regret"] = max(worst["regret"], float((err / np.maximum(bound, 1e-300))[bound > 0].max(initial=0.0)))
        assert (err <= bound).all(), (c["start"], c["p"], float((err - bound).max()))
    print(f"{table} budget {budget}: largest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    A.close()


def test_posterior_mean_twin(dev, tabs):
    """a reward_mode="posterior_mean" env (accepted by the call) stepped along the schedule pays value[0] - regret,
    within 2 H_e day bars (the value's bar and the stepped sum's)"""
    ct = tabs["synth6"]
    rows = torch.arange(K.N, device=dev)
    for start, p in ((0, 0.5), (25, 0.1)):
        pm = _env(dev, tabs, "synth6", 8, start, reward_mode="posterior_mean")
        sched = torch.as_tensor(K.schedule(K.N, ct.T, p, seed=int(100 * p) + start), device=dev)
        c = dict(start=start, p=p, sched=sched, hv=pm.hindsight_posterior_values(sched, value=True))
        assert start or float(c["hv"]["regret"].max()) > 0
        acc = torch.zeros(K.N, dtype=torch.float64, device=dev)
        H = torch.zeros(K.N, dtype=torch.float64, device=dev)
        for s in range(ct.T - c["start"]):
            st = pm.state()
            live = st["finished"] == 0
            if not bool(live.any()):
                break
            t = st["t"].long().clamp(max=ct.T - 1)
            r = pm.step((c["sched"][rows, t] & live).to(torch.int32))[1]
            acc += torch.where(live, r.double(), torch.zeros_like(acc))
            H += live
        err = (c["hv"]["value"][0].double() - c["hv"]["regret"].double() - acc).abs()
        print(f"start {c['start']} p {c['p']}: max |value[0] - regret - stepped return| / (2 H DAY_BAR) = "
              f"{float((err / (2 * H.clamp(min=1) * K.DAY_BAR)).max()):.3f}")
        assert bool((err <= 2 * H * K.DAY_BAR).all())
        pm.close()


# ------------------------------------------------------------------ n_steps, refusals, the C entry
def test_n_steps(dev, tabs):
    """n_steps = 5: [5, N] rows of a 5-day DP, against the restatement; n_steps = T + 3: the default call's rows, then
    NaN gains and 0 beyond T; without value / loss the keys are absent"""
    ct = tabs["synth6"]
    c = _bundle(dev, tabs, "synth6", 8)[1]  # from reset, p = 0.5
    A = _env(dev, tabs, "synth6", 8, 0)
    hv, st0, sched = c["hv"], c["st0"], c["sched"]
    five = A.hindsight_posterior_values(sched, start_state=st0, n_steps=5, value=True, loss=True)
    assert five["alert_gain"].shape == five["value"].shape == five["loss"].shape == (5, K.N)
    envs = list(range(0, K.N, 4))
    st = {k: st0[k].cpu().numpy().astype(np.int64) for k in K.HS_KEYS}
    ref = hindsight_posterior_values_fp64(ct.X, ct.W, ct.n_samples, ct.Y, st, 5, sched.cpu().numpy(), envs=envs)
    left = np.maximum(ref["H"][envs][None, :] - np.arange(5)[:, None], 0)
    for f, key, mult in (("value", "value", 1), ("alert_gain", "gain", 2), ("loss", "loss", 2)):
        got, want = five[f].double().cpu().numpy()[:, envs], ref[key][:, envs]
        assert (np.isnan(got) == np.isnan(want)).all() and (np.nan_to_num(np.abs(got - want)) <= mult * left * K.DAY_BAR).all(), f
    day = torch.arange(ct.T, device=dev)[None, :]
    assert not (five["expert_alert_days"] & (day >= (st0["t"].long() + 5)[:, None])).any()
    for share in (True, False):
        more = A.hindsight_posterior_values(sched, start_state=st0, n_steps=ct.T + 3, value=True, loss=True, share=share)
        for f in FLOATS:
            assert more[f].shape == (ct.T + 3, K.N)
            assert torch.equal(more[f][:ct.T].view(torch.int32), hv[f].view(torch.int32)), f
        assert torch.isnan(more["alert_gain"][ct.T:]).all() and (more["value"][ct.T:] == 0).all() and (more["loss"][ct.T:] == 0).all()
        assert torch.equal(more["expert_alert_days"], hv["expert_alert_days"])
        assert torch.equal(more["regret"].view(torch.int32), hv["regret"].view(torch.int32))
    bare = A.hindsight_posterior_values(sched, start_state=st0)
    assert set(bare) == {"alert_gain", "expert_alert_days", "regret"}
    _same(bare, {k: hv[k] for k in bare})
    words = P.pack_alert_days(sched, (ct.T + 31) // 32)  # packed words are taken as they are
    _same(bare, A.hindsight_posterior_values(words, start_state=st0))
    assert A.check_status() == 0
    A.close()


def _c_call(env, ct, dev, st, sched, ws_bytes):
    n = env.num_envs
    v = _ffi.StateView()
    for k in _ffi.STATE_FIELDS:
        setattr(v, k, st[k].data_ptr())
    words = (ct.T + 31) // 32
    mask = P.pack_alert_days(sched, words)
    outs = dict(gain=torch.full((ct.T, n), 5.0, dtype=torch.float32, device=dev),
                expert=torch.full((n, words), 7, dtype=torch.int32, device=dev),
                regret=torch.full((n,), 5.0, dtype=torch.float32, device=dev),
                value=torch.full((ct.T, n), 5.0, dtype=torch.float32, device=dev),
                loss=torch.full((ct.T, n), 5.0, dtype=torch.float32, device=dev))
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
    rc = env._lib.w2a_hindsight_posterior_along(env._h, C.byref(v), ct.T, mask.data_ptr(), words, None, 0,
                                                outs["gain"].data_ptr(), outs["expert"].data_ptr(),
                                                outs["regret"].data_ptr(), outs["value"].data_ptr(),
                                                outs["loss"].data_ptr(), ws.data_ptr(), ws_bytes, None)
    torch.cuda.synchronize()
    untouched = all(bool((x == (7 if k == "expert" else 5.0)).all()) for k, x in outs.items())
    return rc, env._lib.w2a_last_error(), untouched, outs


def test_refusals(dev, tabs):
    """corrected-semantics fixes, the slot-27 table, a stream capture, too many draws and a workspace one byte short
    (with and without a pool): each with its message and before anything is written; the full workspace is taken"""
    from weather2alert_amd import HeatAlertVecEnv

    ct = tabs["synth6"]
    sched = torch.as_tensor(K.schedule(64, ct.T, 0.3, seed=1), device=dev)
    env = HeatAlertVecEnv(64, tables=ct, device=dev, fixes={"lag"})
    env.reset(seed=1)
    with pytest.raises(ValueError, match=r"hindsight_posterior_values\(\) needs faithful semantics"):
        env.hindsight_posterior_values(sched)
    full = env._lib.w2a_hindsight_posterior_workspace_bytes(64, ct.T, ct.n_samples, ct.T, 14, 1)
    rc, msg, untouched, _ = _c_call(env, ct, dev, env.state(), sched, full)
    assert rc == -1 and b"w2a_hindsight_posterior_along" in msg and b"corrected-semantics" in msg and untouched
    env.close()
    s27 = tabs["slot27"]
    bad = HeatAlertVecEnv(64, tables=s27, device=dev)
    bad.reset(seed=1)
    sched27 = torch.zeros((64, s27.T), dtype=torch.bool, device=dev)
    with pytest.raises(ValueError, match=r"hindsight_posterior_values\(\).*slot-27"):
        bad.hindsight_posterior_values(sched27)
    full27 = bad._lib.w2a_hindsight_posterior_workspace_bytes(64, s27.T, s27.n_samples, s27.T, 1 << 20, 1)
    rc, msg, untouched, _ = _c_call(bad, s27, dev, bad.state(), sched27, full27)
    assert rc == -1 and b"w2a_hindsight_posterior_along: a coefficient row has a nonzero slot-27" in msg and untouched
    bad.close()
    ok = HeatAlertVecEnv(64, tables=ct, device=dev, fixes={"budget"}, autoreset="disabled")
    for budget in (8, 200):  # without and with a pool
        ok.reset(seed=1, options={"budget": budget})
        st = _clone(ok.state())
        full = ok._lib.w2a_hindsight_posterior_workspace_bytes(64, ct.T, ct.n_samples, ct.T, budget, 1)  # one env's pool
        assert (full > ok._lib.w2a_hindsight_posterior_workspace_bytes(64, ct.T, ct.n_samples, ct.T, 0, 1)) == (budget == 200)
        rc, msg, untouched, _ = _c_call(ok, ct, dev, st, sched, full - 1)
        assert rc == -1 and untouched and (b"workspace too small" if budget == 200 else b"workspace smaller than") in msg
        full = ok._lib.w2a_hindsight_posterior_workspace_bytes(64, ct.T, ct.n_samples, ct.T, budget, 64)
        rc, msg, untouched, outs = _c_call(ok, ct, dev, st, sched, full)
        assert rc == 0 and not untouched
        hv = ok.hindsight_posterior_values(sched, start_state=st, value=True, loss=True)
        _same(hv, dict(alert_gain=outs["gain"], expert_alert_days=P.unpack_alert_days(outs["expert"], ct.T),
                       regret=outs["regret"], value=outs["value"], loss=outs["loss"]))
    with pytest.raises(_ffi.W2AError, match="recording a hipGraph"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            ok.hindsight_posterior_values(sched, start_state=st)
    assert ok.check_status() == 0
    ok.close()
    big = _synth(658)  # 16 B x 153 days + 96 B x 658 draws pass 64 KiB: the library refuses
    env = HeatAlertVecEnv(64, tables=big, device=dev)
    env.reset(seed=1)
    with pytest.raises(_ffi.W2AError, match="w2a_hindsight_posterior_along: the tables' n_samples is too large"):
        env.hindsight_posterior_values(sched)
    assert env.hindsight_posterior_values(sched, n_steps=30)["alert_gain"].shape == (30, 64)  # 16 x 30 + 96 x 658 fit
    env.close()


# ------------------------------------------------------------------ the DAgger wiring
def test_expert_labels_feed_imitation_gradient(dev, tabs):
    """imitation_gradient(pol, sched, labels=hindsight_posterior_values(sched)["expert_alert_days"]) runs for the
    linear kind and one MLP shape: the env is forced along the schedule, so "days" equal the call without labels, and
    the gradient is another one"""
    ct = tabs["synth6"]
    c = _bundle(dev, tabs, "synth6", 8)[1]  # from reset, p = 0.5
    A = _env(dev, tabs, "synth6", 8, c["start"])
    sched, labels = c["sched"], c["hv"]["expert_alert_days"]
    assert bool((labels != sched).any()) and bool(labels.any())
    g = E.groups(K.N)
    rng = np.random.default_rng(3)
    W = (rng.standard_normal((E.G, ct.n_obs)) * 0.4).astype(np.float32)
    _, hidden, act, n_out = MATRIX["tanh7x13"]
    pols = {"linear": dict(kind="linear", weight=W, bias=(rng.standard_normal(E.G) * 0.5).astype(np.float32), group=g),
            "mlp": dict(kind="mlp", layers=case_net(ct, "tanh7x13", hidden, n_out), activation=act, group=g)}
    for name, pol in pols.items():
        a = A.imitation_gradient(pol, sched)
        b = A.imitation_gradient(pol, sched, labels=labels)
        assert torch.equal(a["days"], b["days"]) and int(a["days"].sum()) > 0, name
        ga = a["policy_gradient"]["weight"] if name == "linear" else a["policy_gradient"]["layers"][0][0]
        gb = b["policy_gradient"]["weight"] if name == "linear" else b["policy_gradient"]["layers"][0][0]
        assert torch.isfinite(gb).all() and not torch.equal(ga, gb), name
    assert A.check_status() in (0, 4)
    A.close()
