"""Returns under every posterior draw on the GPU (k_posterior_returns): against the reference's per-draw rewards
(tests/golden/posterior_draws.npz), bit-identity of each env's own draw with the rollout's return, every column against
the fp64 restatement (tests/posterior_restatement.py), partial and chained calls, unchanged outputs, the
posterior-mean env, group means, refusals, and full size.
Uniform tables only; the same kernel on ragged episode lengths and slot-27 coefficient rows:
tests/test_table_edges_gpu.py."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

from weather2alert_amd import _ffi, synth, tables

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from posterior_restatement import posterior_returns_fp64  # noqa: E402

pytestmark = pytest.mark.gpu

RETURN_RTOL, RETURN_ATOL = 2e-6, 2e-5  # as tests/test_env_gpu.py
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATE_KEYS = ("t", "used", "streak", "hist14", "budget", "n_days", "county_w", "year_i", "coef_col", "finished")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ct():
    return tables.compile_from_synth(synth.make_synth("linear", n_fips=30, years=[2006, 2007], n_samples=6, seed=17,
                                                      extra_confounder_fips=3))


def _np_state(st):
    return {k: st[k].cpu().numpy().copy() for k in STATE_KEYS}


def _restate(ct, st0, alert_days, n_steps):
    ad = alert_days.cpu().numpy() if torch.is_tensor(alert_days) else alert_days
    return posterior_returns_fp64(ct.X, ct.W, ct.n_samples, len(ct.years), st0, ad, n_steps)


def _params(ct, G, seed, scale=0.4):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((G, ct.n_obs)) * scale).astype(np.float32)
    W[:, ct.feature_names.index("remaining_budget")] *= 0.1
    return W, (rng.standard_normal(G) * 0.5).astype(np.float32)


def _mlp(ct, G, seed, hidden=16):
    rng = np.random.default_rng(seed)
    W1 = (rng.standard_normal((G, hidden, ct.n_obs)) * 0.3).astype(np.float32)
    b1 = (rng.standard_normal((G, hidden)) * 0.3).astype(np.float32)
    Wo = (rng.standard_normal((G, 1, hidden)) * 0.5).astype(np.float32)
    bo = (rng.standard_normal((G, 1)) * 0.3).astype(np.float32)
    return [(W1, b1), (Wo, bo)]


def _own(out, st0):
    """column sample_e of every env: its own draw"""
    return out["posterior_returns"].gather(1, st0["sample"].long()[:, None])[:, 0]


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("data", ["mini", "mini64"])
def test_reference_replay(dev, data):
    """Reset to the fixture's episode tuples, step its actions through step(): posterior_returns of the whole episode
    against the reference's per-draw returns (2e-6 relative or 1e-5 absolute), each day's mean over the draws against
    the reference's mean (1e-5), and the posterior-mean env's step() rewards against the same mean."""
    from weather2alert_amd import HeatAlertVecEnv

    d = dict(np.load(os.path.join(GOLDEN, "posterior_draws.npz")))
    meta = json.loads(str(d["meta_json"]))
    idx = [i for i, e in enumerate(meta["episodes"]) if e["data"] == data]
    ctd = tables.CompiledTables.load_npz(os.path.join(GOLDEN, f"{data}_compiled.npz"))
    K, T, E = ctd.n_samples, ctd.T, len(idx)
    eps = [meta["episodes"][i]["episode_index"].split("_") for i in idx]
    tup = dict(county_w=[ctd.fips_weather.index(f) for f, _ in eps], year_i=[ctd.years.index(int(y)) for _, y in eps],
               coef_col=d["location_index"][idx], sample=d["coef_index"][idx], budget=d["budget"][idx])
    ref = d["reward"][idx][:, :, :K]
    acts = d["actions"][idx]
    alert_days = torch.as_tensor(d["actual"][idx].astype(bool), device=dev)
    env = HeatAlertVecEnv(E, tables=ctd, device=dev, autoreset="disabled")
    pm = HeatAlertVecEnv(E, tables=ctd, device=dev, autoreset="disabled", reward_mode="posterior_mean")
    env.reset(options={"episodes": tup})
    pm.reset(options={"episodes": tup})
    st0 = {k: v.clone() for k, v in env.state().items()}
    day_pr, pm_r = [], []
    for t in range(T):
        st = {k: v.clone() for k, v in env.state().items()}
        a = torch.as_tensor(acts[:, t], device=dev)
        env.step(a)
        _, r, _, _, _ = pm.step(a)
        pm_r.append(r.double().cpu().numpy().copy())
        day_pr.append(env.posterior_returns(st, alert_days, n_steps=1).double().cpu().numpy())
    assert env.check_status() == 0 and pm.check_status() == 0
    np.testing.assert_array_equal(env.state()["used"].cpu().numpy(), d["actual"][idx].sum(1))
    pr = env.posterior_returns(st0, alert_days)
    assert pr.shape == (E, K) and pr.dtype == torch.float32
    np.testing.assert_allclose(pr.double().cpu().numpy(), np.nansum(ref, axis=1), rtol=2e-6, atol=1e-5)
    days = np.stack(day_pr, axis=1)  # [E, T, K]
    live = ~np.isnan(ref[:, :, 0])
    np.testing.assert_allclose(days[live], ref[live], rtol=0, atol=1e-5)
    np.testing.assert_allclose(days.mean(2)[live], np.nanmean(ref, axis=2)[live], rtol=0, atol=1e-5)
    # the posterior-mean reward of step() is the mean over the draws of the per-draw rewards
    pmr = np.stack(pm_r, axis=1)
    print(f"{data}: max |pm step reward - reference draw mean| = {np.abs(pmr[live] - np.nanmean(ref, 2)[live]).max():.2e}")
    np.testing.assert_allclose(pmr[live], np.nanmean(ref, axis=2)[live], rtol=0, atol=1e-5)
    env.close()
    pm.close()


# ------------------------------------------------------------------ own draw, every column
def _policies(ct, n, G):
    g = np.random.default_rng(9).integers(0, G, n) if G > 1 else None
    W, b = _params(ct, G, 6)
    lin = dict(kind="linear", weight=W, bias=b)
    mlp = dict(kind="mlp", layers=_mlp(ct, G, 4), activation="tanh")
    if g is not None:
        lin["group"] = g
        mlp["group"] = g
    return {"linear": lin, "linear_sampled": dict(lin, sample=True, seed=3), "mlp": mlp,
            "mlp_sampled": dict(mlp, sample=True, seed=5)}


@pytest.mark.parametrize("G", [1, 3])
def test_own_draw_is_the_rollouts_return(dev, ct, G):
    """posterior_returns[e, sample_e] == return[e] bit for bit for linear and mlp (greedy and sampled), and the other
    columns against the fp64 restatement."""
    from weather2alert_amd import HeatAlertVecEnv

    n = 4096 + 37
    for name, pol in _policies(ct, n, G).items():
        env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", similar_climate_counties=True)
        env.reset(seed=11, options={"budget": 4})
        st0 = {k: v.clone() for k, v in env.state().items()}
        out = env.rollout(pol, posterior_returns=True, alert_mask=True)
        assert out["posterior_returns"].shape == (n, ct.n_samples)
        assert torch.equal(_own(out, st0), out["return"]), name
        ref = _restate(ct, _np_state(st0), out["alert_days"], ct.T)
        np.testing.assert_allclose(out["posterior_returns"].double().cpu().numpy(), ref, rtol=RETURN_RTOL,
                                   atol=RETURN_ATOL)
        gp = out["group_posterior_returns"]
        assert gp.shape == (G, ct.n_samples)
        assert int(out["alerts"].sum()) > 0
        env.close()


@pytest.mark.parametrize("mfma", [False, True])
@pytest.mark.parametrize("kind", ["threshold", "bernoulli", "always"])
def test_builtin_kinds(dev, ct, kind, mfma):
    """Built-in policies: bit-identical own draw on k_rollout64 (rollout_mfma=False), within 2e-6 relative on
    k_rollout_mfma."""
    from weather2alert_amd import HeatAlertVecEnv

    n = 3000
    pol = {"threshold": dict(kind="threshold", feature="heat_qi", threshold=0.8, require_budget=True),
           "bernoulli": dict(kind="bernoulli", p=0.2, seed=1), "always": dict(kind="always")}[kind]
    env = HeatAlertVecEnv(n, tables=ct, device=dev, similar_climate_counties=True, rollout_mfma=mfma)
    env.reset(seed=5)
    st0 = {k: v.clone() for k, v in env.state().items()}
    out = env.rollout(pol, posterior_returns=True)
    assert env.last_rollout_kernel == ("k_rollout_mfma" if mfma else "k_rollout64")
    assert "alert_days" not in out and "group_posterior_returns" not in out
    own = _own(out, st0)
    if mfma:
        np.testing.assert_allclose(own.double().cpu().numpy(), out["return"].double().cpu().numpy(), rtol=2e-6, atol=0)
    else:
        assert torch.equal(own, out["return"])
    env.close()


@pytest.mark.parametrize("n_samples", [100, 130])
def test_every_column_against_restatement(dev, n_samples):
    """Synthetic tables with 100 and 130 draws (more than two waves of lanes per env), augmentation on, budgets 0, 2
    and the table's default: every column within the reward bars of the fp64 restatement."""
    from weather2alert_amd import HeatAlertVecEnv

    cth = tables.compile_from_synth(synth.make_synth("linear", n_fips=40, years=[2006, 2007], n_samples=n_samples,
                                                     seed=23, extra_confounder_fips=5))
    n = 2048 + 5
    for budget in (0, 2, None):
        env = HeatAlertVecEnv(n, tables=cth, device=dev, autoreset="disabled", similar_climate_counties=True)
        env.reset(seed=budget or 7, options={} if budget is None else {"budget": budget})
        st0 = {k: v.clone() for k, v in env.state().items()}
        W, b = _params(cth, 1, 2)
        out = env.rollout(dict(kind="linear", weight=W, bias=b, sample=True, seed=8), posterior_returns=True,
                          alert_mask=True)
        pr = out["posterior_returns"]
        assert pr.shape == (n, n_samples)
        assert torch.equal(_own(out, st0), out["return"])
        ref = _restate(cth, _np_state(st0), out["alert_days"], cth.T)
        np.testing.assert_allclose(pr.double().cpu().numpy(), ref, rtol=RETURN_RTOL, atol=RETURN_ATOL)
        if budget == 0:
            assert int(out["alerts"].sum()) == 0
        env.close()


# ------------------------------------------------------------------ partial calls
def test_partial_calls_and_arbitrary_start_states(dev, ct):
    """Chained rollouts sum to one call; start states mid-episode, envs finished on entry (zero rows), envs whose
    episode ends inside the call, n_steps shorter than what is left -- against the restatement."""
    from weather2alert_amd import HeatAlertVecEnv

    n = 2500
    W, b = _params(ct, 1, 12)
    pol = dict(kind="linear", weight=W, bias=b)
    A = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", similar_climate_counties=True)
    B = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", similar_climate_counties=True)
    A.reset(seed=3)
    B.reset(seed=3)
    parts = [A.rollout(pol, n_steps=k, posterior_returns=True)["posterior_returns"] for k in (40, 60, 100)]
    whole = B.rollout(pol, posterior_returns=True)["posterior_returns"]
    np.testing.assert_allclose(sum(p.double() for p in parts).cpu().numpy(), whole.double().cpu().numpy(),
                               rtol=2e-6, atol=1e-5)
    # finished on entry: a further call gives zero rows
    again = A.rollout(pol, n_steps=5, posterior_returns=True)["posterior_returns"]
    assert (again == 0).all()
    # arbitrary start states through the method: random days, counters, histories, finished flags, random bitmaps
    rng = np.random.default_rng(4)
    st = _np_state(B.state())
    st["t"] = rng.integers(0, ct.T, n).astype(np.int32)
    st["used"] = rng.integers(0, 4, n).astype(np.int32)
    st["streak"] = rng.integers(0, 3, n).astype(np.int32)
    st["hist14"] = rng.integers(0, 1 << 14, n).astype(np.int32)
    st["finished"] = (rng.random(n) < 0.1).astype(np.int32)
    ad = rng.random((n, ct.T)) < 0.2
    for steps in (1, 17, ct.T):
        got = B.posterior_returns({k: torch.as_tensor(v, device=dev) for k, v in st.items()},
                                  torch.as_tensor(ad, device=dev), n_steps=steps)
        ref = _restate(ct, st, ad, steps)
        np.testing.assert_allclose(got.double().cpu().numpy(), ref, rtol=RETURN_RTOL, atol=RETURN_ATOL)
        assert (got[torch.as_tensor(st["finished"] == 1, device=dev)] == 0).all()
    A.close()
    B.close()


# ------------------------------------------------------------------ nothing else changes
@pytest.mark.parametrize("case", ["linear", "linear_record", "mlp", "threshold", "threshold_mask"])
def test_nothing_else_changes(dev, ct, case):
    from weather2alert_amd import HeatAlertVecEnv

    n = 3001
    g = np.random.default_rng(1).integers(0, 2, n)
    W, b = _params(ct, 2, 3)
    pol = {"linear": dict(kind="linear", weight=W, bias=b, group=g, sample=True, seed=1),
           "mlp": dict(kind="mlp", layers=_mlp(ct, 2, 2), activation="relu", group=g),
           "threshold": dict(kind="threshold", feature="heat_qi", threshold=0.7)}[case.split("_")[0]]
    kw = dict(record=case.endswith("record"), alert_mask=case.endswith("mask"))
    A = HeatAlertVecEnv(n, tables=ct, device=dev, similar_climate_counties=True)
    B = HeatAlertVecEnv(n, tables=ct, device=dev, similar_climate_counties=True)
    A.reset(seed=2)
    B.reset(seed=2)
    for steps in (50, None, 30):
        oa = A.rollout(pol, n_steps=steps, posterior_returns=True, **kw)
        ob = B.rollout(pol, n_steps=steps, **kw)
        extra = {"posterior_returns"} | ({"group_posterior_returns"} if "group_mean_return" in ob else set())
        assert set(oa) - set(ob) == extra and not set(ob) - set(oa)
        for k, v in ob.items():
            if k == "trajectory":  # what the record contract specifies: entries of steps taken, and the end slabs
                ta, val = oa[k], v["valid"]
                for kk in ("valid", "terminated", "alert"):
                    assert torch.equal(ta[kk], v[kk]), kk
                for kk in ("action", "logit", "reward"):
                    assert torch.equal(ta[kk][val], v[kk][val]), kk
                assert torch.equal(ta["obs"][0], v["obs"][0]) and torch.equal(ta["obs"][-1], v["obs"][-1])
                assert torch.equal(ta["obs"][1:-1][val[:-1]], v["obs"][1:-1][val[:-1]])
                continue
            a_ = oa[k]
            if v.is_floating_point():
                a_, v = a_.nan_to_num(7.0), v.nan_to_num(7.0)
            assert torch.equal(a_, v), k
        sa, sb = A.state_dict(), B.state_dict()
        for k in ("state", "obs", "final_return", "reward", "done"):
            assert torch.equal(sa[k], sb[k]), k
        assert sa["host"] == sb["host"]
        assert A.check_status() == 0
    A.close()
    B.close()


def test_posterior_mean_env(dev, ct):
    """reward_mode="posterior_mean": the mean over the draws of posterior_returns is the rollout's return (the
    posterior-mean kernels' bars)."""
    from weather2alert_amd import HeatAlertVecEnv

    n = 2000
    env = HeatAlertVecEnv(n, tables=ct, device=dev, autoreset="disabled", reward_mode="posterior_mean")
    env.reset(seed=6)
    out = env.rollout(dict(kind="bernoulli", p=0.3, seed=2), posterior_returns=True)
    m = out["posterior_returns"].double().mean(1).cpu().numpy()
    np.testing.assert_allclose(m, out["return"].double().cpu().numpy(), rtol=1e-5, atol=1e-4)
    env.close()


def test_group_posterior_returns(dev, ct):
    from weather2alert_amd import HeatAlertVecEnv

    n, G = 5000, 17
    g = np.random.default_rng(2).integers(0, G, n)
    W, b = _params(ct, G, 8)
    env = HeatAlertVecEnv(n, tables=ct, device=dev, similar_climate_counties=True)
    env.reset(seed=1)
    out = env.rollout(dict(kind="linear", weight=W, bias=b, group=g), posterior_returns=True)
    pr = out["posterior_returns"].double().cpu().numpy()
    gp = out["group_posterior_returns"].double().cpu().numpy()
    for j in range(G):
        np.testing.assert_allclose(gp[j], pr[g == j].mean(0), rtol=1e-6)
    np.testing.assert_allclose(out["group_mean_return"].double().cpu().numpy(),
                               [out["return"].double().cpu().numpy()[g == j].mean() for j in range(G)], rtol=1e-6)
    env.close()


def test_refusals(dev, ct):
    from weather2alert_amd import HeatAlertVecEnv

    env = HeatAlertVecEnv(64, tables=ct, device=dev, fixes={"lag"})
    env.reset(seed=1)
    st = env.state()
    with pytest.raises(ValueError, match="lag"):
        env.rollout(dict(kind="never"), posterior_returns=True)
    with pytest.raises(ValueError, match="lag"):
        env.posterior_returns(st, torch.zeros((64, ct.T), dtype=torch.bool, device=dev))
    v = _ffi.StateView()
    for k in _ffi.STATE_FIELDS:
        setattr(v, k, st[k].data_ptr())
    mask = torch.zeros((64, (ct.T + 31) // 32), dtype=torch.int32, device=dev)
    out = torch.empty((64, ct.n_samples), dtype=torch.float32, device=dev)
    rc = env._lib.w2a_posterior_returns(env._h, C.byref(v), mask.data_ptr(), mask.shape[1], 5, out.data_ptr(), None)
    assert rc == -1 and b"corrected-semantics" in env._lib.w2a_last_error()
    env.close()
    ok = HeatAlertVecEnv(64, tables=ct, device=dev, fixes={"budget"})
    ok.reset(seed=1)
    assert ok.rollout(dict(kind="always"), posterior_returns=True)["posterior_returns"].shape == (64, ct.n_samples)
    rc = ok._lib.w2a_posterior_returns(ok._h, C.byref(v), mask.data_ptr(), 1, 5, out.data_ptr(), None)
    assert rc == -1 and b"ceil(T/32)" in ok._lib.w2a_last_error()
    with pytest.raises(ValueError):
        ok.posterior_returns(ok.state(), torch.zeros((63, ct.T), dtype=torch.bool, device=dev))
    ok.close()


# ------------------------------------------------------------------ full size
def test_full_size(dev):
    """1 048 576 envs on BASELINE configs[2]'s synthetic tables (n_samples = 100), a whole episode of a greedy linear
    policy: own draws bit for bit, a strided sample of 4 097 envs against the restatement."""
    from weather2alert_amd import HeatAlertVecEnv

    sd = synth.make_synth("linear", years=list(range(2006, 2017)), n_samples=100, seed=0, extra_confounder_fips=60)
    cth = tables.compile_from_synth(sd)
    n = 1 << 20
    env = HeatAlertVecEnv(n, tables=cth, device=dev, similar_climate_counties=True, autoreset="disabled")
    env.reset(seed=0)
    st0 = {k: v.clone() for k, v in env.state().items()}
    W, b = _params(cth, 1, 1)
    out = env.rollout(dict(kind="linear", weight=W, bias=b), posterior_returns=True, alert_mask=True)
    assert env.check_status() == 0 and out["done"].all()
    pr = out["posterior_returns"]
    assert pr.shape == (n, 100) and torch.isfinite(pr).all()
    assert torch.equal(_own(out, st0), out["return"])
    idx = np.unique(np.concatenate([np.arange(0, n, 256), [n - 1]]))
    assert len(idx) == 4097
    sub = {k: v[idx] for k, v in _np_state(st0).items()}
    ad = out["alert_days"][torch.as_tensor(idx, device=dev)].cpu().numpy()
    ref = _restate(cth, sub, ad, cth.T)
    np.testing.assert_allclose(pr[torch.as_tensor(idx, device=dev)].double().cpu().numpy(), ref, rtol=RETURN_RTOL,
                               atol=RETURN_ATOL)
    env.close()
