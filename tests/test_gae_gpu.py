"""value_gradient(gamma=, gae_lambda=, bootstrap=, value_target=, target=) (k_value_gradient_linear_gae; k_gae_pass1 +
k_gae_finish + the second pass of w2a_policy_gradient_mlp) against the fp64 restatement (tests/gae_restatement.py). As in
tests/test_value_gradient_gpu.py, whose shapes and helpers are used, the reference never touches the kernels under test:
an identical twin from the same seed is stepped day by day through step() along the schedule and the rows and rewards it
returns go to the restatement. Every comparison requires |x - x_ref| <= bound for every component and prints the largest
ratio to the bound."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_edges as E  # noqa: E402
from gae_restatement import gae_linear_fp64, gae_mlp_fp64  # noqa: E402
from policy_gradient_mlp_cases import MATRIX, net as case_net  # noqa: E402
from test_value_gradient_gpu import (G4, _check_linear, _check_mlp, _groups4, _linear_params, _make, _net4,  # noqa: E402
                                     _ratio, _same, _sampled_policy, _values, _weights, _within)
from test_value_gradient_gpu import data, dev  # noqa: E402, F401  (fixtures)
from value_gradient_restatement import _mlp_core, value_linear_fp64, value_mlp_fp64  # noqa: E402

from weather2alert_amd import _ffi, policy  # noqa: E402

pytestmark = pytest.mark.gpu

GL = [(0.99, 0.95), (0.9, 0.0)]


def _step_reference(env, sched, S):
    """`env` stepped through step() along `sched` (attempts by day of the episode) for at most S days from where it
    stands; every env is read on its own days only. Returns numpy obs f64 [S + 1, n, n_obs] (slab s: the row held before
    decision s; slab S: the row the S days leave behind), reward f64 and valid bool [S, n], alive bool [n] (not finished
    after the S days)."""
    n, dv = env.num_envs, env.device
    rows = torch.arange(n, device=dv)
    fin = env.state()["finished"].bool()
    obs = torch.zeros((S + 1, n, env._obs.shape[1]), dtype=torch.float64, device=dv)
    reward = torch.zeros((S, n), dtype=torch.float64, device=dv)
    valid = torch.zeros((S, n), dtype=torch.bool, device=dv)
    for s in range(S):
        obs[s] = env._obs.double()
        if bool(fin.all()):
            break
        t = env.state()["t"].long().clamp(max=sched.shape[1] - 1)
        valid[s] = ~fin
        res = env.step((sched[rows, t] & ~fin).to(torch.int32))
        reward[s] = torch.where(~fin, res[1].double(), torch.zeros_like(reward[s]))
        fin = fin | res[2].bool()
        obs[s + 1] = env._obs.double()
    return dict(obs=obs.cpu().numpy(), reward=reward.cpu().numpy(), valid=valid.cpu().numpy(), alive=(~fin).cpu().numpy())


def _restate(R, w, val, g, G, **kw):
    if val["kind"] == "linear":
        return gae_linear_fp64(R["obs"], R["valid"], R["reward"], R["alive"], w, val["weight"], val["bias"], g, G, **kw)
    return gae_mlp_fp64(R["obs"], R["valid"], R["reward"], R["alive"], w, val["layers"], val["activation"], g, G, **kw)


def _check_grad(out, ref, val, G, n_obs, what, empty=()):
    if val["kind"] == "linear":
        return _check_linear(out, "value_gradient", ref, G, n_obs, what)
    return _check_mlp(out, "value_gradient", ref, val["layers"], what, empty=empty)


def _rows(out, key, ref, rkey, bkey, S, what):
    x = out[key]
    assert x.dtype == torch.float32 and tuple(x.shape) == (S, ref["days"].shape[0]), (what, key)
    a = x.double().cpu().numpy()
    stepped = np.arange(S)[:, None] < ref["days"][None, :]
    assert (a[~stepped] == 0).all(), (what, key)  # exactly zero where the env does not step
    _within(a, ref[rkey], ref[bkey], what, key)


def _check_per_env(out, ref, S, what, target=False):
    assert out["sq_error"].dtype == torch.float32 and out["days"].dtype == torch.int32
    np.testing.assert_array_equal(out["days"].cpu().numpy(), ref["days"], err_msg=what)
    _within(out["sq_error"].double().cpu().numpy(), ref["sq"], ref["sq_bound"], what, "sq_error")
    if target:
        assert "return" not in out and "advantage" not in out and "value_target" not in out
    else:
        _within(out["return"].double().cpu().numpy(), ref["ret"], ref["ret_bound"], what, "return")
        _rows(out, "advantage", ref, "advantage", "adv_bound", S, what)
        _rows(out, "value_target", ref, "value_target", "vt_bound", S, what)
    gl = out["group_loss"].double().cpu().numpy()
    have = ~np.isnan(ref["group_loss"])
    assert np.isnan(gl[~have]).all(), what
    _within(gl[have], ref["group_loss"][have], ref["group_loss_bound"][have], what, "group_loss")


def _flat(out):
    pg = out["value_gradient"]
    parts = [pg["weight"], pg["bias"]] if "weight" in pg else [x for pair in pg["layers"] for x in pair]
    return parts + [out[k] for k in ("sq_error", "days", "return", "group_loss", "advantage", "value_target") if k in out]


def _grad_np(out):
    pg = out["value_gradient"]
    if "weight" in pg:
        return [np.concatenate([pg["weight"].double().cpu().numpy(), pg["bias"].double().cpu().numpy()[:, None]], axis=1)]
    return [x.double().cpu().numpy() for pair in pg["layers"] for x in pair]


def _bound_np(ref):
    if "weight" in ref:
        return [ref["bound"]]
    return [x for pair in ref["bound"] for x in pair]


def _grads_within(a, b, bounds, what, label):
    worst = 0.0
    for x, y, bd in zip(a, b, bounds):
        keep = ~np.isnan(bd)
        assert (np.isnan(x) == np.isnan(y)).all(), (what, label)
        diff = np.abs(x - y)[keep]
        worst = max(worst, _ratio(diff, bd[keep]))
        assert (diff <= bd[keep]).all(), (what, label, worst)
    print(f"{what}: max |{label}| / bound = {worst:.3e}")


def _target_shift_bound(R, w, val, g, G, shift):
    """What moving every target by at most shift[s, e] can move the gradient by: mean_e sum_s |w_e| shift_s |dV_s/dtheta|,
    with the absolute backward pass of the critic's restatement for the MLP kind. In the shapes of _bound_np()."""
    valid = R["valid"]
    S, N = valid.shape
    wa = np.abs(np.ones(N) if w is None else np.asarray(w, np.float64))
    if val["kind"] == "linear":
        o1 = np.concatenate([np.where(valid[:, :, None], R["obs"][:S], 0.0), valid[:, :, None].astype(np.float64)], axis=2)
        per_env = np.einsum("sn,snj->nj", wa[None, :] * shift, np.abs(o1))
        out = np.full((G, o1.shape[2]), np.nan)
        for k in range(G):
            if (g == k).any():
                out[k] = per_env[g == k].mean(axis=0)
        return [out]

    def coef(sel, z, M, e_z, eps):
        return np.zeros((S, int(sel.sum()))), wa[sel][None, :] * shift[:, sel]

    bounds = _mlp_core(val["layers"], val["activation"], R["obs"][:S], valid, g, G, coef)[1]
    return [x for pair in bounds for x in pair]


BASE = [("linear", 1, "hindsight"), ("linear", 3, "rollout"), ("linear", None, "hindsight"), ("linear", None, "rollout"),
        ("mlp", 1, "rollout"), ("mlp", 3, "hindsight"), ("mlp", None, "hindsight"), ("mlp", None, "rollout")]


@pytest.mark.parametrize("kind,n_steps,sched_kind", BASE)
def test_against_stepped_twin(dev, data, kind, n_steps, sched_kind):
    """300 envs (four full waves and a partial one) on the ragged table after a 25-day prefix (t0 > 0, some envs finished
    on entry), groups 0, 1 and 3 of 4 (one empty: a NaN block) in an interleaved order, weights with zeros and negative
    values, n_steps in {1, 3, the rest of the episode}; schedules from hindsight_optimum() and from a sampled rollout
    that uses up budgets; (gamma, lambda) in {(0.99, 0.95), (0.9, 0)}, bootstrap on and off. Defaults are the bits of the
    call without the new keywords, and (1, 1, no bootstrap) through the new kernels is the existing call within the sum
    of the two bounds."""
    n, name = 300, "ragged"
    ct = data[name][0]
    A, B, C_ = (_make(dev, data, name, n) for _ in range(3))
    for e_ in (A, B, C_):
        e_.rollout(_sampled_policy(ct), n_steps=25)
    fin0 = A.state()["finished"].cpu().numpy()
    assert (fin0 != 0).any() and (fin0 == 0).any()
    if sched_kind == "hindsight":
        sched = A.hindsight_optimum()["alert_days"]
    else:
        ro = C_.rollout(_sampled_policy(ct, bias=1.5, seed=7), alert_mask=True)
        assert bool((C_.state()["used"] == C_.state()["budget"]).any())  # budgets used up
        sched = ro["alert_days"]
    g, w = _groups4(n), _weights(n)
    if kind == "linear":
        W, b = _linear_params(ct, G4)
        val = dict(kind="linear", weight=W, bias=b, group=g)
    else:
        layers, act = _net4(ct, "tanh29x9")
        val = dict(kind="mlp", layers=layers, activation=act, group=g)
    S = ct.T if n_steps is None else n_steps
    R = _step_reference(B, sched, S)
    assert n_steps is None or R["alive"].any()  # a truncated chunk: bootstrap has something to do
    for gamma, lam in GL:
        for boot in (False, True):
            what = f"{kind} n_steps={n_steps} {sched_kind} gamma={gamma} lambda={lam} bootstrap={boot}"
            out = A.value_gradient(val, sched, env_weight=w, n_steps=n_steps, advantage=True, gamma=gamma, gae_lambda=lam,
                                   bootstrap=boot, value_target=True)
            assert A.check_status() == 0
            ref = _restate(R, w, val, g, G4, gamma=gamma, lam=lam, bootstrap=boot)
            _check_grad(out, ref, val, G4, ct.n_obs, what, empty=(2,))
            _check_per_env(out, ref, S, what)
    # defaults: the call without the new keywords, bit for bit
    old = A.value_gradient(val, sched, env_weight=w, n_steps=n_steps, advantage=True)
    dflt = A.value_gradient(val, sched, env_weight=w, n_steps=n_steps, advantage=True, gamma=1.0, gae_lambda=1.0,
                            bootstrap=False, value_target=False, target=None)
    assert set(old) == set(dflt) and "value_target" not in dflt
    for x, y in zip(_flat(old), _flat(dflt)):
        assert _same(x, y)
    # (1, 1, bootstrap=False) through the new kernels (value_target=True forces the route) against the existing call
    what = f"{kind} n_steps={n_steps} {sched_kind} (1, 1) new route"
    new = A.value_gradient(val, sched, env_weight=w, n_steps=n_steps, advantage=True, value_target=True)
    ref = _restate(R, w, val, g, G4)
    _check_grad(new, ref, val, G4, ct.n_obs, what, empty=(2,))
    _check_per_env(new, ref, S, what)
    if kind == "linear":
        ref_old = value_linear_fp64(R["obs"], R["valid"], R["reward"], w, W, b, g, G4)
    else:
        ref_old = value_mlp_fp64(R["obs"], R["valid"], R["reward"], w, layers, act, g, G4)
    _grads_within(_grad_np(new), _grad_np(old), [x + y for x, y in zip(_bound_np(ref), _bound_np(ref_old))], what,
                  "new route - existing call")
    for key, bn, bo in (("advantage", "adv_bound", "adv_bound"), ("sq_error", "sq_bound", "sq_bound"),
                        ("return", "ret_bound", "ret_bound")):
        _within(new[key].double().cpu().numpy(), old[key].double().cpu().numpy(), ref[bn] + ref_old[bo], what, key)
    assert torch.equal(new["days"], old["days"])
    for e_ in (A, B, C_):
        e_.close()


@pytest.mark.parametrize("net", list(MATRIX))
def test_mlp_every_instantiation_against_stepped_twin(dev, data, net):
    """The six <WIDTH, LAYERS> instantiations of k_gae_pass1 / k_pgm_pass2 with the nets of
    tests/policy_gradient_mlp_cases.py: 193 envs, G = 5 interleaved groups, a 9-day prefix, a 40-day chunk that every
    env outlives (the extra logit call of the bootstrap), a random schedule with attempts over budget; then fixed targets
    on the same instantiation."""
    pair, hidden, act, n_out = MATRIX[net]
    assert (policy.mlp_width(hidden), len(hidden)) == pair
    n, S = 193, 40
    ct = data["synth"][0]
    A, B = _make(dev, data, "synth", n), _make(dev, data, "synth", n)
    for e_ in (A, B):
        e_.rollout(_sampled_policy(ct), n_steps=9)
    g = E.groups(n)
    layers = case_net(ct, net, hidden, n_out)
    val = dict(kind="mlp", layers=layers, activation=act, group=g)
    sched = torch.as_tensor(np.random.default_rng(21).random((n, ct.T)) < 0.35, device=dev)
    w = _weights(n)
    out = A.value_gradient(val, sched, env_weight=w, n_steps=S, advantage=True, gamma=0.99, gae_lambda=0.95,
                           bootstrap=True, value_target=True)
    assert A.check_status() == 0
    R = _step_reference(B, sched, S)
    assert R["alive"].all()
    ref = _restate(R, w, val, g, E.G, gamma=0.99, lam=0.95, bootstrap=True)
    assert ref["near_kink"] < 0.01
    what = f"<{pair[0]}, {pair[1]}> {net}"
    _check_grad(out, ref, val, E.G, ct.n_obs, what)
    _check_per_env(out, ref, S, what)
    tg = np.random.default_rng(6).standard_normal((S + 2, n)).astype(np.float32)
    out_t = A.value_gradient(val, sched, env_weight=w, n_steps=S, target=torch.as_tensor(tg, device=dev))
    ref_t = _restate(R, w, val, g, E.G, target=tg)
    _check_grad(out_t, ref_t, val, E.G, ct.n_obs, what + " target")
    _check_per_env(out_t, ref_t, S, what + " target", target=True)
    A.close()
    B.close()


EDGES = [("ragged", "linear", None), ("ragged", "tanh7x13", None), ("ragged27", "linear", 30), ("slot27", "relu33", None),
         ("slot27", "linear", 30), ("n8", "linear", None), ("n8", "tanh7x13", 30)]


@pytest.mark.parametrize("name,kind,n_steps", EDGES)
def test_table_edges_and_another_layout(dev, data, name, kind, n_steps):
    """The ragged table from a fresh reset (episode lengths 1, 2 and 3 inside one wave: where the backward sweep
    starts), ragged lengths with slot-27 coefficient rows, a slot-27 table, and the n8 layout of tests/obs_layouts.py:
    65 envs, G = 1 without an order, no weights, both (gamma, lambda) with the bootstrap on; then fixed targets."""
    n = 65
    ct = data[name][0]
    A, B = _make(dev, data, name, n), _make(dev, data, name, n)
    if name == "ragged":  # the shortest episodes and the full-length one, six envs each, at the head of the first wave
        rng = np.random.default_rng(21)
        col = rng.integers(0, ct.S, n)
        cw, yi = np.asarray(ct.fips_to_weather)[col].astype(np.int64), rng.integers(0, ct.Y, n)
        nd_tab = np.asarray(ct.n_days).reshape(-1, ct.Y)
        pairs = [tuple(p) for d in E.SHORTEST + (ct.T,) for p in np.argwhere(nd_tab == d)[:1]]
        for i in range(24):
            cw[i], yi[i] = pairs[i % 4]
        ep = dict(county_w=cw, year_i=yi, coef_col=col, sample=rng.integers(0, ct.n_samples, n),
                  budget=np.where(np.arange(n) % 3 == 0, 0, 12))
        for e_ in (A, B):
            e_.reset(options={"episodes": ep})
    sched = torch.as_tensor(np.random.default_rng(21).random((n, ct.T)) < 0.35, device=dev)
    S = ct.T if n_steps is None else n_steps
    if kind == "linear":
        W, b = _linear_params(ct, 1)
        val = dict(kind="linear", weight=W, bias=b)
    else:
        _, hidden, act, n_out = MATRIX[kind]
        val = dict(kind="mlp", layers=[(W[:1], b[:1]) for W, b in case_net(ct, kind, hidden, n_out)], activation=act)
    R = _step_reference(B, sched, S)
    if name == "ragged":
        lengths = R["valid"].sum(axis=0)
        assert {1, 2, 3, ct.T} <= set(lengths[:64].tolist())
    for gamma, lam in GL:
        what = f"{name} {kind} n_steps={n_steps} gamma={gamma} lambda={lam}"
        out = A.value_gradient(val, sched, n_steps=n_steps, advantage=True, gamma=gamma, gae_lambda=lam, bootstrap=True,
                               value_target=True)
        ref = _restate(R, None, val, None, 1, gamma=gamma, lam=lam, bootstrap=True)
        _check_grad(out, ref, val, 1, ct.n_obs, what)
        _check_per_env(out, ref, S, what)
    tg = np.random.default_rng(6).standard_normal((S, n)).astype(np.float32)
    out_t = A.value_gradient(val, sched, n_steps=n_steps, target=torch.as_tensor(tg, device=dev))
    ref_t = _restate(R, None, val, None, 1, target=tg)
    _check_grad(out_t, ref_t, val, 1, ct.n_obs, f"{name} {kind} target")
    _check_per_env(out_t, ref_t, S, f"{name} {kind} target", target=True)
    A.close()
    B.close()


@pytest.mark.parametrize("kind", ["linear", "mlp"])
def test_chunks_with_a_bootstrap_are_the_whole_call(dev, data, kind):
    """The test of `bootstrap`. With gae_lambda = 0, A_s needs day s and the row after it alone, so with bootstrap=True a
    call with n_steps = 3 gives the first three advantage rows of the whole-episode call, and after stepping the env
    three days along the schedule a second call gives rows 3..5: each within the restatement's bound of a 7-day run of
    the twin, and chunk against whole within twice that bound. Without the bootstrap rows 2 and 5 leave it."""
    n, gamma = 193, 0.9
    ct = data["synth"][0]
    A, B = _make(dev, data, "synth", n), _make(dev, data, "synth", n)
    for e_ in (A, B):
        e_.rollout(_sampled_policy(ct), n_steps=9)
    g = np.arange(n) % 3
    val = _values(ct, g)[kind]
    sched = torch.as_tensor(np.random.default_rng(21).random((n, ct.T)) < 0.35, device=dev)
    kw = dict(advantage=True, gamma=gamma, gae_lambda=0.0)
    whole = A.value_gradient(val, sched, bootstrap=True, **kw)["advantage"].double().cpu().numpy()
    first = A.value_gradient(val, sched, n_steps=3, bootstrap=True, **kw)["advantage"].double().cpu().numpy()
    cut = A.value_gradient(val, sched, n_steps=3, **kw)["advantage"].double().cpu().numpy()
    rows = torch.arange(n, device=dev)
    for _ in range(3):
        t = A.state()["t"].long().clamp(max=ct.T - 1)
        A.step(sched[rows, t].to(torch.int32))
    second = A.value_gradient(val, sched, n_steps=3, bootstrap=True, **kw)["advantage"].double().cpu().numpy()
    R = _step_reference(B, sched, 7)
    assert R["valid"].all()
    ref = _restate(R, None, val, g, 3, gamma=gamma, lam=0.0, bootstrap=True)
    what = f"chunks {kind}"
    bd = ref["adv_bound"][:6]
    _within(whole[:6], ref["advantage"][:6], bd, what, "whole[0:6]")
    _within(first, ref["advantage"][:3], bd[:3], what, "chunk 1")
    _within(second, ref["advantage"][3:6], bd[3:6], what, "chunk 2")
    _within(first, whole[:3], 2 * bd[:3], what, "chunk 1 vs whole")
    _within(second, whole[3:6], 2 * bd[3:6], what, "chunk 2 vs whole")
    assert (np.abs(cut[:2] - whole[:2]) <= 2 * bd[:2]).all() and (np.abs(cut[2] - whole[2]) > 2 * bd[2]).any()
    A.close()
    B.close()


@pytest.mark.parametrize("kind", ["linear", "mlp"])
def test_fixed_targets_reproduce_the_first_call(dev, data, kind):
    """target= with the first call's "value_target" reproduces its gradient and squared error within the sum of the two
    bounds, and matches the restatement on those targets; the same targets on a reward_mode="posterior_mean" env from the
    same seed (no reward is needed) give the same bits."""
    n, S = 193, 60
    ct = data["synth"][0]
    A, B, P = _make(dev, data, "synth", n), _make(dev, data, "synth", n), _make(dev, data, "synth", n, reward_mode="posterior_mean")
    sched = torch.as_tensor(np.random.default_rng(21).random((n, ct.T)) < 0.35, device=dev)
    for e_ in (A, B, P):
        for _ in range(3):
            e_.step(sched[:, 0].to(torch.int32))
    g = np.arange(n) % 3
    val = _values(ct, g)[kind]
    w = _weights(n)
    first = A.value_gradient(val, sched, env_weight=w, n_steps=S, gamma=0.99, gae_lambda=0.95, bootstrap=True,
                             value_target=True)
    again = A.value_gradient(val, sched, env_weight=w, n_steps=S, target=first["value_target"])
    R = _step_reference(B, sched, S)
    ref1 = _restate(R, w, val, g, 3, gamma=0.99, lam=0.95, bootstrap=True)
    ref2 = _restate(R, w, val, g, 3, target=first["value_target"].cpu().numpy())
    what = f"targets {kind}"
    _check_grad(again, ref2, val, 3, ct.n_obs, what)
    _check_per_env(again, ref2, S, what, target=True)
    # again - first = (again - ref2) + (ref2 - ref1) + (ref1 - first). The gradient is linear in the targets, and the ones
    # handed over are within ref1's vt_bound of ref1's own: the middle term is at most that bound carried through |dV/dtheta|
    middle = _target_shift_bound(R, w, val, g, 3, ref1["vt_bound"])
    _grads_within(_grad_np(again), _grad_np(first), [x + y + m for x, y, m in zip(_bound_np(ref1), _bound_np(ref2), middle)],
                  what, "target= - first call")
    with pytest.raises(ValueError):
        P.value_gradient(val, sched, n_steps=S)
    pm = P.value_gradient(val, sched, env_weight=w, n_steps=S, target=first["value_target"])
    assert set(pm) == set(again)
    for x, y in zip(_flat(pm), _flat(again)):
        assert _same(x, y)
    for e_ in (A, B, P):
        e_.close()


@pytest.mark.parametrize("kind", ["linear", "mlp"])
def test_no_side_effects_and_identical_bits(dev, data, kind):
    """Two identical calls return identical bits, for the estimator and for fixed targets; state(), the observation
    buffer and a subsequent sampled rollout() (the RNG) are bit-identical to those of a twin that never made the call."""
    ct = data["synth"][0]
    n = 193
    A, B = _make(dev, data, "synth", n), _make(dev, data, "synth", n)
    g = np.arange(n) % 3
    val = _values(ct, g)[kind]
    sched = torch.as_tensor(np.random.default_rng(21).random((n, ct.T)) < 0.35, device=dev)
    sched0 = sched.clone()
    w = _weights(n)
    for e_ in (A, B):
        for _ in range(3):
            e_.step(sched[:, 0].to(torch.int32))
    kw = dict(env_weight=w, advantage=True, gamma=0.99, gae_lambda=0.95, bootstrap=True, value_target=True, n_steps=50)
    o1 = A.value_gradient(val, sched, **kw)
    o2 = A.value_gradient(val, sched, **kw)
    t1 = A.value_gradient(val, sched, env_weight=w, n_steps=50, target=o1["value_target"])
    t2 = A.value_gradient(val, sched, env_weight=w, n_steps=50, target=o1["value_target"])
    for a_, b_ in ((o1, o2), (t1, t2)):
        assert set(a_) == set(b_)
        for x, y in zip(_flat(a_), _flat(b_)):
            assert _same(x, y)
    sa, sb = A.state(), B.state()
    for k in sb:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(A._obs, B._obs) and torch.equal(sched, sched0) and A.check_status() == 0
    roll = dict(_values(ct, g)["linear"], sample=True, seed=6)
    ra, rb_ = A.rollout(roll, alert_mask=True), B.rollout(roll, alert_mask=True)
    for k, v in rb_.items():
        assert _same(ra[k], v), k
    A.close()
    B.close()


def test_linear_per_env_outputs_do_not_depend_on_groups_or_order(dev, data):
    """sq_error, return, days, advantage and value_target of an env are the same bits with one group or three that share
    a parameter row, and with the handle's feature-row visiting order set or unset."""
    ct = data["synth"][0]
    n = 193
    W, b = _linear_params(ct, 1)
    sched = torch.as_tensor(np.random.default_rng(21).random((n, ct.T)) < 0.35, device=dev)
    outs = []
    for kw, G in (({}, 1), ({}, 3), (dict(lockstep=False, rollout_order=True), 1)):
        env = _make(dev, data, "synth", n, **kw)
        env.rollout(_sampled_policy(ct), n_steps=9)
        val = dict(kind="linear", weight=np.repeat(W, G, axis=0), bias=np.repeat(b, G))
        if G > 1:
            val["group"] = np.arange(n) % G
        outs.append(env.value_gradient(val, sched, n_steps=60, advantage=True, gamma=0.99, gae_lambda=0.95, bootstrap=True,
                                       value_target=True))
        env.close()
    for o in outs[1:]:
        for k in ("sq_error", "return", "days", "advantage", "value_target"):
            assert torch.equal(o[k], outs[0][k]), k
    for x, y in zip(_flat(outs[0])[:2], _flat(outs[2])[:2]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("kind", ["linear", "mlp"])
def test_nothing_is_written_past_the_workspace(dev, data, kind):
    """The entry points through the C ABI on a buffer filled with 0xA5, the true workspace size passed: the bytes behind
    it keep the pattern, and the outputs are the bits of the Python call."""
    ct = data["synth"][0]
    n, S = 193, 17
    env = _make(dev, data, "synth", n)
    g = np.arange(n) % 3
    val = _values(ct, g)[kind]
    sched = torch.as_tensor(np.random.default_rng(21).random((n, ct.T)) < 0.35, device=dev)
    want = env.value_gradient(val, sched, n_steps=S, advantage=True, gamma=0.99, gae_lambda=0.95, bootstrap=True,
                              value_target=True)
    lib = env._lib
    mask = policy.check_value_args(kind, sched, None, S, n, ct.T, dev)[0]
    outs = dict(sq=torch.zeros(n, device=dev), days=torch.zeros(n, dtype=torch.int32, device=dev), ret=torch.zeros(n, device=dev),
                adv=torch.full((S, n), 7.0, device=dev), vt=torch.full((S, n), 7.0, device=dev))
    tail = (0.99, 0.95, 1, outs["vt"].data_ptr(), None, 0)
    with torch.cuda.device(dev):
        if kind == "linear":
            a = policy.check_linear_policy(val, ct.n_obs, n, ct.obs_slot, dev)
            lp = _ffi.LinearPolicy()
            lp.weight, lp.bias, lp.group, lp.n_groups = a.weight_slots.data_ptr(), a.bias.data_ptr(), a.group.data_ptr(), a.n_groups
            wsb = lib.w2a_value_gradient_linear_gae_workspace_bytes(n, S)
            buf = torch.full((wsb + 65536,), 0xA5, dtype=torch.uint8, device=dev)
            grad = torch.zeros((ct.n_obs + 1, n), device=dev)
            rc = lib.w2a_value_gradient_linear_gae(env._h, C.byref(lp), mask.data_ptr(), mask.shape[1], None, S,
                                                   env._obs.data_ptr(), grad.data_ptr(), outs["sq"].data_ptr(),
                                                   outs["days"].data_ptr(), outs["ret"].data_ptr(), outs["adv"].data_ptr(),
                                                   *tail, buf.data_ptr(), wsb, env._stream())
        else:
            a = policy.check_mlp_policy(val, ct.n_obs, n, ct.obs_slot, dev)
            mp = _ffi.MlpPolicy()
            order = a.order if a.group_major else policy.group_order(a.group)
            mp.params, mp.group, mp.order = a.params.data_ptr(), a.group.data_ptr(), order.data_ptr()
            mp.n_groups, mp.n_layers, mp.width, mp.activation = a.n_groups, a.n_layers, a.width, _ffi.MLP_ACTIVATIONS[a.activation]
            wsb = lib.w2a_value_gradient_mlp_gae_workspace_bytes(n, S, a.n_groups, a.width, a.n_layers)
            buf = torch.full((wsb + 65536,), 0xA5, dtype=torch.uint8, device=dev)
            grad = torch.zeros((a.n_groups, policy.mlp_stride(a.width, a.n_layers)), device=dev)
            rc = lib.w2a_value_gradient_mlp_gae(env._h, C.byref(mp), mask.data_ptr(), mask.shape[1], None, S,
                                                env._obs.data_ptr(), grad.data_ptr(), outs["sq"].data_ptr(),
                                                outs["days"].data_ptr(), outs["ret"].data_ptr(), outs["adv"].data_ptr(),
                                                *tail, buf.data_ptr(), wsb, env._stream())
        torch.cuda.synchronize()
    assert rc == 0, lib.w2a_last_error()
    assert buf.data_ptr() % 256 == 0 and bool((buf[wsb:] == 0xA5).all())
    for k, key in (("sq", "sq_error"), ("days", "days"), ("ret", "return"), ("adv", "advantage"), ("vt", "value_target")):
        assert torch.equal(outs[k], want[key]), key
    assert env.check_status() == 0
    env.close()


def test_refusals(dev, data):
    """Bad values of the new arguments are ValueErrors before anything runs: the state is untouched. reward_mode and the
    semantics are refused as before unless targets are given; other semantics stay refused with them."""
    ct = data["synth"][0]
    n = 65
    env = _make(dev, data, "synth", n)
    W, b = _linear_params(ct, 1)
    lin = dict(kind="linear", weight=W, bias=b)
    sched = torch.as_tensor(np.random.default_rng(21).random((n, ct.T)) < 0.35, device=dev)
    before = {k: v.clone() for k, v in env.state().items()}
    obs_before = env._obs.clone()
    tg = torch.zeros((3, n), device=dev)
    bad = [dict(gamma=-0.1), dict(gamma=1.1), dict(gamma=float("nan")), dict(gae_lambda=1.5), dict(gae_lambda=float("inf")),
           dict(bootstrap=1), dict(value_target=1), dict(target=tg[:2]), dict(target=torch.zeros((3, n + 1), device=dev)),
           dict(target=tg.to(torch.int32)), dict(target=tg * float("nan")), dict(target=tg, advantage=True),
           dict(target=tg, value_target=True), dict(target=tg, gamma=0.9), dict(target=tg, gae_lambda=0.9),
           dict(target=tg, bootstrap=True), dict(gamma=0.9, env_weight=np.full(n, np.nan))]
    for kw in bad:
        with pytest.raises(ValueError):
            env.value_gradient(lin, sched, n_steps=3, **kw)
    for k_, v in env.state().items():
        assert torch.equal(v, before[k_]), k_
    assert torch.equal(env._obs, obs_before)
    out = env.value_gradient(lin, sched, n_steps=3, target=torch.zeros((5, n), device=dev))  # more days than the call runs
    assert "return" not in out and set(out) == {"value_gradient", "sq_error", "days", "group_loss"}
    env.load_state_dict(env.state_dict())
    with pytest.raises(RuntimeError):
        env.value_gradient(lin, sched, gamma=0.9)
    env.close()
    fx = _make(dev, data, "synth", n, fixes=["lag"])
    for kw in (dict(gamma=0.9), dict(target=tg)):
        with pytest.raises(ValueError):
            fx.value_gradient(lin, sched, n_steps=3, **kw)
    fx.close()
