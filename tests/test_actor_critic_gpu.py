"""actor_critic_gradient() (k_ac_pass1 / k_ac_finish / k_ac_pass2 and the count, scan and reduce kernels of
w2a_policy_gradient_mlp) against the fp64 restatement (tests/actor_critic_restatement.py) and against the existing
one-head kernels. The reference never touches the kernels under test: an identical twin from the same seed is stepped day
by day through step() with the schedule's actions (a forced day attempted as 0) and its rows, rewards and flags go to the
restatement. Every comparison requires |got - ref| <= bound for every component of the gradient, every per-env output
and "group_objective", "days" equal and "clipped_days" within the restatement's tolerance, NaN exactly for the empty
group, ambiguity shares under AMBIGUOUS_CAP and a case that is not trivial, and prints the largest ratio to the bound.
The cases are those of tests/actor_critic_cases.py (tests/test_actor_critic_cpu.py replays them with the NumPy oracle):
300 envs (four full waves and a partial one), groups 0, 1 and 3 of 4 with group 2 empty, and the six instantiations
again at 3 tiles per wave."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import actor_critic_cases as AC  # noqa: E402
import q_gradient_cases as QC  # noqa: E402
from actor_critic_restatement import AMBIGUOUS_CAP  # noqa: E402

from weather2alert_amd import _ffi, policy  # noqa: E402

pytestmark = pytest.mark.gpu

ORDER = dict(lockstep=False, rollout_order=True)  # the handle's visiting order: not the identity
GID0 = AC.GID0
HAVE = np.array([0, 1, 3])  # the groups that hold envs
PER_ENV = (("surrogate", "L"), ("approx_kl", "kl"), ("entropy", "H"), ("value_loss", "vl"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tabs():
    return AC.make_tables()


def _make(dev, tabs, c, n, gid0=GID0):
    """a fresh env of the case's table, reset, and walked through the days before the call"""
    from weather2alert_amd import HeatAlertVecEnv

    cfg = AC.RESET[c["table"]]
    env = HeatAlertVecEnv(n, tables=tabs[c["table"]].ct, device=dev, autoreset="disabled", env_gid0=gid0,
                          similar_climate_counties=True, **(ORDER if c["order"] else {}))
    env.reset(seed=cfg["seed"], options=dict(cfg["opts"]))
    for day in range(c["prefix"]):
        env.step(torch.as_tensor(QC.prefix_actions(n, day, gid0), device=dev))
    env.check_status()  # on the ragged tables the prefix steps envs past their last day: read, and so cleared, here
    return env


def _twin_rows(env, c, sched, allowed, S):
    """`env` stepped through step() along `sched` (a forced day attempted as 0) for at most S days from where it stands,
    every env read on its own days only: the arrays of actor_critic_cases.oracle_rows"""
    n, dv, T = env.num_envs, env.device, sched.shape[1]
    rows = torch.arange(n, device=dv)
    fin = env.state()["finished"].bool()
    R = dict(obs=torch.zeros((S + 1, n, env._obs.shape[1]), dtype=torch.float64, device=dv),
             reward=torch.zeros((S, n), dtype=torch.float64, device=dv),
             **{k: torch.zeros((S, n), dtype=torch.bool, device=dv) for k in ("valid", "labels", "forced", "issued", "terminal")})
    for s in range(S):
        st = env.state()
        tt = st["t"].long().clamp(max=T - 1)
        R["obs"][s] = env._obs.double()
        R["valid"][s] = ~fin
        R["labels"][s] = sched[rows, tt] & ~fin
        forced = torch.zeros(n, dtype=torch.bool, device=dv) if allowed is None else ~allowed[rows, tt]
        if c["rb"]:
            forced = forced | ((st["budget"] - st["used"]) <= 0)
        R["forced"][s] = forced & ~fin
        res = env.step((R["labels"][s] & ~R["forced"][s]).to(torch.int32))
        R["issued"][s] = (env.state()["used"] > st["used"]) & ~fin
        R["reward"][s] = torch.where(~fin, res[1].double(), torch.zeros_like(R["reward"][s]))
        R["terminal"][s] = res[2].bool() & ~fin
        fin = fin | res[2].bool()
    R["obs"][S] = env._obs.double()
    return {k: v.cpu().numpy() for k, v in R.items()}


def _ratio(diff, bound):
    return float(np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff > 0, np.inf, 0.0)).max())


def _call(env, c, net, sched, w, inputs=None, **extra):
    kw = dict(clip=c["clip"], vf_coef=c["vf_coef"], entropy_coef=c["beta"], env_weight=w, n_steps=c["n_steps"])
    if inputs is None:
        kw.update(gamma=c["gamma"], gae_lambda=c["lam"], bootstrap=c["bootstrap"])
    else:
        kw.update(advantage=inputs[0], value_target=inputs[1], old_log_prob=inputs[2])
    kw.update(extra)
    return env.actor_critic_gradient(net, sched, **kw)


def _check(out, ref, c, R, what, groups=None, envs=slice(None), rows=True):
    """every component within its bound (groups: the rows of the gradient to compare with the reference's; envs: the
    slice of the per-env outputs the reference covers); returns the largest ratio to the bound"""
    assert ref["ambiguous_share"] + ref["near_kink"] + ref["near_tie"] <= AMBIGUOUS_CAP, (what, ref["ambiguous_share"])
    worst = {"gradient": 0.0}
    for (dW, db), (rW, rb), (bW, bb) in zip(out["gradient"]["layers"], ref["layers"], ref["bound"]):
        for got, want, bound in ((dW, rW, bW), (db, rb, bb)):
            assert got.dtype == torch.float32
            got = got.double().cpu().numpy()
            got = got if groups is None else got[groups]
            assert got.shape == want.shape, (what, got.shape, want.shape)
            empty = np.isnan(want)
            assert np.isnan(got[empty]).all() and np.isfinite(got[~empty]).all(), what  # NaN exactly for the empty group
            diff = np.abs(got - want)[~empty]
            worst["gradient"] = max(worst["gradient"], _ratio(diff, bound[~empty]))
            assert (diff <= bound[~empty]).all(), (what, "gradient", worst)
    np.testing.assert_array_equal(out["days"].cpu().numpy()[envs], ref["days"], err_msg=str(what))
    dc = np.abs(out["clipped_days"].cpu().numpy()[envs].astype(np.int64) - ref["clipped"])
    assert (dc <= ref["clipped_tol"]).all(), (what, "clipped_days")
    keys = PER_ENV + ((("return", "ret"),) if "return" in out else ())
    for key, name in keys:
        assert out[key].dtype == torch.float32
        diff = np.abs(out[key].double().cpu().numpy()[envs] - ref[name])
        worst[key] = _ratio(diff, ref[name + "_bound"])
        assert (diff <= ref[name + "_bound"]).all(), (what, key, worst)
    if rows and "advantage" in out:
        S = ref["advantage"].shape[0]
        for key, name, bname, on in (("advantage", "advantage", "adv_bound", R["valid"]),
                                     ("value_target", "value_target", "vt_bound", R["valid"]),
                                     ("log_prob", "lp", "lp_bound", ref["m"])):
            got = out[key].double().cpu().numpy()[:, envs]
            assert out[key].dtype == torch.float32 and got.shape[0] >= S
            assert (got[:S][~on] == 0).all() and (got[S:] == 0).all(), (what, key)  # zero where nothing is formed
            diff = np.abs(got[:S] - ref[name])
            worst[key] = _ratio(diff, ref[bname])
            assert (diff <= ref[bname]).all(), (what, key, worst)
    if groups is None:
        go = out["group_objective"].double().cpu().numpy()
        have = ~np.isnan(ref["group_objective"])
        assert go.shape == have.shape and np.isnan(go[~have]).all() and np.isfinite(go[have]).all(), what
        diff = np.abs(go - ref["group_objective"])[have]
        worst["group_objective"] = _ratio(diff, ref["group_objective_bound"][have])
        assert (diff <= ref["group_objective_bound"][have]).all(), (what, "group_objective", worst)
    AC.not_trivial(c, R, ref, what)
    print(f"{what}: ratio to the bound " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items())
          + f"; ambiguous {ref['ambiguous_share']:.2e}, near_kink {ref['near_kink']:.2e}, scored days "
          f"{int(ref['days'].sum())} of {int(ref['stepped'].sum())}, clipped {int(ref['clipped'].sum())}")
    return max(worst.values())


def _same_bits(a, b, keys):
    for key in keys:
        assert torch.equal(a[key].nan_to_num(7.0), b[key].nan_to_num(7.0)), key
    for (dW, db), (dW2, db2) in zip(a["gradient"]["layers"], b["gradient"]["layers"]):
        assert torch.equal(dW.nan_to_num(7.0), dW2.nan_to_num(7.0)) and torch.equal(db.nan_to_num(7.0), db2.nan_to_num(7.0))


def _setup(dev, tabs, c, n=None, gid0=GID0):
    tb = tabs[c["table"]]
    ct = tb.ct
    n = c["n"] if n is None else n
    sched = torch.as_tensor(AC.schedule(tb, c, n, gid0), device=dev)
    allowed = torch.as_tensor(AC.gate(n, ct.T, gid0), device=dev) if c["gate"] else None
    return tb, ct, n, sched, allowed


def _t(inputs, dev):
    return None if inputs is None else tuple(torch.as_tensor(x, device=dev) for x in inputs)


@pytest.mark.parametrize("name", list(AC.CASES))
def test_against_stepped_twin(dev, tabs, name):
    """Tests 1, 6 and 8 of the feature's list at 1 tile per wave: both modes, the six instantiations with padded units
    under tanh and ReLU, the mini and ragged tables and the n_obs = 8 layouts, gated and at-budget cases (the policy
    coefficient absent and the value term present on forced days: actor_critic_cases.not_trivial holds the reference to
    that, the bound holds the kernel to the reference), chunks with and without the bootstrap, weights with zeros and
    negatives and none, the identity visiting order and the handle's own. No side effects, identical bits."""
    c = AC.case(name)
    tb, ct, n, sched, allowed = _setup(dev, tabs, c)
    A, B = _make(dev, tabs, c, n), _make(dev, tabs, c, n)
    grouped = c["grouped"]
    g = QC.groups(n) if grouped else None
    layers = AC.net(ct, c, AC.G if grouped else 1)
    w = QC.weights(n) if c["weights"] else None
    S = AC.steps(ct, c)
    inputs = AC.epoch_inputs(S, n) if c["mode"] == "epoch" else None
    net = AC.policy_dict(layers, c, g, allowed)
    before = {k: v.clone() for k, v in A.state().items()}
    obs0 = A._obs.clone()
    out, again = _call(A, c, net, sched, w, _t(inputs, dev)), _call(A, c, net, sched, w, _t(inputs, dev))
    assert A.check_status() == 0 and torch.equal(obs0, A._obs)
    for k, v in A.state().items():
        assert torch.equal(v, before[k]), k
    _same_bits(out, again, [k for k in out if k != "gradient"])  # identical calls, identical bits
    assert set(out) == set(again) and ("return" in out) == ("advantage" in out) == (inputs is None)
    assert [(tuple(a.shape), tuple(b.shape)) for a, b in out["gradient"]["layers"]] == \
        [((AC.G if grouped else 1,) + W.shape[1:], (AC.G if grouped else 1,) + b.shape[1:]) for W, b in layers]
    R = _twin_rows(B, c, sched, allowed, S)
    ref = AC.restate(c, R, w, layers, g, AC.G if grouped else None, inputs)
    _check(out, ref, c, R, f"<{AC.INSTANTIATION[c['net']][0]}, {AC.INSTANTIATION[c['net']][1]}> {name}")
    if c["table"] == "ragged":  # envs finished on entry: nothing is scored, nothing is lost
        fin = ~R["valid"][0]
        assert fin.any() and (~fin).any()
        assert (out["value_loss"].cpu().numpy()[fin] == 0).all() and (out["days"].cpu().numpy()[fin] == 0).all()
    A.close()
    B.close()


@pytest.mark.parametrize("name", list(AC.LARGE))
def test_three_tiles_per_wave(dev, tabs, name):
    """131 272 envs on the 12-day table: 2 052 tiles, 3 per wave of the second pass, groups of 1 000 consecutive env ids.
    The six instantiations, collect and epoch alternating. Finite everywhere; three groups rebuilt as small batches with
    the same global env ids and stepped through step() lie inside the bound."""
    c = AC.case(name)
    tb, ct, n, sched, _ = _setup(dev, tabs, c)
    n_groups = (n + QC.GROUP_SIZE - 1) // QC.GROUP_SIZE
    assert ((n + 63) // 64 + 1023) // 1024 == 3  # tiles per wave of pass 2 (csrc/w2a_policy_dispatch.hip.h: pgm_layout)
    g = np.arange(n) // QC.GROUP_SIZE
    big = QC.scaled(AC.net(ct, c, 1), n_groups, 10)
    w = QC.weights(n)
    inputs = AC.epoch_inputs(ct.T, n) if c["mode"] == "epoch" else None
    A = _make(dev, tabs, c, n)
    out = _call(A, c, AC.policy_dict(big, c, g), sched, w, _t(inputs, dev))
    assert A.check_status() == 0
    assert all(bool(torch.isfinite(dW).all()) and bool(torch.isfinite(db).all()) for dW, db in out["gradient"]["layers"])
    A.close()
    for k in QC.CHECKED:
        lo = k * QC.GROUP_SIZE
        nk = min(QC.GROUP_SIZE, n - lo)
        B = _make(dev, tabs, c, nk, GID0 + lo)
        sk = torch.as_tensor(AC.schedule(tb, c, nk, GID0 + lo), device=dev)
        assert torch.equal(sk, sched[lo:lo + nk])
        R = _twin_rows(B, c, sk, None, ct.T)
        B.close()
        ref = AC.restate(c, R, w[lo:lo + nk], [(W[k:k + 1], b[k:k + 1]) for W, b in big], None, None,
                         None if inputs is None else AC.epoch_inputs(ct.T, n, lo, nk))
        _check(out, ref, c, R, f"3 tiles per wave <{AC.INSTANTIATION[c['net']][0]}, {AC.INSTANTIATION[c['net']][1]}> {name}, "
               f"group {k} ({nk} envs)", groups=slice(k, k + 1), envs=slice(lo, lo + nk))


def _one_head(layers, row, c, g, allowed=None):
    return AC.policy_dict(layers[:-1] + [(layers[-1][0][:, row:row + 1], layers[-1][1][:, row:row + 1])], c, g, allowed)


@pytest.mark.parametrize("net,act,kw", [("h7", "relu", dict(gamma=0.97, lam=0.9)),
                                        ("h24x20", "tanh", dict(gamma=0.9, lam=0.8, n_steps=40, bootstrap=True, rb=True)),
                                        ("h64x64", "tanh", dict(gamma=1.0, lam=1.0, gate=True))])
def test_collect_outputs_are_the_one_head_kernels_bits(dev, tabs, net, act, kw):
    """Tests 2 and 9: "advantage" and "value_target" equal value_gradient() of the one-head net (trunk + row 1) with the
    same gamma, gae_lambda and bootstrap bit for bit, "log_prob" equals surrogate_gradient(log_prob=True) of the one-head
    net (trunk + row 0) bit for bit, and gradient=False returns the same three arrays and no "gradient"."""
    c = dict(AC.DEFAULT, net=net, act=act, **kw)
    tb, ct, n, sched, allowed = _setup(dev, tabs, c)
    A = _make(dev, tabs, c, n)
    g = QC.groups(n)
    layers = AC.net(ct, c, AC.G)
    out = _call(A, c, AC.policy_dict(layers, c, g, allowed), sched, None)
    crit = A.value_gradient(_one_head(layers, 1, dict(c, rb=False), g), sched, n_steps=c["n_steps"], advantage=True,
                            value_target=True, gamma=c["gamma"], gae_lambda=c["lam"], bootstrap=c["bootstrap"])
    if not c["gate"]:  # the critic takes no gate: a closed day changes the alerts issued, and so the rows
        assert torch.equal(out["advantage"], crit["advantage"]) and torch.equal(out["value_target"], crit["value_target"])
        assert torch.equal(out["return"], crit["return"]) and bool((out["advantage"] != 0).any())
    act_ = A.surrogate_gradient(_one_head(layers, 0, c, g, allowed), sched, torch.zeros_like(out["advantage"]),
                                n_steps=c["n_steps"], log_prob=True)
    assert torch.equal(out["log_prob"], act_["log_prob"]) and bool((out["log_prob"] != 0).any())
    assert torch.equal(out["days"], act_["days"]) and bool((out["log_prob"] == 0).any())
    bare = _call(A, c, AC.policy_dict(layers, c, g, allowed), sched, None, gradient=False)
    assert "gradient" not in bare and "group_objective" not in bare
    for key in ("advantage", "value_target", "log_prob", "return", "days", "value_loss", "entropy", "surrogate"):
        assert torch.equal(out[key], bare[key]), key
    A.close()


@pytest.mark.parametrize("net,act,mode", [("h7x13", "tanh", "collect"), ("h40", "relu", "epoch")])
def test_a_zero_coefficient_leaves_its_output_row_exactly_zero(dev, tabs, net, act, mode):
    """Tests 3 and 4: with vf_coef = 0 the value row's dW and db are exactly 0; with all-zero advantages and
    entropy_coef = 0 the logit row's are (an epoch; the other row is not zero either time)."""
    c = dict(AC.DEFAULT, net=net, act=act, mode=mode, n_steps=30)
    tb, ct, n, sched, _ = _setup(dev, tabs, c)
    A = _make(dev, tabs, c, n)
    g = QC.groups(n)
    p = AC.policy_dict(AC.net(ct, c, AC.G), c, g)
    inputs = _t(AC.epoch_inputs(30, n), dev)
    out = _call(A, c, p, sched, None, inputs if mode == "epoch" else None, vf_coef=0.0)
    dW, db = (x[HAVE] for x in out["gradient"]["layers"][-1])
    assert bool((dW[:, 1] == 0).all()) and bool((db[:, 1] == 0).all())
    assert bool((dW[:, 0] != 0).any()) and bool((db[:, 0] != 0).all())
    zero_adv = (torch.zeros_like(inputs[0]), inputs[1], inputs[2])
    out = _call(A, c, p, sched, None, zero_adv, entropy_coef=0.0)
    dW, db = (x[HAVE] for x in out["gradient"]["layers"][-1])
    assert bool((dW[:, 0] == 0).all()) and bool((db[:, 0] == 0).all())
    assert bool((dW[:, 1] != 0).any()) and bool((db[:, 1] != 0).all())
    assert bool((out["surrogate"] == 0).all())
    A.close()


def test_chunks_with_bootstrap_give_the_whole_calls_advantages(dev, tabs):
    """Test 5, as tests/test_gae_gpu.py checks for its kernels: with gae_lambda = 0 (A_s = delta_s, nothing crosses a chunk
    boundary but the bootstrap value) a call over n_steps = 40 with bootstrap=True, the 40 days stepped, then the rest,
    gives the whole call's "advantage", "value_target" and "log_prob" rows: each within the restatement's bound of a
    whole run of the twin, and chunk against whole within twice that bound. Without the bootstrap the chunk's last row
    leaves it."""
    c = dict(AC.DEFAULT, net="h24x20", act="tanh", gamma=0.95, lam=0.0)
    tb, ct, n, sched, _ = _setup(dev, tabs, c)
    A, B, T_ = _make(dev, tabs, c, n), _make(dev, tabs, c, n), _make(dev, tabs, c, n)
    g, layers = QC.groups(n), AC.net(ct, c, AC.G)
    p = AC.policy_dict(layers, c, g)
    np_ = lambda o: {key: o[key].double().cpu().numpy() for key in ("advantage", "value_target", "log_prob")}  # noqa: E731
    whole = np_(_call(A, c, p, sched, None, gradient=False))
    k = 40
    first = np_(_call(B, c, p, sched, None, n_steps=k, bootstrap=True, gradient=False))
    cut = np_(_call(B, c, p, sched, None, n_steps=k, gradient=False))
    rows = torch.arange(n, device=dev)
    for _ in range(k):
        st = B.state()
        B.step((sched[rows, st["t"].long().clamp(max=ct.T - 1)] & ~st["finished"].bool()).to(torch.int32))
    rest = np_(_call(B, c, p, sched, None, gradient=False))
    R = _twin_rows(T_, c, sched, None, ct.T)
    ref = AC.restate(c, R, None, layers, g, AC.G)
    for key, name, bname in (("advantage", "advantage", "adv_bound"), ("value_target", "value_target", "vt_bound"),
                             ("log_prob", "lp", "lp_bound")):
        bd = ref[bname]
        assert (np.abs(whole[key] - ref[name]) <= bd).all(), key
        assert (np.abs(first[key] - ref[name][:k]) <= bd[:k]).all() and (np.abs(first[key] - whole[key][:k]) <= 2 * bd[:k]).all(), key
        assert (np.abs(rest[key][:ct.T - k] - ref[name][k:]) <= bd[k:]).all(), key
        assert (np.abs(rest[key][:ct.T - k] - whole[key][k:]) <= 2 * bd[k:]).all() and (whole[key][k:] != 0).any(), key
    bd = ref["adv_bound"]
    assert (np.abs(cut["advantage"][:k - 1] - whole["advantage"][:k - 1]) <= 2 * bd[:k - 1]).all()
    assert (np.abs(cut["advantage"][k - 1] - whole["advantage"][k - 1]) > 2 * bd[k - 1]).any()
    for e_ in (A, B, T_):
        e_.close()


@pytest.mark.parametrize("name", ["h24x20_tanh_epoch_at_budget", "h24_tanh_collect_gated", "h40_relu_collect_ragged"])
def test_collect_then_epoch_with_its_own_outputs(dev, tabs, name):
    """Test 7: an epoch fed the collect call's "advantage", "value_target" and "log_prob" reproduces the collect call's
    gradient within the bound -- the collect reference's gradient, with the bound of an epoch whose inputs are known to
    the collect outputs' own bounds -- and reports clipped_days == 0. approx_kl is 0 up to what the f32 rounding of the
    stored log-probability leaves: rho_s = exp(lp_s - f32(lp_s)) with |lp_s - f32(lp_s)| <= 2^-24 |lp_s| = d, and
    (rho - 1) - log rho <= d^2, formed in fp64 where exp(d) near 1 carries an absolute rounding of 2^-52 (2^-51 per day
    with the subtraction), summed over the scored days and rounded to f32 once: 2^-48 of sum_s lp_s^2, sixteen
    binary orders below what f32 resolves of an lp -- exactly 0 is not attainable from an f32 array of old
    log-probabilities."""
    c = dict(AC.case(name), mode="collect")
    tb, ct, n, sched, allowed = _setup(dev, tabs, c)
    A, B = _make(dev, tabs, c, n), _make(dev, tabs, c, n)
    g, w = QC.groups(n), QC.weights(n)
    layers = AC.net(ct, c, AC.G)
    p = AC.policy_dict(layers, c, g, allowed)
    S = AC.steps(ct, c)
    col = _call(A, c, p, sched, w)
    ep = _call(A, c, p, sched, w, (col["advantage"], col["value_target"], col["log_prob"]))
    assert bool((ep["clipped_days"] == 0).all()) and torch.equal(ep["days"], col["days"])
    R = _twin_rows(B, c, sched, allowed, S)
    rc = AC.restate(c, R, w, layers, g, AC.G)
    d = 2.0 ** -24 * (np.abs(rc["lp"]) + rc["lp_bound"])  # the kernel's own lp_s is within lp_bound of the restated one
    kl_bound = ((d * d + 2.0 ** -51) * rc["m"]).sum(axis=0) * (1 + 2.0 ** -23)
    assert (np.abs(ep["approx_kl"].double().cpu().numpy()) <= kl_bound).all()
    re_ = AC.restate(dict(c, mode="epoch"), R, w, layers, g, AC.G,
                     (rc["advantage"], rc["value_target"], np.where(rc["m"], rc["lp"], -1.0)),
                     adv_err=rc["adv_bound"], target_err=rc["vt_bound"], old_err=rc["lp_bound"])
    worst = 0.0
    for (dW, db), (cW, cb), (rW, rb), (bW, bb) in zip(ep["gradient"]["layers"], col["gradient"]["layers"], rc["layers"],
                                                       re_["bound"]):
        for got, other, want, bound in ((dW, cW, rW, bW), (db, cb, rb, bb)):
            have = ~np.isnan(want)
            diff = np.abs(got.double().cpu().numpy() - want)[have]
            worst = max(worst, _ratio(diff, bound[have]))
            assert (diff <= bound[have]).all(), (name, worst)
            assert bool((got[HAVE] != 0).any()) and bool(torch.isnan(got[2]).all()) and got.shape == other.shape
    for x, y in zip(re_["layers"], rc["layers"]):  # the two references agree: rho = 1 and T - V = A
        have = ~np.isnan(y[0])
        assert np.abs(x[0] - y[0])[have].max() <= 1e-9 * np.abs(y[0][have]).max()
    print(f"{name}: epoch on its own collect outputs, ratio to the bound {worst:.3e}")
    A.close()
    B.close()


def test_workspace_guard_words_are_intact(dev, tabs):
    """Test 8, through the C entry point: a workspace one byte under w2a_actor_critic_mlp_workspace_bytes is refused and
    nothing is written; with exactly that size the guard words behind it stay as they were, in both modes."""
    c = dict(AC.DEFAULT, net="h24x20", act="tanh", n_steps=5)
    tb, ct, n, sched, _ = _setup(dev, tabs, c)
    env = _make(dev, tabs, c, n)
    pol = policy.check_actor_critic_net(AC.policy_dict(AC.net(ct, c, AC.G), c, QC.groups(n)), ct.n_obs, n, ct.obs_slot, dev)
    lib = env._lib
    wsb = lib.w2a_actor_critic_mlp_workspace_bytes(n, 5, pol.n_groups, pol.width, pol.n_layers)
    buf = torch.full((wsb + 65536,), 0xA5, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    grad = torch.full((pol.n_groups, policy.mlp_heads_stride(pol.width, pol.n_layers)), 7.0, dtype=torch.float32, device=dev)
    f = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device=dev)  # noqa: E731
    i = lambda: torch.full((n,), 7, dtype=torch.int32, device=dev)  # noqa: E731
    sur, vl, kl, ent, ret, cl, days = f(n), f(n), f(n), f(n), f(n), i(), i()
    adv, vt, lp = f(5, n), f(5, n), f(5, n)
    mask = policy.pack_alert_days(sched, (ct.T + 31) // 32)
    mp = _ffi.MlpPolicy()
    mp.params, mp.group, mp.order = pol.params.data_ptr(), pol.group.data_ptr(), pol.order.data_ptr()
    mp.n_groups, mp.n_layers, mp.width = pol.n_groups, pol.n_layers, pol.width
    mp.activation, mp.sample, mp.require_budget, mp.seed = _ffi.MLP_ACTIVATIONS["tanh"], 0, 0, 0

    def run(nbytes, epoch):
        ins = (adv.data_ptr(), 5, vt.data_ptr(), 5, lp.data_ptr(), 5) if epoch else (None, 0, None, 0, None, 0)
        outs = (None,) * 4 if epoch else (ret.data_ptr(), adv.data_ptr(), vt.data_ptr(), lp.data_ptr())
        with torch.cuda.device(dev):
            rc = lib.w2a_actor_critic_mlp(env._h, C.byref(mp), mask.data_ptr(), mask.shape[1], None, *ins, 0.2, 0.5, 0.01,
                                          1.0, 1.0, 0, 5, env._obs.data_ptr(), grad.data_ptr(), sur.data_ptr(),
                                          vl.data_ptr(), cl.data_ptr(), kl.data_ptr(), ent.data_ptr(), days.data_ptr(),
                                          *outs, buf.data_ptr(), nbytes, env._stream(), None, 0)
            torch.cuda.synchronize()
        return rc

    assert run(wsb - 1, False) == -1 and b"workspace smaller than w2a_actor_critic_mlp_workspace_bytes" in lib.w2a_last_error()
    assert bool((buf == 0xA5).all()) and bool((grad == 7.0).all()) and bool((adv == 7.0).all()) and bool((days == 7).all())
    assert run(wsb, False) == 0, lib.w2a_last_error()
    assert bool((buf[wsb:] == 0xA5).all()) and not bool((buf[:wsb] == 0xA5).all())
    have = torch.as_tensor(HAVE, device=dev)
    assert bool(torch.isfinite(grad[have]).all()) and bool(torch.isnan(grad[2]).all()) and bool((days != 7).all())
    lp.clamp_(max=0.0)
    assert run(wsb, True) == 0, lib.w2a_last_error()
    assert bool((buf[wsb:] == 0xA5).all()) and bool(torch.isfinite(grad[have]).all())
    assert env.check_status() == 0
    env.close()
