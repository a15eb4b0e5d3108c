"""actor_critic_gradient() without a GPU: the new names are declared, bound and listed; the C entry point refuses a NULL
handle under its own name and sizes its workspace as w2a.h documents; every Python refusal comes before the library is
touched; the fp64 restatement the GPU tests hold the kernels to (tests/actor_critic_restatement.py) is the gradient of
J_g by torch autograd in both modes, gated and not, under tanh and ReLU, and tells wrong estimators apart; every case of
the GPU file, replayed by the NumPy oracle, keeps its ambiguity shares under the cap and is not trivial; and the cases
reach all six <WIDTH, LAYERS> instantiations under both activations."""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import actor_critic_cases as AC  # noqa: E402
import q_gradient_cases as QC  # noqa: E402
from actor_critic_restatement import AMBIGUOUS_CAP, ac_fp64, objective_torch  # noqa: E402

from weather2alert_amd import _ffi, build, policy  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["w2a_actor_critic_mlp", "w2a_actor_critic_mlp_workspace_bytes"]
P = 4096  # a non-NULL, 256-B aligned address that is never read


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.load()


@pytest.fixture(scope="module")
def tabs():
    return AC.make_tables()


# ---- symbols and the C entry point without a handle ---------------------------------------------------------------------
def test_abi_header_and_ffi_agree_on_the_new_names(lib):
    header = open(os.path.join(ROOT, "include", "w2a.h")).read()
    assert set(re.findall(r"\b(w2a_actor_critic_\w+)\s*\(", header)) == set(NEW)
    assert set(NEW) == {s for s in _ffi.SYMBOLS if s.startswith("w2a_actor_critic_")}
    for s in NEW:
        proto = re.search(r"\b" + s + r"\s*\(([^;]*)\);", header).group(1)
        assert len(proto.split(",")) == len(getattr(lib, s).argtypes), s
    assert lib.w2a_abi_version() == _ffi.ABI_VERSION == 18  # the change is additive


def _entry(lib, env=None, **bad):
    mp = _ffi.MlpPolicy(params=P, group=None, order=None, n_groups=1, n_layers=2, width=64, activation=0, sample=0,
                        require_budget=0, seed=0)
    a = dict(net=C.byref(mp), alert_mask=P, mask_words=0, env_weight=None, advantage=None, advantage_days=0,
             value_target=None, value_target_days=0, old_log_prob=None, old_log_prob_days=0, clip=0.2, vf_coef=0.5,
             entropy_coef=0.0, gamma=1.0, lam=1.0, bootstrap=0, n_steps=3, obs=P, grad=P, surrogate=P, value_loss=P,
             clipped_days=P, approx_kl=P, entropy=P, days=P, ret=P, advantage_out=P, value_target_out=P, log_prob_out=P,
             workspace=P, workspace_bytes=1 << 20, stream=None, allowed_days=None, allowed_words=0)
    assert len(a) + 1 == len(lib.w2a_actor_critic_mlp.argtypes)
    a.update(bad)
    rc = lib.w2a_actor_critic_mlp(env, *a.values())
    return rc, lib.w2a_last_error().decode()


def test_a_null_handle_is_refused_first_under_the_entry_points_own_name(lib):
    """W2A_ERR_ARG and "w2a_actor_critic_mlp: NULL handle", whatever else is wrong with the call"""
    name = "w2a_actor_critic_mlp"
    assert _entry(lib) == (-1, f"{name}: NULL handle")
    for bad in (dict(net=None), dict(n_steps=0), dict(alert_mask=None), dict(workspace=None), dict(clip=-1.0),
                dict(advantage=P), dict(grad=None), dict(allowed_days=P, allowed_words=0)):
        assert _entry(lib, **bad) == (-1, f"{name}: NULL handle"), bad


def test_workspace_size_is_the_documented_layout(lib):
    """w2a.h: the layout of w2a_q_gradient_mlp followed by one f32 column [n_steps][num_envs], rounded up to 256 B"""
    size, base = lib.w2a_actor_critic_mlp_workspace_bytes, lib.w2a_q_gradient_mlp_workspace_bytes
    a256 = lambda v: (v + 255) // 256 * 256  # noqa: E731
    for shape in ((100, 10, 1, 16, 1), (70_000, 153, 5, 64, 2), (1, 1, 3, 32, 2), (300, 153, 4, 64, 1), (300, 7, 4, 32, 1)):
        assert size(*shape) == base(*shape) + a256(4 * shape[0] * shape[1]), shape
    for shape in ((0, 10, 1, 16, 1), (100, 0, 1, 16, 1), (100, 10, 0, 16, 1), (100, 10, 1, 48, 1), (100, 10, 1, 16, 3)):
        assert size(*shape) == 0


# ---- refusals before the library is touched -----------------------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the arguments were refused")


def _bare_env(ct, n=6, reward_mode="sampled", fixes=()):
    """an env object no device ever saw (tests/test_lookahead_cpu.py::_bare_env), with a library that must not be read"""
    from weather2alert_amd import HeatAlertVecEnv

    env = object.__new__(HeatAlertVecEnv)
    env.ct, env.num_envs, env.device, env.fixes, env.reward_mode = ct, n, torch.device("cpu"), set(fixes), reward_mode
    env._needs_reset, env._pm, env._obs_current, env._lib, env._h = True, False, True, _NoLibrary(), None
    return env


def _net(rng, hidden, G_, n_obs, rows=2):
    dims = [n_obs] + list(hidden) + [rows]
    return [((rng.standard_normal((G_, dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32),
             (rng.standard_normal((G_, dims[i + 1])) * 0.5).astype(np.float32)) for i in range(len(dims) - 1)]


def test_every_python_refusal_comes_before_the_library(tabs):
    ct = tabs["short"].ct
    env = _bare_env(ct)
    n, T, rng = env.num_envs, ct.T, np.random.default_rng(1)
    net = dict(kind="mlp", layers=_net(rng, (7, 13), 1, ct.n_obs), activation="tanh")
    sched = np.zeros((n, T), bool)
    day = lambda v=0.0: np.full((T, n), v, np.float32)  # noqa: E731
    three = dict(advantage=day(), value_target=day(), old_log_prob=day(-0.5))
    with pytest.raises(RuntimeError, match="reset"):  # every argument is fine: the call gets as far as the state
        env.actor_critic_gradient(net, sched, gamma=0.9, gae_lambda=0.9, bootstrap=True, n_steps=3,
                                  env_weight=np.ones(n, np.float32))
    with pytest.raises(RuntimeError, match="reset"):
        env.actor_critic_gradient(dict(net, allowed_days=np.ones((n, T), bool), require_budget=True), sched, **three)
    with pytest.raises(RuntimeError, match="reset"):
        env.actor_critic_gradient(net, sched, gradient=False)
    W = np.zeros((1, ct.n_obs), np.float32)
    look = dict(net, layers=_net(rng, (5,), 1, ct.n_obs + 3), lookahead={"feature": "heat_qi", "days": 3})
    with pytest.raises(ValueError, match=r"actor_critic_gradient\(\).*lookahead"):
        env.actor_critic_gradient(look, sched)
    with pytest.raises(ValueError, match="kind 'mlp'"):
        env.actor_critic_gradient(dict(kind="linear", weight=W, bias=np.zeros(1, np.float32)), sched)
    with pytest.raises(ValueError, match="exactly 2 rows"):
        env.actor_critic_gradient(dict(net, layers=_net(rng, (7, 13), 1, ct.n_obs, rows=1)), sched)
    for bad in (None, dict(net, activation="gelu"), dict(net, layers=_net(rng, (7, 80), 1, ct.n_obs))):
        with pytest.raises(ValueError):
            env.actor_critic_gradient(bad, sched)
    # one or two of the three epoch arrays
    for keys in (("advantage",), ("value_target",), ("old_log_prob",), ("advantage", "value_target"),
                 ("advantage", "old_log_prob"), ("value_target", "old_log_prob")):
        with pytest.raises(ValueError, match="come together"):
            env.actor_critic_gradient(net, sched, **{k: three[k] for k in keys})
    # surrogate_gradient()'s and value_gradient()'s argument checks
    for kw in (dict(clip=-0.1), dict(clip=float("nan")), dict(clip=True), dict(entropy_coef=float("inf")),
               dict(vf_coef=-1.0), dict(vf_coef=float("nan")), dict(gamma=1.5), dict(gamma=True), dict(gae_lambda=-0.1),
               dict(gae_lambda=float("nan")), dict(bootstrap=1), dict(gradient=1), dict(n_steps=0), dict(n_steps=2.5),
               dict(env_weight=np.ones(n + 1, np.float32)), dict(env_weight=np.full(n, np.nan, np.float32)),
               dict(env_weight=np.ones(n, np.int64)),
               dict(three, advantage=day()[:, :-1]), dict(three, value_target=day()[:2], n_steps=3),
               dict(three, old_log_prob=day(0.5)), dict(three, advantage=day(np.nan)),
               dict(three, value_target=np.zeros((T, n), np.int64)),
               dict(three, gamma=0.9), dict(three, gae_lambda=0.9), dict(three, bootstrap=True), dict(three, gradient=False)):
        with pytest.raises(ValueError):
            env.actor_critic_gradient(net, sched, **kw)
    for bad_sched in (None, sched[:, :-1], sched.astype(np.int32), sched[:-1]):
        with pytest.raises(ValueError):
            env.actor_critic_gradient(net, bad_sched)
    with pytest.raises(ValueError):
        env.actor_critic_gradient(dict(net, allowed_days=np.ones((n, T - 1), bool)), sched)
    # collecting needs rewards: refused for posterior_mean as value_gradient() does; an epoch forms none and is taken
    pm = _bare_env(ct, reward_mode="posterior_mean")
    with pytest.raises(ValueError, match="reward_mode='sampled'"):
        pm.actor_critic_gradient(net, sched)
    with pytest.raises(RuntimeError, match="reset"):
        pm.actor_critic_gradient(net, sched, **three)
    with pytest.raises(ValueError):
        _bare_env(ct, fixes=("lag",)).actor_critic_gradient(net, sched)


# ---- the restatement against autograd -----------------------------------------------------------------------------------
def _toy(seed, n=12, S=10, n_obs=20):
    """12 envs, 10 days: random rows, rewards and labels; envs that end early, one finished on entry, forced days"""
    rng = np.random.default_rng(seed)
    days = rng.integers(3, S + 3, n)  # > S: still running when the call ends
    days[0] = 0
    valid = np.arange(S)[:, None] < days[None, :]
    terminal = valid & (np.arange(S)[:, None] == (days - 1)[None, :])
    return dict(obs=rng.standard_normal((S + 1, n, n_obs)).astype(np.float32).astype(np.float64), valid=valid,
                terminal=terminal, labels=(rng.random((S, n)) < 0.4) & valid, forced=(rng.random((S, n)) < 0.25) & valid,
                reward=rng.standard_normal((S, n)) * 0.7, g=np.array([0, 1, 3])[np.arange(n) % 3], w=rng.standard_normal(n),
                A=rng.standard_normal((S, n)), T=rng.standard_normal((S, n)), old=-0.05 - 1.5 * rng.random((S, n)) ** 2)


def _autograd(T, layers, act, m, A, Tg, old, clip, vf, beta, G_=4):
    P = [(torch.tensor(np.asarray(W, np.float64), requires_grad=True), torch.tensor(np.asarray(b, np.float64), requires_grad=True))
         for W, b in layers]
    J = objective_torch(T["obs"], T["labels"], T["valid"], m, T["w"], P, act, T["g"], G_, A, Tg, old, clip, vf, beta)
    sum(j for j in J if j is not None).backward()
    return [(W.grad.numpy(), b.grad.numpy()) for W, b in P]


@pytest.mark.parametrize("hidden,act", [((7,), "tanh"), ((24, 20), "relu"), ((24, 40), "relu"), ((64, 64), "tanh")])
@pytest.mark.parametrize("gated", [False, True])
def test_restatement_is_the_gradient_of_the_objective_by_autograd(hidden, act, gated):
    """12 envs, 10 days, to 1e-10 relative: collect (GAE with and without the bootstrap; A and T detached, rho = 1) and
    epoch (given advantages, targets and old log-probabilities, days on both sides of the clip edges), with and without
    forced days, tanh and ReLU"""
    rng = np.random.default_rng(5)
    T = _toy(3)
    layers = _net(rng, hidden, 4, 20)
    forced = T["forced"] if gated else np.zeros_like(T["forced"])
    args = (T["obs"], T["labels"], T["valid"], forced, T["terminal"], T["reward"], T["w"], layers, act, T["g"], 4)
    seen_clipped = False
    for kw in (dict(gamma=0.9, lam=0.8, bootstrap=True, beta=0.02), dict(gamma=1.0, lam=1.0, bootstrap=False, beta=0.0),
               dict(advantage=T["A"], value_target=T["T"], old_log_prob=T["old"], beta=0.02, clip=0.2),
               dict(advantage=T["A"], value_target=T["T"], old_log_prob=T["old"], beta=0.0, clip=0.0, vf_coef=1.3)):
        ref = ac_fp64(*args, **kw)
        epoch = "advantage" in kw
        A, Tg = (T["A"], T["T"]) if epoch else (ref["advantage"], ref["value_target"])
        want = _autograd(T, layers, act, ref["m"], A, Tg, T["old"] if epoch else None, kw.get("clip", 0.2),
                         kw.get("vf_coef", 0.5), kw["beta"])
        scale = max(np.abs(x).max() for wb in want for x in wb)
        assert scale > 0
        for (dW, db), (aW, ab) in zip(ref["layers"], want):
            have = ~np.isnan(dW).reshape(dW.shape[0], -1).all(axis=1)
            assert list(have) == [True, True, False, True]  # group 2 is empty
            assert np.abs(dW[have] - aW[have]).max() <= 1e-10 * scale and np.abs(db[have] - ab[have]).max() <= 1e-10 * scale, kw
        assert ref["days"][0] == 0 and ref["vl"][0] == 0 and (ref["days"] == (T["valid"] & ~forced).sum(axis=0)).all()
        if epoch:
            seen_clipped |= bool(ref["clipped"].any()) and bool((ref["m"] & ref["live"] & (ref["rho"] != 1)).any())
        else:
            assert (ref["clipped"] == 0).all() and np.abs(ref["kl"]).max() == 0
            np.testing.assert_allclose(ref["vl"], 0.5 * (ref["advantage"] ** 2).sum(axis=0), rtol=1e-12)
    assert seen_clipped


def _outside(got, ref):
    return any((np.abs(x - r)[~np.isnan(r)] > bd[~np.isnan(r)]).any() for wb, rb, bb in zip(got, ref["layers"], ref["bound"])
               for x, r, bd in zip(wb, rb, bb))


def test_the_restatement_tells_a_wrong_estimator_apart():
    """the value term dropped on forced days, the factor 1/2 lost, the two rows swapped, gamma off by 0.01, the forced
    days scored: each leaves the bound of the right one"""
    rng = np.random.default_rng(6)
    T = _toy(4)
    layers = _net(rng, (24, 40), 4, 20)
    args = (T["obs"], T["labels"], T["valid"], T["forced"], T["terminal"], T["reward"], T["w"], layers, "tanh", T["g"], 4)
    kw = dict(gamma=0.9, lam=0.8, bootstrap=True, beta=0.02)
    ref = ac_fp64(*args, **kw)
    assert not _outside(ac_fp64(*args, **kw)["layers"], ref)
    unforced = args[:3] + (np.zeros_like(T["forced"]),) + args[4:]
    for what, other in (("value_on_scored_only", ac_fp64(*args, **kw, mutant="value_on_scored_only")),
                        ("no_half", ac_fp64(*args, **kw, mutant="no_half")),
                        ("swap_rows", ac_fp64(*args, **kw, mutant="swap_rows")),
                        ("gamma", ac_fp64(*args, **dict(kw, gamma=0.91))), ("forced days scored", ac_fp64(*unforced, **kw))):
        assert _outside(other["layers"], ref), what


# ---- the GPU file's cases, replayed by the oracle -----------------------------------------------------------------------
def _reference(tabs, name, n=None, gid0=AC.GID0, lo=0, layers=None):
    c = AC.case(name)
    tb = tabs[c["table"]]
    ct = tb.ct
    n_all = c["n"]
    n = n_all if n is None else n
    sched = AC.schedule(tb, c, n, gid0)
    allowed = AC.gate(n, ct.T, gid0) if c["gate"] else None
    R = AC.oracle_rows(tb, c, n, sched, allowed, gid0)
    grouped = c["grouped"] and layers is None
    g = QC.groups(n) if grouped else None
    if layers is None:
        layers = AC.net(ct, c, AC.G if grouped else 1)
    w = QC.weights(n_all)[lo:lo + n] if c["weights"] else None
    inputs = AC.epoch_inputs(AC.steps(ct, c), n_all, lo, n) if c["mode"] == "epoch" else None
    return c, R, AC.restate(c, R, w, layers, g, AC.G if grouped else None, inputs)


@pytest.mark.parametrize("name", list(AC.CASES))
def test_gpu_cases_stay_under_the_ambiguity_cap(tabs, name):
    """ambiguous_share (days inside the clip edge's error band) + near_kink + near_tie <= AMBIGUOUS_CAP from the
    restatement alone, and the case is not trivial: alerts and non-alerts are scored, epoch cases clip some days and not
    others, gated and at-budget cases force days that keep their value term"""
    c, R, ref = _reference(tabs, name)
    print(f"{name}: ambiguous {ref['ambiguous_share']:.2e}, near_kink {ref['near_kink']:.2e}, scored {int(ref['days'].sum())} "
          f"of {int(ref['stepped'].sum())} days, clipped {int(ref['clipped'].sum())}")
    assert ref["ambiguous_share"] + ref["near_kink"] + ref["near_tie"] <= AMBIGUOUS_CAP
    AC.not_trivial(c, R, ref, name)
    if c["table"] == "ragged":
        assert (~R["valid"][0]).any() and R["valid"][0].any()  # envs finished on entry (the 25-day prefix)


@pytest.mark.parametrize("name", list(AC.LARGE))
def test_large_gpu_cases_stay_under_the_ambiguity_cap(tabs, name):
    """the groups the 3-tiles-per-wave cases check, rebuilt as small batches with the same global env ids"""
    c = AC.case(name)
    ct = tabs[c["table"]].ct
    n_groups = (c["n"] + QC.GROUP_SIZE - 1) // QC.GROUP_SIZE
    big = QC.scaled(AC.net(ct, c, 1), n_groups, 10)
    for k in QC.CHECKED:
        lo = k * QC.GROUP_SIZE
        nk = min(QC.GROUP_SIZE, c["n"] - lo)
        _, R, ref = _reference(tabs, name, n=nk, gid0=AC.GID0 + lo, lo=lo, layers=[(W[k:k + 1], b[k:k + 1]) for W, b in big])
        assert ref["ambiguous_share"] + ref["near_kink"] <= AMBIGUOUS_CAP, (name, k)
        AC.not_trivial(c, R, ref, (name, k))


def test_gpu_cases_reach_every_instantiation_under_both_activations_and_modes():
    """by the host's own padding rule, not by the nets' names: the 1-tile cases run all six <WIDTH, LAYERS> pairs under
    tanh and under ReLU and each pair in both modes, every one of them with padded units; the 3-tile cases all six
    pairs; the tables include the mini table, a ragged one and the n_obs = 8 layout; gated cases exist in both modes"""
    pairs = {(w, nl) for w in policy.MLP_WIDTHS for nl in (1, 2)}
    inst = lambda c: (policy.mlp_width(QC.NETS[c["net"]][0]), len(QC.NETS[c["net"]][0]))  # noqa: E731
    cases = [AC.case(n) for n in AC.CASES]
    assert {(inst(c), c["act"]) for c in cases} == {(p, a) for p in pairs for a in ("tanh", "relu")}
    assert {(inst(c), c["mode"]) for c in cases} == {(p, m) for p in pairs for m in ("collect", "epoch")}
    padded = [c for c in cases if any(h != inst(c)[0] for h in QC.NETS[c["net"]][0])]
    assert {(inst(c), c["mode"]) for c in padded} == {(p, m) for p in pairs for m in ("collect", "epoch")}
    assert {inst(AC.case(n)) for n in AC.LARGE} == pairs and {AC.case(n)["mode"] for n in AC.LARGE} == {"collect", "epoch"}
    assert {"synth", "ragged", "n8"} <= {c["table"] for c in cases}
    assert {c["mode"] for c in cases if c["gate"]} == {"collect", "epoch"}
    assert all(inst(c) == AC.INSTANTIATION[c["net"]] for c in cases)
