"""actor_critic_gradient() (k_ac_pass1 / k_ac_finish / k_ac_pass2 and the host's packing by obs_slot) on observation
layouts other than the generator's own (tests/obs_layouts.py: columns on slots that are not their index, empty slots,
n_obs of 29, 28, 8 and 5, run-time slots in reverse order, two ragged variants) and on the slot-27 tables of
tests/table_edges.py, where a collect call pays rewards with a coefficient on the agent's own 14-day alert count. The
cases are those of tests/actor_critic_layout_cases.py. The reference never touches the kernels under test: an identical
twin is stepped day by day through step() along the schedule (tests/test_obs_layouts_gpu.py holds step() on these layouts
to the oracle, tests/test_table_edges_gpu.py and tests/test_env_gpu.py its slot-27 rewards to fp64) and its rows,
rewards and flags go to the fp64 restatement (tests/actor_critic_restatement.py). Every bound is the restatement's own,
checked by the helpers of tests/test_actor_critic_gpu.py; every ambiguity share stays under the restatement's cap
(tests/test_actor_critic_layouts_cpu.py holds that without a GPU). 193 envs on the layouts (three full waves and a
partial one), 300 on the slot-27 tables, groups 0, 1 and 3 of 4 with group 2 empty, weights with zeros and negative
values, every table on the identity visiting order and on the handle's own."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import actor_critic_layout_cases as K  # noqa: E402
import q_gradient_cases as QC  # noqa: E402
import test_actor_critic_gpu as TA  # noqa: E402  (the checks of the kernel's own test file: the existing bounds)

pytestmark = pytest.mark.gpu

WORST = {}
HAVE = [0, 1, 3]  # the groups that hold envs


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tabs():
    return K.make_tables()


def _worst(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))
    print(f"    worst ratio to the bound so far, {key}: {WORST[key]:.3e}")


def _env(tb, dev, c, **kw):
    """a fresh env of the case's table, reset, and walked through the days before the call"""
    from weather2alert_amd import HeatAlertVecEnv

    cfg = K.reset_cfg(tb.name)
    env = HeatAlertVecEnv(c["n"], tables=tb.ct, device=dev, autoreset="disabled", env_gid0=K.GID0,
                          similar_climate_counties=True, **(K.ORDER if c["order"] else {}), **kw)
    env.reset(seed=cfg["seed"], options=dict(cfg["opts"]))
    for day in range(c["prefix"]):
        env.step(torch.as_tensor(QC.prefix_actions(c["n"], day), device=dev))
    env.check_status()  # on the ragged tables the prefix steps envs past their last day: read, and so cleared, here
    assert not c["order"] or env.rollout_order
    return env


def _setup(dev, tabs, c):
    tb = tabs[c["table"]]
    sched = torch.as_tensor(K.schedule(tb, c), device=dev)
    gate = K.gate(tb, c)
    return tb, sched, None if gate is None else torch.as_tensor(gate, device=dev)


def _call(A, tb, c, layers, sched, allowed, **extra):
    return TA._call(A, c, K.policy_dict(layers, c, K.groups(c), allowed), sched, K.weights(c), TA._t(K.inputs(tb, c), A.device),
                    **extra)


def _snapshot(A):
    return {k: v.clone() for k, v in A.state().items()}, A._obs.clone()


def _untouched(A, snap):
    before, obs0 = snap
    assert A.check_status() == 0 and torch.equal(obs0, A._obs)
    for k, v in A.state().items():
        assert torch.equal(v, before[k]), k


# ------------------------------------------------------------------ 1 and 5: the stepped twin, identical bits, no side effects
@pytest.mark.parametrize("cid", list(K.CASES))
def test_against_stepped_twin(dev, tabs, cid):
    """Every table in both modes, the six instantiations under tanh and ReLU, from reset on the ragged tables (the 1-, 2-
    and 3-day episodes walked from their first day) and after a prefix (envs finished on entry), gated and at-budget
    cases, 7-day chunks with the bootstrap: every gradient component, the per-env outputs, the rows, "days",
    "clipped_days" and "group_objective" inside the restatement's bounds of the twin stepped through step(), NaN exactly
    for the empty group. On slot27 / ragged27 the twin's own rewards are the reference: step() carries the slot-27 term.
    The first layer's dW comes back [G, h, n_obs] in the layout's own column order. Two identical calls give identical
    bits; the state, the observation buffer and the status word are untouched."""
    c = K.CASES[cid]
    tb, sched, allowed = _setup(dev, tabs, c)
    ct, n = tb.ct, c["n"]
    A, B = _env(tb, dev, c), _env(tb, dev, c)
    layers = K.net(ct, c, K.G)
    snap = _snapshot(A)
    out, again = _call(A, tb, c, layers, sched, allowed), _call(A, tb, c, layers, sched, allowed)
    _untouched(A, snap)
    assert set(out) == set(again) and ("return" in out) == ("advantage" in out) == (c["mode"] == "collect")
    TA._same_bits(out, again, [k for k in out if k != "gradient"])
    assert [(tuple(a.shape), tuple(b.shape)) for a, b in out["gradient"]["layers"]] == \
        [((K.G,) + W.shape[1:], (K.G,) + b.shape[1:]) for W, b in layers]
    assert out["gradient"]["layers"][0][0].shape[2] == ct.n_obs
    S = K.steps(ct, c)
    R = TA._twin_rows(B, c, sched, allowed, S)
    ref = K.reference(tb, c, R, layers=layers)
    inst = K.AC.INSTANTIATION[c["net"]]
    r = TA._check(out, ref, c, R, f"<{inst[0]}, {inst[1]}> {cid}")
    _worst(("slot-27 tables" if tb.slot27 else "layouts") + f", {c['mode']}", r)
    fin = ~R["valid"][0]
    if c["prefix"] and tb.ragged:  # envs finished on entry: nothing is scored, nothing is lost
        assert fin.any() and (~fin).any()
        assert (out["value_loss"].cpu().numpy()[fin] == 0).all() and (out["days"].cpu().numpy()[fin] == 0).all()
    if c["prefix"] == 0:
        assert not fin.any()
    if tb.ragged and c["prefix"] == 0:  # the shortest episodes, from their first day
        nd = K.tuples(tb, n)["n_days"]
        for d in (1, 2, 3):
            assert (R["valid"].sum(axis=0)[nd == d] == d).all()
        assert (nd <= 3).any() and (R["valid"].sum(axis=0)[nd == ct.T] == S).all() and (nd == ct.T).any()
        np.testing.assert_array_equal(out["days"].cpu().numpy()[nd <= 3], ref["days"][nd <= 3])
    if tb.slot27:  # scored days of envs with a slot-27 coefficient and alerts in their 14-day window
        a2w = tb.a2w[A.state()["coef_col"].cpu().numpy()]
        count14 = R["obs"][:S][:, :, ct.feature_names.index("alert_2wks")]
        assert a2w.any() and (ref["m"] & (count14 > 0))[:, a2w].any(), cid
    if c["bootstrap"]:
        alive = R["valid"][S - 1] & ~R["terminal"][S - 1]
        assert alive.any() and (~alive & R["valid"][0]).any()  # a bootstrap row, and ends inside the chunk
    A.close()
    B.close()


# ------------------------------------------------------------------ 2: the one-head kernels' bits
@pytest.mark.parametrize("table,net,act,kw", [
    ("permuted", "h24x20", "tanh", dict(gamma=0.9, lam=0.8, n_steps=20, bootstrap=True, rb=True)),
    ("narrow", "h7", "relu", dict(gamma=0.97, lam=0.9)),
    ("slot27", "h40", "tanh", dict(gamma=1.0, lam=1.0, order=True))])
def test_collect_outputs_are_the_one_head_kernels_bits(dev, tabs, table, net, act, kw):
    """As tests/test_actor_critic_gpu.py (tests 2 and 9 of the feature's list) on permuted, narrow and slot27:
    "advantage", "value_target" and "return" equal value_gradient() of the one-head net (trunk + row 1) with the same
    gamma, gae_lambda and bootstrap bit for bit; "log_prob" and "days" equal surrogate_gradient(log_prob=True) of the
    one-head net (trunk + row 0). tests/test_obs_layouts_learners_gpu.py holds both one-head kernels to their own
    restatements on these layouts."""
    c = K._case(net, act, "collect", table, "bits", **kw)
    assert table in K.BITS_TABLES
    tb, sched, _ = _setup(dev, tabs, c)
    ct = tb.ct
    A = _env(tb, dev, c)
    g = K.groups(c)
    layers = K.net(ct, c, K.G)
    out = TA._call(A, c, K.policy_dict(layers, c, g), sched, None)
    crit = A.value_gradient(TA._one_head(layers, 1, dict(c, rb=False), g), sched, n_steps=c["n_steps"], advantage=True,
                            value_target=True, gamma=c["gamma"], gae_lambda=c["lam"], bootstrap=c["bootstrap"])
    assert torch.equal(out["advantage"], crit["advantage"]) and torch.equal(out["value_target"], crit["value_target"])
    assert torch.equal(out["return"], crit["return"]) and bool((out["advantage"] != 0).any())
    actor = A.surrogate_gradient(TA._one_head(layers, 0, c, g), sched, torch.zeros_like(out["advantage"]),
                                 n_steps=c["n_steps"], log_prob=True)
    assert torch.equal(out["log_prob"], actor["log_prob"]) and bool((out["log_prob"] != 0).any())
    assert torch.equal(out["days"], actor["days"]) and bool((out["days"] > 0).any())
    if c["rb"]:  # forced days: stepped and valued, not scored
        assert bool(((out["log_prob"] == 0) & (out["value_target"] != 0)).any())
    assert A.check_status() == 0
    A.close()


# ------------------------------------------------------------------ 3: one column alone
@pytest.mark.parametrize("name", K.ONE_COLUMN)
def test_one_column_alone(dev, tabs, name):
    """A first layer that is zero except on one observation column (obs_layout_learner_cases.one_column: a table column
    off its index; `remaining_budget`, slot 26, on narrow), scaled by column_scale so that the column moves the hidden
    units: a kernel or a host that reads or returns another slot for that column has no random matrix to hide behind.
    Every component inside the bounds of the stepped twin's restatement; the first-layer dW of THAT column within its
    bound and outside its bound of zero; exactly zero in every column whose input is 0 on every stepped day (permuted
    has two; the gradient with respect to a weight is sum coefficient_s x_js whatever the weight is, so the other columns
    are not zero); and shifting that column's weights changes the per-env outputs, again inside the bounds."""
    tb = tabs[name]
    ct = tb.ct
    c = K.CASES[K.ONE_COLUMN_CASES[name]]
    col = K.one_column(ct)
    _, sched, allowed = _setup(dev, tabs, c)
    A, B = _env(tb, dev, c), _env(tb, dev, c)
    S = K.steps(ct, c)
    R = TA._twin_rows(B, c, sched, allowed, S)
    zero = K.zero_columns(R)
    assert col not in zero and (name != "permuted" or len(zero) >= 1)
    outs = []
    for shift in (0.0, K.ONE_COLUMN_SHIFT):
        layers = K.one_column_net(ct, c, col, shift)
        out = _call(A, tb, c, layers, sched, allowed)
        ref = K.reference(tb, c, R, layers=layers)
        what = f"{name}: column {ct.feature_names[col]} (slot {ct.obs_slot[col]}) alone, shift {shift}"
        _worst("one column alone", TA._check(out, ref, c, R, what))
        dW = out["gradient"]["layers"][0][0].double().cpu().numpy()[HAVE]
        rW, bW = ref["layers"][0][0][HAVE], ref["bound"][0][0][HAVE]
        diff = np.abs(dW - rW)[:, :, col]
        print(f"    {what}: dW of the column at {TA._ratio(diff, bW[:, :, col]):.3e} of its bound")
        assert (diff <= bW[:, :, col]).all() and (np.abs(dW[:, :, col]) > bW[:, :, col]).any(), what
        assert (dW[:, :, zero] == 0).all(), (what, zero)
        others = [j for j in range(ct.n_obs) if j != col and j not in zero]
        assert (np.abs(dW[:, :, others]) > bW[:, :, others]).any(), what
        outs.append(out)
    a, b = outs
    assert not torch.equal(a["value_loss"], b["value_loss"]) and not torch.equal(a["entropy"], b["entropy"])
    assert not torch.equal(a["gradient"]["layers"][0][0][HAVE], b["gradient"]["layers"][0][0][HAVE])
    assert A.check_status() == 0
    A.close()
    B.close()


# ------------------------------------------------------------------ 4: a posterior-mean env
def test_posterior_mean_env_runs_an_epoch_and_refuses_to_collect(dev, tabs):
    """No other test runs actor_critic_gradient() on a reward_mode="posterior_mean" env on a device
    (tests/test_actor_critic_cpu.py holds the refusal on a bare object): on permuted, from the same seed and prefix, an
    epoch forms no reward and gives the sampled env's bits; a collect call raises ValueError and touches nothing."""
    c = dict(K.CASES["h24_relu_epoch_permuted"], order=False)  # the visiting order is a sampled env's option
    tb, sched, allowed = _setup(dev, tabs, c)
    A, P = _env(tb, dev, c), _env(tb, dev, c, reward_mode="posterior_mean", pm_kernel="vector")
    assert P.reward_mode == "posterior_mean" and torch.equal(A._obs, P._obs)
    for k, v in A.state().items():  # the prefix paid the two envs different rewards and left them the same episodes
        assert v.is_floating_point() or torch.equal(v, P.state()[k]), k
    layers = K.net(tb.ct, c, K.G)
    snap = _snapshot(P)
    out, pm = _call(A, tb, c, layers, sched, allowed), _call(P, tb, c, layers, sched, allowed)
    assert set(out) == set(pm) and "return" not in pm
    TA._same_bits(out, pm, [k for k in out if k != "gradient"])
    assert bool((pm["days"] > 0).any()) and bool((pm["clipped_days"] > 0).any())
    assert all(bool(torch.isfinite(x[HAVE]).all()) and bool((x[HAVE] != 0).any()) for wb in pm["gradient"]["layers"] for x in wb)
    with pytest.raises(ValueError, match="reward_mode='sampled'"):
        P.actor_critic_gradient(K.policy_dict(layers, c, K.groups(c)), sched, env_weight=K.weights(c))
    _untouched(P, snap)
    A.close()
    P.close()
