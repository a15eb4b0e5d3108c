"""q_gradient() (k_qg_pass1 / k_qg_pass2 and the count, scan and reduce kernels of w2a_policy_gradient_mlp) against the fp64
restatement (tests/q_restatement.py). The reference never touches the kernels under test: an identical twin from the
same seed is stepped day by day through step() with the schedule's actions and the rows, rewards and budgets it returns
go to the restatement. Every comparison requires |got - ref| <= bound for every component of the gradient, of "loss",
"return", "group_loss", "td_error" and "td_target", equal "days", NaN exactly for the empty group, ambiguity shares under
AMBIGUOUS_CAP and a case that is not trivial, and prints the largest ratio to the bound. The cases are those of
tests/q_gradient_cases.py (tests/test_q_gradient_cpu.py replays them with the NumPy oracle): 300 envs (four full waves and
a partial one), groups 0, 1 and 3 of 4 with group 2 empty, and the six instantiations again at 3 tiles per wave. Which
<WIDTH, LAYERS> pair a net runs is the host's padding rule (24, 40 pads to <64, 2>; 24, 20 is the <32, 2> net):
test_q_gradient_cpu.py::test_gpu_cases_reach_every_instantiation_under_both_activations holds the coverage."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q_gradient_cases as QC  # noqa: E402
from q_restatement import AMBIGUOUS_CAP, q_fp64  # noqa: E402

from weather2alert_amd import _ffi, policy  # noqa: E402

pytestmark = pytest.mark.gpu

ORDER = dict(lockstep=False, rollout_order=True)  # the handle's visiting order: not the identity
GID0 = QC.E.GID0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tabs():
    return QC.make_tables()


def _make(dev, tabs, c, n, gid0=GID0):
    """a fresh env of the case's table, reset, and walked through the days before the call"""
    from weather2alert_amd import HeatAlertVecEnv

    cfg = QC.RESET[c["table"]]
    env = HeatAlertVecEnv(n, tables=tabs[c["table"]].ct, device=dev, autoreset="disabled", env_gid0=gid0,
                          similar_climate_counties=True, **(ORDER if c["order"] else {}))
    env.reset(seed=cfg["seed"], options=dict(cfg["opts"]))
    for day in range(c["prefix"]):
        env.step(torch.as_tensor(QC.prefix_actions(n, day, gid0), device=dev))
    env.check_status()  # on the ragged table the prefix steps envs past their last day: read, and so cleared, here
    return env


def _twin_rows(env, sched, S):
    """`env` stepped through step() along `sched` (attempts by day of the episode) for at most S days from where it
    stands, every env read on its own days only: what tests/q_restatement.py takes."""
    n, dv = env.num_envs, env.device
    rows = torch.arange(n, device=dv)
    fin = env.state()["finished"].bool()
    R = dict(obs=torch.zeros((S + 1, n, env._obs.shape[1]), dtype=torch.float64, device=dv),
             reward=torch.zeros((S, n), dtype=torch.float64, device=dv),
             left_after=torch.zeros((S, n), dtype=torch.int64, device=dv),
             **{k: torch.zeros((S, n), dtype=torch.bool, device=dv) for k in ("valid", "issued", "terminal")})
    for s in range(S):
        st = env.state()
        R["obs"][s] = env._obs.double()
        R["valid"][s] = ~fin
        act = sched[rows, st["t"].long().clamp(max=sched.shape[1] - 1)] & ~fin
        res = env.step(act.to(torch.int32))
        after = env.state()
        R["issued"][s] = (after["used"] > st["used"]) & ~fin
        R["reward"][s] = torch.where(~fin, res[1].double(), torch.zeros_like(R["reward"][s]))
        R["terminal"][s] = res[2].bool() & ~fin
        R["left_after"][s] = (after["budget"] - after["used"]).long()
        fin = fin | res[2].bool()
    R["obs"][S] = env._obs.double()
    return {k: v.cpu().numpy() for k, v in R.items()}


def _ratio(diff, bound):
    return float(np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff > 0, np.inf, 0.0)).max())


def _call(env, c, q, tg, sched, w, **extra):
    kw = dict(target_net=tg, gamma=c["gamma"], double=c["double"], loss=c["loss"], huber_delta=c["huber_delta"],
              env_weight=w, n_steps=c["n_steps"], bootstrap=c["bootstrap"], td_error=True, td_target=True)
    kw.update(extra)
    return env.q_gradient(q, sched, **kw)


def _restate(c, R, w, layers, target, g, n_groups):
    return q_fp64(R["obs"], R["issued"], R["valid"], R["terminal"], R["reward"], R["left_after"], w, layers, target,
                  c["act"], g, n_groups, gamma=c["gamma"], double=c["double"], loss=c["loss"],
                  huber_delta=c["huber_delta"], bootstrap=c["bootstrap"], require_budget=c["rb"])


def _check(out, ref, c, R, what, groups=None, envs=slice(None)):
    """every component within its bound (groups: the rows of the gradient to compare with the reference's; envs: the
    slice of the per-env outputs the reference covers); returns the largest ratio to the bound"""
    assert ref["near_tie"] + ref["near_kink"] <= AMBIGUOUS_CAP, (what, ref["near_tie"], ref["near_kink"])
    worst = {"gradient": 0.0}
    for (dW, db), (rW, rb), (bW, bb) in zip(out["q_gradient"]["layers"], ref["layers"], ref["bound"]):
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
    assert out["loss"].dtype == torch.float32 and out["days"].dtype == torch.int32 and out["return"].dtype == torch.float32
    np.testing.assert_array_equal(out["days"].cpu().numpy()[envs], ref["days"], err_msg=str(what))
    for key, name in (("loss", "loss"), ("return", "ret")):
        diff = np.abs(out[key].double().cpu().numpy()[envs] - ref[name])
        worst[key] = _ratio(diff, ref[name + "_bound"])
        assert (diff <= ref[name + "_bound"]).all(), (what, key, worst)
    S = ref["td_error"].shape[0]
    for key in ("td_error", "td_target"):
        got = out[key].double().cpu().numpy()[:, envs]
        assert out[key].dtype == torch.float32 and got.shape[1] == ref[key].shape[1] and got.shape[0] >= S
        assert (got[:S][~R["valid"]] == 0).all() and (got[S:] == 0).all(), (what, key)  # zero where the env does not step
        diff = np.abs(got[:S] - ref[key])
        worst[key] = _ratio(diff, ref[key + "_bound"])
        assert (diff <= ref[key + "_bound"]).all(), (what, key, worst)
    if groups is None:
        gl = out["group_loss"].double().cpu().numpy()
        have = ~np.isnan(ref["group_loss"])
        assert gl.shape == have.shape and np.isnan(gl[~have]).all() and np.isfinite(gl[have]).all(), what
        diff = np.abs(gl - ref["group_loss"])[have]
        worst["group_loss"] = _ratio(diff, ref["group_loss_bound"][have])
        assert (diff <= ref["group_loss_bound"][have]).all(), (what, "group_loss", worst)
    # a case that scores nothing, clamps nothing or everything, or never masks proves little
    d = np.abs(ref["td_error"])[R["valid"]]
    assert d.size and (d > 0).any() and R["issued"].any() and (R["valid"] & ~R["issued"]).any(), what
    if c["loss"] == "huber":
        assert (d > c["huber_delta"]).any() and (d < c["huber_delta"]).any(), what
    if c["rb"]:
        assert ref["masked"].any() and (ref["has_next"] & ~ref["masked"]).any(), what  # some next-row max was masked
    print(f"{what}: ratio to the bound " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items())
          + f"; near_tie {ref['near_tie']:.2e}, near_kink {ref['near_kink']:.2e}, scored days {int(ref['days'].sum())}, "
          f"masked next rows {int(ref['masked'].sum())}")
    return max(worst.values())


def _dict(layers, act, g=None, rb=False):
    q = dict(kind="mlp", layers=layers, activation=act, require_budget=rb)
    if g is not None:
        q["group"] = g
    return q


@pytest.mark.parametrize("name", list(QC.CASES))
def test_against_stepped_twin(dev, tabs, name):
    """The six instantiations (seven two-row nets with padded widths), each under tanh and ReLU, at 1 tile per wave: a distinct
    target net and none, double on and off, squared and Huber loss, gamma 1.0, 0.99 and 0.9, n_steps 1 and 3 with and
    without bootstrap, a 9-day prefix and none, the ragged table with envs finished on entry, a sampled-at-budget schedule
    with require_budget (masked next rows), weights with zeros and negatives and none, the identity visiting order and
    the handle's own, four groups with one empty and one group with group=None."""
    c = QC.case(name)
    tb = tabs[c["table"]]
    ct, n = tb.ct, c["n"]
    A, B = _make(dev, tabs, c, n), _make(dev, tabs, c, n)
    g = QC.groups(n) if c["grouped"] else None
    layers, target = QC.nets(ct, c, QC.G if c["grouped"] else 1)
    sched = torch.as_tensor(QC.schedule(tb, c["table"], c, n), device=dev)
    w = QC.weights(n) if c["weights"] else None
    S = ct.T if c["n_steps"] is None else c["n_steps"]
    before = {k: v.clone() for k, v in A.state().items()}
    obs0 = A._obs.clone()
    q, tg = _dict(layers, c["act"], g, c["rb"]), (None if target is None else _dict(target, c["act"], g))
    out = _call(A, c, q, tg, sched, w)
    again = _call(A, c, q, tg, sched, w)
    assert A.check_status() == 0 and torch.equal(obs0, A._obs)
    for k, v in A.state().items():
        assert torch.equal(v, before[k]), k
    for key in ("loss", "days", "return", "group_loss", "td_error", "td_target"):  # identical calls, identical bits
        assert torch.equal(out[key].nan_to_num(7.0), again[key].nan_to_num(7.0)), key
    for (dW, db), (dW2, db2) in zip(out["q_gradient"]["layers"], again["q_gradient"]["layers"]):
        assert torch.equal(dW.nan_to_num(7.0), dW2.nan_to_num(7.0)) and torch.equal(db.nan_to_num(7.0), db2.nan_to_num(7.0))
    assert [(tuple(a.shape), tuple(b.shape)) for a, b in out["q_gradient"]["layers"]] == \
        [((QC.G if c["grouped"] else 1,) + W.shape[1:], (QC.G if c["grouped"] else 1,) + b.shape[1:]) for W, b in layers]
    assert tuple(out["td_error"].shape) == (S, n)
    R = _twin_rows(B, sched, S)
    ref = _restate(c, R, w, layers, target, g, QC.G if c["grouped"] else None)
    _check(out, ref, c, R, f"<{QC.INSTANTIATION[c['net']][0]}, {QC.INSTANTIATION[c['net']][1]}> {name}")
    if c["table"] == "ragged":  # envs finished on entry: their loss and days are 0
        fin = ~R["valid"][0]
        assert fin.any() and (~fin).any()
        assert (out["loss"].cpu().numpy()[fin] == 0).all() and (out["days"].cpu().numpy()[fin] == 0).all()
        assert (out["td_error"].cpu().numpy()[:, fin] == 0).all()
    if c["sched"] == "sampled":
        st = B.state()
        assert bool((st["used"] >= st["budget"]).any())  # envs at the budget
    A.close()
    B.close()


@pytest.mark.parametrize("name", list(QC.LARGE))
def test_three_tiles_per_wave(dev, tabs, name):
    """131 272 envs on the 12-day table: 2 052 tiles, 3 per wave of the second pass, groups of 1 000 consecutive env ids
    (every group boundary inside a tile, most inside a wave's second or third tile), the last group with 272 envs. The six
    instantiations, <32, 2> under both activations. Finite everywhere; three groups rebuilt as small
    batches with the same global env ids and stepped through step() lie inside the bound."""
    c = QC.case(name)
    tb = tabs[c["table"]]
    ct, n = tb.ct, c["n"]
    n_groups = (n + QC.GROUP_SIZE - 1) // QC.GROUP_SIZE
    n_tiles = (n + 63) // 64
    assert (n_tiles + 1023) // 1024 == 3  # tiles per wave of pass 2 (csrc/w2a_policy_dispatch.hip.h: pgm_layout)
    g = np.arange(n) // QC.GROUP_SIZE
    online, target = QC.nets(ct, c, 1)
    online, target = QC.scaled(online, n_groups, 10), (None if target is None else QC.scaled(target, n_groups, 11))
    w = QC.weights(n)
    A = _make(dev, tabs, c, n)
    sched = torch.as_tensor(QC.host_schedule(c["sched"], n, ct.T), device=dev)
    q, tg = _dict(online, c["act"], g, c["rb"]), (None if target is None else _dict(target, c["act"], g))
    out = _call(A, c, q, tg, sched, w)
    assert A.check_status() == 0
    assert all(bool(torch.isfinite(dW).all()) and bool(torch.isfinite(db).all()) for dW, db in out["q_gradient"]["layers"])
    A.close()
    for k in QC.CHECKED:
        lo = k * QC.GROUP_SIZE
        nk = min(QC.GROUP_SIZE, n - lo)
        B = _make(dev, tabs, c, nk, GID0 + lo)
        sk = torch.as_tensor(QC.host_schedule(c["sched"], nk, ct.T, GID0 + lo), device=dev)
        assert torch.equal(sk, sched[lo:lo + nk])
        R = _twin_rows(B, sk, ct.T)
        B.close()
        pick = lambda L: None if L is None else [(W[k:k + 1], b[k:k + 1]) for W, b in L]  # noqa: E731
        ref = _restate(c, R, w[lo:lo + nk], pick(online), pick(target), None, None)
        _check(out, ref, c, R, f"3 tiles per wave <{QC.INSTANTIATION[c['net']][0]}, {QC.INSTANTIATION[c['net']][1]}> {name}, "
               f"group {k} ({nk} envs)", groups=slice(k, k + 1), envs=slice(lo, lo + nk))


@pytest.mark.parametrize("net,act", [("h7", "relu"), ("h64x64", "tanh")])
def test_head_identity(dev, tabs, net, act):
    """A net whose two output rows are equal has max_a' Qt = Qt(., a*) whatever a* is: "td_target" is bit-equal with
    double on and off (each head is its own chain, in mlp_logit's order), and so is everything else."""
    c = dict(QC.DEFAULT, net=net, act=act, n_steps=40)
    ct, n = tabs["synth"].ct, c["n"]
    A = _make(dev, tabs, c, n)
    g = QC.groups(n)
    layers, target = QC.nets(ct, c, QC.G)
    same = lambda L: L[:-1] + [(np.repeat(L[-1][0][:, :1], 2, axis=1), np.repeat(L[-1][1][:, :1], 2, axis=1))]  # noqa: E731
    q, tg = _dict(same(layers), act, g), _dict(same(target), act, g)
    sched = torch.as_tensor(QC.host_schedule("random", n, ct.T), device=dev)
    off, on = _call(A, c, q, tg, sched, None, double=False), _call(A, c, q, tg, sched, None, double=True)
    assert bool((off["td_target"] != 0).any())
    for key in ("td_target", "td_error", "loss"):
        assert torch.equal(off[key], on[key]), key
    for (dW, db), (dW2, db2) in zip(off["q_gradient"]["layers"], on["q_gradient"]["layers"]):
        assert torch.equal(dW.nan_to_num(7.0), dW2.nan_to_num(7.0)) and torch.equal(db.nan_to_num(7.0), db2.nan_to_num(7.0))
    # the two rows see the same hidden layers: with a_s = 0 everywhere row 1 gets no gradient
    zero = _call(A, c, q, tg, torch.zeros_like(sched), None)
    have = torch.as_tensor(np.array([0, 1, 3]))
    dWo, dbo = zero["q_gradient"]["layers"][-1]
    assert bool((dWo[have][:, 1] == 0).all()) and bool((dbo[have][:, 1] == 0).all()) and bool((dWo[have][:, 0] != 0).any())
    A.close()


def test_workspace_one_byte_short_is_refused_and_nothing_is_written(dev, tabs):
    """through the C entry point: a workspace one byte under w2a_q_gradient_mlp_workspace_bytes returns W2A_ERR_ARG and
    leaves workspace, guard region and outputs as they were; the exact size is accepted and the guard stays untouched"""
    c = dict(QC.DEFAULT, net="h24x20", act="tanh", n_steps=5)
    ct, n = tabs["synth"].ct, c["n"]
    env = _make(dev, tabs, c, n)
    g = QC.groups(n)
    pol, tparams = policy.check_q_net(_dict(QC.nets(ct, c, QC.G)[0], "tanh", g), _dict(QC.nets(ct, c, QC.G)[1], "tanh", g),
                                      ct.n_obs, n, ct.obs_slot, dev)
    lib = env._lib
    wsb = lib.w2a_q_gradient_mlp_workspace_bytes(n, 5, pol.n_groups, pol.width, pol.n_layers)
    stride = policy.mlp_heads_stride(pol.width, pol.n_layers)
    buf = torch.full((wsb + 65536,), 0xA5, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    grad = torch.full((pol.n_groups, stride), 7.0, dtype=torch.float32, device=dev)
    loss, ret = (torch.full((n,), 7.0, dtype=torch.float32, device=dev) for _ in range(2))
    days = torch.full((n,), 7, dtype=torch.int32, device=dev)
    mask = policy.pack_alert_days(torch.as_tensor(QC.host_schedule("random", n, ct.T), device=dev), (ct.T + 31) // 32)
    mp, tp = _ffi.MlpPolicy(), _ffi.MlpPolicy()
    for s_, params in ((mp, pol.params), (tp, tparams)):
        s_.params, s_.group, s_.order = params.data_ptr(), pol.group.data_ptr(), pol.order.data_ptr()
        s_.n_groups, s_.n_layers, s_.width = pol.n_groups, pol.n_layers, pol.width
        s_.activation, s_.sample, s_.require_budget, s_.seed = _ffi.MLP_ACTIVATIONS["tanh"], 0, 0, 0

    def run(nbytes):
        with torch.cuda.device(dev):
            rc = lib.w2a_q_gradient_mlp(env._h, C.byref(mp), C.byref(tp), mask.data_ptr(), mask.shape[1], None, 5,
                                        env._obs.data_ptr(), grad.data_ptr(), loss.data_ptr(), days.data_ptr(),
                                        ret.data_ptr(), 0.99, 1, 1, 1.0, 0, None, None, buf.data_ptr(), nbytes, env._stream())
            torch.cuda.synchronize()
        return rc

    assert run(wsb - 1) == -1 and b"workspace smaller than w2a_q_gradient_mlp_workspace_bytes" in lib.w2a_last_error()
    assert bool((buf == 0xA5).all()) and bool((grad == 7.0).all()) and bool((loss == 7.0).all()) and bool((days == 7).all())
    assert run(wsb) == 0, lib.w2a_last_error()
    assert bool((buf[wsb:] == 0xA5).all()) and not bool((buf[:wsb] == 0xA5).all())
    have = torch.as_tensor(np.array([0, 1, 3]), device=dev)
    assert bool(torch.isfinite(grad[have]).all()) and bool(torch.isnan(grad[2]).all()) and bool((days != 7).all())
    assert env.check_status() == 0
    env.close()


def test_refusals_on_the_device(dev, tabs):
    """A stale observation buffer (after load_state_dict) is a RuntimeError, as value_gradient()'s; bad arguments are
    ValueErrors before anything runs: the state is untouched."""
    c = dict(QC.DEFAULT, net="h7", act="tanh")
    ct, n = tabs["synth"].ct, 65
    env = _make(dev, tabs, c, n)
    layers = QC.nets(ct, c, 1)[0]
    q = _dict(layers, "tanh")
    sched = torch.as_tensor(QC.host_schedule("random", n, ct.T), device=dev)
    before = {k: v.clone() for k, v in env.state().items()}
    one_row = _dict(layers[:-1] + [(layers[-1][0][:, :1], layers[-1][1][:, :1])], "tanh")
    for bad, kw in ((one_row, {}), (dict(q, sample=True), {}), (dict(q, allowed_days=np.ones((n, ct.T), bool)), {}),
                    (q, dict(gamma=2.0)), (q, dict(loss="l1")), (q, dict(target_net=one_row)), (q, dict(n_steps=0))):
        with pytest.raises(ValueError):
            env.q_gradient(bad, sched, **kw)
    for k, v in env.state().items():
        assert torch.equal(v, before[k]), k
    env.q_gradient(q, sched, n_steps=3)
    env.load_state_dict(env.state_dict())
    with pytest.raises(RuntimeError, match="observation buffer"):
        env.q_gradient(q, sched)
    env.close()
